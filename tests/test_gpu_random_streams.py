"""Every in-kernel random stream against its independent statement (oracle/philox.py; tests/test_philox_cpu.py holds the statement to
Random123's known-answer vectors and to its statistics).

Exact streams (dropout factors, batch draws, box units): integer arithmetic and exact float conversions, ``np.array_equal``.

Normals: the kernels run Box-Muller in float32 — part sampling through libm (logf, cospif / sinpif on the exact 2 u2), the chain
kernels through the hardware log2 / sin / cos — the statement in float64 on the same 24-bit uniforms.  |dz| = |kernel - statement| is judged
element by element: a keying error (a wrong counter word, a dropped high half, the wrong N in the global point id) moves an element by O(1),
so EVERY element must sit under the gate, and the gate is twice the worst |dz| measured on an MI355X, never above 1e-2:

    stream                                          worst |dz| measured     gate
    part normals (libm)                             5.16e-6                 1.04e-5      (logf's ulp at r = 5.7 and the float32 product r cos)
    chain noise (hardware transcendentals)          7.89e-5                 1.58e-4      (the float32 mu at t = 1, where sqrt(pv var) = 1e-3)

(MEASURED_LIBM / MEASURED_HW below; profiles/random_streams_parity.txt has the per-test table; the entry points that take one step at
t >= 2 sit at 3e-6 .. 1e-5).  The signed mean of dz over the draws of
each test is within 5 standard errors of zero.

The chain noise is observed through the chain itself.  The engine is built from synth.make_denoiser_weights with the output projection
(weight and bias) set to zero: eps = 0 in every precision and kernel variant, so a DDPM step is x' = mu(x) + sqrt(pv[t] var) z with mu affine
in x.  From two consecutive snapshots z_t = (x' - mu(x)) / sqrt(pv[t] var), with mu in float64 on the GPU's own float32 x and the float32
tables of oracle.diffusion (what the reference's extract_into_tensor reads) and the scale as the kernel rounds it; the t = T snapshot gives the
start draw, (x_T - anchor) / sqrt(var).  |dz| of the chain therefore includes the float32 rounding of mu, amplified by 1 / sqrt(pv var)
(largest at t = 1): part of MEASURED_HW.

Global point id: (shape_offset + b) N' + n with N' the point count of the LAUNCH — the engine pads N = 100 to 128 before the launch, so 128
enters the id (asserted: the statement with 128 matches, the one with 100 is off by O(1) from the second shape on).
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from difffacto_amd import synth  # noqa: E402
from oracle import diffusion as odf  # noqa: E402
from oracle import philox as ph  # noqa: E402
from _variants import NAMES, forced, ran  # noqa: E402

MEASURED_LIBM, MEASURED_HW = 5.2e-6, 7.9e-5
GATE_LIBM, GATE_HW = 2 * MEASURED_LIBM, 2 * MEASURED_HW
assert GATE_LIBM <= 1e-2 and GATE_HW <= 1e-2

F32, F64 = np.float32, np.float64
T, B = 10, 3
SEED_LO, SEED_HI = 0x1234ABCD, 0x1234ABCD + (5 << 32)          # differ in the high word only
OFFSETS = (0, 5, 1 << 40)
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _judge(name, got, want, gate):
    """Every element under the gate; the signed mean within 5 standard errors of zero.  Returns max |dz|."""
    dz = np.asarray(got, dtype=F64).reshape(-1) - np.asarray(want, dtype=F64).reshape(-1)
    worst, mean, se = float(np.abs(dz).max()), float(dz.mean()), float(dz.std() / math.sqrt(dz.size))
    print(f"RANDOM_STREAMS {name}: n={dz.size} max|dz|={worst:.3e} mean={mean:+.2e} ({mean / se if se > 0 else 0.0:+.2f} se)")
    assert worst <= gate, (name, worst, gate)
    assert abs(mean) <= 5 * se, (name, mean, se)
    return worst


# ================================================================================================ exact streams
@pytest.mark.parametrize("p", [0.2, 0.5, 1e-5, 0.99999, 2.0 ** -17], ids=["p0.2", "p0.5", "p1e-5", "p0.99999", "p2^-17"])
def test_dropout_factors_bit_exact(p):
    """dfx_debug_dropout_factors against the statement: n = 4 (half a group), 12 (a group and a half), 1020 / 1028 (both sides of a launch
    block's 1024 elements), 2^16 + 4.  The hook starts at element 0, so a group index at or above 2^32 (counter word 1 nonzero) cannot be
    reached through it: that word is covered by the statement's layout alone."""
    from difffacto_amd.training import dropout_factors
    for seed in (777, 1 << 32, (1 << 64) - 1, 0xDEADBEEF00000005):
        for site in (0, 1, 9, 1000):
            for n in (4, 12, 1020, 1028, (1 << 16) + 4):
                got = dropout_factors(seed, site, p, n).cpu().numpy()
                want = ph.dropout_factors(seed, site, p, n)
                assert got.dtype == want.dtype == F32 and np.array_equal(got, want), (seed, site, n, int((got != want).sum()))
    want = ph.dropout_factors(777, 0, p, (1 << 16) + 4)
    print(f"RANDOM_STREAMS dropout p={p:.6g}: threshold {ph.dropout_threshold(p)}, keep factor {want.max():.9g}, "
          f"dropped {int((want == 0).sum())} of {want.size}")
    assert want.max() > 0 and (want == 0).any()                       # both values occur: the comparison is not of constants


@pytest.mark.parametrize("N", [10, 11, 1025, 2048])
@pytest.mark.parametrize("C", [1, 5, 8])
def test_batch_draws_bit_exact(N, C):
    """dfx_batch_draw: items over a set of three clouds (1000, 0 and 4000 points): a plain item, sample_id 7, sample_id 2^40 + 3, the empty
    cloud (M = 0), an index past the set and a negative one (M = 0); seeds with and without a high word."""
    from difffacto_amd import _ffi
    offsets = np.array([0, 1000, 1000, 5000], dtype=np.int64)
    index = np.array([0, 2, 2, 1, 3, -1, 0], dtype=np.int64)
    sample_id = np.array([0, 7, (1 << 40) + 3, 7, (1 << 40) + 3, 0, (1 << 40) + 3], dtype=np.int64)
    nb = index.size
    d_offsets, d_index, d_id = cu(offsets), cu(index), cu(sample_id)
    for seed in (9, (0xABCD << 32) | 9, (1 << 64) - 1):
        choice = torch.full((nb, N), -1, dtype=torch.int32, device="cuda")
        drop_u = torch.full((nb, C), -1.0, device="cuda")
        aug_u = torch.full((nb, 6), -1.0, device="cuda")
        _ffi.check(_ffi.lib().dfx_batch_draw(_ffi.ptr(d_offsets), 3, _ffi.ptr(d_index), _ffi.ptr(d_id), nb, N, C, seed,
                                             _ffi.ptr(choice), _ffi.ptr(drop_u), _ffi.ptr(aug_u), _ffi.current_stream()), "dfx_batch_draw")
        w_choice, w_drop, w_aug = ph.batch_draw(offsets, index, sample_id, N, C, seed)
        assert np.array_equal(choice.cpu().numpy(), w_choice), seed
        assert np.array_equal(drop_u.cpu().numpy(), w_drop) and np.array_equal(aug_u.cpu().numpy(), w_aug), seed
        assert not w_choice[3:6].any() and w_choice[0].max() < 1000 and w_choice[1].max() < 4000
        assert N < 64 or (len(np.unique(w_choice[0])) > N // 4 and not np.array_equal(w_choice[1], w_choice[2]))


@pytest.mark.parametrize("C", [1, 4])
def test_box_units_bit_exact(C):
    """dfx_debug_part_box_units at pair0 = 0, 5, 2^33: words 0, 1, 2 of each counter, word 3 discarded (the triple (1, 2, 3) is another
    tensor: asserted, so the comparison tells the two apart)."""
    from difffacto_amd import _ffi
    P = 3
    for seed in (11, (0xFACE << 32) | 11):
        for pair0 in (0, 5, 1 << 33):
            units = torch.full((P, C, 2, ph.BOX_PTS, 3), -1.0, device="cuda")
            _ffi.check(_ffi.lib().dfx_debug_part_box_units(seed, pair0, P, C, _ffi.ptr(units), _ffi.current_stream()), "box_units")
            got = units.cpu().numpy()
            words = ph.box_words(seed, pair0, P, C)
            assert np.array_equal(got, ph.box_units(seed, pair0, P, C)) and np.array_equal(got, ph.unit24(words[..., :3])), (seed, pair0)
            assert not np.array_equal(got, ph.unit24(words[..., 1:])) and not np.array_equal(got[..., 2], ph.unit24(words[..., 3]))
    # pairs 5, 6, 7 of a launch from 0 are pairs 0, 1, 2 of a launch from 5
    a = torch.empty(8, C, 2, ph.BOX_PTS, 3, device="cuda")
    _ffi.check(_ffi.lib().dfx_debug_part_box_units(11, 0, 8, C, _ffi.ptr(a), _ffi.current_stream()), "box_units")
    assert np.array_equal(a[5:].cpu().numpy(), ph.box_units(11, 5, 3, C))


# ================================================================================================ part-sampling normals (libm)
@pytest.mark.parametrize("row0", [0, 1 << 33], ids=["row0", "row2^33"])
@pytest.mark.parametrize("J", [1, 4])
@pytest.mark.parametrize("n_draws", [4, 64])
def test_part_normals_against_float64_statement(n_draws, J, row0):
    from difffacto_amd.part_sampling import draw_normals
    rows = 3
    for seed in (3, (0xBEEF << 32) | 3):
        got = draw_normals(rows, J, seed, row0=row0, n_draws=n_draws).cpu().numpy()
        want = ph.part_normals(seed, row0, rows, J, n_draws)
        assert got.shape == want.shape == (rows, n_draws, 3, J)
        dz = np.abs(got.astype(F64) - want)
        print(f"RANDOM_STREAMS part normals seed={seed:#x} row0={row0} J={J} n_draws={n_draws}: max|dz|={dz.max():.3e}")
        assert dz.max() <= GATE_LIBM, (seed, float(dz.max()))


def test_part_normals_signed_mean():
    """One larger draw (3 rows x 512 draws x 3 axes x 8 parts) for the signed-mean condition and the measured worst |dz| of the libm stream."""
    from difffacto_amd.part_sampling import draw_normals
    got = draw_normals(3, 8, 20240521, row0=(1 << 33) - 1, n_draws=512).cpu().numpy()    # rows 2^33 - 1, 2^33, 2^33 + 1
    _judge("part normals (libm), 3 x 512 x 3 x 8", got, ph.part_normals(20240521, (1 << 33) - 1, 3, 8, 512), GATE_LIBM)


# ================================================================================================ chain noise (hardware transcendentals)
_ENGINES = {}


def _engine(prec):
    from difffacto_amd.engine import DenoiserEngine
    if prec not in _ENGINES:
        W = synth.make_denoiser_weights(seed=0)
        W["proj_out.weight"] = np.zeros_like(W["proj_out.weight"])
        W["proj_out.bias"] = np.zeros_like(W["proj_out.bias"])
        _ENGINES[prec] = DenoiserEngine({k: torch.from_numpy(v) for k, v in W.items()}, num_timesteps=T, precision=prec)
    return _ENGINES[prec]


_CASES = {}


def _case(N):
    """Latents with mixed valid parts, per-point anchors / variances in (B,N,3) layout, a clean cloud; computed once per N."""
    if N not in _CASES:
        part_code, mean, logvar, valid = synth.make_latents(B, seed=41, all_valid=True)
        valid[1] = [1, 0, 1, 1]
        valid[2] = [0, 0, 1, 0]
        var = np.exp(logvar).astype(F32)
        seg = synth.make_seg_mask(valid, N)
        assert seg.shape == (B, N)
        a, v = odf.gather_params(seg, mean, var)                                       # (B,3,N) float32
        rng = np.random.default_rng(N)
        x0 = (a + 0.5 * np.sqrt(v) * rng.standard_normal((B, 3, N))).astype(F32)
        _CASES[N] = dict(part_code=part_code, mean=mean, var=var, valid=valid, seg=seg, x0=x0,
                         a=np.ascontiguousarray(a.transpose(0, 2, 1)), v=np.ascontiguousarray(v.transpose(0, 2, 1)))
    return _CASES[N]


def _ctx(eng, c):
    return eng.prepare_shapes(*(torch.from_numpy(c[k]) for k in ("part_code", "mean", "var", "valid")))


TB = odf.Tables(T)


def _tab(name, t, tb=TB):
    return F64(tb.f32(name, t))


def _mu(x, a, t):
    """Posterior mean of a DDPM step with eps = 0, float64 arithmetic on float32 inputs: c1 x0 + c2 x + c3 a, x0 = sra (x - a) + a."""
    x, a = x.astype(F64), a.astype(F64)
    x0 = _tab("sqrt_recip_alphas_cumprod", t) * (x - a) + a
    return _tab("posterior_mean_coef1", t) * x0 + _tab("posterior_mean_coef2", t) * x + _tab("posterior_mean_coef3", t) * a


def _mu_ddim(x, a, t):
    """DDIM update with eps = 0: (x0 - a) sqrt(alphas_cumprod_prev[t]) + a."""
    x, a = x.astype(F64), a.astype(F64)
    x0 = _tab("sqrt_recip_alphas_cumprod", t) * (x - a) + a
    return (x0 - a) * F64(np.sqrt(TB.f32("alphas_cumprod_prev", t))) + a


def _scale(v, t):
    """sqrt(pv[t] var) as the kernel rounds it: float32 product, float32 square root (both correctly rounded)."""
    return np.sqrt(TB.f32("posterior_variance", t) * v).astype(F64)


@functools.lru_cache(maxsize=None)
def _stmt(seed, shape_offset, N, t, stream):
    """(B,N,3) statement normals of a launch of B shapes of N points (padded to whole wavefronts in the global point id)."""
    gid = ph.chain_gid(shape_offset, B, N)
    assert gid.shape == (B, -(-N // 32) * 32)
    return ph.chain_normals(seed, gid[:, :N], t, stream)


def _snap(t):
    return t.cpu().numpy()


VARIANTS = [("bf16", 8), ("bf16", 4), ("bf16", 2), ("bf16", 1), ("bf16", 16), ("bf16", 0), ("f32", 8), ("f32", 4), ("f32", 2), ("f32", 1), ("f32", 0)]
VIDS = [p + "-" + {0: "auto", 1: "coop" if p == "bf16" else "direct", 16: "coop2"}.get(n, "pipe%d" % n) for p, n in VARIANTS]


def _took(prec, nw, n_launch):
    """Assert the variant by name.  Code 16 (k_denoise_coop2) works on pairs of wavefronts: a launch of N % 64 != 0 takes k_denoise_coop."""
    if prec == "bf16" and nw == 16 and n_launch % 64:
        from difffacto_amd.engine import last_kernel_variant
        v = last_kernel_variant()
        assert v == NAMES["bf16"][1], v
        return v
    return ran(prec, nw)


@pytest.mark.parametrize("prec,nw", VARIANTS, ids=VIDS)
def test_chain_noise_every_step_every_variant(prec, nw):
    """T = 10, ret_interval = 1: the t = T snapshot is stream 1 keyed by T; snapshot t (t = 9 .. 1) from snapshot t + 1 is stream 0 keyed by
    t; pred (t = 0) adds no noise.  N = 96 (three wavefronts per shape) and N = 100 (padded to 128), shape_offset 0 / 5 / 2^40, two seeds
    that differ in the high word."""
    eng = _engine(prec)
    worst, names, dzs = 0.0, set(), []
    for N in (96, 100):
        c = _case(N)
        ctx, seg, a, v = _ctx(eng, c), cu(c["seg"]), c["a"], c["v"]
        n_launch = -(-N // 32) * 32
        assert n_launch == {96: 96, 100: 128}[N]
        for off in OFFSETS:
            for seed in (SEED_LO, SEED_HI):
                with forced(nw):
                    pred, traj = eng.sample_chain(ctx, seg, seed=seed, ret_interval=1, shape_offset=off)
                    names.add(_took(prec, nw, n_launch))
                traj, pred = _snap(traj), _snap(pred)
                assert traj.shape == (T, B, N, 3) and pred.shape == (B, N, 3)
                got = [(traj[0].astype(F64) - a) / np.sqrt(v).astype(F64)]
                want = [_stmt(seed, off, N, T, ph.STREAM_START)]
                for k in range(1, T):
                    t = T - k
                    got.append((traj[k].astype(F64) - _mu(traj[k - 1], a, t)) / _scale(v, t))
                    want.append(_stmt(seed, off, N, t, ph.STREAM_STEP))
                dz = np.abs(np.stack(got) - np.stack(want))
                assert dz.max() <= GATE_HW, (N, off, hex(seed), float(dz.max()), np.unravel_index(dz.argmax(), dz.shape))
                worst = max(worst, float(dz.max()))
                dzs.append((np.stack(got) - np.stack(want)).reshape(-1))
                if N == 100 and off == 0:   # which N enters the global point id: 128.  With 100 the second and third shape read other counters.
                    wrong = ph.chain_normals(seed, np.arange(B, dtype=np.uint64)[:, None] * np.uint64(100) + np.arange(N, dtype=np.uint64)[None, :],
                                             T, ph.STREAM_START)
                    dzw = np.abs(got[0] - wrong)
                    assert dzw[0].max() <= GATE_HW and dzw[1:].max() > 0.5
                e0 = np.abs(pred.astype(F64) - _mu(traj[T - 1], a, 0)).max()                 # t = 0: the mean itself, no noise
                assert e0 <= 4e-7 * (1 + np.abs(pred).max()), float(e0)
    dz = np.concatenate(dzs)
    print(f"RANDOM_STREAMS chain {prec} forced {nw} -> {sorted(names)}:")
    _judge(f"chain noise {prec}/{nw}", dz, np.zeros_like(dz), GATE_HW)


def test_chain_noise_differs_where_the_key_differs():
    """The two seeds (high word), the three shape offsets and the two streams give different clouds (the statement says so; this is the GPU)."""
    eng, c = _engine("bf16"), _case(96)
    ctx, seg = _ctx(eng, c), cu(c["seg"])
    runs = {(s, o): eng.sample_chain(ctx, seg, seed=s, ret_interval=1, shape_offset=o)[1] for s in (SEED_LO, SEED_HI) for o in OFFSETS}
    keys = list(runs)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            assert float(((runs[keys[i]] - runs[keys[j]]).abs() > 1e-3).float().mean()) > 0.9, (keys[i], keys[j])
    # shape 1 of a launch at offset 5 is shape 0 of a launch at offset 6: bit-equal start draws
    one = eng.sample_chain(ctx, seg, seed=SEED_LO, ret_interval=1, shape_offset=6)[1]
    a = torch.from_numpy(c["a"]).cuda()
    v = torch.from_numpy(c["v"]).cuda()
    z5 = (runs[(SEED_LO, 5)][0, 1] - a[1]) / v[1].sqrt()
    z6 = (one[0, 0] - a[0]) / v[0].sqrt()
    assert float((z5 - z6).abs().max()) < 1e-5


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_p_sample_and_p_sample_ddim_noise(prec):
    """One step at one t through the generator-protocol entry points: stream 0 keyed by t; N = 100 (padded), shape_offset 5."""
    eng, N, off = _engine(prec), 100, 5
    c = _case(N)
    ctx, seg, a, v = _ctx(eng, c), cu(c["seg"]), c["a"], c["v"]
    x = c["x0"]                                                                          # (B,3,N)
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))
    for t in (7, 1):
        out = _snap(eng.p_sample(ctx, cu(x), seg, t, seed=SEED_HI, shape_offset=off)).transpose(0, 2, 1)
        ran(prec)
        _judge(f"p_sample {prec} t={t}", (out.astype(F64) - _mu(xt, a, t)) / _scale(v, t), _stmt(SEED_HI, off, N, t, ph.STREAM_STEP), GATE_HW)
        out = _snap(eng.p_sample_ddim(ctx, cu(x), seg, t, 1.0, seed=SEED_HI, shape_offset=off)).transpose(0, 2, 1)
        ran(prec)
        _judge(f"p_sample_ddim {prec} t={t} eta=1", (out.astype(F64) - _mu_ddim(xt, a, t)) / _scale(v, t),
               _stmt(SEED_HI, off, N, t, ph.STREAM_STEP), GATE_HW)
    out0 = _snap(eng.p_sample(ctx, cu(x), seg, 0, seed=SEED_HI, shape_offset=off)).transpose(0, 2, 1)     # t = 0: no noise
    assert np.abs(out0.astype(F64) - _mu(xt, a, 0)).max() <= 4e-7 * (1 + np.abs(out0).max())


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_sample_chain_ddim_noise(prec):
    """DDIM chain over the steps [0, 3, 7], eta = 1: the start draw is stream 1 keyed by T, the steps stream 0 keyed by their own t."""
    eng, N, off, steps = _engine(prec), 100, 1 << 40, [0, 3, 7]
    c = _case(N)
    ctx, seg, a, v = _ctx(eng, c), cu(c["seg"]), c["a"], c["v"]
    pred, traj = eng.sample_chain_ddim(ctx, seg, steps, 1.0, seed=SEED_HI, ret_interval=1, shape_offset=off)
    ran(prec)
    traj = _snap(traj)
    slot = lambda t: traj[T - t]
    got = [(slot(T).astype(F64) - a) / np.sqrt(v).astype(F64), (slot(7).astype(F64) - _mu_ddim(slot(T), a, 7)) / _scale(v, 7),
           (slot(3).astype(F64) - _mu_ddim(slot(7), a, 3)) / _scale(v, 3)]
    want = [_stmt(SEED_HI, off, N, T, ph.STREAM_START), _stmt(SEED_HI, off, N, 7, ph.STREAM_STEP), _stmt(SEED_HI, off, N, 3, ph.STREAM_STEP)]
    _judge(f"sample_chain_ddim {prec} steps {steps} eta=1", np.stack(got), np.stack(want), GATE_HW)
    assert np.abs(_snap(pred).astype(F64) - _mu_ddim(slot(3), a, 0)).max() <= 4e-7 * (1 + np.abs(traj).max())


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_refine_chain_start_draw_and_steps(prec):
    """refine_chain, n_steps = 3: x_s = qa (x0 - a) + a + qb sqrt(var) z with z = stream 1 keyed by n_steps (not by T), then steps t = 2, 1, 0
    on stream 0.  (a) explicit zero step noise isolates the start draw: the t = 2 snapshot is mu_2(x_s), inverted in float64;
    (b) explicit zero start noise isolates the step draws; (c) both drawn: the t = 2 snapshot is the sum of the two terms, each within its
    gate, and the t = 1 snapshot follows from it."""
    eng, N, off, n = _engine(prec), 100, 5, 3
    c = _case(N)
    ctx, seg, a, v = _ctx(eng, c), cu(c["seg"]), c["a"], c["v"]
    x0 = cu(c["x0"])
    x0t = np.ascontiguousarray(c["x0"].transpose(0, 2, 1)).astype(F64)
    a64, L = a.astype(F64), np.sqrt(v).astype(F64)
    qa, qb = _tab("sqrt_alphas_cumprod", n - 1), _tab("sqrt_one_minus_alphas_cumprod", n - 1)
    k = _tab("posterior_mean_coef1", n - 1) * _tab("sqrt_recip_alphas_cumprod", n - 1) + _tab("posterior_mean_coef2", n - 1)   # d mu / d x
    z_start = _stmt(SEED_HI, off, N, n, ph.STREAM_START)
    z2, z1 = _stmt(SEED_HI, off, N, 2, ph.STREAM_STEP), _stmt(SEED_HI, off, N, 1, ph.STREAM_STEP)
    zeros_steps, zeros_start = torch.zeros(n, B, 3, N, device="cuda"), torch.zeros(B, 3, N, device="cuda")
    # (a)
    _, traj = eng.refine_chain(ctx, seg, x0, n, step_noise=zeros_steps, seed=SEED_HI, ret_interval=1, shape_offset=off)
    ran(prec)
    s2 = _snap(traj)[0].astype(F64)
    xs = a64 + (s2 - _mu(a, a, n - 1)) / k                       # mu is affine with mu(a) = (c1 + c2 + c3) a: x_s - a = (mu(x_s) - mu(a)) / k
    _judge(f"refine_chain {prec} start draw (stream 1, keyed by n_steps = {n})", (xs - qa * (x0t - a64) - a64) / (qb * L), z_start, GATE_HW)
    wrong = _stmt(SEED_HI, off, N, T, ph.STREAM_START)
    assert np.abs((xs - qa * (x0t - a64) - a64) / (qb * L) - wrong).max() > 0.5       # not keyed by T
    # (b)
    _, traj = eng.refine_chain(ctx, seg, x0, n, start_noise=zeros_start, seed=SEED_HI, ret_interval=1, shape_offset=off)
    ran(prec)
    tr = _snap(traj)
    assert tr.shape[0] == 2
    xs0 = (qa * (x0t - a64) + a64).astype(F32)
    got = [(tr[0].astype(F64) - _mu(xs0, a, 2)) / _scale(v, 2), (tr[1].astype(F64) - _mu(tr[0], a, 1)) / _scale(v, 1)]
    _judge(f"refine_chain {prec} step draws t = 2, 1", np.stack(got), np.stack([z2, z1]), GATE_HW)
    # (c)
    _, traj = eng.refine_chain(ctx, seg, x0, n, seed=SEED_HI, ret_interval=1, shape_offset=off)
    ran(prec)
    tr = _snap(traj)
    xs_want = qa * (x0t - a64) + a64 + qb * L * z_start
    resid = np.abs(tr[0].astype(F64) - (_mu(xs_want, a, 2) + _scale(v, 2) * z2))
    assert np.all(resid <= GATE_HW * (k * qb * L + _scale(v, 2))), float((resid / (k * qb * L + _scale(v, 2))).max())
    _judge(f"refine_chain {prec} both drawn, t = 1", (tr[1].astype(F64) - _mu(tr[0], a, 1)) / _scale(v, 1), z1, GATE_HW)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_sample_chain_from_noise_with_a_held_part(prec):
    """sample_chain_from, n_steps = 3, from a given state; shape 0 holds part 1: its points come back as given, every other point carries
    stream 0 of t = 2 and t = 1."""
    eng, N, off, n = _engine(prec), 100, 1 << 40, 3
    c = _case(N)
    ctx, seg, a, v = _ctx(eng, c), cu(c["seg"]), c["a"], c["v"]
    x = c["x0"]
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))
    hold = torch.tensor([1 << 1, 0, 0], dtype=torch.int32)
    pred, traj = eng.sample_chain_from(ctx, seg, cu(x), n, seed=SEED_LO, ret_interval=1, shape_offset=off, hold=hold)
    ran(prec)
    tr, pred = _snap(traj), _snap(pred)
    assert tr.shape[0] == 2
    held = np.zeros((B, N), dtype=bool)
    held[0] = c["seg"][0] == 1
    assert held.sum() == N // 4
    for s in (tr[0], tr[1], pred):
        assert np.array_equal(s[held], xt[held])
    free = ~held
    got = [((tr[0].astype(F64) - _mu(xt, a, 2)) / _scale(v, 2))[free], ((tr[1].astype(F64) - _mu(tr[0], a, 1)) / _scale(v, 1))[free]]
    want = [_stmt(SEED_LO, off, N, 2, ph.STREAM_STEP)[free], _stmt(SEED_LO, off, N, 1, ph.STREAM_STEP)[free]]
    _judge(f"sample_chain_from {prec} t = 2, 1 (one held part)", np.stack(got), np.stack(want), GATE_HW)
