"""The denoiser kernels against a float64 oracle and a rounding model (oracle/highprec.py), judged by rms and per-group statistics
(tests/_errstats.py) instead of a max-abs over the tensor against a number the kernel printed once.

Every case computes the float64 truth once and, on the same inputs in the same process, the two yardsticks: the fp32 numpy oracle's
error (what fp32 arithmetic costs) and the bf16 rounding model's error (what bf16 operands on the matrix pipe cost).  A kernel's error
is judged against its yardstick: every bound below is `factor x (yardstick computed here)`.  The factors (tests/_errstats.py: R32, RB,
RMAX, G) are the largest ratio measured on the MI355X over all cases of this file x 1.25, within the conditions that
tests/test_oracle_highprec_cpu.py enforces (each deliberately wrong variant of the rounding model must fail the same acceptance
function).  The kernel a case names is forced and the one that ran is asserted (tests/_variants.py).  One line per case and variant is
printed (`HIGHPREC ...`); profiles/highprec_parity.txt holds them.

Measured (MI355X, see profiles/highprec_parity.txt) and the thresholds that follow:

                 measured worst   x 1.25   threshold    where
  R32                6.69          8.36     8.0  (cap)   eps B3_N100 t=0, both fp32 kernels (bit-identical); rms 7.6e-7 in every case
  RB                 1.134         1.418    1.42         eps_t B4_N2048, shape 3 (t = 500) judged on its own, k_denoise_pipe<8>
  RMAX               1.223         1.529    1.53         eps B4_N2048 t=6, outlier gamma3 weights (fold moved to channel 109)
  G[lane]            1.170         1.463    1.25 (cap)   same case
  G[lane16]          1.087         1.359    1.25 (cap)   same case
  G[wave]            1.060         1.325    1.25 (cap)   same case
  G[tile]            1.090         1.363    1.37         eps B1_N8192 t=5
  G[shape]           1.312         1.640    1.64         eps B12_N2048 t=500
  G[coord]           1.320         1.650    1.65         eps B1_N8192 t=500, outlier gamma3 weights
  q_sample           2.04 ulps              4 ulps       of the element's largest term (bound from counting roundings, see the test)
  masked MSE         0.49 ulps              4 ulps       of the loss (same)
  wall time of this file: 82 s, CPU oracles included (354 lines); tests/test_gpu_benched_kernel.py took 29 s in the same run (its
  code is the parent commit's).  NOT MET: the file was to stay within that file's time.  Where the 82 s go: eps B12_N2048 about 25 s,
  the plain-pack / moved-fold cases over the t list about 19 s, the T = 100 chains 14 s, eps B4_N2048 and B1_N8192 8 s each, the
  posterior steps 6 s — nearly all of it the float64 and rounding-model forwards on the CPU.  Cutting B or N of the largest case alone
  does not reach 29 s (without B12_N2048 altogether: about 57 s); the t list is not to be cut.

Two findings went into the yardsticks instead of into wider thresholds (details in tests/_errstats.py and oracle/highprec.py):
  * against the rounding model as first stated (bf16 rounding of both operands of to_q, to_out, FF net.0 and net.2) the folded bf16
    pack measured up to 1.39x on rms — above RB's cap once the 1.25 is applied — while the plain pack (dfx_debug_w1_fold(0)) measured 0.87x:
    the fold rounds weight DIFFERENCES (denoiser_setup.hip: k_pack_w1).  The model restates that pack (`w1_fold=`, the channel the engine
    reports): 1.13x.  The FF net.2 site stays a bf16 rounding of both operands although the kernels run it in fp16 with a polynomial
    fp16 GELU: the model overstates the operand rounding there (1 to 12 % of the yardstick) and states no GELU error (oracle/highprec.py).
  * in the DDIM update at small t the eps terms nearly cancel and the model's error on x_{t-1} falls to 1e-10; what a bf16 kernel shows
    there (2e-8) is the fp32 rounding of the update, equal to the fp32 oracle's own (ratio 1.0).  Outputs of the posterior step are
    therefore judged against RB x model + R32 x fp32 yardstick.
"""
import contextlib
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _errstats as es  # noqa: E402
from difffacto_amd import synth  # noqa: E402
from oracle import denoiser as odn  # noqa: E402
from oracle import diffusion as odf  # noqa: E402
from oracle import highprec as hp  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1000
T_LIST = (0, 1, 5, 6, 500, 998, 999)     # both ends and the middle: an off-by-one in c_t is smallest at small t
ALL_GROUPS = tuple(es.GROUPINGS)
#             name        B   N     seed mixed  group ratios asserted (every group >= 512 values; N = 100 is judged on rms and max alone)
EPS_CASES = {"B4_N2048": (4, 2048, 11, True, ALL_GROUPS),
             "B1_N8192": (1, 8192, 13, False, ("lane", "lane16", "wave", "tile", "coord")),
             "B3_N100": (3, 100, 14, True, ()),                       # the padded path
             "B12_N2048": (12, 2048, 15, True, ALL_GROUPS)}           # XCD remap (8 shapes) + natural-order tail (4)
#                  label               forced variant (tests/_variants.py; "direct": dfx_debug_force_direct)   lane grouping of the kernel
BF16_VARIANTS = (("k_denoise_pipe<8>", 8), ("k_denoise<bf16>", "direct"), ("k_denoise_coop", 1))
F32_VARIANTS = (("k_denoise_pipe_f32<8>", 8), ("k_denoise<f32>", 1))


def _tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _engine(W, prec, T=T):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from difffacto_amd.engine import DenoiserEngine
    return DenoiserEngine({k: _tt(v) for k, v in W.items()}, num_timesteps=T, precision=prec)


def _prep(eng, c):
    return eng.prepare_shapes(*map(_tt, (c["part_code"], c["mean"], c["var"], c["valid"])))


class _Run:
    """Force a kernel variant for the launches inside (tests/_variants.forced; "direct": dfx_debug_force_direct, which that helper
    does not cover), and assert afterwards (`ran`) that the last launch took it."""

    def __init__(self, prec, label, how):
        self.prec, self.label, self.how = prec, label, how
        self.stack = contextlib.ExitStack()

    def __enter__(self):
        from _variants import forced
        from difffacto_amd import _ffi
        if self.how == "direct":
            _ffi.lib().dfx_debug_force_direct(1)
            self.stack.callback(_ffi.lib().dfx_debug_force_direct, 0)
        else:
            self.stack.enter_context(forced(self.how))
        return self

    def __exit__(self, *exc):
        self.stack.close()

    def ran(self):
        from _variants import ran
        from difffacto_amd.engine import last_kernel_variant
        if self.how == "direct":
            assert last_kernel_variant() == self.label, f"expected {self.label}, the launch took {last_kernel_variant()}"
        else:
            assert ran(self.prec, self.how) == self.label
        return self.label


def _variants(prec):
    return BF16_VARIANTS if prec == "bf16" else F32_VARIANTS


def _judge(fails, label, variant, prec, got, truth, yard, groups=(), floor=None):
    """Print the case's line and collect its failures.  got, truth (B,3,N); yard: the yardstick's `stats` on the same case."""
    k = es.stats(np.asarray(got, dtype=np.float64) - truth)
    tail = "" if floor is None or prec != "bf16" else f" | fp32 floor max {floor['max']:.3e} rms {floor['rms']:.3e}"
    print(es.line(label, variant, k, yard) + tail, flush=True)
    fails += [f"{label} [{variant}]: {f}" for f in es.accept(prec, k, yard, groups if prec == "bf16" else (), floor)]
    return k


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    """Not a gate: the wall time of this module (CPU oracles included) goes next to the measurements."""
    t0 = time.time()
    yield
    print(f"\nHIGHPREC wall time of tests/test_gpu_denoiser_highprec.py: {time.time() - t0:.0f} s", flush=True)


@pytest.fixture(scope="module")
def W():
    return synth.make_denoiser_weights(seed=0)


@pytest.fixture(scope="module")
def tb():
    return odf.Tables(T)


@pytest.fixture(scope="module")
def engines(W):
    e = {}

    def get(prec):
        if prec not in e:
            e[prec] = _engine(W, prec)
        return e[prec]
    yield get
    for v in e.values():
        v.close()


def _fold_of(eng):
    """The hidden channel whose K slot carries the first FF bias in this bf16 engine's pack (None: plain pack): the rounding model
    restates the pack the engine reports (oracle/highprec.py: w1_fold)."""
    folded, _ = eng.w1_fold()
    return eng.w1_fold_channel() if folded else None


@pytest.fixture(scope="module")
def yardsticks(W, engines):
    """(case name, t[, weights, fold]) -> the case, the float64 eps, the fp32 oracle's eps and the rounding model's eps, computed once
    and shared by every variant, precision and test of this module."""
    cache, exact, cases, nets = {}, {}, {}, {}

    def get(name, t, Wx=None, wkey="W", fold="engine"):
        if fold == "engine":
            fold = _fold_of(engines("bf16"))
            assert fold == 127, fold
        if name not in cases:
            B, N, seed, mixed, _ = EPS_CASES[name]
            cases[name] = es.make_case(B, N, seed, mixed)
        c = cases[name]
        Wx = W if Wx is None else Wx
        tk = tuple(np.atleast_1d(t).tolist())
        if (name, tk, wkey) not in exact:          # the truth and the fp32 oracle do not depend on the pack
            if wkey not in nets:
                nets[wkey] = hp.Net(Wx)
            exact[name, tk, wkey] = (es.eps_of(hp, nets[wkey], c, t), es.eps_of(odn, Wx, c, t))
        truth, e32 = exact[name, tk, wkey]
        key = (name, tk, wkey, fold)
        if key not in cache:
            if (wkey, fold) not in nets:
                nets[wkey, fold] = hp.Net(Wx, operand_round="bf16", w1_fold=fold)
            emod = es.eps_of(hp, nets[wkey, fold], c, t)
            cache[key] = dict(case=c, truth=truth, eps32=e32, epsmod=emod, f32=es.stats(e32 - truth), bf16=es.stats(emod - truth))
        return cache[key]
    return get


# ------------------------------------------------------------------------------------------------ eps
@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("name", sorted(EPS_CASES))
def test_eps_every_variant_vs_float64(yardsticks, engines, name, prec):
    eng = engines(prec)
    groups = EPS_CASES[name][4]
    fails = []
    cx = None
    for t in T_LIST:
        y = yardsticks(name, t)
        c = y["case"]
        cx = cx or _prep(eng, c)
        for label, how in _variants(prec):
            with _Run(prec, label, how) as r:
                eps = eng.eps(cx, _tt(c["x"]), _tt(c["seg"]), t).cpu().numpy()
                r.ran()
            _judge(fails, f"eps {name} t={t}", label, prec, eps, y["truth"], y[prec], groups)
    assert not fails, "\n".join(fails)


def test_eps_bf16_plain_w1_pack_and_moved_fold_channel_vs_float64(W, yardsticks):
    """The bf16 engine without the W1 bias fold (dfx_debug_w1_fold(0)), and on the weights whose outlier gamma3[127] moves the fold to
    another channel (as in test_w1_bias_fold_moves_to_another_channel_around_an_outlier_and_is_selectable): the rounding model runs
    on the same weights and restates the pack the engine reports, so the yardstick moves with them.  Over the whole t list, on the two
    shapes whose group statistics are asserted; the kernel is the launcher's own choice, as these packs restrict it (the plain pack
    rules the pipelined and co-operative 32-point kernels out) and the other variants of each are bit-identical."""
    from difffacto_amd import _ffi
    from difffacto_amd.engine import last_kernel_variant
    Wo = {k: v.copy() for k, v in W.items()}
    Wo["transformer_blocks.2.norm3.weight"][127] *= 64.0
    fails = []
    for wkey, Wx, mode in (("W", W, 0), ("outlier", Wo, -1)):
        _ffi.lib().dfx_debug_w1_fold(mode)
        try:
            eng = _engine(Wx, "bf16")
        finally:
            _ffi.lib().dfx_debug_w1_fold(-1)
        ch = _fold_of(eng)
        assert ch is None if mode == 0 else ch not in (127, None), (wkey, ch)
        for name in ("B4_N2048", "B1_N8192"):
            cx = None
            for t in T_LIST:
                y = yardsticks(name, t, Wx, wkey, ch)
                c = y["case"]
                cx = cx or _prep(eng, c)
                eps = eng.eps(cx, _tt(c["x"]), _tt(c["seg"]), t).cpu().numpy()
                v = last_kernel_variant()
                _judge(fails, f"eps {name} t={t} weights={wkey} w1_fold={'plain' if ch is None else f'channel {ch}'}", v, "bf16", eps,
                       y["truth"], y["bf16"], EPS_CASES[name][4])
        eng.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_eps_t_per_shape_t_vs_float64(yardsticks, engines, prec):
    """dfx_denoise_eps_t: every shape at its own t, judged per shape (rms, max) and over the tensor (lane and wavefront groups)."""
    name, tt = "B4_N2048", np.array([0, 999, 5, 500])
    eng = engines(prec)
    y = yardsticks(name, tt)
    c = y["case"]
    cx = _prep(eng, c)
    ymod = y["eps32"] if prec == "f32" else y["epsmod"]
    fails = []
    variants = (("k_denoise_pipe<8>", 8), ("k_denoise<bf16>", "direct")) if prec == "bf16" else F32_VARIANTS
    for label, how in variants:
        with _Run(prec, label, how) as r:
            eps = eng.eps_t(cx, _tt(c["x"]), _tt(c["seg"]), _tt(tt.astype(np.int32))).cpu().numpy()
            r.ran()
        _judge(fails, f"eps_t {name} t={tt.tolist()}", label, prec, eps, y["truth"], y[prec], ("lane", "lane16", "wave", "tile", "coord"))
        for b in range(c["B"]):
            _judge(fails, f"eps_t {name} shape {b} t={int(tt[b])}", label, prec, eps[b:b + 1], y["truth"][b:b + 1],
                   es.stats(ymod[b:b + 1] - y["truth"][b:b + 1]))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ one posterior step
_P32 = {}     # (sampler, t) -> the fp32 numpy oracle's step on the B4_N2048 case: the fp32 yardstick, and the bf16 kernels' fp32 floor


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("sampler", ["ddpm", "ddim_eta0", "ddim_eta1"])
def test_p_sample_vs_float64(W, yardsticks, engines, sampler, prec):
    """dfx_p_sample / dfx_p_sample_ddim fed the oracle's own x_t: x_{t-1} and pred_xstart.  The posterior is exact in the rounding model
    (fp32 VALU work on the GPU), so the model's x_{t-1} is the float64 posterior of the model's eps.  The DDIM x_{t-1} of the bf16
    kernels alone is judged with the fp32 yardstick added (`floor`): at small t its two eps terms nearly cancel, the model's error on
    x_{t-1} drops to 1e-10 and what is left of a bf16 kernel's error is the fp32 rounding of the update (equal to the fp32 oracle's own).
    The DDPM x_{t-1} and pred_xstart are judged against the model alone."""
    name = "B4_N2048"
    eng = engines(prec)
    eta = None if sampler == "ddpm" else float(sampler[-1])
    tbx = odf.Tables(T) if eta is None else odf.Tables(T, ddim_sampling=True, ddim_nsteps=10, ddim_eta=eta)
    fails = []
    cx = None
    label, how = _variants(prec)[0]
    groups = ("lane", "lane16", "wave", "tile")
    for t in T_LIST:
        y = yardsticks(name, t)
        c = y["case"]
        cx = cx or _prep(eng, c)
        z = np.random.default_rng(1000 + t).standard_normal(c["x"].shape).astype(np.float32)
        args = (c["x"], t, c["anchors"], c["ctx"], c["variance"], c["seg"], c["valid"], z)
        truth = hp.p_sample(tbx, W, *args, eps=y["truth"])
        if (sampler, t) not in _P32:
            _P32[sampler, t] = odf.p_sample(tbx, W, *args)
        y32 = _P32[sampler, t]
        yd = y32 if prec == "f32" else hp.p_sample(tbx, W, *args, eps=y["epsmod"])
        with _Run(prec, label, how) as r:
            if eta is None:
                xp, x0 = eng.p_sample(cx, _tt(c["x"]), _tt(c["seg"]), t, noise=_tt(z), want_xstart=True)
            else:
                xp, x0 = eng.p_sample_ddim(cx, _tt(c["x"]), _tt(c["seg"]), t, eta, noise=_tt(z), want_xstart=True)
            r.ran()
        for key, got in (("sample", xp), ("pred_xstart", x0)):
            ys = es.stats(np.asarray(yd[key], dtype=np.float64) - truth[key])
            floor = None        # the DDIM x_{t-1} alone is judged with the fp32 yardstick added (tests/_errstats.accept)
            if eta is not None and key == "sample" and prec == "bf16":
                floor = es.stats(np.asarray(y32[key], dtype=np.float64) - truth[key])
            _judge(fails, f"p_sample[{sampler}] {key} {name} t={t}", label, prec, got.cpu().numpy(), truth[key], ys, groups, floor)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ T = 100 chain
CHAIN_CASES = {"B4_N256": (4, 256, 5, 10),      # the inputs of test_chain_bf16_vs_f32_reported
               "B2_N64": (2, 64, 77, 9)}        # the inputs of test_chain_f32_vs_oracle_T100


@pytest.fixture(scope="module")
def chains(W):
    """T = 100 DDPM chains on the CPU — float64, fp32 numpy oracle, rounding model —, final cloud and every 10th snapshot."""
    cache = {}

    def get(name):
        if name not in cache:
            B, N, lseed, nseed = CHAIN_CASES[name]
            Tc = 100
            eb = _engine(W, "bf16", T=Tc)
            fold = _fold_of(eb)
            eb.close()
            part_code, mean, logvar, valid = synth.make_latents(B, seed=lseed)
            seg = synth.make_seg_mask(valid, N)
            var = np.exp(logvar).astype(np.float32)
            rng = np.random.default_rng(nseed)
            xT = rng.standard_normal((B, 3, N)).astype(np.float32)
            zs = rng.standard_normal((Tc, B, 3, N)).astype(np.float32)
            anchors, variance = odf.gather_params(seg, mean, var)
            args = (anchors, [part_code, np.concatenate([mean, var], 1)], variance, seg, valid, xT, zs)
            tbc = odf.Tables(Tc)
            cache[name] = dict(lat=(part_code, mean, var, valid), seg=seg, xT=xT, zs=zs,
                               truth=hp.decode(tbc, W, *args, ret_traj=True, ret_interval=10),
                               f32=odf.decode(tbc, W, *args, ret_traj=True, ret_interval=10),
                               bf16=hp.decode(tbc, W, *args, ret_traj=True, ret_interval=10, operand_round="bf16", w1_fold=fold))
        return cache[name]
    return get


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("name", sorted(CHAIN_CASES))
def test_chain_T100_vs_float64(W, chains, name, prec):
    """dfx_sample_chain, explicit noise: the final cloud and every snapshot against the float64 chain, relative to the yardstick chain's
    own deviation at the same snapshot.  (The weights are contractive at this length: the three CPU chains stay together.)"""
    from _variants import ran
    ch = chains(name)
    eng = _engine(W, prec, T=100)
    cx = eng.prepare_shapes(*map(_tt, ch["lat"]))
    pred, traj = eng.sample_chain(cx, _tt(ch["seg"]), x_T_noise=_tt(ch["xT"]), step_noise=_tt(ch["zs"]), ret_interval=10)
    v = ran(prec)
    got = {"pred": pred.cpu().numpy()}
    for k, t in enumerate(eng.snapshot_times(10)):
        got[t] = traj[k].cpu().numpy()
    eng.close()
    fails = []
    for key in ["pred"] + [t for t in got if t != "pred"]:
        truth = ch["truth"][key].transpose(0, 2, 1)
        ys = es.stats(np.asarray(ch[prec][key], dtype=np.float64).transpose(0, 2, 1) - truth)
        if key == 100:           # the prior sample x_T = a + L z: no network in it; fp32 against fp32 in both precisions
            ys = es.stats(np.asarray(ch["f32"][key], dtype=np.float64).transpose(0, 2, 1) - truth)
            _judge(fails, f"chain T=100 {name} snapshot t={key}", v, "f32", got[key].transpose(0, 2, 1), truth, ys)
            continue
        _judge(fails, f"chain T=100 {name} {'final cloud' if key == 'pred' else f'snapshot t={key}'}", v, prec, got[key].transpose(0, 2, 1),
               truth, ys)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ q_sample, masked MSE
ULPS = 4      # see the two docstrings


def test_q_sample_vs_float64_in_ulps(W, engines, tb):
    """k_q_sample evaluates sa (x0 - a) + a + s1 sqrt(v) z in fp32 without contraction: seven roundings (the difference, its product,
    the sum, the square root, two products, the last sum), each at most half an ulp of its result, none larger than the largest term
    -> 3.5, gated at 4 ulps of the largest term of each element.  B = 1 and B = 3, N = 100 and N = 1000 (not multiples of 32 / 256)."""
    eng = engines("f32")
    worst = 0.0
    for B, N, seed in ((1, 100, 21), (3, 1000, 22), (1, 8190, 23)):
        c = es.make_case(B, N, seed, mixed=B > 1)
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((B, 3, N)).astype(np.float32)
        tt = np.array([0, 999, 500][:B]) if B > 1 else np.array([seed * 37 % T])
        q = eng.q_sample(_prep(eng, c), _tt(c["seg"]), _tt(c["x"]), _tt(tt.astype(np.int32)), _tt(z)).cpu().numpy()
        ref = hp.q_sample(tb, c["x"], tt, c["anchors"], z, c["variance"])
        a, x0, v = (np.asarray(k, dtype=np.float64) for k in (c["anchors"], c["x"], c["variance"]))
        sa = hp.coef(tb, "sqrt_alphas_cumprod", tt)[:, None, None]
        s1 = hp.coef(tb, "sqrt_one_minus_alphas_cumprod", tt)[:, None, None]
        big = np.maximum.reduce([np.abs(x0 - a), np.abs(a), np.abs(s1 * np.sqrt(v) * z), np.abs(sa * (x0 - a) + a), np.abs(ref)])
        ulps = np.abs(q - ref) / np.spacing(big.astype(np.float32)).astype(np.float64)
        print(f"HIGHPREC q_sample B={B} N={N} t={tt.tolist()} [k_q_sample] max {np.abs(q - ref).max():.3e} | worst element {ulps.max():.2f} ulps "
              f"of its largest term (gate {ULPS})", flush=True)
        worst = max(worst, float(ulps.max()))
        assert odf.q_sample(tb, c["x"], tt, c["anchors"], z, c["variance"]).dtype == np.float32
    assert worst <= ULPS, worst


def test_masked_mse_vs_float64_in_ulps(engines):
    """k_masked_mse: per point ((t - p)^2 fl) summed over 3 coordinates and divided by 3 in fp32, then float64 accumulation and one
    cast.  Every term is non-negative, so the relative error of the loss is at most that of a term: the difference 0.5 ulp (doubled by
    the square: 1), the square 0.5, the flag product 0.5, two sums 1, the division 0.5, the final cast 0.5 -> 4 ulps of the loss in the
    worst case of equal signs everywhere."""
    eng = engines("f32")
    worst = 0.0
    for B, N, seed in ((1, 100, 31), (1, 8190, 32), (3, 1000, 33)):
        rng = np.random.default_rng(seed)
        target = rng.standard_normal((B, 3, N)).astype(np.float32)
        pred = (target + 0.3 * rng.standard_normal((B, 3, N))).astype(np.float32)
        flags = (rng.random((B, 1, N)) < 0.7).astype(np.float32)
        for name, fl in (("flags", flags), ("noflags", None)):
            got = float(eng.masked_mse(_tt(target), _tt(pred), None if fl is None else _tt(fl)).item())
            ref = hp.masked_mse(target, pred, fl)
            ulps = abs(got - ref) / float(np.spacing(np.float32(ref)))
            print(f"HIGHPREC masked_mse B={B} N={N} {name} [k_masked_mse] loss {ref:.9f} err {abs(got - ref):.3e} = {ulps:.2f} ulps (gate {ULPS})",
                  flush=True)
            worst = max(worst, ulps)
    assert worst <= ULPS, worst
