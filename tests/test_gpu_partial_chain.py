"""Partial reverse chains on the GPU: dfx_sample_chain_from (a caller's state), dfx_refine_chain (q_sample fused into the prologue),
dfx_sample_chain_ddim_from and the `hold` mask, through DenoiserEngine.

What is asserted bit for bit needs no tolerance: a step is a pure function of (x, t, ctx, seed, global point id) and a snapshot is an exact
fp32 copy of the state, so a chain resumed from its own snapshot continues it; the fused start computes q_sample's expression; a held point
is a copy.  Everything against the reference's goldens / the numpy oracle is gated by the existing fp32 chain gate (test_gpu_denoiser.py).

Sweep shape: T = 12, B = 3, N = 288 (one full 256-point tile of the pipelined kernels and a partial one: wavefronts that store nothing),
one shape with an absent part, one with a single part.  k_denoise_coop2 takes N % 64 == 0: it runs at N = 320."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from difffacto_amd import synth  # noqa: E402
from oracle import diffusion as odf  # noqa: E402
from _variants import forced, ran  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL_F32_CHAIN = 1e-3            # the existing gates of tests/test_gpu_denoiser.py
TOL_BF16_CHAIN_T100 = 3.5e-3
VARIANTS = [("bf16", 8), ("bf16", 4), ("bf16", 2), ("bf16", 1), ("bf16", 16), ("f32", 8), ("f32", 4), ("f32", 2), ("f32", 1)]
VIDS = [p + "-" + {1: "coop" if p == "bf16" else "direct", 16: "coop2"}.get(n, "pipe%d" % n) for p, n in VARIANTS]
T, B = 12, 3
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def W():
    return synth.make_denoiser_weights(seed=0)


_ENGINES = {}


def _engine(W, T, prec):
    from difffacto_amd.engine import DenoiserEngine
    if (T, prec) not in _ENGINES:
        _ENGINES[(T, prec)] = DenoiserEngine({k: torch.from_numpy(v) for k, v in W.items()}, num_timesteps=T, precision=prec)
    return _ENGINES[(T, prec)]


def _case(N, B=B, seed=41):
    """Latents, part ids and a clean cloud (points around their part's anchor) of the sweep batch, as numpy."""
    part_code, mean, logvar, valid = synth.make_latents(B, seed=seed, all_valid=True)
    if B >= 3:
        valid[1] = [1, 0, 1, 1]      # an absent part
        valid[2] = [0, 0, 1, 0]      # a single part
    var = np.exp(logvar).astype(np.float32)
    seg = synth.make_seg_mask(valid, N)
    anchors, variance = odf.gather_params(seg, mean, var)
    rng = np.random.default_rng(N + seed)
    x0 = (anchors + 0.5 * np.sqrt(variance) * rng.standard_normal((B, 3, N))).astype(np.float32)
    return dict(part_code=part_code, mean=mean, var=var, valid=valid, seg=seg, anchors=anchors, variance=variance, x0=x0,
                cctx=[part_code, np.concatenate([mean, var], 1)], rng=rng)


def _ctx(eng, c, rows=slice(None)):
    return eng.prepare_shapes(*(torch.from_numpy(np.ascontiguousarray(c[k][rows])) for k in ("part_code", "mean", "var", "valid")))


def _n_of(nw):
    return 320 if nw == 16 else 288


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
@pytest.mark.parametrize("tag", ["B2_N128_mixed", "B3_N64_allvalid"])
def test_from_golden_states_f32(W, tag):
    """The reference's own trajectory (T = 10): from its state i, the remaining 10 - i steps with its noise give its `pred` and its t = 5 entry."""
    g = np.load(os.path.join(GOLDEN, f"chain_T10_{tag}.npz"))
    eng = _engine(W, 10, "f32")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ctx = eng.prepare_shapes(t(g["part_code"]), t(g["mean"]), t(np.exp(g["logvar"]).astype(np.float32)), t(g["valid"]))
    ri = int(g["ret_interval"])
    assert ri == 5
    for i in (0, 3, 9):
        n = 10 - i
        pred, traj = eng.sample_chain_from(ctx, t(g["seg"]), t(g["traj"][i]), n, step_noise=t(g["step_noise"][i:]), ret_interval=ri)
        err = float(np.abs(pred.cpu().numpy() - g["decode_pred"]).max())
        times = eng.snapshot_times(ri, n)
        assert times == {0: [10, 5], 3: [5], 9: []}[i] and traj.shape[0] == len(times)
        print(f"golden {tag} from state {i} ({n} steps): pred max-abs {err:.3e}")
        assert err < TOL_F32_CHAIN, (i, err)
        for k, tt in enumerate(times):
            e = float(np.abs(traj[k].cpu().numpy() - g[f"decode_{tt}"]).max())
            assert e < TOL_F32_CHAIN, (i, tt, e)


# ------------------------------------------------------------------------------------------------ 2. resume identity
@pytest.mark.parametrize("prec,nw", VARIANTS, ids=VIDS)
def test_resume_from_own_snapshot_is_bitwise(W, prec, nw):
    N, ri, seed = _n_of(nw), 4, 2024
    eng = _engine(W, T, prec)
    c = _case(N)
    ctx, seg = _ctx(eng, c), cu(c["seg"])
    with forced(nw):
        full_pred, full_traj = eng.sample_chain(ctx, seg, seed=seed, ret_interval=ri)
        ran(prec, nw)
        times = eng.snapshot_times(ri)
        assert times == [12, 8, 4]
        for k, ts in enumerate(times):
            x = full_traj[k].transpose(1, 2).contiguous()          # (B,N,3) snapshot -> (B,3,N) state
            pred, traj = eng.sample_chain_from(ctx, seg, x, ts, seed=seed, ret_interval=ri)
            ran(prec, nw)
            _same(pred, full_pred, f"pred from t={ts}")
            later = eng.snapshot_times(ri, ts)
            assert later == ([12, 8, 4] if ts == 12 else times[k + 1:]) and traj.shape[0] == len(later)
            _same(traj, full_traj[len(times) - len(later):], f"snapshots from t={ts}")
    assert bool(torch.isfinite(full_pred).all())


@pytest.mark.parametrize("prec,nw", VARIANTS, ids=VIDS)
def test_ddim_resume_from_own_snapshot_is_bitwise(W, prec, nw):
    """'quad' list on T = 40, [0, 0, 2, 5, 10, 16, 23, 32]: from the t = 10 slot, the entries below 10."""
    N, ri, seed, eta = _n_of(nw), 5, 77, 1.0
    eng = _engine(W, 40, prec)
    steps = odf.Tables(40, ddim_sampling=True, ddim_nsteps=8, ddim_discretize="quad", ddim_eta=eta).steps
    assert steps == [0, 0, 2, 5, 10, 16, 23, 32]
    c = _case(N)
    ctx, seg = _ctx(eng, c), cu(c["seg"])
    with forced(nw):
        full_pred, full_traj = eng.sample_chain_ddim(ctx, seg, steps, eta, seed=seed, ret_interval=ri)
        ran(prec, nw)
        times = eng.snapshot_times(ri)
        x = full_traj[times.index(10)].transpose(1, 2).contiguous()
        pred, traj = eng.sample_chain_ddim(ctx, seg, steps[:4], eta, seed=seed, ret_interval=ri, x_init=x, n_steps=10)
        ran(prec, nw)
    _same(pred, full_pred, "ddim pred from t=10")
    assert traj.shape[0] == 1                                        # t = 5, the one executed timestep with a slot
    _same(traj[0], full_traj[times.index(5)], "ddim snapshot t=5")


# ------------------------------------------------------------------------------------------------ 3. fused start = q_sample + given state
@pytest.mark.parametrize("prec,nw", VARIANTS, ids=VIDS)
def test_refine_equals_q_sample_then_from_bitwise(W, prec, nw):
    N, ri = _n_of(nw), 4
    eng = _engine(W, T, prec)
    c = _case(N)
    ctx, seg, x0 = _ctx(eng, c), cu(c["seg"]), cu(c["x0"])
    z = cu(c["rng"].standard_normal((B, 3, N)).astype(np.float32))
    zs = cu(c["rng"].standard_normal((T, B, 3, N)).astype(np.float32))
    for n in (1, 5, 12):
        x_t = eng.q_sample(ctx, seg, x0, torch.full((B,), n - 1, dtype=torch.int32), z)
        with forced(nw):
            want_pred, want_traj = eng.sample_chain_from(ctx, seg, x_t, n, step_noise=zs[:n], ret_interval=ri)
            ran(prec, nw)
            pred, traj = eng.refine_chain(ctx, seg, x0, n, start_noise=z, step_noise=zs[:n], ret_interval=ri)
            ran(prec, nw)
        _same(pred, want_pred, f"pred n={n}")
        times = eng.snapshot_times(ri, n, fused=True)
        assert times == {1: [], 5: [4], 12: [8, 4]}[n] and traj.shape[0] == len(times)
        _same(traj, want_traj[want_traj.shape[0] - len(times):], f"snapshots n={n}")
        assert not torch.equal(pred, x0.transpose(1, 2))


# ------------------------------------------------------------------------------------------------ 4. numpy oracle, padded N
def test_refine_and_ddim_from_vs_oracle_N100(W):
    N = 100
    eng = _engine(W, T, "f32")
    c = _case(N)
    ctx, seg = _ctx(eng, c), cu(c["seg"])
    z = c["rng"].standard_normal((B, 3, N)).astype(np.float32)
    zs = c["rng"].standard_normal((T, B, 3, N)).astype(np.float32)
    tb = odf.Tables(T)
    for n in (1, 5, 12):
        x = odf.q_sample(tb, c["x0"], np.full((B,), n - 1), c["anchors"], z, c["variance"]).astype(np.float32)
        snaps = {}
        for i, t in enumerate(range(n - 1, -1, -1)):
            x = odf.p_sample(tb, W, x, t, c["anchors"], c["cctx"], c["variance"], c["seg"], c["valid"], zs[i])["sample"]
            snaps[t] = x
        pred, traj = eng.refine_chain(ctx, seg, cu(c["x0"]), n, start_noise=cu(z), step_noise=cu(zs[:n]), ret_interval=4)
        assert pred.shape == (B, N, 3) and pred.is_contiguous()
        err = float(np.abs(pred.cpu().numpy() - x.transpose(0, 2, 1)).max())
        print(f"refine_chain N=100 n={n}: max-abs vs oracle {err:.3e}")
        assert err < TOL_F32_CHAIN, (n, err)
        for k, t in enumerate(eng.snapshot_times(4, n, fused=True)):
            assert traj.shape[1:] == (B, N, 3)
            assert float(np.abs(traj[k].cpu().numpy() - snaps[t].transpose(0, 2, 1)).max()) < TOL_F32_CHAIN, (n, t)
    # DDIM from a given state: the oracle's own tables ('quad' on T = 40), the entries below 16
    tbd = odf.Tables(40, ddim_sampling=True, ddim_nsteps=8, ddim_discretize="quad", ddim_eta=1.0)
    engd = _engine(W, 40, "f32")
    ctxd = _ctx(engd, c)
    steps = [s for s in tbd.steps if s < 16]
    assert steps == [0, 0, 2, 5, 10]
    x = x_init = odf.q_sample(tbd, c["x0"], np.full((B,), 10), c["anchors"], z, c["variance"]).astype(np.float32)
    for i, t in enumerate(steps[::-1]):
        x = odf.p_sample(tbd, W, x, t, c["anchors"], c["cctx"], c["variance"], c["seg"], c["valid"], zs[i])["sample"]
    pred, _ = engd.sample_chain_ddim(ctxd, seg, steps, 1.0, step_noise=cu(zs[:len(steps)]), x_init=cu(x_init), n_steps=16)
    err = float(np.abs(pred.cpu().numpy() - x.transpose(0, 2, 1)).max())
    print(f"sample_chain_ddim x_init N=100 steps {steps}: max-abs vs oracle {err:.3e}")
    assert err < TOL_F32_CHAIN, err


# ------------------------------------------------------------------------------------------------ 5. bf16 against fp32
def test_refine_bf16_vs_f32_T100(W):
    TT, BB, N, n = 100, 2, 128, 40
    ef, eb = _engine(W, TT, "f32"), _engine(W, TT, "bf16")
    c = _case(N, B=BB, seed=5)
    rng = c["rng"]
    xT = cu(rng.standard_normal((BB, 3, N)).astype(np.float32))
    zs = cu(rng.standard_normal((TT, BB, 3, N)).astype(np.float32))
    seg, x0 = cu(c["seg"]), cu(c["x0"])
    cf, cb = _ctx(ef, c), _ctx(eb, c)
    full = (ef.sample_chain(cf, seg, x_T_noise=xT, step_noise=zs)[0] - eb.sample_chain(cb, seg, x_T_noise=xT, step_noise=zs)[0]).abs()
    pf, _ = ef.refine_chain(cf, seg, x0, n, start_noise=xT, step_noise=zs[TT - n:])
    pb, _ = eb.refine_chain(cb, seg, x0, n, start_noise=xT, step_noise=zs[TT - n:])
    d = (pf - pb).abs()
    print(f"bf16 vs f32, T=100 B=2 N=128: refine_chain n=40 max-abs {d.max().item():.3e} (mean {d.mean().item():.3e}); "
          f"full chain on the same inputs max-abs {full.max().item():.3e} (mean {full.mean().item():.3e})")
    assert d.max().item() <= TOL_BF16_CHAIN_T100


# ------------------------------------------------------------------------------------------------ 6. held parts
def _hold_masks(valid):
    """Per-shape bitmasks: one present part / all present parts but one / a bit of an absent part (none where every part is present)."""
    first = np.argmax(valid, axis=1)
    present = (valid != 0).astype(np.int64) @ (1 << np.arange(valid.shape[1]))
    absent = np.array([0 if v.all() else 1 << int(np.argmin(v)) for v in valid])
    return {"one part": 1 << first, "all but one": present & ~(1 << first), "absent part": absent}


@pytest.mark.parametrize("prec,nw", [("bf16", 8), ("bf16", 1), ("f32", 1)], ids=["bf16-pipe8", "bf16-coop", "f32-direct"])
def test_held_parts_are_the_source_and_the_rest_is_untouched(W, prec, nw):
    N, ri, seed = 288, 4, 99
    eng = _engine(W, T, prec)
    c = _case(N)
    ctx, seg = _ctx(eng, c), cu(c["seg"])
    x = cu(c["x0"])
    src = x.transpose(1, 2)                                           # (B,N,3) like pred
    masks = _hold_masks(c["valid"])
    assert masks["absent part"].tolist() == [0, 2, 1] and masks["one part"].tolist() == [1, 1, 4] and masks["all but one"].tolist() == [14, 12, 0]
    runs = {"from": lambda **kw: eng.sample_chain_from(ctx, seg, x, T, seed=seed, ret_interval=ri, **kw),
            "refine": lambda **kw: eng.refine_chain(ctx, seg, x, 9, seed=seed, ret_interval=ri, **kw)}
    for how, run in runs.items():
        with forced(nw):
            free_pred, free_traj = run()
            ran(prec, nw)
        assert free_traj.shape[0] == (3 if how == "from" else 2)
        for name, mask in masks.items():
            with forced(nw):
                pred, traj = run(hold=torch.from_numpy(mask.astype(np.int32)))
                ran(prec, nw)
            held = ((cu(mask.astype(np.int64))[:, None] >> seg.long()) & 1).bool()   # (B,N)
            assert int(held.sum()) == {"one part": 72 + 144 + 288, "all but one": 216 + 144, "absent part": 0}[name]
            for what, got, free in [("pred", pred, free_pred)] + [(f"slot {k}", traj[k], free_traj[k]) for k in range(traj.shape[0])]:
                assert torch.equal(got[held], src[held]), (how, name, what, "held points")
                assert torch.equal(got[~held], free[~held]), (how, name, what, "other points")
        # the (B, n_class) 0/1 form of the same mask
        as_bits = torch.from_numpy(((masks["all but one"][:, None] >> np.arange(4)) & 1).astype(np.float32))
        with forced(nw):
            p2, _ = run(hold=as_bits)
            p1, _ = run(hold=torch.from_numpy(masks["all but one"].astype(np.int32)))
        _same(p2, p1, "hold as (B,n_class)")
        assert not torch.equal(free_pred, src)


# ------------------------------------------------------------------------------------------------ 7. batch split over calls
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_split_batch_with_shape_offset_is_bitwise(W, prec):
    N, seed = 288, 31337
    eng = _engine(W, T, prec)
    c = _case(N)
    seg, x0 = cu(c["seg"]), cu(c["x0"])
    hold = torch.tensor([1, 1, 0], dtype=torch.int32)
    for how in ("refine_chain", "sample_chain_from"):
        whole_pred, whole_traj = getattr(eng, how)(_ctx(eng, c), seg, x0, 9, seed=seed, ret_interval=4, hold=hold)
        for rows, off in ((slice(0, 2), 0), (slice(2, 3), 2)):
            pred, traj = getattr(eng, how)(_ctx(eng, c, rows), seg[rows], x0[rows], 9, seed=seed, ret_interval=4, hold=hold[rows], shape_offset=off)
            _same(pred, whole_pred[rows], f"{how} rows {rows}")
            _same(traj, whole_traj[:, rows], f"{how} snapshots rows {rows}")
        other, _ = getattr(eng, how)(_ctx(eng, c, slice(2, 3)), seg[2:], x0[2:], 9, seed=seed, hold=hold[2:], shape_offset=0)
        assert not torch.equal(other, whole_pred[2:])                    # the noise follows the global row


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors_raise_before_any_launch(W):
    from difffacto_amd import _ffi
    from difffacto_amd.engine import last_kernel_variant
    N = 64
    eng = _engine(W, T, "f32")
    c = _case(N)
    ctx, seg, x0 = _ctx(eng, c), cu(c["seg"]), cu(c["x0"])
    eng.eps(ctx, x0, seg, 0)
    _ffi.lib().dfx_set_event_timing(1)
    try:
        eng.eps(ctx, x0, seg, 0)
        marker = _ffi.lib().dfx_last_kernel_ms()                         # changes with every timed launch
        bad = [
            (lambda: eng.sample_chain_from(ctx, seg, x0, 0), "n_steps"),
            (lambda: eng.sample_chain_from(ctx, seg, x0, T + 1), "n_steps"),
            (lambda: eng.refine_chain(ctx, seg, x0, 0), "n_steps"),
            (lambda: eng.refine_chain(ctx, seg, x0, T + 1), "n_steps"),
            (lambda: eng.sample_chain_from(ctx, seg, None, 3), "start cloud"),
            (lambda: eng.refine_chain(ctx, seg, None, 3), "start cloud"),
            (lambda: eng.sample_chain_ddim(ctx, seg, [0, 2, 5], 1.0, x_init=x0, n_steps=5), "below n_steps"),
            (lambda: eng.sample_chain_ddim(ctx, seg, [1, 2], 1.0, x_init=x0), "start at 0"),
            (lambda: eng.sample_chain_from(ctx, seg, x0[:, :, :32], 3), r"\(B,3,N\)"),
            (lambda: eng.sample_chain_from(ctx, seg, x0, 3, step_noise=torch.zeros(2, B, 3, N)), "step_noise"),
            (lambda: eng.refine_chain(ctx, seg, x0, 3, start_noise=torch.zeros(B, 3, N + 32)), "start_noise"),
            (lambda: eng.sample_chain_from(ctx, seg, x0, 3, hold=torch.zeros(B + 1, dtype=torch.int32)), "hold"),
        ]
        for call, msg in bad:
            with pytest.raises(RuntimeError, match=msg):
                call()
            assert _ffi.lib().dfx_last_kernel_ms() == marker, msg
        # the C entry points check for themselves and say why
        pred = torch.empty(B, N, 3, device="cuda")
        L = _ffi.lib()
        p = _ffi.ptr
        for call, msg in [
            (lambda: L.dfx_sample_chain_from(eng._h, p(ctx.buf), p(seg), p(x0), 0, None, 0, 0, None, 0, None, p(pred), B, N, None), r"n_steps=0 outside \[1,12\]"),
            (lambda: L.dfx_refine_chain(eng._h, p(ctx.buf), p(seg), p(x0), T + 1, None, None, 0, 0, None, 0, None, p(pred), B, N, None), r"n_steps=13 outside"),
            (lambda: L.dfx_sample_chain_from(eng._h, p(ctx.buf), p(seg), None, 3, None, 0, 0, None, 0, None, p(pred), B, N, None), "null start cloud"),
            (lambda: L.dfx_refine_chain(eng._h, p(ctx.buf), p(seg), p(x0), 3, None, None, 0, 0, None, 0, None, None, B, N, None), "null pred"),
            (lambda: L.dfx_sample_chain_from(eng._h, p(ctx.buf), p(seg), p(x0), 3, None, 0, 0, None, 0, None, p(pred), B, 48, None), "multiple of 32"),
        ]:
            with pytest.raises(RuntimeError, match=msg):
                _ffi.check(call(), "partial chain")
            assert L.dfx_last_kernel_ms() == marker, msg
        arr = (_ffi.ctypes.c_int32 * 2)(0, T)
        rc = L.dfx_sample_chain_ddim_from(eng._h, p(ctx.buf), p(seg), arr, 2, 1.0, p(x0), None, 0, 0, None, 0, None, p(pred), B, N, None)
        with pytest.raises(RuntimeError, match="outside"):
            _ffi.check(rc, "ddim from")
        assert L.dfx_last_kernel_ms() == marker
    finally:
        _ffi.lib().dfx_set_event_timing(0)
    # empty batch: a no-op
    pred, _ = eng.sample_chain_from(ctx, torch.zeros(0, N, dtype=torch.int32), torch.zeros(0, 3, N), 3)
    assert pred.shape == (0, N, 3)
    assert last_kernel_variant()
