"""The latent sampler (latents_kernels.hip with mfma_linear.h) and the aligner's training kernels (aligner_train.hip, noise_opt.hip) at the
configurations of tests/_latent_cfg.py beyond the shipped one, and at the batch sizes where dfx::lin::launch changes kernels.

Truth: the float64 restatement (oracle/latents_highprec.py; float64 autograd of `_aligner_torch` for gradients).  Yardstick: the fp32
numpy oracle's (the float32 CPU autograd's) error against the same truth on the same case.  A kernel is accepted when its max-abs and
rms errors are within F (FG for gradients) of the yardstick's; d_part_code and d_noise are judged shape by shape.  The existing
absolute gates (1e-4 x max(1, |ref|) for outputs, 5e-4 of max-abs for gradients) stay as outer bounds.  One `LATCFG` line per case is
printed; profiles/latent_configs_parity.txt holds them, tests/_latent_cfg.py the factors.

Which kernel runs where (from the conditions of dfx::lin::launch; `k_lin/4` = split-K):
  every configuration at B <= 11 (M <= 264 rows): k_lin or k_lin/4 (K >= 128 and <= 256 tiles) for all products; GEGLU and coupling products
    are k_lin at every size.  tiny: K = 24 (tail only), 56 (one trip + 3 tail blocks), N = 24, 40, 64, 6; wide: K = 104, 136 (split-K,
    tail on wave 0), 1024, 4096; k_attn<16> (tiny), <64> (wide), <32> (others); k_ln at 1 (tiny, one), 2 (plain), 4, 8 (mid), 16 (wide)
    values per lane
  shipped widths, R = 1344 / 1345 shapes: QKV (N = 768) last k_lin launch / first k_lin_wide launch (4-row last block); the rest k_lin
  R = 2047 / 2048: QKV k_lin_wide -> k_lin_wide_lds<4> (M = 8192); residual products (N = 256) k_lin
  S = 8192 (M = 32768): proj_in + class embedding (r_mod = 4) k_lin_wide_lds<2> (K = 288), QKV and to_out k_lin_wide_lds<4>, FF out
    (K = 1024) k_lin_wide; flows (4 groups) k_lin_wide_lds<4> for the two ReLU layers
  mid at R = 2048: proj_in and to_out (N = 512, K = 288 / 512) k_lin_wide_lds<2>, QKV (K = 512) k_lin_wide_lds<2>, FF out (K = 2048) k_lin_wide
  wide at R = 512 (M = 4096): proj_in + class embedding (r_mod = 8, N = 1024) k_lin_wide, QKV, to_out, FF out (K = 4096) k_lin_wide
"""
import functools

import numpy as np
import pytest
import torch

import _latent_cfg as lc
from oracle import latents as ol
from oracle import latents_highprec as oh

pytestmark = pytest.mark.gpu

OUT_TOL, G_RTOL, G_ATOL = 1e-4, 5e-4, 1e-7
FLOAT_OUT = ("part_code", "mean", "logvar", "params", "mean_per_point", "logvar_per_point")


@functools.lru_cache(maxsize=None)
def _weights(tag):
    W = lc.weights(tag)
    return W, oh.widen(W)


@functools.lru_cache(maxsize=None)
def _sampler(tag):
    from difffacto_amd.latents import LatentSampler
    cfg = lc.CONFIGS[tag]
    return LatentSampler(_weights(tag)[0], n_class=cfg["n_class"], zdim=cfg["zdim"], n_heads=cfg["heads"], d_head=cfg["d_head"], cimle=cfg["cimle"],
                         noise_dim=cfg["noise_dim"], noise_scale=lc.NOISE_SCALE)


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _kw(tag):
    cfg = lc.CONFIGS[tag]
    return dict(noise_scale=lc.NOISE_SCALE, heads=cfg["heads"], cimle=cfg["cimle"])


def _judge(label, variant, what, got, o32, truth, worst):
    """Outer absolute gate, then the yardstick gate at F; prints the case's line and keeps the worst ratio."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    truth = np.asarray(truth, np.float64)
    assert got.shape == truth.shape, (label, what, got.shape, truth.shape)
    assert np.abs(got - truth).max() <= OUT_TOL * max(1.0, np.abs(truth).max()), (label, what)
    k, y = lc.err_stats(got, truth), lc.err_stats(o32, truth)
    r = lc.ratio(k, y)
    if what not in worst or r > worst[what][0]:
        worst[what] = (r, (k, y))
    fails = lc.accept(k, y, lc.F)
    assert not fails, (label, variant, what, fails)


def _report(label, variant, worst):
    for what, (r, (k, y)) in worst.items():
        print(lc.line(label, variant, what, r, k, y), flush=True)


# ---------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("B", [1, 5, 11])
@pytest.mark.parametrize("tag", ["shipped", "tiny", "wide", "one", "plain", "mid"])
def test_inference_entry_points_follow_the_float64_restatement(tag, B):
    """flow_reverse, part_aligner, sample_latents (with and without a given part_code, every fixed_id pattern) and compose_latents.  B = 11 with
    J = 3 is 33 token rows: a partial 32-row tile.  npoints = 3 J: a multiple of J that is no multiple of 4 J."""
    cfg, (Wn, W64), ls = lc.CONFIGS[tag], _weights(tag), _sampler(tag)
    J, kw, npoints = cfg["n_class"], _kw(tag), 3 * cfg["n_class"]
    fixed = list(lc.fixed_patterns(J).items())
    for K in ((1, 3) if cfg["cimle"] else (1,)):
        worst, R = {}, B * K
        for pi, pattern in enumerate(lc.VALID_PATTERNS):
            x = lc.inputs(tag, B, K, 1000 * B + 10 * K + pi, pattern)
            depth = cfg["flow_depth"]
            # the pieces on their own
            if pi == 0:
                got = ls.flow_reverse(T(x["w_noise"]))
                if depth:
                    f32 = np.stack([ol.flow_reverse(np.ascontiguousarray(x["w_noise"][..., j]), Wn, j, depth) for j in range(J)], axis=-1)
                    f64 = np.stack([oh.flow_reverse(x["w_noise"][..., j], W64, j, depth) for j in range(J)], axis=-1)
                    _judge(f"{tag} B={B} K={K}", "flow_reverse", "flow", got, f32, f64, worst)
                else:
                    assert np.array_equal(got.cpu().numpy(), x["w_noise"])
            code_r, valid_r = np.repeat(x["code"], K, axis=0), np.repeat(x["valid"], K, axis=0)
            m, l = ls.part_aligner(T(code_r), T(valid_r), T(x["noise"]))
            m32, l32 = ol.part_aligner_forward(Wn, code_r, valid_r, x["noise"], **kw)
            m64, l64 = oh.part_aligner_forward(W64, code_r, valid_r, x["noise"], **kw)
            _judge(f"{tag} B={B} K={K} {pattern}", "part_aligner", "aligner mean", m, m32, m64, worst)
            _judge(f"{tag} B={B} K={K} {pattern}", "part_aligner", "aligner logvar", l, l32, l64, worst)
            # the editing front end with the identity recipe: the aligner's bits on copied codes and noise rows
            c = ls.compose_latents(T(x["code"]), np.repeat(np.arange(B)[:, None], J, axis=1).repeat(K, axis=0), T(valid_r), noise_src=T(x["noise"]), npoints=npoints)
            assert torch.equal(c["mean"], m) and torch.equal(c["logvar"], l) and np.array_equal(c["part_code"].cpu().numpy(), code_r)
            assert (c["noise"] is None) if not cfg["cimle"] else np.array_equal(c["noise"].cpu().numpy(), x["noise"])
            # sample_latents: two (fixed_id, given part_code) combinations per validity pattern, rotating through all eight
            for given in (False, True):
                fname, fid = fixed[(pi + 2 * given + (K == 3)) % 4]
                label = f"{tag} B={B} K={K} {pattern} fixed={fname} given={int(given)}"
                a = (None if given else x["w_noise"], x["noise"], x["valid"], fid, K, npoints)
                pc = dict(part_code=x["code"]) if given else {}
                o32 = ol.sample_latents(Wn, *a, **kw, **pc)
                o64 = oh.sample_latents(W64, *a, **kw, **pc)
                out = ls.sample_latents(T(a[0]), T(x["noise"]), T(x["valid"]), fid, K=K, npoints=npoints, part_code=T(x["code"]) if given else None)
                assert np.array_equal(out["seg_mask"].cpu().numpy(), o32["seg_mask"]) and out["seg_mask"].dtype == torch.int32, label
                assert np.array_equal(out["valid_id"].cpu().numpy(), o32["valid_id"]), label
                assert (out["noise"] is None) if not cfg["cimle"] else np.array_equal(out["noise"].cpu().numpy(), o32["noise"]), label
                if given or not depth:
                    assert np.array_equal(out["part_code"].cpu().numpy(), o32["part_code"]), label
                o32 = dict(o32, params=o32["ctx"][1])
                for k in FLOAT_OUT:
                    assert tuple(out[k].shape)[0] == R
                    _judge(label, "sample_latents", k, out[k], o32[k], o64[k], worst)
        _report(f"{tag} B={B} K={K}", "inference", worst)


def test_handle_level_rejections_without_cimle():
    ls, x = _sampler("plain"), lc.inputs("plain", 2, 1, 5)
    noise = np.zeros((2, 8), np.float32)
    ls.noise_dim = 8                                                    # let the Python layer's shape check pass: the library decides
    try:
        with pytest.raises(RuntimeError, match="noise must be given iff"):
            ls.part_aligner(T(x["code"]), T(x["valid"]), T(noise))
        with pytest.raises(RuntimeError, match="aligner_noise must be given iff"):
            ls.sample_latents(T(x["w_noise"]), T(noise), T(x["valid"]), K=1, npoints=10)
        with pytest.raises(RuntimeError, match="K must be 1 without cimle"):
            ls.sample_latents(T(x["w_noise"]), None, T(x["valid"]), K=2, npoints=10)
    finally:
        ls.noise_dim = 0
    with pytest.raises(RuntimeError, match="cIMLE"):
        ls.optimize_noise(T(x["code"]), T(x["valid"]), T(noise), {}, 3)


# ---------------------------------------------------------------------------------------------------- batch-size boundaries of the launcher
def _flows_torch(W, x, depth):
    """oracle/latents_highprec.py:flow_reverse for all parts in torch (float64 on the device: rocBLAS, not code under test).  x (S,Z,J)."""
    F = torch.nn.functional
    out = []
    for j in range(x.shape[2]):
        h = x[..., j]
        d = h.shape[1] - h.shape[1] // 2
        for i in range(depth - 1, -1, -1):
            p, swap = f"flow.{j}.chain.{i}.net_s_t.", i % 2 == 0
            if swap:
                h = torch.cat([h[:, d:], h[:, :d]], dim=1)
            t = F.relu(F.linear(h[:, :d], W[p + "0.weight"], W[p + "0.bias"]))
            s_t = F.linear(F.relu(F.linear(t, W[p + "2.weight"], W[p + "2.bias"])), W[p + "4.weight"], W[p + "4.bias"])
            n = h.shape[1] - d
            y1 = (h[:, d:] - s_t[:, n:]) / torch.sigmoid(s_t[:, :n] + 2.0)
            h = torch.cat([y1, h[:, :d]] if swap else [h[:, :d], y1], dim=1)
        out.append(h)
    return torch.stack(out, dim=-1)


def _truth_device(tag, x):
    """float64 (part_code, mean, logvar) of sample_latents(K = 1, nothing fixed) on the device."""
    cfg, Wn = lc.CONFIGS[tag], _weights(tag)[0]
    W = {k: torch.from_numpy(v).cuda().double() for k, v in Wn.items()}
    t = lambda a: torch.from_numpy(a).cuda().double()
    with torch.no_grad():
        code = _flows_torch(W, t(x["w_noise"]), cfg["flow_depth"])
        m, l = lc._aligner_torch(W, code, t(x["valid"]), t(x["noise"]), lc.NOISE_SCALE, cfg["heads"], cfg["cimle"])
    return {"part_code": code.cpu().numpy(), "mean": m.cpu().numpy(), "logvar": l.cpu().numpy()}


@pytest.mark.parametrize("tag", ["shipped_short", "mid", "wide"])
def test_device_float64_truth_is_the_numpy_restatement(tag):
    """The large cases take their float64 truth from torch on the device; here it is held to oracle/latents_highprec.py at B = 5, 1e-12 relative."""
    x = lc.inputs(tag, 5, 1, 77, "shape_all_absent")
    J = lc.CONFIGS[tag]["n_class"]
    o64 = oh.sample_latents(_weights(tag)[1], x["w_noise"], x["noise"], x["valid"], np.zeros(J), 1, J, **_kw(tag))
    dev = _truth_device(tag, x)
    for k, v in dev.items():
        assert np.abs(v - o64[k]).max() <= 1e-12 * np.abs(o64[k]).max(), (tag, k)


BOUNDARIES = [("shipped_short", 1344, -1), ("shipped_short", 1345, -1), ("shipped_short", 1345, 1), ("shipped_short", 1345, 0), ("shipped_short", 2047, -1),
              ("shipped_short", 2048, -1), ("shipped_short", 8192, -1), ("mid", 2048, -1), ("wide", 512, -1)]


@pytest.mark.parametrize("tag,S,split", BOUNDARIES)
def test_launcher_boundaries_follow_the_float64_truth(tag, S, split):
    """S shapes, K = 1 (M = S J token rows): the row counts on both sides of every kernel switch of dfx::lin::launch at the shipped widths (aligner
    depth 1, flow depth 2, so that the oracles stay short), K = 512 LDS blocks (mid) and r_mod = 8 / K = 4096 through k_lin_wide (wide);
    `split`: dfx_debug_lin_split_k mode (1 and 0 must pass the gate of the automatic choice)."""
    from difffacto_amd import _ffi
    cfg, (Wn, _), ls = lc.CONFIGS[tag], _weights(tag), _sampler(tag)
    J = cfg["n_class"]
    x = lc.inputs(tag, S, 1, 300 + S, "shape_all_absent")
    x["valid"][1::7, 0] = 0
    lib = _ffi.lib()
    lib.dfx_debug_lin_split_k(split)
    try:
        out = ls.sample_latents(T(x["w_noise"]), T(x["noise"]), T(x["valid"]), None, K=1, npoints=J)
        torch.cuda.synchronize()
    finally:
        lib.dfx_debug_lin_split_k(-1)
    o32 = ol.sample_latents(Wn, x["w_noise"], x["noise"], x["valid"], np.zeros(J), 1, J, **_kw(tag))
    truth, worst = _truth_device(tag, x), {}
    label = f"{tag} S={S} split_k={split}"
    assert np.array_equal(out["valid_id"].cpu().numpy(), x["valid"]) and np.array_equal(out["seg_mask"].cpu().numpy(), o32["seg_mask"])
    for k in ("part_code", "mean", "logvar"):
        _judge(label, "boundary", k, out[k], o32[k], truth[k], worst)
    _report(label, "boundary", worst)


# ---------------------------------------------------------------------------------------------------- training
def _route(tag, P, x, d_mean=True, d_logvar=True, code_grad=True, noise_grad=True):
    from difffacto_amd import training
    cfg = lc.CONFIGS[tag]
    for p in P.values():
        p.grad = None
    t = lambda a: torch.from_numpy(a).cuda()
    c, z = t(x["code"]).requires_grad_(code_grad), t(x["noise"]).requires_grad_(noise_grad)
    mean, logvar = training.aligner_train_forward(P, c, t(x["valid"]), z, n_class=cfg["n_class"], zdim=cfg["zdim"], n_heads=cfg["heads"], d_head=cfg["d_head"],
                                                  noise_dim=cfg["noise_dim"], noise_scale=lc.NOISE_SCALE)
    loss = 0
    if d_mean:
        loss = loss + (mean * t(x["d_mean"])).sum()
    if d_logvar:
        loss = loss + (logvar * t(x["d_logvar"])).sum()
    loss.backward()
    return dict(mean=mean.detach(), logvar=logvar.detach(), d_part_code=c.grad, d_noise=z.grad, grads={k: p.grad.clone() for k, p in P.items() if p.grad is not None})


def _judge_grads(label, got, t32, t64, worst, params=True):
    for k in ("d_part_code", "d_noise"):
        g, ref = got[k].cpu().numpy(), t64[k]
        assert np.abs(g - ref).max() <= G_ATOL + G_RTOL * np.abs(ref).max(), (label, k)
        r = lc.shape_ratio(g, t32[k], ref)
        worst[k] = max(worst.get(k, 0.0), float(r.max()))
        print(f"LATCFG {label} [training] {k}: worst shape {int(np.argmax(r))} at {r.max():.3f} x the yardstick's worst shape ({lc.per_shape(t32[k], ref).max():.3e})", flush=True)
        fails = lc.accept_shapes(g, t32[k], ref, lc.FG)
        assert not fails, (label, k, fails)
    if not params:
        return
    assert set(got["grads"]) == set(t64["grads"]) - {"pre_norm.weight", "pre_norm.bias"}
    top = (0.0, None)
    for n, g in got["grads"].items():
        g, ref = g.cpu().numpy(), t64["grads"][n]
        assert np.abs(g - ref).max() <= G_ATOL + G_RTOL * np.abs(ref).max(), (label, n)
        k, y = lc.err_stats(g, ref), lc.err_stats(t32["grads"][n], ref)
        top = max(top, (lc.ratio(k, y), n), key=lambda t: t[0])
        fails = lc.accept(k, y, lc.FG)
        assert not fails, (label, n, fails)
    worst["param"] = max(worst.get("param", 0.0), top[0])
    print(f"LATCFG {label} [training] {len(got['grads'])} parameter gradients: worst ratio {top[0]:.3f} ({top[1]})", flush=True)


@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("tag", ["shipped", "tiny", "wide", "one", "mid"])
def test_training_kernels_follow_float64_autograd(tag, B):
    """aligner_train_forward + backward at every cimle configuration and validity pattern (B = 17 with J = 3: 51 rows, a partial 16-row tile of k_mm).
    Before k_attn_bwd read `valid`, the shape with every part absent failed the per-shape gate here (its dq / dk are zero in the reference) while
    the 5e-4 gate of the tensor's max-abs still passed."""
    cfg, (Wn, W64), ls = lc.CONFIGS[tag], _weights(tag), _sampler(tag)
    for pi, pattern in enumerate(lc.VALID_PATTERNS):
        x = lc.inputs(tag, B, 1, 2000 * B + pi, pattern)
        label, worst = f"{tag} B={B} {pattern}", {}
        a = (Wn, tag, x["code"], x["valid"], x["noise"])
        t64, t32 = lc.autograd(*a, x["d_mean"], x["d_logvar"], torch.float64), lc.autograd(*a, x["d_mean"], x["d_logvar"], torch.float32)
        o32 = ol.part_aligner_forward(Wn, x["code"], x["valid"], x["noise"], **_kw(tag))
        train = _route(tag, lc.aligner_params(Wn, "cuda", grad=True), x)
        assert len(train["grads"]) == 7 + 13 * cfg["depth"]
        for k, o in (("mean", o32[0]), ("logvar", o32[1])):
            _judge(label, "training", "train " + k, train[k], o, t64[k], worst)
        m, l = ls.part_aligner(T(x["code"]), T(x["valid"]), T(x["noise"]))  # the inference kernels, as the existing test holds them together
        assert float((m - train["mean"]).abs().max()) < OUT_TOL and float((l - train["logvar"]).abs().max()) < OUT_TOL
        _report(label, "training", worst)
        _judge_grads(label, train, t32, t64, worst)
        # dfx_aligner_input_backward (frozen weights): the bits of the training backward's data gradients
        frozen = _route(tag, lc.aligner_params(Wn, "cuda", grad=False), x)
        assert not frozen["grads"] and torch.equal(frozen["mean"], train["mean"]) and torch.equal(frozen["logvar"], train["logvar"])
        assert torch.equal(frozen["d_part_code"], train["d_part_code"]) and torch.equal(frozen["d_noise"], train["d_noise"]), label
        alone = _route(tag, lc.aligner_params(Wn, "cuda", grad=False), x, code_grad=False)
        assert alone["d_part_code"] is None and torch.equal(alone["d_noise"], frozen["d_noise"])
        if pi == 3:       # one cotangent only, on the pattern with the all-absent shape
            for dm, dl in ((True, False), (False, True)):
                one = _route(tag, lc.aligner_params(Wn, "cuda", grad=True), x, d_mean=dm, d_logvar=dl)
                s64 = lc.autograd(*a, x["d_mean"] if dm else None, x["d_logvar"] if dl else None, torch.float64)
                s32 = lc.autograd(*a, x["d_mean"] if dm else None, x["d_logvar"] if dl else None, torch.float32)
                _judge_grads(f"{label} d_{'mean' if dm else 'logvar'} only", one, s32, s64, worst)


# ---------------------------------------------------------------------------------------------------- the noise optimizer
@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_noise_optimizer_trace_follows_the_float64_restatement(tag):
    """The check of test_gpu_noise_opt.py::test_trace_follows_the_float64_restatement_and_stopped_rows_freeze at J = 3, ND = 8 and J = 8, ND = 40,
    through the same editing.noise_opt_replay."""
    from difffacto_amd import editing
    cfg, ls = lc.CONFIGS[tag], _sampler(tag)
    J, Z, ND, R, MAXIT = cfg["n_class"], cfg["zdim"], cfg["noise_dim"], 4, 200
    rng = np.random.Generator(np.random.PCG64(13))
    code = rng.standard_normal((R, Z, J)).astype(np.float32)
    valid = np.ones((R, J), np.float32)
    valid[1, 1] = 0
    ref_mean = (rng.standard_normal((R, 3, J)) * 0.3).astype(np.float32)
    ref_var = (rng.uniform(0.2, 0.6, size=(R, 3, J)) ** 2).astype(np.float32)
    ep = np.array([0, 2, J - 1, 0])
    fix = np.ones((R, J), np.float32)
    fix[np.arange(R), ep] = 0
    new_mean = ref_mean[np.arange(R), :, ep] + np.array([0.15, 0.0, -0.1], np.float32)
    z0 = rng.standard_normal((R, ND)).astype(np.float32)
    prob = editing.noise_problem(valid, ref_mean, ref_var, fix, ep, new_mean=new_mean)
    code, valid, z0 = map(torch.from_numpy, (code, valid, z0))
    out = ls.optimize_noise(code, valid, z0, prob, MAXIT, trace=True)
    tr, iters, zend = out["trace"].cpu().numpy().astype(np.float64), out["iters_done"].cpu().numpy(), out["z"].cpu().numpy()
    assert tr.shape == (MAXIT, R, 5 + 2 * ND)
    for r in range(R):
        n = int(iters[r])
        assert 1 <= n <= MAXIT and not tr[n:, r].any()
        L, lr, zt, g = tr[:n, r, 0], tr[:n, r, 4], tr[:n, r, 5:5 + ND], tr[:n, r, 5 + ND:]
        rep = editing.noise_opt_replay(L, g, z0[r].numpy())
        assert rep["n"] == n and np.array_equal(rep["lr"].astype(np.float32), lr.astype(np.float32)), (r, n, rep["n"])
        assert [k for k in rep["reduced_at"] if k < n - 1] == [k for k in range(n - 1) if lr[k + 1] != lr[k]]
        assert rep["stopped_at"] == n - 1 if n < MAXIT else rep["stopped_at"] in (None, MAXIT - 1)
        zall = np.concatenate([zt, zend[r][None].astype(np.float64)])
        bound = np.arange(n + 1) * 8 * 2.0 ** -24 * max(1.0, np.abs(zall).max())
        dev = np.abs(zall - rep["z"]).max(1)
        print(f"LATCFG {tag} noise_opt row {r}: {n} iterations, L {L[0]:.3f} -> {L[-1]:.5f}, worst z deviation / bound = {np.max(dev[1:] / bound[1:]):.3f}")
        assert np.all(dev <= bound), (r, int(np.argmax(dev - bound)))
        assert L[-1] < L[0]
    m2, l2 = ls.part_aligner(code, valid, out["z"])
    assert float((m2 - out["mean"]).abs().max()) < OUT_TOL and float((l2 - out["logvar"]).abs().max()) < OUT_TOL
    m0, l0 = ls.part_aligner(code, valid, z0)
    first = editing.noise_losses(prob, m0.double(), l0.double(), z0.cuda().double())
    for i, k in enumerate(("L", "fit", "edit", "reg")):
        assert np.allclose(first[k].cpu().numpy(), tr[0, :, i], rtol=1e-4, atol=1e-5), k
