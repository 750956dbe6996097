"""Part re-configuration editing on the GPU: the aligner's noise gradient (dfx_aligner_input_backward through training.AlignerTrainFn),
the on-device noise optimizer (dfx_noise_opt_run) and the Python layer on top (networks.AnchorDiffAE.edit_latent / optimize_latent /
cimle_forward, editing.reconfigure_part / invert_noise), against the reference's goldens under tests/golden/noiseopt/
(make_golden_noiseopt.py), torch autograd through a restatement of the aligner that is itself checked against oracle/latents.py, and the
float64 host restatement of the optimizer rules (editing.noise_opt_replay)."""
import os

import numpy as np
import pytest
import torch

from difffacto_amd import synth
from _latent_cfg import _aligner_torch
from _replay import replay_draws

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "noiseopt")
OUT_TOL, G_RTOL, G_ATOL = 1e-4, 5e-4, 1e-7      # the gates of test_part_aligner_training_kernels_vs_reference_autograd_golden


def _model(T=10, N=64, K=1, precision="f32", **flags):
    from difffacto_amd.networks import AnchorDiffAE
    from test_modules_cpu import model_cfg
    m = AnchorDiffAE(**model_cfg(num_timesteps=T, npoints=N, cimle_sample_num=K, **flags), precision=precision)
    W = {"diffusion.model." + k: v for k, v in synth.make_denoiser_weights(0).items()}
    W.update({"encoder." + k: v for k, v in synth.make_latent_weights(0).items()})
    W.update({"encoder.encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.cuda().eval().requires_grad_(False)


@pytest.fixture(scope="module")
def model():
    return _model()


def _parse_losses(losses):
    """utils/misc.py:120-132."""
    parsed = {k: v.mean() for k, v in losses.items()}
    return sum(v for k, v in parsed.items() if "loss" in k), parsed


def _grad_close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    print(f"{what}: max err {err:.2e}, {err / scale:.2e} of max-abs {scale:.2e}")
    assert err <= G_ATOL + G_RTOL * scale, (what, err, scale)


def _aligner_params(seed=0, grad=False):
    W = {k[len("part_aligner."):]: v for k, v in synth.make_latent_weights(seed).items() if k.startswith("part_aligner.")}
    return {k: torch.from_numpy(v.copy()).cuda().requires_grad_(grad) for k, v in W.items()}


def _aligner_case(B, seed, absent):
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(B, 256, 4, generator=g)
    valid = torch.ones(B, 4)
    for b, j in absent:
        valid[b, j] = 0
    noise = torch.randn(B, 32, generator=g)
    dm, dl = torch.randn(B, 3, 4, generator=g), torch.randn(B, 3, 4, generator=g)
    return [t.cuda() for t in (code, valid, noise, dm, dl)]


def _route(P, code, valid, noise, dm, dl, code_grad=True, noise_grad=True):
    from difffacto_amd import training
    for p in P.values():
        p.grad = None
    c, z = code.clone().requires_grad_(code_grad), noise.clone().requires_grad_(noise_grad)
    mean, logvar = training.aligner_train_forward(P, c, valid, z, noise_scale=100.0)
    ((mean * dm).sum() + (logvar * dl).sum()).backward()
    return mean.detach(), logvar.detach(), c.grad, z.grad, {k: p.grad.clone() for k, p in P.items() if p.grad is not None}


# ---------------------------------------------------------------------------------------------------- 1: the reference's goldens
@pytest.mark.parametrize("tag", ["edit_point_B1", "edit_point_B3"])
def test_edit_latent_loss_and_noise_gradient_match_the_reference(model, tag):
    """gate 1: AnchorDiffAE.edit_latent through the mirror (frozen weights, z a leaf) against the reference's loss dict and torch autograd's
    z.grad of parse_losses' total."""
    g = np.load(os.path.join(GOLD, f"{tag}.npz"))
    t = lambda k: torch.from_numpy(g[k]).cuda()
    model.noise_reg_loss, model.reg_loss_weight = bool(g["noise_reg_loss"]), float(g["reg_loss_weight"])
    z = torch.nn.Parameter(t("z"))
    seg_flag = torch.nn.functional.one_hot(t("in/seg_mask"), num_classes=4)
    losses = model.edit_latent(z, t("in/input"), seg_flag, t("in/present"), t("ref_means"), t("ref_vars"), t("fix_ids"), int(g["edit_id"]),
                               t("edit_part_mean") if "edit_part_mean" in g.files else None,
                               t("edit_part_var") if "edit_part_var" in g.files else None, fit_weight=float(g["fit_weight"]))
    assert set(losses) == {k[5:] for k in g.files if k.startswith("loss/")}
    for k, v in losses.items():
        ref = g["loss/" + k]
        assert tuple(v.shape) == ref.shape, (k, tuple(v.shape), ref.shape)
        err = float(np.abs(v.detach().cpu().numpy() - ref).max())
        print(f"{tag} {k}: {ref.ravel()[:3]} err {err:.2e}")
        assert err < OUT_TOL, (k, err)
    total, _ = _parse_losses(losses)
    assert abs(float(total.detach()) - float(g["total"])) < OUT_TOL
    total.backward()
    _grad_close(z.grad.cpu().numpy(), g["z_grad"], f"{tag} z.grad")


def test_optimize_latent_loss_and_noise_gradient_match_the_reference(model):
    """gate 1: optimize_latent goes through the whole encoder like the reference (the reparameterisation draw is replayed)."""
    g = np.load(os.path.join(GOLD, "optimize_point_B2.npz"))
    batch = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in/")}
    model.noise_reg_loss, model.reg_loss_weight = True, 1.0
    z = torch.nn.Parameter(torch.from_numpy(g["z"]).cuda())
    with replay_draws([g[f"draw_{i}"] for i in range(int(g["n_draws"]))]) as queue:
        losses = model.optimize_latent(batch, z, device="cuda")
    assert not queue
    assert set(losses) == {k[5:] for k in g.files if k.startswith("loss/")}
    for k, v in losses.items():
        ref = g["loss/" + k]
        assert tuple(v.shape) == ref.shape, (k, tuple(v.shape), ref.shape)
        err = float(np.abs(v.detach().cpu().numpy() - ref).max())
        print(f"optimize_point_B2 {k}: err {err:.2e} (|ref| {np.abs(ref).max():.2e})")
        # the terms that depend on z: the aligner's gate.  The prior terms (flows over PointNetV2's part codes, independent of z, up to 1e3 in
        # size) have their own kernel tests (test_gpu_encoder_train.py: 1e-5 relative on given codes); here 1e-3 relative, the widest end-to-end
        # fp32 gate of the suite (test_train_mode_vs_oracle_full_gradients), since the codes come through the native encoder
        assert err < (OUT_TOL if k in ("fit_loss", "reg_loss") else 1e-3 * max(1.0, float(np.abs(ref).max()))), (k, err)
    total, _ = _parse_losses({k: v for k, v in losses.items() if isinstance(v, torch.Tensor)})
    total.backward()
    _grad_close(z.grad.cpu().numpy(), g["z_grad"], "optimize_point_B2 z.grad")


# ---------------------------------------------------------------------------------------------------- 2, 4: the two autograd routes
@pytest.mark.parametrize("B", [1, 5, 64])
def test_input_backward_has_the_bits_of_the_training_backward(B):
    """gate 2: d_part_code of dfx_aligner_input_backward (frozen weights) equals the one dfx_aligner_train_backward writes (weights requiring a
    gradient) bit for bit, and d_noise is the same bits on both routes; one absent part."""
    case = _aligner_case(B, 40 + B, [(B // 2, 2)])
    frozen = _route(_aligner_params(grad=False), *case)
    train = _route(_aligner_params(grad=True), *case)
    assert not frozen[4] and len(train[4]) == 72
    assert torch.equal(frozen[0], train[0]) and torch.equal(frozen[1], train[1])
    assert frozen[2] is not None and torch.equal(frozen[2], train[2]), "d_part_code"
    assert frozen[3] is not None and torch.equal(frozen[3], train[3]), "d_noise"
    assert bool(torch.isfinite(frozen[3]).all()) and float(frozen[3].abs().max()) > 0
    # noise alone (the optimizer's case): the same d_noise bits without d_part_code
    alone = _route(_aligner_params(grad=False), *case, code_grad=False)
    assert alone[2] is None and torch.equal(alone[3], frozen[3])


def test_callers_without_a_noise_gradient_keep_their_launches_and_bits(monkeypatch):
    """gate 4: with noise that does not require a gradient the training route makes the calls it made before (one dfx_aligner_train_backward, no
    dfx_aligner_input_backward) and gives the bits of the route that also asks for d_noise (whose extra pass only adds d_noise)."""
    from difffacto_amd import _ffi
    lib, calls = _ffi.lib(), []
    for name in ("dfx_aligner_train_backward", "dfx_aligner_input_backward"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(real, name))
    case = _aligner_case(5, 77, [(1, 3)])
    P = _aligner_params(grad=True)
    plain = _route(P, *case, noise_grad=False)
    assert calls == ["dfx_aligner_train_backward"] and plain[3] is None
    del calls[:]
    both = _route(P, *case, noise_grad=True)
    assert calls == ["dfx_aligner_train_backward", "dfx_aligner_input_backward"]
    assert torch.equal(plain[0], both[0]) and torch.equal(plain[1], both[1]) and torch.equal(plain[2], both[2])
    assert set(plain[4]) == set(both[4]) and all(torch.equal(plain[4][k], both[4][k]) for k in plain[4])
    del calls[:]
    frozen = _route(_aligner_params(grad=False), *case, noise_grad=False)       # part_code alone, frozen weights: the data chain only
    assert calls == ["dfx_aligner_input_backward"] and torch.equal(frozen[2], plain[2])


# ---------------------------------------------------------------------------------------------------- 3: torch autograd through a restatement
@pytest.mark.parametrize("B,seed,absent", [(2, 5, [(0, 1)]), (7, 6, [(2, 0), (4, 3), (4, 2)])])
def test_noise_gradient_vs_torch_autograd_through_the_oracle(B, seed, absent):
    """gate 3: shapes and weights the goldens do not cover.  The torch restatement is first held to oracle/latents.py's forward."""
    from oracle import latents as ol
    Wn = synth.make_latent_weights(seed)
    code, valid, noise, dm, dl = _aligner_case(B, 100 + seed, absent)
    W64 = {k: torch.from_numpy(v).double() for k, v in Wn.items()}
    z64 = noise.cpu().double().requires_grad_(True)
    c64 = code.cpu().double().requires_grad_(True)
    m64, l64 = _aligner_torch(W64, c64, valid.cpu().double(), z64)
    mo, lo = ol.part_aligner_forward(Wn, code.cpu().numpy(), valid.cpu().numpy(), noise.cpu().numpy(), noise_scale=100.0)
    assert np.abs(m64.detach().numpy() - mo).max() < OUT_TOL and np.abs(l64.detach().numpy() - lo).max() < OUT_TOL
    ((m64 * dm.cpu().double()).sum() + (l64 * dl.cpu().double()).sum()).backward()
    P = {k[len("part_aligner."):]: torch.from_numpy(v.copy()).cuda() for k, v in Wn.items() if k.startswith("part_aligner.")}
    mean, logvar, dcode, dnoise, _ = _route(P, code, valid, noise, dm, dl)
    assert float((mean.cpu().double() - m64.detach()).abs().max()) < OUT_TOL and float((logvar.cpu().double() - l64.detach()).abs().max()) < OUT_TOL
    _grad_close(dnoise.cpu().numpy(), z64.grad.numpy(), f"B={B} d_noise")
    _grad_close(dcode.cpu().numpy(), c64.grad.numpy(), f"B={B} d_part_code")


# ---------------------------------------------------------------------------------------------------- 5, 8: the optimizer itself
@pytest.fixture(scope="module")
def sampler():
    from difffacto_amd.latents import LatentSampler
    return LatentSampler(synth.make_latent_weights(0), noise_scale=100.0)


def _problems(R, seed):
    """R synthetic rows: part codes, masks (some absent parts), the shape's own parameters, an edit of part e = r % 4 or of the first present part."""
    from difffacto_amd import editing
    rng = np.random.Generator(np.random.PCG64(seed))
    code = rng.standard_normal((R, 256, 4)).astype(np.float32)
    valid = np.ones((R, 4), np.float32)
    for r in range(R):
        if r % 3 == 1:
            valid[r, (r // 3) % 4] = 0
    ref_mean = (rng.standard_normal((R, 3, 4)) * 0.3).astype(np.float32)
    ref_var = (rng.uniform(0.2, 0.6, size=(R, 3, 4)) ** 2).astype(np.float32)
    ep = np.array([next(j for j in ((r + k) % 4 for k in range(4)) if valid[r, j]) for r in range(R)])
    fix = np.ones((R, 4), np.float32)
    fix[np.arange(R), ep] = 0
    new_var = ref_var[np.arange(R), :, ep] * np.array([1.0, 1.0, 1.2], np.float32)
    new_mean = ref_mean[np.arange(R), :, ep] + np.array([0.15, 0.0, -0.1], np.float32)
    z0 = rng.standard_normal((R, 32)).astype(np.float32)
    prob = editing.noise_problem(valid, ref_mean, ref_var, fix, ep, new_mean=new_mean, new_var=new_var)
    return torch.from_numpy(code), torch.from_numpy(valid), torch.from_numpy(z0), prob


def _rows(prob, idx):
    return {k: (v[idx] if isinstance(v, torch.Tensor) else v) for k, v in prob.items()}


def test_trace_follows_the_float64_restatement_and_stopped_rows_freeze(sampler):
    """gate 5: editing.noise_opt_replay fed with the kernel's own traced losses and gradients: same learning rates, reductions and stop iteration;
    z within k * 8 * 2^-24 * max(1, max|z|); a row that stopped at iteration s has the bits of a run with max_iter = s + 1."""
    from difffacto_amd import editing
    R, MAXIT, ND = 6, 400, 32
    code, valid, z0, prob = _problems(R, 11)
    out = sampler.optimize_noise(code, valid, z0, prob, MAXIT, trace=True)
    tr, iters, zend = out["trace"].cpu().numpy().astype(np.float64), out["iters_done"].cpu().numpy(), out["z"].cpu().numpy()
    assert tr.shape == (MAXIT, R, 5 + 2 * ND)
    stopped_rows = []
    for r in range(R):
        n = int(iters[r])
        assert 1 <= n <= MAXIT
        assert not tr[n:, r].any(), "trace rows after the stop are zero"
        L, lr, zt, g = tr[:n, r, 0], tr[:n, r, 4], tr[:n, r, 5:5 + ND], tr[:n, r, 5 + ND:]
        rep = editing.noise_opt_replay(L, g, z0[r].numpy())
        assert rep["n"] == n and np.array_equal(rep["lr"].astype(np.float32), lr.astype(np.float32)), (r, n, rep["n"])
        # a reduction shows in the trace as the next iteration's rate (one made by the last iteration's scheduler step is not traced)
        assert [k for k in rep["reduced_at"] if k < n - 1] == [k for k in range(n - 1) if lr[k + 1] != lr[k]]
        assert rep["stopped_at"] == n - 1 if n < MAXIT else rep["stopped_at"] in (None, MAXIT - 1)
        zall = np.concatenate([zt, zend[r][None].astype(np.float64)])
        bound = np.arange(n + 1) * 8 * 2.0 ** -24 * max(1.0, np.abs(zall).max())
        dev = np.abs(zall - rep["z"]).max(1)
        print(f"row {r}: {n} iterations, L {L[0]:.3f} -> {L[-1]:.5f}, lr {sorted(set(lr.tolist()), reverse=True)}, "
              f"worst z deviation / bound = {np.max(dev[1:] / bound[1:]):.3f}")
        assert np.all(dev <= bound), (r, int(np.argmax(dev - bound)))
        assert L[-1] < L[0]
        if n < MAXIT:
            stopped_rows.append((r, n))
    assert stopped_rows, "no row met the stop rule: the frozen-row check needs one"
    for r, n in stopped_rows[:2]:
        short = sampler.optimize_noise(code, valid, z0, prob, n)
        assert torch.equal(short["z"][r], out["z"][r]) and int(short["iters_done"][r]) == n
        assert torch.equal(short["mean"][r], out["mean"][r]) and torch.equal(short["logvar"][r], out["logvar"][r])
    # the returned (mean, logvar) are the aligner's at the returned z, and the loss restatement agrees with the kernel's traced terms
    m2, l2 = sampler.part_aligner(code, valid, out["z"])
    assert float((m2 - out["mean"]).abs().max()) < OUT_TOL and float((l2 - out["logvar"]).abs().max()) < OUT_TOL
    m0, l0 = sampler.part_aligner(code, valid, z0)
    first = editing.noise_losses(prob, m0.double(), l0.double(), z0.cuda().double())
    for i, k in enumerate(("L", "fit", "edit", "reg")):
        assert np.allclose(first[k].cpu().numpy(), tr[0, :, i], rtol=1e-4, atol=1e-5), k


def test_a_row_gives_the_same_bits_alone_and_inside_any_batch(sampler):
    """gate 8: rows are independent problems and no kernel's arithmetic depends on the row count."""
    MAXIT = 120
    code, valid, z0, prob = _problems(256, 21)
    big = sampler.optimize_noise(code, valid, z0, prob, MAXIT)
    again = sampler.optimize_noise(code, valid, z0, prob, MAXIT)
    for k in ("z", "mean", "logvar", "iters_done"):
        assert torch.equal(big[k], again[k]), k
    for row in (3, 100):
        alone = sampler.optimize_noise(code[row:row + 1], valid[row:row + 1], z0[row:row + 1], _rows(prob, slice(row, row + 1)), MAXIT)
        idx = torch.tensor([0, 7, row, 250, 31, 8, 9])
        seven = sampler.optimize_noise(code[idx], valid[idx], z0[idx], _rows(prob, idx), MAXIT)
        for k in ("z", "mean", "logvar", "iters_done"):
            assert torch.equal(alone[k][0], big[k][row]) and torch.equal(seven[k][2], big[k][row]), (row, k)
    assert bool(torch.isfinite(big["z"]).all())


# ---------------------------------------------------------------------------------------------------- 6, 7: the reference's trajectories
def _native_traj(model, g, pre):
    from difffacto_amd import editing
    t = lambda k: torch.from_numpy(g[pre + k])
    seg_flag = torch.nn.functional.one_hot(t("in/seg_mask"), num_classes=4).float()
    with torch.no_grad():
        code = model.encoder.get_part_code(t("in/input").cuda(), seg_flag.cuda())[0].transpose(1, 2).contiguous()
    tgt = {"new_mean": t("edit_part_mean")} if pre + "edit_part_mean" in g.files else {"new_var": t("edit_part_var")}
    prob = editing.noise_problem(t("in/present"), t("in/part_shift"), t("in/part_scale") ** 2, t("fix_ids"), int(g[pre + "edit_id"]),
                                 fit_weight=float(g["fit_weight"]), reg_weight=float(g["reg_loss_weight"]), **tgt)
    out = model.encoder.sampler().optimize_noise(code, t("in/present"), t("z0"), prob, int(g["max_iter"]), trace=True)
    n = int(out["iters_done"][0])
    return out["trace"][:n, 0].cpu().numpy().astype(np.float64), n


@pytest.mark.parametrize("p", [0, 1])
def test_trajectory_parity_with_the_reference_loop(model, p):
    """gates 6 and 7.  Over the first 40 iterations max|z_native_k - z64_k| <= 2 P_k + 1e-6, P_k = the running maximum of what a 5e-4 relative
    gradient perturbation (the gradient gate) does to the reference's own float64 trajectory, and the learning rates are the reference's; the native
    final L is below the initial one and at most (1 + m) times the larger reference final, m = max(0.05, twice the fp32 / fp64 reference gap)."""
    g = np.load(os.path.join(GOLD, "edit_traj.npz"))
    pre = f"p{p}/"
    tr, n = _native_traj(model, g, pre)
    z64, zp, lr64 = g[pre + "f64/z"], g[pre + "pert/z"], g[pre + "f64/lr"]
    K = 40
    assert n >= K and len(z64) >= K and len(zp) >= K
    P = np.maximum.accumulate(np.abs(zp[:K] - z64[:K]).max(1))
    dev = np.abs(tr[:K, 5:37] - z64[:K]).max(1)
    print(f"p{p}: native deviation from the fp64 reference over {K} iterations: max {dev.max():.2e}, P_{K} = {P[-1]:.2e}, max dev / P_{K} = "
          f"{dev.max() / P[-1]:.1e}, worst dev_k / (2 P_k + 1e-6) = {np.max(dev / (2 * P + 1e-6)):.3f}; the fp32 reference deviates by "
          f"{np.abs(g[pre + 'f32/z'][:K] - z64[:K]).max():.2e}")
    assert np.all(dev <= 2 * P + 1e-6), int(np.argmax(dev - 2 * P))
    assert np.array_equal(tr[:K, 4].astype(np.float32), lr64[:K].astype(np.float32))
    f32, f64 = float(g[pre + "f32/L"][-1]), float(g[pre + "f64/L"][-1])
    m = max(0.05, 2 * abs(f32 - f64) / min(f32, f64))
    print(f"p{p}: native {n} iterations, L {tr[0, 0]:.4f} -> {tr[-1, 0]:.5f}; reference fp32 {len(g[pre + 'f32/L'])} it. {f32:.5f}, fp64 {len(g[pre + 'f64/L'])} it. {f64:.5f}, m = {m:.3f}")
    assert abs(tr[0, 0] - float(g[pre + "f64/L"][0])) < 1e-3 * float(g[pre + "f64/L"][0])
    assert tr[-1, 0] < tr[0, 0] and tr[-1, 0] <= (1 + m) * max(f32, f64)


# ---------------------------------------------------------------------------------------------------- 9: the Python layer end to end
def test_reconfigure_part_is_one_optimizer_call_and_one_chain_launch(monkeypatch):
    from difffacto_amd import editing, engine, latents
    model = _model(10, 64, 1, "bf16")
    enc, diff = model.encoder, model.diffusion
    calls = {"opt": 0, "chain": 0}
    real_opt, real_chain = latents.LatentSampler.optimize_noise, engine.DenoiserEngine.sample_chain
    monkeypatch.setattr(latents.LatentSampler, "optimize_noise", lambda self, *a, **k: (calls.__setitem__("opt", calls["opt"] + 1), real_opt(self, *a, **k))[1])
    monkeypatch.setattr(engine.DenoiserEngine, "sample_chain", lambda self, *a, **k: (calls.__setitem__("chain", calls["chain"] + 1), real_chain(self, *a, **k))[1])
    gen = torch.Generator().manual_seed(9)
    S, E, T = 3, 2, 2                                                   # shapes x candidate edits x random starts
    codes = torch.randn(S, 256, 4, generator=gen).cuda()
    valid = torch.ones(S, 4)
    valid[1, 3] = 0
    ref_mean, ref_var = torch.randn(S, 3, 4, generator=gen) * 0.3, (torch.rand(S, 3, 4, generator=gen) * 0.4 + 0.2) ** 2
    shape_row = np.repeat(np.arange(S), E * T)
    scale = torch.tensor([[1.0, 1.0, 1.2], [1.3, 1.0, 1.0]]).repeat_interleave(T, 0).repeat(S, 1)          # (R, 3)
    new_var = ref_var[torch.as_tensor(shape_row), :, 0] * scale
    z0 = torch.randn(len(shape_row), 32, generator=gen)
    out = editing.reconfigure_part(enc, diff, codes, ref_mean, ref_var, 0, new_var=new_var, valid_id=valid, shape_row=shape_row, z0=z0,
                                   max_iter=150, npoints=64, seed=5)
    R = S * E * T
    assert calls == {"opt": 1, "chain": 1}
    assert out["pred"].shape == (R, 64, 3) and out["seg_mask"].shape == (R, 64) and out["z"].shape == (R, 32)
    assert out["mean"].shape == out["logvar"].shape == (R, 3, 4) and out["iters_done"].shape == (R,)
    assert bool(torch.isfinite(out["pred"]).all()) and all(out["losses"][k].shape == (R,) for k in ("L", "fit", "edit", "reg"))
    idx = torch.as_tensor(shape_row).cuda()
    m0, l0 = enc.sampler().part_aligner(codes[idx], valid.cuda()[idx], z0)
    target = torch.log(new_var).cuda()
    before, after = ((l0[..., 0] - target) ** 2).mean(1), ((out["logvar"][..., 0] - target) ** 2).mean(1)
    print("edited part, mse(logvar, target) at z0 -> at the optimized z:", before.cpu().numpy().round(3), after.cpu().numpy().round(4))
    assert bool((after < before).all())
    assert torch.allclose(after, out["losses"]["edit"], rtol=1e-4, atol=1e-6)
    with pytest.raises(ValueError):
        editing.reconfigure_part(enc, diff, codes, ref_mean, ref_var, 3, new_var=new_var, valid_id=valid, shape_row=shape_row, z0=z0, npoints=64)
    inv = editing.invert_noise(enc, codes, ref_mean, ref_var, valid_id=valid, max_iter=100)
    assert "pred" not in inv and inv["z"].shape == (S, 32) and bool((inv["losses"]["edit"] == 0).all())
    # cimle_forward decodes under given noises with the reference's keys (anchor_gen.py:837-870)
    g = np.load(os.path.join(GOLD, "edit_point_B3.npz"))
    batch = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in/")}
    K = 2
    pred = model.cimle_forward(batch, device="cuda", noise=torch.randn(3, K, 32, generator=gen).cuda())
    with torch.no_grad():
        ctx, mpp, lpp, _, _, _ = enc(batch, "cuda", noise=torch.zeros(3, 1, 32).cuda())
        dk = set(model.decode(mpp, ctx=ctx, variance=torch.exp(lpp), anchor_assignments=batch["ref_seg_mask"].cuda().to(torch.int32), valid_id=batch["present"].cuda()))
    want = {f"{k}_sample {i}" for k in dk for i in range(K)} | {f"sample prior {i}" for i in range(K)} | \
        {"pred", "input", "input_ref", "seg_mask", "pred_seg_mask", "ref_seg_mask", "shift", "scale"}
    assert set(pred) == want
    assert pred["pred"].shape == (3, 64, 3) and pred["pred_sample 1"].shape == (3, 64, 3) and pred["sample prior 0"].shape == (3, 64, 3)
    assert pred["pred_seg_mask"].shape == (3 * K, 64) and all(not v.is_cuda for v in pred.values())


# ---------------------------------------------------------------------------------------------------- timing: strictly less work
def test_input_backward_pair_is_not_slower_than_the_training_pair():
    """At B = 256 one [forward + dfx_aligner_input_backward] pair against one [forward + dfx_aligner_train_backward] pair, same process, HIP events,
    median of 20 after warm-up: the first launches a subset of the second's kernels."""
    from difffacto_amd import _ffi, training
    B, cfg = 256, (4, 256, 8, 32, 32, 100.0, 5)
    P = _aligner_params()
    names = training.aligner_param_names(5)
    ps = [P[n] for n in names]
    code, valid, noise, dm, dl = _aligner_case(B, 3, [(1, 2)])
    lib = _ffi.lib()
    nbytes = lib.dfx_aligner_train_workspace_bytes(B, 4, 256, 32, 8, 32, 5)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) & ~255
    mean, logvar = torch.empty(B, 3, 4, device="cuda"), torch.empty(B, 3, 4, device="cuda")
    dz, dn = torch.empty(B, 256, 4, device="cuda"), torch.empty(B, 32, device="cuda")
    views = training._flat_slices([p.shape for p in ps], "cuda")
    w, gs = training._aligner_struct(ps, cfg), training._aligner_struct(views, cfg)
    st = _ffi.current_stream()

    def fwd():
        _ffi.check(lib.dfx_aligner_train_forward(w, wp, nbytes, code.data_ptr(), valid.data_ptr(), noise.data_ptr(), mean.data_ptr(), logvar.data_ptr(), B, st), "fwd")

    def pair_input():
        fwd()
        _ffi.check(lib.dfx_aligner_input_backward(w, wp, nbytes, valid.data_ptr(), dm.data_ptr(), dl.data_ptr(), dn.data_ptr(), None, B, st), "input")

    def pair_train():
        fwd()
        _ffi.check(lib.dfx_aligner_train_backward(w, wp, nbytes, valid.data_ptr(), dm.data_ptr(), dl.data_ptr(), gs, dz.data_ptr(), B, st), "train")

    def median_ms(f, n=20, warm=5):
        for _ in range(warm):
            f()
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    t_train, t_input = median_ms(pair_train), median_ms(pair_input)
    print(f"B = {B}: forward + input backward {t_input:.3f} ms, forward + training backward {t_train:.3f} ms")
    assert t_input <= t_train
