"""PointNetV2 part encoder in train mode on the HIP path (encoder side): batch-statistics BatchNorm forward,
running-statistics update, and the backward, against the reference class's own autograd (golden) and the torch-CPU oracle.

Tolerances (fp32; the batch statistics and the column reductions sum in a different order than torch): outputs 2e-5 max-abs,
running statistics 1e-5, gradients 1e-3 of each tensor's max-abs (BatchNorm over B = 5 samples in the heads amplifies
rounding: 1 / sqrt(var + eps) of five numbers).
The same kernels against float64 on the branch they took, with the fp32 oracle's own error as yardstick: tests/test_gpu_encoder_train_highprec.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
# a bias in front of a train-mode BatchNorm has a mathematically ZERO gradient (the batch mean removes it): what torch and the
# kernels return for these is rounding noise of the reductions (1e-4), compared in absolute terms only
ZERO_GRAD = {f"conv{i}.bias" for i in (1, 2, 3, 4)} | {f"{h}.{i}.bias" for h in ("mlp_m", "mlp_v") for i in (0, 3)}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(W, x, attn, dm, dv, precision="f32", momentum=0.1):
    from difffacto_amd import training
    P = {n: torch.from_numpy(W[n].copy()).cuda().requires_grad_(True) for n in training.PNV2_PARAMS}
    Bf = {n: torch.from_numpy(W[n].copy()).cuda() for n in training.PNV2_BUFFERS}
    m, v = training.pointnet_v2_train_forward(P, Bf, torch.from_numpy(x).cuda(), torch.from_numpy(attn).cuda(), momentum=momentum,
                                              precision=precision)
    ((m * torch.from_numpy(dm).cuda()).sum() + (v * torch.from_numpy(dv).cuda()).sum()).backward()
    torch.cuda.synchronize()
    return dict(m=m.detach().cpu().numpy(), v=v.detach().cpu().numpy(), running={n: b.cpu().numpy() for n, b in Bf.items()},
                grads={n: p.grad.cpu().numpy() for n, p in P.items()})


def test_train_mode_vs_reference_autograd_golden():
    from difffacto_amd import synth
    g = dict(np.load(os.path.join(GOLD, "pointnet_v2_train_B5_N160.npz")))
    W = synth.make_pointnet_v2_weights(int(g["weight_seed"]))
    r = _run(W, g["x"], g["attn"], g["dm"], g["dv"])
    assert np.abs(r["m"] - g["m"]).max() < 2e-5 and np.abs(r["v"] - g["v"]).max() < 2e-5
    n = 0
    worst = 0.0
    for key in g:
        if key.startswith("r/"):
            assert np.abs(r["running"][key[2:]] - g[key]).max() < 1e-5, key
        elif key.startswith("g/") or key.startswith("gs/"):
            name = key.split("/", 1)[1]
            got = r["grads"][name].astype(np.float64).ravel()
            ref = g[key].astype(np.float64)
            if key.startswith("gs/"):
                l2 = g["gn/" + name][1]
                assert abs(np.sqrt((got ** 2).sum()) - l2) <= 1e-3 * l2 + 1e-7, (name, "L2")
                got = got[g["gi/" + name]]
            n += 1
            if name in ZERO_GRAD:
                assert np.abs(got).max() < 5e-3 and np.abs(ref).max() < 5e-3, name
                continue
            scale = max(np.abs(ref).max(), 1e-30)
            err = np.abs(got - ref).max()
            assert err <= 1e-3 * scale + 1e-7, (name, err, scale)
            worst = max(worst, err / scale)
    assert n == 36
    print(f"36 parameter gradients vs the reference's autograd: worst max-abs error / max-abs = {worst:.2e}")


@pytest.mark.parametrize("B,N,precision,tol", [(4, 333, "f32", 1e-3), (8, 1024, "f32", 1e-3)])
def test_train_mode_vs_oracle_full_gradients(B, N, precision, tol):
    from difffacto_amd import synth
    from oracle import pointnet_v2_train as pt
    rng = np.random.Generator(np.random.PCG64(B * 1000 + N))
    W = synth.make_pointnet_v2_weights(2)
    x = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    seg = rng.integers(0, 4, size=(B, N))
    seg[0][seg[0] == 2] = 1                                    # shape 0 lacks part 2
    attn = np.eye(4, dtype=np.float32)[seg]
    dm, dv = rng.standard_normal((B, 4, 256)).astype(np.float32), rng.standard_normal((B, 4, 256)).astype(np.float32)
    ref = pt.outputs_and_grads(W, x, attn, dm, dv)
    r = _run(W, x, attn, dm, dv, precision=precision)
    otol = 2e-5 if precision == "f32" else 5e-2
    assert np.abs(r["m"] - ref["m"]).max() < otol * max(1.0, np.abs(ref["m"]).max())
    assert np.abs(r["v"] - ref["v"]).max() < otol * max(1.0, np.abs(ref["v"]).max())
    for k, a in ref["running"].items():
        assert np.abs(r["running"][k] - a).max() < (1e-5 if precision == "f32" else 3e-2), k
    worst = 0.0
    for k, gr in ref["grads"].items():
        if k in ZERO_GRAD:
            assert np.abs(r["grads"][k]).max() < (5e-3 if precision == "f32" else 5e-2), k
            continue
        scale = max(np.abs(gr).max(), 1e-30)
        err = np.abs(r["grads"][k] - gr).max()
        assert err <= tol * scale + 1e-7, (k, err, scale)
        worst = max(worst, err / scale)
    print(f"B={B} N={N} {precision}: worst gradient error / max-abs = {worst:.2e}")


@pytest.mark.parametrize("B,N", [(8, 2048), (9, 1000), (5, 2048)])
def test_batch_statistics_from_the_product_epilogue_match_the_two_pass_ones(B, N):
    """From 8192 rows on the fp32 trunk's products leave (count, mean, M2) partials of their output columns in the epilogue and BatchNorm's
    batch statistics are merged from them (Chan's formula) instead of two passes over the layer's output (dfx_debug_bn_fused_stats).  Same
    function, different summation order: outputs, running statistics and gradients agree to fp32 rounding — also with a ragged last row tile
    (9000 rows) and with more workgroups than row tiles (10240 rows)."""
    from difffacto_amd import _ffi, synth
    rng = np.random.Generator(np.random.PCG64(B * 77 + N))
    W = synth.make_pointnet_v2_weights(4)
    x = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    attn = np.eye(4, dtype=np.float32)[rng.integers(0, 4, size=(B, N))]
    dm, dv = rng.standard_normal((B, 4, 256)).astype(np.float32), rng.standard_normal((B, 4, 256)).astype(np.float32)
    fused = _run(W, x, attn, dm, dv)
    _ffi.lib().dfx_debug_bn_fused_stats(0)
    try:
        two = _run(W, x, attn, dm, dv)
    finally:
        _ffi.lib().dfx_debug_bn_fused_stats(1)
    assert any(not np.array_equal(fused["running"][k], two["running"][k]) for k in two["running"]), "the epilogue statistics were not used"
    assert np.abs(fused["m"] - two["m"]).max() < 2e-5 * max(1.0, np.abs(two["m"]).max())
    assert np.abs(fused["v"] - two["v"]).max() < 2e-5 * max(1.0, np.abs(two["v"]).max())
    for k, a in two["running"].items():
        assert np.abs(fused["running"][k] - a).max() < 1e-6 * max(1.0, np.abs(a).max()), k
    # Gradients: a discontinuous function of the statistics' last bits — a max-pool arg-max or a ReLU unit at ~0 that falls the other way moves
    # whole entries (tools/experiments/ab_bn_stats.py against the CPU oracle: at 8 x 2048 the EPILOGUE path agrees with the oracle to 3.6e-5 of max-abs and the
    # two-pass path sits 1.2e-2 away on bn2.bias; at 16 x 1024 both sit 4.8e-2 away on one head bias and 1.3e-5 from each other).  Hence: relative
    # L2 per tensor as for the flows' known kink case, and most tensors to rounding.
    worst, close = 0.0, 0
    names = [k for k in two["grads"] if k not in ZERO_GRAD and k != "bn4.bias"]   # (bn4.bias: mathematically zero too — the heads' BatchNorm removes it)
    for k in names:
        gr = two["grads"][k]
        err = np.abs(fused["grads"][k] - gr).max() / max(np.abs(gr).max(), 1e-30)
        worst = max(worst, err)
        close += err <= 1e-3
        assert np.linalg.norm((fused["grads"][k] - gr).ravel()) <= 5e-2 * np.linalg.norm(gr.ravel()) + 1e-7, k
    assert close >= len(names) // 2, (close, len(names))
    print(f"B={B} N={N}: epilogue vs two-pass batch statistics: m max-abs {np.abs(fused['m'] - two['m']).max():.1e}, worst gradient error / max-abs {worst:.1e}")


def test_one_launch_batchnorm_of_the_heads_is_bit_identical_to_the_multi_launch_passes():
    """BatchNorm over few rows (the heads normalise over the B shapes) runs as one kernel per direction with the sums in the multi-launch path's
    order.  Below 8192 points the trunk takes the same kernels under both settings of dfx_debug_bn_fused_stats, so everything must be the same bits."""
    from difffacto_amd import _ffi, synth
    rng = np.random.Generator(np.random.PCG64(91))
    B, N = 7, 333
    W = synth.make_pointnet_v2_weights(6)
    x = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    attn = np.eye(4, dtype=np.float32)[rng.integers(0, 4, size=(B, N))]
    dm, dv = rng.standard_normal((B, 4, 256)).astype(np.float32), rng.standard_normal((B, 4, 256)).astype(np.float32)
    one = _run(W, x, attn, dm, dv)
    _ffi.lib().dfx_debug_bn_fused_stats(0)
    try:
        multi = _run(W, x, attn, dm, dv)
    finally:
        _ffi.lib().dfx_debug_bn_fused_stats(1)
    assert np.array_equal(one["m"], multi["m"]) and np.array_equal(one["v"], multi["v"])
    for k in multi["running"]:
        assert np.array_equal(one["running"][k], multi["running"][k]), k
    for k in multi["grads"]:
        assert np.array_equal(one["grads"][k], multi["grads"][k]), k


def test_bf16_products_run_and_stay_close():
    """precision="bf16" rounds the trunk's matrix-product operands to bf16.  Through four BatchNorm layers, a max-pool whose
    arg-max can flip under that noise, and BatchNorm over only B samples in the heads, outputs move by a few percent and
    gradients discontinuously: the drop-in module trains this encoder in fp32; here only closeness of the outputs and
    finiteness / rough agreement (cosine > 0.7 on the trunk weights) of the gradients are required."""
    from difffacto_amd import synth
    rng = np.random.Generator(np.random.PCG64(11))
    B, N = 16, 1024
    W = synth.make_pointnet_v2_weights(2)
    x = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    attn = np.eye(4, dtype=np.float32)[rng.integers(0, 4, size=(B, N))]
    dm, dv = rng.standard_normal((B, 4, 256)).astype(np.float32), rng.standard_normal((B, 4, 256)).astype(np.float32)
    f, b = _run(W, x, attn, dm, dv, precision="f32"), _run(W, x, attn, dm, dv, precision="bf16")
    assert np.abs(b["m"] - f["m"]).max() < 0.15 * np.abs(f["m"]).max() and np.abs(b["v"] - f["v"]).max() < 0.15 * np.abs(f["v"]).max()
    assert not np.array_equal(b["m"], f["m"])
    for k in ("conv2.weight", "conv3.weight", "conv4.weight"):
        gb, gf = b["grads"][k].ravel().astype(np.float64), f["grads"][k].ravel().astype(np.float64)
        assert np.isfinite(gb).all()
        assert gb @ gf / (np.linalg.norm(gb) * np.linalg.norm(gf)) > 0.7, k


def test_module_train_mode_is_native_and_matches_the_golden():
    """encoders.PointNetV2 in train(): forward / backward through libdfx, running statistics and num_batches_tracked updated."""
    from difffacto_amd import synth
    from difffacto_amd.encoders import PointNetV2
    g = dict(np.load(os.path.join(GOLD, "pointnet_v2_train_B5_N160.npz")))
    W = synth.make_pointnet_v2_weights(int(g["weight_seed"]))
    enc = PointNetV2(zdim=256, num_anchors=4, per_part_mlp=True)
    sd = enc.state_dict()
    for k, a in W.items():
        sd[k] = torch.from_numpy(a.copy())
    enc.load_state_dict(sd)
    enc = enc.cuda().train()
    m, v = enc(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["attn"]).cuda())
    assert m.grad_fn is not None and type(m.grad_fn).__name__.startswith("PointNetV2TrainFn")
    ((m * torch.from_numpy(g["dm"]).cuda()).sum() + (v * torch.from_numpy(g["dv"]).cuda()).sum()).backward()
    assert np.abs(m.detach().cpu().numpy() - g["m"]).max() < 2e-5
    assert int(enc.bn1.num_batches_tracked) == 1
    assert np.abs(enc.bn3.running_var.cpu().numpy() - g["r/bn3.running_var"]).max() < 1e-5
    gw = enc.conv4.weight.grad.cpu().numpy().ravel()
    ref = g["gs/conv4.weight"]
    assert np.abs(gw[g["gi/conv4.weight"]] - ref).max() <= 1e-3 * np.abs(ref).max()
    enc.eval()
    with torch.no_grad():      # the eval handle is rebuilt with the updated running statistics
        m2, _ = enc(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["attn"]).cuda())
    assert torch.isfinite(m2).all() and not torch.equal(m2, m.detach())


def _prior_run(W, part_code, logvar, valid, prior_var, kl):
    from difffacto_amd import training
    names = training.flow_param_names(14)
    P = {n: torch.from_numpy(W[n].copy()).cuda().requires_grad_(True) for n in names}
    z = torch.from_numpy(part_code).cuda().requires_grad_(True)
    lv = torch.from_numpy(logvar).cuda().requires_grad_(True)
    loss, log_p, ent = training.prior_loss(P, z, lv, torch.from_numpy(valid).cuda(), prior_var=prior_var, kl_weight=kl)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), log_p=log_p.cpu().numpy(), entropy=ent.cpu().numpy(), d_part_code=z.grad.cpu().numpy(),
                d_logvar=lv.grad.cpu().numpy(), grads={n: p.grad.cpu().numpy() for n, p in P.items()})


def test_prior_loss_vs_reference_autograd_golden():
    """Flows forward + log-det + log-likelihood + entropy and the backward against the reference's get_prior_loss + autograd:
    loss 1e-5 relative, d part_code / d logvar 2e-4, the 336 flow-parameter gradients 1e-3 of each tensor's max-abs."""
    from difffacto_amd import synth
    g = dict(np.load(os.path.join(GOLD, "prior_loss_B6.npz")))
    W = synth.make_latent_weights(int(g["weight_seed"]))
    r = _prior_run(W, g["part_code"], g["logvar"], g["valid"], float(g["prior_var"]), float(g["kl_weight"]))
    assert abs(r["loss"] - float(g["loss"])) < 1e-5 * abs(float(g["loss"]))
    for k in ("d_part_code", "d_logvar"):
        assert np.abs(r[k] - g[k]).max() <= 2e-4 * np.abs(g[k]).max() + 1e-12, k
    n, worst = 0, 0.0
    for key in g:
        if key.startswith("g/") or key.startswith("gs/"):
            name = key.split("/", 1)[1]
            got = r["grads"][name].astype(np.float64).ravel()
            ref = g[key].astype(np.float64)
            if key.startswith("gs/"):
                l2 = g["gn/" + name][1]
                assert abs(np.sqrt((got ** 2).sum()) - l2) <= 1e-3 * l2 + 1e-12, (name, "L2")
                got = got[g["gi/" + name]]
            scale = max(np.abs(ref).max(), 1e-30)
            err = np.abs(got - ref).max()
            assert err <= 1e-3 * scale + 1e-12, (name, err, scale)
            worst = max(worst, err / scale)
            n += 1
    assert n == 336
    print(f"336 flow-parameter gradients vs the reference's autograd: worst max-abs error / max-abs = {worst:.2e}")


@pytest.mark.parametrize("B,strict", [(32, True), (70, True), (37, False)])
def test_prior_loss_vs_oracle_other_batch(B, strict):
    """Against oracle/prior_loss.py on other batches (ragged part validity).  strict: every element of every gradient within 1e-3
    of its tensor's max-abs.  B = 37 is kept as the known kink case: one ReLU unit of one sample has a pre-activation of ~0
    and comes out on the other side under the kernels' fp32 summation order, so that sample's derivative differs by the
    unit's share (a property of the function, not of either implementation): relative L2 per tensor within 5e-2 there."""
    from difffacto_amd import synth
    from oracle import prior_loss as pl
    rng = np.random.Generator(np.random.PCG64(3))
    W = synth.make_latent_weights(1)
    z = rng.standard_normal((B, 256, 4)).astype(np.float32)
    lv = (-2.0 + 0.5 * rng.standard_normal((B, 4, 256))).astype(np.float32)
    _, _, _, valid = synth.make_latents(B, seed=5)
    ref = pl.loss_and_grads(W, z, lv, valid, prior_var=1.0, kl_weight=5e-4)
    r = _prior_run(W, z, lv, valid, 1.0, 5e-4)
    assert abs(r["loss"] - ref["loss"]) < 1e-5 * abs(ref["loss"])
    assert np.abs(r["log_p"] - ref["log_p"]).max() < 1e-5 * np.abs(ref["log_p"]).max()
    assert np.abs(r["entropy"] - ref["entropy"]).max() < 1e-5 * np.abs(ref["entropy"]).max()
    assert np.abs(r["d_logvar"] - ref["d_logvar"]).max() <= 1e-5 * np.abs(ref["d_logvar"]).max()
    pairs = [("d_part_code", r["d_part_code"], ref["d_part_code"])] + [(k, r["grads"][k], gr) for k, gr in ref["grads"].items()]
    for name, a, b in pairs:
        if strict:
            assert np.abs(a - b).max() <= 1e-3 * max(np.abs(b).max(), 1e-30) + 1e-12, name
        else:
            assert np.linalg.norm((a - b).ravel()) <= 5e-2 * max(np.linalg.norm(b.ravel()), 1e-30), name


def test_stage1_training_step_against_composed_oracles():
    """The whole stage-1 training forward + backward through the drop-in modules (encoder.forward -> training_losses, as
    anchor_gen.py:970-1020 strings them together) against the same composition of the torch-CPU oracles with the
    reparameterisation noise replayed: loss values and gradients of PointNetV2, the flows and the denoiser."""
    from difffacto_amd import synth, training
    from difffacto_amd.encoders import PartEncoderForTransformerDecoder
    from difffacto_amd.modules import AnchoredDiffusion
    from oracle import pointnet_v2_train as pt, prior_loss as pl, torch_cpu, train as otrain
    from test_modules_cpu import DIFF_CFG
    B, N, T = 6, 256, 100
    rng = np.random.Generator(np.random.PCG64(21))
    W_pn, W_lat, W_dn = synth.make_pointnet_v2_weights(0), synth.make_latent_weights(0), synth.make_denoiser_weights(0)
    _, gt_shift, lvv, valid = synth.make_latents(B, seed=2)
    gt_std = np.exp(0.5 * lvv).astype(np.float32)                       # 'part_scale' is a std: squared by the encoder
    seg = synth.make_seg_mask(valid, N)
    ref = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    attn = np.eye(4, dtype=np.float32)[seg]
    eps = rng.standard_normal((B, 4, 256)).astype(np.float32)
    noise = rng.standard_normal((B, 3, N)).astype(np.float32)
    t = rng.integers(0, T, size=(B,)).astype(np.int64)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc = PartEncoderForTransformerDecoder(encoder=dict(type="PointNetV2", zdim=256, per_part_mlp=True), n_class=4, part_aligner=None,
                                           include_z=False, include_part_code=True, include_params=True, use_gt_params=True, kl_weight=5e-4,
                                           use_flow=True, gen=True, prior_var=1.0)
    sd = enc.state_dict()
    for k, a in W_pn.items():
        sd["encoder." + k] = torch.from_numpy(a.copy())
    for k, a in W_lat.items():
        if k.startswith("flow."):
            sd[k] = torch.from_numpy(a.copy())
    enc.load_state_dict(sd)
    diff = AnchoredDiffusion(num_timesteps=T, precision="f32", **{**DIFF_CFG, "net": dict(DIFF_CFG["net"], dropout=0.0)})
    diff.model.load_state_dict({k: torch.from_numpy(v) for k, v in W_dn.items()})
    enc, diff = enc.cuda().train(), diff.cuda().train()
    pcds = {"input": cu(ref), "ref": cu(ref), "present": cu(valid), "dp_present": cu(valid), "ref_seg_mask": cu(seg.astype(np.int64)),
            "ref_attn_map": cu(attn), "part_shift": cu(gt_shift), "part_scale": cu(gt_std), "noise": torch.zeros(B, 32).cuda()}
    real_randn = torch.randn
    try:
        torch.randn = lambda *a, **k: cu(eps)                     # the reparameterisation draw (misc.py:282-285)
        losses = training.stage1_losses(enc, diff, pcds, t=cu(t), noise=cu(noise))
    finally:
        torch.randn = real_randn
    total = losses["prior_loss"] + losses["fit_loss"].sum() + losses["mse_loss"]
    total.backward()
    torch.cuda.synchronize()
    # ---- the same composition on the CPU oracles ----
    Wp = {k: torch.from_numpy(a.copy()) for k, a in W_pn.items()}
    for k, v in Wp.items():
        if "running" not in k:
            v.requires_grad_(True)
    Wf = {k: torch.from_numpy(a.copy()).requires_grad_(True) for k, a in W_lat.items() if k.startswith("flow.")}
    Wd = {k: torch.from_numpy(a.copy()).requires_grad_(True) for k, a in W_dn.items()}
    m, lv = pt.forward(Wp, torch.from_numpy(ref), torch.from_numpy(attn))
    part_code = (m + torch.exp(0.5 * lv) * torch.from_numpy(eps)).transpose(1, 2)
    prior, _, _ = pl.prior_loss(Wf, part_code, lv, torch.from_numpy(valid), prior_var=1.0, kl_weight=5e-4)
    mean_t, gt_var = torch.from_numpy(gt_shift), torch.from_numpy(gt_std) ** 2
    idx = torch.from_numpy(seg.astype(np.int64))[:, None, :].expand(-1, 3, -1)
    anc_pp, var_pp = torch.gather(mean_t, 2, idx), torch.gather(gt_var, 2, idx)
    flags = torch.gather(torch.from_numpy(valid)[:, None, :], 2, torch.from_numpy(seg.astype(np.int64))[:, None, :])
    sa = torch.from_numpy(diff.sqrt_alphas_cumprod).float()[torch.from_numpy(t)].view(-1, 1, 1)
    s1 = torch.from_numpy(diff.sqrt_one_minus_alphas_cumprod).float()[torch.from_numpy(t)].view(-1, 1, 1)
    x0 = torch.from_numpy(ref).transpose(1, 2)
    x_t = sa * (x0 - anc_pp) + anc_pp + s1 * torch.sqrt(var_pp) * torch.from_numpy(noise)
    eps_hat = torch_cpu.transformer_net_forward(Wd, x_t, torch.from_numpy(t), [part_code, torch.cat([mean_t, gt_var], 1)],
                                                anc_pp.transpose(1, 2), var_pp.transpose(1, 2), torch.from_numpy(valid), torch.from_numpy(seg))
    mse = otrain.masked_mse(torch.from_numpy(noise), eps_hat, flags)
    (prior + mse).backward()
    assert abs(float(losses["prior_loss"].detach()) - float(prior.detach())) < 1e-5 * abs(float(prior.detach()))
    assert abs(float(losses["mse_loss"].detach()) - float(mse.detach())) < 2e-5 * abs(float(mse.detach()))
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))
    worst = {}
    for name, p in enc.encoder.named_parameters():
        if name in ZERO_GRAD:
            continue
        worst["pn"] = max(worst.get("pn", 0.0), rel(p.grad.cpu().numpy(), Wp[name].grad.numpy()))
    for name, p in enc.named_parameters():
        if name.startswith("flow."):
            worst["flow"] = max(worst.get("flow", 0.0), rel(p.grad.cpu().numpy(), Wf[name].grad.numpy()))
    for name, p in diff.model.named_parameters():
        worst["denoiser"] = max(worst.get("denoiser", 0.0), rel(p.grad.cpu().numpy(), Wd[name].grad.numpy()))
    print("stage-1 step, worst relative L2 gradient error per group:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert worst["pn"] < 2e-3 and worst["flow"] < 2e-3 and worst["denoiser"] < 2e-3, worst


def test_stage1_prior_branch_on_a_second_stream_is_bit_identical():
    """stage1_losses(overlap_prior=True) runs the prior loss (flows) on a second stream beside the denoiser, forward and
    backward.  Same kernels, same order within each branch: every loss entry and every parameter gradient must equal the
    single-stream run bit for bit, repeatedly (a missing stream dependency would show up as a mismatch or a NaN), and an
    optimiser step taken right after backward() must see the finished gradients."""
    from difffacto_amd import synth, training
    from difffacto_amd.encoders import PartEncoderForTransformerDecoder
    from difffacto_amd.modules import AnchoredDiffusion
    from test_modules_cpu import DIFF_CFG
    B, N, T = 48, 1024, 100
    rng = np.random.Generator(np.random.PCG64(5))
    W_pn, W_lat, W_dn = synth.make_pointnet_v2_weights(0), synth.make_latent_weights(0), synth.make_denoiser_weights(0)
    _, gt_shift, lvv, valid = synth.make_latents(B, seed=3)
    seg = synth.make_seg_mask(valid, N)
    ref = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pcds = {"input": cu(ref), "ref": cu(ref), "present": cu(valid), "dp_present": cu(valid), "ref_seg_mask": cu(seg.astype(np.int64)),
            "ref_attn_map": cu(np.eye(4, dtype=np.float32)[seg]), "part_shift": cu(gt_shift), "part_scale": cu(np.exp(0.5 * lvv).astype(np.float32)),
            "noise": torch.zeros(B, 32).cuda()}
    t, noise = cu(rng.integers(0, T, size=(B,)).astype(np.int64)), cu(rng.standard_normal((B, 3, N)).astype(np.float32))

    def build():
        enc = PartEncoderForTransformerDecoder(encoder=dict(type="PointNetV2", zdim=256, per_part_mlp=True), n_class=4, part_aligner=None,
                                               include_z=False, include_part_code=True, include_params=True, use_gt_params=True,
                                               kl_weight=5e-4, use_flow=True, gen=True, prior_var=1.0)
        sd = enc.state_dict()
        sd.update({"encoder." + k: torch.from_numpy(a.copy()) for k, a in W_pn.items()})
        sd.update({k: torch.from_numpy(a.copy()) for k, a in W_lat.items() if k.startswith("flow.")})
        enc.load_state_dict(sd)
        diff = AnchoredDiffusion(num_timesteps=T, precision="f32", **{**DIFF_CFG, "net": dict(DIFF_CFG["net"], dropout=0.0)})
        diff.model.load_state_dict({k: torch.from_numpy(v) for k, v in W_dn.items()})
        return enc.cuda().train(), diff.cuda().train()

    def step(overlap, iters):
        enc, diff = build()
        params = [p for p in list(enc.parameters()) + list(diff.parameters()) if p.requires_grad]
        opt = training.Adam(params, lr=1e-3, max_norm=10.0)
        outs = []
        for _ in range(iters):
            opt.zero_grad()
            g = torch.Generator(device="cuda").manual_seed(11)
            real = torch.randn
            try:
                torch.randn = lambda *a, **k: real(*a, generator=g, **{kk: v for kk, v in k.items() if kk != "generator"})
                losses = training.stage1_losses(enc, diff, pcds, t=t, noise=noise, overlap_prior=overlap)
            finally:
                torch.randn = real
            (losses["prior_loss"] + losses["fit_loss"].sum() + losses["mse_loss"]).backward()
            grads = [None if p.grad is None else p.grad.clone() for p in params]
            opt.step()                                      # reads the gradients on the main stream, no synchronize in between
            outs.append((losses["prior_loss"].detach().clone(), losses["mse_loss"].detach().clone(), grads, [p.detach().clone() for p in params]))
        torch.cuda.synchronize()
        return outs

    serial, over = step(False, 3), step(True, 3)
    for (pa, ma, ga, wa), (pb, mb, gb, wb) in zip(serial, over):
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and bool(torch.isfinite(pb))
        for x, y in zip(ga, gb):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x, y)
        for x, y in zip(wa, wb):
            assert torch.equal(x, y)


# ---------------------------------------------------------------------------------- stage 2: the part aligner's training kernels
def test_part_aligner_training_kernels_vs_reference_autograd_golden():
    """aligner_train.hip (exact fp32) against torch autograd through the reference's PartAlignerTransformer (tests/golden/aligner_grads_B5.npz, shapes
    with one and two absent parts): outputs 1e-4, gradients of every parameter and of part_code 5e-4 of the tensor's max-abs; pre_norm.* gets no
    gradient in either (unused with cimle / cond_noise_type 0, part_encoders.py:119-131)."""
    from _train_case import check_against_golden
    from difffacto_amd import synth, training
    g = dict(np.load(os.path.join(GOLD, "aligner_grads_B5.npz")))
    W = {k[len("part_aligner."):]: v for k, v in synth.make_latent_weights(int(g["weight_seed"])).items() if k.startswith("part_aligner.")}
    P = {k: torch.from_numpy(v.copy()).cuda().requires_grad_(True) for k, v in W.items()}
    z = torch.from_numpy(g["part_code"]).cuda().requires_grad_(True)
    mean, logvar = training.aligner_train_forward(P, z, torch.from_numpy(g["valid"]).cuda(), torch.from_numpy(g["noise"]).cuda(), noise_scale=100.0)
    assert np.abs(mean.detach().cpu().numpy() - g["mean"]).max() < 1e-4 and np.abs(logvar.detach().cpu().numpy() - g["logvar"]).max() < 1e-4
    ((mean * torch.from_numpy(g["d_mean"]).cuda()).sum() + (logvar * torch.from_numpy(g["d_logvar"]).cuda()).sum()).backward()
    grads = {k: p.grad.cpu().numpy() for k, p in P.items() if p.grad is not None}
    assert set(P) - set(grads) == set(g["no_grad_params"].tolist()) == {"pre_norm.weight", "pre_norm.bias"}
    n, worst = check_against_golden(g, grads, rtol=5e-4, atol=1e-7)
    assert n == len(grads) == 72, (n, len(grads))
    e = np.abs(z.grad.cpu().numpy() - g["d_part_code"]).max() / np.abs(g["d_part_code"]).max()
    print(f"part aligner training kernels vs reference autograd: {n} parameter gradients, worst {worst:.1e} of max-abs; d part_code {e:.1e}")
    assert e < 5e-4
    # the inference kernels of the latent sampler compute the same forward
    from difffacto_amd.latents import LatentSampler
    ls = LatentSampler(synth.make_latent_weights(int(g["weight_seed"])), noise_scale=100.0)
    m2, lv2 = ls.part_aligner(z.detach(), torch.from_numpy(g["valid"]).cuda(), torch.from_numpy(g["noise"]).cuda())
    assert float((m2 - mean.detach()).abs().max()) < 1e-4 and float((lv2 - logvar.detach()).abs().max()) < 1e-4


def test_stage2_training_step_matches_the_reference():
    """tests/golden/stage2_step_B4_N64_T10.npz: ONE stage-2 training forward + backward of the reference's AnchorDiffAE (train() mode, gen_chair
    configuration with the part aligner and fit_loss_type 4, Dropout 0; anchor_gen.py:970-1021, runner.py:310-312).  The mirror (networks.AnchorDiffAE,
    fp32 kernels) with the same numpy seed for the timestep sampler and the recorded torch draws replayed: every entry of the loss dict, the total,
    the BatchNorm running statistics PointNetV2 leaves behind, and d total / d (every parameter of the part aligner) — what stage 2 optimises."""
    from _replay import replay_draws
    from _train_case import check_against_golden
    from difffacto_amd import synth
    from difffacto_amd.networks import AnchorDiffAE
    from test_modules_cpu import model_cfg
    g = dict(np.load(os.path.join(GOLD, "stage2_step_B4_N64_T10.npz")))
    batch = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("in/")}
    draws = [g[f"draw_{i}"] for i in range(int(g["n_draws"]))]
    T, N = 10, batch["ref"].shape[1]
    m = AnchorDiffAE(**model_cfg(num_timesteps=T, npoints=N, net=dict(dropout=0.0)), precision="f32")   # cfg.model of gen_chair.py (pinned on CPU), Dropout 0
    W = {"diffusion.model." + k: v for k, v in synth.make_denoiser_weights(0).items()}
    W.update({"encoder." + k: v for k, v in synth.make_latent_weights(0).items()})
    W.update({"encoder.encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    m = m.cuda().train()
    np.random.seed(int(g["np_seed"]))
    with replay_draws(draws) as queue:
        losses = m(batch, device="cuda", epoch=int(g["epoch"]))
    assert not queue
    total = sum(v.mean() for k, v in losses.items() if "loss" in k)          # parse_losses (utils/misc.py:120-132)
    total.backward()
    for k in [k for k in g if k.startswith("loss/")]:
        ref, got = g[k], losses[k[5:]].detach().cpu().numpy().reshape(g[k].shape)
        assert np.abs(got - ref).max() <= 2e-4 * max(1.0, np.abs(ref).max()), (k, got, ref)
    assert abs(float(total.detach()) - float(g["total"])) <= 2e-4 * abs(float(g["total"]))
    bn = m.encoder.encoder.state_dict()
    for k in [k for k in g if k.startswith("bn/")]:
        assert np.abs(bn[k[3:]].cpu().numpy() - g[k]).max() <= 1e-5 * max(1.0, np.abs(g[k]).max()), k
    grads = {k: p.grad.cpu().numpy() for k, p in m.encoder.part_aligner.named_parameters() if p.grad is not None}
    n, worst = check_against_golden(g, grads, rtol=2e-3, atol=1e-7)
    assert n == 72
    print(f"stage-2 step vs reference: total {float(total.detach()):.6f} / {float(g['total']):.6f}, {n} aligner gradients, worst {worst:.1e} of max-abs")
    # ... and the optimiser of stage 2 (runner.py:88: encoder.part_aligner.parameters()) moves exactly those
    from difffacto_amd import training
    before = m.encoder.part_aligner.proj_out.weight.detach().clone()
    training.Adam(list(m.encoder.part_aligner.parameters()), lr=2e-3, max_norm=10.0).step()
    assert not torch.equal(before, m.encoder.part_aligner.proj_out.weight.detach())
