"""No result may depend on what a workspace or an output buffer held before the call (include/dfx.h: "outputs are caller-allocated
and fully written by the call (no dependence on pre-zeroed outputs unless stated)").

Every case computes everything its entry point hands back or updates under the three allocation modes of tests/_dirty.py: `zero`
twice (bit-reproducibility), then `stale` (the buffers of the same call at the same shapes on other inputs: another seed, values
scaled by 4, another validity pattern, another dropout seed), and `ff` (every byte 0xFF, inside guard bands) only if `stale` was
bit-identical.  The three must be the same bits.  A case that float atomics make non-reproducible is listed in NOT_BIT_REPRODUCIBLE
with the atomic and is judged on the keys named there by the tolerance its parity test already carries, plus isfinite.

Waits and loop bounds read from memory (read from csrc/ before the cases were written): no kernel of the library waits on device
memory (no spin loop, no cooperative launch, no compare-and-swap loop anywhere in csrc/), and no `for` / `while` of a kernel takes its
bound from a caller's workspace or output: the bounds are kernel arguments, inputs (labels, indices) or LDS counters the kernel itself
sets first.  k_emd initialises its whole auction state (as, ass_inv, max_idx, max_inc, list0 and the LDS counters cnt[2]) in its
prologue, in LDS and in the workspace alike; dfx_noise_opt_run's stopped-row flags and counter are written by k_noise_init before the
first step and the host's early exit reads that counter only; dfx_masked_mse_f32 memsets its two doubles; the fused SA kernel's tile
loop runs to a.nt[], a kernel argument.  Hence every case runs all three modes; ZERO_STALE_ONLY is empty.

Library-owned workspaces (hipMalloc'd inside LatentSampler, dfx_shared_mlp, dfx_pointnet_v2 and the denoiser's pool) are out of the
harness's reach and are tested by sequence on one handle: Y then X at one shape, a larger shape on Y then the smaller on X; X must be
the bits of X on a fresh handle.

Dependences found: none (FIXES is empty; profiles/dirty_memory.txt holds the run).  The one cell that differed under `ff` was no
result: the 128 bytes of alignment padding between two regions of the shape-context buffer (see test_inference_engine)."""
import fnmatch
import time

import numpy as np
import pytest
import torch

import _gradstats as gs
import _latent_cfg as lc
import _batch_case as bc
from _dirty import allocations, first_difference, snapshot

pytestmark = pytest.mark.gpu

# ---- tables --------------------------------------------------------------------------------------------------------------------------
# function that allocates with torch.empty / empty_like (module.Class.function under difffacto_amd/) -> the test that holds it
COVERED = {
    "training.DenoiserTrainFn.forward": "test_denoiser_training_step",
    "training.DenoiserTrainFn.backward": "test_denoiser_training_step",
    "training.MaskedMSEFn.forward": "test_denoiser_training_step",
    "training.MaskedMSEFn.backward": "test_denoiser_training_step",
    "training.dropout_factors": "test_dropout_factors",
    "training.PointNetV2TrainFn.forward": "test_pointnet_v2_training_step",
    "training.pointnet_v2_branch": "test_pointnet_v2_training_step",
    "training.PriorLossFn.forward": "test_prior_loss",
    "training.PriorLossFn.backward": "test_prior_loss",
    "training.prior_loss_branch": "test_prior_loss",
    "training.AlignerTrainFn.forward": "test_aligner_training",
    "training.AlignerTrainFn.backward": "test_aligner_training",
    "latents.LatentSampler.optimize_noise": "test_noise_optimizer_trace",
    "pointnet2_ops.pointnet2_modules._SharedMLPTrainFn.forward": "test_shared_mlp_training",
    "pointnet2_ops.pointnet2_modules._SharedMLPTrainFn.backward": "test_shared_mlp_training",
    "pointnet2_ops.pointnet2_modules._PointnetSAModuleBase._forward_native": "test_set_abstraction_eval_forward",
    "pointnet2_ops.pointnet2_modules.PointnetFPModule._forward_native": "test_feature_propagation_eval_forward",
    "encoders.PointNetV2.forward": "test_pointnet_v2_eval_forward",
    "pointnet2_ops.pointnet2_utils.FurthestPointSampling.forward": "test_furthest_point_sampling",
    "pointnet2_ops.pointnet2_utils.BallQuery.forward": "test_ball_query",
    "pointnet2_ops.pointnet2_utils.ThreeNN.forward": "test_three_nn_and_interpolate",
    "pointnet2_ops.pointnet2_utils.ThreeInterpolate.forward": "test_three_nn_and_interpolate",
    "pointnet2_ops.pointnet2_utils.ThreeInterpolate.backward": "test_three_nn_and_interpolate",
    "pointnet2_ops.pointnet2_utils.GatherOperation.forward": "test_gather_and_group",
    "pointnet2_ops.pointnet2_utils.GatherOperation.backward": "test_gather_and_group",
    "pointnet2_ops.pointnet2_utils.GroupingOperation.forward": "test_gather_and_group",
    "pointnet2_ops.pointnet2_utils.GroupingOperation.backward": "test_gather_and_group",
    "metrics.emdFunction.forward": "test_emd",
    "metrics.emdFunction.backward": "test_emd",
    "engine.DenoiserEngine.prepare_shapes": "test_inference_engine",
    "engine.DenoiserEngine.eps": "test_inference_engine",
    "engine.DenoiserEngine.eps_t": "test_inference_engine",
    "engine.DenoiserEngine.p_sample": "test_inference_engine",
    "engine.DenoiserEngine.p_sample_ddim": "test_inference_engine",
    "engine.DenoiserEngine.sample_chain": "test_inference_engine",
    "engine.DenoiserEngine.sample_chain_ddim": "test_inference_engine",
    "engine.DenoiserEngine._chain_from": "test_inference_engine",
    "engine.DenoiserEngine.q_sample": "test_inference_engine",
    "engine.DenoiserEngine.masked_mse": "test_inference_engine",
    "latents.LatentSampler.flow_reverse": "test_latent_sampler",
    "latents.LatentSampler.flow_reverse_part": "test_latent_sampler",
    "latents.LatentSampler.part_aligner": "test_latent_sampler",
    "latents.LatentSampler.sample_latents": "test_latent_sampler",
    "latents.LatentSampler.compose_latents": "test_latent_sampler",
    "latents.LatentSampler.part_search": "test_latent_sampler",
    "latents.LatentSampler.part_search_global": "test_latent_sampler",
    "part_sampling.draw_stats": "test_part_sampling",
    "part_sampling.draw_normals": "test_part_sampling",
    "part_sampling.select_diverse": "test_part_sampling",
    "part_sampling.select_diverse_global": "test_part_sampling",
    "part_sampling.select_fit": "test_part_sampling",
    "evaluation.part_snapping": "test_part_metrics",
    "evaluation.part_boxes": "test_part_metrics",
    "evaluation.part_clouds": "test_part_metrics",
    "evaluation.box_pairwise": "test_part_metrics",
    "evaluation.occupancy_grid": "test_occupancy",
    "evaluation._device_jsd": "test_occupancy",
    "evaluation.entropy_of_occupancy_grid": "test_occupancy",
    "data.PartCloudSet.draw": "test_batch_assembly",
    "data.PartCloudSet.batch": "test_batch_assembly",
}
# function -> why no case holds it
EXEMPT = {
    "metrics.ChamferFunction.forward": "held to the contract by tests/test_gpu_chamfer.py, which poisons d1, d2, i1, i2 before the call",
    "metrics.ChamferFunction.backward": "held to the contract by tests/test_gpu_chamfer.py, which poisons both gradient buffers before the call",
    "parallel.gather_clouds": "receive buffers of torch.distributed gather / all_gather, which write every element; no libdfx kernel reads them",
    "parallel.probe_gather": "receive buffers of one four-element torch.distributed gather, which writes every element; no libdfx kernel reads them",
    "parallel.allreduce_gradients": "every slice of the flat bucket is filled by copy_ of a gradient or by zero_() before the all-reduce reads it",
    "training._PinnedRing.to_device": "host-pinned staging, overwritten by copy_ from the source array before it is read",
    "pipeline._FrontEnd.__init__": "the two noise buffers are filled by normal_() at the top of _body before sample_latents reads them",
}
# case-id pattern -> (the atomic that causes it, {result-key pattern: (atol, rtol) of the existing parity test}).  Only the candidates
# named from the source: the float atomicAdd scatters of pointnet2_kernels.hip and the float64 atomics of k_masked_mse.
NOT_BIT_REPRODUCIBLE = {
    "gather-*": ("atomicAdd(grad_points + bc * N + a, ...) of gather_points_grad (pointnet2_kernels.hip:53)",
                 {"d_features": (1e-4, 1e-5)}),            # tests/test_gpu_pointnet2.py::test_gather_matches_oracle
    "group-*": ("atomicAdd(P + l * N, ...) of group_points_grad (pointnet2_kernels.hip:417)",
                {"d_features": (2e-3, 1e-4)}),             # ::test_group_matches_oracle
    "three_nn-*": ("atomicAdd(P + I[k], g * W[k]) of three_interpolate_grad (pointnet2_kernels.hip:507-509)",
                   {"d_features": (1e-3, 1e-4)}),          # ::test_three_nn_interpolate_match_oracle
    "denoiser-train-*": ("atomicAdd(acc, s) in float64 of k_masked_mse (denoiser_kernel.hip:2158): the loss alone; its backward reads only the "
                         "sum of the flags, which is exact in any order", {"loss": (5e-6, 0.0)}),     # tests/test_gpu_train.py: |loss - golden| < 5e-6
    "engine-*": ("atomicAdd(acc, s) in float64 of k_masked_mse (denoiser_kernel.hip:2158)", {"masked_mse": (5e-6, 0.0)}),
}
ZERO_STALE_ONLY = {}     # entry point -> reason; empty: see the module docstring
# (failing case, cell, mode that caught it, remedy) of every dependence found
FIXES = ()

LINES = []


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print(f"\nDIRTY wall time of tests/test_gpu_dirty_memory.py: {time.time() - t0:.0f} s, {len(LINES)} cases", flush=True)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def _loose_keys(case_id):
    for pat, (_, keys) in NOT_BIT_REPRODUCIBLE.items():
        if fnmatch.fnmatch(case_id, pat):
            return keys
    return {}


def _tol_of(key, loose):
    for pat, tol in loose.items():
        if fnmatch.fnmatch(key, pat):
            return tol
    return None


def _compare(case_id, a, b):
    """None if b equals a: bit for bit, except on the keys NOT_BIT_REPRODUCIBLE names for this case (tolerance + isfinite)."""
    loose = _loose_keys(case_id)
    strict_a = {k: v for k, v in a.items() if _tol_of(k, loose) is None}
    strict_b = {k: v for k, v in b.items() if _tol_of(k, loose) is None}
    d = first_difference(strict_a, strict_b)
    if d is not None:
        return d
    for k in a:
        tol = _tol_of(k, loose)
        if tol is not None:
            if k not in b or not bool(torch.isfinite(b[k]).all()):
                return f"{k}: missing or not finite"
            if not torch.allclose(b[k].double(), a[k].double(), atol=tol[0], rtol=tol[1]):
                return f"{k}: max-abs difference {float((b[k].double() - a[k].double()).abs().max()):.3e} beyond atol {tol[0]} rtol {tol[1]}"
    return None


def three_modes(case_id, prep, call):
    """prep(alt) -> state (fresh inputs / modules; alt = the recorded run's other inputs, same shapes); call(state) -> {name: tensor}.
    prep runs outside the harness, call inside."""
    def once(mode, alt=False, recording=None):
        state = prep(alt)
        torch.cuda.synchronize()
        with allocations(mode, recording=recording) as h:
            out = call(state)
            torch.cuda.synchronize()
            snap = snapshot(out)
        del out, state
        return snap, h

    z1, hz = once("zero")
    z2, _ = once("zero")
    repro = first_difference(z1, z2) is None
    d = _compare(case_id, z1, z2)
    assert d is None, f"{case_id}: two zero runs differ outside NOT_BIT_REPRODUCIBLE: {d}"
    _, rec = once("record", alt=True)
    s, hs = once("stale", recording=rec.recording)
    ds = _compare(case_id, z1, s)
    line = f"DIRTY {case_id}: results {len(z1)} | served zero {hz.served} stale {hs.served}"
    if ds is not None:
        LINES.append(line + f" | zero x2 reproducible {'yes' if repro else 'no'} | stale identical NO ({ds}) | ff not attempted")
        print(LINES[-1], flush=True)
        pytest.fail(f"{case_id}: stale differs from zero: {ds}")
    f, hf = once("ff")
    df = _compare(case_id, z1, f)
    LINES.append(line + f" ff {hf.served} | zero x2 reproducible {'yes' if repro else 'no'} | stale identical yes | ff identical {'yes' if df is None else 'NO (' + df + ')'}")
    print(LINES[-1], flush=True)
    assert df is None, f"{case_id}: ff differs from zero: {df}"
    assert hz.served == hs.served == hf.served > 0


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib():
    from difffacto_amd import _ffi
    return _ffi.lib()


def _grads(prefix, named):
    return {f"{prefix}{k}": p.grad for k, p in named.items() if p.grad is not None}


# ---- denoiser training step ----------------------------------------------------------------------------------------------------------
TRAIN_SHAPES = {"B8_N32": (8, 32, 31, False, False), "B3_N160": (3, 160, 32, True, True), "B5_N480": (5, 480, 33, True, True)}
TRAIN_PATHS = {"f32": ("f32", 1, "layer_f32"), "layer": ("bf16", 0, "layer_bf16"), "fused": ("bf16", 1, "fused_bf16")}
TRAIN_DROPS = {"p0": (None, None), "p0.2": ((0.2, 20261019), (0.2, 777))}
TRAIN_CASES = [(n, p, d, 1) for n in TRAIN_SHAPES for p in TRAIN_PATHS for d in TRAIN_DROPS] + [("B5_N480", "fused", "p0.2", 0)]


def _train_prep(name, alt):
    B, N, seed, mixed, flags = TRAIN_SHAPES[name]
    c = gs.make_train_case(B, N, seed + (100 if alt else 0), mixed=mixed, with_flags=flags)
    if alt:   # other values at 4 x the scale, and the validity pattern of the batch reversed (the single-part shape comes last)
        c = {k: (v if k == "W" or v is None else np.ascontiguousarray(v[::-1])) for k, v in c.items()}
        for k in ("x_t", "noise", "ctx_code"):
            c[k] = (4 * c[k]).astype(np.float32)
    s = {k: cu(v) for k, v in c.items() if k != "W"}
    s["P"] = {k: cu(v).requires_grad_(True) for k, v in c["W"].items()}
    for k in ("ctx_code", "ctx_mv", "x_t", "variances_pt"):
        s[k].requires_grad_(True)
    return s


def _train_call(s, path, drop, streams):
    from difffacto_amd import training
    prec, fused, record = TRAIN_PATHS[path]
    L = _lib()
    L.dfx_debug_train_fused(fused)
    L.dfx_debug_train_streams(streams)
    try:
        eps = training.denoiser_train_forward(s["P"], s["x_t"], s["t"], s["ctx_code"], s["ctx_mv"], s["anchors_pt"], s["variances_pt"], s["valid"],
                                              s["assignment"], precision=prec, dropout=drop)
        took = L.dfx_debug_last_train_path().decode()
        loss = training.masked_mse(s["noise"], eps, s["flags"])
        loss.backward()
        torch.cuda.synchronize()
    finally:
        L.dfx_debug_train_fused(1)
        L.dfx_debug_train_streams(1)
    assert took == record + ("_dropout" if drop else ""), f"path {path}: the library took {took}"
    out = {"eps": eps, "loss": loss, "d_ctx_code": s["ctx_code"].grad, "d_ctx_mv": s["ctx_mv"].grad, "d_x": s["x_t"].grad, "d_variances": s["variances_pt"].grad}
    out.update(_grads("g/", s["P"]))
    assert len(out) == 6 + 77 and all(v is not None for v in out.values())
    return out


@pytest.mark.parametrize("name,path,dkey,streams", TRAIN_CASES, ids=[f"{n}-{p}-{d}" + ("" if s else "-one_stream") for n, p, d, s in TRAIN_CASES])
def test_denoiser_training_step(name, path, dkey, streams):
    """denoiser_train_forward -> masked_mse -> backward; x_t and variances_pt require grad.  (8, 32): the smallest fused shape; (3, 160): a
    quarter-full workgroup; (5, 480): slabs with an empty row range.  Workspace-carried state: the PathRecord, written by the forward
    before the backward reads it.  No wait or loop bound is read from the workspace."""
    drop, drop_alt = TRAIN_DROPS[dkey]
    state = {"alt": False}

    def prep(alt):
        state["alt"] = alt
        return _train_prep(name, alt)
    three_modes(f"denoiser-train-{name}-{path}-{dkey}" + ("" if streams else "-one_stream"), prep,
                lambda s: _train_call(s, path, drop_alt if state["alt"] else drop, streams))


def test_dropout_factors():
    """dfx_debug_dropout_factors: every one of the n factors is written (n = 1000: a ragged last group of four)."""
    from difffacto_amd import training
    three_modes("dropout-factors", lambda alt: dict(seed=5 if alt else 20261019, site=3 if alt else 1000),
                lambda s: {"f": training.dropout_factors(s["seed"], s["site"], 0.2, 1000)})


# ---- PointNetV2 training step --------------------------------------------------------------------------------------------------------
def _pnv2_prep(B, N, alt):
    from difffacto_amd import synth, training
    rng = np.random.Generator(np.random.PCG64(B * 1000 + N + (500 if alt else 0)))
    W = synth.make_pointnet_v2_weights(2)
    x = (rng.uniform(-1, 1, size=(B, N, 3)) * (4 if alt else 1)).astype(np.float32)
    seg = rng.integers(0, 4, size=(B, N))
    if alt:
        seg[B - 1][seg[B - 1] == 0] = 3                        # the last shape lacks part 0
    else:
        seg[0][seg[0] == 2] = 1                                # shape 0 lacks part 2
    attn = np.eye(4, dtype=np.float32)[seg]
    return dict(P={n: cu(W[n].copy()).requires_grad_(True) for n in training.PNV2_PARAMS}, Bf={n: cu(W[n].copy()) for n in training.PNV2_BUFFERS},
                x=cu(x), attn=cu(attn), dm=cu(rng.standard_normal((B, 4, 256)).astype(np.float32)), dv=cu(rng.standard_normal((B, 4, 256)).astype(np.float32)))


def _pnv2_call(s, fused_stats):
    from difffacto_amd import training
    L = _lib()
    L.dfx_debug_bn_fused_stats(fused_stats)
    try:
        m, v = training.pointnet_v2_train_forward(s["P"], s["Bf"], s["x"], s["attn"])
        branch = training.pointnet_v2_branch(m)
        ((m * s["dm"]).sum() + (v * s["dv"]).sum()).backward()
        torch.cuda.synchronize()
    finally:
        L.dfx_debug_bn_fused_stats(1)
    out = {"m": m, "v": v}
    out.update({f"running/{k}": b for k, b in s["Bf"].items()})
    out.update(_grads("g/", s["P"]))
    out.update({f"branch/{k}": b for k, b in branch.items()})
    assert len(out) == 2 + len(training.PNV2_BUFFERS) + 36 + 8
    return out


@pytest.mark.parametrize("B,N,fused_stats", [(2, 33, 1), (4, 333, 1), (8, 1024, 1), (8, 1024, 0)])
def test_pointnet_v2_training_step(B, N, fused_stats):
    """m, v, the running statistics (training.PNV2_BUFFERS: the trunk's eight and the heads' eight), 36 gradients and the exported branch.  (8, 1024) = 8192 rows: the epilogue statistics partials
    (rows of (count, mean, M2)) with both settings of dfx_debug_bn_fused_stats.  No wait or loop bound is read from the workspace."""
    three_modes(f"pointnet_v2-train-B{B}_N{N}-stats{fused_stats}", lambda alt: _pnv2_prep(B, N, alt), lambda s: _pnv2_call(s, fused_stats))


# ---- prior loss ----------------------------------------------------------------------------------------------------------------------
def _prior_prep(B, alt):
    from difffacto_amd import synth, training
    rng = np.random.Generator(np.random.PCG64(3 + (50 if alt else 0)))
    W = synth.make_latent_weights(1)
    z = (rng.standard_normal((B, 256, 4)) * (4 if alt else 1)).astype(np.float32)
    lv = (-2.0 + 0.5 * rng.standard_normal((B, 4, 256))).astype(np.float32)
    valid = synth.make_latents(B, seed=9 if alt else 5)[3]
    if B > 1:
        valid[B - 1 if alt else 0] = [0, 1, 0, 0] if alt else [1, 0, 1, 1]
    return dict(P={n: cu(W[n].copy()).requires_grad_(True) for n in training.flow_param_names(14)}, z=cu(z).requires_grad_(True),
                lv=cu(lv).requires_grad_(True), valid=cu(valid))


def _prior_call(s):
    from difffacto_amd import training
    loss, log_p, ent = training.prior_loss(s["P"], s["z"], s["lv"], s["valid"], prior_var=1.0, kl_weight=5e-4)
    branch = training.prior_loss_branch(loss)
    loss.backward()
    out = {"loss": loss, "log_p": log_p, "entropy": ent, "d_part_code": s["z"].grad, "d_logvar": s["lv"].grad}
    out.update(_grads("g/", s["P"]))
    out.update({f"branch/{k}": b for k, b in branch.items()})
    assert len(out) == 5 + 336 + 2
    return out


@pytest.mark.parametrize("B", [1, 37, 65])
def test_prior_loss(B):
    """loss, log_p, entropy, both data gradients, 336 parameter gradients, the exported ReLU masks.  B = 65: one row past the 64-row slab
    of carve_flow; ragged validity.  No wait or loop bound is read from the workspace."""
    three_modes(f"prior_loss-B{B}", lambda alt: _prior_prep(B, alt), _prior_call)


# ---- aligner training ----------------------------------------------------------------------------------------------------------------
ALIGNER_VARIANTS = {"params": dict(grad=True), "frozen": dict(grad=False), "d_noise_only": dict(grad=False, code_grad=False),
                    "d_mean_only": dict(grad=True, d_logvar=False)}


def _aligner_prep(tag, B, alt, grad=True, code_grad=True, **_):
    x = lc.inputs(tag, B, 1, 2000 * B + (7 if alt else 0), "shape_all_absent" if alt else "one_absent")
    s = {k: cu((4 * v).astype(np.float32) if alt and k in ("code", "noise") else v) for k, v in x.items()}
    s["P"] = lc.aligner_params(lc.weights(tag), "cuda", grad=grad)
    s["code"].requires_grad_(code_grad)
    s["noise"].requires_grad_(True)
    return s


def _aligner_call(tag, s, d_mean=True, d_logvar=True, **_):
    from difffacto_amd import training
    cfg = lc.CONFIGS[tag]
    mean, logvar = training.aligner_train_forward(s["P"], s["code"], s["valid"], s["noise"], n_class=cfg["n_class"], zdim=cfg["zdim"], n_heads=cfg["heads"],
                                                  d_head=cfg["d_head"], noise_dim=cfg["noise_dim"], noise_scale=lc.NOISE_SCALE)
    loss = 0
    if d_mean:
        loss = loss + (mean * s["d_mean"]).sum()
    if d_logvar:
        loss = loss + (logvar * s["d_logvar"]).sum()
    loss.backward()
    out = {"mean": mean, "logvar": logvar, "d_part_code": s["code"].grad, "d_noise": s["noise"].grad}
    out.update(_grads("g/", s["P"]))
    return out


@pytest.mark.parametrize("variant", list(ALIGNER_VARIANTS))
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("tag", ["tiny", "shipped"])
def test_aligner_training(tag, B, variant):
    """aligner_train_forward + backward: with parameter gradients, frozen (dfx_aligner_input_backward), d_noise only, one cotangent only.
    B = 17 with J = 3: 51 rows, a partial 16-row tile.  No wait or loop bound is read from the workspace."""
    kw = ALIGNER_VARIANTS[variant]
    three_modes(f"aligner-train-{tag}-B{B}-{variant}", lambda alt: _aligner_prep(tag, B, alt, **kw), lambda s: _aligner_call(tag, s, **kw))


# ---- latent sampler, noise optimizer -------------------------------------------------------------------------------------------------
_SAMPLERS = {}


def _sampler(tag, fresh=False):
    from difffacto_amd.latents import LatentSampler
    cfg = lc.CONFIGS[tag]
    make = lambda: LatentSampler(lc.weights(tag), n_class=cfg["n_class"], zdim=cfg["zdim"], n_heads=cfg["heads"], d_head=cfg["d_head"], cimle=cfg["cimle"],
                                 noise_dim=cfg["noise_dim"], noise_scale=lc.NOISE_SCALE)
    if fresh:
        return make()
    if tag not in _SAMPLERS:
        _SAMPLERS[tag] = make()
    return _SAMPLERS[tag]


def _noise_opt_prep(alt):
    from difffacto_amd import editing
    cfg = lc.CONFIGS["tiny"]
    J, Z, ND, R = cfg["n_class"], cfg["zdim"], cfg["noise_dim"], 4
    rng = np.random.Generator(np.random.PCG64(14 if alt else 13))
    code = (rng.standard_normal((R, Z, J)) * (4 if alt else 1)).astype(np.float32)
    valid = np.ones((R, J), np.float32)
    valid[2 if alt else 1, 0 if alt else 1] = 0
    ref_mean = (rng.standard_normal((R, 3, J)) * 0.3).astype(np.float32)
    ref_var = (rng.uniform(0.2, 0.6, size=(R, 3, J)) ** 2).astype(np.float32)
    ep = np.array([0, 2, J - 1, 0])
    fix = np.ones((R, J), np.float32)
    fix[np.arange(R), ep] = 0
    new_mean = ref_mean[np.arange(R), :, ep] + np.array([0.15, 0.0, -0.1], np.float32)
    z0 = rng.standard_normal((R, ND)).astype(np.float32)
    return dict(code=torch.from_numpy(code), valid=torch.from_numpy(valid), z0=torch.from_numpy(z0),
                prob=editing.noise_problem(valid, ref_mean, ref_var, fix, ep, new_mean=new_mean))


def test_noise_optimizer_trace():
    """LatentSampler.optimize_noise, tiny, R = 4 with one absent part, 20 iterations, trace=True: z, mean, logvar, iters_done and the whole
    trace, including the rows behind a stopped row that dfx.h promises as zeros.  The per-row stopped flags and the stopped-row counter
    live in the workspace; k_noise_init writes both before the first step, and only the host's early exit reads the counter."""
    ls = _sampler("tiny")
    three_modes("noise_opt-tiny-R4", _noise_opt_prep, lambda s: ls.optimize_noise(s["code"], s["valid"], s["z0"], s["prob"], 20, trace=True))


def _latent_prep(tag, B, alt):
    cfg = lc.CONFIGS[tag]
    J, Z, ND, K = cfg["n_class"], cfg["zdim"], cfg["noise_dim"], 3
    x = lc.inputs(tag, B, K, 1000 * B + (3 if alt else 0), "shape_all_absent" if alt else "one_absent")
    x = {k: torch.from_numpy((4 * v).astype(np.float32) if alt and k in ("w_noise", "code") else v) for k, v in x.items()}
    rng = np.random.Generator(np.random.PCG64(77 + alt))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x.update(valid_r=x["valid"].repeat_interleave(K, 0), code_r=x["code"].repeat_interleave(K, 0), K=K,
             code_a=((np.arange(B)[:, None] + np.arange(J)[None, :] * (2 if alt else 1)) % B).astype(np.int32), new=f(B, Z), tm=0.3 * f(B, 3, J), tl=-2 + 0.3 * f(B, 3, J),
             weight=x["valid"] * torch.from_numpy((np.arange(J) != (1 if alt else 0)).astype(np.float32))[None], wpart=f(B * K, Z))
    return x


def _latent_call(tag, ls, x):
    cfg = lc.CONFIGS[tag]
    J, K, B = cfg["n_class"], x["K"], x["valid"].shape[0]
    npoints = 3 * J
    fid = lc.fixed_patterns(J)["last"]
    out = {"flow_reverse": ls.flow_reverse(x["w_noise"]), "flow_reverse_part": ls.flow_reverse_part(J - 1, x["wpart"])}
    m, l = ls.part_aligner(x["code_r"], x["valid_r"], x["noise"])
    out.update({"aligner/mean": m, "aligner/logvar": l})
    a = ls.sample_latents(x["w_noise"], x["noise"], x["valid"], None, K=K, npoints=npoints)
    b = ls.sample_latents(None, x["noise"], x["valid"], fid, K=K, npoints=npoints, part_code=x["code"])
    c = ls.compose_latents(x["code"], np.repeat(x["code_a"], K, axis=0), x["valid_r"], noise_src=x["noise"], npoints=npoints)
    for name, d in (("sample", a), ("sample_given_fixed", b), ("compose", c)):
        out.update({f"{name}/{k}": v for k, v in d.items()})
    kw = dict(new_code=x["new"], new_part=J - 1, return_scores=True)
    searches = {"search_fit": ls.part_search(x["code"], x["code_a"], x["valid"], x["noise"], K, "fit", P=1, target_mean=x["tm"], target_logvar=x["tl"], weight=x["weight"], **kw),
                "search_first": ls.part_search(x["code"], x["code_a"], x["valid"], x["noise"], K, "first", P=2, **kw),
                "search_diverse": ls.part_search(x["code"], x["code_a"], x["valid"], x["noise"], K, "diverse", P=2, seed=9, row0=70, row_budget=2 * K, **kw),
                "search_global": ls.part_search_global(x["code"], x["code_a"], x["valid"], x["noise"], K, min(B * K, 4), seed=9, return_scores=True)}
    for name, d in searches.items():
        out.update({f"{name}/{k}": v for k, v in d.items()})
    return out


@pytest.mark.parametrize("B", [1, 11])
@pytest.mark.parametrize("tag", ["tiny", "shipped"])
def test_latent_sampler(tag, B):
    """flow_reverse, flow_reverse_part, part_aligner, sample_latents (drawn codes; given part_code with the last part fixed), compose_latents,
    part_search in its three modes and part_search_global, every returned tensor.  B = 11 with J = 3: 33 token rows, a partial 32-row tile.
    The handle's own workspace is library-owned (see the sequence tests).  No wait or loop bound is read from a caller's buffer: the
    search's chunk loop runs on the host over row_budget."""
    ls = _sampler(tag)
    three_modes(f"latent_sampler-{tag}-B{B}", lambda alt: _latent_prep(tag, B, alt), lambda x: _latent_call(tag, ls, x))


# ---- shared-MLP training, SA / FP eval forward ---------------------------------------------------------------------------------------
def _randomize(mod, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = mod.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            a = rng.uniform(0.5, 1.5, size=tuple(v.shape))
        elif k.endswith("running_mean") or k.endswith("bias"):
            a = rng.uniform(-0.2, 0.2, size=tuple(v.shape))
        elif v.dim() == 1:
            a = rng.uniform(0.8, 1.2, size=tuple(v.shape))
        else:
            a = rng.uniform(-1, 1, size=tuple(v.shape)) / np.sqrt(v.shape[1])
        sd[k] = torch.from_numpy(a.astype(np.float32))
    mod.load_state_dict(sd)
    return mod.cuda()


MLP_CASES = [([6, 64, 64, 128], 2, 37, 16, True, True), ([131, 128, 128], 2, 30, 1, False, True), ([259, 256, 512, 1024], 2, 1, 128, True, True),
             ([6, 64, 64, 128], 2, 37, 16, True, False)]


@pytest.mark.parametrize("spec,B,M,ns,pool,train", MLP_CASES, ids=["sa1_pool", "fp_nopool", "groupall_1024", "eval_under_autograd"])
def test_shared_mlp_training(spec, B, M, ns, pool, train):
    """pm.shared_mlp_train: y, d_x, every parameter gradient and the running statistics.  The ns-slab partials that wgrad, bn_fwd and bn_bwd
    share in the workspace are live at every shape here.  No wait or loop bound is read from the workspace."""
    from difffacto_amd.pointnet2_ops import pointnet2_modules as pm

    def prep(alt):
        g = torch.Generator().manual_seed(6 if alt else 5)
        mod = _randomize(pm.build_shared_mlp(list(spec), bn=True), 7).train(train)
        return dict(mod=mod, x=((4 if alt else 1) * torch.randn(B, spec[0], M, ns, generator=g)).cuda().requires_grad_(True),
                    gout=torch.randn((B, spec[-1], M) if pool else (B, spec[-1], M, ns), generator=g).cuda())

    def call(s):
        y = pm.shared_mlp_train(s["mod"], s["x"], pool=pool)
        y.backward(s["gout"])
        out = {"y": y, "d_x": s["x"].grad}
        out.update(_grads("g/", dict(s["mod"].named_parameters())))
        out.update({f"buffer/{k}": b for k, b in s["mod"].named_buffers()})
        return out
    three_modes(f"shared_mlp-train-{'-'.join(map(str, spec))}-B{B}_M{M}_ns{ns}-{'train' if train else 'eval'}", prep, call)


SA_CASES = [(3, 256, 21, 16, [4, 32, 32, 64]), (2, 400, 50, 40, [4, 64, 64, 128]), (2, 400, 37, 96, [4, 64, 64, 128]), (2, 400, 33, 128, [4, 128, 128, 256])]


def _sa_prep(B, N, C, alt):
    rng = np.random.Generator(np.random.PCG64(B * 1000 + N + (17 if alt else 0)))
    return dict(xyz=cu(rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)), feats=cu(((4 if alt else 1) * rng.standard_normal((B, C, N))).astype(np.float32)))


@pytest.mark.parametrize("force_general", [False, True], ids=["fused", "general"])
@pytest.mark.parametrize("B,N,npoint,nsample,mlp", SA_CASES, ids=["1tile", "2tiles", "3tiles", "4tiles"])
def test_set_abstraction_eval_forward(B, N, npoint, nsample, mlp, force_general):
    """FPS -> gather -> ball query -> dfx_sa_forward_f32 with 1, 2, 3 and 4 tiles per centre (3 tiles: a centre straddles workgroups and the
    kernel takes its atomic-max path into `out`, which the entry point clears), fused and general.  Results: the centres and the features."""
    from difffacto_amd.pointnet2_ops.pointnet2_modules import PointnetSAModule
    mod = _randomize(PointnetSAModule(npoint=npoint, radius=0.6, nsample=nsample, mlp=list(mlp)), nsample).eval()

    def call(s):
        with torch.no_grad():
            new_xyz = mod._centres(s["xyz"])
            out = mod._forward_native(0, s["xyz"], new_xyz, s["feats"], force_general=force_general)
        if not force_general:
            assert _lib().dfx_shared_mlp_is_fused(mod._native(0).handle()) == 1
        return {"new_xyz": new_xyz, "features": out}
    three_modes(f"sa-eval-B{B}_N{N}_M{npoint}_ns{nsample}-{'general' if force_general else 'fused'}", lambda alt: _sa_prep(B, N, mlp[0], alt), call)


def test_set_abstraction_group_all_eval_forward():
    from difffacto_amd.pointnet2_ops.pointnet2_modules import PointnetSAModule
    mod = _randomize(PointnetSAModule(mlp=[4, 32, 64]), 3).eval()

    def call(s):
        with torch.no_grad():
            return {"features": mod(s["xyz"], s["feats"])[1]}
    three_modes("sa-eval-groupall-B2_N100", lambda alt: _sa_prep(2, 100, 4, alt), call)


@pytest.mark.parametrize("with_known", [True, False], ids=["known", "no_known"])
def test_feature_propagation_eval_forward(with_known):
    """dfx_fp_forward_f32: three_nn + interpolation + shared MLP in one call; without `known` the (B, C2, 1) features are broadcast."""
    from difffacto_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    mod = _randomize(PointnetFPModule(mlp=[5 + 3, 32, 20]), 4).eval()

    def prep(alt):
        rng = np.random.Generator(np.random.PCG64(21 + alt))
        f = lambda *s: cu(((4 if alt else 1) * rng.standard_normal(s)).astype(np.float32))
        return dict(unknown=f(2, 50, 3), known=f(2, 20, 3) if with_known else None, uf=f(2, 3, 50), kf=f(2, 5, 20 if with_known else 1))

    def call(s):
        with torch.no_grad():
            return {"features": mod(s["unknown"], s["known"], s["uf"], s["kf"])}
    three_modes(f"fp-eval-{'known' if with_known else 'no_known'}", prep, call)


def _pnv2_module():
    from difffacto_amd import synth
    from difffacto_amd.encoders import PointNetV2
    enc = PointNetV2(zdim=256, num_anchors=4, per_part_mlp=True)
    sd = enc.state_dict()
    for k, a in synth.make_pointnet_v2_weights(2).items():
        sd[k] = torch.from_numpy(a.copy())
    enc.load_state_dict(sd)
    return enc.cuda().eval()


def _pnv2_eval_inputs(B, N, seed, scale=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    seg = rng.integers(0, 4, size=(B, N))
    seg[0][seg[0] == 2] = 1
    return cu((scale * rng.uniform(-1, 1, size=(B, N, 3))).astype(np.float32)), cu(np.eye(4, dtype=np.float32)[seg])


def test_pointnet_v2_eval_forward():
    enc = _pnv2_module()

    def call(s):
        with torch.no_grad():
            m, v = enc(*s)
        return {"m": m, "v": v}
    three_modes("pointnet_v2-eval-B3_N200", lambda alt: _pnv2_eval_inputs(3, 200, 8 + alt, 4 if alt else 1), call)


# ---- pointnet2 primitives ------------------------------------------------------------------------------------------------------------
def _pu():
    from difffacto_amd.pointnet2_ops import pointnet2_utils
    return pointnet2_utils


@pytest.mark.parametrize("B,N,M", [(2, 700, 64), (1, 20000, 64)])
def test_furthest_point_sampling(B, N, M):
    """(1, 20000, 64): the streaming kernel with its `tmp` distance scratch, which the kernel fills with 1e10 before its first pick."""
    def prep(alt):
        rng = np.random.default_rng(N + M + alt)
        return cu(((4 if alt else 1) * rng.standard_normal((B, N, 3))).astype(np.float32))
    three_modes(f"fps-B{B}_N{N}_M{M}", prep, lambda xyz: {"idx": _pu().furthest_point_sample(xyz, M)})


def test_ball_query():
    """(3, 100, 7, r 0.5, ns 5) with one centre that has no neighbour: its row must come back as zeros, not as what the buffer held."""
    B, N, M, r, ns = 3, 100, 7, 0.5, 5

    def prep(alt):
        rng = np.random.default_rng(N * 7 + M + alt)
        xyz = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
        new_xyz = xyz[:, rng.permutation(N)[:M]].copy()
        new_xyz[:, 0 if alt else -1] = 50.0
        return cu(xyz), cu(new_xyz)

    def call(s):
        idx = _pu().ball_query(r, ns, *s)
        return {"idx": idx}
    three_modes("ball_query-B3_N100_M7", prep, call)


def test_three_nn_and_interpolate():
    B, n, m, c = 1, 5, 3, 2

    def prep(alt):
        rng = np.random.default_rng(n + m + alt)
        f = lambda *s: ((4 if alt else 1) * rng.standard_normal(s)).astype(np.float32)
        return dict(unknown=cu(f(B, n, 3)), known=cu(f(B, m, 3)), w=cu(rng.random((B, n, 3)).astype(np.float32)), feats=cu(f(B, c, m)).requires_grad_(True), g=cu(f(B, c, n)))

    def call(s):
        dist, idx = _pu().three_nn(s["unknown"], s["known"])
        out = _pu().three_interpolate(s["feats"], idx, s["w"])
        out.backward(s["g"])
        return {"dist": dist, "idx": idx, "out": out, "d_features": s["feats"].grad}
    three_modes("three_nn-B1_n5_m3_c2", prep, call)


@pytest.mark.parametrize("kind,shape", [("gather", (2, 7, 1, 5)), ("group", (1, 3, 100, 9, 5))])
def test_gather_and_group(kind, shape):
    def prep(alt):
        rng = np.random.default_rng(sum(shape) + alt)
        B, C, N = shape[:3]
        isz, gsz = ((B, shape[3]), (B, C, shape[3])) if kind == "gather" else ((B, shape[3], shape[4]), (B, C, shape[3], shape[4]))
        f = lambda *s: ((4 if alt else 1) * rng.standard_normal(s)).astype(np.float32)
        return dict(pts=cu(f(B, C, N)).requires_grad_(True), idx=cu(rng.integers(0, N, size=isz).astype(np.int32)), g=cu(f(*gsz)))

    def call(s):
        out = (_pu().gather_operation if kind == "gather" else _pu().grouping_operation)(s["pts"], s["idx"])
        out.backward(s["g"])
        return {"out": out, "d_features": s["pts"].grad}
    three_modes(f"{kind}-{'_'.join(map(str, shape))}", prep, call)


# ---- EMD -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_global", [0, 1], ids=["state_lds", "state_workspace"])
@pytest.mark.parametrize("B,n,iters", [(1, 96, 40), (2, 257, 300)])
def test_emd(B, n, iters, state_global):
    """dist, assignment and the backward.  With dfx_debug_emd_state_global(1) the auction's state lives in the caller's workspace; k_emd's
    prologue writes as, ass_inv, max_idx, max_inc and list0 there and the two list counters are LDS words it sets itself, so no loop bound
    is read from the workspace."""
    from difffacto_amd.metrics import emdFunction

    def prep(alt):
        rng = np.random.Generator(np.random.PCG64(n + iters + alt))
        return dict(a=cu(rng.uniform(0, 1, (B, n, 3)).astype(np.float32)).requires_grad_(True), b=cu(rng.uniform(0, 1, (B, n, 3)).astype(np.float32)),
                    w=torch.linspace(0.5, 1.5, n, device="cuda")[None].expand(B, -1))

    def call(s):
        L = _lib()
        L.dfx_debug_emd_state_global(state_global)
        try:
            d, asg = emdFunction.apply(s["a"], s["b"], 0.002, iters)
            (d * s["w"]).sum().backward()
            torch.cuda.synchronize()
        finally:
            L.dfx_debug_emd_state_global(0)
        return {"dist": d, "assignment": asg, "d_xyz1": s["a"].grad}
    three_modes(f"emd-B{B}_n{n}_it{iters}-{'workspace' if state_global else 'lds'}", prep, call)


# ---- inference engine ----------------------------------------------------------------------------------------------------------------
ENG_T, ENG_B, ENG_N = 12, 3, 288
_ENGINES = {}


def _engine(prec, fresh=False):
    from difffacto_amd import synth
    from difffacto_amd.engine import DenoiserEngine
    make = lambda: DenoiserEngine({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(seed=0).items()}, num_timesteps=ENG_T, precision=prec)
    if fresh:
        return make()
    if prec not in _ENGINES:
        _ENGINES[prec] = make()
    return _ENGINES[prec]


def _engine_case(B, N, alt, seed=41):
    from difffacto_amd import synth
    from oracle import diffusion as odf
    part_code, mean, logvar, valid = synth.make_latents(B, seed=seed + (9 if alt else 0), all_valid=True)
    if B >= 3:
        valid[2 if alt else 1] = [1, 0, 1, 1]      # an absent part
        valid[0 if alt else 2] = [0, 0, 1, 0]      # a single part
    var = np.exp(logvar).astype(np.float32)
    seg = synth.make_seg_mask(valid, N)
    anchors, variance = odf.gather_params(seg, mean, var)
    rng = np.random.default_rng(N + seed + alt)
    k = 4 if alt else 1
    x0 = (anchors + 0.5 * np.sqrt(variance) * rng.standard_normal((B, 3, N))).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return dict(latents=tuple(t(a) for a in ((k * part_code).astype(np.float32), mean, var, valid)), seg=cu(seg), x0=cu(k * x0),
                noise=cu(rng.standard_normal((B, 3, N)).astype(np.float32)), flags=cu((rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32)),
                tvec=torch.tensor([(3 + alt + 4 * b) % ENG_T for b in range(B)]), seed=2024 + alt)


def _engine_call(eng, c):
    nbytes = _lib().dfx_shape_ctx_bytes(eng._h, c["seg"].shape[0])
    ctx = eng.prepare_shapes(*c["latents"])
    seg, x0, seed = c["seg"], c["x0"], c["seed"]
    B = c["seg"].shape[0]
    a1 = (128 * B + 255) & ~255                      # csrc/denoiser_internal.h: shape_ctx_view carves three 256-byte aligned regions
    a2 = a1 + 2048 * B
    out = {"ctx/part": ctx.buf[:128 * B], "ctx/cpart": ctx.buf[a1:a2], "ctx/as_ms": ctx.buf[a2:nbytes], "eps": eng.eps(ctx, x0, seg, 5), "eps_t": eng.eps_t(ctx, x0, seg, c["tvec"]), "q_sample": eng.q_sample(ctx, seg, x0, c["tvec"], c["noise"]),
           "masked_mse": eng.masked_mse(c["noise"], x0, c["flags"])}
    out["p_sample"], out["p_sample_xstart"] = eng.p_sample(ctx, x0, seg, 5, seed=seed, want_xstart=True)
    out["p_sample_given_noise"] = eng.p_sample(ctx, x0, seg, 0, noise=c["noise"])
    out["ddim_step"], out["ddim_step_xstart"] = eng.p_sample_ddim(ctx, x0, seg, 5, 0.5, seed=seed, want_xstart=True)
    chains = {"chain": eng.sample_chain(ctx, seg, seed=seed, ret_interval=4), "chain_no_traj": eng.sample_chain(ctx, seg, seed=seed),
              "ddim": eng.sample_chain_ddim(ctx, seg, [0, 2, 5, 8, 11], 0.5, seed=seed, ret_interval=4),
              "from": eng.sample_chain_from(ctx, seg, x0, 8, seed=seed, ret_interval=4, hold=[0, 2, 0]),
              "refine": eng.refine_chain(ctx, seg, x0, 8, seed=seed, ret_interval=4),
              "ddim_from": eng.sample_chain_ddim(ctx, seg, [0, 2, 5], 0.5, seed=seed, ret_interval=4, x_init=x0, n_steps=8)}
    for name, (pred, traj) in chains.items():
        out[f"{name}/pred"] = pred
        if traj is not None:
            out[f"{name}/traj"] = traj           # every returned slot
    return out


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_inference_engine(prec):
    """prepare_shapes (the torch.empty context buffer: its three regions part [B][32], cpart [B][4][128] and the attention records up to
    dfx_shape_ctx_bytes; the 128 bytes of alignment padding between `part` and `cpart` at B = 3 belong to no region, are written by nobody
    and, as the identical results of every consumer below show, are read by nobody), denoise_eps / eps_t, q_sample, masked_mse, p_sample and the DDIM
    step with pred_xstart, sample_chain with and without snapshots, the DDIM chain, sample_chain_from with a held part, refine_chain and the
    DDIM chain from x_init: T = 12, B = 3, N = 288 (a full 256-point tile and a partial one), one shape with an absent part, one with a single
    part.  Every trajectory slot that is returned is compared.  The chain kernels take their step count and snapshot interval as
    arguments; nothing is read back from `traj` or `pred`."""
    eng = _engine(prec)
    three_modes(f"engine-{prec}", lambda alt: _engine_case(ENG_B, ENG_N, alt), lambda c: _engine_call(eng, c))


# ---- part sampling, part metrics, occupancy, batch assembly --------------------------------------------------------------------------
@pytest.mark.parametrize("path", [-1, 1], ids=["one_workgroup", "launch_per_pick"])
def test_part_sampling(path):
    """draw_stats, draw_normals, select_diverse, select_fit and select_diverse_global on both of its paths (dfx_debug_diverse_global_path),
    G = 3, K = 5, J = 4 with an absent part.  The global selection's workspace holds the rows' running minimum distances and pick flags,
    which its first step initialises; the pick loop runs to the argument P."""
    from difffacto_amd import part_sampling as psm
    G, K, J, P = 3, 5, 4, 4

    def prep(alt):
        rng = np.random.Generator(np.random.PCG64(60 + alt))
        f = lambda *s: cu(((4 if alt else 1) * rng.standard_normal(s)).astype(np.float32))
        valid = np.ones((G, J), np.float32)
        valid[2 if alt else 0, 0 if alt else 3] = 0
        return dict(mean=f(G * K, 3, J), logvar=cu((-2 + 0.3 * rng.standard_normal((G * K, 3, J))).astype(np.float32)), valid=cu(valid), tm=f(G, 3, J),
                    tl=cu((-2 + 0.3 * rng.standard_normal((G, 3, J))).astype(np.float32)), seed=11 + alt)

    def call(s):
        L = _lib()
        L.dfx_debug_diverse_global_path(path)
        try:
            out = {"stats": psm.draw_stats(G * K, J, s["seed"], row0=3, n_draws=64), "normals": psm.draw_normals(2, J, s["seed"], n_draws=8)}
            for name, d in (("diverse", psm.select_diverse(s["mean"], s["logvar"], s["valid"], K, P, seed=s["seed"], n_draws=64)),
                            ("global_farthest", psm.select_diverse_global(s["mean"], s["logvar"], s["valid"], K, P + 3, rule="farthest", seed=s["seed"], n_draws=64)),
                            ("global_first_pick", psm.select_diverse_global(s["mean"], s["logvar"], s["valid"], K, P + 3, rule="first_pick", stats=out["stats"])),
                            ("fit", psm.select_fit(s["mean"], s["logvar"], s["tm"], s["tl"], s["valid"], K))):
                out.update({f"{name}/{k}": v for k, v in d.items()})
            torch.cuda.synchronize()
        finally:
            L.dfx_debug_diverse_global_path(-1)
        return out
    three_modes(f"part_sampling-path{path}", prep, call)


def _labelled_clouds(B, N, alt, seed=5):
    rng = np.random.default_rng(seed + alt)
    clouds = [bc.box_cloud(rng, 4, [N // 4] * 4) for _ in range(B)]
    xyz = np.stack([c[0] for c in clouds]).astype(np.float32) * (4 if alt else 1)
    lab = np.stack([c[1] for c in clouds]).astype(np.int64)
    lab[B - 1 if alt else 0][lab[B - 1 if alt else 0] == 3] = 0        # one shape lacks part 3
    return xyz, lab


def test_part_metrics():
    """part_snapping (a pair with an absent part: status 0 and its distance cell), part_boxes (NaN boxes of absent parts), part_clouds (masks and
    zero rows behind a part's last point) and box_pairwise in its three metrics; B = 3, N = 400."""
    from difffacto_amd import evaluation as ev

    def prep(alt):
        xyz, lab = _labelled_clouds(3, 400, alt)
        return cu(xyz), cu(lab)

    def call(s):
        xyz, lab = s
        dist, status = ev.part_snapping(xyz, lab, [(0, 1), (1, 3), (2, 3)])
        boxes, count = ev.part_boxes(xyz, lab)
        clouds, masks, ccount = ev.part_clouds(xyz, lab, n_out=128)
        A = ev.BoxSet.from_counts(boxes, count)
        out = {"snap/dist": dist, "snap/status": status, "boxes": boxes, "count": count, "clouds": clouds, "masks": masks, "clouds_count": ccount}
        for metric in ("l2", "iou", "chamfer"):
            out[f"pairwise/{metric}"] = ev.box_pairwise(A, A, metric=metric, seed=3)
        return out
    three_modes("part_metrics-B3_N400", prep, call)


def test_occupancy():
    """occupancy_grid with labels and the cell index, added to an earlier call's counters (out=), the JSD of two rows and the entropy;
    resolution 8 in the sphere, B = 3, N = 400, one non-finite point for n_bad."""
    from difffacto_amd import evaluation as ev

    def prep(alt):
        xyz, lab = _labelled_clouds(3, 400, alt, seed=8)
        xyz = (xyz / (np.abs(xyz).max() * 2.2)).astype(np.float32)
        xyz[1 if alt else 2, 7] = np.nan
        return cu(xyz), cu(lab)

    def call(s):
        xyz, lab = s
        counters, bern, index, n_bad = ev.occupancy_grid(xyz, lab, n_class=4, resolution=8, return_index=True)
        out = {"counters": counters.clone(), "bernoulli": bern.clone(), "index": index, "n_bad": n_bad.clone()}
        c2, b2, _, nb2 = ev.occupancy_grid(xyz[:2], lab[:2], n_class=4, resolution=8, out=(counters, bern, n_bad))
        out.update({"added/counters": c2, "added/bernoulli": b2, "added/n_bad": nb2, "jsd": ev._device_jsd(c2[1].contiguous(), c2[2].contiguous())})
        ent, cnt = ev.entropy_of_occupancy_grid(xyz[:1], 8, in_sphere=True)      # (shape 0 is finite in both input sets)
        out.update({"entropy": torch.tensor(ent), "entropy_counters": torch.from_numpy(cnt)})
        return out
    three_modes("occupancy-B3_N400_R8", prep, call)


def test_batch_assembly():
    """PartCloudSet.draw and PartCloudSet.batch (dropout_part, augmentation), every tensor of the collated item; clouds of 40, 300 and 2700
    points, B = 4 with a repeated index, npoints = 256."""
    from difffacto_amd import data

    def prep(alt):
        rng = np.random.default_rng(alt)
        clouds = []
        for k in range(6):
            m = (40, 300, 2700)[k % 3]
            clouds.append(bc.box_cloud(rng, 4, np.bincount(rng.integers(0, 4, m - 4), minlength=4) + 1))
        return dict(ds=data.PartCloudSet.from_arrays(clouds, 4), index=[0, 2, 4, 0] if alt else [3, 5, 1, 3], seed=9 if alt else 5)

    def call(s):
        b = s["ds"].batch(s["index"], seed=s["seed"], npoints=256, dropout_part=0.3, augment=True)
        idx = torch.tensor(s["index"], device="cuda")
        choice, drop_u, aug_u = s["ds"].draw(idx, idx, s["seed"], 256)
        plain = s["ds"].batch(s["index"], seed=s["seed"], npoints=256)
        out = {k: v for k, v in b.items() if torch.is_tensor(v)}
        out.update({f"plain/{k}": v for k, v in plain.items() if torch.is_tensor(v)})
        out.update({"draw/choice": choice, "draw/drop_u": drop_u, "draw/aug_u": aug_u})
        return out
    three_modes("batch-B4_N256", prep, call)


# ---- library-owned workspaces: by sequence on one handle ------------------------------------------------------------------------------
def _sequence(what, make, run, small_x, small_y, large_y):
    """run(handle, inputs) -> {name: tensor}.  X on a fresh handle; then on one other handle Y, X, larger Y, X: X's bits every time."""
    fresh = snapshot(run(make(), small_x))
    h = make()
    run(h, small_y)
    d = first_difference(fresh, snapshot(run(h, small_x)))
    assert d is None, f"{what}: X after Y at the same shape differs from X on a fresh handle: {d}"
    run(h, large_y)
    d = first_difference(fresh, snapshot(run(h, small_x)))
    assert d is None, f"{what}: X after a larger shape on Y differs from X on a fresh handle: {d}"
    LINES.append(f"DIRTY sequence {what}: fresh == after Y == after larger Y: yes")
    print(LINES[-1], flush=True)


def test_sequence_sample_latents():
    run = lambda ls, x: ls.sample_latents(x["w_noise"], x["noise"], x["valid"], None, K=x["K"], npoints=9)
    _sequence("sample_latents tiny B 11 then 5", lambda: _sampler("tiny", fresh=True), run, _latent_prep("tiny", 5, False), _latent_prep("tiny", 5, True),
              _latent_prep("tiny", 11, True))


def test_sequence_general_set_abstraction():
    from difffacto_amd.pointnet2_ops.pointnet2_modules import PointnetSAModule
    make = lambda: _randomize(PointnetSAModule(npoint=37, radius=0.6, nsample=96, mlp=[4, 64, 64, 128]), 96).eval()

    def run(mod, s):
        with torch.no_grad():
            new_xyz = mod._centres(s["xyz"])
            return {"features": mod._forward_native(0, s["xyz"], new_xyz, s["feats"], force_general=True)}
    _sequence("general SA B 3 N 500 then B 2 N 400", make, run, _sa_prep(2, 400, 4, False), _sa_prep(2, 400, 4, True), _sa_prep(3, 500, 4, True))


def test_sequence_pointnet_v2_eval_forward():
    def run(enc, s):
        with torch.no_grad():
            m, v = enc(*s)
        return {"m": m, "v": v}
    _sequence("PointNetV2 eval B 5 N 333 then B 3 N 200", _pnv2_module, run, _pnv2_eval_inputs(3, 200, 8), _pnv2_eval_inputs(3, 200, 9, 4), _pnv2_eval_inputs(5, 333, 10, 4))


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_sequence_sample_chain(prec):
    def run(eng, c):
        ctx = eng.prepare_shapes(*c["latents"])
        pred, traj = eng.sample_chain(ctx, c["seg"], seed=c["seed"], ret_interval=4)
        return {"pred": pred, "traj": traj}
    _sequence(f"sample_chain {prec} B 6 then 3", lambda: _engine(prec, fresh=True), run, _engine_case(3, ENG_N, False), _engine_case(3, ENG_N, True),
              _engine_case(6, ENG_N, True))
