"""Training-mode denoiser on the HIP path: forward with saved activations, backward, loss gradient, Adam.

Tolerances (fp32 everywhere; the reductions over B*N rows run in a different order than torch's):
  gradients     5e-4 of the tensor's max-abs + 1e-7   (measured ~1e-5)
  eps / loss    2e-5 / 5e-6
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _train_case import GOLD, check_against_golden, load_case  # noqa: E402
from difffacto_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(case, with_flags=True, precision="f32", dropout=None, before_backward=None):
    from difffacto_amd import training
    dev = "cuda"
    P = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in case["W"].items()}
    cc = torch.from_numpy(case["ctx_code"]).to(dev).requires_grad_(True)
    cm = torch.from_numpy(case["ctx_mv"]).to(dev).requires_grad_(True)
    eps = training.denoiser_train_forward(P, torch.from_numpy(case["x_t"]).to(dev), torch.from_numpy(case["t"]).to(dev), cc, cm,
                                          torch.from_numpy(case["anchors_pt"]).to(dev), torch.from_numpy(case["variances_pt"]).to(dev),
                                          None if case["valid"] is None else torch.from_numpy(case["valid"]).to(dev),
                                          torch.from_numpy(case["assignment"]).to(dev), precision=precision, dropout=dropout)
    flags = torch.from_numpy(case["flags"]).to(dev) if with_flags and case["flags"] is not None else None
    loss = training.masked_mse(torch.from_numpy(case["noise"]).to(dev), eps, flags)
    if before_backward is not None:
        before_backward(eps)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), eps=eps.detach().cpu().numpy(), grads={k: v.grad.cpu().numpy() for k, v in P.items()},
                d_ctx_code=cc.grad.cpu().numpy(), d_ctx_mv=cm.grad.cpu().numpy(), params=P)


def test_forward_backward_vs_reference_autograd_golden():
    g, c = load_case("B3_N64_T10")
    r = _run(c)
    assert abs(r["loss"] - float(g["loss"])) < 5e-6, (r["loss"], float(g["loss"]))
    assert np.abs(r["eps"] - g["eps"]).max() < 2e-5
    n, worst = check_against_golden(g, r["grads"], rtol=5e-4, atol=1e-7)
    assert n == 77
    print(f"77 parameter gradients vs the reference's autograd: worst max-abs error / max-abs = {worst:.2e}")
    for k in ("d_ctx_code", "d_ctx_mv"):
        err = np.abs(r[k] - g[k]).max()
        assert err <= 5e-4 * np.abs(g[k]).max() + 1e-8, (k, err)


@pytest.mark.parametrize("B,N,all_valid,with_flags", [(2, 96, True, False), (5, 32, False, True), (1, 2048, False, True), (3, 100, False, True)])
def test_forward_backward_vs_oracle_full_gradients(B, N, all_valid, with_flags):
    """Every element of every gradient against oracle/train.py (pinned to the reference by the golden above) on seeded
    inputs of other shapes: ragged part validity, no flags, N = 2048, N = 100 (not a multiple of 32: padded on the host side)."""
    from difffacto_amd import synth
    from oracle import train
    rng = np.random.Generator(np.random.PCG64(100 + B + N))
    W = synth.make_denoiser_weights(3)
    pc, mean, logvar, valid = synth.make_latents(B, seed=7 + B, all_valid=all_valid)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32) if with_flags else None)
    ref = train.loss_and_grads(**c)
    r = _run(c, with_flags)
    assert abs(r["loss"] - ref["loss"]) < 5e-6 * max(1.0, abs(ref["loss"]))
    assert np.abs(r["eps"] - ref["eps"]).max() < 2e-5
    worst = 0.0
    for k, gr in ref["grads"].items():
        scale = max(np.abs(gr).max(), 1e-30)
        err = np.abs(r["grads"][k] - gr).max()
        assert err <= 5e-4 * scale + 1e-7, (k, err, scale)
        worst = max(worst, err / scale)
    for k in ("d_ctx_code", "d_ctx_mv"):
        assert np.abs(r[k] - ref[k]).max() <= 5e-4 * np.abs(ref[k]).max() + 1e-8, k
    print(f"B={B} N={N}: worst gradient error / max-abs = {worst:.2e}")


@pytest.mark.parametrize("tn,M,N,K,a_bf,b_bf", [(0, 300, 128, 128, 0, 0), (0, 1000, 1024, 128, 1, 0), (0, 512, 128, 1024, 1, 0),
                                               (1, 128, 128, 4100, 0, 0), (1, 1024, 128, 4100, 1, 1), (1, 128, 512, 9000, 0, 1),
                                               (1, 256, 256, 70, 1, 0), (1, 128, 128, 4100, 1, 1), (1, 128, 128, 64, 1, 0), (1, 128, 128, 64, 0, 1),
                                               (1, 256, 128, 64, 1, 0)])
def test_bf16_product_kernels_against_torch(tn, M, N, K, a_bf, b_bf):
    """gemm_bf16.h through its test hook: fp32 or bf16-stored operands, ragged row counts, several tiles per axis; the
    reference is a float64 product of the bf16-rounded operands (fp32 accumulation order differs: 2e-5 of the max-abs)."""
    from difffacto_amd import _ffi
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    rnd = lambda *s: torch.randn(*s, generator=g)
    if tn == 0:
        A, B = rnd(M, K), rnd(N, K)
        bias, resid = rnd(N), rnd(M, N)
    else:
        A, B = rnd(K, M), rnd(K, N)
        bias = resid = None
    Ar, Br = A.bfloat16().double(), B.bfloat16().double()
    ref = Ar @ Br.T + bias.double() + resid.double() if tn == 0 else Ar.T @ Br
    Ad = (A.bfloat16() if a_bf else A).cuda().contiguous()
    Bd = (B.bfloat16() if b_bf else B).cuda().contiguous()
    C = torch.empty(M, N, device="cuda")
    db = torch.empty(M, device="cuda") if tn else None
    ws = torch.empty((K // 64 + 1) * (M * N + M), device="cuda") if tn else None
    p = lambda t: None if t is None else t.data_ptr()
    bias_d = None if bias is None else bias.cuda()
    resid_d = None if resid is None else resid.cuda()
    rc = _ffi.lib().dfx_debug_gemm_bf16(tn, Ad.data_ptr(), Ad.shape[1], a_bf, Bd.data_ptr(), Bd.shape[1], b_bf, p(bias_d), p(resid_d),
                                       C.data_ptr(), p(db), p(ws), 0 if ws is None else ws.numel(), M, N, K, _ffi.current_stream())
    _ffi.check(rc, "dfx_debug_gemm_bf16")
    torch.cuda.synchronize()
    err = (C.cpu().double() - ref).abs().max().item()
    assert err < 2e-5 * ref.abs().max().item() + 1e-6, err
    if tn:
        col = (Ar if a_bf else A.double()).sum(0)     # column sums use the stored values (exact fp32 sums of fp32 inputs)
        assert (db.cpu().double() - col).abs().max().item() < 1e-4 * col.abs().max().item() + 1e-5


def test_bf16_matrix_products_within_stated_tolerance():
    """precision="bf16": the linear layers over the B*N points run on the bf16 matrix pipe (operands rounded to bf16, fp32
    accumulate).  Measured against the fp32 autograd oracle (profiles/r02_parity_headline.txt; deterministic kernels, the same on
    every box): loss 3.9e-6 relative (r03 box; 4.4e-7 in r02's log — the scalar sits at fp32 resolution), eps 2.2e-3 max-abs (|eps| ~ 1), worst gradient 5.8e-3 of its max-abs in max norm and 4.3e-3
    in relative L2.  Gates at 3x: 6.6e-3, 1.7e-2, 1.3e-2 (GPU-side bf16 rounding); the loss scalar is compared with a CPU-autograd
    oracle at fp32 resolution whose value moves with the host's BLAS and thread count (9x between two boxes): 1e-4."""
    from difffacto_amd import synth
    from oracle import train
    B, N = 2, 1024
    rng = np.random.Generator(np.random.PCG64(77))
    W = synth.make_denoiser_weights(3)
    pc, mean, logvar, valid = synth.make_latents(B, seed=9, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    ref = train.loss_and_grads(**c)
    r = _run(c, True, precision="bf16")
    f = _run(c, True, precision="f32")
    assert any(not np.array_equal(r["grads"][k], f["grads"][k]) for k in f["grads"]), "bf16 path not taken"
    assert abs(r["loss"] - ref["loss"]) < 1e-4 * abs(ref["loss"]), abs(r["loss"] - ref["loss"]) / abs(ref["loss"])
    assert np.abs(r["eps"] - ref["eps"]).max() < 6.6e-3, np.abs(r["eps"] - ref["eps"]).max()
    worst_max = worst_l2 = 0.0
    for k, gr in ref["grads"].items():
        scale = max(np.abs(gr).max(), 1e-30)
        e_max = np.abs(r["grads"][k] - gr).max() / scale
        e_l2 = np.linalg.norm((r["grads"][k] - gr).ravel()) / max(np.linalg.norm(gr.ravel()), 1e-30)
        assert e_max < 1.7e-2 and e_l2 < 1.3e-2, (k, e_max, e_l2)
        worst_max, worst_l2 = max(worst_max, e_max), max(worst_l2, e_l2)
    print(f"bf16 products: loss rel err {abs(r['loss'] - ref['loss']) / abs(ref['loss']):.1e}, eps max-abs {np.abs(r['eps'] - ref['eps']).max():.1e}, "
          f"gradients worst max-norm {worst_max:.1e}, worst relative L2 {worst_l2:.1e}")


@pytest.mark.parametrize("dropout", [None, (0.2, 777)], ids=["p0", "p0.2"])
@pytest.mark.parametrize("B,N", [(2, 1024), (3, 160), (1, 4096)])
def test_fused_feed_forward_matches_the_layer_by_layer_bf16_path(B, N, dropout, g_max=2e-2, g_l2=1.3e-2):
    """train_ff_fused.h (one kernel per direction for the GEGLU feed-forward: [a | g] and hid stay in registers, recomputed in
    the backward) against the layer-by-layer bf16 kernels it replaces: same bf16 operands; differences = fp32 summation order,
    the fast sigmoid-form GELU (2.7e-4) instead of erf, and [a | g] no longer rounded to bf16 between forward and backward.
    Both must sit inside the stated bf16 tolerance against the fp32 oracle; here they are compared with each other.
    N = 160: a workgroup's trailing wavefronts fall off the end of the rows (ragged last tile).
    dropout = (0.2, seed) — the shipped train_chair_stage1.py setting: the fused kernels draw the SAME Philox factors (dfx_dropout.h: keyed by
    (seed, site, element)) as the layer-by-layer kernels — forward in k_ff<false, true>, kept as one bit per element for k_ff<true, true> and
    k_ff_wgrad<true> — so the two paths must agree within the same gates as without dropout."""
    from difffacto_amd import _ffi, synth
    rng = np.random.Generator(np.random.PCG64(B * 1000 + N))
    W = synth.make_denoiser_weights(5)
    pc, mean, logvar, valid = synth.make_latents(B, seed=11, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    fused = _run(c, True, precision="bf16", dropout=dropout)
    _ffi.lib().dfx_debug_train_fused(0)
    try:
        layer = _run(c, True, precision="bf16", dropout=dropout)
    finally:
        _ffi.lib().dfx_debug_train_fused(1)
    assert any(not np.array_equal(fused["grads"][k], layer["grads"][k]) for k in layer["grads"]), "fused path not taken"
    if dropout is not None:   # dropout did something, and a different seed gives different factors on the fused path
        plain = _run(c, True, precision="bf16")
        other = _run(c, True, precision="bf16", dropout=(dropout[0], dropout[1] + 1))
        # (on eps, not on the scalar loss: two dropout patterns can land on the same loss to five digits — tools/fuzz_parity.py found B = 5, N = 160, seed 717135)
        assert np.abs(plain["eps"] - fused["eps"]).max() > 1e-3 and np.abs(other["eps"] - fused["eps"]).max() > 1e-3
    e_eps = np.abs(fused["eps"] - layer["eps"]).max()
    worst_max = worst_l2 = 0.0
    for k, gr in layer["grads"].items():
        scale = max(np.abs(gr).max(), 1e-30)
        e_max = np.abs(fused["grads"][k] - gr).max() / scale
        e_l2 = np.linalg.norm((fused["grads"][k] - gr).ravel()) / max(np.linalg.norm(gr.ravel()), 1e-30)
        worst_max, worst_l2 = max(worst_max, e_max), max(worst_l2, e_l2)
        # measured worst over the three shapes (r03 box; `transformer_blocks.1.norm2.weight`): 6.7e-3 of max-abs / 4.4e-3 relative L2 -> gates at 3x
        # (tools/fuzz_parity.py, round 6, 5.6 k random shapes: 0.2 % of the DROPOUT cases exceed these gates — small tensors of runs with <= 1 k points,
        # worst 3.8e-2 of max-abs; the same rate with round 5's forward, 15 / 5465 against 12 / 5648: the sweep passes g_max = 4e-2, g_l2 = 3e-2 for them)
        assert e_max < g_max and e_l2 < g_l2, (k, e_max, e_l2)
    print(f"fused vs layer-by-layer FF (B={B}, N={N}, dropout={dropout}): loss {fused['loss']:.6f} / {layer['loss']:.6f}, eps max-abs {e_eps:.1e}, "
          f"gradients worst max-norm {worst_max:.1e}, worst relative L2 {worst_l2:.1e}")
    # measured over the three shapes here and ~120 random ones (tools/fuzz_parity.py, r03): loss up to 1.9e-4 relative, eps up to 3.3e-3 -> 3x
    e_loss = abs(fused["loss"] - layer["loss"]) / abs(layer["loss"])
    assert e_loss < 6e-4 and e_eps < 1e-2, (e_loss, e_eps)


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_fused_path_at_other_depths(depth):
    """The fused backward passes the gradient between the blocks through two alternating buffers (bf16-pair tiles; the head writes the
    first, block 0 hands fp32 rows to the stem — in w.dh or w.dh2 depending on the depth's parity) and batches the finishing kernels over the
    blocks: depths 1, 2 and 4 (the shipped network has 5) against the layer-by-layer bf16 kernels, the gates of the depth-5 test."""
    from difffacto_amd import _ffi, synth
    B, N = 2, 224
    rng = np.random.Generator(np.random.PCG64(600 + depth))
    W = synth.make_denoiser_weights(8, depth=depth)
    pc, mean, logvar, valid = synth.make_latents(B, seed=23, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    fused = _run(c, True, precision="bf16")
    _ffi.lib().dfx_debug_train_fused(0)
    try:
        layer = _run(c, True, precision="bf16")
    finally:
        _ffi.lib().dfx_debug_train_fused(1)
    assert set(fused["grads"]) == set(layer["grads"]) and any(not np.array_equal(fused["grads"][k], layer["grads"][k]) for k in layer["grads"])
    e_eps = np.abs(fused["eps"] - layer["eps"]).max()
    worst, at = 0.0, None
    for k, gr in layer["grads"].items():
        e = np.abs(fused["grads"][k] - gr).max() / max(np.abs(gr).max(), 1e-30)
        if e > worst:
            worst, at = e, k
    print(f"depth {depth}: fused vs layer-by-layer eps max-abs {e_eps:.1e}, gradients worst max-norm {worst:.1e} ({at})")
    assert e_eps < 1e-2 and worst < 2e-2, (e_eps, worst, at)


def test_layernorm3_fold_with_awkward_affine_parameters():
    """Round 5: the fused kernels fold LayerNorm3's affine into W1 / b1 (W1 diag(g3), b1 + W1 b3) and take d gamma3 / d beta3 / dW1 from the
    weight-gradient side (G = d[a|g]^T xhat3: dW1 = G diag(g3) + db1 (x) b3, d gamma3 = sum_o W1 o G, d beta3 = sum_o W1[o][.] db1[o]).
    Nothing divides by gamma: exact zeros, sign changes and large entries in gamma3 / beta3 must give the same gradients as the fp32 autograd
    oracle within the bf16 gates of test_bf16_matrix_products_within_stated_tolerance (the awkward entries make |xn3| larger, so the gates
    are the same 3x-measured ones: eps 6.6e-3, gradients 1.7e-2 max-norm) — including d gamma3 at the channels where gamma3 = 0."""
    from difffacto_amd import synth
    from oracle import train
    B, N = 2, 512
    rng = np.random.Generator(np.random.PCG64(515))
    W = {k: v.copy() for k, v in synth.make_denoiser_weights(3).items()}
    for i in range(5):
        g, b = W[f"transformer_blocks.{i}.norm3.weight"], W[f"transformer_blocks.{i}.norm3.bias"]
        g[rng.choice(128, 12, replace=False)] = 0.0
        g[rng.choice(128, 12, replace=False)] *= -1.0
        g[rng.choice(128, 4, replace=False)] *= 3.0
        b[rng.choice(128, 8, replace=False)] = 0.0
        b[rng.choice(128, 8, replace=False)] += 0.5
    pc, mean, logvar, valid = synth.make_latents(B, seed=19, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    ref = train.loss_and_grads(**c)
    r = _run(c, True, precision="bf16")
    e_eps = np.abs(r["eps"] - ref["eps"]).max()
    worst, at = 0.0, None
    for k, gr in ref["grads"].items():
        e = np.abs(r["grads"][k] - gr).max() / max(np.abs(gr).max(), 1e-30)
        if e > worst:
            worst, at = e, k
    z = [np.abs(r["grads"][f"transformer_blocks.{i}.norm3.weight"] - ref["grads"][f"transformer_blocks.{i}.norm3.weight"])[W[f"transformer_blocks.{i}.norm3.weight"] == 0].max()
         / np.abs(ref["grads"][f"transformer_blocks.{i}.norm3.weight"]).max() for i in range(5)]
    print(f"LayerNorm3 fold, awkward gamma3 / beta3: eps max-abs {e_eps:.1e}, gradients worst max-norm {worst:.1e} ({at}), d gamma3 where gamma3 = 0: {max(z):.1e}")
    assert e_eps < 6.6e-3 and worst < 1.7e-2 and max(z) < 1.7e-2, (e_eps, worst, at, z)


def test_fused_training_step_is_bit_reproducible():
    """No atomics anywhere in the fused path (column sums through LDS tiles in fixed order, per-slab / per-shape partials summed in
    order): two runs of the same iteration give bit-identical eps and gradients."""
    from difffacto_amd import synth
    B, N = 4, 1024
    rng = np.random.Generator(np.random.PCG64(99))
    W = synth.make_denoiser_weights(2)
    pc, mean, logvar, valid = synth.make_latents(B, seed=21, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    a = _run(c, True, precision="bf16")
    b = _run(c, True, precision="bf16")
    assert np.array_equal(a["eps"], b["eps"])
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k], b["grads"][k]), k


def test_backward_follows_the_forwards_record_not_the_live_switch():
    """The path is planned once, by the forward, and kept per workspace (csrc/train_plan.h, PathRecord): flipping dfx_debug_train_fused(0)
    between a default forward and its backward changes nothing — every gradient is the same bits as an untoggled step's — and a backward
    called with the other precision is refused with the record's values.  B = 2, N = 128: 256 rows, the smallest shape on the fused path."""
    from difffacto_amd import _ffi, synth
    B, N = 2, 128
    rng = np.random.Generator(np.random.PCG64(256))
    W = synth.make_denoiser_weights(4)
    pc, mean, logvar, valid = synth.make_latents(B, seed=27, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    L = _ffi.lib()
    plain = _run(c, True, precision="bf16")
    assert L.dfx_debug_last_train_path() == b"fused_bf16"
    try:
        flipped = _run(c, True, precision="bf16", before_backward=lambda eps: L.dfx_debug_train_fused(0))
    finally:
        L.dfx_debug_train_fused(1)
    assert L.dfx_debug_last_train_path() == b"fused_bf16"
    assert flipped["loss"] == plain["loss"] and np.array_equal(flipped["eps"], plain["eps"])
    assert set(flipped["grads"]) == set(plain["grads"]) and len(plain["grads"]) == 77
    for k in plain["grads"]:
        assert np.array_equal(flipped["grads"][k], plain["grads"][k]), k
    assert np.array_equal(flipped["d_ctx_code"], plain["d_ctx_code"]) and np.array_equal(flipped["d_ctx_mv"], plain["d_ctx_mv"])

    def other_precision(eps):
        assert eps.grad_fn.prec == _ffi.DFX_PREC_BF16
        eps.grad_fn.prec = _ffi.DFX_PREC_F32
    with pytest.raises(RuntimeError, match=r"the forward of this workspace ran with precision 1, dropout 0, B 2, N 128"):
        _run(c, True, precision="bf16", before_backward=other_precision)


@pytest.mark.parametrize("B,N", [(4, 1024), (3, 160), (16, 2048)])
def test_side_stream_training_step_is_bit_identical_to_the_single_stream_one(B, N):
    """The fused path forks its context branch (forward) and its parameter-gradient reductions (backward: head / stem partial sums in
    buffers of their own, the finishing kernels' leaves) onto the device's side stream and joins before it returns
    (dfx_debug_train_streams, default on).  Same kernels, operands and summation orders: eps, loss and every gradient are the same
    bits as with every launch on the caller's stream — also when the call itself runs on a non-default torch stream, and three times in
    a row (the event ring, buffers written by one iteration's side work and read by the next)."""
    import torch
    from difffacto_amd import _ffi, synth
    rng = np.random.Generator(np.random.PCG64(77 + B))
    W = synth.make_denoiser_weights(3)
    pc, mean, logvar, valid = synth.make_latents(B, seed=31, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    _ffi.lib().dfx_debug_train_streams(0)
    try:
        one = _run(c, True, precision="bf16")
    finally:
        _ffi.lib().dfx_debug_train_streams(1)
    runs = [_run(c, True, precision="bf16") for _ in range(3)]
    with torch.cuda.stream(torch.cuda.Stream()):
        runs.append(_run(c, True, precision="bf16"))
    torch.cuda.synchronize()
    for two in runs:
        assert two["loss"] == one["loss"]
        assert np.array_equal(two["eps"], one["eps"])
        for k in one["grads"]:
            assert np.array_equal(two["grads"][k], one["grads"][k]), k
        assert np.array_equal(two["d_ctx_code"], one["d_ctx_code"]) and np.array_equal(two["d_ctx_mv"], one["d_ctx_mv"])


def test_dropout_training_step_is_bit_reproducible_on_a_full_chip():
    """Round 6 regression: the backward dX kernel fetches each chunk pair's dropout bit word with an asynchronous load that sits among the
    LDS-DMA pieces of the weight ring; the counted wait that was meant to cover it (loads complete in order) does not: a load that returns to a
    register and LDS-DMA loads complete out of order against each other once the chip is busy, and the word was occasionally stale — every
    gradient below the last block differed by ~2e-3 from run to run at B >= 16 x 2048 (small shapes never showed it: the round-5 tests passed).
    The word is now waited for with vmcnt(0).  Five runs of one iteration with Dropout(0.2), >= 1024 workgroups, in both stream modes: same bits."""
    from difffacto_amd import _ffi, synth
    B, N = 64, 2048
    rng = np.random.Generator(np.random.PCG64(5))
    W = synth.make_denoiser_weights(1)
    pc, mean, logvar, valid = synth.make_latents(B, seed=13, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32), flags=None)
    try:
        for streams in (0, 1):
            _ffi.lib().dfx_debug_train_streams(streams)
            runs = [_run(c, False, precision="bf16", dropout=(0.2, 4242)) for _ in range(5)]
            if streams == 0:
                one = runs[0]
            for two in runs:
                assert two["loss"] == one["loss"]
                assert np.array_equal(two["eps"], one["eps"])
                for k in one["grads"]:
                    assert np.array_equal(two["grads"][k], one["grads"][k]), (streams, k)
                assert np.array_equal(two["d_ctx_code"], one["d_ctx_code"]) and np.array_equal(two["d_ctx_mv"], one["d_ctx_mv"])
    finally:
        _ffi.lib().dfx_debug_train_streams(1)


def test_training_step_with_its_side_stream_is_capturable_as_one_hip_graph():
    """The fork / join onto libdfx's side stream inside dfx_denoiser_train_backward uses plain event record / wait pairs, so a stream capture of
    the caller's stream (torch.cuda.graph) takes the side work into the same graph: forward + loss + backward captured once, replayed twice,
    gives the eager call's bits."""
    import torch
    from difffacto_amd import synth, training
    B, N = 4, 1024
    rng = np.random.Generator(np.random.PCG64(123))
    W = synth.make_denoiser_weights(3)
    pc, mean, logvar, valid = synth.make_latents(B, seed=41, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = {k: cu(v).requires_grad_(True) for k, v in W.items()}
    args = [cu((anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32)), cu(rng.integers(0, 1000, size=(B,)).astype(np.int32)), cu(pc),
            cu(np.concatenate([mean, var], 1).astype(np.float32)), cu(anc.transpose(0, 2, 1)), cu(vr.transpose(0, 2, 1)), cu(valid), cu(seg.astype(np.int32))]
    noise = cu(rng.standard_normal((B, 3, N)).astype(np.float32))

    def step():
        for p in P.values():
            p.grad = None
        loss = training.masked_mse(noise, training.denoiser_train_forward(P, *args, precision="bf16"), None)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):   # warm-up: lazy initialisation (LDS attributes, the side stream and its events) must not happen under capture
            eager_loss = step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = {k: p.grad.clone() for k, p in P.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap_loss = step()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert float(cap_loss.detach()) == float(eager_loss.detach())
    for k, p in P.items():
        assert torch.equal(p.grad, eager[k]), k


def test_dropout_factors_and_replayed_mask_parity():
    """Dropout of train() mode: (i) the Philox factors are 0 or 1/(1-p) with the right frequency and differ between sites and
    seeds; (ii) forward + backward with dropout agree with torch autograd when the SAME factors are replayed into the
    torch-CPU oracle at the reference's dropout sites (behind to_out, behind the GEGLU, time_embed included)."""
    from difffacto_amd import synth, training
    from oracle import train
    p, seed = 0.2, 123456789
    f = training.dropout_factors(seed, 3, p, 1 << 20).cpu().numpy()
    assert set(np.unique(f)) == {0.0, np.float32(1.0 / (1.0 - p))}
    assert abs((f == 0).mean() - p) < 3e-3
    assert not np.array_equal(f, training.dropout_factors(seed, 5, p, 1 << 20).cpu().numpy())
    assert not np.array_equal(f, training.dropout_factors(seed + 1, 3, p, 1 << 20).cpu().numpy())
    B, N = 2, 96
    rng = np.random.Generator(np.random.PCG64(5))
    W = synth.make_denoiser_weights(3)
    pc, mean, logvar, valid = synth.make_latents(B, seed=4, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
             ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
             anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
             valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
             flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))
    drops = {"te": training.dropout_factors(seed, 1000, p, B * 1024).cpu().numpy().reshape(B, 1024)}
    for i in range(5):
        drops[("attn", i)] = training.dropout_factors(seed, 2 * i, p, B * N * 128).cpu().numpy().reshape(B, N, 128)
        drops[("ff", i)] = training.dropout_factors(seed, 2 * i + 1, p, B * N * 512).cpu().numpy().reshape(B, N, 512)
    ref = train.loss_and_grads(**c, drops=drops)
    r = _run(c, True, dropout=(p, seed))
    r0 = _run(c, True)
    assert abs(r["loss"] - r0["loss"]) > 1e-3                      # dropout did something
    assert abs(r["loss"] - ref["loss"]) < 5e-6 * max(1.0, abs(ref["loss"]))
    assert np.abs(r["eps"] - ref["eps"]).max() < 3e-5
    for k, gr in ref["grads"].items():
        scale = max(np.abs(gr).max(), 1e-30)
        assert np.abs(r["grads"][k] - gr).max() <= 5e-4 * scale + 1e-7, k
    for k in ("d_ctx_code", "d_ctx_mv"):
        assert np.abs(r[k] - ref[k]).max() <= 5e-4 * np.abs(ref[k]).max() + 1e-8, k


def _seeded_case(B, N, wseed, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    W = synth.make_denoiser_weights(wseed)
    pc, mean, logvar, valid = synth.make_latents(B, seed=seed % 97 + 1, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    return dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
                ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
                anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
                valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
                flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))


def replayed_drops(seed, p, B, N, depth=5):
    """The factors the HIP kernels draw (dfx_dropout.h: Philox keyed by (seed, site, element group)) in the shapes oracle/train.py replays
    them at the reference's dropout sites: behind to_out (attention.py:84), behind the GEGLU (attention.py:177), time_embed."""
    from difffacto_amd import training
    drops = {"te": training.dropout_factors(seed, 1000, p, B * 1024).cpu().numpy().reshape(B, 1024)}
    for i in range(depth):
        drops[("attn", i)] = training.dropout_factors(seed, 2 * i, p, B * N * 128).cpu().numpy().reshape(B, N, 128)
        drops[("ff", i)] = training.dropout_factors(seed, 2 * i + 1, p, B * N * 512).cpu().numpy().reshape(B, N, 512)
    return drops


@pytest.mark.parametrize("path", ["fused", "layer"])
@pytest.mark.parametrize("B,N", [(2, 1024), (3, 160), (1, 4096)])
def test_bf16_dropout_paths_against_the_oracle_with_replayed_factors(B, N, path, g_max=1.7e-2, g_l2=1.3e-2):
    """config 5 AS SHIPPED (train_chair_stage1.py:38: Dropout 0.2, bf16 products) compared with the fp32 torch-autograd
    oracle DIRECTLY — not through another HIP path.  The Philox factors of (p, seed) are replayed into oracle/train.py at the reference's sites;
    `fused` = k_ff_fwd_chain / k_ff<true, true> / k_ff_wgrad<true> (1 / (1 - p) folded into the `a` half of the packed W1, one-bit masks,
    masks re-gathered in the transposed orientation by the weight-gradient kernel), `layer` = the layer-by-layer bf16 kernels (the middle
    link of the old chain of comparisons).  The path is asserted from the library's own record (dfx_debug_last_train_path).
    Gates = the p = 0 gates of test_bf16_matrix_products_within_stated_tolerance (3x the measured p = 0 values: eps 6.6e-3 max-abs,
    gradients 1.7e-2 of max-abs / 1.3e-2 relative L2) — dropout scales activations by at most 1.25 and zeroes the rest, it does not
    widen the bf16 rounding; measured values are printed (profiles/r06_parity_prints.txt).  The random-shape sweep (tools/fuzz_parity.py, 169 cases)
    found the tail of BOTH bf16 paths above these one-shape gates on small tensors (bias / LayerNorm vectors, to_k): worst 3.1e-2 of max-abs, 2.4e-2
    relative L2 — it runs with g_max = 5e-2, g_l2 = 4e-2 (profiles/r06_fuzz_train.txt).  That tail is neither explained nor confirmed yet: tests/test_gpu_train_highprec.py
    judges both bf16 paths against a rounding model of the same inputs instead of one number for all tensors, and on its shapes (256 to 6144 rows) the small tensors sit within
    1.07 x rms / 1.21 x max-abs of the model when pooled, the model's own worst max-abs error on a 128-vector or a to_k being 7.3e-3 of max-abs; no shape of the sweep's tail
    (<= 1 k points, other seeds) has been judged that way."""
    from difffacto_amd import _ffi
    from oracle import train
    p, seed = 0.2, 20260930 + B * 7 + N
    c = _seeded_case(B, N, wseed=3, seed=900 + B * 31 + N)
    ref = train.loss_and_grads(**c, drops=replayed_drops(seed, p, B, N))
    ref0 = train.loss_and_grads(**c)
    _ffi.lib().dfx_debug_train_fused(1 if path == "fused" else 0)
    try:
        r = _run(c, True, precision="bf16", dropout=(p, seed))
        took = _ffi.lib().dfx_debug_last_train_path().decode()
    finally:
        _ffi.lib().dfx_debug_train_fused(1)
    assert took == ("fused_bf16_dropout" if path == "fused" else "layer_bf16_dropout"), took
    assert np.abs(ref["eps"] - ref0["eps"]).max() > 1e-2        # the replayed factors did something in the oracle
    e_loss = abs(r["loss"] - ref["loss"]) / abs(ref["loss"])
    e_eps = np.abs(r["eps"] - ref["eps"]).max()
    worst_max = worst_l2 = 0.0
    at = None
    for k, gr in ref["grads"].items():
        scale = max(np.abs(gr).max(), 1e-30)
        e_max = np.abs(r["grads"][k] - gr).max() / scale
        e_l2 = np.linalg.norm((r["grads"][k] - gr).ravel()) / max(np.linalg.norm(gr.ravel()), 1e-30)
        if e_max > worst_max:
            worst_max, at = e_max, k
        worst_l2 = max(worst_l2, e_l2)
    e_ctx = max(np.abs(r[k] - ref[k]).max() / np.abs(ref[k]).max() for k in ("d_ctx_code", "d_ctx_mv"))
    print(f"bf16 + dropout 0.2, {took} (B={B}, N={N}) vs fp32 autograd oracle with replayed factors: loss rel {e_loss:.1e}, eps max-abs {e_eps:.1e}, "
          f"gradients worst max-norm {worst_max:.1e} ({at}), worst relative L2 {worst_l2:.1e}, d ctx {e_ctx:.1e}")
    assert e_loss < 1e-3 and e_eps < 6.6e-3, (e_loss, e_eps)
    assert worst_max < g_max and worst_l2 < g_l2 and e_ctx < g_max, (worst_max, at, worst_l2, e_ctx)


def test_smallest_shapes_and_no_validity_mask():
    """B = 1, N = 32 (one attention block, one product slab) with valid = None (all parts present), no flags, both precisions'
    code paths: against the oracle."""
    from difffacto_amd import synth
    from oracle import train
    rng = np.random.Generator(np.random.PCG64(1))
    B, N = 1, 32
    W = synth.make_denoiser_weights(5)
    pc, mean, logvar, _ = synth.make_latents(B, seed=3, all_valid=True)
    seg = rng.integers(0, 4, size=(B, N)).astype(np.int32)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    c = dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=np.array([999], np.int64), ctx_code=pc,
             ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32), anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)),
             variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)), valid=None, assignment=seg,
             noise=rng.standard_normal((B, 3, N)).astype(np.float32), flags=None)
    ref = train.loss_and_grads(**c)
    for prec in ("f32", "bf16"):       # bf16 falls back to the fp32 kernels below 256 rows: same numbers
        r = _run(c, False, precision=prec)
        assert abs(r["loss"] - ref["loss"]) < 5e-6 * max(1.0, abs(ref["loss"]))
        for k, gr in ref["grads"].items():
            assert np.abs(r["grads"][k] - gr).max() <= 5e-4 * max(np.abs(gr).max(), 1e-30) + 1e-7, (prec, k)


def test_adam_with_clipping_matches_torch():
    """Three steps of dfx Adam + clip_grad_norm_(max_norm) against torch.optim.Adam + torch.nn.utils.clip_grad_norm_ on
    the CPU (what Runner.train does, runner.py:312-316), on tensors of awkward sizes."""
    from difffacto_amd import training
    rng = np.random.Generator(np.random.PCG64(5))
    shapes = [(1024, 128), (3,), (128, 522), (77,)]
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    ref = [torch.from_numpy(a.copy()).requires_grad_(True) for a in p0]
    mine = [torch.from_numpy(a.copy()).cuda() for a in p0]
    opt_ref = torch.optim.Adam(ref, lr=2e-3, betas=(0.9, 0.999), eps=1e-8)
    opt = training.Adam(mine, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=10.0)
    for step in range(3):
        gs = [(rng.standard_normal(s) * (30.0 if step == 0 else 0.01)).astype(np.float32) for s in shapes]   # step 0 clips
        for p, g in zip(ref, gs):
            p.grad = torch.from_numpy(g.copy())
        for p, g in zip(mine, gs):
            p.grad = torch.from_numpy(g.copy()).cuda()
        n_ref = torch.nn.utils.clip_grad_norm_(ref, 10.0)
        opt_ref.step()
        n = opt.step()
        assert abs(float(n) - float(n_ref)) <= 1e-5 * float(n_ref)
        for a, b in zip(mine, ref):
            assert np.abs(a.cpu().numpy() - b.detach().numpy()).max() < 2e-6


def test_training_steps_reduce_the_loss():
    """Five optimiser steps on one fixed batch through the autograd functions: the masked MSE goes down."""
    from difffacto_amd import training
    g, c = load_case("B3_N64_T10")
    dev = "cuda"
    P = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in c["W"].items()}
    opt = training.Adam(list(P.values()), lr=1e-3, max_norm=10.0)
    args = [torch.from_numpy(c[k]).to(dev) for k in ("x_t", "t", "ctx_code", "ctx_mv", "anchors_pt", "variances_pt", "valid", "assignment")]
    noise, flags = torch.from_numpy(c["noise"]).to(dev), torch.from_numpy(c["flags"]).to(dev)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = training.masked_mse(noise, training.denoiser_train_forward(P, *args), flags)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] and all(np.isfinite(losses)), losses
    assert opt.last_step_was_flat   # the backward leaves the gradients in one buffer: clip + Adam are one launch each


def test_train_entry_points_reject_bad_arguments():
    from difffacto_amd import _ffi
    lib = _ffi.lib()
    assert lib.dfx_denoiser_train_workspace_bytes(0, 64, 5) == 0
    assert lib.dfx_denoiser_train_workspace_bytes(2, 64, 5) > 0
    w = _ffi.DenoiserWeights()
    w.depth = 5
    rc = lib.dfx_denoiser_train_forward(w, None, 0, None, None, None, None, None, None, None, None, None, 2, 64, 0, 0.0, 0, None)
    assert rc != 0 and b"null" in lib.dfx_last_error()


def test_module_api_training_losses_backward_like_the_reference():
    """The reference's call sequence (anchor_gen.py:1020, runner.py:312-316) through the drop-in modules: train() mode,
    diffusion.training_losses(...)['mse_loss'].backward(), clip + Adam — parameter gradients against the golden."""
    from difffacto_amd import training
    from difffacto_amd.modules import AnchoredDiffusion
    from test_modules_cpu import DIFF_CFG
    g, c = load_case("B3_N64_T10")
    net = dict(DIFF_CFG["net"], dropout=0.0)
    d = AnchoredDiffusion(num_timesteps=10, precision="f32", **{**DIFF_CFG, "net": net})
    d.model.load_state_dict({k: torch.from_numpy(v) for k, v in c["W"].items()})
    d = d.cuda().train()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = [cu(c["ctx_code"]).requires_grad_(True), cu(c["ctx_mv"]).requires_grad_(True)]
    anchors, variance = cu(c["anchors_pt"].transpose(0, 2, 1)), cu(c["variances_pt"].transpose(0, 2, 1))     # (B,3,N)
    r = d.training_losses(cu(g["x_start"]), cu(g["t"]), anchors=anchors, variance=variance, ctx=ctx, anchor_assignment=cu(c["assignment"]),
                          valid_id=cu(c["valid"]), flags=cu(c["flags"]), noise=cu(c["noise"]))
    loss = r["mse_loss"]
    assert abs(float(loss.detach()) - float(g["loss"])) < 5e-6
    loss.backward()
    grads = {k: p.grad.cpu().numpy() for k, p in d.model.named_parameters()}
    n, worst = check_against_golden(g, grads, rtol=5e-4, atol=1e-7)
    assert n == 77
    assert np.abs(ctx[0].grad.cpu().numpy() - g["d_ctx_code"]).max() <= 5e-4 * np.abs(g["d_ctx_code"]).max() + 1e-8
    opt = training.Adam(list(d.model.parameters()), lr=1e-3, max_norm=10.0)
    before = d.model.proj_out.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, d.model.proj_out.weight.detach())
    # dropout > 0 in train() mode: libdfx's Philox dropout; the loss differs from the p = 0 value and from step to step,
    # and is reproducible under torch.manual_seed
    d2 = AnchoredDiffusion(num_timesteps=10, precision="f32", **{**DIFF_CFG, "net": dict(DIFF_CFG["net"], dropout=0.2)})
    d2.model.load_state_dict({k: torch.from_numpy(v) for k, v in c["W"].items()})
    d2 = d2.cuda().train()
    args = dict(anchors=anchors, variance=variance, ctx=ctx, anchor_assignment=cu(c["assignment"]), valid_id=cu(c["valid"]),
                flags=cu(c["flags"]), noise=cu(c["noise"]))
    torch.manual_seed(7)
    l1 = float(d2.training_losses(cu(g["x_start"]), cu(g["t"]), **args)["mse_loss"].detach())
    l2 = float(d2.training_losses(cu(g["x_start"]), cu(g["t"]), **args)["mse_loss"].detach())
    torch.manual_seed(7)
    l1b = float(d2.training_losses(cu(g["x_start"]), cu(g["t"]), **args)["mse_loss"].detach())
    assert l1 == l1b and l1 != l2 and abs(l1 - float(g["loss"])) > 1e-4 and np.isfinite([l1, l2]).all()


def test_inference_engine_follows_the_weights_across_adam_steps():
    """training.Adam writes parameters through raw pointers (no torch version bump); the packed-weight cache of
    TransformerNet.engine() must still notice.  train -> validate -> train -> validate: every engine().eps after a step equals
    a freshly built engine on the current weights and differs from the previous one.  A second backward through one forward
    (released workspace) raises instead of reading freed memory."""
    from difffacto_amd import training
    from difffacto_amd.engine import DenoiserEngine
    from difffacto_amd.modules import AnchoredDiffusion
    from test_modules_cpu import DIFF_CFG
    g, c = load_case("B3_N64_T10")
    d = AnchoredDiffusion(num_timesteps=10, precision="f32", **{**DIFF_CFG, "net": dict(DIFF_CFG["net"], dropout=0.0)})
    d.model.load_state_dict({k: torch.from_numpy(v) for k, v in c["W"].items()})
    d = d.cuda().train()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = [cu(c["ctx_code"]), cu(c["ctx_mv"])]
    anchors, variance = cu(c["anchors_pt"].transpose(0, 2, 1)), cu(c["variances_pt"].transpose(0, 2, 1))
    seg, valid, x = cu(c["assignment"]), cu(c["valid"]), cu(g["x_start"])
    opt = training.Adam(list(d.model.parameters()), lr=5e-2, max_norm=10.0)

    def validate():
        with torch.no_grad():
            return d.model.engine().eps(d.model.shape_context(ctx, valid), x, seg, 3).clone()

    prev = validate()
    for it in range(3):
        opt.zero_grad()
        loss = d.training_losses(x, cu(g["t"]), anchors=anchors, variance=variance, ctx=ctx, anchor_assignment=seg, valid_id=valid,
                                 flags=cu(c["flags"]), noise=cu(c["noise"]))["mse_loss"]
        loss.backward()
        if it == 0:
            with pytest.raises(RuntimeError, match="ran twice"):
                loss.backward()
        opt.step()
        cur = validate()
        fresh = DenoiserEngine({k: v.detach() for k, v in d.model.named_parameters()}, 10, precision="f32")
        ref = fresh.eps(fresh.prepare_shapes(ctx[0], ctx[1][:, :3], ctx[1][:, 3:], valid), x, seg, 3)
        fresh.close()
        assert torch.equal(cur, ref), it
        assert (cur - prev).abs().max().item() > 1e-4, it
        prev = cur


def test_training_loop_over_iterations_matches_the_reference_loop():
    """tests/golden/train_loop_B3_N64_T10.npz: three iterations of the reference's loop (runner/runner.py:299-316: zero_grad ->
    training_losses -> backward -> clip_grad_norm_(10) -> Adam.step -> LinearLR.step, optimizers/schedulers.py:8-19) on the reference's
    denoiser (dropout 0, fp32).  The same loop through the drop-in modules + training.Adam + training.linear_lr in DFX_PREC_F32:
    per-iteration loss, gradient norm and learning rate at 1e-5 relative, the parameter vector's L2 norm / sum and 256 sampled elements
    of every parameter after every step.  Adam's first steps move every element by ~lr * g / (|g| + 1e-8): an element whose gradient
    is rounding noise around zero (structurally dead weights: K/V columns of always-zero context entries ...) moves by anything up to
    lr in either implementation, so the sampled elements are gated in two classes with the reference's own sampled gradients (pg/*):
    resolved gradient (>= 1e-4 of the tensor's largest in every iteration so far) -> 1e-4 x max|p|; the rest -> the 2.5 lr bound."""
    from difffacto_amd import training
    from difffacto_amd.modules import AnchoredDiffusion
    from test_modules_cpu import DIFF_CFG
    g = np.load(os.path.join(GOLD, "train_loop_B3_N64_T10.npz"))
    W = synth.make_denoiser_weights(int(g["weight_seed"]))
    d = AnchoredDiffusion(num_timesteps=10, precision="f32", **{**DIFF_CFG, "net": dict(DIFF_CFG["net"], dropout=0.0)})
    d.model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    d = d.cuda().train()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    seg = g["seg"].astype(np.int64)
    mean, var = g["mean"], np.exp(g["logvar"]).astype(np.float32)
    idx = np.broadcast_to(seg[:, None, :], (seg.shape[0], 3, seg.shape[1]))
    anchors, variance = cu(np.take_along_axis(mean, idx, 2)), cu(np.take_along_axis(var, idx, 2))
    ctx = [cu(g["part_code"]), cu(np.concatenate([mean, var], 1).astype(np.float32))]
    s0, s1, lr0, lr1 = (float(v) for v in g["sched"])
    opt = training.Adam(list(d.model.parameters()), lr=lr0, max_norm=float(g["max_norm"]))
    named = list(d.model.named_parameters())
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-30)
    worst = {"loss": 0.0, "grad_norm": 0.0, "l2": 0.0, "elem": 0.0}
    n_res = n_tot = 0
    for it in range(int(g["iters"])):
        opt.lr = training.linear_lr(it, s0, s1, lr0, lr1)
        assert rel(opt.lr, float(g["lr"][it])) < 1e-12
        opt.zero_grad()
        loss = d.training_losses(cu(g["x_start"][it]), cu(g["t"][it]), anchors=anchors, variance=variance, ctx=ctx,
                                 anchor_assignment=cu(g["seg"].astype(np.int32)), valid_id=cu(g["valid"]), flags=None, noise=cu(g["noise"][it]))["mse_loss"]
        loss.backward()
        norm = opt.step()
        worst["loss"] = max(worst["loss"], rel(float(loss.detach()), float(g["loss"][it])))
        worst["grad_norm"] = max(worst["grad_norm"], rel(float(norm), float(g["grad_norm"][it])))
        flat = torch.cat([p.detach().reshape(-1).double() for _, p in named])
        worst["l2"] = max(worst["l2"], rel(float(flat.norm()), float(g["param_l2"][it])))
        assert abs(float(flat.sum()) - float(g["param_sum"][it])) <= 1e-5 * float(flat.abs().sum())
        for name, p in named:
            ref = g["ps/" + name][it].astype(np.float64)
            gref = np.abs(g["pg/" + name][:it + 1].astype(np.float64))
            got = p.detach().reshape(-1)[torch.from_numpy(g["pi/" + name]).cuda()].cpu().numpy().astype(np.float64)
            err = np.abs(got - ref)
            scale = max(float(np.abs(ref).max()), 1e-3)
            # elements whose gradient was resolved (>= 1e-4 of the tensor's largest sampled gradient in every iteration so far):
            resolved = (gref >= 1e-4 * gref.max(axis=1, keepdims=True)).all(axis=0)
            assert err.max() <= 2.5 * lr0 * (it + 1), (name, it, err.max())
            if resolved.any():
                worst["elem"] = max(worst["elem"], float(err[resolved].max() / scale))
            n_res += int(resolved.sum())
            n_tot += err.size
    print("training loop vs reference:", {k: f"{v:.2e}" for k, v in worst.items()}, f"{n_res}/{n_tot} sampled elements with a resolved gradient")
    assert worst["loss"] < 1e-5 and worst["grad_norm"] < 1e-5 and worst["l2"] < 1e-5 and worst["elem"] < 1e-4, worst
    assert n_res > 0.8 * n_tot


def test_linear_lr_schedule_values():
    """optimizers/schedulers.py:8-19 at the shipped settings (configs/gen_chair.py: 2e-3 -> 1e-4 over epochs 4000..8000)."""
    from difffacto_amd.training import linear_lr
    f = lambda e: linear_lr(e, 4000, 8000, 2e-3, 1e-4)
    assert f(0) == f(4000) == 2e-3 and abs(f(6000) - 1.05e-3) < 1e-15 and abs(f(8000) - 1e-4) < 1e-15 and abs(f(9000) - 1e-4) < 1e-15
