"""Cases of tests/test_gpu_train_bits.py and of tools/make_train_bits_golden.py, which writes that test's fixture: one construction, so the
two cannot diverge.  A case is one denoiser training iteration (forward + masked_mse + backward) on seeded synthetic inputs; its result is the
SHA-256 of the raw bytes of every output."""
import hashlib
import os

import numpy as np
import torch

from difffacto_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_bits", "parent.json")
DROPOUT = (0.2, 777)

#        name               depth  B  N    precision  dfx_debug_train_fused  dropout   dfx_debug_last_train_path
CASES = [("fused_d5_8x32",    5,   8, 32,  "bf16", 1, None,    "fused_bf16"),            # smallest fused shape: one live wavefront per k_ff workgroup
         ("fused_d5_8x32_p",  5,   8, 32,  "bf16", 1, DROPOUT, "fused_bf16_dropout"),
         ("fused_d5_3x160",   5,   3, 160, "bf16", 1, None,    "fused_bf16"),            # ragged last workgroup
         ("fused_d5_3x160_p", 5,   3, 160, "bf16", 1, DROPOUT, "fused_bf16_dropout"),
         ("fused_d5_5x480",   5,   5, 480, "bf16", 1, None,    "fused_bf16"),            # 75 tiles over 64 weight-gradient slabs: empty slabs
         ("fused_d5_5x480_p", 5,   5, 480, "bf16", 1, DROPOUT, "fused_bf16_dropout"),
         ("fused_d2_2x224",   2,   2, 224, "bf16", 1, None,    "fused_bf16"),            # the other parity of the dh / dh2 hand-over to the stem
         ("fused_d2_2x224_p", 2,   2, 224, "bf16", 1, DROPOUT, "fused_bf16_dropout"),
         ("layer_bf16_3x160", 5,   3, 160, "bf16", 0, DROPOUT, "layer_bf16_dropout"),
         ("layer_f32_3x160",  5,   3, 160, "f32",  1, None,    "layer_f32")]


def make_inputs(depth, B, N):
    rng = np.random.Generator(np.random.PCG64(9000 + 100 * depth + 7 * B + N))
    W = synth.make_denoiser_weights(6, depth=depth)
    pc, mean, logvar, valid = synth.make_latents(B, seed=31, all_valid=False)
    seg = synth.make_seg_mask(valid, N)
    var = np.exp(logvar).astype(np.float32)
    idx = np.broadcast_to(seg.astype(np.int64)[:, None, :], (B, 3, N))
    anc, vr = np.take_along_axis(mean, idx, axis=2), np.take_along_axis(var, idx, axis=2)
    return dict(W=W, x_t=(anc + np.sqrt(vr) * rng.standard_normal((B, 3, N))).astype(np.float32), t=rng.integers(0, 1000, size=(B,)).astype(np.int64),
                ctx_code=pc, ctx_mv=np.concatenate([mean, var], axis=1).astype(np.float32),
                anchors_pt=np.ascontiguousarray(anc.transpose(0, 2, 1)), variances_pt=np.ascontiguousarray(vr.transpose(0, 2, 1)),
                valid=valid, assignment=seg.astype(np.int32), noise=rng.standard_normal((B, 3, N)).astype(np.float32),
                flags=(rng.uniform(size=(B, 1, N)) > 0.3).astype(np.float32))


def run_case(case):
    """-> {output name: sha256 hex of its raw bytes}: loss, eps, every parameter gradient, d_ctx_code, d_ctx_mv, d_x, d_variances."""
    from difffacto_amd import _ffi, training
    name, depth, B, N, precision, fused_sw, dropout, path = case
    c = make_inputs(depth, B, N)
    dev = "cuda"
    leaf = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)  # noqa: E731
    P = {k: leaf(v) for k, v in c["W"].items()}
    x, cc, cm, vr = leaf(c["x_t"]), leaf(c["ctx_code"]), leaf(c["ctx_mv"]), leaf(c["variances_pt"])
    L = _ffi.lib()
    L.dfx_debug_train_fused(fused_sw)
    try:
        eps = training.denoiser_train_forward(P, x, torch.from_numpy(c["t"]).to(dev), cc, cm, torch.from_numpy(c["anchors_pt"]).to(dev), vr,
                                              torch.from_numpy(c["valid"]).to(dev), torch.from_numpy(c["assignment"]).to(dev),
                                              precision=precision, dropout=dropout)
        took = L.dfx_debug_last_train_path().decode()
        loss = training.masked_mse(torch.from_numpy(c["noise"]).to(dev), eps, torch.from_numpy(c["flags"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        L.dfx_debug_train_fused(1)
    assert took == path, f"{name}: expected the path {path}, the forward took {took}"
    out = {"loss": loss.detach(), "eps": eps.detach(), "d_ctx_code": cc.grad, "d_ctx_mv": cm.grad, "d_x": x.grad, "d_variances": vr.grad}
    out.update({"g/" + k: v.grad for k, v in P.items()})
    res = {}
    for k, v in out.items():
        a = np.ascontiguousarray(v.cpu().numpy())
        assert a.dtype == np.float32 and np.isfinite(a).all(), (name, k)
        res[k] = hashlib.sha256(a.tobytes()).hexdigest()
    return res
