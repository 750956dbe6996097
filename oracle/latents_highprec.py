"""float64 restatement of the latent front end (ORACLE — test only): the truth that the fp32 numpy oracle (oracle/latents.py) and
the kernels are both measured against.

The same reference operations as oracle/latents.py, in the same order (flow.py:21-72, part_encoders.py:88-143 both cimle branches,
:1052-1110), every array float64: inputs are the fp32 arrays widened exactly, no intermediate is rounded to fp32.

``mutate`` names one deliberately wrong variant (tests/test_latent_configs_cpu.py shows that the acceptance function of the GPU tests
rejects each); None is the restatement:

    "class_mod4"   class embedding row j % 4 instead of j
    "drop_in8"     the last 8 input channels of proj_in dropped
    "head32"       heads split at width 32 whatever d_head
    "no_pre_norm"  pre_norm skipped (cimle=False)
    "swap_parity"  flow layers swap on odd instead of even indices
"""
import math

import numpy as np
from scipy.special import erf as _erf

F64 = np.float64
LN_EPS = 1e-5
MUTATIONS = ("class_mod4", "drop_in8", "head32", "no_pre_norm", "swap_parity")


def widen(W):
    return {k: np.asarray(v, dtype=F64) for k, v in W.items()}


def linear(x, w, b=None):
    y = x @ w.T
    return y if b is None else y + b


def layer_norm(x, w, b):
    xc = x - x.mean(axis=-1, keepdims=True)
    return xc / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + LN_EPS) * w + b


def coupling_reverse(x, W, prefix, swap):
    D = x.shape[1]
    d = D - D // 2
    if swap:
        x = np.concatenate([x[:, d:], x[:, :d]], axis=1)
    h = np.maximum(linear(x[:, :d], W[prefix + "net_s_t.0.weight"], W[prefix + "net_s_t.0.bias"]), 0)
    h = np.maximum(linear(h, W[prefix + "net_s_t.2.weight"], W[prefix + "net_s_t.2.bias"]), 0)
    s_t = linear(h, W[prefix + "net_s_t.4.weight"], W[prefix + "net_s_t.4.bias"])
    out_dim = D - d
    scale = 1.0 / (1.0 + np.exp(-(s_t[:, :out_dim] + 2.0)))
    y1 = (x[:, d:] - s_t[:, out_dim:]) / scale
    return np.concatenate([y1, x[:, :d]] if swap else [x[:, :d], y1], axis=1)


def flow_reverse(x, W, part, depth, mutate=None):
    x = np.asarray(x, dtype=F64)
    for i in range(depth - 1, -1, -1):
        x = coupling_reverse(x, W, f"flow.{part}.chain.{i}.", swap=(i % 2 == (1 if mutate == "swap_parity" else 0)))
    return x


def self_attention(x, mask, W, prefix, heads, mutate=None):
    B, J, C = x.shape
    q, k, v = (linear(x, W[prefix + f"to_{n}.weight"]) for n in "qkv")
    d = C // heads
    scale = d ** -0.5
    if mutate == "head32":
        heads, d = C // 32, 32
    q, k, v = (t.reshape(B, J, heads, d).transpose(0, 2, 1, 3) for t in (q, k, v))
    sim = np.einsum("bhid,bhjd->bhij", q, k) * scale
    sim = np.where(mask.astype(bool)[:, None, None, :], sim, -float(np.finfo(np.float32).max))
    e = np.exp(sim - sim.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    out = np.einsum("bhij,bhjd->bhid", p, v).transpose(0, 2, 1, 3).reshape(B, J, C)
    return linear(out, W[prefix + "to_out.0.weight"], W[prefix + "to_out.0.bias"])


def feed_forward_glu(x, W, prefix):
    a, g = np.split(linear(x, W[prefix + "net.0.proj.weight"], W[prefix + "net.0.proj.bias"]), 2, axis=-1)
    return linear(a * (g * 0.5 * (1.0 + _erf(g / math.sqrt(2.0)))), W[prefix + "net.2.weight"], W[prefix + "net.2.bias"])


def part_aligner_forward(W, part_code, valid_id, noise, noise_scale=100.0, heads=8, cimle=True, mutate=None):
    """W float64 (``widen``).  -> mean (B,3,J), logvar (B,3,J), float64."""
    P = "part_aligner."
    part_code, valid_id = np.asarray(part_code, dtype=F64), np.asarray(valid_id, dtype=F64)
    B, _, J = part_code.shape
    x = part_code
    if cimle:
        nz = np.asarray(noise, dtype=F64) * F64(np.float32(noise_scale))
        x = np.concatenate([part_code, np.repeat(nz[:, :, None], J, axis=2)], axis=1)
    else:
        assert noise is None
    x = x.transpose(0, 2, 1)
    w_in = W[P + "proj_in.weight"]
    if mutate == "drop_in8":
        x, w_in = x[..., :-8], w_in[:, :-8]
    x = linear(x, w_in, W[P + "proj_in.bias"])
    emb = W[P + "class_emb.weight"]
    x = x + (emb[np.arange(J) % 4] if mutate == "class_mod4" else emb)[None]
    if not cimle and mutate != "no_pre_norm":
        x = layer_norm(x, W[P + "pre_norm.weight"], W[P + "pre_norm.bias"])
    i = 0
    while f"{P}transformer_blocks.{i}.norm2.weight" in W:
        p = f"{P}transformer_blocks.{i}."
        x = self_attention(layer_norm(x, W[p + "norm2.weight"], W[p + "norm2.bias"]), valid_id, W, p + "attn2.", heads, mutate) + x
        x = feed_forward_glu(layer_norm(x, W[p + "norm3.weight"], W[p + "norm3.bias"]), W, p + "ff.") + x
        i += 1
    x = linear(layer_norm(x, W[P + "post_norm.weight"], W[P + "post_norm.bias"]), W[P + "proj_out.weight"], W[P + "proj_out.bias"])
    h = x.transpose(0, 2, 1)
    return h[:, :3].copy(), h[:, 3:].copy()


def sample_latents(W, w_noise, aligner_noise, valid_id, fixed_id, K, sample_points, prior_var=1.0, noise_scale=100.0, log_scale_var=0.0,
                   part_code=None, heads=8, cimle=True, mutate=None):
    """oracle/latents.py:sample_latents in float64 (the integer outputs and the copies are the same arrays)."""
    from .latents import flow_depth, seg_mask_ids
    S, J = np.shape(valid_id)
    if part_code is None:
        part_code = np.asarray(w_noise, dtype=F64) * F64(np.float32(np.sqrt(prior_var)))
        depth = flow_depth(W)
        if depth:
            part_code = np.stack([flow_reverse(part_code[..., i], W, i, depth, mutate) for i in range(J)], axis=-1)
    part_code = np.asarray(part_code, dtype=F64)
    fixed_id, valid_id = np.asarray(fixed_id, dtype=F64), np.asarray(valid_id, dtype=F64)
    noise = None
    if cimle:
        noise = np.asarray(aligner_noise, dtype=F64)
    else:
        assert K == 1 and aligner_noise is None
    fixed_valid = np.clip(valid_id[0][None] + fixed_id[None], 0, 1)
    part_code = part_code * (1 - fixed_id)[None, None] + fixed_id[None, None] * part_code[0][None]
    valid_id = valid_id * (1 - fixed_id)[None] + fixed_id[None] * fixed_valid
    if noise is not None and np.any(fixed_id == 1):
        noise = np.broadcast_to(noise.reshape(S, K, -1)[0][None], (S, K, noise.shape[-1])).reshape(S * K, -1)
    part_code, valid_id = np.repeat(part_code, K, axis=0), np.repeat(valid_id, K, axis=0)
    mean, logvar = part_aligner_forward(W, part_code, valid_id, noise, noise_scale, heads, cimle, mutate)
    seg = seg_mask_ids(valid_id, sample_points)
    lv = logvar + F64(np.float32(log_scale_var))
    idx = np.broadcast_to(seg[:, None, :].astype(np.int64), (mean.shape[0], 3, seg.shape[1]))
    return {"mean_per_point": np.take_along_axis(mean, idx, axis=2), "logvar_per_point": np.take_along_axis(lv, idx, axis=2), "seg_mask": seg,
            "valid_id": valid_id, "part_code": part_code, "mean": mean, "logvar": logvar, "noise": noise,
            "params": np.concatenate([mean, np.exp(lv)], axis=1)}
