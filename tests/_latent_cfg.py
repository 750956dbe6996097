"""Test helper: the named configurations of the latent sampler / aligner-training entry points beyond the shipped one, their seeded
weights and inputs, the torch restatement of the aligner that serves as gradient reference, and the acceptance functions with the
factors measured on the MI355X (profiles/latent_configs_parity.txt).

Forward: err = |kernel - float64 truth| (oracle/latents_highprec.py), yardstick = |fp32 numpy oracle - float64 truth| on the same
case; max-abs and rms; accepted when err <= F x yardstick.  Gradients: the same with the float32 CPU autograd of `_aligner_torch`
as yardstick and the float64 autograd as truth, factor FG; d_part_code / d_noise per shape (each shape's max-abs error against the
yardstick's worst shape, so that one wrong shape cannot hide under the tensor's max-abs), parameter gradients per tensor.
"""
import numpy as np
import torch

from difffacto_amd import synth

MAX_DEPTH = 8       # DFX_MAX_DEPTH

# parts / zdim / heads x d_head / depth / noise / flow depth x hidden / cimle
CONFIGS = {
    "shipped": dict(n_class=4, zdim=256, heads=8, d_head=32, depth=5, noise_dim=32, flow_depth=14, flow_hidden=256, cimle=True),
    "tiny": dict(n_class=3, zdim=48, heads=4, d_head=16, depth=2, noise_dim=8, flow_depth=2, flow_hidden=40, cimle=True),
    "wide": dict(n_class=8, zdim=64, heads=16, d_head=64, depth=1, noise_dim=40, flow_depth=3, flow_hidden=136, cimle=True),
    "one": dict(n_class=1, zdim=32, heads=2, d_head=32, depth=3, noise_dim=16, flow_depth=1, flow_hidden=8, cimle=True),
    "plain": dict(n_class=5, zdim=128, heads=4, d_head=32, depth=MAX_DEPTH, noise_dim=0, flow_depth=0, flow_hidden=0, cimle=False),
    "mid": dict(n_class=4, zdim=256, heads=16, d_head=32, depth=1, noise_dim=32, flow_depth=2, flow_hidden=256, cimle=True),
}
# shipped widths with a short oracle: the batch-size boundary cases of the launcher
CONFIGS["shipped_short"] = dict(CONFIGS["shipped"], depth=1, flow_depth=2)
NOISE_SCALE = 100.0
VALID_PATTERNS = ("all", "one_absent", "one_present", "shape_all_absent")

# ---- thresholds of the GPU gate (tests/test_gpu_latent_configs.py) ----------------------------------------------------------------------
# Each is the largest ratio measured on the MI355X over all cases of that file x 1.25 (profiles/latent_configs_parity.txt: 401 forward
# lines, 180 data-gradient lines, 90 parameter-gradient lines).  The kernels are deterministic on fixed seeds; the margin is for cases added
# later.  tests/test_latent_configs_cpu.py holds both factors to the condition that every deliberately wrong variant is still rejected
# (the weakest there: heads split at width 32 on `tiny`, 273 x; gradient through absent keys on `tiny`, 204 x on d_part_code, 27 x on d_noise).
#            measured worst  x 1.25   case
#   F           10.319       12.90    plain B=1 K=1 logvar_per_point (15 values, 8 blocks; yardstick at its rounding floor); next:
#                                     6.896 mid B=1 training forward mean, 6.561 wide B=5 training forward mean (k_mm: K = 4096 summed in sequence)
#   FG           9.053       11.32    wide B=17 one_present proj_out.bias (6 values); next: 5.387 shipped B=1 transformer_blocks.2.norm3.weight,
#                                     4.376 wide B=5 one_present d_part_code (worst shape)
# inference alone: sample_latents / part_aligner / flow_reverse at most 10.3 (above), the launcher's batch-size boundaries at most 4.2
F = 12.9
FG = 11.32


def synth_kwargs(cfg):
    return dict(n_class=cfg["n_class"], flow_depth=cfg["flow_depth"], flow_hidden=cfg["flow_hidden"] or 8, depth=cfg["depth"], heads=cfg["heads"],
                d_head=cfg["d_head"], noise_dim=cfg["noise_dim"], zdim=cfg["zdim"])


def weights(tag, seed=0):
    """fp32 numpy weights of a named configuration (the shipped one: synth's defaults, bit for bit)."""
    return synth.make_latent_weights(seed, **synth_kwargs(CONFIGS[tag]))


def validity(tag, B, pattern, rng=None):
    """(B, J) float32 mask.  `one` has a single part: its patterns are all present, and for the last pattern shape B // 2 absent."""
    J = CONFIGS[tag]["n_class"]
    v = np.ones((B, J), np.float32)
    b = np.arange(B)
    if pattern == "one_absent" and J > 1:
        v[b, (b + 1) % J] = 0
    elif pattern == "one_present" and J > 1:
        v[:] = 0
        v[b, (2 * b + 1) % J] = 1
    elif pattern == "shape_all_absent":
        if J > 1:
            v[b[::2], (b[::2] // 2) % J] = 0
        v[B // 2] = 0
    return v


def fixed_patterns(J):
    """none, part 0, part J-1, all."""
    e = np.eye(J, dtype=np.int32)
    return {"none": np.zeros(J, np.int32), "first": e[0], "last": e[J - 1], "all": np.ones(J, np.int32)}


def inputs(tag, B, K, seed, pattern="one_absent"):
    """Seeded draws of one case: w_noise (B,Z,J), aligner noise (B*K,ND) or None, validity, a given part code, cotangents."""
    cfg = CONFIGS[tag]
    rng = np.random.Generator(np.random.PCG64(seed))
    J, Z, ND = cfg["n_class"], cfg["zdim"], cfg["noise_dim"]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(w_noise=f(B, Z, J), noise=f(B * K, ND) if cfg["cimle"] else None, valid=validity(tag, B, pattern), code=f(B, Z, J),
                d_mean=f(B * K, 3, J), d_logvar=f(B * K, 3, J))


def aligner_params(W, device, grad=False):
    return {k[len("part_aligner."):]: torch.from_numpy(v.copy()).to(device).requires_grad_(grad) for k, v in W.items() if k.startswith("part_aligner.")}


def _aligner_torch(W, code, valid, noise, noise_scale=100.0, heads=8, cimle=True, mutate=None):
    """oracle/latents.py:part_aligner_forward op by op in torch, for autograd: float64 for the truth, float32 on the CPU for the yardstick.
    ``mutate="absent_keys_grad"``: the keys of absent parts are masked by adding -finfo.max instead of masked_fill, which passes the
    gradient to sim; it differs only where a shape has every part absent (the rule of k_attn_bwd before it read `valid`)."""
    P = "part_aligner."
    F = torch.nn.functional
    B, _, J = code.shape
    if cimle:
        x = torch.cat([code, (noise * noise_scale)[:, :, None].expand(-1, -1, J)], dim=1).transpose(1, 2)
    else:
        assert noise is None
        x = code.transpose(1, 2)
    x = F.linear(x, W[P + "proj_in.weight"], W[P + "proj_in.bias"]) + W[P + "class_emb.weight"][None]
    if not cimle:
        x = F.layer_norm(x, (x.shape[-1],), W[P + "pre_norm.weight"], W[P + "pre_norm.bias"], 1e-5)
    depth = 0
    while f"{P}transformer_blocks.{depth}.norm2.weight" in W:
        depth += 1
    for i in range(depth):
        p = f"{P}transformer_blocks.{i}."
        C = x.shape[-1]
        xn = F.layer_norm(x, (C,), W[p + "norm2.weight"], W[p + "norm2.bias"], 1e-5)
        q, k, v = (F.linear(xn, W[p + f"attn2.to_{n}.weight"]).reshape(B, J, heads, C // heads).transpose(1, 2) for n in "qkv")
        sim = torch.einsum("bhid,bhjd->bhij", q, k) * (C // heads) ** -0.5
        absent = ~valid.bool()[:, None, None, :]
        if mutate == "absent_keys_grad":
            sim = sim + absent.to(sim.dtype) * -torch.finfo(torch.float32).max      # sim is absorbed: the same softmax, d sim kept
        else:
            assert mutate is None
            sim = sim.masked_fill(absent, -torch.finfo(torch.float32).max)
        o = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), v).transpose(1, 2).reshape(B, J, C)
        x = F.linear(o, W[p + "attn2.to_out.0.weight"], W[p + "attn2.to_out.0.bias"]) + x
        h = F.linear(F.layer_norm(x, (C,), W[p + "norm3.weight"], W[p + "norm3.bias"], 1e-5), W[p + "ff.net.0.proj.weight"], W[p + "ff.net.0.proj.bias"])
        a, gate = h.chunk(2, dim=-1)
        x = F.linear(a * F.gelu(gate), W[p + "ff.net.2.weight"], W[p + "ff.net.2.bias"]) + x
    C = x.shape[-1]
    x = F.linear(F.layer_norm(x, (C,), W[P + "post_norm.weight"], W[P + "post_norm.bias"], 1e-5), W[P + "proj_out.weight"], W[P + "proj_out.bias"])
    h = x.transpose(1, 2)
    return h[:, :3], h[:, 3:]


def autograd(Wn, tag, code, valid, noise, d_mean, d_logvar, dtype, mutate=None, params=True):
    """mean, logvar, d_part_code, d_noise and {name: parameter gradient} of `_aligner_torch` on the CPU in `dtype`, as float64 numpy."""
    cfg = CONFIGS[tag]
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
    W = {k: t(v).requires_grad_(params) for k, v in Wn.items() if k.startswith("part_aligner.")}
    c, z = t(code).requires_grad_(True), t(noise).requires_grad_(True)
    m, l = _aligner_torch(W, c, t(valid), z, NOISE_SCALE, cfg["heads"], cfg["cimle"], mutate)
    loss = 0
    if d_mean is not None:
        loss = loss + (m * t(d_mean)).sum()
    if d_logvar is not None:
        loss = loss + (l * t(d_logvar)).sum()
    loss.backward()
    n = lambda a: a.detach().double().numpy()
    grads = {k[len("part_aligner."):]: n(p.grad) for k, p in W.items() if p.grad is not None} if params else {}
    return dict(mean=n(m), logvar=n(l), d_part_code=n(c.grad), d_noise=n(z.grad), grads=grads)


# ---- acceptance -------------------------------------------------------------------------------------------------------------------------
# Some cases hold a handful of values (J = 1, B = 1: three means), where the fp32 oracle's error can be zero or tiny by luck.  No fp32
# result is better than its own rounding, so a yardstick is never taken below the rounding of the truth to fp32: half an ulp of the
# largest value for max-abs, and 2^-24 / sqrt(3) of the rms value (a uniform relative error within +-2^-24) for rms.
HALF_ULP = 2.0 ** -24


def err_stats(got, truth):
    t = np.asarray(truth, np.float64)
    e = np.abs(np.asarray(got, np.float64) - t)
    return dict(max=float(e.max()), rms=float(np.sqrt((e * e).mean())), floor_max=HALF_ULP * float(np.abs(t).max()),
                floor_rms=HALF_ULP / np.sqrt(3.0) * float(np.sqrt((t * t).mean())))


def yard(y, s):
    return max(y[s], y["floor_" + s])


def ratio(k, y):
    """Largest of the max-abs and rms ratios of a kernel's `err_stats` to the yardstick's; an all-zero truth admits only a zero error."""
    return max((0.0 if k[s] == 0 else np.inf) if yard(y, s) == 0 else k[s] / yard(y, s) for s in ("max", "rms"))


def accept(kernel, yardstick, factor):
    """Failures (empty = accepted) of a kernel's `err_stats` against the yardstick's on the same case."""
    return [f"{s} {kernel[s]:.3e} > {factor} x {yard(yardstick, s):.3e}" for s in ("max", "rms") if not kernel[s] <= factor * yard(yardstick, s)]


def per_shape(got, truth):
    e = np.abs(np.asarray(got, np.float64) - np.asarray(truth, np.float64))
    return e.reshape(e.shape[0], -1).max(1)


def shape_ratio(got, yardstick, truth):
    """Every shape's max-abs error over the yardstick's worst shape -> (B,) ratios."""
    return per_shape(got, truth) / max(per_shape(yardstick, truth).max(), HALF_ULP * float(np.abs(truth).max()))


def accept_shapes(got, yardstick, truth, factor):
    r = shape_ratio(got, yardstick, truth)
    return [f"shape {b}: max-abs error {r[b]:.1f} x the yardstick's worst shape > {factor}" for b in np.nonzero(~(r <= factor))[0]]


def line(label, variant, what, r, k, y):
    return (f"LATCFG {label} [{variant}] {what}: max {k['max']:.3e} rms {k['rms']:.3e} | yardstick max {yard(y, 'max'):.3e} rms {yard(y, 'rms'):.3e} | "
            f"ratio {r:.3f}")
