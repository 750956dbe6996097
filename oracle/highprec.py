"""float64 restatement of the denoiser and of the anchored diffusion, with a rounding hook (ORACLE — test only).

The same operations as ``oracle/denoiser.py`` and ``oracle/diffusion.py`` (whose text and fp32 bits stay what the golden
and index-exact CPU tests stand on), written out in float64: every intermediate is float64, inputs (weights, latents,
clouds, noise) are the callers' fp32 arrays widened exactly, and the schedule coefficients are the reference's own fp32
table entries (``oracle.diffusion.Tables.f32``) widened exactly — the kernels are bit-exact on the tables
(``test_tables_bit_exact_vs_reference``), so the tables are inputs, not part of the error.

Two yardsticks come out of it:

* ``operand_round=None``: the float64 truth.  ``|fp32 numpy oracle - truth|`` is what fp32 arithmetic costs.
* ``operand_round="bf16"``: the *rounding model* of the bf16 kernels.  Both operands of the four per-block products that the
  bf16 kernels run on the matrix pipe are rounded to bf16 (fp32 first, as the kernel holds fp32 values, then round-to-nearest-
  even to bf16); the products accumulate in float64; nothing else is rounded.  ``|model - truth|`` is what the operand
  format costs.  The model holds no constant fitted to a kernel's output.

The model rounds at the reference's layout of the four products.  The kernels evaluate algebraically folded forms of them, so the
model states WHICH products pay an operand rounding, one per operand, and is not a mirror of the kernels' operands — except
for the ``w1_fold`` site below, which restates the kernel's pack.  Per transformer block:

  product, and what the model rounds            what denoiser_kernel.hip / denoiser_setup.hip round instead
  to_q: LN2's affine output, to_q.weight        ``attention`` / ``attn_m0``: ``sim = A_s xhat + sbias``.  The NOT affine normalised row
                                                  (``ln_to_act`` -> ``Act<DFX_PREC_BF16>::set``) and the prepare-time record
                                                  ``A_s = scale K_s Wq diag(gamma2)`` (32 x 128 per shape, bf16 tiles of the attention
                                                  record) are rounded; to_q.weight itself never is, and q k^T is not a separate product
  to_out.0: the 128-wide attention output,      ``attention`` / ``attn_m1``: ``h += M_s P``.  The 32 softmax weights (``pa.set(sim)``,
    to_out.0.weight                               ``attn_softmax``) and the record ``M_s = Wout V_s`` (128 x 32) are rounded; neither
                                                  to_out.0.weight nor the attention output exists at run time
  FF net.0: LN3's affine output, W1             ``ff_chunk`` / ``ff_m`` GEMM1.  ``k_pack_w1`` folds gamma3 into W1 in EVERY pack and
                                                  ``ln_to_act`` is never affine in bf16, so also the plain pack rounds
                                                  ``W1 diag(gamma3)`` and xhat (beta3 goes into fp32 accumulator initialisers)
  FF net.2: a * gelu(g), W2, both to bf16       ``ff_chunk`` / ``ff_m`` GEMM2 (``mma_hid``) is an FP16 product, v_mfma_f32_32x32x16_f16:
                                                  W2 is packed as fp16 (denoiser_internal.h, FF_A_SCALE / FF_G_SCALE) and ``hid`` is fp16
                                                  (``pk_f16`` = cvt_pkrtz, round toward zero), from a degree-5 fp16 polynomial GELU in the
                                                  pipelined kernels (``gelu16_f16_math``, 3.9e-4 abs) or the sigmoid form in the direct one

What that leaves between model and kernels, as measured on the CPU: rounding the net.2 site to fp16 (3 more mantissa bits) instead
of bf16 lowers the yardstick by 1 to 12 %, so the model OVERSTATES that site's operand rounding and that slack is what absorbs
the fp16 GELU's approximation and truncation, which the model does not state; the folded attention and plain-pack forms round
operands of the same count and size, statistically the same cost.  The kernels measured 0.87 x (plain pack) to 1.13 x (folded) the
model's rms (tests/_errstats.py).

``w1_fold=k`` (bf16 engines that carry the first FF bias in hidden channel k's K slot, ``dfx_denoiser_w1_fold`` /
``dfx_debug_w1_fold_channel``; k = 127 unless an outlier moved it) DOES restate the kernel's pack in the net.0 site: denoiser_setup.hip
``k_pack_w1`` (the ``PREC == DFX_PREC_BF16 && fold`` branch) stores, with W1' = W1 diag(gamma3), the DIFFERENCES
``bf16(W1'[r][c] - W1'[r][k])`` for c != k and ``bf16(b1[r] + W1[r] . beta3)`` in column k, and denoiser_kernel.hip ``bias_slot_one``
puts the constant 1 into slot k of the rounded, not affine LayerNorm output (``ln_to_act``).  Equal in real arithmetic (the
normalised row sums to zero); in bf16 every weight of a row rounds with a step that follows ``|W1'[r][k]|``, which the
reference-layout model cannot show: it measured 1.39 x too small for the folded kernels.

Exact in the model, as they are fp32 VALU work or prepare-time fp32 work on the GPU: ``proj_in`` + ``pre_norm``
(``proj_in_prenorm``), the LayerNorm statistics (``ln_stats`` / ``ln_stats_fast``), the softmax (``softmax4``), the to_k / to_v
products and the time embedding (prepare time: ``c_t`` rows, attention records), the bias adds, ``post_norm`` + ``proj_out``
(``post_eps``) and the posterior update (``step_epilogue``).

``mutate=`` is a test hook: four deliberately wrong variants of the rounding model, used by the CPU self-test of the
error statistics (tests/test_oracle_highprec_cpu.py) to prove that the acceptance function can fail:

* ``"truncate"``        activations are truncated to bf16 instead of rounded (weights stay rounded);
* ``("drop_unit", u)``  hidden unit ``u`` of block ``MUT_BLOCK``'s second FF product is dropped for points with ``n % 32 == MUT_LANE``
                        (one wrong fragment element for one lane; a wrong fragment would lose 8 of the 512);
* ``("halve_unit", u)`` the same unit is halved instead of dropped;
* ``"t_plus_one"``      the time embedding is taken one step late (t + 1): a time table off by one.

The unit is the caller's choice and does not depend on the mutated run, the fold or the rounding: ``ff_unit_ranking`` orders the
512 units by the energy ``E[h_u^2] |W2[:, u]|^2`` they carry into the residual stream in the FLOAT64 forward of the same inputs, and
the self-test takes rank ``MUT_RANK``.  What the self-test then proves is a statement about weight: a halved or dropped unit of at
least that rank's energy in one lane is seen; lighter units are seen less, and the lightest not at all (their whole contribution is
below the rounding noise of the other 511) — the figures are in the self-test's docstring.
"""
import math

import numpy as np
from scipy.special import erf as _erf

from . import diffusion as odf

F64 = np.float64
LN_EPS = 1e-5  # torch.nn.LayerNorm default
MUTATIONS = ("truncate", "drop_unit", "halve_unit", "t_plus_one")
MUT_BLOCK, MUT_LANE, MUT_RANK = 2, 5, 64


def round_bf16(x, truncate=False):
    """float64 -> fp32 (nearest even) -> bf16 (nearest even, or truncated), returned as float64.  Finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    if not truncate:
        u = u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))
    return (u & np.uint32(0xFFFF0000)).view(np.float32).astype(F64)


class Net:
    """The weights widened to float64 once, the rounded copies of the four per-block matrices, and the two switches."""

    ROUNDED = ("attn2.to_q.weight", "attn2.to_out.0.weight", "ff.net.0.proj.weight", "ff.net.2.weight")

    def __init__(self, W, operand_round=None, mutate=None, w1_fold=None):
        if w1_fold is not None and (operand_round is None or not 0 <= int(w1_fold) < 128):
            raise ValueError("w1_fold: a hidden channel 0..127 of the rounding model (operand_round='bf16')")
        self.w1_fold = None if w1_fold is None else int(w1_fold)
        if operand_round not in (None, "bf16"):
            raise ValueError(f"operand_round: None or 'bf16', not {operand_round!r}")
        self.mutate_unit = self.capture = None
        if isinstance(mutate, tuple):
            mutate, self.mutate_unit = mutate[0], int(mutate[1])
            if mutate not in ("drop_unit", "halve_unit"):
                raise ValueError(f"mutate: only drop_unit / halve_unit take a unit, not {mutate!r}")
        elif mutate in ("drop_unit", "halve_unit"):
            raise ValueError(f"mutate: ({mutate!r}, unit) — the unit is the caller's choice (ff_unit_ranking)")
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError(f"mutate: one of {MUTATIONS}, not {mutate!r}")
        if mutate in ("truncate", "drop_unit", "halve_unit") and operand_round is None:
            raise ValueError(f"mutate={mutate!r} is a mutation of the rounding model: needs operand_round='bf16'")
        self.operand_round, self.mutate = operand_round, mutate
        self.W = {k: np.asarray(v).astype(F64) for k, v in W.items()}
        self.depth = 0
        while f"transformer_blocks.{self.depth}.norm2.weight" in self.W:
            self.depth += 1
        self.Wr = {}
        if operand_round == "bf16":
            for i in range(self.depth):
                for name in self.ROUNDED:
                    k = f"transformer_blocks.{i}.{name}"
                    self.Wr[k] = round_bf16(self.W[k])

    def act(self, x):
        """An activation operand of a matrix-pipe product."""
        if self.operand_round is None:
            return x
        return round_bf16(x, truncate=self.mutate == "truncate")

    def weight(self, key):
        """A weight operand of a matrix-pipe product."""
        return self.Wr[key] if self.operand_round is not None else self.W[key]


def as_net(W, operand_round=None, mutate=None, w1_fold=None):
    if isinstance(W, Net):
        assert operand_round is None and mutate is None and w1_fold is None, "the switches live in the Net"
        return W
    return Net(W, operand_round, mutate, w1_fold)


def timestep_embedding(t, dim=256, max_period=10000):
    t = np.asarray(t).astype(F64)
    half = dim // 2
    freqs = np.exp(-math.log(max_period) * np.arange(half, dtype=F64) / half)
    args = t[:, None] * freqs[None]
    return np.concatenate([np.cos(args), np.sin(args)], axis=-1)


def linear(x, w, b=None):
    y = x @ w.T
    return y if b is None else y + b


def layer_norm(x, w, b):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(axis=-1, keepdims=True)
    return xc / np.sqrt(var + LN_EPS) * w + b


def gelu(x):
    return x * 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))


def normalise(x):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    return xc / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + LN_EPS)


def folded_ff0(net, x, prefix, norm):
    """net.0 of a block's FF as the folded bf16 pack computes it (module docstring, ``w1_fold``).  x: the block's LayerNorm3 INPUT."""
    W, k = net.W, net.w1_fold
    key = (prefix, k)
    if key not in net.Wr:
        w1g = W[prefix + "net.0.proj.weight"] * W[norm + "weight"][None, :]
        wf = w1g - w1g[:, k:k + 1]
        wf[:, k] = W[prefix + "net.0.proj.bias"] + W[prefix + "net.0.proj.weight"] @ W[norm + "bias"]
        net.Wr[key] = round_bf16(wf)
    a = net.act(normalise(x))
    a[..., k] = 1.0
    return a @ net.Wr[key].T


def feed_forward_glu(net, x, prefix, rounded=False, block=None, norm=None):
    """FeedForward(glu=True).  ``rounded``: the two products are matrix-pipe products (a transformer block's FF; the time
    embedding's FF is not).  ``norm``: with ``net.w1_fold``, x is the LayerNorm's input and ``norm`` its parameter prefix."""
    W = net.W
    k0, k2 = prefix + "net.0.proj.weight", prefix + "net.2.weight"
    if rounded and net.w1_fold is not None:
        h = folded_ff0(net, x, prefix, norm)
    elif rounded:
        h = linear(net.act(x), net.weight(k0), W[prefix + "net.0.proj.bias"])
    else:
        h = linear(x, W[k0], W[prefix + "net.0.proj.bias"])
    a, g = np.split(h, 2, axis=-1)
    h = a * gelu(g)
    if net.capture is not None and block == MUT_BLOCK:
        net.capture["energy"] = (h * h).mean(axis=(0, 1)) * (W[k2] * W[k2]).sum(axis=0)
    if not rounded:
        return linear(h, W[k2], W[prefix + "net.2.bias"])
    h = net.act(h)
    if net.mutate in ("drop_unit", "halve_unit") and block == MUT_BLOCK:
        h = h.copy()                                            # (B, N, 512): points along axis 1
        h[:, MUT_LANE::32, net.mutate_unit] *= 0.0 if net.mutate == "drop_unit" else 0.5
    return linear(h, net.weight(k2), W[prefix + "net.2.bias"])


def ff_unit_ranking(W, *forward_args):
    """The 512 hidden units of block ``MUT_BLOCK``'s FF, heaviest first, by their mean-square contribution ``E[h_u^2] |W2[:, u]|^2`` to
    the FF output in the float64 forward (no rounding, no mutation) of ``transformer_net_forward(W, *forward_args)``."""
    net = Net(W)
    net.capture = {}
    transformer_net_forward(net, *forward_args)
    return np.argsort(-net.capture["energy"], kind="stable")


def cross_attention(net, x, context, mask, prefix, heads=8):
    W = net.W
    B, N, _ = x.shape
    J = context.shape[1]
    q = linear(net.act(x), net.weight(prefix + "to_q.weight"))
    k = linear(context, W[prefix + "to_k.weight"])
    v = linear(context, W[prefix + "to_v.weight"])
    inner = q.shape[-1]
    d = inner // heads
    scale = d ** -0.5
    q = q.reshape(B, N, heads, d).transpose(0, 2, 1, 3)
    k = k.reshape(B, J, heads, d).transpose(0, 2, 1, 3)
    v = v.reshape(B, J, heads, d).transpose(0, 2, 1, 3)
    sim = np.einsum("bhid,bhjd->bhij", q, k) * scale
    if mask is not None:
        assert mask.shape == (B, J)
        keep = np.asarray(mask).astype(bool)[:, None, None, :]
        sim = np.where(keep, sim, -float(np.finfo(np.float32).max))
    sim = sim - sim.max(axis=-1, keepdims=True)
    e = np.exp(sim)
    p = e / e.sum(axis=-1, keepdims=True)
    out = np.einsum("bhij,bhjd->bhid", p, v)
    out = out.transpose(0, 2, 1, 3).reshape(B, N, inner)
    return linear(net.act(out), net.weight(prefix + "to_out.0.weight"), W[prefix + "to_out.0.bias"])


def transformer_block(net, x, context, mask, i):
    W = net.W
    prefix = f"transformer_blocks.{i}."
    x = cross_attention(net, layer_norm(x, W[prefix + "norm2.weight"], W[prefix + "norm2.bias"]),
                        context, mask, prefix + "attn2.") + x
    if net.w1_fold is not None:
        return feed_forward_glu(net, x, prefix + "ff.", rounded=True, block=i, norm=prefix + "norm3.") + x
    x = feed_forward_glu(net, layer_norm(x, W[prefix + "norm3.weight"], W[prefix + "norm3.bias"]),
                         prefix + "ff.", rounded=True, block=i) + x
    return x


def build_context(net, t, ctx_list, n_class=4):
    ctx = np.concatenate([np.asarray(c).astype(F64) for c in ctx_list], axis=1)
    ctx = ctx.transpose(0, 2, 1)
    B = ctx.shape[0]
    eye = np.broadcast_to(np.eye(n_class, dtype=F64)[None], (B, n_class, n_class))
    ctx = np.concatenate([ctx, eye], axis=-1)
    t = np.asarray(t)
    if net.mutate == "t_plus_one":
        t = t + 1
    t_emb = feed_forward_glu(net, timestep_embedding(t, 256), "time_embed.")
    return np.concatenate([ctx, np.broadcast_to(t_emb[:, None, :], (B, ctx.shape[1], 256))], axis=-1)


def transformer_net_forward(W, x, t, ctx_list, anchors, variances, valid_id, anchor_assignment, n_class=4,
                            operand_round=None, mutate=None, w1_fold=None):
    """TransformerNet.forward; arguments as ``oracle.denoiser.transformer_net_forward`` (``W``: the fp32 dict or a ``Net``).
    Returns eps (B,3,N) float64."""
    net = as_net(W, operand_round, mutate, w1_fold)
    x = np.asarray(x).astype(F64)
    anchors, variances = np.asarray(anchors).astype(F64), np.asarray(variances).astype(F64)
    ctx = build_context(net, t, ctx_list, n_class)
    assert ctx.shape[-1] == 522
    onehot = np.eye(n_class, dtype=F64)[np.asarray(anchor_assignment).astype(np.int64)]  # (B,N,J)
    h = np.concatenate([x.transpose(0, 2, 1), anchors, variances, onehot], axis=-1)     # (B,N,13)
    assert h.shape[-1] == 13
    Wd = net.W
    h = linear(h, Wd["proj_in.weight"], Wd["proj_in.bias"])
    h = layer_norm(h, Wd["pre_norm.weight"], Wd["pre_norm.bias"])
    for i in range(net.depth):
        h = transformer_block(net, h, ctx, valid_id, i)
    h = layer_norm(h, Wd["post_norm.weight"], Wd["post_norm.bias"])
    h = linear(h, Wd["proj_out.weight"], Wd["proj_out.bias"])
    return np.ascontiguousarray(h.transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------ diffusion
def coef(tb, name, t):
    """The reference's fp32 table entry (``extract_into_tensor``), widened exactly."""
    return np.asarray(tb.f32(name, t)).astype(F64)


def _w(*arrays):
    return tuple(np.asarray(a).astype(F64) for a in arrays)


def predict_xstart_from_eps(tb, x_t, t, anchors, eps, sqrt_variance):
    return coef(tb, "sqrt_recip_alphas_cumprod", t) * (x_t - anchors) + anchors \
        - coef(tb, "sqrt_recipm1_alphas_cumprod", t) * sqrt_variance * eps


def q_posterior_mean(tb, x_start, x_t, t, anchors):
    return (coef(tb, "posterior_mean_coef1", t) * x_start + coef(tb, "posterior_mean_coef2", t) * x_t
            + coef(tb, "posterior_mean_coef3", t) * anchors)


def p_mean_variance(tb, W, x, t, anchors, ctx, variance, anchor_assignment, valid_id, operand_round=None, mutate=None, eps=None, w1_fold=None):
    """``eps``: the network's output on these very inputs, where the caller has it already (the network is then not run)."""
    x, anchors, variance = _w(x, anchors, variance)
    B = x.shape[0]
    if eps is None:
        eps = transformer_net_forward(as_net(W, operand_round, mutate, w1_fold), x, np.full((B,), t, dtype=np.int64), ctx,
                                      anchors.transpose(0, 2, 1), variance.transpose(0, 2, 1), valid_id, anchor_assignment)
    eps = np.asarray(eps).astype(F64)
    L = np.sqrt(variance)
    model_variance = coef(tb, "posterior_variance", t) * variance
    pred_xstart = predict_xstart_from_eps(tb, x, t, anchors, eps, L)
    mean = q_posterior_mean(tb, pred_xstart, x, t, anchors)
    return dict(mean=mean, variance=model_variance, pred_xstart=pred_xstart, eps=eps)


def p_sample(tb, W, x, t, anchors, ctx, variance, anchor_assignment, valid_id, noise, operand_round=None, mutate=None, eps=None, w1_fold=None):
    """DDPM step, or the DDIM step when ``tb.ddim_sampling`` (as ``oracle.diffusion.p_sample``).  ``eps``: see ``p_mean_variance``."""
    x, anchors, variance, noise = _w(x, anchors, variance, noise)
    out = p_mean_variance(tb, W, x, t, anchors, ctx, variance, anchor_assignment, valid_id, operand_round, mutate, eps, w1_fold)
    nz = 1.0 if t != 0 else 0.0
    if tb.ddim_sampling:
        xt_dir = np.sqrt(variance) * coef(tb, "xt_dir_coeff", t) * out["eps"]
        sample = ((out["pred_xstart"] - anchors) * np.sqrt(coef(tb, "alphas_cumprod_prev", t)) + anchors + xt_dir
                  + float(tb.ddim_eta) * nz * np.sqrt(out["variance"]) * noise)
    else:
        sample = out["mean"] + nz * np.sqrt(out["variance"]) * noise
    return dict(sample=sample, pred_xstart=out["pred_xstart"], eps=out["eps"])


def p_sample_loop_progressive(tb, W, anchors, ctx, variance, anchor_assignment, valid_id, x_T_noise, step_noise,
                              operand_round=None, mutate=None, w1_fold=None):
    net = as_net(W, operand_round, mutate, w1_fold)
    anchors, variance, x_T_noise = _w(anchors, variance, x_T_noise)
    pcd = np.sqrt(variance) * x_T_noise + anchors
    yield tb.T, dict(sample=pcd)
    for n, i in enumerate(tb.steps[::-1]):
        out = p_sample(tb, net, pcd, i, anchors, ctx, variance, anchor_assignment, valid_id, step_noise[n])
        yield i, out
        pcd = out["sample"]


def decode(tb, W, anchors, ctx, variance, anchor_assignment, valid_id, x_T_noise, step_noise, ret_traj=True, ret_interval=10,
           operand_round=None, mutate=None, w1_fold=None):
    """AnchorDiffAE.decode: 'pred' (B,N,3) and every ``ret_interval``-th t (t = T included) when ``ret_traj``."""
    final = {}
    for t, sample in p_sample_loop_progressive(tb, W, anchors, ctx, variance, anchor_assignment, valid_id, x_T_noise, step_noise,
                                               operand_round, mutate, w1_fold):
        if t == 0:
            final["pred"] = sample["sample"].transpose(0, 2, 1)
        elif ret_traj and t % ret_interval == 0:
            final[t] = sample["sample"].transpose(0, 2, 1)
    return final


def q_sample(tb, x_start, t, anchors, noise, variance):
    x_start, anchors, noise, variance = _w(x_start, anchors, noise, variance)
    sa = coef(tb, "sqrt_alphas_cumprod", t)[:, None, None]
    s1 = coef(tb, "sqrt_one_minus_alphas_cumprod", t)[:, None, None]
    return sa * (x_start - anchors) + anchors + s1 * np.sqrt(variance) * noise


def masked_mse(target, pred, flags=None):
    """((target - pred)^2 * flags).mean(1).sum() / flags.sum(), or the plain mean without flags."""
    target, pred = _w(target, pred)
    d = (target - pred) ** 2
    if flags is None:
        return float(d.mean())
    flags = np.asarray(flags).astype(F64)
    return float((d * flags).mean(axis=1).sum() / flags.sum())


def training_losses(tb, W, x_start, t, anchors, variance, ctx, anchor_assignment, valid_id, flags, noise,
                    operand_round=None, mutate=None, w1_fold=None):
    net = as_net(W, operand_round, mutate, w1_fold)
    anchors, variance = _w(anchors, variance)
    x_t = q_sample(tb, x_start, t, anchors, noise, variance)
    eps = transformer_net_forward(net, x_t, np.asarray(t, dtype=np.int64), ctx, anchors.transpose(0, 2, 1),
                                  variance.transpose(0, 2, 1), valid_id, anchor_assignment)
    return dict(mse_loss=masked_mse(noise, eps, flags), x_t=x_t, eps=eps)


# ------------------------------------------------------------------------------------------------ fp32, the kernels' accumulation order
def _accumulate_into(acc, x, w, terms_per_step):
    """acc (..., O) fp32 += x (..., K) @ w (O, K)^T, sequentially over K with one fp32 rounding of the accumulator per
    ``terms_per_step`` products (the products and the step's sum are exact here)."""
    shp = acc.shape
    a = np.ascontiguousarray(acc, dtype=np.float32).reshape(-1, shp[-1])
    x2 = np.asarray(x, dtype=F64).reshape(-1, x.shape[-1])
    w = np.asarray(w, dtype=F64)
    for k in range(0, x2.shape[1], terms_per_step):
        a = (a.astype(F64) + x2[:, k:k + terms_per_step] @ w[:, k:k + terms_per_step].T).astype(np.float32)
    return a.reshape(shp)


def fp32_residual_order_forward(W, x, t, ctx_list, anchors, variances, valid_id, anchor_assignment, terms_per_step=2, n_class=4):
    """The fp32 numpy oracle (``oracle.denoiser``, same functions) with ONE thing changed to what the fp32 kernels do: the to_out.0 and
    the FF net.2 products are accumulated term by term straight into the fp32 residual stream, as denoiser_kernel.hip ``attention``
    (``mma_tile<PREC>(h[t], ...)``) and ``ff_chunk`` (``mma_tile<PREC>(h[t], ck2 + ...)``) do with ``h`` as the C operand of a chain of
    64 / 256 ``v_mfma_f32_32x32x2_f32`` — every step rounds at the size of h, not at the size of the product.  ``terms_per_step``: 2 = one
    rounding per MFMA (two k), 1 = one per product.  Explains, and checks on the CPU, why the fp32 kernels' error is a multiple of the
    BLAS-ordered oracle's (tests/_errstats.py: R32)."""
    from . import denoiser as dn
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    ctx = dn.build_context(W, t, ctx_list, n_class)
    onehot = np.eye(n_class, dtype=f32)[np.asarray(anchor_assignment).astype(np.int64)]
    h = np.concatenate([x.transpose(0, 2, 1), anchors, variances, onehot], axis=-1).astype(f32)
    h = dn.layer_norm(dn.linear(h, W["proj_in.weight"], W["proj_in.bias"]), W["pre_norm.weight"], W["pre_norm.bias"])
    B, N, _ = h.shape
    heads, J = 8, ctx.shape[1]
    keep = np.asarray(valid_id).astype(bool)[:, None, None, :]
    for i in range(dn.depth_of(W)):
        p = f"transformer_blocks.{i}."
        xn = dn.layer_norm(h, W[p + "norm2.weight"], W[p + "norm2.bias"])
        q, k, v = (dn.linear(a, W[p + f"attn2.to_{n}.weight"]) for a, n in ((xn, "q"), (ctx, "k"), (ctx, "v")))
        d = q.shape[-1] // heads
        q = q.reshape(B, N, heads, d).transpose(0, 2, 1, 3)
        k = k.reshape(B, J, heads, d).transpose(0, 2, 1, 3)
        v = v.reshape(B, J, heads, d).transpose(0, 2, 1, 3)
        sim = (np.einsum("bhid,bhjd->bhij", q, k).astype(f32) * f32(d ** -0.5)).astype(f32)
        sim = np.where(keep, sim, f32(-np.finfo(np.float32).max)).astype(f32)
        e = np.exp(sim - sim.max(axis=-1, keepdims=True)).astype(f32)
        pr = (e / e.sum(axis=-1, keepdims=True, dtype=f32)).astype(f32)
        o = np.einsum("bhij,bhjd->bhid", pr, v).astype(f32).transpose(0, 2, 1, 3).reshape(B, N, heads * d)
        h = _accumulate_into((h + W[p + "attn2.to_out.0.bias"]).astype(f32), o, W[p + "attn2.to_out.0.weight"], terms_per_step)
        xn = dn.layer_norm(h, W[p + "norm3.weight"], W[p + "norm3.bias"])
        a, g = np.split(dn.linear(xn, W[p + "ff.net.0.proj.weight"], W[p + "ff.net.0.proj.bias"]), 2, axis=-1)
        h = _accumulate_into((h + W[p + "ff.net.2.bias"]).astype(f32), (a * dn.gelu(g)).astype(f32), W[p + "ff.net.2.weight"], terms_per_step)
    h = dn.linear(dn.layer_norm(h, W["post_norm.weight"], W["post_norm.bias"]), W["proj_out.weight"], W["proj_out.bias"])
    return np.ascontiguousarray(h.transpose(0, 2, 1)).astype(f32)
