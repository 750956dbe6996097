"""PyTorch-CPU restatement of the denoiser evaluation and the anchored DDPM step (ORACLE — test / baseline only).

Same unfused op sequence as the reference's modules, written with the torch CPU ops the reference itself would run
(`F.linear`, `F.layer_norm`, `F.gelu`, `softmax`, `einsum`): TransformerNet.forward attention.py:385-440, CrossAttention
:179-204, GEGLU FeedForward :50-94, timestep_embedding nets/utils.py:7-24, p_mean_variance / p_sample
anchored_diffusion.py:227-395, 450-484.  It exists for `bench.py`'s `cpu_baseline` leg — "the reference's CPU PyTorch path
timed on the box's host cores" cannot be the reference itself (it does not travel to the GPU box), so this restatement,
pinned to the same reference goldens as the numpy oracle (tests/test_oracle_golden.py), stands in for it — and as a second,
independent oracle.  Never imported by the product path.
"""
import math

import torch
import torch.nn.functional as F


def _w(W, k):
    return W[k]


def timestep_embedding(t, dim=256, max_period=10000, dtype=torch.float32):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=dtype) / half)
    args = t[:, None].to(dtype) * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


class RoundedLinear(torch.autograd.Function):
    """``F.linear`` with both operands of each of its three products passed through a rounding hook — the operand format of a
    matrix-pipe product, in whatever dtype the surrounding graph runs (the accumulation stays in that dtype):
    forward ``round(x) round(W)^T + b``; backward ``dX = round_b(dY) round_b(W)``, ``dW = round_b(dY)^T round_b(x)``, ``db = sum dY``.
    ``rounds`` = (round, round_b): the backward's hook is an argument of its own only so that a test can state a wrong one.  The
    products are written as autograd writes them for ``F.linear`` (rows flattened, ``x^T dY`` transposed), so the identity hook
    gives ``F.linear``'s bits in both directions."""

    @staticmethod
    def forward(ctx, rounds, x, w, b):
        rf, rb = rounds
        ctx.rb = rb
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.linear(rf(x), rf(w), b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        rb = ctx.rb
        dy2 = dy.reshape(-1, dy.shape[-1])
        dyr = rb(dy2)
        dx = dyr.mm(rb(w)).reshape(x.shape)
        dw = rb(x.reshape(-1, x.shape[-1])).t().mm(dyr).t()
        return None, dx, dw, (dy2.sum(0) if ctx.has_bias else None)


class ScaleFwdBwd(torch.autograd.Function):
    """y = x * f_fwd with the gradient dx = dy * f_bwd: a dropout whose backward may read OTHER factors than its forward applied
    (a stale mask word).  Used only by the deliberately wrong variants of oracle/train.py; f_bwd = f_fwd is the plain product."""

    @staticmethod
    def forward(ctx, x, f_fwd, f_bwd):
        ctx.save_for_backward(f_bwd)
        return x * f_fwd

    @staticmethod
    def backward(ctx, dy):
        return dy * ctx.saved_tensors[0], None, None


def _drop(h, drop):
    """drop: None, a factor tensor, or (forward factors, backward factors)."""
    if drop is None:
        return h
    if isinstance(drop, tuple):
        return ScaleFwdBwd.apply(h, drop[0], drop[1])
    return h * drop


def _lin(rounds):
    """The product at a matrix-pipe site: F.linear, or RoundedLinear with the hooks."""
    if rounds is None:
        return F.linear
    return lambda x, w, b=None: RoundedLinear.apply(rounds, x, w, b)


def feed_forward(x, W, p, drop=None, rounds=None, fold_norm=None):
    """drop: explicit dropout factors (0 or 1/(1-p)) behind the GEGLU (attention.py:84), or None (eval mode).
    fold_norm (with rounds): the parameter prefix of the LayerNorm in front; x is then that LayerNorm's INPUT and the first product is
    evaluated as the fused training kernels evaluate it (train_ff_fused.h:86-89, ``k_ff_pack``): (W1 diag(gamma)) xhat + (b1 + W1 beta)
    with the folded weight and the plain normalised row as the rounded operands, the folded bias in full precision."""
    lin = _lin(rounds)
    if fold_norm is not None:
        w1 = W[p + "net.0.proj.weight"]
        wf, bf = w1 * W[fold_norm + "weight"][None, :], W[p + "net.0.proj.bias"] + w1 @ W[fold_norm + "bias"]
        if drop is not None:   # the dropout scale 1 / (1 - p) rides on the `a` half of the folded weight and bias (PackArgs::keep_a); the factors only select
            keep = drop.max()
            scale = torch.cat([torch.full_like(bf[:bf.shape[0] // 2], float(keep)), torch.ones_like(bf[bf.shape[0] // 2:])])
            wf, bf, drop = wf * scale[:, None], bf * scale, drop / keep
        a, g = lin(F.layer_norm(x, (x.shape[-1],)), wf, bf).chunk(2, dim=-1)
    else:
        a, g = lin(x, W[p + "net.0.proj.weight"], W[p + "net.0.proj.bias"]).chunk(2, dim=-1)
    h = _drop(a * F.gelu(g), drop)
    return lin(h, W[p + "net.2.weight"], W[p + "net.2.bias"])


class RoundedBmm(torch.autograd.Function):
    """RoundedLinear with one weight per shape and no bias: y[b] = round(x[b]) round(w[b])^T, x (B,N,K), w (B,O,K)."""

    @staticmethod
    def forward(ctx, rounds, x, w):
        rf, rb = rounds
        ctx.rb = rb
        ctx.save_for_backward(x, w)
        return rf(x) @ rf(w).transpose(1, 2)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dyr = ctx.rb(dy)
        return None, dyr @ ctx.rb(w), dyr.transpose(1, 2) @ ctx.rb(x)


def folded_cross_attention(x, context, mask, W, p, heads, drop, rounds):
    """The same attention as the fused training kernels evaluate it (train_attn_fused.h:7-18): the four keys / values of a shape are
    the same for all its points, so per shape  A_s[(h, j)][c] = 1/4 sum_{d in h} k_j[d] Wq[d][c]  (32 x 128) and
    M_s[c][(h, j)] = sum_{d in h} Wo[c][d] v_j[d]  (128 x 32) are folded in full precision (``k_attn_fold``, fp32) and the two
    products over the points are  sim = A_s xn2  and  M_s P: THEIR operands are what the matrix pipe rounds — A_s, xn2, M_s and the
    32 softmax weights in the forward; dh1, dsim in the backward — and the gradients of Wq, Wo, k, v are unfolded from dA_s, dM_s in
    full precision (``k_attn_unfold_*``).  Equal to ``cross_attention`` in real arithmetic."""
    B, N, C = x.shape
    J = context.shape[1]
    k, v = F.linear(context, W[p + "to_k.weight"]), F.linear(context, W[p + "to_v.weight"])
    d = C // heads
    A = torch.einsum("bjhd,hdc->bhjc", k.reshape(B, J, heads, d), W[p + "to_q.weight"].reshape(heads, d, C)).reshape(B, heads * J, C) * d ** -0.5
    M = torch.einsum("chd,bjhd->bchj", W[p + "to_out.0.weight"].reshape(C, heads, d), v.reshape(B, J, heads, d)).reshape(B, C, heads * J)
    sim = RoundedBmm.apply(rounds, x, A).reshape(B, N, heads, J)
    if mask is not None:
        sim = sim.masked_fill(~mask.bool()[:, None, None, :], -torch.finfo(sim.dtype).max)
    out = RoundedBmm.apply(rounds, sim.softmax(dim=-1).reshape(B, N, heads * J), M) + W[p + "to_out.0.bias"]
    return _drop(out, drop)


def cross_attention(x, context, mask, W, p, heads=8, drop=None, rounds=None, fold=False):
    """fold (with rounds): the rounding sites of the fused training kernels' folded attention instead of the reference layout's."""
    if fold:
        return folded_cross_attention(x, context, mask, W, p, heads, drop, rounds)
    B, N, _ = x.shape
    J = context.shape[1]
    lin = _lin(rounds)
    q, k, v = lin(x, W[p + "to_q.weight"]), F.linear(context, W[p + "to_k.weight"]), F.linear(context, W[p + "to_v.weight"])
    d = q.shape[-1] // heads
    q, k, v = (t.reshape(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * d ** -0.5
    if mask is not None:
        sim = sim.masked_fill(~mask.bool()[:, None, None, :], -torch.finfo(sim.dtype).max)
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v).transpose(1, 2).reshape(B, N, heads * d)
    out = lin(out, W[p + "to_out.0.weight"], W[p + "to_out.0.bias"])
    return _drop(out, drop)   # to_out = Sequential(Linear, Dropout)  (attention.py:177)


def transformer_net_forward(W, x, t, ctx_list, anchors, variances, valid_id, anchor_assignment, n_class=4, depth=5, drops=None,
                            dtype=torch.float32, rounds=None, taps=None, between=None, attn_fold=False, ff_fold=False):
    """Arguments as oracle.denoiser.transformer_net_forward, torch CPU tensors; returns eps (B,3,N).
    dtype: every tensor is expected in it and the constants made here (timestep embedding, one-hot columns) follow it.
    rounds: None, or (round, round_backward) — the hooks of RoundedLinear at the four per-block products over the points (to_q,
    to_out.0, FF net.0, FF net.2; oracle/train.py lists why those).  taps: a dict that receives proj_in's output (`h0`) and
    pre_norm's (`hpre`, gradient retained).  between: a function applied to the residual stream between two blocks.  attn_fold: the
    attention's rounding sites as the fused training kernels have them (folded_cross_attention).  ff_fold: LayerNorm3's affine
    folded into the first feed-forward product, as they do (feed_forward: fold_norm)."""
    B = x.shape[0]
    ctx = torch.cat(ctx_list, dim=1).transpose(1, 2)
    ctx = torch.cat([ctx, torch.eye(n_class, dtype=dtype)[None].expand(B, -1, -1)], dim=-1)
    drops = drops or {}   # explicit dropout factors: {"te": (B,1024), ("attn", i): (B,N,128), ("ff", i): (B,N,512)}
    t_emb = feed_forward(timestep_embedding(t, dtype=dtype), W, "time_embed.", drops.get("te"))
    ctx = torch.cat([ctx, t_emb[:, None, :].expand(-1, ctx.shape[1], -1)], dim=-1)
    onehot = F.one_hot(anchor_assignment.long(), n_class).to(dtype)
    h = torch.cat([x.transpose(1, 2), anchors, variances, onehot], dim=-1)
    h0 = F.linear(h, W["proj_in.weight"], W["proj_in.bias"])
    h = F.layer_norm(h0, (128,), W["pre_norm.weight"], W["pre_norm.bias"])
    if taps is not None:
        if h.requires_grad:
            h.retain_grad()
        taps["h0"], taps["hpre"] = h0, h
    for i in range(depth):
        p = f"transformer_blocks.{i}."
        if between is not None and i > 0:
            h = between(h)
        h = cross_attention(F.layer_norm(h, (128,), W[p + "norm2.weight"], W[p + "norm2.bias"]), ctx, valid_id, W, p + "attn2.",
                            drop=drops.get(("attn", i)), rounds=rounds, fold=attn_fold and rounds is not None) + h
        if ff_fold and rounds is not None:
            h = feed_forward(h, W, p + "ff.", drops.get(("ff", i)), rounds, fold_norm=p + "norm3.") + h
        else:
            h = feed_forward(F.layer_norm(h, (128,), W[p + "norm3.weight"], W[p + "norm3.bias"]), W, p + "ff.", drops.get(("ff", i)), rounds) + h
    h = F.layer_norm(h, (128,), W["post_norm.weight"], W["post_norm.bias"])
    return F.linear(h, W["proj_out.weight"], W["proj_out.bias"]).transpose(1, 2)


def p_sample(tables, W, x, t, anchors, ctx_list, variance, anchor_assignment, valid_id, noise):
    """One reverse step; ``tables`` = oracle.diffusion.Tables (float64 numpy, cast to fp32 at use like the reference)."""
    B = x.shape[0]
    f = lambda name: float(getattr(tables, name).astype("float32")[t])
    eps = transformer_net_forward(W, x, torch.full((B,), t, dtype=torch.long), ctx_list, anchors.transpose(1, 2),
                                  variance.transpose(1, 2), valid_id, anchor_assignment)
    L = torch.sqrt(variance)
    x0 = f("sqrt_recip_alphas_cumprod") * (x - anchors) + anchors - f("sqrt_recipm1_alphas_cumprod") * L * eps
    mean = f("posterior_mean_coef1") * x0 + f("posterior_mean_coef2") * x + f("posterior_mean_coef3") * anchors
    nz = 1.0 if t != 0 else 0.0
    return mean + nz * torch.sqrt(f("posterior_variance") * variance) * noise, eps
