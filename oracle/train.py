"""Gradient oracle for the training-mode denoiser (ORACLE — test infrastructure only, never imported by the product).

PyTorch-CPU autograd over the restated forward of oracle/torch_cpu.py (TransformerNet.forward attention.py:385-440,
dropout = 0) and the masked mse_loss of AnchoredDiffusion.training_losses (anchored_diffusion.py:840-847).  Pinned to
the reference's own autograd by tests/golden/train_grads_*.npz (tests/test_oracle_golden.py).

Three things come out of ``loss_and_grads`` (tests/_gradstats.py, tests/test_gpu_train_highprec.py judge kernels with them):

* ``dtype=torch.float64``: the truth.  Every tensor, the timestep embedding and the one-hot columns are float64; the fp32 inputs are
  widened exactly.  ``|dtype=torch.float32 run - truth|`` is what fp32 arithmetic costs (the yardstick of the fp32 kernels).
* ``dtype=torch.float64, operand_round=round_bf16``: the *rounding model* of the bf16 training kernels.  At every product that those
  kernels run on the matrix pipe, both operands are rounded to bf16 — in the forward and in the two backward products (input
  gradient and weight gradient, oracle.torch_cpu.RoundedLinear) — and nothing else is.  ``|model - truth|`` is what the operand
  format costs (the yardstick of the bf16 kernels).  The model holds no constant fitted to a kernel's output.
* ``dtype=torch.float32, operand_round=round_bf16``: the same model in fp32 arithmetic, a stand-in for a correct bf16 kernel, and
  ``mutate=`` its deliberately wrong variants (tests/test_oracle_train_highprec_cpu.py).

Sites of the hook — the products over the B x N points, per transformer block (difffacto_amd/csrc/train_kernels.hip):

  product (forward; backward dX, dW)     layer-by-layer bf16 path (``lin`` :1773, ``wgrad`` :1824 -> gemm_bf16.h)       fused bf16 path
  to_q       xn2 Wq^T                    fwd :2344 (xn2 stored bf16); dX :2528, dW :2526 (dq stored bf16)               ``k_attn_fold`` (train_attn_fused.h:76) folds A_s = scale K_s Wq into a
                                                                                                                        per-shape 32 x 128 bf16 operand; the other operand is xn2
  to_out.0   att Wo^T + bo               fwd :2353 / :2355 (att stored bf16); dX :2521, dW :2519                        folded M_s = Wo V_s (128 x 32 bf16), operand = the 32 softmax weights;
                                                                                                                        dWq / dWo unfolded by ``k_attn_unfold_w`` in fp32
  FF net.0   xn3 W1^T + b1               fwd :2358 ([a | g] stored bf16, AG_BF16); dX :2511, dW :2509                   ``k_ff_pack`` (train_ff_fused.h:106) packs W1 diag(gamma3) as bf16; operand xhat3;
                                                                                                                        dW1 = G diag(g3) + db1 (x) b3 (``k_ff_wgrad_finish`` :2079)
  FF net.2   hid W2^T + b2               fwd :2362 (hid stored bf16); dX :2505, dW :2503                                fp16 GEMM2 with the polynomial GEGLU in the forward, bf16 in the backward

  NOT rounded, in the model as in the kernels:
  * to_k / to_v and their gradients: rows = the B x 4 context tokens.  ``lin`` takes the bf16 kernel only from 256 rows
    (gemm_bf16.h ``nt_ok``: M >= 256) and ``wgrad`` only from R >= 256 (:1835), i.e. from B = 64; below that — every case of the
    test files — they are the fp32 kernels on either path (fused: :2291, :2571, :2576).  From B = 64 the kernels do round them and
    this model would understate them.
  * the time embedding's two products (B rows; :2259, :2261, :2589-2593): fp32 for the same reason.
  * stem and head: proj_in has K = 13 padded to 16, not a multiple of gemm_bf16.h's TK = 32, so ``lin`` :2287 / ``wgrad`` :2583 are
    fp32; the fused path's ``k_stem_fwd`` / ``k_stem_bwd`` / ``k_stem_dx`` / ``k_head_bwd`` and the layer path's ``k_eps_fwd`` /
    ``k_eps_bwd`` are fp32 VALU kernels.
  * LayerNorm statistics, softmax, GEGLU, dropout, bias sums: fp32 VALU work.

The model rounds at the REFERENCE's layout of the four products, which is the layer-by-layer path's: that path's errors correlate
0.996 - 0.999 with the model's, element by element.  The fused path rounds OTHER matrices, and a weight's rounding error is shared by
all points — a coherent error, of which another rounded matrix is another draw: against the reference-layout model the fused kernels
measured 0.46 x to 2.1 x rms (3.7 x for one head's share of d to_q.weight), anti-correlated with the model's W1 component.  Two
switches restate the fused operands, and with both the fused kernels sit at <= 1.18 x rms with correlation 0.97 (tests/_gradstats.py):
  * ``attn_fold``: the attention's two products as oracle.torch_cpu.folded_cross_attention — A_s, xn2, M_s, the 32 softmax weights, dh1
    and dsim are the rounded operands; the folds and unfolds themselves are full precision (fp32 kernels).
  * ``ff_fold``: FF net.0 as (W1 diag(gamma3)) xhat3 + (b1 + W1 beta3): the folded weight and the plain normalised row are the rounded
    operands, the folded bias is exact, and with dropout the scale 1 / (1 - p) rides on the `a` half of the folded weight and bias
    (PackArgs::keep_a) while the factors only select.  The gradients of W1, gamma3, beta3 follow by autograd from the folded ones in
    full precision, as ``k_ff_wgrad_finish`` / ``k_ln3_param`` unfold them in fp32.
Not restated, and measured not to matter (each under 5 % of the yardstick): the fused kernels' sigmoid-form GELU, the forward's fp16
polynomial GEGLU with its fp16 GEMM2 (the model rounds that site to bf16 in both directions), the bf16 pair (hi + lo, 2^-17) that carries the
gradient between two blocks (the MFMA operand is the hi half = the round-to-nearest bf16 the model applies to dY).
"""
import numpy as np
import torch

from . import torch_cpu
from .highprec import round_bf16 as _round_bf16_np

MUTATIONS = ("truncate", "fold_bias_term", "chunk_scale", "halve_unit", "stale_mask_tile", "stem_dx_term", "lost_lo")
MUT_BLOCK, MUT_CHUNK, MUT_UNIT, MUT_TILE = 2, 5, 200, 1    # block, 32-unit chunk, hidden unit (row of ff0), 32-point tile of a mutation


def round_bf16(x, truncate=False):
    """oracle.highprec.round_bf16 on a torch tensor of any float dtype (-> fp32 -> bf16 -> the tensor's dtype)."""
    return torch.from_numpy(_round_bf16_np(x.detach().numpy(), truncate=truncate)).to(x.dtype)


def truncate_bf16(x):
    return round_bf16(x, truncate=True)


def identity(x):
    return x


class _RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16: the residual stream's gradient between two blocks with the lo half of the pair lost."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        return round_bf16(dy)


def masked_mse(target, pred, flags):
    """((target - pred)^2 * flags).mean(1).sum() / flags.sum(); flags (B,1,N) or None -> plain mean."""
    d = (target - pred) ** 2
    if flags is None:
        return d.mean()
    return (d * flags).mean(dim=1).sum() / flags.sum()


def loss_and_grads(W, x_t, t, ctx_code, ctx_mv, anchors_pt, variances_pt, valid, assignment, noise, flags, drops=None,
                   dtype=torch.float32, operand_round=None, mutate=None, attn_fold=False, ff_fold=False):
    """W: dict name -> float32 numpy array.  x_t, noise (B,3,N); anchors_pt, variances_pt (B,N,3); flags (B,1,N) or None.
    drops: explicit dropout factors as numpy arrays, keys as in oracle.torch_cpu.transformer_net_forward, or None.
    dtype: torch.float32 (the fp32 oracle the goldens pin) or torch.float64 (module docstring).
    operand_round: None or a callable tensor -> tensor (``round_bf16``; ``identity`` must change nothing), module docstring.
    attn_fold, ff_fold (with operand_round): the attention's two products / the first feed-forward product rounded where the FUSED path
      rounds them (module docstring); both together are the fused path's yardstick.
    mutate: None or one of MUTATIONS — deliberately wrong variants, for the self-test of the acceptance function only:
      truncate         the two backward products of every site truncate to bf16 instead of rounding (needs operand_round)
      fold_bias_term   every block's ff0 weight gradient without the db1 (x) beta3 term of the LayerNorm3 fold
      chunk_scale      (needs drops) rows of chunk MUT_CHUNK's `a` half of block MUT_BLOCK's dW1 and db1 left multiplied by 1/(1-p)
      halve_unit       row MUT_UNIT of block MUT_BLOCK's ff0 weight gradient halved
      stale_mask_tile  (needs drops) block MUT_BLOCK's FF dropout backward reads tile MUT_TILE + 1's factors for the 32 points of tile MUT_TILE of every shape
      stem_dx_term     d_x / d_variances from a pre_norm backward without the xhat * mean(dy g xhat) term
      lost_lo          the gradient between two blocks rounded to bf16 (reported by the self-test, not required to fail)
    Returns dict(loss, eps, grads{name: array}, d_ctx_code, d_ctx_mv, d_x (B,3,N), d_variances (B,N,3)) as numpy in `dtype`."""
    assert mutate is None or mutate in MUTATIONS, mutate
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    leaf = lambda a: tt(a).clone().requires_grad_(True)
    Wt = {k: leaf(v) for k, v in W.items()}
    cc, cm, xt, vr = leaf(ctx_code), leaf(ctx_mv), leaf(x_t), leaf(variances_pt)
    depth = 0
    while f"transformer_blocks.{depth}.norm2.weight" in W:
        depth += 1
    rounds = None
    if operand_round is not None:
        rounds = (operand_round, truncate_bf16 if mutate == "truncate" else operand_round)
    else:
        assert mutate != "truncate", "truncate is a mutation of the rounding model"
    td = None if drops is None else {k: tt(v) for k, v in drops.items()}
    p_keep = None
    if mutate in ("chunk_scale", "stale_mask_tile"):
        assert td is not None, f"{mutate} is a mutation of the dropout path"
        p_keep = float(td[("ff", MUT_BLOCK)].max())     # 1 / (1 - p)
    if mutate == "stale_mask_tile":
        f = td[("ff", MUT_BLOCK)]
        fb = f.clone()
        fb[:, 32 * MUT_TILE:32 * (MUT_TILE + 1)] = f[:, 32 * (MUT_TILE + 1):32 * (MUT_TILE + 2)]
        td[("ff", MUT_BLOCK)] = (f, fb)
    taps = {} if mutate == "stem_dx_term" else None
    eps = torch_cpu.transformer_net_forward(Wt, xt, torch.from_numpy(np.asarray(t, dtype=np.int64)), [cc, cm], tt(anchors_pt), vr,
                                            None if valid is None else torch.from_numpy(valid), torch.from_numpy(np.asarray(assignment)),
                                            depth=depth, drops=td, dtype=dtype, rounds=rounds, taps=taps, attn_fold=attn_fold, ff_fold=ff_fold,
                                            between=_RoundGrad.apply if mutate == "lost_lo" else None)
    loss = masked_mse(tt(noise), eps, None if flags is None else tt(flags))
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in Wt.items() if v.grad is not None}
    d_x, d_var = xt.grad.numpy(), vr.grad.numpy()
    blk = f"transformer_blocks.{MUT_BLOCK}.ff.net.0.proj."
    if mutate == "fold_bias_term":
        for i in range(depth):
            p = f"transformer_blocks.{i}."
            grads[p + "ff.net.0.proj.weight"] = grads[p + "ff.net.0.proj.weight"] - np.outer(grads[p + "ff.net.0.proj.bias"], np.asarray(W[p + "norm3.bias"]).astype(grads[p + "ff.net.0.proj.bias"].dtype))
    elif mutate == "chunk_scale":
        rows = slice(32 * MUT_CHUNK, 32 * (MUT_CHUNK + 1))
        for k in ("weight", "bias"):
            g = grads[blk + k].copy()
            g[rows] *= p_keep
            grads[blk + k] = g
    elif mutate == "halve_unit":
        g = grads[blk + "weight"].copy()
        g[MUT_UNIT] *= 0.5
        grads[blk + "weight"] = g
    elif mutate == "stem_dx_term":
        with torch.no_grad():
            h0, dy = taps["h0"], taps["hpre"].grad
            rstd = 1.0 / torch.sqrt(h0.var(dim=-1, unbiased=False, keepdim=True) + 1e-5)
            dyg = dy * Wt["pre_norm.weight"]
            d0 = rstd * (dyg - dyg.mean(dim=-1, keepdim=True))          # the xhat * mean(dyg * xhat) term is missing
            din = d0 @ Wt["proj_in.weight"]                             # (B, N, 13): x 0..2, anchors 3..5, variances 6..8, one-hot 9..12
            d_x, d_var = din[..., 0:3].transpose(1, 2).contiguous().numpy(), din[..., 6:9].contiguous().numpy()
    return dict(loss=float(loss.detach()), eps=eps.detach().numpy(), grads=grads, d_ctx_code=cc.grad.numpy(), d_ctx_mv=cm.grad.numpy(),
                d_x=d_x, d_variances=d_var)
