"""Prior loss of the part encoder with gradients (ORACLE — test infrastructure only).

PyTorch-CPU restatement of PartEncoder.get_prior_loss (part_encoders.py:1143-1182, use_flow=True): per part, the valid shapes'
latents go FORWARD through that part's 14 coupling layers (flow.py:9-49: y1 = x1 sigmoid(s + 2) + t, logpx - log det),
log p(w) under N(0, prior_var) — with the reference's own normalisation constant, -0.5 log(2 pi) * dim PER ELEMENT
(misc.py:301-317 called with dim = 256 and summed over the 256 elements) — minus the Gaussian entropy of the posterior
(misc.py:292-295), averaged over the valid parts of a shape and over the batch, times kl_weight.  Pinned to the reference by
tests/golden/prior_loss_*.npz.

The 2 x 14 x 4 ReLU layers of the coupling nets make the loss piecewise smooth; a float64 run is the truth of another implementation only on
the piece that implementation took (oracle/pointnet_v2_train.py says why):
  record=   a dict that receives the pre-activations of net_s_t.0 (`h1`) and net_s_t.2 (`h2`) of every layer, (depth, M B, H) with the rows
            part-major (part * B + shape) as in the HIP kernels' workspace.
  branch=   {"h1": masks, "h2": masks} of those shapes (non-zero = the gradient passes) forces the ReLU choices IN THE DERIVATIVE ONLY.
The defaults (fp32, no record, no branch) run exactly the statements they always ran.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


class _ForcedReLU(torch.autograd.Function):
    """relu(x) whose derivative is the given 0 / 1 mask."""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return F.relu(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def coupling_forward(x, W, prefix, swap, relu=lambda h, site: F.relu(h)):
    d = x.shape[1] - x.shape[1] // 2
    if swap:
        x = torch.cat([x[:, d:], x[:, :d]], 1)
    h = relu(F.linear(x[:, :d], W[prefix + "0.weight"], W[prefix + "0.bias"]), "h1")
    h = relu(F.linear(h, W[prefix + "2.weight"], W[prefix + "2.bias"]), "h2")
    s_t = F.linear(h, W[prefix + "4.weight"], W[prefix + "4.bias"])
    out = x.shape[1] - d
    scale = torch.sigmoid(s_t[:, :out] + 2.0)
    y1 = x[:, d:] * scale + s_t[:, out:]
    logdet = torch.log(scale).sum(1)
    y = torch.cat([y1, x[:, :d]], 1) if swap else torch.cat([x[:, :d], y1], 1)
    return y, logdet


def prior_loss(W, part_code, logvar, valid, depth=14, prior_var=1.0, kl_weight=5e-4, record=None, branch=None):
    """part_code (B, C, M), logvar (B, M, C), valid (B, M) torch tensors; W: dict 'flow.{i}.chain.{l}.net_s_t.*' -> tensors.
    Returns (loss, log_p_part (B, M), entropy (B, M))."""
    B, C, M = part_code.shape
    entropy = 0.5 * logvar.reshape(B * M, -1).sum(1) + 0.5 * C * (1.0 + math.log(2 * math.pi))
    log_p = torch.zeros(B, M)
    cols = []
    pre = {"h1": [[None] * M for _ in range(depth)], "h2": [[None] * M for _ in range(depth)]}
    for i in range(M):
        x = part_code[:, :, i]
        delta = torch.zeros(B, dtype=part_code.dtype)
        for l in range(depth):
            def relu(h, site, i=i, l=l):
                if record is not None:
                    pre[site][l][i] = h.detach()
                if branch is None:
                    return F.relu(h)
                mask = torch.from_numpy(np.ascontiguousarray(branch[site][l, i * B:(i + 1) * B]))
                return _ForcedReLU.apply(h, (mask != 0).to(h.dtype))
            x, ld = coupling_forward(x, W, f"flow.{i}.chain.{l}.net_s_t.", swap=(l % 2 == 0), relu=relu)
            delta = delta - ld
        log_pw = (-math.log(prior_var) - 0.5 * math.log(2 * math.pi) * C - x.pow(2) / (2.0 * prior_var)).sum(1)
        cols.append(torch.where(valid[:, i] == 1, log_pw - delta, torch.zeros(B, dtype=part_code.dtype)))
    log_p = torch.stack(cols, 1)
    if record is not None:
        for site in pre:
            record[site] = torch.stack([torch.cat(rows, 0) for rows in pre[site]], 0).numpy()
    entropy = entropy.view(B, M)
    loss_prior = ((-log_p - entropy) * valid).sum(1) / valid.sum(1)
    return kl_weight * loss_prior.mean(), log_p, entropy


def loss_and_grads(W, part_code, logvar, valid, dtype=torch.float32, record=False, branch=None, **kw):
    """numpy in / out: loss, log_p_part, entropy, d loss / d (part_code, logvar, every flow parameter), computed in `dtype`.
    record = True adds the entry `record` (module docstring); branch: module docstring."""
    Wt = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone().requires_grad_(True) for k, a in W.items() if k.startswith("flow.")}
    z = torch.from_numpy(part_code).to(dtype).clone().requires_grad_(True)
    lv = torch.from_numpy(logvar).to(dtype).clone().requires_grad_(True)
    rec = {} if record else None
    loss, log_p, ent = prior_loss(Wt, z, lv, torch.from_numpy(valid).to(dtype), record=rec, branch=branch, **kw)
    loss.backward()
    out = dict(loss=float(loss.detach()), log_p=log_p.detach().numpy(), entropy=ent.detach().numpy(), d_part_code=z.grad.numpy(),
               d_logvar=lv.grad.numpy(), grads={k: t.grad.numpy() for k, t in Wt.items()})
    if record:
        out["record"] = rec
    return out
