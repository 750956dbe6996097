"""PointNetV2 part encoder in TRAIN mode (batch-statistics BatchNorm) with gradients (ORACLE — test infrastructure only).

PyTorch-CPU restatement of python/difffacto/models/encoders/pointnet.py:187-213 (per_part_mlp=True) using
``F.batch_norm(training=True)`` exactly where the reference's ``nn.BatchNorm1d`` modules sit, differentiated by torch
autograd.  Pinned to the reference class's own autograd by tests/golden/pointnet_v2_train_*.npz.

The function is piecewise smooth: 512 ReLU channels per point in the trunk, 768 per shape in the heads, and a max over the points
per (shape, part, channel).  Two runs that round differently can land on different pieces, and their derivatives then differ by a
unit's whole share, so a float64 run is the truth of another implementation only on the piece that implementation took:
  record=   a dict that receives, in the layouts of the HIP kernels' workspace, every ReLU site's pre-activation (`pre`: bn1 / bn2 / bn3
            (B N, C), mlp_m.1 / mlp_m.4 / mlp_v.1 / mlp_v.4 (B, 4 C)), the pool's input `pool_in` (B N, 512), its selected point per (shape, part,
            channel) `sel` (B, 4, 512), -1 where the maximum is the 0 of a non-member point (zero gradient whichever point is named: one state), and
            `gap`, the distance from the maximum to the runner-up among the member points' values and that 0.
  branch=   {site: mask (kernel layout, non-zero = the gradient passes), "pool": sel} forces those choices IN THE DERIVATIVE ONLY: the forward
            values stay the true ReLU / max.
  head_products="chain"   the heads' grouped products with their sums over K as one chain of fused multiply-adds (_ChainGroupedLinear): the fp32
            yardstick of kernels that accumulate on a matrix pipe.  chain_order=seed takes the chains' terms in a drawn order: another draw of
            the same implementation's rounding error.
  head_bn="written"       the heads' BatchNorm over the B rows, and bn4 in front of the pool, with fp32 reductions, the mean as sum x fl(1 / R) and the
            backward written out (_WrittenOutBatchNorm): the layers whose bias gradients are the large mathematically zero ones.
The defaults (fp32, no record, no branch, torch's products) run exactly the statements they always ran.
"""
import numpy as np
import torch
import torch.nn.functional as F

TRUNK_SITES = ("bn1", "bn2", "bn3")
HEAD_SITES = ("mlp_m.1", "mlp_m.4", "mlp_v.1", "mlp_v.4")


class _ForcedReLU(torch.autograd.Function):
    """relu(x) whose derivative is the given 0 / 1 mask."""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return F.relu(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def _fma(acc, a, b):
    """fp32 acc + a b with one rounding (the product of two fp32 numbers is exact in float64)."""
    return (acc.double() + a.double() * b.double()).to(acc.dtype)


class _ChainGroupedLinear(torch.autograd.Function):
    """The heads' grouped 1x1 convolution over the B rows with every sum over K taken as ONE chain of fused multiply-adds in index order — how
    a matrix pipe accumulates (one accumulator per output, K steps) — in the forward product, in the input gradient (chain over the output
    channels) and in the weight gradient (chain over the rows).  torch's own fp32 products take such a chain from a few dozen rows on; below
    that (the heads: B rows) they sum K in interleaved partial sums, whose rounding error measures 2.7 - 3.4 x smaller (K = 128 .. 512)."""

    @staticmethod
    def forward(ctx, x, W, b, groups, order):
        B, G = x.shape[0], groups
        ctx.order = order
        xg, Wg = x.reshape(B, G, -1).transpose(0, 1), W.reshape(G, W.shape[0] // G, W.shape[1])       # (G,B,K), (G,N,K)
        ctx.save_for_backward(xg, Wg)
        acc = torch.zeros(G, B, Wg.shape[1], dtype=x.dtype)
        for k in _chain_order(Wg.shape[2], order):
            acc = _fma(acc, xg[:, :, k, None], Wg[:, None, :, k])
        return (acc + b.reshape(G, 1, -1)).transpose(0, 1).reshape(B, -1)

    @staticmethod
    def backward(ctx, dy):
        xg, Wg = ctx.saved_tensors
        G, B, K = xg.shape
        dyg = dy.reshape(B, G, -1).transpose(0, 1)                                                       # (G,B,N)
        dx = torch.zeros(G, B, K, dtype=dy.dtype)
        for n in _chain_order(Wg.shape[1], ctx.order):
            dx = _fma(dx, dyg[:, :, n, None], Wg[:, None, n, :])
        dW, db = torch.zeros_like(Wg), torch.zeros(G, Wg.shape[1], dtype=dy.dtype)
        for r in range(B):
            dW = _fma(dW, dyg[:, r, :, None], xg[:, r, None, :])
            db = db + dyg[:, r]
        return dx.transpose(0, 1).reshape(B, -1), dW.reshape(-1, K, 1), db.reshape(-1), None, None


def _chain_order(n, order):
    """The order in which a chain takes its n terms: index order (order None or 0), or the permutation drawn from seed `order` — every order is an
    fp32 chain of the same quality with another draw of its rounding error (a matrix pipe's own order is a permutation too: two terms per step)."""
    return range(n) if not order else [int(i) for i in np.random.Generator(np.random.PCG64(1000 * order + n)).permutation(n)]


def _sum4(a):
    """Column sums of a (R, C) the way a 256-thread workgroup with four row groups takes them: rows r = j (mod 4) in order, then (s0 + s1) + (s2 + s3)."""
    parts = []
    for j in range(4):
        if a.shape[0] > 512:          # (many rows: the row groups' sums as torch takes them; the kernels go through slabs of rows there)
            parts.append(a[j::4].sum(0))
            continue
        s = torch.zeros(a.shape[1], dtype=a.dtype)
        for r in range(j, a.shape[0], 4):
            s = s + a[r]
        parts.append(s)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


class _WrittenOutBatchNorm(torch.autograd.Function):
    """Batch-statistics BatchNorm over a few rows with every reduction in the working precision and the backward written out:
    dz = g rstd (dy - sum(dy) / R - xhat sum(dy xhat) / R), the sums over four row groups.  The gradient of a bias in front of the BatchNorm is
    mathematically zero: in fp32 it is the rounding left over when sum(dz) cancels, and how much is left follows the arrangement of these
    statements — torch's own CPU BatchNorm arranges them differently and leaves several times less or more, channel by channel."""

    @staticmethod
    def forward(ctx, z, g, b, rm, rv, momentum, eps):
        R = z.shape[0]
        inv = torch.tensor(1.0 / R, dtype=z.dtype)
        mu = _sum4(z) * inv
        var = _sum4((z - mu) * (z - mu)) * inv
        rs = 1.0 / torch.sqrt(var + eps)
        xh = (z - mu) * rs
        if momentum >= 0:
            rm.copy_((1 - momentum) * rm + momentum * mu)
            rv.copy_((1 - momentum) * rv + momentum * var * torch.tensor(R / (R - 1) if R > 1 else 1.0, dtype=z.dtype))
        ctx.save_for_backward(xh, rs, g, inv)
        return xh * g + b

    @staticmethod
    def backward(ctx, dy):
        xh, rs, g, inv = ctx.saved_tensors
        db, dg = _sum4(dy), _sum4(dy * xh)
        return g * rs * (dy - db * inv - xh * dg * inv), dg, db, None, None, None, None


def _pool_record(w, attn, idx, record):
    """w (B,512,N,A), attn (B,N,A), idx (B,512,A): the max's own index."""
    B, C, N, A = w.shape
    member = (attn != 0)
    hit = member.unsqueeze(1).expand(B, C, N, A).gather(2, idx.unsqueeze(2)).squeeze(2)
    record["sel"] = torch.where(hit, idx, torch.full_like(idx, -1)).permute(0, 2, 1).contiguous().numpy().astype(np.int32)
    if record.get("light"):
        return
    ninf = torch.tensor(float("-inf"), dtype=w.dtype)
    top = torch.where(member.unsqueeze(1), w.detach(), ninf).topk(min(2, N), dim=2).values            # (B,512,<=2,A)
    zero = torch.where((~member).any(1), torch.zeros((), dtype=w.dtype), ninf).view(B, 1, 1, A).expand(B, C, 1, A)
    cand = torch.cat([top, zero], 2).sort(dim=2, descending=True).values
    gap = cand[:, :, 0] - cand[:, :, 1]
    record["gap"] = torch.nan_to_num(gap, nan=float("inf")).permute(0, 2, 1).contiguous().numpy()


def forward(Wt, x, attn, num_anchors=4, reweight_by_anchor=True, eps=1e-5, momentum=0.1, running=None, record=None, branch=None,
            head_products="torch", head_bn="torch", chain_order=None):
    """Wt: dict name -> torch tensor (state_dict names).  x (B,N,3), attn (B,N,A) torch tensors.  `running`: optional dict that
    receives the updated running statistics (as nn.BatchNorm1d would leave them).  Returns m, v (B, A, zdim)."""
    B, N = x.shape[0], x.shape[1]
    if record is not None:
        record["pre"] = {}

    def bn(h, p):
        rm = Wt[p + "running_mean"].detach().clone()
        rv = Wt[p + "running_var"].detach().clone()
        if head_bn == "written" and (p.startswith("mlp_") or p == "bn4."):
            C = h.shape[1]
            y = _WrittenOutBatchNorm.apply(h.transpose(1, 2).reshape(-1, C), Wt[p + "weight"], Wt[p + "bias"], rm, rv, momentum, eps)
            y = y.reshape(h.shape[0], h.shape[2], C).transpose(1, 2)
            if running is not None:
                running[p + "running_mean"], running[p + "running_var"] = rm, rv
            return y
        y = F.batch_norm(h, rm, rv, Wt[p + "weight"], Wt[p + "bias"], training=True, momentum=momentum, eps=eps)
        if running is not None:
            running[p + "running_mean"], running[p + "running_var"] = rm, rv
        return y

    def relu(h, site):
        """h (B, C, L): rows (b, l), columns C in the kernels' layout."""
        if record is not None:
            record["pre"][site] = h.detach().transpose(1, 2).reshape(-1, h.shape[1]).numpy()
        if branch is None:
            return F.relu(h)
        mask = torch.from_numpy(np.ascontiguousarray(branch[site])).reshape(B, h.shape[2], h.shape[1]).transpose(1, 2)
        return _ForcedReLU.apply(h, (mask != 0).to(h.dtype))

    h = x.transpose(1, 2)
    for i in (1, 2, 3, 4):
        h = bn(F.conv1d(h, Wt[f"conv{i}.weight"], Wt[f"conv{i}.bias"]), f"bn{i}.")
        if i < 4:
            h = relu(h, f"bn{i}")
    w = h.unsqueeze(-1) * attn.unsqueeze(1)
    if reweight_by_anchor:
        w = w * num_anchors
    if record is None and branch is None:
        pooled = torch.max(w, 2, keepdim=True)[0].view(B, 512, num_anchors)
    else:
        mx, idx = torch.max(w, 2)
        pooled = mx
        if record is not None:
            if not record.get("light"):
                record["pool_in"] = (h.detach() * (num_anchors if reweight_by_anchor else 1)).transpose(1, 2).reshape(B * N, 512).numpy()
            _pool_record(w, attn, idx, record)
        if branch is not None:
            sel = torch.from_numpy(np.ascontiguousarray(branch["pool"])).long().permute(0, 2, 1)       # (B,512,A)
            picked = w.gather(2, sel.clamp_min(0).unsqueeze(2)).squeeze(2) * (sel >= 0).to(w.dtype)
            pooled = picked + (mx - picked).detach()
    z = pooled.transpose(1, 2).reshape(B, -1, 1)
    gconv = lambda t, p: F.conv1d(t, Wt[p + ".weight"], Wt[p + ".bias"], groups=num_anchors)
    if head_products == "chain":       # (a restated fp32 yardstick: _ChainGroupedLinear)
        gconv = lambda t, p: _ChainGroupedLinear.apply(t[:, :, 0], Wt[p + ".weight"], Wt[p + ".bias"], num_anchors, chain_order).unsqueeze(-1)
    else:
        assert head_products == "torch", head_products
    outs = []
    for name in ("mlp_m", "mlp_v"):
        t = relu(bn(gconv(z, name + ".0"), name + ".1."), name + ".1")
        t = relu(bn(gconv(t, name + ".3"), name + ".4."), name + ".4")
        t = gconv(t, name + ".6")
        outs.append(t.reshape(B, num_anchors, -1))
    return outs[0], outs[1]


def outputs_and_grads(W, x, attn, dm, dv, dtype=torch.float32, record=False, branch=None, **kw):
    """numpy in / out: m, v, updated running statistics, and d (sum(m dm) + sum(v dv)) / d (every trainable parameter), computed in `dtype`.
    record = True adds the entry `record` (module docstring); branch: module docstring."""
    Wt = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone() for k, a in W.items()}
    for k, t in Wt.items():
        if "running" not in k:
            t.requires_grad_(True)
    running = {}
    rec = ({"light": True} if record == "light" else {}) if record else None    # "light": pre-activations and sel only (no pool_in, no gap)
    m, v = forward(Wt, torch.from_numpy(x).to(dtype), torch.from_numpy(attn).to(dtype), running=running, record=rec, branch=branch, **kw)
    ((m * torch.from_numpy(dm).to(dtype)).sum() + (v * torch.from_numpy(dv).to(dtype)).sum()).backward()
    out = dict(m=m.detach().numpy(), v=v.detach().numpy(), running={k: t.numpy() for k, t in running.items()},
               grads={k: t.grad.numpy() for k, t in Wt.items() if t.requires_grad})
    if record:
        out["record"] = rec
    return out
