"""Generation metrics on libdfx's Chamfer / EMD kernels — mirrors the metric functions of
python/difffacto/datasets/evaluation_utils.py (``emd_approx`` :84-89, ``EMD_CD`` :106-140, ``_pairwise_EMD_CD_`` :143-202,
``knn`` :207-248, ``lgan_mmd_cov`` :251-278, ``compute_all_metrics`` :500-560): MMD / COV / 1-NNA under CD and EMD.

The distance work (nearest-neighbour scans, the auction) is native; what remains in torch is bookkeeping on the small
(N_sample x N_ref) distance matrices.  Point clouds are (num_clouds, n, 3) float32 device tensors.

The part-level metrics of the gen_part evaluation (snapping, part boxes, per-part metrics; ``evaluate_gen_part``) follow below,
then the occupancy-grid JSD (``jsd_between_point_cloud_sets`` :568-583 and its helpers, ``part_jsd``)."""
import functools
import warnings

import numpy as np
import torch

from . import _ffi
from .metrics import EMD, ChamferDistanceL2_split


def distChamferCUDA(x, y):
    """(dist1 (B,n), dist2 (B,m)) squared nearest-neighbour distances (evaluation_utils.py:17-19)."""
    return ChamferDistanceL2_split(reduce=False)(x, y)


def emd_approx(sample, ref):
    assert sample.size(1) == ref.size(1), "Not sure what would EMD do in this case"
    return EMD(0.002, 10000, True)(sample, ref)   # (B,)


# One workgroup of the auction kernel serves one pair of clouds and owns a compute unit while it runs (its state fills most of the
# 160 KiB of LDS): a launch of the reference's `batch_size` (32) pairs would leave 7/8 of the chip idle for the 54 ms an auction
# takes.  The pairs are independent, so they go to the kernels this many at a time whatever `batch_size` says (never fewer than it).
PAIRS_PER_LAUNCH = 1024


def EMD_CD(sample_pcs, ref_pcs, batch_size, accelerated_cd=True, reduced=True):
    """Paired CD / EMD of sample i vs reference i."""
    assert sample_pcs.shape[0] == ref_pcs.shape[0]
    cd, emd = [], []
    step = max(int(batch_size), PAIRS_PER_LAUNCH)
    for s in range(0, sample_pcs.shape[0], step):
        a, b = sample_pcs[s:s + step].contiguous(), ref_pcs[s:s + step].contiguous()
        dl, dr = distChamferCUDA(a, b)
        cd.append(dl.mean(1) + dr.mean(1))
        emd.append(emd_approx(a, b))
    cd, emd = torch.cat(cd), torch.cat(emd)
    return {"MMD-CD": cd.mean() if reduced else cd, "MMD-EMD": emd.mean() if reduced else emd}


def _pairwise_EMD_CD_(sample_pcs, ref_pcs, batch_size, accelerated_cd=True, verbose=False, mask_sample=None, mask_ref=None):
    """All-pairs (N_sample, N_ref) CD and EMD matrices; optional per-point masks weight the two Chamfer directions.
    (The reference walks sample by sample, `batch_size` references per call; here pair p = (p // N_ref, p % N_ref) of the flattened
    matrix goes out in launches of PAIRS_PER_LAUNCH — the same kernels on the same pairs, a full chip per launch.)"""
    Ns, Nr = sample_pcs.shape[0], ref_pcs.shape[0]
    step = max(int(batch_size), PAIRS_PER_LAUNCH)
    all_cd, all_emd = [], []
    for p0 in range(0, Ns * Nr, step):
        p = torch.arange(p0, min(Ns * Nr, p0 + step), device=sample_pcs.device)
        i, r = torch.div(p, Nr, rounding_mode="floor"), p % Nr
        smp, ref = sample_pcs[i].contiguous(), ref_pcs[r].contiguous()
        dl, dr = distChamferCUDA(smp, ref)
        dl_mean = dl.mean(1) if mask_sample is None else (dl * mask_sample[i]).sum(1) / mask_sample[i].sum(1)
        dr_mean = dr.mean(1) if mask_ref is None else (dr * mask_ref[r]).sum(1) / mask_ref[r].sum(1)
        all_cd.append(dl_mean + dr_mean)
        all_emd.append(emd_approx(smp, ref))
    return torch.cat(all_cd).view(Ns, Nr), torch.cat(all_emd).view(Ns, Nr)


def knn(Mxx, Mxy, Myy, k, sqrt=False, one_way=False):
    """Leave-one-out k-NN two-sample test (1-NNA for k = 1) on the block matrix [[Mxx, Mxy], [Mxy^T, Myy]]: a cloud is
    predicted to belong to set x when at least k/2 of its k nearest other clouds do.  Returns the reference's dict
    (tp, fp, fn, tn, precision, recall, acc_t, acc_f, acc) as 0-dim tensors."""
    nx, ny = Mxx.size(0), Myy.size(0)
    is_x = torch.cat((torch.ones(nx), torch.zeros(ny))).to(Mxx)
    D = torch.cat([torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.t(), Myy), 1)], 0)
    if sqrt:
        D = D.abs().sqrt()
    D = D + torch.diag(torch.full((nx + ny,), float("inf")).to(Mxx))           # exclude the cloud itself
    nearest = D.topk(k, dim=0, largest=False).indices                           # (k, nx + ny)
    votes = is_x[nearest].sum(0)
    pred = (votes >= k / 2.0).float()
    if one_way:
        pred = pred[:nx]
        is_x = pred[:nx]   # as in the reference (:229-231): the one-way variant scores the x block against itself
    tp, fp = (pred * is_x).sum(), (pred * (1 - is_x)).sum()
    fn, tn = ((1 - pred) * is_x).sum(), ((1 - pred) * (1 - is_x)).sum()
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "precision": tp / (tp + fp + 1e-10), "recall": tp / (tp + fn + 1e-10),
            "acc_t": tp / (tp + fn + 1e-10), "acc_f": tn / (tn + fp + 1e-10), "acc": (is_x == pred).float().mean()}


def lgan_mmd_cov(all_dist, thresh=1000):
    """all_dist (N_sample, N_ref).  The reference's variant (:251-278): lgan_mmd = mean over references of the distance to
    their closest sample; lgan_cov = number of distinct closest samples over the references (references whose closest
    sample is farther than ``thresh`` are folded onto the best-matched reference's sample) / N_ref; lgan_mmd_smp = mean
    over samples of the distance to their closest reference."""
    N_ref = all_dist.size(1)
    min_val_fromsmp, _ = torch.min(all_dist, dim=1)
    min_val, idx = torch.min(all_dist, dim=0)
    min_val, order = torch.sort(min_val)
    sorted_idx = idx[order]
    outlier = min_val > thresh
    if torch.any(outlier):
        sorted_idx[outlier] = sorted_idx[0]
    cov = torch.tensor(float(sorted_idx.unique().numel()) / float(N_ref)).to(all_dist)
    return {"lgan_mmd": min_val.mean(), "lgan_cov": cov, "lgan_mmd_smp": min_val_fromsmp.mean()}


def compute_all_metrics(sample_pcs, ref_pcs, batch_size, accelerated_cd=True, one_way=False, mask=None):
    """MMD / COV under CD and EMD + 1-NNA accuracies (evaluation_utils.py:500-560)."""
    results = {}
    M_rs_cd, M_rs_emd = _pairwise_EMD_CD_(ref_pcs, sample_pcs, batch_size, mask_ref=mask)
    results.update({f"{k}-CD": v for k, v in lgan_mmd_cov(M_rs_cd.t()).items()})
    results.update({f"{k}-EMD": v for k, v in lgan_mmd_cov(M_rs_emd.t()).items()})
    M_rr_cd, M_rr_emd = _pairwise_EMD_CD_(ref_pcs, ref_pcs, batch_size)
    if not one_way:
        M_ss_cd, M_ss_emd = _pairwise_EMD_CD_(sample_pcs, sample_pcs, batch_size, mask_ref=mask, mask_sample=mask)
    else:
        inf = float("inf")
        M_ss_cd = torch.full((sample_pcs.shape[0],) * 2, inf).to(M_rr_cd)
        M_ss_emd = torch.full((sample_pcs.shape[0],) * 2, inf).to(M_rr_cd)
    for name, (rr, rs, ss) in (("CD", (M_rr_cd, M_rs_cd, M_ss_cd)), ("EMD", (M_rr_emd, M_rs_emd, M_ss_emd))):
        res = knn(rr, rs, ss, 1, sqrt=False, one_way=one_way)
        results.update({f"1-NN-{name}-{k}": v for k, v in res.items() if "acc" in k})
    return results


# ---------------------------------------------------------------------------------------------------------------------
# Part-level metrics of the gen_part evaluation (ShapeNetSeg.evaluate, shapenet_seg.py:375-388): snapping, part boxes, per-part
# MMD / COV / 1-NNA.  The point work (part extraction, nearest-neighbour scans, order statistics, box-set distance matrices) runs in
# libdfx's part_metrics.hip; what remains here is the reference's bookkeeping on small tensors.
SNAPPING_TABLES = {"Chair": [(0, [1, 2]), (1, [2]), (3, [0, 1])], "Airplane": [(1, [0]), (2, [0]), (3, [0, 1])]}
BOX_METRIC_IDS = {"l2": 0, "iou": 1, "chamfer": 2}
PART_MIN_POINTS = 100   # parts with at most this many points get no box and no cloud (:313, :440)
PART_CLOUD_POINTS = 512
SNAPPING_K = 50


def _dev_cloud(x):
    x = torch.as_tensor(x)
    return (x if x.is_cuda else x.cuda()).float().contiguous()


def _dev_labels(m, device):
    return torch.as_tensor(m).to(device=device, dtype=torch.int32).contiguous()


def part_snapping(xyz, labels, pairs, k=SNAPPING_K):
    """Native snapping distances: xyz (B,N,3), labels (B,N), pairs [(a,b), ...] -> dist (B,P) fp32, status (B,P) int32 on the device
    (0 = a part is absent, 1 = computed, 2 = a part has fewer than k points; dfx_part_snapping_f32)."""
    xyz = _dev_cloud(xyz)
    lab = _dev_labels(labels, xyz.device)
    B, N, _ = xyz.shape
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    C = int(pr.max()) + 1 if pr.size else 1
    dist = torch.empty(B, len(pr), device=xyz.device)
    status = torch.empty(B, len(pr), dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _ffi.check(_ffi.lib().dfx_part_snapping_f32(_ffi.ptr(xyz), _ffi.ptr(lab), B, N, C, pr.ctypes.data_as(_ffi.c_fp), len(pr), int(k),
                                                    _ffi.ptr(dist), _ffi.ptr(status), _ffi.current_stream()), "dfx_part_snapping_f32")
    return dist, status


def compute_snapping_metric(preds, preds_mask, cls="Chair", connected=None):
    """Snapping metric (evaluation_utils.py:385-421): for every part i of the class table and every shape, the smallest snapping
    distance to the parts it connects to (pairs with an absent part skipped), averaged over the shapes that have one.  ``connected``
    ([(i, [j, ...]), ...]) replaces the Chair / Airplane tables; any other ``cls`` without it raises ValueError (the reference fails
    on an unbound local).  A present part with fewer than 50 points raises ValueError, as the reference's topk does, and so does a
    key without any shape."""
    if connected is None:
        if cls not in SNAPPING_TABLES:
            raise ValueError(f"compute_snapping_metric: no part table for class {cls!r} (Chair, Airplane; or pass connected=)")
        connected = SNAPPING_TABLES[cls]
    pairs = [(i, j) for i, js in connected for j in js]
    dist, status = part_snapping(preds, preds_mask, pairs)
    dist, status = dist.cpu(), status.cpu()
    bad = (status == 2).nonzero()
    if len(bad):
        s, p = (int(v) for v in bad[0])
        raise ValueError(f"compute_snapping_metric: shape {s}: part {pairs[p][0]} or {pairs[p][1]} has fewer than {SNAPPING_K} points")
    out, col = {}, 0
    for i, js in connected:
        d, st = dist[:, col:col + len(js)], status[:, col:col + len(js)]
        col += len(js)
        has = (st == 1).any(1)
        if not bool(has.any()):
            raise ValueError(f"compute_snapping_metric: no shape has part {i} together with any of parts {list(js)}")
        out[f"snapping_{cls}_{i}"] = torch.where(st == 1, d, torch.full_like(d, float("inf"))).min(1).values[has].mean()
    return out


def part_boxes(xyz, labels, n_class=4, thresh=1.0, normalize=True, min_points=PART_MIN_POINTS):
    """Native part boxes (the box step of compute_bbox_metric, :287-333): -> (boxes (B,n_class,2,3) = (lo, hi), count (B,n_class)) on
    the device; boxes of parts with count <= min_points are NaN."""
    xyz = _dev_cloud(xyz)
    lab = _dev_labels(labels, xyz.device)
    B, N, _ = xyz.shape
    boxes = torch.empty(B, n_class, 2, 3, device=xyz.device)
    count = torch.empty(B, n_class, dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _ffi.check(_ffi.lib().dfx_part_boxes_f32(_ffi.ptr(xyz), _ffi.ptr(lab), B, N, n_class, int(bool(normalize)), int(min_points),
                                                 float(thresh), _ffi.ptr(boxes), _ffi.ptr(count), _ffi.current_stream()),
                   "dfx_part_boxes_f32")
    return boxes, count


def part_clouds(xyz, labels, n_class=4, n_out=PART_CLOUD_POINTS, min_points=PART_MIN_POINTS):
    """Native part clouds (the extraction step of compute_part_metric, :423-486, with its per-part, per-axis normalisation):
    -> (clouds (B,n_class,n_out,3), masks (B,n_class,n_out), count (B,n_class)) on the device."""
    xyz = _dev_cloud(xyz)
    lab = _dev_labels(labels, xyz.device)
    B, N, _ = xyz.shape
    clouds = torch.empty(B, n_class, n_out, 3, device=xyz.device)
    masks = torch.empty(B, n_class, n_out, device=xyz.device)
    count = torch.empty(B, n_class, dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _ffi.check(_ffi.lib().dfx_part_clouds_f32(_ffi.ptr(xyz), _ffi.ptr(lab), B, N, n_class, int(min_points), int(n_out),
                                                  _ffi.ptr(clouds), _ffi.ptr(masks), _ffi.ptr(count), _ffi.current_stream()),
                   "dfx_part_clouds_f32")
    return clouds, masks, count


class BoxSet:
    """Part boxes of M shapes: boxes (M,C,2,3) fp32 (lo, hi), present (M,C) int32 on one device.  ``from_dicts`` takes the
    reference's form, a list of {class: (lo (1,3), hi (1,3))}."""

    def __init__(self, boxes, present):
        self.boxes = boxes.float().contiguous()
        self.present = present.to(torch.int32).contiguous()

    def __len__(self):
        return self.boxes.shape[0]

    @classmethod
    def from_counts(cls, boxes, count, min_points=PART_MIN_POINTS):
        return cls(boxes, count > min_points)

    @classmethod
    def from_dicts(cls, dicts, n_class, device="cuda"):
        boxes = torch.full((len(dicts), n_class, 2, 3), float("nan"))
        present = torch.zeros(len(dicts), n_class, dtype=torch.int32)
        for m, d in enumerate(dicts):
            for c, (lo, hi) in d.items():
                if 0 <= c < n_class:
                    boxes[m, c, 0], boxes[m, c, 1], present[m, c] = torch.as_tensor(lo).reshape(3), torch.as_tensor(hi).reshape(3), 1
        return cls(boxes.to(device), present.to(device))


def _matrix_seed(seed, which):
    return (int(seed) + which * 0x9E3779B97F4A7C15) % (1 << 64)


def box_pairwise(A, B, metric="chamfer", seed=None, row0=0, units=None):
    """D (len(A), len(B)) with D[i,j] = dist(A_i, B_j) on the device (dfx_part_box_pairwise_f32).  metric: 'l2' | 'iou' | 'chamfer'.
    chamfer draws: ``units`` (Ma*Mb, C, 2, 512, 3) replaces the Philox stream, else the stream keyed by ``seed`` (None: drawn from
    torch's generator) and the global pair index (row0 + i) * len(B) + j."""
    if metric not in BOX_METRIC_IDS:
        raise ValueError(f"unknown box metric {metric!r} (l2, iou, chamfer)")
    from .engine import resolve_seed
    seed = resolve_seed(seed)
    assert A.boxes.shape[1] == B.boxes.shape[1], "box sets with different class counts"
    D = torch.empty(len(A), len(B), device=A.boxes.device)
    if units is not None:
        units = units.to(A.boxes.device).float().contiguous()
        assert units.shape == (len(A) * len(B), A.boxes.shape[1], 2, 512, 3), units.shape
    with torch.cuda.device(A.boxes.device):
        _ffi.check(_ffi.lib().dfx_part_box_pairwise_f32(_ffi.ptr(A.boxes), _ffi.ptr(A.present), len(A), _ffi.ptr(B.boxes),
                                                        _ffi.ptr(B.present), len(B), A.boxes.shape[1], BOX_METRIC_IDS[metric],
                                                        seed % (1 << 64), int(row0), _ffi.ptr(units), _ffi.ptr(D),
                                                        _ffi.current_stream()), "dfx_part_box_pairwise_f32")
    return D


def _box_lohi(d, c):
    lo, hi = d[c]
    return torch.as_tensor(lo, dtype=torch.float32).reshape(3), torch.as_tensor(hi, dtype=torch.float32).reshape(3)


def _walk_classes(n_class, A, B, term):
    """The reference's class walk: presence differs -> inf (a (1,) tensor), both absent -> skipped, else term(...)."""
    dist = []
    for c in range(n_class):
        a, b = A.get(c, None), B.get(c, None)
        if (a is not None) != (b is not None):
            return torch.ones(1) * float("inf")
        if a is None:
            continue
        dist.append(term(_box_lohi(A, c), _box_lohi(B, c)))
    return dist


def part_chamfer(n_class, A, B, accelerated=False):
    """Box Chamfer of one pair (:23-40) on the host: 512 points uniform in each box from torch.rand, Chamfer-L2, mean over classes."""
    def term(a, b):
        pa = torch.rand([512, 3]) * (a[1] - a[0]) + a[0]
        pb = torch.rand([512, 3]) * (b[1] - b[0]) + b[0]
        d = ((pa[:, None] - pb[None]) ** 2).sum(-1)
        return d.min(1)[0].mean() + d.min(0)[0].mean()
    dist = _walk_classes(n_class, A, B, term)
    return dist if isinstance(dist, torch.Tensor) else torch.tensor(dist).mean()


def part_l2(n_class, A, B, accelerated=False):
    """Box L2 of one pair (:42-62): mean squared difference of [(hi-lo)/2, (hi+lo)/2], mean over classes."""
    def term(a, b):
        va = torch.cat([(a[1] - a[0]) / 2.0, (a[1] + a[0]) / 2.0])
        vb = torch.cat([(b[1] - b[0]) / 2.0, (b[1] + b[0]) / 2.0])
        return torch.nn.functional.mse_loss(va, vb)
    dist = _walk_classes(n_class, A, B, term)
    return dist if isinstance(dist, torch.Tensor) else torch.tensor(dist).mean()


def _iou_box(lo, hi):
    """The axis-aligned box the reference's get_3d_box(hi - lo, 0, (hi + lo) / 2) spans (iou.py:115-140): box_size is read as
    (l, w, h) with l along x, h along y and w along z, so the y-extent is dz and the z-extent dy.  float64 corners."""
    size = (hi - lo).numpy()
    ctr = ((hi + lo) / 2.0).numpy().astype(np.float64)
    half = np.array([size[0] / 2, size[2] / 2, size[1] / 2], np.float32).astype(np.float64)
    return ctr - half, ctr + half, float(np.float64(size[0]) * np.float64(size[1]) * np.float64(size[2]))


def part_miou(n_class, A, B, accelerated=True):
    """1 - mean 3-D IoU of one pair (:64-82, iou.py:82-140), float64 as in the reference (whose iou.py cannot run under numpy >= 2:
    ``from numpy import *`` shadows the built-in min / max)."""
    def term(a, b):
        la, ha, va = _iou_box(*a)
        lb, hb, vb = _iou_box(*b)
        inter = float(np.prod(np.maximum(0.0, np.minimum(ha, hb) - np.maximum(la, lb))))
        return inter / (va + vb - inter)
    dist = _walk_classes(n_class, A, B, term)
    return dist if isinstance(dist, torch.Tensor) else 1.0 - torch.tensor(dist, dtype=torch.float64).mean()


def lgan_mmd_cov_match(all_dist):
    """(:273-285) lgan_mmd / lgan_mmd_smp as lgan_mmd_cov; lgan_cov = distinct closest references over the samples / N_ref.
    Returns (dict, closest reference per sample)."""
    N_ref = all_dist.size(1)
    min_val_fromsmp, min_idx = torch.min(all_dist, dim=1)
    min_val, _ = torch.min(all_dist, dim=0)
    cov = torch.tensor(float(min_idx.unique().view(-1).size(0)) / float(N_ref)).to(all_dist)
    return {"lgan_mmd": min_val.mean(), "lgan_cov": cov, "lgan_mmd_smp": min_val_fromsmp.mean()}, min_idx.view(-1)


_BOX_FUNCS = {"part_chamfer": "chamfer", "part_l2": "l2", "part_miou": "iou"}


def _native_box_metric(dist_func):
    """(metric name, n_class) when dist_func is part_chamfer / part_l2 / part_miou with n_class bound by functools.partial."""
    if isinstance(dist_func, functools.partial) and dist_func.func in (part_chamfer, part_l2, part_miou) and len(dist_func.args) == 1 \
            and not dist_func.keywords:
        return _BOX_FUNCS[dist_func.func.__name__], int(dist_func.args[0])
    return None


def compute_all_metrics_cust_func(sample_pcs, ref_pcs, dist_func, dist_name, accelerated_cd=False, no_nn=False, thresh=1000, seed=None):
    """MMD / COV + 1-NNA under a custom pair distance (:336-383).  The reference hands ``lgan_mmd_cov`` a ``cov_thresh`` that is not
    defined in its scope (every call raises NameError); what it evidently means, and what this passes, is ``thresh``.
    Box sets (BoxSet, or lists of {class: (lo, hi)}) with ``functools.partial(part_chamfer | part_l2 | part_miou, n_class)`` go to the
    native distance matrices (chamfer: one seed per call, ``seed`` or drawn from torch's generator; rs / rr / ss each get a stream of
    their own); any other callable runs the reference's pair loop, dist_func(ref_pcs[i], sample_pcs[j], accelerated=...)."""
    results = {}
    native = _native_box_metric(dist_func)
    if native is not None:
        metric, n_class = native
        from .engine import resolve_seed
        seed = resolve_seed(seed)
        S = sample_pcs if isinstance(sample_pcs, BoxSet) else BoxSet.from_dicts(sample_pcs, n_class)
        R = ref_pcs if isinstance(ref_pcs, BoxSet) else BoxSet.from_dicts(ref_pcs, n_class)
        assert S.boxes.shape[1] == n_class and R.boxes.shape[1] == n_class
        # the matrices go to the host, where the reference builds them (torch.zeros): its topk then breaks ties among +inf the same way
        dist = lambda X, Y, which: box_pairwise(X, Y, metric, seed=_matrix_seed(seed, which)).cpu()  # noqa: E731
    else:
        S, R = sample_pcs, ref_pcs

        def dist(X, Y, which):
            out = torch.zeros([len(X), len(Y)])
            for i in range(len(X)):
                for j in range(len(Y)):
                    out[i, j] = dist_func(X[i], Y[j], accelerated=accelerated_cd)
            return out
    rs = dist(R, S, 0)
    results.update({f"{k}-{dist_name}": v for k, v in lgan_mmd_cov(rs.t(), thresh=thresh).items()})
    if no_nn:
        return results
    rr, ss = dist(R, R, 1), dist(S, S, 2)
    res = knn(rr, rs, ss, 1, sqrt=False)
    results.update({f"1-NN-{dist_name}-{k}": v for k, v in res.items() if "acc" in k})
    return results


def compute_bbox_metric(preds, preds_mask, refs, refs_mask, batch_size, n_class=4, thresh=1.0, metric="chamfer", no_nn=False,
                        cov_thresh=100, seed=None):
    """Box metrics (:287-333): per shape the whole-shape normalisation, per part with more than 100 points the box
    [quantile(1 - thresh), quantile(thresh)]; then compute_all_metrics_cust_func under part_chamfer / part_iou / part_l2 with
    ``thresh=cov_thresh``.  Keys carry the reference's double prefix, e.g. ``bbox_lgan_mmd-bbox_chamfer``."""
    if metric not in BOX_METRIC_IDS:
        raise ValueError(f"compute_bbox_metric: unknown metric {metric!r} (chamfer, iou, l2)")
    P = BoxSet.from_counts(*part_boxes(preds, preds_mask, n_class, thresh))
    R = BoxSet.from_counts(*part_boxes(refs, refs_mask, n_class, thresh))
    func = {"chamfer": part_chamfer, "iou": part_miou, "l2": part_l2}[metric]
    res = compute_all_metrics_cust_func(P, R, functools.partial(func, n_class), f"bbox_{metric}", accelerated_cd=True, no_nn=no_nn,
                                        thresh=cov_thresh, seed=seed)
    return {f"bbox_{k}": v for k, v in res.items()}


def _class_parts(clouds, masks, count, n_class, min_points=PART_MIN_POINTS):
    keep = (count > min_points).cpu()          # the one count copy
    out = []
    for j in range(n_class):
        idx = keep[:, j].nonzero().squeeze(1).to(clouds.device)
        out.append((clouds[:, j].index_select(0, idx), masks[:, j].index_select(0, idx)))
    return out


def compute_part_metric(preds, preds_mask, refs, refs_mask, batch_size, n_class=4):
    """Per-part MMD / COV / 1-NNA (:423-486): every part with more than 100 points becomes a 512-point cloud (repeated in index
    order, masked past its own points), normalised per axis; compute_all_metrics runs per class with the sample masks, and the
    results are averaged with weights = the class's share of all reference parts.  Keys ``part_weighted_{k}``.  Every class is
    normalised (the reference's loop is range(4), the same for n_class = 4).  A class without any kept part raises ValueError."""
    P = _class_parts(*part_clouds(preds, preds_mask, n_class), n_class)
    R = _class_parts(*part_clouds(refs, refs_mask, n_class), n_class)
    for j in range(n_class):
        if P[j][0].shape[0] == 0 or R[j][0].shape[0] == 0:
            raise ValueError(f"compute_part_metric: part {j} has no sample or no reference with more than {PART_MIN_POINTS} points")
    total = sum(r[0].shape[0] for r in R)
    weight = [r[0].shape[0] / total for r in R]
    metrics = [compute_all_metrics(P[j][0], R[j][0], 32, mask=P[j][1]) for j in range(n_class)]
    avg = {f"part_weighted_{k}": 0 for k in metrics[0]}
    for j, m in enumerate(metrics):
        for k, v in m.items():
            avg[f"part_weighted_{k}"] += v * weight[j]
    return avg


def _fps2048(x, m):
    from .pointnet2_ops import pointnet2_utils as pu
    x = _dev_cloud(x)
    idx = pu.furthest_point_sample(x, 2048)
    pts = pu.gather_operation(x.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    lab = torch.gather(_dev_labels(m, x.device), 1, idx.long())
    return pts, lab


def _normalize_shapes(x):
    """(x - (min+max)/2) / (largest extent / 2) per shape (shapenet_seg.py:338-347)."""
    mx, mn = x.max(1)[0].reshape(-1, 1, 3), x.min(1)[0].reshape(-1, 1, 3)
    shift = ((mn + mx) / 2).reshape(-1, 1, 3)
    scale = (mx - mn).max(-1)[0].reshape(-1, 1, 1) / 2
    return (x - shift) / scale


def gen_part_inputs(results):
    """(preds, preds_mask, refs, refs_mask) on the device from the model's forward dicts, as ShapeNetSeg.evaluate prepares them."""
    preds, preds_mask, refs, refs_mask = [], [], [], []
    for d in results:
        pred, pm, ref, rm = d["pred"], d["pred_seg_mask"], d["input_ref"], d["ref_seg_mask"]
        if pred.shape[1] > 2048:
            pred, pm = _fps2048(pred, pm)
        if ref.shape[1] > 2048:   # (:331-333 unpack a tuple of one; the FPS indices are meant)
            ref, rm = _fps2048(ref, rm)
        pred, ref = _dev_cloud(pred), _dev_cloud(ref)
        preds.append(_normalize_shapes(pred))
        refs.append(_normalize_shapes(ref))
        preds_mask.append(_dev_labels(pm, pred.device))
        refs_mask.append(_dev_labels(rm, ref.device))
    return torch.cat(preds), torch.cat(preds_mask), torch.cat(refs), torch.cat(refs_mask)


def evaluate_gen_part(results, class_choice, n_class=4, batch_size=32, seed=None):
    """The metric half of ShapeNetSeg.evaluate for eval_mode='gen_part' (shapenet_seg.py:300-388), without save_only and without
    saving: snapping on the samples and on the references ("oracle_"), box Chamfer, per-part metrics and the whole-shape
    MMD / COV / 1-NNA, merged in the reference's order."""
    preds, preds_mask, refs, refs_mask = gen_part_inputs(results)
    snapping = compute_snapping_metric(preds, preds_mask, cls=class_choice)
    oracle = compute_snapping_metric(refs, refs_mask, cls=class_choice)
    bbox = compute_bbox_metric(preds, preds_mask, refs, refs_mask, batch_size, n_class=n_class, metric="chamfer", seed=seed)
    part = compute_part_metric(preds, preds_mask, refs, refs_mask, batch_size, n_class=n_class)
    metrics = compute_all_metrics(preds, refs, batch_size)
    metrics.update(snapping)
    metrics.update({f"oracle_{k}": v for k, v in oracle.items()})
    metrics.update(part)
    metrics.update(bbox)
    return metrics


# ---------------------------------------------------------------------------------------------------------------------
# Occupancy-grid JSD (evaluation_utils.py:544-648, from latent_3d_points): every point goes to its nearest cell of a resolution^3
# grid in the unit cube, clipped to the sphere of radius 0.5; the JSD compares the two sets' per-cell point counts.  The point work
# (nearest kept cell, counters) and the reductions run in libdfx's occupancy.hip on integer counters: the same cells and counts as
# the reference's KD-tree, an exact tie going to the lower cell index.  Clouds are read as float32.
OCCUPANCY_MAX_RESOLUTION = 40
OCCUPANCY_MAX_CLASSES = 16


def occupancy_num_cells(resolution, in_sphere=True):
    """Kept cells of the grid (host only)."""
    n = _ffi.lib().dfx_occupancy_num_cells(int(resolution), int(bool(in_sphere)))
    if n < 0:
        _ffi.check(n, "dfx_occupancy_num_cells")
    return n


def occupancy_cell_mask(resolution, in_sphere=True):
    """The keep mask (R,R,R) bool, C order (host only)."""
    R = int(resolution)
    mask = np.zeros((R, R, R) if 2 <= R <= OCCUPANCY_MAX_RESOLUTION else (1,), np.uint8)
    _ffi.check(_ffi.lib().dfx_occupancy_cell_mask(R, int(bool(in_sphere)), mask.ctypes.data_as(_ffi.c_fp)), "dfx_occupancy_cell_mask")
    return mask.astype(bool)


def occupancy_grid(pclouds, labels=None, n_class=0, resolution=28, in_sphere=True, return_index=False, out=None):
    """Native occupancy counters of B clouds (B,N,3): -> (counters int64 (rows,cells), bernoulli int32 (rows,cells), cell_index int32
    (B,N) or None, n_bad int32 (1,)) on the device; rows = n_class + 1 with ``labels`` (B,N) (row 0 = every point, row 1 + c = the
    points labelled c), else 1.  ``out`` = (counters, bernoulli, n_bad) of an earlier call is added to (chunked sets).  Shapes, dtypes
    and devices are checked here, before a pointer reaches the library: ValueError."""
    x = _dev_cloud(pclouds)
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError(f"occupancy_grid: clouds of shape {tuple(x.shape)}, expected (B,N,3) with B, N > 0")
    B, N, _ = x.shape
    lab = None if labels is None else _dev_labels(labels, x.device)
    if lab is not None:
        if tuple(lab.shape) != (B, N):
            raise ValueError(f"occupancy_grid: labels of shape {tuple(lab.shape)}, expected {(B, N)}")
        if not 0 <= int(n_class) <= OCCUPANCY_MAX_CLASSES:
            raise ValueError(f"occupancy_grid: n_class = {n_class} outside [0,{OCCUPANCY_MAX_CLASSES}]")
    rows = 1 if lab is None else int(n_class) + 1
    cells = occupancy_num_cells(resolution, in_sphere)
    if out is None:
        counters = torch.empty(rows, max(cells, 1), dtype=torch.int64, device=x.device)
        bern = torch.empty(rows, max(cells, 1), dtype=torch.int32, device=x.device)
        n_bad = torch.empty(1, dtype=torch.int32, device=x.device)
    else:
        counters, bern, n_bad = out
        for name, t, shape, dtype in (("counters", counters, (rows, cells), torch.int64), ("bernoulli", bern, (rows, cells), torch.int32),
                                      ("n_bad", n_bad, (1,), torch.int32)):
            if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.device == x.device and t.is_contiguous()):
                raise ValueError(f"occupancy_grid: out's {name} must be a contiguous {dtype} tensor of shape {shape} on {x.device}, got "
                                 f"{(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__}")
    index = torch.empty(B, N, dtype=torch.int32, device=x.device) if return_index else None
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib().dfx_occupancy_grid_f32(_ffi.ptr(x), _ffi.ptr(lab), B, N, int(n_class), int(resolution), int(bool(in_sphere)),
                                                     int(out is not None), _ffi.ptr(counters), _ffi.ptr(bern), _ffi.ptr(index),
                                                     _ffi.ptr(n_bad), _ffi.current_stream()), "dfx_occupancy_grid_f32")
    return counters, bern, index, n_bad


def _require_finite(n_bad, what):
    n = int(n_bad.item())
    if n:
        raise ValueError(f"{what}: input contains {n} point(s) with NaN or infinity")


_COUNT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _device_jsd(P, Q):
    """P, Q: contiguous int64 vectors of one length on one device."""
    assert P.device == Q.device and P.dtype == Q.dtype == torch.int64 and P.shape == Q.shape and P.dim() == 1, (P.device, Q.device, P.shape, Q.shape)
    out = torch.empty(1, dtype=torch.float64, device=P.device)
    with torch.cuda.device(P.device):
        _ffi.check(_ffi.lib().dfx_occupancy_jsd_f64(_ffi.ptr(P), _ffi.ptr(Q), P.numel(), _ffi.ptr(out), _ffi.current_stream()),
                   "dfx_occupancy_jsd_f64")
    return out


def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """(grid, spacing) (:547-565): the cell centres of a resolution^3 grid in the unit cube, float32 (R,R,R,3); with clip_sphere the
    cells inside the sphere of radius 0.5, (cells,3) in C order."""
    R = int(resolution)
    spacing = 1.0 / float(R - 1)
    axis = (np.arange(R, dtype=np.float64) * spacing - 0.5).astype(np.float32)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1)
    if clip_sphere:
        grid = grid.reshape(-1, 3)[occupancy_cell_mask(R, True).reshape(-1)]
    return grid, spacing


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, verbose=False):
    """(entropy, counters) (:586-626): counters (cells,) float64 numpy = points per cell over all clouds; entropy = the mean over the
    cells of the entropy (nats) of "the cell is occupied in a cloud".  Non-finite input raises ValueError (sklearn's check)."""
    x = _dev_cloud(pclouds)
    if verbose:
        bound = 0.5 + 10e-4
        if float(x.max().abs()) > bound or float(x.min().abs()) > bound:
            warnings.warn("Point-clouds are not in unit cube.")
        if in_sphere and float(x.square().sum(2).sqrt().max()) > bound:
            warnings.warn("Point-clouds are not in unit sphere.")
    counters, bern, _, n_bad = occupancy_grid(x, resolution=grid_resolution, in_sphere=in_sphere)
    _require_finite(n_bad, "entropy_of_occupancy_grid")
    ent = torch.empty(1, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib().dfx_occupancy_entropy_f64(_ffi.ptr(bern), bern.shape[1], x.shape[0], _ffi.ptr(ent), _ffi.current_stream()),
                   "dfx_occupancy_entropy_f64")
    return np.float64(ent.item()), counters[0].cpu().numpy().astype(np.float64)


def jensen_shannon_divergence(P, Q):
    """JSD in bits of two count vectors (:629-648), np.float64.  Two integer tensors of which one is on a device go to the native
    fixed-order reduction there (the other one is moved to it); anything else, float weights included, is summed with numpy on the
    host."""
    if torch.is_tensor(P) and torch.is_tensor(Q) and (P.is_cuda or Q.is_cuda) and P.dtype in _COUNT_DTYPES and Q.dtype in _COUNT_DTYPES:
        device = P.device if P.is_cuda else Q.device
        P, Q = P.to(device=device, dtype=torch.int64), Q.to(device=device, dtype=torch.int64)
        if bool((P < 0).any()) or bool((Q < 0).any()):
            raise ValueError("Negative values.")
        if P.shape != Q.shape:
            raise ValueError("Non equal size.")
        return np.float64(_device_jsd(P.reshape(-1).contiguous(), Q.reshape(-1).contiguous()).item())
    P = np.asarray(P.cpu() if torch.is_tensor(P) else P, np.float64)
    Q = np.asarray(Q.cpu() if torch.is_tensor(Q) else Q, np.float64)
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError("Negative values.")
    if len(P) != len(Q):
        raise ValueError("Non equal size.")

    def bits(v):
        v = v[v > 0]
        return -np.sum(v * np.log(v)) / np.log(2.0)
    P_, Q_ = P / np.sum(P), Q / np.sum(Q)
    return np.float64(bits((P_ + Q_) / 2.0) - (bits(P_) + bits(Q_)) / 2.0)


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """JSD between two sets of clouds (S,N,3) inside the unit cube (:568-583): occupancy counters on the sphere-clipped grid."""
    cs, _, _, bad_s = occupancy_grid(sample_pcs, resolution=resolution, in_sphere=True)
    cr, _, _, bad_r = occupancy_grid(_dev_cloud(ref_pcs).to(cs.device), resolution=resolution, in_sphere=True)
    out = _device_jsd(cs[0], cr[0])
    _require_finite(bad_s + bad_r, "jsd_between_point_cloud_sets")
    return np.float64(out.item())


def part_jsd(preds, preds_mask, refs, refs_mask, n_class=4, resolution=28):
    """{"jsd": whole shapes, "part_c_jsd": the points labelled c} from one counting pass per set (labels outside [0,n_class) count in
    "jsd" only).  A part without points in either set gives NaN."""
    cp, _, _, bad_p = occupancy_grid(preds, preds_mask, n_class, resolution, True)
    cr, _, _, bad_r = occupancy_grid(_dev_cloud(refs).to(cp.device), refs_mask, n_class, resolution, True)
    vals = torch.cat([_device_jsd(cp[r], cr[r]) for r in range(n_class + 1)])
    empty = ((cp.sum(1) == 0) | (cr.sum(1) == 0)).cpu()
    _require_finite(bad_p + bad_r, "part_jsd")
    vals = vals.cpu().numpy()
    vals[empty.numpy()] = np.nan
    return {("jsd" if r == 0 else f"part_{r - 1}_jsd"): np.float64(vals[r]) for r in range(n_class + 1)}
