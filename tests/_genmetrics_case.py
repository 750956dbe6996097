"""Shared by test_gen_metrics_cpu.py and test_gpu_evaluation.py: the loader of tests/golden/genmetrics/ (make_golden_genmetrics.py) and a
plain numpy float64 restatement of the bookkeeping behind MMD / COV / 1-NNA, written from the definitions:

knn_vote        leave-one-out k-NN two-sample vote on the block matrix [[Mxx, Mxy], [Mxy^T, Myy]]
mmd_cov         MMD, COV (with the threshold fold) and MMD-smp of an (N_sample, N_ref) distance matrix
chamfer_matrix  all-pairs Chamfer-L2 with optional per-point masks weighting the two directions
emd_matrix      all-pairs EMD through the C oracle's auction (oracle/pointnet2.c), sqrt(dist) averaged in float64
cd_standin, emd_standin   the host stand-ins for the two device calls (distChamferCUDA, emd_approx) that the generator gives the
                reference and the CPU tests give the mirror

No function here breaks ties: callers keep the entries of a column apart."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GM = os.path.join(ROOT, "tests", "golden", "genmetrics")
F64 = np.float64

KNN_KEYS = ("tp", "fp", "fn", "tn", "precision", "recall", "acc_t", "acc_f", "acc")
KNN_COUNTS = ("tp", "fp", "fn", "tn", "acc")
MMDCOV_KEYS = ("lgan_mmd", "lgan_cov", "lgan_mmd_smp")
ALL_KEYS = tuple(f"{k}-{d}" for d in ("CD", "EMD") for k in MMDCOV_KEYS) + \
    tuple(f"1-NN-{d}-{k}" for d in ("CD", "EMD") for k in ("acc_t", "acc_f", "acc"))
MATRICES = ("rs_cd", "rs_emd", "rr_cd", "rr_emd", "ss_cd", "ss_emd")


def load(name):
    return np.load(os.path.join(GM, name), allow_pickle=False)


def result(z, prefix="res_"):
    """{key: float64} of the recorded result dict, in the recorded key order (``{prefix}keys``)."""
    return {str(k): F64(z[f"{prefix}{k}"]) for k in z[f"{prefix}keys"]}


def knn_cases():
    """(Mxx, Mxy, Myy, k, sqrt, one_way, {key: float32}) of knn.npz."""
    z = load("knn.npz")
    keys = [str(k) for k in z["res_keys"]]
    for c in range(int(z["n_cases"])):
        k, sqrt, one_way = (int(v) for v in z[f"c{c}_args"])
        yield z[f"c{c}_Mxx"], z[f"c{c}_Mxy"], z[f"c{c}_Myy"], k, bool(sqrt), bool(one_way), dict(zip(keys, z[f"c{c}_res"]))


def mmdcov_cases():
    """(D, thresh, {key: float32}) of mmdcov.npz."""
    z = load("mmdcov.npz")
    keys = [str(k) for k in z["res_keys"]]
    for c in range(int(z["n_cases"])):
        yield z[f"c{c}_D"], float(z[f"c{c}_thresh"]), dict(zip(keys, z[f"c{c}_res"]))


def knn_vote(Mxx, Mxy, Myy, k, sqrt=False, one_way=False):
    """Every cloud of x (nx) and y (ny) looks at its k nearest OTHER clouds of the union and is predicted "x" when at least half of
    them are x.  Distances: x_i-x_j = Mxx[i,j], x_i-y_j = Mxy[i,j] both ways, y_i-y_j = Myy[i,j]; with ``sqrt`` the root of their
    absolute value.  tp / fp / fn / tn count (predicted x?, is x?) over all clouds; ``one_way`` keeps the x clouds only and takes
    their prediction as their label (the reference's definition), so fp = fn = 0.  acc_t = tp / (tp + fn), acc_f = tn / (tn + fp),
    acc = share of clouds whose prediction equals their label."""
    Mxx, Mxy, Myy = (np.asarray(m, F64) for m in (Mxx, Mxy, Myy))
    nx, ny = Mxx.shape[0], Myy.shape[0]
    n = nx + ny

    def dist(a, b):   # from cloud a to cloud b as the column of cloud b reads it
        if a < nx and b < nx:
            d = Mxx[a, b]
        elif a >= nx and b >= nx:
            d = Myy[a - nx, b - nx]
        else:
            d = Mxy[a, b - nx] if a < nx else Mxy[b, a - nx]
        return np.sqrt(abs(d)) if sqrt else d
    pred = np.zeros(n, bool)
    for c in range(n):
        others = sorted((o for o in range(n) if o != c), key=lambda o: dist(o, c))[:k]
        pred[c] = 2 * sum(o < nx for o in others) >= k
    label = np.arange(n) < nx
    if one_way:
        pred = pred[:nx]
        label = pred.copy()
    tp, fp = int((pred & label).sum()), int((pred & ~label).sum())
    fn, tn = int((~pred & label).sum()), int((~pred & ~label).sum())
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "precision": tp / (tp + fp + 1e-10), "recall": tp / (tp + fn + 1e-10),
            "acc_t": tp / (tp + fn + 1e-10), "acc_f": tn / (tn + fp + 1e-10), "acc": float((pred == label).mean())}


def mmd_cov(D, thresh=1000):
    """D (N_sample, N_ref).  lgan_mmd: mean over the references of the distance to their closest sample.  lgan_cov: distinct closest
    samples over the references / N_ref, where a reference whose closest sample is farther than ``thresh`` counts the closest sample
    of the best-matched reference (the one with the smallest such distance) instead of its own.  lgan_mmd_smp: mean over the samples
    of the distance to their closest reference."""
    D = np.asarray(D, F64)
    n_ref = D.shape[1]
    to_ref = [min(D[:, r]) for r in range(n_ref)]
    who = [int(np.argmin(D[:, r])) for r in range(n_ref)]
    best = int(np.argmin(to_ref))
    matched = {who[r] if not to_ref[r] > thresh else who[best] for r in range(n_ref)}
    return {"lgan_mmd": float(np.mean(to_ref)), "lgan_cov": len(matched) / n_ref, "lgan_mmd_smp": float(np.mean([min(row) for row in D]))}


def chamfer_matrix(A, B, mask_a=None, mask_b=None):
    """(len(A), len(B)) float64: for the pair (i, j) the mean over A_i's points of the squared distance to the nearest point of B_j
    plus the mean over B_j's points of the squared distance to the nearest point of A_i, by direct differences; a mask (clouds, n)
    weights its side's points (weighted mean)."""
    A, B = np.asarray(A, F64), np.asarray(B, F64)
    out = np.zeros((len(A), len(B)), F64)
    for i, a in enumerate(A):
        wa = np.ones(len(a)) if mask_a is None else np.asarray(mask_a[i], F64)
        for j, b in enumerate(B):
            wb = np.ones(len(b)) if mask_b is None else np.asarray(mask_b[j], F64)
            d = ((a[:, None] - b[None]) ** 2).sum(-1)
            out[i, j] = (d.min(1) * wa).sum() / wa.sum() + (d.min(0) * wb).sum() / wb.sum()
    return out


def emd_matrix(A, B):
    """(len(A), len(B)) float64: the C oracle's auction (eps 0.002, 10000 iterations, A_i bidding for B_j's points) on float32 clouds,
    the mean of sqrt(matched squared distance) taken in float64."""
    from oracle import pointnet2 as o
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    out = np.zeros((len(A), len(B)), F64)
    for i, a in enumerate(A):
        dist, _ = o.emd_forward(np.repeat(a[None], len(B), 0), B, 0.002, 10000)
        out[i] = np.sqrt(dist.astype(F64)).mean(1)
    return out


def cd_standin(x, y):
    """Host stand-in for distChamferCUDA on torch tensors (B,n,3), (B,m,3): float64 direct differences, float32 on return."""
    import torch
    a, b = x.numpy().astype(F64), y.numpy().astype(F64)
    d = ((a[:, :, None] - b[:, None]) ** 2).sum(-1)
    return torch.from_numpy(d.min(2).astype(np.float32)), torch.from_numpy(d.min(1).astype(np.float32))


def emd_standin(sample, ref):
    """Host stand-in for emd_approx on torch tensors: the C oracle's auction, sqrt(dist).mean(1) in float32."""
    import torch
    from oracle import pointnet2 as o
    dist, _ = o.emd_forward(sample.numpy(), ref.numpy(), 0.002, 10000)
    return torch.from_numpy(np.sqrt(dist).mean(1))


def column_gap(D):
    """Smallest gap between the smallest and the second-smallest entry over the columns of D (inf for columns with one finite entry)."""
    D = np.asarray(D, F64)
    gap = np.inf
    for c in range(D.shape[1]):
        col = np.sort(D[:, c])
        if len(col) > 1 and np.isfinite(col[1]):
            gap = min(gap, col[1] - col[0])
    return float(gap)


def column_spacing(D):
    """Smallest difference between any two finite entries of one column of D."""
    D = np.asarray(D, F64)
    gap = np.inf
    for c in range(D.shape[1]):
        col = np.sort(D[np.isfinite(D[:, c]), c])
        if len(col) > 1:
            gap = min(gap, np.diff(col).min())
    return float(gap)


def block_matrix(Mxx, Mxy, Myy):
    """[[Mxx, Mxy], [Mxy^T, Myy]] with +inf on the diagonal, float64."""
    D = np.block([[np.asarray(Mxx, F64), np.asarray(Mxy, F64)], [np.asarray(Mxy, F64).T, np.asarray(Myy, F64)]])
    np.fill_diagonal(D, np.inf)
    return D


def all_metrics(rs_cd, rs_emd, rr_cd, rr_emd, ss_cd=None, ss_emd=None):
    """The twelve keys of compute_all_metrics from its matrices (rs = references x samples, rr, ss; ss = None: one way), in order."""
    out = {}
    for name, rs in (("CD", rs_cd), ("EMD", rs_emd)):
        out.update({f"{k}-{name}": v for k, v in mmd_cov(np.asarray(rs, F64).T).items()})
    for name, rr, rs, ss in (("CD", rr_cd, rs_cd, ss_cd), ("EMD", rr_emd, rs_emd, ss_emd)):
        one_way = ss is None
        if one_way:
            ss = np.full((np.shape(rs)[1],) * 2, np.inf)
        res = knn_vote(rr, rs, ss, 1, one_way=one_way)
        out.update({f"1-NN-{name}-{k}": res[k] for k in ("acc_t", "acc_f", "acc")})
    return out
