#!/usr/bin/env python
"""Golden vectors of the reference's part-level generation metrics (dev container only; the reference's own functions on CPU).

    python tests/golden/make_golden_partmetrics.py

Written to tests/golden/partmetrics/ with their own MANIFEST.sha256 (manifest.content_hash).  Inputs are seeded synthetic shapes:
per-part anisotropic blobs that touch their neighbours, labels shuffled over the point order, ten points labelled 5 (no part).

snapping.npz   compute_snapping_metric for Chair and Airplane on four shapes (one without part 1): one call per complete shape
               ("{cls}_shape{k}_{key}") and the means over all four ("{cls}_mean_{key}")
clouds.npz     compute_part_metric: the per-class clouds, masks and weights handed to compute_all_metrics (captured by a wrapper;
               Tensor.cuda made a no-op), parts of about 80, 150, 400 and 700 points
boxes.npz      the box dicts of compute_bbox_metric at thresh 1.0 and 0.95 (captured), with rs / rr / ss matrices of part_l2 and
               part_miou (recorded per pair by wrapping dist_func) and the final dicts
chamfer.npz    compute_bbox_metric with metric 'chamfer' at M = N = 2: torch.rand served from a recorded numpy stream, the unit draws
               stored per (matrix, pair, class, side), with the matrices and the final dict

Workarounds, each only around the call that needs it: the module global ``cov_thresh`` is set to the value compute_bbox_metric
passes as ``thresh`` (evaluation_utils.py:357 reads an undefined name); iou.py's ``min`` / ``max`` are restored to the built-ins
(``from numpy import *`` shadows them under numpy >= 2); ``distChamferCUDA`` is pointed at the pure-torch ``distChamfer`` and
Tensor.cuda is a no-op.
"""
import builtins
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "partmetrics")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)

import manifest  # noqa: E402
import ref_import  # noqa: E402

F32 = np.float32
N_CLASS = 4
CENTRES = np.array([[0.0, 0.0, 0.0], [0.0, 0.55, 0.0], [0.5, 0.0, 0.1], [0.0, -0.5, -0.1]], F32)
HALF = np.array([[0.35, 0.3, 0.25], [0.3, 0.28, 0.2], [0.25, 0.35, 0.3], [0.32, 0.22, 0.3]], F32)   # dy != dz everywhere


def make_shapes(rng, sizes):
    """sizes: per shape the point count of parts 0..3; every shape gets ten extra points labelled 5; same N for all shapes."""
    xyz, lab = [], []
    for sz in sizes:
        pts, ls = [], []
        for j, n in enumerate(sz):
            u = rng.uniform(-1, 1, (n, 3)).astype(F32)
            u /= np.maximum(1.0, np.linalg.norm(u, axis=1, keepdims=True)).astype(F32)
            pts.append(CENTRES[j] + u * HALF[j] * rng.uniform(0.85, 1.15, 3).astype(F32))
            ls.append(np.full(n, j, np.int64))
        pts.append(rng.uniform(-0.2, 0.2, (10, 3)).astype(F32))
        ls.append(np.full(10, 5, np.int64))
        p, l = np.concatenate(pts).astype(F32), np.concatenate(ls)
        perm = rng.permutation(len(p))
        xyz.append(p[perm])
        lab.append(l[perm])
    assert len({len(p) for p in xyz}) == 1
    return np.stack(xyz), np.stack(lab)


@contextlib.contextmanager
def patched(obj, name, value):
    had = hasattr(obj, name)
    old = getattr(obj, name, None)
    setattr(obj, name, value)
    try:
        yield
    finally:
        if had:
            setattr(obj, name, old)
        else:
            delattr(obj, name)


@contextlib.contextmanager
def box_workarounds(eu, cov_thresh):
    import difffacto.datasets.iou as iou
    with patched(eu, "cov_thresh", cov_thresh), patched(iou, "min", builtins.min), patched(iou, "max", builtins.max), \
            patched(eu, "distChamferCUDA", eu.distChamfer), patched(torch.Tensor, "cuda", lambda self, *a, **k: self), \
            contextlib.redirect_stdout(io.StringIO()):
        yield


def boxes_to_arrays(params):
    boxes = np.full((len(params), N_CLASS, 2, 3), np.nan, F32)
    present = np.zeros((len(params), N_CLASS), np.int32)
    for m, d in enumerate(params):
        for c, (lo, hi) in d.items():
            boxes[m, c, 0], boxes[m, c, 1], present[m, c] = lo.numpy().reshape(3), hi.numpy().reshape(3), 1
    return boxes, present


def run_bbox(eu, preds, pmask, refs, rmask, thresh, metric, cov_thresh=100):
    """compute_bbox_metric with the box dicts captured and every dist_func call recorded in call order."""
    cap, calls = {}, []
    orig = eu.compute_all_metrics_cust_func

    def cust(sample_pcs, ref_pcs, dist_func, dist_name, **kw):
        cap["sample"], cap["ref"] = sample_pcs, ref_pcs

        def rec(A, B, accelerated=False):
            v = dist_func(A, B, accelerated=accelerated)
            calls.append(float(v.reshape(-1)[0]))
            return v
        return orig(sample_pcs, ref_pcs, rec, dist_name, **kw)
    with box_workarounds(eu, cov_thresh), patched(eu, "compute_all_metrics_cust_func", cust):
        res = eu.compute_bbox_metric(torch.from_numpy(preds), torch.from_numpy(pmask), torch.from_numpy(refs), torch.from_numpy(rmask),
                                     32, n_class=N_CLASS, thresh=thresh, metric=metric, cov_thresh=cov_thresh)
    M, N = len(cap["sample"]), len(cap["ref"])
    c = np.asarray(calls, F32)
    rs, rr, ss = c[:N * M].reshape(N, M), c[N * M:N * M + N * N].reshape(N, N), c[N * M + N * N:].reshape(M, M)
    return cap, (rs, rr, ss), {k: float(v) for k, v in res.items()}


def main():
    ref_import.import_reference()
    import difffacto.datasets.evaluation_utils as eu
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261016)
    quiet = contextlib.redirect_stdout(io.StringIO())

    # ---- snapping ----
    xyz, lab = make_shapes(rng, [[700, 400, 150, 140], [400, 700, 80, 210], [150, 80, 400, 760], [700, 0, 400, 290]])
    out = {"xyz": xyz, "labels": lab.astype(np.int32)}
    for cls in ("Chair", "Airplane"):
        with quiet:
            for k in range(3):   # the fourth shape alone leaves a key without any value (the reference then fails)
                for key, v in eu.compute_snapping_metric(torch.from_numpy(xyz[k:k + 1]), torch.from_numpy(lab[k:k + 1]), cls=cls).items():
                    out[f"{cls}_shape{k}_{key}"] = np.asarray(v, F32)
            for key, v in eu.compute_snapping_metric(torch.from_numpy(xyz), torch.from_numpy(lab), cls=cls).items():
                out[f"{cls}_mean_{key}"] = np.asarray(v, F32)
    np.savez(os.path.join(OUT, "snapping.npz"), **out)

    # ---- part clouds ----
    preds, pmask = make_shapes(rng, [[700, 400, 150, 80], [400, 80, 700, 150], [150, 700, 80, 400]])
    refs, rmask = make_shapes(rng, [[80, 150, 400, 700], [700, 400, 150, 80], [400, 150, 700, 80]])
    cap = []

    def cam(pred, ref, bs, mask=None, **kw):
        cap.append((pred.numpy(), ref.numpy(), mask.numpy()))
        return {f"w{j}": torch.tensor(1.0 if j == len(cap) - 1 else 0.0) for j in range(N_CLASS)}
    with quiet, patched(torch.Tensor, "cuda", lambda self, *a, **k: self), patched(eu, "compute_all_metrics", cam):
        w = eu.compute_part_metric(torch.from_numpy(preds), torch.from_numpy(pmask), torch.from_numpy(refs), torch.from_numpy(rmask), 32,
                                   n_class=N_CLASS)
    out = {"preds": preds, "preds_mask": pmask.astype(np.int32), "refs": refs, "refs_mask": rmask.astype(np.int32),
           "weights": np.asarray([float(w[f"part_weighted_w{j}"]) for j in range(N_CLASS)], np.float64)}
    for j, (p, r, m) in enumerate(cap):
        out[f"pred_{j}"], out[f"ref_{j}"], out[f"mask_{j}"] = p, r, m
    np.savez(os.path.join(OUT, "clouds.npz"), **out)

    # ---- boxes, l2 / iou matrices ----
    preds, pmask = make_shapes(rng, [[700, 400, 150, 140], [400, 700, 90, 200], [500, 300, 300, 290], [600, 0, 500, 290]])
    refs, rmask = make_shapes(rng, [[650, 450, 150, 140], [300, 700, 200, 190], [520, 280, 330, 260]])
    out = {"preds": preds, "preds_mask": pmask.astype(np.int32), "refs": refs, "refs_mask": rmask.astype(np.int32)}
    for q in (1.0, 0.95):
        tag = "q100" if q == 1.0 else "q095"
        for metric in ("l2", "iou"):
            cap, (rs, rr, ss), res = run_bbox(eu, preds, pmask, refs, rmask, q, metric)
            out[f"{tag}_{metric}_rs"], out[f"{tag}_{metric}_rr"], out[f"{tag}_{metric}_ss"] = rs, rr, ss
            for k, v in res.items():
                out[f"{tag}_{metric}_res_{k}"] = np.asarray(v, np.float64)
        out[f"{tag}_pred_boxes"], out[f"{tag}_pred_present"] = boxes_to_arrays(cap["sample"])
        out[f"{tag}_ref_boxes"], out[f"{tag}_ref_present"] = boxes_to_arrays(cap["ref"])
    np.savez(os.path.join(OUT, "boxes.npz"), **out)

    # ---- box chamfer with recorded torch.rand ----
    preds, pmask = make_shapes(rng, [[500, 300, 300, 300], [600, 250, 350, 200]])
    refs, rmask = make_shapes(rng, [[450, 350, 300, 300], [700, 400, 300, 0]])
    draws = []
    rs_rng = np.random.default_rng(7)

    def rand(*size, **kw):
        u = (rs_rng.integers(0, 1 << 24, size=tuple(size[0]) if len(size) == 1 else size) * 2.0 ** -24).astype(F32)
        draws.append(u)
        return torch.from_numpy(u)
    order = []   # (matrix, i, j) per part_chamfer call, with its first draw
    orig_pc = eu.part_chamfer

    def pc(n_class, A, B, accelerated=False):
        order.append(len(draws))
        return orig_pc(n_class, A, B, accelerated)
    with patched(eu.torch, "rand", rand), patched(eu, "part_chamfer", pc):
        cap, (rs, rr, ss), res = run_bbox(eu, preds, pmask, refs, rmask, 1.0, "chamfer")
    out = {"preds": preds, "preds_mask": pmask.astype(np.int32), "refs": refs, "refs_mask": rmask.astype(np.int32),
           "rs": rs, "rr": rr, "ss": ss}
    out["pred_boxes"], out["pred_present"] = boxes_to_arrays(cap["sample"])
    out["ref_boxes"], out["ref_present"] = boxes_to_arrays(cap["ref"])
    for k, v in res.items():
        out[f"res_{k}"] = np.asarray(v, np.float64)
    M, N = len(preds), len(refs)
    shapes = {"rs": (N, M, out["ref_present"], out["pred_present"]), "rr": (N, N, out["ref_present"], out["ref_present"]),
              "ss": (M, M, out["pred_present"], out["pred_present"])}
    call = 0
    for name in ("rs", "rr", "ss"):
        R, S, pa, pb = shapes[name]
        units = np.zeros((R * S, N_CLASS, 2, 512, 3), F32)
        for i in range(R):
            for j in range(S):
                d = order[call]
                call += 1
                for c in range(N_CLASS):
                    if pa[i, c] != pb[j, c]:
                        break
                    if not pa[i, c]:
                        continue
                    units[i * S + j, c, 0], units[i * S + j, c, 1] = draws[d], draws[d + 1]
                    d += 2
        out[f"units_{name}"] = units
    np.savez_compressed(os.path.join(OUT, "chamfer.npz"), **out)

    path = os.path.join(OUT, "MANIFEST.sha256")
    with open(path, "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    for fn in sorted(os.listdir(OUT)):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
