#!/usr/bin/env python
"""Times the part-metric kernels at the offline evaluation's sizes (2800 samples vs 700 references of 2048 points, Chair) and, in the
same process, the existing Chamfer kernel's pair-distance rate at 128 x 2048 x 2048 as the yardstick.

    python tools/bench_part_metrics.py [--samples 2800] [--refs 700] [--full]

Without --full the box Chamfer matrices are timed on a slice of rows (--rows) and scaled to the whole rs / rr / ss evaluation;
--full runs all of it.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difffacto_amd import evaluation as ev  # noqa: E402
from difffacto_amd.metrics import ChamferFunction  # noqa: E402


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def shapes(rng, M, N=2048):
    lab = np.sort(rng.integers(0, 4, (M, N)), 1).astype(np.int32)
    centre = np.asarray([[0, 0, 0], [0, .5, 0], [.5, 0, 0], [0, -.5, 0]], np.float32)[lab]
    x = (rng.standard_normal((M, N, 3)).astype(np.float32) * 0.15 + centre).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2800)
    ap.add_argument("--refs", type=int, default=700)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    xs, ls = shapes(rng, a.samples)
    xr, lr = shapes(rng, a.refs)
    out = {"samples": a.samples, "refs": a.refs, "points": 2048}
    # yardstick: the existing Chamfer kernel, 128 clouds of 2048 x 2048
    c1, c2 = shapes(rng, 128)[0], shapes(rng, 128)[0]
    t = timed(lambda: ChamferFunction.apply(c1, c2))
    out["chamfer_yardstick_pairdist_per_s"] = 2 * 128 * 2048 * 2048 / t
    pairs = [(i, j) for i, js in ev.SNAPPING_TABLES["Chair"] for j in js]
    out["snapping_s"] = timed(lambda: ev.part_snapping(xs, ls, pairs))
    out["boxes_q095_s"] = timed(lambda: ev.part_boxes(xs, ls, 4, 0.95))
    out["boxes_q100_s"] = timed(lambda: ev.part_boxes(xs, ls, 4, 1.0))
    out["clouds_s"] = timed(lambda: ev.part_clouds(xs, ls, 4))
    S = ev.BoxSet.from_counts(*ev.part_boxes(xs, ls, 4, 0.95))
    R = ev.BoxSet.from_counts(*ev.part_boxes(xr, lr, 4, 0.95))
    for m in ("l2", "iou"):
        out[f"box_{m}_rs_s"] = timed(lambda: ev.box_pairwise(R, S, m, seed=1))
    terms = lambda X, Y: float((X.present.float() @ Y.present.float().t()).sum())   # (pair, class) terms when all present match
    n_pairs_total = a.refs * a.samples + a.refs ** 2 + a.samples ** 2
    if a.full:
        t = timed(lambda: [ev.box_pairwise(X, Y, "chamfer", seed=1) for X, Y in ((R, S), (R, R), (S, S))], reps=1)
        work = terms(R, S) + terms(R, R) + terms(S, S)
    else:
        sub = ev.BoxSet(S.boxes[:a.rows], S.present[:a.rows])
        t1 = timed(lambda: ev.box_pairwise(sub, S, "chamfer", seed=1))
        work = terms(sub, S)
        t = t1 * n_pairs_total / (a.rows * a.samples)
        out["box_chamfer_slice_s"] = t1
        out["box_chamfer_rate_pairdist_per_s"] = work * 2 * 512 * 512 / t1
    if a.full:
        out["box_chamfer_rate_pairdist_per_s"] = work * 2 * 512 * 512 / t
    out["box_chamfer_all_matrices_s"] = t
    out["box_chamfer_vs_yardstick"] = out["box_chamfer_rate_pairdist_per_s"] / out["chamfer_yardstick_pairdist_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
