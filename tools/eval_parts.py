#!/usr/bin/env python
"""gen_part metrics of two point-cloud sets: snapping (samples and "oracle_" references), box metric, per-part MMD / COV / 1-NNA
and whole-shape MMD / COV / 1-NNA, merged as ShapeNetSeg.evaluate does (evaluation.evaluate_gen_part).

    python tools/eval_parts.py SAMPLES REFS [--class Chair] [--n-class 4] [--thresh 1.0] [--cov-thresh 100]
                               [--metric chamfer|iou|l2] [--no-nn] [--seed S] [--jsd]

SAMPLES / REFS: a `bench.py --dump-outputs` folder (clouds.npy (M,N,3), seg_mask.npy (M,N)) or an .npz with `clouds` and `seg_mask`.
--thresh / --cov-thresh / --metric / --no-nn set the box metric as the offline tool's flags do.  --jsd adds the occupancy-grid JSD of the
whole shapes (`jsd`) and of every part (`part_k_jsd`), on the normalised clouds scaled by 0.5 into the unit cube."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difffacto_amd import evaluation as ev  # noqa: E402


def load(path):
    if os.path.isdir(path):
        return np.load(os.path.join(path, "clouds.npy")), np.load(os.path.join(path, "seg_mask.npy"))
    z = np.load(path)
    return z["clouds"], z["seg_mask"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("samples")
    ap.add_argument("refs")
    ap.add_argument("--class", dest="cls", default="Chair")
    ap.add_argument("--n-class", type=int, default=4)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--cov-thresh", type=float, default=100)
    ap.add_argument("--metric", default="chamfer", choices=sorted(ev.BOX_METRIC_IDS))
    ap.add_argument("--no-nn", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--jsd", action="store_true")
    a = ap.parse_args()
    (xs, ms), (xr, mr) = load(a.samples), load(a.refs)
    results = [dict(pred=torch.from_numpy(xs.astype(np.float32)), pred_seg_mask=torch.from_numpy(ms.astype(np.int64)),
                    input_ref=torch.from_numpy(xr.astype(np.float32)), ref_seg_mask=torch.from_numpy(mr.astype(np.int64)))]
    p, pm, r, rm = ev.gen_part_inputs(results)
    out = ev.compute_all_metrics(p, r, 32)
    out.update(ev.compute_snapping_metric(p, pm, cls=a.cls))
    out.update({f"oracle_{k}": v for k, v in ev.compute_snapping_metric(r, rm, cls=a.cls).items()})
    out.update(ev.compute_part_metric(p, pm, r, rm, 32, n_class=a.n_class))
    out.update(ev.compute_bbox_metric(p, pm, r, rm, 32, n_class=a.n_class, thresh=a.thresh, metric=a.metric, no_nn=a.no_nn,
                                      cov_thresh=a.cov_thresh, seed=a.seed))
    if a.jsd:
        out.update(ev.part_jsd(p * 0.5, pm, r * 0.5, rm, n_class=a.n_class))
    print(json.dumps({k: float(v) for k, v in out.items()}, indent=1))


if __name__ == "__main__":
    main()
