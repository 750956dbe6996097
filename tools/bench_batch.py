#!/usr/bin/env python
"""Time of the native batch assembly next to a numpy per-item loop.

    python tools/bench_batch.py [--with-stage1 | --stage1-ms MS]

GPU: HIP-event time of dfx_batch_draw + dfx_batch_build_f32 for B = 128 items of N = 2048 points over a synthetic resident set of
3000 clouds x 2700 points (labelled boxes), median of 5 after a warm-up.  CPU: wall time of the float32 numpy per-item loop
(tests/_batch_case.item_numpy, the work a Python loader does per item, without collation or the host-to-device copy) for the same
128 items on one core of the same machine.  --with-stage1: also time the stage-1 training step in this process with bench.py's
own stage1_iteration (its train_iteration.stage1 line) and report batch assembly / step; --stage1-ms takes that figure from
outside instead.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _batch_case as bc  # noqa: E402
from difffacto_amd import data  # noqa: E402


def synthetic_set(n_clouds, n_points, seed=0):
    rng = np.random.default_rng(seed)
    clouds = []
    for _ in range(n_clouds):
        counts = np.maximum((rng.dirichlet(np.full(4, 4.0)) * n_points).astype(np.int64), 1)
        counts[0] += n_points - counts.sum()
        clouds.append(bc.box_cloud(rng, 4, counts))
    return clouds


def gpu_ms(ds, index, sample_id, npoints, options, repeats=5):
    idx = torch.from_numpy(index).cuda()
    sid = torch.from_numpy(sample_id).cuda()
    times = []
    for r in range(repeats + 1):               # the first run is the warm-up
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = ds.batch(idx, sample_id=sid, seed=1, npoints=npoints, check=False, **options)
        stop.record()
        stop.synchronize()
        out["check"].raise_if_bad()
        if r:
            times.append(start.elapsed_time(stop))
    return float(np.median(times)), times


def numpy_ms(ds, clouds, index, sample_id, npoints, cfg):
    idx = torch.from_numpy(index).cuda()
    choice, drop_u, aug_u = (t.cpu().numpy() for t in ds.draw(idx, torch.from_numpy(sample_id).cuda(), 1, npoints))
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for r, s in enumerate(index):
        bc.item_numpy(clouds[s][0], clouds[s][1], choice[r], drop_u[r], aug_u[r], 4, cfg, dtype=np.float32)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=3000)
    ap.add_argument("--cloud-points", type=int, default=2700)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--stage1-ms", type=float, default=None)
    ap.add_argument("--with-stage1", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    clouds = synthetic_set(a.clouds, a.cloud_points)
    ds = data.PartCloudSet.from_arrays(clouds, 4)
    rng = np.random.default_rng(1)
    index = rng.permutation(a.clouds)[:a.batch].astype(np.int64)
    sample_id = np.arange(a.batch, dtype=np.int64)
    result = {"clouds": a.clouds, "cloud_points": a.cloud_points, "batch": a.batch, "npoints": a.npoints,
              "resident_mbytes": round((ds.points.numel() * 4 + ds.labels.numel() * 4) / 2 ** 20, 1)}
    for label, options in (("plain", dict()), ("dropout_augment", dict(dropout_part=0.2, augment=True))):
        med, times = gpu_ms(ds, index, sample_id, a.npoints, options)
        result[f"gpu_draw_build_ms.{label}"] = round(med, 4)
        result[f"gpu_runs_ms.{label}"] = [round(t, 4) for t in times]
    cfg = dict(bc.DEFAULT_CFG, dropout_part=0.2, augment_shift=True, augment_scale=True)
    result["numpy_f32_loop_ms_one_core"] = round(numpy_ms(ds, clouds, index, sample_id, a.npoints, cfg), 2)
    result["numpy_over_gpu"] = round(result["numpy_f32_loop_ms_one_core"] / result["gpu_draw_build_ms.dropout_augment"], 1)
    if a.with_stage1:
        import bench
        a.stage1_ms = bench.stage1_iteration(a.batch, a.npoints)["ms"]
    if a.stage1_ms:
        result["stage1_step_ms"] = round(a.stage1_ms, 3)
        result["batch_over_stage1_step"] = round(result["gpu_draw_build_ms.dropout_augment"] / a.stage1_ms, 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
