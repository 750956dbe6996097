#!/usr/bin/env python
"""Times the native occupancy-grid JSD (evaluation.jsd_between_point_cloud_sets) at the evaluation's size, and the same quantity through
scikit-learn's KD-tree on the host cores of the same box.

    python tools/bench_jsd.py [--samples 2800] [--refs 700] [--points 2048] [--resolution 28] [--reps 5] [--host-jobs 1] [--no-host]

Two seeded inputs: "box" = clouds uniform in a random box, normalised to [-1, 1] as the evaluation does and scaled by 0.5 (the corners
lie outside the sphere: those points take the kernel's column walk); "ball" = clouds uniform in the ball of radius 0.5 (every point
takes the eight-cell path).  Native: HIP-event time of the two counting launches plus the reduction (median and minimum over --reps
after a warm-up), and the wall time of the whole call with the clouds on the device.  Host: NearestNeighbors(n_neighbors=1) on the
sphere-clipped grid, one kneighbors query per cloud, np.bincount, the numpy JSD; --host-jobs is sklearn's n_jobs.  One JSON line per
input."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difffacto_amd import evaluation as ev  # noqa: E402


def make_clouds(kind, n, points, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "box":
        x = (torch.rand(n, points, 3, generator=g) * 2 - 1) * (0.6 + 0.4 * torch.rand(n, 1, 3, generator=g))
        return ev._normalize_shapes(x) * 0.5
    d = torch.randn(n, points, 3, generator=g)
    return d / d.norm(dim=2, keepdim=True) * (0.5 * torch.rand(n, points, 1, generator=g) ** (1 / 3))


def native(s, r, R, reps):
    cells = ev.occupancy_num_cells(R, True)
    ms, wall = [], []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        cs = ev.occupancy_grid(s, resolution=R)[0]
        cr = ev.occupancy_grid(r, resolution=R)[0]
        out = ev._device_jsd(cs[0], cr[0])
        b.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val = ev.jsd_between_point_cloud_sets(s, r, R)
        t1 = time.perf_counter()
        assert val == float(out) and cs.shape[1] == cells
        if rep:   # the first round loads the code object and uploads the grid's table
            ms.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return val, ms, wall


def host(s, r, R, jobs):
    from sklearn.neighbors import NearestNeighbors
    grid, _ = ev.unit_cube_grid_point_cloud(R, True)
    t0 = time.perf_counter()
    nn = NearestNeighbors(n_neighbors=1, n_jobs=jobs).fit(grid)
    counters = []
    for pcs in (s, r):
        c = np.zeros(len(grid), np.int64)
        for pc in pcs:
            c += np.bincount(nn.kneighbors(pc, return_distance=False)[:, 0], minlength=len(grid))
        counters.append(c)
    val = ev.jensen_shannon_divergence(*counters)
    return val, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2800)
    ap.add_argument("--refs", type=int, default=700)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-jobs", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_jsd.py needs a GPU: there is no CPU path to time")
    for kind in ("box", "ball"):
        s, r = make_clouds(kind, a.samples, a.points, 1), make_clouds(kind, a.refs, a.points, 2)
        outside = float(((torch.cat([s, r]).norm(dim=2)) > 0.5).float().mean())
        sd, rd = s.cuda(), r.cuda()
        val, ms, wall = native(sd, rd, a.resolution, a.reps)
        res = {"input": kind, "samples": a.samples, "refs": a.refs, "points": a.points, "resolution": a.resolution,
               "share_of_points_outside_sphere": round(outside, 4), "jsd": float(val),
               "native_event_ms_median": float(np.median(ms)), "native_event_ms_min": float(np.min(ms)),
               "native_call_wall_ms_median": float(np.median(wall))}
        if not a.no_host:
            hv, hms = host(s.numpy(), r.numpy(), a.resolution, a.host_jobs)
            res.update({"host_sklearn_ms": hms, "host_jobs": a.host_jobs, "host_cpus_available": len(os.sched_getaffinity(0)),
                        "host_jsd": float(hv), "jsd_abs_diff": abs(float(hv) - float(val))})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
