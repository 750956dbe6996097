#!/usr/bin/env python
"""Golden vectors of the reference's occupancy-grid JSD (dev container only; the reference's own functions on CPU, with
scikit-learn 1.7.2 and scipy 1.15.3).

    python tests/golden/make_golden_jsd.py

Written to tests/golden/jsd/ with their own MANIFEST.sha256 (manifest.content_hash).

clouds.npz         two float32 sets, a (6,256,3) and b (5,256,3): per cloud one third of the points uniform in the box [-1,1], one
                   third uniform in the ball of radius 0.5, one third normal with sigma 0.2, shuffled
r{R}_{cube|sphere}.npz   for R in 8, 28, 32 and in_sphere False / True: mask (the keep mask of unit_cube_grid_point_cloud as packed bits
                   over (R,R,R) in C order), cells, index_a / index_b (kneighbors of the grid's NearestNeighbors per point, int32),
                   counters_a / counters_b and entropy_a / entropy_b (entropy_of_occupancy_grid), bernoulli_a / bernoulli_b (recounted
                   from the indices as the reference counts them), jsd_ab (jensen_shannon_divergence of the two counters), jsd_aa (a
                   against itself), the type names of the returned values

The generator asserts that every fixture point's first and second neighbour distances differ by more than 1e-8: no fixture point
sits on a tie, which the reference leaves open.
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "jsd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)

import manifest  # noqa: E402
import ref_import  # noqa: E402

F32 = np.float32
SEED = 20261018
MIN_GAP = 1e-8


def make_set(rng, n_clouds, n_points):
    third = n_points // 3
    out = []
    for _ in range(n_clouds):
        box = rng.uniform(-1, 1, (third, 3))
        d = rng.standard_normal((third, 3))
        ball = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.5 * rng.uniform(0, 1, (third, 1)) ** (1 / 3))
        normal = 0.2 * rng.standard_normal((n_points - 2 * third, 3))
        pts = np.concatenate([box, ball, normal]).astype(F32)
        out.append(pts[rng.permutation(n_points)])
    return np.stack(out)


def main():
    ref_import.import_reference()
    import difffacto.datasets.evaluation_utils as eu
    from sklearn.neighbors import NearestNeighbors
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(SEED)
    sets = {"a": make_set(rng, 6, 256), "b": make_set(rng, 5, 256)}
    np.savez(os.path.join(OUT, "clouds.npz"), **sets)
    quiet = contextlib.redirect_stderr(io.StringIO())   # tqdm
    smallest = np.inf
    for R in (8, 28, 32):
        for sphere in (False, True):
            grid, _ = eu.unit_cube_grid_point_cloud(R, sphere)
            full, _ = eu.unit_cube_grid_point_cloud(R, False)
            grid = grid.reshape(-1, 3)
            kept_rows = {row.tobytes() for row in grid}                 # the cell centres are distinct
            keep = np.array([row.tobytes() in kept_rows for row in full.reshape(-1, 3)])
            assert keep.sum() == len(grid) and np.array_equal(full.reshape(-1, 3)[keep], grid)
            out = {"mask": np.packbits(keep), "cells": np.asarray(len(grid), np.int64)}
            nn = NearestNeighbors(n_neighbors=2).fit(grid)
            nn1 = NearestNeighbors(n_neighbors=1).fit(grid)
            for name, pcs in sets.items():
                idx = []
                bern = np.zeros(len(grid), np.int32)
                for pc in pcs:
                    dist, two = nn.kneighbors(pc)
                    _, one = nn1.kneighbors(pc)                       # the reference's own query
                    one = np.squeeze(one)
                    assert np.array_equal(one, two[:, 0])
                    gap = float((dist[:, 1] - dist[:, 0]).min())
                    smallest = min(smallest, gap)
                    assert gap > MIN_GAP, f"R={R} sphere={sphere} set {name}: neighbour gap {gap:g}: change SEED"
                    idx.append(one.astype(np.int32))
                    bern[np.unique(one)] += 1
                with quiet, warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ent, counters = eu.entropy_of_occupancy_grid(pcs, R, sphere)
                idx = np.stack(idx)
                assert np.array_equal(np.bincount(idx.reshape(-1), minlength=len(grid)), counters)
                out[f"index_{name}"], out[f"counters_{name}"], out[f"bernoulli_{name}"] = idx, counters, bern
                out[f"entropy_{name}"] = np.asarray(ent, np.float64)
                out[f"type_entropy_{name}"] = np.asarray(type(ent).__name__)
                out[f"type_counters_{name}"] = np.asarray(f"{type(counters).__name__}:{counters.dtype}")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                jab = eu.jensen_shannon_divergence(out["counters_a"], out["counters_b"])
                jaa = eu.jensen_shannon_divergence(out["counters_a"], out["counters_a"])
                if sphere:
                    with quiet:
                        assert eu.jsd_between_point_cloud_sets(sets["a"], sets["b"], R) == jab
            assert jaa == 0.0
            out["jsd_ab"], out["jsd_aa"], out["type_jsd"] = np.asarray(jab, np.float64), np.asarray(jaa, np.float64), np.asarray(type(jab).__name__)
            np.savez_compressed(os.path.join(OUT, f"r{R}_{'sphere' if sphere else 'cube'}.npz"), **out)
    print(f"smallest first/second neighbour gap over all fixture points: {smallest:.3g}")

    with open(os.path.join(OUT, "MANIFEST.sha256"), "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    for fn in sorted(os.listdir(OUT)):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
