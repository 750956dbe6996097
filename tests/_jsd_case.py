"""Shared pieces of the occupancy-JSD tests (test_jsd_cpu.py, test_gpu_jsd.py): the recorded reference cases of tests/golden/jsd/
(make_golden_jsd.py) and a numpy float64 brute force over all kept cells with the lower-index tie rule."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JSD = os.path.join(ROOT, "tests", "golden", "jsd")
CASES = [(R, sphere) for R in (8, 28, 32) for sphere in (False, True)]


def case_name(R, sphere):
    return f"r{R}_{'sphere' if sphere else 'cube'}.npz"


def load_case(R, sphere):
    return np.load(os.path.join(JSD, case_name(R, sphere)))


def load_clouds():
    z = np.load(os.path.join(JSD, "clouds.npz"))
    return {"a": z["a"], "b": z["b"]}


def recorded_mask(z, R):
    return np.unpackbits(z["mask"])[:R ** 3].astype(bool).reshape(R, R, R)


def grid_axis(R):
    """float32(i * (1.0 / (R - 1)) - 0.5), product and difference in double."""
    return (np.arange(R, dtype=np.float64) * (1.0 / float(R - 1)) - 0.5).astype(np.float32)


def keep_mask(R, sphere):
    """The keep mask (R,R,R) from float32 arithmetic of this file's own: sqrt((x*x + y*y) + z*z) <= 0.5."""
    a = grid_axis(R)
    if not sphere:
        return np.ones((R, R, R), bool)
    sq = a * a
    s = (sq[:, None, None] + sq[None, :, None]) + sq[None, None, :]
    assert s.dtype == np.float32
    return np.sqrt(s) <= np.float32(0.5)


def brute_force(points, R, sphere, chunk=128):
    """Compact index of the nearest kept cell per point (n,3) float32: (dx*dx + dy*dy) + dz*dz in float64 over every kept cell,
    np.argmin's first minimum = the lower compact index on a tie.  -1 for a non-finite point."""
    a = grid_axis(R).astype(np.float64)
    ijk = np.argwhere(keep_mask(R, sphere))            # C order
    gx, gy, gz = a[ijk[:, 0]], a[ijk[:, 1]], a[ijk[:, 2]]
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.full(len(p), -1, np.int32)
    ok = np.isfinite(p).all(1)
    idx = np.flatnonzero(ok)
    for s in range(0, len(idx), chunk):
        q = p[idx[s:s + chunk]]
        dx, dy, dz = q[:, 0:1] - gx[None], q[:, 1:2] - gy[None], q[:, 2:3] - gz[None]
        out[idx[s:s + chunk]] = np.argmin((dx * dx + dy * dy) + dz * dz, axis=1)
    return out


def count(index, cells, labels=None, n_class=0):
    """(counters int64 (rows,cells), bernoulli int32 (rows,cells)) from per-point indices (B,N), as the kernel defines its rows."""
    B = index.shape[0]
    rows = 1 if labels is None else n_class + 1
    counters, bern = np.zeros((rows, cells), np.int64), np.zeros((rows, cells), np.int32)
    for b in range(B):
        for r in range(rows):
            sel = index[b] >= 0
            if r > 0:
                sel = sel & (labels[b] == r - 1)
            c = np.bincount(index[b][sel], minlength=cells)
            counters[r] += c
            bern[r] += (c > 0)
    return counters, bern


def mixed_points(rng, n):
    """Points in and around the unit cube: box [-1,1], ball 0.5, normal sigma 0.2, a few far away."""
    k = max(n // 3, 1)
    d = rng.standard_normal((k, 3))
    ball = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.5 * rng.uniform(0, 1, (k, 1)) ** (1 / 3))
    pts = np.concatenate([rng.uniform(-1, 1, (k, 3)), ball, 0.2 * rng.standard_normal((max(n - 2 * k, 0), 3))])[:n]
    pts = pts[rng.permutation(len(pts))]
    return np.ascontiguousarray(pts, np.float32)
