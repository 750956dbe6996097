"""Selective noise sampling (diverse generation): a float64 restatement of the selection over all rows of a call
(dfx_select_diverse_global: the intent of PartEncoder.subsample_params_global, part_encoders.py:591-621, and the rule the reference
executes), the ctypes wrapper of its host twin, the shapes and hand-made cases shared by test_selective_cpu.py and
test_gpu_selective.py, and the fixture loader of tests/golden/selective/.

Layouts are those of _part_sampling_case.py: candidate row g K + k, scores (G K,6,J), valid (G,J); picks are GLOBAL rows.  The
restatement takes a ``variant`` that makes it deliberately wrong (the gates' self-test): ``own_mask`` (a pair is compared on the
candidate's own parts, not on the common ones), ``no_div`` (no division by the number of common parts), ``tie_high`` (ties to the highest
index); the fourth wrong variant is the first-pick rule passed off as the farthest one."""
import ctypes
import os

import numpy as np

import _part_sampling_case as ps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selective")
F32, F64 = np.float32, np.float64
RULES = {"farthest": 0, "first_pick": 1}

# G, K, J, P: one row; two rows; one row per group; every row picked; odd everything; the shipped K; K above a workgroup of the
# per-group kernel; more rows than the 1024 threads of the global kernel
SHAPES = [(1, 1, 4, 1), (1, 2, 4, 2), (3, 1, 1, 3), (2, 64, 4, 128), (7, 37, 5, 40), (5, 100, 4, 50), (1, 257, 8, 9), (33, 100, 4, 330)]
SEEDS = (1, 2, 3)


def row_masks(valid, K):
    return np.repeat(np.asarray(valid, F64), K, axis=0)


def finite_rows(scores, masks):
    sc = np.asarray(scores, F64)
    on = masks != 0
    return on.any(1) & (np.isfinite(sc) | ~on[:, None, :]).all((1, 2))


def dist_to(sc, masks, s, variant=None):
    """Distance of every row to row s: over the parts valid in both, / their number; NaN where there is no common part."""
    w = masks if variant == "own_mask" else masks * masks[s]
    n = w.sum(1)
    with np.errstate(all="ignore"):
        d = (np.where(w[:, None, :] != 0, (sc - sc[s]) ** 2, 0.0) * w[:, None, :]).sum((1, 2))
        return np.where(n > 0, d if variant == "no_div" else d / np.where(n > 0, n, 1.0), np.nan)


def diverse_global_f64(scores, valid, K, P, rule, variant=None):
    """-> idx (P,) int32 global rows, dist (P,) the winner's smallest distance to the earlier picks (0 for pick 0 and non-finite picks,
    inf for a pick without a common part with any earlier one), gap (P,) = (best - runner-up) / best of every step (inf for the first
    step, a step without a runner-up, a non-finite pick or an infinite best)."""
    sc = np.asarray(scores, F64)
    masks = row_masks(valid, K)
    R = sc.shape[0]
    ok = finite_rows(sc, masks)
    good = np.flatnonzero(ok)
    idx, dist, gap = [], [], []
    free = ok.copy()
    mind = np.full(R, np.inf)
    if len(good):
        idx.append(int(good[0])), dist.append(0.0), gap.append(np.inf)
        free[good[0]] = False
    while len(idx) < min(P, len(good)):
        if rule == "farthest" or len(idx) == 1:
            d = dist_to(sc, masks, idx[-1], variant)
            mind = np.where(np.isnan(d), mind, np.minimum(mind, d))
        cand = np.flatnonzero(free)
        vals = mind[cand]
        best = vals.max()
        tied = cand[vals == best]
        pick = int(tied[-1] if variant == "tie_high" else tied[0])
        rest = vals[cand != pick]
        gap.append((best - rest.max()) / best if len(rest) and np.isfinite(best) and best > 0 else np.inf)
        idx.append(pick), dist.append(best)
        free[pick] = False
    for i in np.flatnonzero(~ok)[:P - len(idx)]:
        idx.append(int(i)), dist.append(0.0), gap.append(np.inf)
    return np.array(idx, np.int32), np.array(dist), np.array(gap)


def host_diverse_global(L, scores, valid, K, P, rule):
    scores, valid = ps._c(scores), ps._c(valid)
    G, J = valid.shape
    idx, dist, n_bad = np.zeros(P, np.int32), np.zeros(P, F64), np.zeros(1, np.int32)
    rc = L.dfx_debug_select_diverse_global_host(ps._p(scores), ps._p(valid), G, K, J, P, RULES[rule], ps._p(idx), ps._p(dist), ps._p(n_bad))
    assert rc == 0, L.dfx_last_error()
    return idx, dist, int(n_bad[0])


def same_dist(a, b, rtol=1e-12):
    """Pick distances agree: the same infinities, the finite ones to rtol."""
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(a)
    return np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin]) and np.allclose(a[fin], b[fin], rtol=rtol, atol=0)


# ---------------------------------------------------------------------------------------------------- hand-made cases
def twins_case():
    """12 rows in 2 groups; rows 3 and 9 are identical and far from every other row."""
    rng = np.random.Generator(np.random.PCG64(78))
    sc = (0.1 * rng.standard_normal((12, 6, 4))).astype(F32)
    sc[3] = sc[9] = 5.0
    return sc, np.ones((2, 4), F32), 6


def disjoint_case():
    """3 groups of 4 rows with masks {0,1}, {2,3}, {0,1}: the first row of the middle group shares no part with pick 0."""
    rng = np.random.Generator(np.random.PCG64(79))
    sc = rng.standard_normal((12, 6, 4)).astype(F32)
    return sc, np.array([[1, 1, 0, 0], [0, 0, 1, 1], [1, 1, 0, 0]], F32), 4


def bad_rows_case():
    """3 groups of 4 rows; row 2 has a NaN on a valid part, row 1 a NaN on an absent part only (finite as far as it is read), and the
    last group has no valid part at all: its 4 rows and row 2 are not finite."""
    rng = np.random.Generator(np.random.PCG64(80))
    sc = rng.standard_normal((12, 6, 4)).astype(F32)
    valid = np.array([[1, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]], F32)
    sc[2, 4, 2] = np.nan
    sc[1, 0, 1] = np.nan
    return sc, valid, 4


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))
