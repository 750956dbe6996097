"""Part-level sampling: float64 restatements of the candidate scores and selections (PartEncoder.subsample_params,
part_encoders.py:545-589; the fit arg-min of sample_with_fixed_latents :678-682), ctypes wrappers of the host twins
(dfx_debug_part_scores_host / _select_diverse_host / _select_fit_host), input makers and fixture loaders shared by
test_part_sampling_cpu.py and test_gpu_part_sampling.py.

Layouts: candidate row g K + k; mean, logvar (G K,3,J); valid (G,J); stats (G K,4,3,J) = mean, unbiased std, min, max of the row's unit
draws; scores (G K,6,J).  The restatements take a ``variant`` that makes them deliberately wrong (the gates' self-test):
``box_all`` (box over absent parts too), ``no_div`` (distance without / sum(valid)), ``part_kept`` (fit weight = valid, the resampled
part not zeroed), ``tie_high`` (ties to the highest index); ``stats_of(biased=True)`` is the biased-std variant."""
import ctypes
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partsample")
F32, F64 = np.float32, np.float64
VP = ctypes.c_void_p


def _p(a):
    return None if a is None else a.ctypes.data_as(VP)


def _c(a, dt=F32):
    return np.ascontiguousarray(np.asarray(a), dtype=dt)


# ---------------------------------------------------------------------------------------------------- float64 restatements
def stats_of(u, biased=False):
    """u (R,n,3,J) normals -> (R,4,3,J) float64: mean, std (unbiased unless ``biased``), min, max over the n draws."""
    u = np.asarray(u, F64)
    return np.stack([u.mean(1), u.std(1, ddof=0 if biased else 1), u.min(1), u.max(1)], axis=1)


def scores_f64(mean, logvar, valid, stats, K, variant=None):
    """The closed form of :555-560 in float64: (G K,6,J)."""
    mean, logvar, stats = np.asarray(mean, F64), np.asarray(logvar, F64), np.asarray(stats, F64)
    v = np.repeat(np.asarray(valid) != 0, K, axis=0)[:, None, :]                     # (R,1,J)
    if variant == "box_all":
        v = np.ones_like(v)
    sg = np.exp(0.5 * logvar)
    ubar, ustd, umin, umax = stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3]
    with np.errstate(all="ignore"):
        hi = np.where(v, mean + sg * umax, -np.inf).max(2)                           # (R,3)
        lo = np.where(v, mean + sg * umin, np.inf).min(2)
        shift = (hi + lo) / 2
        scale = (hi - lo).max(1) / 2                                                 # (R,)
        return np.concatenate([(mean + sg * ubar - shift[:, :, None]) / scale[:, None, None],
                               2.0 * np.log(sg * ustd / scale[:, None, None])], axis=1)


def pair_dist(a, b, valid, variant=None):
    """Distance of score rows a (..,6,J), b (..,6,J) under the (J,) mask: sum over valid of (a - b)^2 / sum(valid), float64."""
    m = np.asarray(valid, F64)
    d = ((np.asarray(a, F64) - np.asarray(b, F64)) ** 2)[..., m != 0].sum((-1, -2))
    return d if variant == "no_div" else d / m.sum()


def diverse_f64(scores, valid, K, P, variant=None):
    """Greedy farthest-candidate selection (:562-585) on fp32 or fp64 scores, float64 distances.  -> idx (G,P) int32, dist (G,P) the
    pick's distance to the earlier picks (0 for the first), gap (G,P): (best - runner-up) / best of every step (inf for a step without
    a runner-up or the first).  Non-finite candidates (on a valid part) are picked last, lowest index first."""
    scores, valid = np.asarray(scores, F64), np.asarray(valid)
    G, J = valid.shape
    sc = scores.reshape(G, K, 6, J)
    idx, dist, gap = np.zeros((G, P), np.int32), np.zeros((G, P)), np.full((G, P), np.inf)
    for g in range(G):
        ok = np.isfinite(sc[g][:, :, valid[g] != 0]).all((1, 2))
        good = [i for i in range(K) if ok[i]]
        sel = [good[0]] if good else []
        mind = np.full(K, np.inf)
        while len(sel) < min(P, len(good)):
            mind = np.minimum(mind, pair_dist(sc[g], sc[g, sel[-1]], valid[g], variant))
            free = np.array([i for i in good if i not in sel])
            vals = mind[free]
            best = vals.max()
            tied = free[vals == best]
            pick = int(tied[-1] if variant == "tie_high" else tied[0])
            rest = np.sort(vals[free != pick])
            if len(rest) and best > 0:
                gap[g, len(sel)] = (best - rest[-1]) / best
            dist[g, len(sel)] = best
            sel.append(pick)
        sel += [i for i in range(K) if not ok[i]][:P - len(sel)]
        idx[g] = sel
    return idx, dist, gap


def fit_f64(mean, logvar, tm, tl, weight, K, variant=None):
    """:678-682 in float64: -> idx (G,) int32, fit (G,K), gap (G,) = (runner-up - best) / best (inf when best is 0 or K is 1)."""
    w = np.asarray(weight, F64)
    G, J = w.shape
    m, l = np.asarray(mean, F64).reshape(G, K, 3, J), np.asarray(logvar, F64).reshape(G, K, 3, J)
    with np.errstate(all="ignore"):
        inner = ((m - np.asarray(tm, F64)[:, None]) ** 2).sum(2) + ((l - np.asarray(tl, F64)[:, None]) ** 2).sum(2)     # (G,K,J)
        fit = np.where(w[:, None, :] != 0, w[:, None, :] * inner, 0.0).sum(2)
    idx, gap = np.zeros(G, np.int32), np.full(G, np.inf)
    for g in range(G):
        f = np.where(np.isfinite(fit[g]), fit[g], np.inf)
        best = f.min()
        tied = np.nonzero(f == best)[0]
        idx[g] = tied[-1] if variant == "tie_high" else tied[0]
        rest = np.sort(np.delete(f, idx[g]))
        if len(rest) and best > 0 and np.isfinite(best):
            gap[g] = (rest[0] - best) / best
    return idx, fit, gap


def fit_weight(valid, part, variant=None):
    """w = valid with the resampled part zeroed (:679-680)."""
    w = np.array(valid, F32, copy=True)
    if variant != "part_kept":
        w[:, part] = 0
    return w


def ulp32(x):
    """One float32 ulp at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


# ---------------------------------------------------------------------------------------------------- host twins
def host_scores(L, mean, logvar, valid, stats, K):
    mean, logvar, valid, stats = _c(mean), _c(logvar), _c(valid), _c(stats)
    G, J = valid.shape
    out = np.zeros((G * K, 6, J), F32)
    rc = L.dfx_debug_part_scores_host(_p(mean), _p(logvar), _p(valid), _p(stats), G, K, J, _p(out))
    assert rc == 0, L.dfx_last_error()
    return out


def host_diverse(L, scores, valid, K, P):
    scores, valid = _c(scores), _c(valid)
    G, J = valid.shape
    idx, dist, n_bad = np.zeros((G, P), np.int32), np.zeros((G, P), F64), np.zeros(1, np.int32)
    rc = L.dfx_debug_select_diverse_host(_p(scores), _p(valid), G, K, J, P, _p(idx), _p(dist), _p(n_bad))
    assert rc == 0, L.dfx_last_error()
    return idx, dist, int(n_bad[0])


def host_fit(L, mean, logvar, tm, tl, weight, K):
    mean, logvar, tm, tl, weight = _c(mean), _c(logvar), _c(tm), _c(tl), _c(weight)
    G, J = weight.shape
    idx, fit, n_bad = np.zeros(G, np.int32), np.zeros((G, K), F32), np.zeros(1, np.int32)
    rc = L.dfx_debug_select_fit_host(_p(mean), _p(logvar), _p(tm), _p(tl), _p(weight), G, K, J, _p(idx), _p(fit), _p(n_bad))
    assert rc == 0, L.dfx_last_error()
    return idx, fit, int(n_bad[0])


# ---------------------------------------------------------------------------------------------------- inputs
def validity(G, J, rng):
    """(G,J) 0/1 floats cycling through: all valid, one absent, the first absent, two absent (as far as J allows; never empty)."""
    v = np.ones((G, J), F32)
    for g in range(G):
        kind = g % 4
        if kind == 1 and J > 1:
            v[g, 1 + rng.integers(J - 1)] = 0
        elif kind == 2 and J > 1:
            v[g, 0] = 0
        elif kind == 3 and J > 2:
            v[g, rng.choice(J, 2, replace=False)] = 0
    return v


def make_case(G, K, J, seed, n_draws=64):
    """Aligner-like parameters (anchors within the unit box, log-variances around -4), validity patterns, stats of real draws."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mean = (0.5 * rng.standard_normal((G * K, 3, J))).astype(F32)
    logvar = (-4.0 + 0.7 * rng.standard_normal((G * K, 3, J))).astype(F32)
    valid = validity(G, J, rng)
    stats = stats_of(rng.standard_normal((G * K, n_draws, 3, J)).astype(F32)).astype(F32)
    tm = (0.5 * rng.standard_normal((G, 3, J))).astype(F32)
    tl = (-4.0 + 0.7 * rng.standard_normal((G, 3, J))).astype(F32)
    return dict(mean=mean, logvar=logvar, valid=valid, stats=stats, tm=tm, tl=tl, G=G, K=K, J=J)


# G, K, J, P: the shapes the issue names (K = 1, 2; P = K; J in 1, 4, 5, 8; G in 1, 7; K around the wavefront / workgroup sizes)
BOUNDARY_SHAPES = [(1, 1, 4, 1), (1, 2, 4, 2), (7, 2, 1, 1), (1, 63, 5, 8), (7, 64, 4, 64), (1, 65, 8, 5), (7, 257, 4, 9), (1, 100, 4, 100)]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))
