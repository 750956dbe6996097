"""Candidate selection of part-level sampling on device tensors (csrc/part_sampling.hip): the statistics of the unit
draws of ``PartEncoder.subsample_params`` (part_encoders.py:545-589), its greedy diverse selection in closed form, and the fit
arg-min of ``sample_with_fixed_latents`` (:678-682).  Usable on their own on any (mean, logvar) candidates; the search that runs the
aligner over the candidates is ``LatentSampler.part_search``, the whole mode ``editing.sample_part``.

Candidate row ``g * K + k`` is candidate k of group g.  Every function launches on the current stream and returns device tensors;
``n_bad`` (1,) int32 counts the candidates whose score is not finite (never picked while a finite one remains).
"""
import torch

from . import _ffi

MODES = {"fit": 0, "first": 1, "diverse": 2}   # DFX_SEARCH_*
RULES = {"farthest": 0, "first_pick": 1}       # DFX_DIVERSE_*


def rule_id(rule):
    if isinstance(rule, str):
        if rule not in RULES:
            raise ValueError(f"rule {rule!r} not in {sorted(RULES)}")
        return RULES[rule]
    return int(rule)


def _f(t, device=None):
    return None if t is None else t.detach().to(device=device or t.device, dtype=torch.float32).contiguous()


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("part_sampling: device tensors expected (there is no CPU path)")


def draw_stats(rows, n_class, seed, row0=0, n_draws=512, device="cuda"):
    """(rows,4,3,n_class): mean, unbiased std, min, max of ``n_draws`` standard normals per (global row row0 + r, axis, part), Philox
    keyed by (seed, global row, axis, part, draw).  The normals are never stored; a call split over ``row0`` gives the same numbers."""
    out = torch.empty(int(rows), 4, 3, int(n_class), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        rc = _ffi.lib().dfx_part_draw_stats(int(seed), int(row0), int(rows), int(n_class), int(n_draws), _ffi.ptr(out), _ffi.current_stream())
    _ffi.check(rc, "dfx_part_draw_stats")
    return out


def draw_normals(rows, n_class, seed, row0=0, n_draws=512, device="cuda"):
    """Debug: the (rows,n_draws,3,n_class) normals ``draw_stats`` reduces."""
    out = torch.empty(int(rows), int(n_draws), 3, int(n_class), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        rc = _ffi.lib().dfx_debug_part_draw_normals(int(seed), int(row0), int(rows), int(n_class), int(n_draws), _ffi.ptr(out),
                                                    _ffi.current_stream())
    _ffi.check(rc, "dfx_debug_part_draw_normals")
    return out


def select_diverse(mean, logvar, valid, K, P, stats=None, seed=0, row0=0, n_draws=512):
    """Greedy diverse selection: mean, logvar (G K,3,J), valid (G,J) -> dict idx (G,P) int32, scores (G K,6,J), n_bad.  ``stats``
    (G K,4,3,J) as ``draw_stats`` writes them, or None: ``draw_stats(G K, J, seed, row0, n_draws)`` first."""
    _need_gpu(mean)
    mean, logvar, valid, stats = _f(mean), _f(logvar, mean.device), _f(valid, mean.device), _f(stats, mean.device)
    G, J = valid.shape
    K, P = int(K), int(P)
    if stats is None:
        stats = draw_stats(G * K, J, seed, row0=row0, n_draws=n_draws, device=mean.device)
    assert tuple(mean.shape) == (G * K, 3, J) == tuple(logvar.shape) and (stats is None or tuple(stats.shape) == (G * K, 4, 3, J))
    idx = torch.empty(G, P, dtype=torch.int32, device=mean.device)
    scores = torch.empty(G * K, 6, J, dtype=torch.float32, device=mean.device)
    n_bad = torch.empty(1, dtype=torch.int32, device=mean.device)
    with torch.cuda.device(mean.device):
        rc = _ffi.lib().dfx_select_diverse(_ffi.ptr(mean), _ffi.ptr(logvar), _ffi.ptr(valid), _ffi.ptr(stats), G, K, J, P, _ffi.ptr(idx), _ffi.ptr(scores), _ffi.ptr(n_bad), _ffi.current_stream())
    _ffi.check(rc, "dfx_select_diverse")
    return {"idx": idx, "scores": scores, "n_bad": n_bad}


def select_diverse_global(mean, logvar, valid, K, P, rule="farthest", stats=None, seed=0, row0=0, n_draws=512):
    """Greedy diverse selection over all G K rows of the call (``dfx_select_diverse_global``): mean, logvar (G K,3,J),
    valid (G,J) -> dict idx (P,) int32 GLOBAL rows, scores (G K,6,J), n_bad.  Two rows are compared on the parts valid in both; a pair
    without a common part is skipped.  ``rule``: 'farthest' (farthest-point selection, the reference's intent) or 'first_pick' (distance
    to pick 0 only, what the reference's subsample_params_global executes).  ``stats`` as ``select_diverse``."""
    _need_gpu(mean)
    mean, logvar, valid, stats = _f(mean), _f(logvar, mean.device), _f(valid, mean.device), _f(stats, mean.device)
    G, J = valid.shape
    K, P, rule = int(K), int(P), rule_id(rule)
    if stats is None:
        stats = draw_stats(G * K, J, seed, row0=row0, n_draws=n_draws, device=mean.device)
    assert tuple(mean.shape) == (G * K, 3, J) == tuple(logvar.shape) and tuple(stats.shape) == (G * K, 4, 3, J)
    idx = torch.empty(P, dtype=torch.int32, device=mean.device)
    scores = torch.empty(G * K, 6, J, dtype=torch.float32, device=mean.device)
    n_bad = torch.empty(1, dtype=torch.int32, device=mean.device)
    nbytes = _ffi.lib().dfx_select_diverse_global_workspace_bytes(G * K)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=mean.device)
    with torch.cuda.device(mean.device):
        rc = _ffi.lib().dfx_select_diverse_global(_ffi.ptr(mean), _ffi.ptr(logvar), _ffi.ptr(valid), _ffi.ptr(stats), G, K, J, P, rule, _ffi.ptr(idx),
                                                  _ffi.ptr(scores), _ffi.ptr(n_bad), (ws.data_ptr() + 15) & ~15, nbytes, _ffi.current_stream())
    _ffi.check(rc, "dfx_select_diverse_global")
    return {"idx": idx, "scores": scores, "n_bad": n_bad}


def select_fit(mean, logvar, target_mean, target_logvar, weight, K):
    """Fit selection: mean, logvar (G K,3,J); target_mean, target_logvar (G,3,J); weight (G,J) = the validity mask with the resampled
    part zeroed -> dict idx (G,) int32 (the smallest weighted squared distance, the lowest index of equal ones), fit (G,K), n_bad."""
    _need_gpu(mean)
    dev = mean.device
    mean, logvar, target_mean, target_logvar, weight = _f(mean), _f(logvar, dev), _f(target_mean, dev), _f(target_logvar, dev), _f(weight, dev)
    G, J = weight.shape
    K = int(K)
    assert tuple(mean.shape) == (G * K, 3, J) == tuple(logvar.shape) and tuple(target_mean.shape) == (G, 3, J) == tuple(target_logvar.shape)
    idx = torch.empty(G, dtype=torch.int32, device=dev)
    fit = torch.empty(G, K, dtype=torch.float32, device=dev)
    n_bad = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _ffi.lib().dfx_select_fit(_ffi.ptr(mean), _ffi.ptr(logvar), _ffi.ptr(target_mean), _ffi.ptr(target_logvar), _ffi.ptr(weight), G, K, J,
                                       _ffi.ptr(idx), _ffi.ptr(fit), _ffi.ptr(n_bad), _ffi.current_stream())
    _ffi.check(rc, "dfx_select_fit")
    return {"idx": idx, "fit": fit, "n_bad": n_bad}
