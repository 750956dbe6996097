#!/usr/bin/env python
"""Golden vectors of the reference's part-level sampling (dev container only; same conventions as make_golden_edit.py, whose
helpers this imports).

    python tests/golden/make_golden_partsample.py

Written to tests/golden/partsample/ with their own MANIFEST.sha256.  configs/gen_chair.py with num_timesteps = 10, npoints = 64, the
synthetic weights of synth.make_*_weights(seed=0); the reference's own methods run on CPU:

fix_S4_E3.npz            PartEncoder.sample_with_fixed_latents(fix_size=True) (part_encoders.py:623-710) on 4 shapes x 3 new styles of
                         part 1, K = 100; shapes 1 and 3 have an absent part (shape 3 its first).  in/*: the arguments; draw_*: w, then
                         one (E K, noise_dim) per shape; cand/mean, cand/logvar: every candidate's aligner output (what the arg-min
                         reads; captured from the reference's own get_params_from_part_code calls); out/*: the returned tensors
one_part_S2_E2_T10.npz   the same call through AnchorDiffAE.sample_one_part (anchor_gen.py:307-337) with the T = 10 chain: cand/* as
                         above, out/pred and the chain draws (chain_at = index of x_T)
diverse_G6_K100_P8.npz   PartEncoder.subsample_params (:545-589) called directly on 6 groups x 100 candidates -> 8 picks, one group per
                         validity pattern (all valid, one absent, the first absent, two absent, then two more); mean / logvar are the
                         reference aligner's outputs for random codes; stats: the four float64 statistics of the 600 recorded
                         (512,3,4) draws (the draws themselves are 15 MB and are not stored); ids, sel_mean, sel_logvar: what the
                         reference returned

Only fix_size=True runs in the reference's sample_with_fixed_latents; the two other branches raise (a boolean mask / a Python list
where gather_operation needs indices), so they have no fixture.

Every decision of a fixture (greedy step, arg-min) gets its float64 gap (best to runner-up, relative to the winner), and the
reference's float32 distance / fit loss its largest relative deviation from the float64 one (both are the reference's own
float32 values: the fit loss recorded at its arg-min, the distances at its mse_loss calls).  A fixture whose smallest gap is below 20 x that deviation is refused; both numbers are stored (min_gap, max_dev).
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "partsample")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_forward as mgf  # noqa: E402  (sets up sys.path for ref_import / difffacto_amd)
from make_golden_edit import _model, _watch_chain  # noqa: E402
from make_golden_forward import DrawRecorder  # noqa: E402
import manifest  # noqa: E402
import _part_sampling_case as ps  # noqa: E402

F32, F64 = np.float32, np.float64
T, N, K = 10, 64, 100      # K is hard-coded in the reference (:664)
MARGIN = 20.0


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _inputs(S, seed, absent, zdim, J=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    valid = np.ones((S, J), F32)
    for s, j in absent:
        valid[s, j] = 0
    seg = np.zeros((S, N), np.int64)
    for s in range(S):
        ids = np.flatnonzero(valid[s])
        seg[s] = ids[rng.integers(0, len(ids), size=N)]
    return dict(codes=rng.standard_normal((S, zdim, J)).astype(F32), valid=valid,
                mean=(0.3 * rng.standard_normal((S, 3, J))).astype(F32), logvar=(-4 + 0.5 * rng.standard_normal((S, 3, J))).astype(F32),
                seg_mask=seg)


def _capture_params(enc, store):
    """Record what the reference's aligner returns for every candidate batch."""
    orig = enc.get_params_from_part_code

    def wrapped(*a, **k):
        m, l = orig(*a, **k)
        store.append((m.detach().numpy().copy(), l.detach().numpy().copy()))
        return m, l

    enc.get_params_from_part_code = wrapped


def _capture_fit(store):
    """Record the tensors the reference takes its arg-min over (:681: the float32 fit loss of every candidate, (E,K) per shape)."""
    orig = torch.Tensor.argmin

    def wrapped(self, *a, **k):
        store.append(self.detach().clone().numpy())
        return orig(self, *a, **k)

    torch.Tensor.argmin = wrapped
    return lambda: setattr(torch.Tensor, "argmin", orig)


def _fit_margins(cand, fit32, inp, part, E):
    """Float64 gap of every arg-min, and the deviation of the reference's own float32 fit loss (recorded at its arg-min) from the float64 one."""
    gaps, devs, picks = [], [], []
    assert len(fit32) == len(cand)
    for s, (m, l) in enumerate(cand):
        w = ps.fit_weight(np.repeat(inp["valid"][s:s + 1], E, 0), part)
        tm, tl = np.repeat(inp["mean"][s:s + 1], E, 0), np.repeat(inp["logvar"][s:s + 1], E, 0)
        idx, fit64, gap = ps.fit_f64(m, l, tm, tl, w, K)
        assert fit32[s].shape == fit64.shape
        devs.append(np.abs(fit32[s].astype(F64) - fit64).max() / fit64.min())
        gaps.append(gap.min())
        picks.append(idx)
    return min(gaps), max(devs), np.stack(picks)


def _check(tag, min_gap, max_dev):
    print(f"{tag}: smallest float64 gap {min_gap:.3g}, largest float32 deviation {max_dev:.3g} (ratio {min_gap / max_dev:.3g})")
    if not min_gap >= MARGIN * max_dev:
        raise SystemExit(f"{tag}: a decision is within {MARGIN} x the float32 deviation: a near-tie, choose another seed")


def gen_fix(tag="fix_S4_E3", S=4, E=3, part=1, seed=301):
    model = _model()
    enc = model.encoder
    inp = _inputs(S, seed, ((1, 2), (3, 0)), enc.zdim)
    cand = []
    _capture_params(enc, cand)
    fit32 = []
    restore = _capture_fit(fit32)
    t = lambda k: torch.from_numpy(inp[k].copy())
    with DrawRecorder(seed + 1) as rec, torch.no_grad(), _quiet():
        ctx, mpp, lpp, seg, valid, (codes, noise, means, logvars) = enc.sample_with_fixed_latents(
            t("codes"), t("valid"), t("mean"), t("logvar"), t("seg_mask"), part, E, True, 1, False)
    restore()
    min_gap, max_dev, picks = _fit_margins(cand, fit32, inp, part, E)
    _check(tag, min_gap, max_dev)
    out = mgf.np_out(dict(codes=codes, noise=noise, means=means, logvars=logvars, valid=valid, seg=seg, mean_per_point=mpp,
                          logvar_per_point=lpp))
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **{f"in/{k}": v for k, v in inp.items()}, **rec.as_dict(), **out,
                        **{"cand/mean": np.stack([m for m, _ in cand]), "cand/logvar": np.stack([l for _, l in cand])},
                        picks=picks, part=np.array(part), E=np.array(E), K=np.array(K), n_draws=np.array(len(rec.draws)),
                        min_gap=np.array(min_gap), max_dev=np.array(max_dev))


def gen_one_part(tag="one_part_S2_E2_T10", S=2, E=2, part=2, seed=311):
    model = _model()
    inp = _inputs(S, seed, ((1, 3),), model.encoder.zdim)
    cand = []
    _capture_params(model.encoder, cand)
    fit32 = []
    restore = _capture_fit(fit32)
    t = lambda k: torch.from_numpy(inp[k].copy())
    with DrawRecorder(seed + 1) as rec, torch.no_grad(), _quiet(), contextlib.redirect_stderr(io.StringIO()):
        at = _watch_chain(model, rec)
        chain = model.decode
        model.decode = lambda *a, **k: chain(*a, **{**k, "device": "cpu"})      # :330 hard-codes device='cuda'
        pred, seg, valid, codes, noise, means, logvars = model.sample_one_part(
            t("codes"), t("valid"), t("mean"), t("logvar"), t("seg_mask"), part, E, True, 1, False)
    restore()
    fit32 = fit32[:len(cand)]      # the chain takes no arg-min; keep the search's
    min_gap, max_dev, picks = _fit_margins(cand, fit32, inp, part, E)
    _check(tag, min_gap, max_dev)
    out = mgf.np_out(dict(pred=pred, seg=seg, valid=valid, codes=codes, noise=noise, means=means, logvars=logvars))
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **{f"in/{k}": v for k, v in inp.items()}, **rec.as_dict(), **out, picks=picks,
                        **{"cand/mean": np.stack([m for m, _ in cand]), "cand/logvar": np.stack([l for _, l in cand])},
                        part=np.array(part), E=np.array(E), K=np.array(K), T=np.array(T), n_draws=np.array(len(rec.draws)),
                        chain_at=np.array(at[0]), min_gap=np.array(min_gap), max_dev=np.array(max_dev))


def _capture_distances(store):
    """Record the element-wise squared differences the reference's greedy loop computes (its float32 scores against the selected ones)."""
    import torch.nn.functional as F
    orig = F.mse_loss

    def wrapped(*a, **k):
        d = orig(*a, **k)
        store.append(d.detach().clone())
        return d

    F.mse_loss = wrapped
    return lambda: setattr(F, "mse_loss", orig)


def gen_diverse(tag="diverse_G6_K100_P8", G=6, P=8, seed=11):
    model = _model()
    enc = model.encoder
    J = enc.n_class
    rng = np.random.Generator(np.random.PCG64(seed))
    valid = np.ones((G, J), F32)
    valid[1, 2] = 0
    valid[2, 0] = 0
    valid[3, [1, 3]] = 0
    valid[4, 3] = 0
    codes = torch.from_numpy(rng.standard_normal((G * K, enc.zdim, J)).astype(F32))
    noise = torch.from_numpy(rng.standard_normal((G * K, enc.part_aligner.noise_dim)).astype(F32))
    with torch.no_grad(), _quiet():
        mean, logvar = enc.get_params_from_part_code(codes, torch.from_numpy(np.repeat(valid, K, 0)), noise=noise)
    mean, logvar = mean.reshape(G, K, 3, J), logvar.reshape(G, K, 3, J)
    sq = []
    restore = _capture_distances(sq)
    with DrawRecorder(seed + 1) as rec, torch.no_grad(), _quiet():
        (sel_mean, sel_logvar), ids = enc.subsample_params(mean.clone(), logvar.clone(), torch.from_numpy(valid.copy()), P, return_ids=True)
    restore()
    ids = np.stack([np.asarray(i) for i in ids]).astype(np.int32)
    assert len(rec.draws) == G * K and rec.draws[0].shape == (512, 3, J)
    stats = ps.stats_of(np.stack(rec.draws))                                                   # (G K,4,3,J) float64
    m, l = mean.reshape(G * K, 3, J).numpy(), logvar.reshape(G * K, 3, J).numpy()
    sc64 = ps.scores_f64(m, l, valid, stats, K)
    idx64, dist64, gap = ps.diverse_f64(sc64, valid, K, P)
    assert np.array_equal(idx64, ids), "the float64 closed form picks what the reference picked"
    # the reference's own float32 distances (one recorded call per step and free candidate, in its loop order) against the float64 ones
    dev, call = 0.0, 0
    s64 = sc64.reshape(G, K, 6, J)
    for g in range(G):
        v = torch.from_numpy(valid[g])
        for t in range(1, P):
            sel = list(ids[g, :t])
            for i in (i for i in range(K) if i not in sel):
                d32 = float(((sq[call] * v[None, None]).sum((-1, -2)) / v.sum()).min())
                d64 = float(min(ps.pair_dist(s64[g, i], s64[g, p], valid[g]) for p in sel))
                dev = max(dev, abs(d32 - d64) / dist64[g, t])
                call += 1
    assert call == len(sq)
    min_gap = float(gap[:, 1:].min())
    _check(tag, min_gap, dev)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), mean=m, logvar=l, valid=valid, stats=stats, ids=ids,
                        sel_mean=sel_mean.numpy().astype(F32), sel_logvar=sel_logvar.numpy().astype(F32), K=np.array(K), P=np.array(P),
                        min_gap=np.array(min_gap), max_dev=np.array(dev))


def main():
    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    gen_diverse()
    gen_fix()
    gen_one_part()
    path = os.path.join(OUT, "MANIFEST.sha256")
    with open(path, "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                size = os.path.getsize(os.path.join(OUT, fn))
                assert size < 1 << 20, (fn, size)
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
