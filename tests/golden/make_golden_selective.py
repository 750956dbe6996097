#!/usr/bin/env python
"""Golden vectors of the reference's selective noise sampling (dev container only; same conventions as make_golden_partsample.py,
whose helpers this imports).

    python tests/golden/make_golden_selective.py

Written to tests/golden/selective/ with their own MANIFEST.sha256.  configs/gen_chair.py with num_timesteps = 10, npoints = 64, the
synthetic weights of synth.make_*_weights(seed=0); the reference's own methods run on CPU:

global_first_pick_all.npz      PartEncoder.subsample_params_global (part_encoders.py:591-621) called directly on the reference aligner's
global_first_pick_absent2.npz  outputs for 6 shapes x 100 noises, num = 24: every part valid / part 2 absent in every shape (one mask
                               shared by all rows).  codes (6,zdim,4), noise (600,noise_dim), valid (6,4), mean / logvar (600,3,4):
                               the aligner's outputs; stats: the four float64 statistics of the 600 recorded (512,3,4) draws; ids,
                               sel_mean, sel_logvar: what the reference returned.  The reference never appends to out_score (:603), so
                               its ids are "row 0, then by descending distance to row 0": the FIRST_PICK rule.
sample_latents_shape_S3.npz    PartEncoder.sample_latents (:1052-1110) with selective_noise_sampling = True: 3 shapes (shape 1 without
sample_latents_shape_S3_fixed.npz  part 2), K = 100 -> 10 rows per shape; the second run with fixed_id = [0,1,0,0].  in/valid, in/fixed_id;
                               draw_0 = w, draw_1 = the aligner noises; stats of the 300 (512,3,4) draws that follow; cand/mean,
                               cand/logvar: the aligner's outputs for all 300 candidates; ids (3,10): the picks (the rows of cand/*
                               the returned parameters equal); out/*: the returned tensors.

Every greedy step gets its float64 gap (best to runner-up, relative to the winner), and the reference's float32 distances (recorded
at its mse_loss calls) their largest deviation from the float64 ones relative to the smallest winning distance.  A fixture whose
smallest gap is below 20 x that deviation is refused; both numbers are stored (min_gap, max_dev).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "selective")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_forward as mgf  # noqa: E402  (sets up sys.path for ref_import / difffacto_amd)
from make_golden_edit import _model  # noqa: E402
from make_golden_forward import DrawRecorder  # noqa: E402
from make_golden_partsample import _capture_distances, _capture_params, _check, _quiet  # noqa: E402
import manifest  # noqa: E402
import _part_sampling_case as ps  # noqa: E402
import _selective_case as sel  # noqa: E402

F32, F64 = np.float32, np.float64
N, K, KEEP = 64, 100, 10      # K and the 10 kept rows are hard-coded in the reference (:1064, :1090, :1096)


def gen_global(tag, absent, S=6, P=24, seed=401):
    enc = _model().encoder
    J = enc.n_class
    rng = np.random.Generator(np.random.PCG64(seed))
    valid = np.ones((S, J), F32)
    if absent is not None:
        valid[:, absent] = 0
    codes = rng.standard_normal((S, enc.zdim, J)).astype(F32)
    noise = rng.standard_normal((S * K, enc.part_aligner.noise_dim)).astype(F32)
    rows_valid = torch.from_numpy(np.repeat(valid, K, 0))
    with torch.no_grad(), _quiet():
        mean, logvar = enc.get_params_from_part_code(torch.from_numpy(np.repeat(codes, K, 0)), rows_valid, noise=torch.from_numpy(noise))
    sq = []
    restore = _capture_distances(sq)
    with DrawRecorder(seed + 1) as rec, torch.no_grad(), _quiet():
        (sel_mean, sel_logvar), ids = enc.subsample_params_global(mean.clone(), logvar.clone(), rows_valid.clone(), P)
    restore()
    ids = ids.numpy().astype(np.int32)
    assert len(rec.draws) == S * K and rec.draws[0].shape == (512, 3, J) and len(sq) == P - 1
    stats = ps.stats_of(np.stack(rec.draws))
    m, l = mean.numpy(), logvar.numpy()
    sc64 = ps.scores_f64(m, l, valid, stats, K)
    idx64, dist64, gap = sel.diverse_global_f64(sc64, valid, K, P, "first_pick")
    assert np.array_equal(idx64, ids), "the float64 first-pick rule picks what the reference picked"
    far, _, _ = sel.diverse_global_f64(sc64, valid, K, P, "farthest")
    assert not np.array_equal(far, ids), "farthest-point selection picks other rows: the reference does not do it"
    # the reference's own float32 distances to row 0 (every recorded call holds the same ones) against the float64 ones
    v = rows_valid[:, None, :] * rows_valid[:1, None, :]
    d32 = ((sq[0][:, 0] * v).sum((-1, -2)) / v[:, 0].sum(-1)).numpy().astype(F64)
    d64 = sel.dist_to(sc64, sel.row_masks(valid, K), 0)
    dev = float(np.abs(d32 - d64).max() / dist64[1:].min())
    min_gap = float(gap[1:].min())
    _check(tag, min_gap, dev)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), codes=codes, noise=noise, valid=valid, mean=m, logvar=l, stats=stats, ids=ids,
                        sel_mean=sel_mean.numpy().astype(F32), sel_logvar=sel_logvar.numpy().astype(F32), K=np.array(K), P=np.array(P),
                        min_gap=np.array(min_gap), max_dev=np.array(dev))


def gen_shape(tag, fixed, S=3, seed=411):
    enc = _model().encoder
    enc.selective_noise_sampling = True
    J = enc.n_class
    valid = np.ones((S, J), F32)
    valid[1, 2] = 0
    fixed = np.asarray(fixed, F32)
    cand = []
    _capture_params(enc, cand)
    sq = []
    restore = _capture_distances(sq)
    with DrawRecorder(seed + 1) as rec, torch.no_grad(), _quiet():
        ctx, mpp, lpp, seg, valid_out, (codes, means, logvars, noise) = enc.sample_latents(
            S, N, "cpu", fixed_id=torch.from_numpy(fixed.copy()), valid_id=torch.from_numpy(valid.copy()), epoch=0)
    restore()
    assert len(cand) == 1 and len(rec.draws) == 2 + S * K and rec.draws[1].shape == (S * K, enc.part_aligner.noise_dim) and rec.draws[1].any()
    m, l = cand[0]
    stats = ps.stats_of(np.stack(rec.draws[2:]))
    merged = valid * (1 - fixed) + fixed * np.clip(valid[:1] + fixed, 0, 1)                  # :1072-1075
    sc64 = ps.scores_f64(m, l, merged, stats, K)
    idx64, dist64, gap = ps.diverse_f64(sc64, merged, K, KEEP)
    got_m = means.numpy().reshape(S, KEEP, 3, J)
    ids = np.array([[int(np.flatnonzero((m.reshape(S, K, 3, J)[s] == got_m[s, p]).all((1, 2)))[0]) for p in range(KEEP)] for s in range(S)], np.int32)
    assert np.array_equal(idx64, ids), "the float64 closed form picks what the reference picked"
    # the reference's float32 distances (one recorded call per step and free candidate, in its loop order) against the float64 ones
    dev, call = 0.0, 0
    s64 = sc64.reshape(S, K, 6, J)
    for g in range(S):
        v = torch.from_numpy(merged[g])
        for t in range(1, KEEP):
            picked = list(ids[g, :t])
            for i in (i for i in range(K) if i not in picked):
                d32 = float(((sq[call] * v[None, None]).sum((-1, -2)) / v.sum()).min())
                d64 = float(min(ps.pair_dist(s64[g, i], s64[g, p], merged[g]) for p in picked))
                dev = max(dev, abs(d32 - d64) / dist64[g, t])
                call += 1
    assert call == len(sq)
    min_gap = float(gap[:, 1:].min())
    _check(tag, min_gap, dev)
    out = mgf.np_out(dict(ctx0=ctx[0], ctx1=ctx[1], mean_per_point=mpp, logvar_per_point=lpp, seg=seg, valid=valid_out, codes=codes, means=means,
                          logvars=logvars))
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **{"in/valid": valid, "in/fixed_id": fixed.astype(np.int32)}, draw_0=rec.draws[0],
                        draw_1=rec.draws[1], stats=stats, **{"cand/mean": m, "cand/logvar": l}, ids=ids, **out, K=np.array(K),
                        keep=np.array(KEEP), N=np.array(N), min_gap=np.array(min_gap), max_dev=np.array(dev))


def main():
    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    gen_global("global_first_pick_all", None)
    gen_global("global_first_pick_absent2", 2)
    gen_shape("sample_latents_shape_S3", [0, 0, 0, 0])
    gen_shape("sample_latents_shape_S3_fixed", [0, 1, 0, 0])
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
