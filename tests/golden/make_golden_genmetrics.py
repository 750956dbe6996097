#!/usr/bin/env python
"""Golden vectors of the reference's whole-set generation metrics: MMD / COV / 1-NNA under CD and EMD (dev container only; the
reference's own functions on CPU, nothing of its text is copied: its functions are called and what they return is recorded).

    python tests/golden/make_golden_genmetrics.py

Written to tests/golden/genmetrics/ with their own MANIFEST.sha256 (manifest.content_hash).  Deterministic: a second run writes the
same manifest.  The seed and the smallest decision margin of every fixture are printed and stored in it.

The reference's two CUDA extensions cannot load here and are replaced, only around the calls that need them, by
  distChamferCUDA   a float64 brute force from the definition: per-point squared nearest-neighbour distances in both directions by
                    direct differences, cast to float32 on return (not the reference's expanded-form distChamfer, whose cancellation
                    error test_oracle_pointnet2_cpu.py documents)
  emd_approx        oracle.pointnet2.emd_forward(a, b, 0.002, 10000) then sqrt(dist).mean(1), as _brute of test_gpu_evaluation.py
Tensor.cuda is a no-op around the same calls and the reference's prints are silenced.

knn.npz           the reference's knn on seeded block matrices (bookkeeping only), every key of its dict: (nx, ny) in (1,1) [k = 1
                  only: two clouds have one neighbour], (5,7), (12,12), (20,9); k in 1, 2, 3; sqrt off / on (one negative entry when
                  on); one_way off / on (Myy all +inf when on); symmetric Mxx, Myy, entries uniform in [0.1, 1]: 40 cases
mmdcov.npz        the reference's lgan_mmd_cov on (5,7), (9,4), (1,3) matrices at thresh 1000, 0.3, 0.15, 0.0 (no outlier, some, all
                  folded onto sorted_idx[0]): 12 cases
all_metrics_{plain,masked,one_way}.npz
                  the reference's compute_all_metrics(sample, ref, batch_size=3, ...): inputs, the matrices rs / rr / ss for CD and
                  EMD (captured by wrapping _pairwise_EMD_CD_; one_way has no ss), every key of the result in order.  N_sample = 7,
                  N_ref = 6, n = 64 points in the unit cube; samples 0..2 are references 0..2 + 0.02 N(0,1) (clipped to the cube), the
                  rest uniform in [0.2, 0.8]^3.  masked: every sample cloud keeps its first 24..64 points (one keeps all 64), repeated
                  in index order up to 64, mask = 1 on the first pass only, handed over as mask=.  one_way: the masked clouds and mask
                  with one_way=True.
paired.npz        the reference's EMD_CD(accelerated_cd=True) on 6 pairs (the plain fixture's samples 0..5 and references),
                  batch_size=4, reduced both ways
part_weighted.npz the reference's compute_part_metric end to end on the inputs of partmetrics/clouds.npz (read, never rewritten):
                  every part_weighted_* key it may hold (see below) and the six matrices per class

Decision margins.  COV and 1-NNA count argmin decisions, so a fixture whose decisions rounding can flip is useless.  For every
all_metrics fixture, on float64 matrices (tests/_genmetrics_case.py: chamfer_matrix, emd_matrix) and for CD and EMD alike, the gap
between the smallest and the second-smallest entry is at least MARGIN = 1e-4 (100 x the 1e-6 the matrices are held to) in every
column of the leave-one-out block matrix that a decision reads, and in every column of the (sample, reference) matrix (each
reference's closest sample).  The plain fixture also has acc, acc_t, acc_f and lgan_cov strictly inside (0, 1) and acc_t != acc_f, for
CD and EMD.  Every fixture's EMD decisions differ from its CD ones: lgan_cov-EMD != lgan_cov-CD and, where 1-NNA is not 1 by definition
(one_way), at least one of 1-NN-EMD-acc_t / acc_f / acc differs from its CD twin, so that a CD matrix left in an EMD line shows.  CD and
EMD rank these clouds alike most of the time, which is why the search runs over seeds 0..255: upward from 0, the first seed that
passes everything is taken (plain: 121, masked and one_way: 4).  Were none to reach MARGIN for a fixture, the seed with the largest
margin among those that pass the rest would be taken and that fixture's ``tol`` set to a hundredth of it.  That did not happen: every
fixture carries tol = 1e-6.  part_weighted.npz cannot choose its inputs: for a distance (CD, EMD) whose margin is below 100 x tol in any class, the
keys that count decisions (lgan_cov-*, 1-NN-*) are left out and ``left_out`` / ``why_left_out`` say so; ``keys`` lists what is held.  On
the committed clouds.npz the CD margins are 4.5e-4 and more, the EMD margin of class 2 is 5.8e-5: the EMD decision keys are left out, the
MMD keys of both distances and every CD key are held.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "genmetrics")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import _genmetrics_case as gm  # noqa: E402
import manifest  # noqa: E402
import ref_import  # noqa: E402
from make_golden_partmetrics import patched  # noqa: E402

F32, F64 = np.float32, np.float64
MARGIN = 1e-4
TOL = 1e-6
N_SAMPLE, N_REF, N_POINTS = 7, 6, 64
SEEDS = 256


@contextlib.contextmanager
def standins(eu):
    with patched(eu, "distChamferCUDA", gm.cd_standin), patched(eu, "emd_approx", gm.emd_standin), \
            patched(torch.Tensor, "cuda", lambda self, *a, **k: self), contextlib.redirect_stdout(io.StringIO()), \
            contextlib.redirect_stderr(io.StringIO()):
        yield


def capture_matrices(eu, call):
    """call() under the stand-ins with every _pairwise_EMD_CD_ result recorded in call order."""
    mats = []
    orig = eu._pairwise_EMD_CD_

    def rec(*a, **k):
        k["verbose"] = False
        cd, emd = orig(*a, **k)
        mats.append((cd.numpy().copy(), emd.numpy().copy()))
        return cd, emd
    with standins(eu), patched(eu, "_pairwise_EMD_CD_", rec):
        res = call()
    return mats, res


def clouds(seed, masked):
    rng = np.random.default_rng(seed)
    ref = rng.uniform(0, 1, (N_REF, N_POINTS, 3)).astype(F32)
    near = np.clip(ref[:3] + 0.02 * rng.standard_normal((3, N_POINTS, 3)), 0, 1).astype(F32)
    sample = np.concatenate([near, rng.uniform(0.2, 0.8, (N_SAMPLE - 3, N_POINTS, 3)).astype(F32)])
    if not masked:
        return sample, ref, None
    count = rng.integers(24, N_POINTS, N_SAMPLE)
    count[rng.integers(0, N_SAMPLE)] = N_POINTS
    mask = np.zeros((N_SAMPLE, N_POINTS), F32)
    for i, c in enumerate(count):
        sample[i] = sample[i][np.arange(N_POINTS) % c]
        mask[i, :c] = 1
    return sample, ref, mask


def margins(sample, ref, mask, one_way):
    """float64 matrices and per distance the smallest decision gap (block-matrix columns, reference-to-sample minimum)."""
    m = {"rs_cd": gm.chamfer_matrix(ref, sample, None, mask), "rs_emd": gm.emd_matrix(ref, sample),
         "rr_cd": gm.chamfer_matrix(ref, ref), "rr_emd": gm.emd_matrix(ref, ref)}
    if not one_way:
        m["ss_cd"], m["ss_emd"] = gm.chamfer_matrix(sample, sample, mask, mask), gm.emd_matrix(sample, sample)
    gap = {}
    for d in ("cd", "emd"):
        ss = m.get(f"ss_{d}", np.full((len(sample),) * 2, np.inf))
        block = gm.block_matrix(m[f"rr_{d}"], m[f"rs_{d}"], ss)
        if one_way:
            block = block[:, :len(ref)]
        gap[d] = min(gm.column_gap(block), gm.column_gap(m[f"rs_{d}"].T))
    return m, gap


def nontrivial(m):
    r = gm.all_metrics(**m)
    for d in ("CD", "EMD"):
        if not all(0 < r[k] < 1 for k in (f"1-NN-{d}-acc", f"1-NN-{d}-acc_t", f"1-NN-{d}-acc_f", f"lgan_cov-{d}")):
            return False
        if abs(r[f"1-NN-{d}-acc_t"] - r[f"1-NN-{d}-acc_f"]) < 1e-6:
            return False
    return True


def distinct(r):
    """The EMD decisions differ from the CD ones: lgan_cov, and at least one of the 1-NN accuracies.  Without this a CD matrix in
    an EMD line of compute_all_metrics would give the recorded numbers."""
    return r["lgan_cov-EMD"] != r["lgan_cov-CD"] and any(r[f"1-NN-EMD-{k}"] != r[f"1-NN-CD-{k}"] for k in ("acc_t", "acc_f", "acc"))


def search(masked, need_nontrivial):
    """(seed, tol): the first seed of 0..SEEDS-1 whose metrics are as wanted (distinct; plain: nontrivial) and whose margins reach
    MARGIN, else the one with the largest margin among those and tol = margin / 100."""
    best, why = None, {"trivial metrics": 0, "EMD decisions equal CD's": 0, "margin": 0}
    for seed in range(SEEDS):
        sample, ref, mask = clouds(seed, masked)
        m, gap = margins(sample, ref, mask, False)
        g = min(gap.values())
        if need_nontrivial and not nontrivial(m):
            why["trivial metrics"] += 1
        elif not distinct(gm.all_metrics(**m)):
            why["EMD decisions equal CD's"] += 1
        elif g >= MARGIN:
            print(f"  seed {seed} taken: gap CD {gap['cd']:.3g} EMD {gap['emd']:.3g}; seeds rejected before it: {why}")
            return seed, TOL
        else:
            why["margin"] += 1
            if best is None or g > best[1]:
                best = (seed, g)
    assert best is not None
    return best[0], best[1] / 100


def all_metrics_fixture(eu, name, seed, tol, masked, one_way):
    sample, ref, mask = clouds(seed, masked)
    m64, gap = margins(sample, ref, mask, one_way)
    assert min(gap.values()) >= 100 * tol * (1 - 1e-9), (name, gap, tol)
    kw = {} if mask is None else {"mask": torch.from_numpy(mask)}
    mats, res = capture_matrices(eu, lambda: eu.compute_all_metrics(torch.from_numpy(sample), torch.from_numpy(ref), batch_size=3,
                                                                    one_way=one_way, **kw))
    assert len(mats) == (2 if one_way else 3)
    out = {"sample": sample, "ref": ref, "seed": np.int64(seed), "tol": F64(tol), "gap_cd": F64(gap["cd"]), "gap_emd": F64(gap["emd"]),
           "one_way": np.int32(one_way)}
    if mask is not None:
        out["mask"] = mask
    for tag, (cd, emd) in zip(("rs", "rr", "ss"), mats):
        out[f"{tag}_cd"], out[f"{tag}_emd"] = cd, emd
        assert np.abs(cd - m64[f"{tag}_cd"]).max() < tol and np.abs(emd - m64[f"{tag}_emd"]).max() < tol, (name, tag)
    out["res_keys"] = np.array(list(res))
    for k, v in res.items():
        out[f"res_{k}"] = np.asarray(v.numpy())
    if name == "plain":
        for d in ("CD", "EMD"):
            a, t, f, c = (float(res[k]) for k in (f"1-NN-{d}-acc", f"1-NN-{d}-acc_t", f"1-NN-{d}-acc_f", f"lgan_cov-{d}"))
            assert all(0 < v < 1 for v in (a, t, f, c)) and t != f, (d, a, t, f, c)
    got = {k: float(v) for k, v in res.items()}
    assert got["lgan_cov-EMD"] != got["lgan_cov-CD"] and (one_way or distinct(got)), (name, got)
    np.savez(os.path.join(OUT, f"all_metrics_{name}.npz"), **out)
    print(f"all_metrics_{name}: seed {seed}, smallest margin CD {gap['cd']:.3g} EMD {gap['emd']:.3g}, tol {tol:.3g}; " +
          ", ".join(f"{k} {float(v):.4g}" for k, v in res.items()))
    return sample, ref


def symmetric(rng, n):
    u = rng.uniform(0.1, 1, (n, n))
    return (np.triu(u) + np.triu(u, 1).T).astype(F32)


def knn_fixture(eu):
    rng = np.random.default_rng(20261020)
    out, c = {}, 0
    for nx, ny in ((1, 1), (5, 7), (12, 12), (20, 9)):
        for k in ((1,) if nx + ny == 2 else (1, 2, 3)):
            for sqrt in (False, True):
                for one_way in (False, True):
                    while True:   # redrawn until no two entries of a column are closer than 1e-5 (root taken or not): no ties
                        Mxx, Mxy, Myy = symmetric(rng, nx), rng.uniform(0.1, 1, (nx, ny)).astype(F32), symmetric(rng, ny)
                        if sqrt:
                            Mxy[rng.integers(0, nx), rng.integers(0, ny)] *= -1
                        if one_way:
                            Myy[:] = np.inf
                        block = np.abs(gm.block_matrix(Mxx, Mxy, Myy))
                        if min(gm.column_spacing(block), gm.column_spacing(np.sqrt(block))) > 1e-5:
                            break
                    with contextlib.redirect_stdout(io.StringIO()):
                        res = eu.knn(torch.from_numpy(Mxx), torch.from_numpy(Mxy), torch.from_numpy(Myy), k, sqrt=sqrt, one_way=one_way)
                    out[f"c{c}_Mxx"], out[f"c{c}_Mxy"], out[f"c{c}_Myy"] = Mxx, Mxy, Myy
                    out[f"c{c}_args"] = np.asarray([k, sqrt, one_way], np.int32)
                    assert tuple(res) == gm.KNN_KEYS
                    out[f"c{c}_res"] = np.asarray([v.numpy() for v in res.values()], F32)
                    c += 1
    out["n_cases"], out["res_keys"] = np.int32(c), np.array(list(res))
    np.savez(os.path.join(OUT, "knn.npz"), **out)
    print(f"knn: {c} cases")


def mmdcov_fixture(eu):
    rng = np.random.default_rng(20261021)
    out, c, covs = {}, 0, []
    for ns, nr in ((5, 7), (9, 4), (1, 3)):
        D = rng.uniform(0.1, 1, (ns, nr)).astype(F32)
        for thresh in (1000, 0.3, 0.15, 0.0):
            with contextlib.redirect_stdout(io.StringIO()):
                res = eu.lgan_mmd_cov(torch.from_numpy(D.copy()), thresh=thresh)
            out[f"c{c}_D"], out[f"c{c}_thresh"] = D, F64(thresh)
            assert tuple(res) == gm.MMDCOV_KEYS
            out[f"c{c}_res"] = np.asarray([v.numpy() for v in res.values()], F32)
            covs.append(float(res["lgan_cov"]))
            c += 1
        n_out = [int((D.min(0) > t).sum()) for t in (1000, 0.3, 0.15, 0.0)]
        print(f"mmdcov {ns}x{nr}: outliers per thresh {n_out}, cov {covs[-4:]}")
        assert n_out[0] == 0 and n_out[3] == nr
    out["n_cases"], out["res_keys"] = np.int32(c), np.array(list(gm.MMDCOV_KEYS))
    np.savez(os.path.join(OUT, "mmdcov.npz"), **out)


def paired_fixture(eu, sample, ref):
    out = {"sample": sample[:N_REF], "ref": ref}
    for reduced in (True, False):
        with standins(eu):
            res = eu.EMD_CD(torch.from_numpy(sample[:N_REF]), torch.from_numpy(ref), 4, accelerated_cd=True, reduced=reduced)
        tag = "reduced" if reduced else "full"
        out[f"{tag}_keys"] = np.array(list(res))
        for k, v in res.items():
            out[f"{tag}_{k}"] = np.asarray(v.numpy())
    np.savez(os.path.join(OUT, "paired.npz"), **out)
    print("paired: MMD-CD %.6g MMD-EMD %.6g" % (float(out["reduced_MMD-CD"]), float(out["reduced_MMD-EMD"])))


def part_weighted_fixture(eu):
    z = np.load(os.path.join(HERE, "partmetrics", "clouds.npz"))
    mats, res = capture_matrices(eu, lambda: eu.compute_part_metric(torch.from_numpy(z["preds"]), torch.from_numpy(z["preds_mask"]).long(),
                                                                    torch.from_numpy(z["refs"]), torch.from_numpy(z["refs_mask"]).long(),
                                                                    32, n_class=4))
    assert len(mats) == 12
    out, gaps = {}, {"CD": [], "EMD": []}
    for j in range(4):
        sample, ref, mask = z[f"pred_{j}"], z[f"ref_{j}"], z[f"mask_{j}"]
        m64, gap = margins(sample, ref, mask, False)
        gaps["CD"].append(gap["cd"])
        gaps["EMD"].append(gap["emd"])
        out[f"gap_{j}"] = np.asarray([gap["cd"], gap["emd"]], F64)
        for tag, (cd, emd) in zip(("rs", "rr", "ss"), mats[3 * j:3 * j + 3]):
            out[f"{tag}_cd_{j}"], out[f"{tag}_emd_{j}"] = cd, emd
            err = max(np.abs(cd - m64[f"{tag}_cd"]).max(), np.abs(emd - m64[f"{tag}_emd"]).max())
            assert err < TOL, (j, tag, err)
        print(f"part_weighted class {j}: {len(sample)} x {len(ref)} clouds, margin CD {gap['cd']:.3g} EMD {gap['emd']:.3g}")
    # a distance whose margin is below 100 x tol in any class keeps its MMD keys only (they involve no decision)
    decided = {d: min(g) >= 100 * TOL for d, g in gaps.items()}
    keys = [k for k in res if "mmd" in k or decided["EMD" if "EMD" in k else "CD"]]
    left = [k for k in res if k not in keys]
    out["tol"] = F64(TOL)
    out["all_keys"], out["keys"], out["left_out"] = np.array(list(res)), np.array(keys), np.array(left, dtype="U64")
    out["why_left_out"] = np.array("; ".join(f"{d}: a class's smallest decision margin {min(g):.3g} is below 100 x tol = {100 * TOL:g}"
                                             for d, g in gaps.items() if not decided[d]))
    for k in keys:
        out[f"res_{k}"] = np.asarray(res[k].numpy())
    np.savez(os.path.join(OUT, "part_weighted.npz"), **out)
    print(f"part_weighted: smallest margin CD {min(gaps['CD']):.3g} EMD {min(gaps['EMD']):.3g}; keys held {len(keys)}, left out {left}")


def main():
    with contextlib.redirect_stdout(io.StringIO()):
        ref_import.import_reference()
        import difffacto.datasets.evaluation_utils as eu
    os.makedirs(OUT, exist_ok=True)
    knn_fixture(eu)
    mmdcov_fixture(eu)
    print("plain: seed search")
    seed, tol = search(False, True)
    sample, ref = all_metrics_fixture(eu, "plain", seed, tol, False, False)
    paired_fixture(eu, sample, ref)
    print("masked: seed search")
    seed, tol = search(True, False)
    all_metrics_fixture(eu, "masked", seed, tol, True, False)
    all_metrics_fixture(eu, "one_way", seed, tol, True, True)
    part_weighted_fixture(eu)
    with open(os.path.join(OUT, "MANIFEST.sha256"), "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    for fn in sorted(os.listdir(OUT)):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
