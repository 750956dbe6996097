"""CPU checks of the whole-set generation metrics' bookkeeping (difffacto_amd.evaluation: knn, lgan_mmd_cov, compute_all_metrics,
_pairwise_EMD_CD_'s pair and mask handling) against the reference's recorded values (tests/golden/genmetrics/,
make_golden_genmetrics.py) and against the float64 restatement of tests/_genmetrics_case.py.  No kernel runs here: where a test goes
through _pairwise_EMD_CD_, the two device calls are replaced by the host stand-ins the fixtures were recorded with."""
import os
import sys

import numpy as np
import pytest
import torch

import _genmetrics_case as gm

F32 = np.float32
FIXTURES = ("plain", "masked", "one_way")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _f32(v):
    return F32(float(v))


def test_knn_matches_reference_fixture():
    """The reference's knn on 40 block matrices: counts and acc bit-equal, the ratios (they carry + 1e-10) within 1e-6 relative."""
    from difffacto_amd import evaluation as ev
    n = 0
    for Mxx, Mxy, Myy, k, sqrt, one_way, want in gm.knn_cases():
        got = ev.knn(_t(Mxx), _t(Mxy), _t(Myy), k, sqrt=sqrt, one_way=one_way)
        case = (Mxx.shape[0], Myy.shape[0], k, sqrt, one_way)
        assert tuple(got) == gm.KNN_KEYS == tuple(want), case
        for key in gm.KNN_KEYS:
            assert got[key].dtype == torch.float32 and got[key].dim() == 0, (case, key)
            if key in gm.KNN_COUNTS:
                assert _f32(got[key]) == want[key], (case, key, float(got[key]), want[key])
            else:
                assert float(got[key]) == pytest.approx(float(want[key]), rel=1e-6, abs=0), (case, key)
        n += 1
    assert n == 40


def test_lgan_mmd_cov_matches_reference_fixture():
    """The reference's lgan_mmd_cov on 12 cases: lgan_cov and lgan_mmd bit-equal; lgan_mmd_smp within 1e-6 relative, because the
    reference sorts the samples' minima before it averages them and the mirror does not: one float32 ulp of summation order."""
    from difffacto_amd import evaluation as ev
    n, covs = 0, {}
    for D, thresh, want in gm.mmdcov_cases():
        got = ev.lgan_mmd_cov(_t(D), thresh=thresh)
        assert tuple(got) == gm.MMDCOV_KEYS == tuple(want)
        assert _f32(got["lgan_cov"]) == want["lgan_cov"], (D.shape, thresh, float(got["lgan_cov"]), want["lgan_cov"])
        assert _f32(got["lgan_mmd"]) == want["lgan_mmd"], (D.shape, thresh)
        assert float(got["lgan_mmd_smp"]) == pytest.approx(float(want["lgan_mmd_smp"]), rel=1e-6, abs=0), (D.shape, thresh)
        covs.setdefault(D.shape, []).append(float(want["lgan_cov"]))
        n += 1
    assert n == 12
    # the fixture itself: the fold changes COV (no outlier / some / all) on the 5 x 7 matrix
    assert len(set(covs[(5, 7)])) == 3


def _distinct(rng, *shapes):
    """Matrices whose entries (all of them, across the matrices) lie at least 1.5e-3 apart, in (0.05, 1)."""
    total = sum(int(np.prod(s)) for s in shapes)
    vals = 0.05 + 2e-3 * rng.permutation(total) + rng.uniform(0, 5e-4, total)
    assert vals.max() < 1
    out, at = [], 0
    for s in shapes:
        out.append(vals[at:at + int(np.prod(s))].reshape(s).astype(F32))
        at += int(np.prod(s))
    return out


KNN_SIZES = [(1, 1), (1, 6), (6, 1), (2, 3), (5, 7), (9, 4), (8, 8), (3, 11), (10, 10), (12, 5)]


def test_knn_matches_float64_restatement_and_conserves_mass():
    """50 seeded block matrices (1 x 1, non-square, k up to 5, sqrt with negative entries, one_way with a finite or an infinite Myy):
    tp / fp / fn / tn equal the restatement's counts; tp + fp + fn + tn = nx + ny (nx one way); acc = (tp + tn) / total."""
    from difffacto_amd import evaluation as ev
    rng = np.random.default_rng(11)
    seen_k, seen = set(), set()
    for case in range(50):
        nx, ny = KNN_SIZES[case % len(KNN_SIZES)]
        k = 1 if nx + ny == 2 else int(rng.integers(1, min(5, nx + ny - 1) + 1))
        # the flags walk through their four combinations once per pass over the sizes, shifted by one every pass: each size meets each
        sqrt, one_way = divmod((case + case // len(KNN_SIZES)) % 4, 2)
        sqrt, one_way = bool(sqrt), bool(one_way)
        seen.add((nx, ny, sqrt, one_way))
        Mxx, Mxy, Myy = _distinct(rng, (nx, nx), (nx, ny), (ny, ny))
        if sqrt:
            Mxy[rng.uniform(size=Mxy.shape) < 0.2] *= -1
            Mxx[rng.uniform(size=Mxx.shape) < 0.2] *= -1
        if one_way and rng.uniform() < 0.5:
            Myy[:] = np.inf
        seen_k.add(k)
        got = ev.knn(_t(Mxx), _t(Mxy), _t(Myy), k, sqrt=sqrt, one_way=one_way)
        want = gm.knn_vote(Mxx, Mxy, Myy, k, sqrt=sqrt, one_way=one_way)
        tag = (case, nx, ny, k, sqrt, one_way)
        for key in ("tp", "fp", "fn", "tn"):
            assert float(got[key]) == want[key], (tag, key, float(got[key]), want[key])
        total = nx if one_way else nx + ny
        counts = [float(got[key]) for key in ("tp", "fp", "fn", "tn")]
        assert sum(counts) == total, tag
        assert all(c == int(c) and c >= 0 for c in counts), tag
        assert abs(float(got["acc"]) - (counts[0] + counts[3]) / total) <= 2.0 ** -24, tag   # the float32 nearest the quotient
        assert abs(float(got["acc"]) - want["acc"]) <= 2.0 ** -24, tag
        for key in ("precision", "recall", "acc_t", "acc_f"):
            assert float(got[key]) == pytest.approx(want[key], rel=1e-6, abs=0), (tag, key)
    assert seen_k == {1, 2, 3, 4, 5}
    assert len(seen) == 4 * len(KNN_SIZES)   # every size with sqrt off / on and one_way off / on


MMD_SIZES = [(1, 1), (1, 5), (6, 1), (2, 3), (5, 7), (9, 4), (8, 8), (3, 11), (16, 10), (12, 5)]


def test_lgan_mmd_cov_matches_float64_restatement():
    """50 seeded matrices at thresholds above all, between two, exactly on one (the fold is a strict >) and below all of the
    references' closest distances: COV bit-equal to the restatement's count / N_ref, the two means within 1e-6 relative."""
    from difffacto_amd import evaluation as ev
    rng = np.random.default_rng(12)
    folds, seen = 0, set()
    for case in range(50):
        ns, nr = MMD_SIZES[case % len(MMD_SIZES)]
        which = (case + case // len(MMD_SIZES)) % 4   # shifted by one every pass over the sizes: each size meets each threshold
        seen.add((ns, nr, which))
        D, = _distinct(rng, (ns, nr))
        closest = np.sort(D.min(0))
        mid = float(closest[nr // 2])
        thresh = [1000, mid + 5e-4, mid, 0.0][which]
        got = ev.lgan_mmd_cov(_t(D), thresh=thresh)
        want = gm.mmd_cov(D, thresh=thresh)
        assert _f32(got["lgan_cov"]) == F32(want["lgan_cov"]), (case, ns, nr, thresh, float(got["lgan_cov"]), want["lgan_cov"])
        assert float(got["lgan_mmd"]) == pytest.approx(want["lgan_mmd"], rel=1e-6, abs=0), case
        assert float(got["lgan_mmd_smp"]) == pytest.approx(want["lgan_mmd_smp"], rel=1e-6, abs=0), case
        folds += want["lgan_cov"] != gm.mmd_cov(D)["lgan_cov"]
    assert folds >= 10   # the fold changed COV in many of the cases
    assert len(seen) == 4 * len(MMD_SIZES)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_fixture(name):
    """The float64 restatement against the reference itself: its Chamfer matrices from the recorded clouds and masks within the
    fixture's tolerance, and its metrics from the recorded matrices equal to the recorded result (means within 1e-6 relative)."""
    z = gm.load(f"all_metrics_{name}.npz")
    S, R = z["sample"], z["ref"]
    M = z["mask"] if "mask" in z.files else None
    tol = float(z["tol"])
    assert np.abs(gm.chamfer_matrix(R, S, None, M) - z["rs_cd"]).max() < tol
    assert np.abs(gm.chamfer_matrix(R, R) - z["rr_cd"]).max() < tol
    mats = {m: z[m] for m in gm.MATRICES if m in z.files}
    if name == "one_way":
        assert int(z["one_way"]) == 1 and "ss_cd" not in z.files
    else:
        assert np.abs(gm.chamfer_matrix(S, S, M, M) - z["ss_cd"]).max() < tol
    want = gm.result(z)
    got = gm.all_metrics(**mats)
    assert tuple(got) == gm.ALL_KEYS == tuple(want)
    for k in gm.ALL_KEYS:
        assert got[k] == pytest.approx(want[k], rel=1e-6, abs=0), k
    # the decision margins the generator asserted, on the recorded float32 matrices
    for d in ("cd", "emd"):
        block = gm.block_matrix(z[f"rr_{d}"], z[f"rs_{d}"], mats.get(f"ss_{d}", np.full((len(S),) * 2, np.inf)))
        gap = min(gm.column_gap(block[:, :len(R)] if name == "one_way" else block), gm.column_gap(z[f"rs_{d}"].T))
        assert gap >= 99 * tol and gap == pytest.approx(float(z[f"gap_{d}"]), abs=2 * tol), (d, gap)
    if name == "plain":
        for d in ("CD", "EMD"):
            vals = [want[f"1-NN-{d}-acc"], want[f"1-NN-{d}-acc_t"], want[f"1-NN-{d}-acc_f"], want[f"lgan_cov-{d}"]]
            assert all(0 < v < 1 for v in vals) and vals[1] != vals[2], (d, vals)
    # the EMD decisions differ from the CD ones, so a CD matrix left in an EMD line of compute_all_metrics cannot give these numbers
    assert want["lgan_cov-EMD"] != want["lgan_cov-CD"]
    if name != "one_way":   # one way every 1-NN key is 1 by definition
        assert any(want[f"1-NN-EMD-{k}"] != want[f"1-NN-CD-{k}"] for k in ("acc_t", "acc_f", "acc"))


def _check_result(got, want):
    """Counts (COV, acc) and lgan_mmd bit-equal; the ratios (+ 1e-10) and lgan_mmd_smp (summation order) within 1e-6 relative."""
    assert list(got) == list(want)
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and got[k].dim() == 0, k
        if k.endswith("acc_t") or k.endswith("acc_f") or "mmd_smp" in k:
            assert float(got[k]) == pytest.approx(v, rel=1e-6, abs=0), k
        else:
            assert float(got[k]) == v, (k, float(got[k]), v)


@pytest.mark.parametrize("name", FIXTURES)
def test_compute_all_metrics_wiring_on_recorded_matrices(monkeypatch, name):
    """compute_all_metrics with _pairwise_EMD_CD_ serving the recorded matrices: which pair of sets each call gets, which mask goes
    where, which matrix is transposed, the key names and their order, without a kernel."""
    from difffacto_amd import evaluation as ev
    z = gm.load(f"all_metrics_{name}.npz")
    S, R = _t(z["sample"]), _t(z["ref"])
    M = _t(z["mask"]) if "mask" in z.files else None
    one_way = bool(z["one_way"])
    calls = []

    def served(sample_pcs, ref_pcs, batch_size, accelerated_cd=True, verbose=False, mask_sample=None, mask_ref=None):
        tag = ("r" if sample_pcs is R else "s" if sample_pcs is S else "?") + ("r" if ref_pcs is R else "s" if ref_pcs is S else "?")
        masks = {"rs": (None, M), "rr": (None, None), "ss": (M, M)}[tag]
        assert mask_sample is masks[0] and mask_ref is masks[1], tag
        assert batch_size == 3
        calls.append(tag)
        return _t(z[f"{tag}_cd"]), _t(z[f"{tag}_emd"])
    monkeypatch.setattr(ev, "_pairwise_EMD_CD_", served)
    got = ev.compute_all_metrics(S, R, batch_size=3, one_way=one_way, mask=M)
    assert sorted(calls) == (["rr", "rs"] if one_way else ["rr", "rs", "ss"])
    _check_result(got, gm.result(z))


@pytest.fixture
def host_ev(monkeypatch):
    """The mirror with its two device calls replaced by the host stand-ins."""
    from difffacto_amd import evaluation as ev
    monkeypatch.setattr(ev, "distChamferCUDA", gm.cd_standin)
    monkeypatch.setattr(ev, "emd_approx", gm.emd_standin)
    return ev


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("launch", [1024, 4])
def test_pairwise_bookkeeping_reproduces_the_recorded_matrices(host_ev, monkeypatch, name, launch):
    """_pairwise_EMD_CD_'s own work (pair p = (p // N_ref, p % N_ref), the masked means, the reshape) on the host stand-ins: the
    matrices of every call within the fixture's tolerance, the result equal to the recorded one; 4 pairs per launch cut rows."""
    ev = host_ev
    z = gm.load(f"all_metrics_{name}.npz")
    S, R = _t(z["sample"]), _t(z["ref"])
    M = _t(z["mask"]) if "mask" in z.files else None
    tol = float(z["tol"])
    monkeypatch.setattr(ev, "PAIRS_PER_LAUNCH", launch)
    mats, orig = [], ev._pairwise_EMD_CD_

    def rec(*a, **k):
        out = orig(*a, **k)
        mats.append(out)
        return out
    monkeypatch.setattr(ev, "_pairwise_EMD_CD_", rec)
    got = ev.compute_all_metrics(S, R, batch_size=3, one_way=bool(z["one_way"]), mask=M)
    assert len(mats) == (2 if name == "one_way" else 3)
    for tag, (cd, emd) in zip(("rs", "rr", "ss"), mats):
        assert cd.shape == emd.shape == z[f"{tag}_cd"].shape
        assert np.abs(cd.numpy() - z[f"{tag}_cd"]).max() < tol, tag
        assert np.abs(emd.numpy() - z[f"{tag}_emd"]).max() < tol, tag
    want = gm.result(z)
    assert list(got) == list(want)
    for k, v in want.items():
        assert float(got[k]) == pytest.approx(v, rel=0, abs=tol if "mmd" in k else 1e-6), k


def test_pairwise_masks_weight_their_own_side(host_ev):
    """mask_sample alone and mask_ref alone against the restatement: a swap of the two, or a mask applied to the other direction,
    changes the Chamfer matrix by far more than the tolerance."""
    ev = host_ev
    z = gm.load("all_metrics_masked.npz")
    S, R, M = z["sample"], z["ref"], z["mask"]
    only_s = ev._pairwise_EMD_CD_(_t(S), _t(R), 3, mask_sample=_t(M))[0].numpy()
    only_r = ev._pairwise_EMD_CD_(_t(R), _t(S), 3, mask_ref=_t(M))[0].numpy()
    assert np.abs(only_s - gm.chamfer_matrix(S, R, M, None)).max() < 1e-6
    assert np.abs(only_r - gm.chamfer_matrix(R, S, None, M)).max() < 1e-6
    assert np.abs(only_s - only_r.T).max() < 1e-6
    assert np.abs(gm.chamfer_matrix(S, R, M, None) - gm.chamfer_matrix(S, R, None, None)).max() > 1e-3   # the mask matters here


def test_emd_cd_pairs_match_reference_fixture(host_ev):
    ev = host_ev
    z = gm.load("paired.npz")
    S, R = _t(z["sample"]), _t(z["ref"])
    for tag, reduced in (("reduced", True), ("full", False)):
        got = ev.EMD_CD(S, R, 4, reduced=reduced)
        assert list(got) == [str(k) for k in z[f"{tag}_keys"]] == ["MMD-CD", "MMD-EMD"]
        for k in got:
            assert got[k].shape == z[f"{tag}_{k}"].shape and np.abs(got[k].numpy() - z[f"{tag}_{k}"]).max() < 1e-6, (tag, k)


def test_part_weighted_fixture_is_consistent():
    """part_weighted.npz: the recorded matrices of every class give, through the restatement and clouds.npz's weights, the recorded
    part_weighted_* values; the keys left out are named with the reason, and only keys of a distance whose margin is too small."""
    z = gm.load("part_weighted.npz")
    w = np.load(os.path.join(gm.ROOT, "tests", "golden", "partmetrics", "clouds.npz"))["weights"]
    keys, left = [str(k) for k in z["keys"]], [str(k) for k in z["left_out"]]
    assert [str(k) for k in z["all_keys"]] == [f"part_weighted_{k}" for k in gm.ALL_KEYS]
    assert sorted(keys + left) == sorted(str(k) for k in z["all_keys"])
    tol = float(z["tol"])
    gaps = np.stack([z[f"gap_{j}"] for j in range(4)])
    for col, d in enumerate(("CD", "EMD")):
        short = gaps[:, col].min() < 100 * tol
        assert [k for k in left if k.endswith(f"-{d}") or f"-{d}-" in k] == \
            ([f"part_weighted_{k}" for k in gm.ALL_KEYS if "mmd" not in k and d in k] if short else [])
        assert (d in str(z["why_left_out"])) == short
    per_class = [gm.all_metrics(**{m: z[f"{m}_{j}"] for m in gm.MATRICES}) for j in range(4)]
    for k in keys:
        want = sum(w[j] * per_class[j][k[len("part_weighted_"):]] for j in range(4))
        assert float(z[f"res_{k}"]) == pytest.approx(want, rel=1e-6, abs=0), k


def test_gen_metrics_golden_manifest():
    sys.path.insert(0, os.path.join(gm.ROOT, "tests", "golden"))
    import manifest
    want = {}
    for line in open(os.path.join(gm.GM, "MANIFEST.sha256")):
        if line.strip() and not line.startswith("#"):
            h, name = line.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(gm.GM, f)) for f in sorted(os.listdir(gm.GM)) if f.endswith(".npz")}
    assert want == have
    assert sorted(have) == sorted([f"all_metrics_{n}.npz" for n in FIXTURES] + ["knn.npz", "mmdcov.npz", "paired.npz", "part_weighted.npz"])
    assert all(os.path.getsize(os.path.join(gm.GM, f)) < 1 << 20 for f in have)
