"""GPU: the generation metrics (MMD / COV / 1-NNA under CD and EMD, python/difffacto/datasets/evaluation_utils.py) on the
native Chamfer / EMD kernels vs a brute-force numpy evaluation with the C oracle's EMD."""
import os

import numpy as np
import pytest
import torch

import _genmetrics_case as gm

pytestmark = pytest.mark.gpu


def _brute(sample, ref):
    from oracle import pointnet2 as o
    cd = np.zeros((len(sample), len(ref)), np.float32)
    emd = np.zeros_like(cd)
    for i, a in enumerate(sample):
        for j, b in enumerate(ref):
            d = ((a[:, None] - b[None]) ** 2).sum(-1)
            cd[i, j] = d.min(1).mean() + d.min(0).mean()
            dist, _ = o.emd_forward(a[None], b[None], 0.002, 10000)
            emd[i, j] = np.sqrt(dist).mean()
    return cd, emd


def test_pairwise_and_all_metrics_vs_bruteforce():
    from difffacto_amd import evaluation as ev
    rng = np.random.Generator(np.random.PCG64(2))
    ref = rng.uniform(0, 1, (4, 128, 3)).astype(np.float32)
    smp = np.concatenate([ref[:2] + 0.01 * rng.standard_normal((2, 128, 3)).astype(np.float32), rng.uniform(0, 1, (3, 128, 3)).astype(np.float32)])
    smp = np.clip(smp, 0, 1)
    S, R = torch.from_numpy(smp).cuda(), torch.from_numpy(ref).cuda()
    cd, emd = ev._pairwise_EMD_CD_(S, R, batch_size=3)
    cd_ref, emd_ref = _brute(smp, ref)
    assert np.abs(cd.cpu().numpy() - cd_ref).max() < 1e-6
    assert np.abs(emd.cpu().numpy() - emd_ref).max() < 1e-6
    paired = ev.EMD_CD(S[:4], R, batch_size=3, reduced=False)
    assert np.abs(paired["MMD-CD"].cpu().numpy() - np.diag(cd_ref[:4])).max() < 1e-6
    assert np.abs(paired["MMD-EMD"].cpu().numpy() - np.diag(emd_ref[:4])).max() < 1e-6
    res = ev.compute_all_metrics(S, R, batch_size=3)
    # the two perturbed copies are the closest samples of references 0 and 1
    assert abs(float(res["lgan_mmd-CD"]) - cd_ref.min(0).mean()) < 1e-6
    emd_rs = _brute(ref, smp)[1]   # the auction is not symmetric: compute_all_metrics bids references against samples (:504)
    assert abs(float(res["lgan_mmd_smp-EMD"]) - emd_rs.T.min(1).mean()) < 1e-6
    assert float(res["lgan_cov-CD"]) == len(set(cd_ref.argmin(0).tolist())) / 4
    for k in ("1-NN-CD-acc", "1-NN-EMD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f"):
        assert 0.0 <= float(res[k]) <= 1.0
    # 1-NNA on two identical sets: every cloud's nearest neighbour (leave-one-out) is its twin in the other set -> accuracy 0
    res_same = ev.compute_all_metrics(R.clone(), R, batch_size=4)
    assert float(res_same["1-NN-CD-acc"]) == 0.0 and float(res_same["lgan_cov-CD"]) == 1.0 and float(res_same["lgan_mmd-CD"]) == 0.0


def test_pairwise_launch_size_does_not_change_the_matrices(monkeypatch):
    """The all-pairs matrices go to the kernels PAIRS_PER_LAUNCH pairs at a time: any launch size gives the same numbers (masks too)."""
    from difffacto_amd import evaluation as ev
    g = torch.Generator(device="cuda").manual_seed(5)
    S, R = torch.rand(5, 96, 3, device="cuda", generator=g), torch.rand(7, 96, 3, device="cuda", generator=g)
    ms, mr = (torch.rand(5, 96, device="cuda", generator=g) > 0.3).float(), (torch.rand(7, 96, device="cuda", generator=g) > 0.3).float()
    whole = ev._pairwise_EMD_CD_(S, R, batch_size=32, mask_sample=ms, mask_ref=mr)
    monkeypatch.setattr(ev, "PAIRS_PER_LAUNCH", 1)
    for bs in (1, 4, 9):
        part = ev._pairwise_EMD_CD_(S, R, batch_size=bs, mask_sample=ms, mask_ref=mr)
        assert torch.equal(part[1], whole[1])                       # the auction: bit-identical per pair
        assert torch.allclose(part[0], whole[0], rtol=1e-6, atol=0)   # Chamfer means: torch reductions
    paired = ev.EMD_CD(S, R[:5], batch_size=2, reduced=False)
    assert torch.equal(paired["MMD-EMD"], torch.diagonal(ev._pairwise_EMD_CD_(S, R[:5], batch_size=2)[1]))


# ---------------------------------------------------------------------------------------------------------------------
# Against the reference's own metric functions (tests/golden/genmetrics/, make_golden_genmetrics.py: the reference's
# compute_all_metrics / EMD_CD / compute_part_metric with a float64 brute-force Chamfer and the C oracle's auction in place of its two
# CUDA extensions) and the float64 restatement of tests/_genmetrics_case.py.  The fixtures' argmin decisions have margins of at least
# 100 x the matrix tolerance, so COV and 1-NNA cannot flip on rounding.
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _recording(monkeypatch, ev):
    """Every (cd, emd) that _pairwise_EMD_CD_ returns from here on, in call order."""
    mats, orig = [], ev._pairwise_EMD_CD_

    def rec(*a, **k):
        out = orig(*a, **k)
        mats.append(out)
        return out
    monkeypatch.setattr(ev, "_pairwise_EMD_CD_", rec)
    return mats


def _fixture_inputs(z):
    return _cuda(z["sample"]), _cuda(z["ref"]), (_cuda(z["mask"]) if "mask" in z.files else None), bool(z["one_way"])


def _check_all_metrics(got, want, tol):
    """lgan_cov-* and the 1-NN-* keys within 1e-6, the mmd keys within the matrix tolerance; names and order as recorded."""
    assert list(got) == list(want)
    for k, v in want.items():
        assert abs(float(got[k]) - v) < (tol if "mmd" in k else 1e-6), (k, float(got[k]), v)


@pytest.mark.parametrize("name", ["plain", "masked", "one_way"])
def test_all_metrics_match_the_reference(monkeypatch, name):
    """compute_all_metrics on the device against the reference's: the matrices of every _pairwise_EMD_CD_ call within the fixture's
    tolerance (1e-6 absolute, unit-cube clouds of 64 points), then every key of the result."""
    from difffacto_amd import evaluation as ev
    z = gm.load(f"all_metrics_{name}.npz")
    S, R, M, one_way = _fixture_inputs(z)
    tol = float(z["tol"])
    mats = _recording(monkeypatch, ev)
    got = ev.compute_all_metrics(S, R, batch_size=3, one_way=one_way, mask=M)
    assert len(mats) == (2 if one_way else 3)
    worst = {}
    for tag, (cd, emd) in zip(("rs", "rr", "ss"), mats):
        assert cd.shape == emd.shape == z[f"{tag}_cd"].shape
        worst[f"{tag}_cd"] = float(np.abs(cd.cpu().numpy() - z[f"{tag}_cd"]).max())
        worst[f"{tag}_emd"] = float(np.abs(emd.cpu().numpy() - z[f"{tag}_emd"]).max())
    print(f"\nall_metrics_{name}: worst matrix error " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (tolerance {tol:g})")
    assert max(worst.values()) < tol, worst
    _check_all_metrics(got, gm.result(z), tol)


def test_masks_weight_their_own_side_on_the_device():
    """mask_sample alone and mask_ref alone: the Chamfer matrix against the float64 restatement, so that a swap of the two masks (or
    a mask on the other direction) fails; the mask changes the entries by more than 1e-3 here."""
    from difffacto_amd import evaluation as ev
    z = gm.load("all_metrics_masked.npz")
    S, R, M = z["sample"], z["ref"], z["mask"]
    only_s = ev._pairwise_EMD_CD_(_cuda(S), _cuda(R), 3, mask_sample=_cuda(M))[0].cpu().numpy()
    only_r = ev._pairwise_EMD_CD_(_cuda(R), _cuda(S), 3, mask_ref=_cuda(M))[0].cpu().numpy()
    want = gm.chamfer_matrix(S, R, M, None)
    assert np.abs(want - gm.chamfer_matrix(S, R, None, M[:len(R)])).max() > 1e-3 and np.abs(want - gm.chamfer_matrix(S, R)).max() > 1e-3
    assert np.abs(only_s - want).max() < 1e-6
    assert np.abs(only_r - gm.chamfer_matrix(R, S, None, M)).max() < 1e-6


def test_paired_emd_cd_matches_the_reference(monkeypatch):
    """EMD_CD against the reference's on 6 pairs, reduced and not.  batch_size only matters below PAIRS_PER_LAUNCH, so the comparison
    of batch_size 4 and 1 is made with one pair per launch: 4 cuts the six pairs into 4 + 2, 1 into six launches, and both give the
    single launch's numbers (the auction bit for bit, the Chamfer means as far as torch's reductions promise)."""
    from difffacto_amd import evaluation as ev
    z = gm.load("paired.npz")
    S, R = _cuda(z["sample"]), _cuda(z["ref"])
    for tag, reduced in (("reduced", True), ("full", False)):
        got = ev.EMD_CD(S, R, 4, reduced=reduced)
        assert list(got) == [str(k) for k in z[f"{tag}_keys"]]
        for k in got:
            err = float(np.abs(got[k].cpu().numpy() - z[f"{tag}_{k}"]).max())
            print(f"\npaired {tag} {k}: error {err:.3g} (tolerance 1e-06)")
            assert got[k].shape == z[f"{tag}_{k}"].shape and err < 1e-6, (tag, k, err)
        with monkeypatch.context() as m:
            m.setattr(ev, "PAIRS_PER_LAUNCH", 1)
            for bs in (4, 1):
                cut = ev.EMD_CD(S, R, bs, reduced=reduced)
                if not reduced:
                    assert torch.equal(cut["MMD-EMD"], got["MMD-EMD"])
                assert all(torch.allclose(cut[k], got[k], rtol=1e-6, atol=0) for k in got)


def test_part_metric_matches_the_reference(monkeypatch):
    """compute_part_metric end to end against the reference's on partmetrics/clouds.npz's inputs: the six matrices of every class
    within 1e-6 and the part_weighted_* keys part_weighted.npz holds.  Left out there, for the reason it records: the keys that count
    decisions under EMD (part_weighted_lgan_cov-EMD, part_weighted_1-NN-EMD-*), because class 2's smallest EMD decision margin on these
    inputs (5.8e-5) is below 100 x the matrix tolerance."""
    from difffacto_amd import evaluation as ev
    z = gm.load("part_weighted.npz")
    c = np.load(os.path.join(gm.ROOT, "tests", "golden", "partmetrics", "clouds.npz"))
    tol = float(z["tol"])
    mats = _recording(monkeypatch, ev)
    got = ev.compute_part_metric(_cuda(c["preds"]), _cuda(c["preds_mask"]), _cuda(c["refs"]), _cuda(c["refs_mask"]), 32, n_class=4)
    assert len(mats) == 12 and list(got) == [str(k) for k in z["all_keys"]]
    worst = 0.0
    for j in range(4):
        for tag, (cd, emd) in zip(("rs", "rr", "ss"), mats[3 * j:3 * j + 3]):
            worst = max(worst, float(np.abs(cd.cpu().numpy() - z[f"{tag}_cd_{j}"]).max()), float(np.abs(emd.cpu().numpy() - z[f"{tag}_emd_{j}"]).max()))
    print(f"\npart_weighted: worst matrix error {worst:.3g} (tolerance {tol:g})")
    assert worst < tol
    keys = [str(k) for k in z["keys"]]
    assert len(keys) == 8 and [str(k) for k in z["left_out"]] == [f"part_weighted_{k}" for k in gm.ALL_KEYS if "EMD" in k and "mmd" not in k]
    for k in keys:
        assert abs(float(got[k]) - float(z[f"res_{k}"])) < (tol if "mmd" in k else 1e-6), (k, float(got[k]), float(z[f"res_{k}"]))


def test_all_metrics_do_not_depend_on_the_input_layout():
    """Non-contiguous views of the same clouds and mask (a slice along the point axis, a slice of padded coordinates, every other
    mask column of a wider tensor) give the numbers of the contiguous copies."""
    from difffacto_amd import evaluation as ev
    z = gm.load("all_metrics_masked.npz")
    S, R, M, _ = _fixture_inputs(z)
    want = ev.compute_all_metrics(S, R, batch_size=3, mask=M)
    big_s = torch.full((S.shape[0], 2 * S.shape[1], 3), 0.5, device="cuda")
    big_s[:, 32:96] = S
    big_r = torch.full((R.shape[0], R.shape[1], 4), 0.25, device="cuda")
    big_r[..., :3] = R
    big_m = torch.ones(M.shape[0], 2 * M.shape[1], device="cuda")
    big_m[:, ::2] = M
    Sv, Rv, Mv = big_s[:, 32:96], big_r[..., :3], big_m[:, ::2]
    assert not Sv.is_contiguous() and not Rv.is_contiguous() and not Mv.is_contiguous()
    got = ev.compute_all_metrics(Sv, Rv, batch_size=3, mask=Mv)
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))
    _check_all_metrics(got, gm.result(z), float(z["tol"]))


def test_pairwise_across_the_default_launch_size():
    """33 x 32 clouds of 32 points are 1056 pairs: the default PAIRS_PER_LAUNCH = 1024 ends in the middle of the last row.  Chamfer
    against the float64 restatement within 1e-6; the auction equal to the same call on the two halves of the sample set (one launch
    each)."""
    from difffacto_amd import evaluation as ev
    assert ev.PAIRS_PER_LAUNCH == 1024
    rng = np.random.default_rng(33)
    S, R = rng.uniform(0, 1, (33, 32, 3)).astype(np.float32), rng.uniform(0, 1, (32, 32, 3)).astype(np.float32)
    Sd, Rd = _cuda(S), _cuda(R)
    cd, emd = ev._pairwise_EMD_CD_(Sd, Rd, batch_size=32)
    assert cd.shape == emd.shape == (33, 32)
    err = float(np.abs(cd.cpu().numpy() - gm.chamfer_matrix(S, R)).max())
    print(f"\n33 x 32 pairs: worst Chamfer error {err:.3g} (tolerance 1e-06)")
    assert err < 1e-6
    top, bottom = ev._pairwise_EMD_CD_(Sd[:17], Rd, batch_size=32), ev._pairwise_EMD_CD_(Sd[17:], Rd, batch_size=32)
    assert torch.equal(emd, torch.cat([top[1], bottom[1]]))
    assert torch.allclose(cd, torch.cat([top[0], bottom[0]]), rtol=1e-6, atol=0)
    assert float(emd.min()) > 0
