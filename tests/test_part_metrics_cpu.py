"""CPU checks of the part-level generation metrics: the dfx_part_* entry points are exported and bound and reject bad arguments before
touching a GPU; the mirror's ValueErrors; the host part_l2 / part_miou, lgan_mmd_cov_match and the generic-callable path of
compute_all_metrics_cust_func against the reference's recorded values (tests/golden/partmetrics/, make_golden_partmetrics.py); the
fixtures' manifest."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PM = os.path.join(ROOT, "tests", "golden", "partmetrics")
NEW = ("dfx_part_snapping_f32", "dfx_part_boxes_f32", "dfx_part_clouds_f32", "dfx_part_box_pairwise_f32", "dfx_debug_part_box_units")


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_part_metric_symbols_are_exported_and_bound(L):
    from difffacto_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert L.dfx_version() >= 102 and L.dfx_abi_version() == 5


FAKE = ctypes.c_void_p(0x1000)   # a non-null "device pointer": never dereferenced, the checks fail first


def _err(L, rc):
    return rc, (L.dfx_last_error() or b"").decode()


def _snap(L, xyz=FAKE, lab=FAKE, B=2, N=64, C=4, pairs=((0, 1), (1, 2)), k=50, dist=FAKE, status=FAKE):
    pr = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    hp = None if pr is None else pr.ctypes.data_as(ctypes.c_void_p)
    return _err(L, L.dfx_part_snapping_f32(xyz, lab, B, N, C, hp, 0 if pr is None else len(pr), k, dist, status, None))


def test_snapping_rejects_bad_arguments_without_a_gpu(L):
    for kw, msg in [(dict(xyz=None), "null"), (dict(lab=None), "null"), (dict(dist=None), "null"), (dict(status=None), "null"),
                    (dict(pairs=None), "null"), (dict(B=0), "positive"), (dict(N=0), "positive"), (dict(C=0), "positive"),
                    (dict(k=0), "positive"), (dict(k=-3), "positive"), (dict(N=8193), "above"), (dict(pairs=((0, 4),)), "outside"),
                    (dict(pairs=((-1, 2),)), "outside")]:
        rc, m = _snap(L, **kw)
        assert rc == -1 and msg in m, (kw, rc, m)


def test_boxes_clouds_pairwise_reject_bad_arguments_without_a_gpu(L):
    def boxes(xyz=FAKE, B=2, N=64, C=4, q=0.95, out=FAKE, mp=100):
        return _err(L, L.dfx_part_boxes_f32(xyz, FAKE, B, N, C, 1, mp, q, out, FAKE, None))
    for kw, msg in [(dict(xyz=None), "null"), (dict(out=None), "null"), (dict(B=0), "positive"), (dict(N=-1), "positive"),
                    (dict(C=0), "positive"), (dict(N=9000), "above"), (dict(q=1.5), "outside"), (dict(q=-0.1), "outside"),
                    (dict(mp=-1), "negative")]:
        rc, m = boxes(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)

    def clouds(xyz=FAKE, B=2, N=64, C=4, n_out=512, out=FAKE):
        return _err(L, L.dfx_part_clouds_f32(xyz, FAKE, B, N, C, 100, n_out, out, FAKE, FAKE, None))
    for kw, msg in [(dict(xyz=None), "null"), (dict(out=None), "null"), (dict(B=0), "positive"), (dict(C=-2), "positive"),
                    (dict(N=8193), "above"), (dict(n_out=0), "n_out")]:
        rc, m = clouds(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)

    def pw(a=FAKE, Ma=2, Mb=3, C=4, metric=0, D=FAKE, row0=0):
        return _err(L, L.dfx_part_box_pairwise_f32(a, FAKE, Ma, FAKE, FAKE, Mb, C, metric, 1, row0, None, D, None))
    for kw, msg in [(dict(a=None), "null"), (dict(D=None), "null"), (dict(Ma=0), "positive"), (dict(Mb=0), "positive"),
                    (dict(C=0), "positive"), (dict(metric=3), "unknown metric"), (dict(metric=-1), "unknown metric"),
                    (dict(row0=-1), "negative")]:
        rc, m = pw(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)


def test_mirror_raises_value_error_for_unknown_class_and_metric():
    from difffacto_amd import evaluation as ev
    x, m = torch.zeros(1, 64, 3), torch.zeros(1, 64, dtype=torch.int32)
    with pytest.raises(ValueError, match="Car"):
        ev.compute_snapping_metric(x, m, cls="Car")
    with pytest.raises(ValueError, match="emd"):
        ev.compute_bbox_metric(x, m, x, m, 32, metric="emd")
    with pytest.raises(ValueError, match="emd"):
        ev.box_pairwise(None, None, metric="emd")


def _dicts(boxes, present):
    return [{c: (torch.from_numpy(boxes[m, c, 0][None].copy()), torch.from_numpy(boxes[m, c, 1][None].copy()))
             for c in range(boxes.shape[1]) if present[m, c]} for m in range(len(boxes))]


def _matrices(func, n_class, S, R):
    rs = np.array([[float(func(n_class, R[i], S[j]).reshape(-1)[0]) for j in range(len(S))] for i in range(len(R))], np.float32)
    rr = np.array([[float(func(n_class, R[i], R[j]).reshape(-1)[0]) for j in range(len(R))] for i in range(len(R))], np.float32)
    ss = np.array([[float(func(n_class, S[i], S[j]).reshape(-1)[0]) for j in range(len(S))] for i in range(len(S))], np.float32)
    return rs, rr, ss


@pytest.mark.parametrize("tag", ["q100", "q095"])
@pytest.mark.parametrize("metric", ["l2", "iou"])
def test_host_pair_distances_match_reference(tag, metric):
    from difffacto_amd import evaluation as ev
    z = np.load(os.path.join(PM, "boxes.npz"))
    S, R = _dicts(z[f"{tag}_pred_boxes"], z[f"{tag}_pred_present"]), _dicts(z[f"{tag}_ref_boxes"], z[f"{tag}_ref_present"])
    # the fixture's boxes are anisotropic: a "fixed" (x, y, z) reading of get_3d_box's (l, w, h) gives other IoUs
    b = z[f"{tag}_pred_boxes"][z[f"{tag}_pred_present"] == 1]
    assert np.abs((b[:, 1, 1] - b[:, 0, 1]) - (b[:, 1, 2] - b[:, 0, 2])).max() > 0.1
    func = ev.part_l2 if metric == "l2" else ev.part_miou
    for name, got in zip(("rs", "rr", "ss"), _matrices(func, 4, S, R)):
        want = z[f"{tag}_{metric}_{name}"].copy()
        if metric == "iou" and name != "rs":
            # a box against itself: the reference's polygon clipping can return more than the box (IoU above 1); knn masks the diagonal
            assert np.all(np.diag(got) == 0)
            np.fill_diagonal(want, 0)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=f"{tag} {metric} {name}")


def test_host_miou_axis_reading():
    """One box against its copy shifted by half its y-extent along y: the reference reads the y-extent as dz, so the overlap is
    1 - dy / (2 dz) of the box, not 1/2."""
    from difffacto_amd import evaluation as ev
    lo, hi = torch.tensor([[0.0, 0.0, 0.0]]), torch.tensor([[1.0, 0.4, 2.0]])
    sh = torch.tensor([[0.0, 0.2, 0.0]])
    d = float(ev.part_miou(1, {0: (lo, hi)}, {0: (lo + sh, hi + sh)}))
    ov = 1 - 0.2 / 2.0
    assert abs(d - (1 - ov / (2 - ov))) < 1e-6


def test_lgan_mmd_cov_match_and_generic_callable_against_reference():
    from difffacto_amd import evaluation as ev
    z = np.load(os.path.join(PM, "boxes.npz"))
    rs = torch.from_numpy(z["q100_l2_rs"])
    res, idx = ev.lgan_mmd_cov_match(rs.t())
    dist = rs.t()
    assert torch.equal(idx, dist.min(1)[1])
    assert float(res["lgan_cov"]) == pytest.approx(len(set(idx.tolist())) / dist.shape[1])
    assert float(res["lgan_mmd"]) == pytest.approx(float(dist.min(0)[0].mean()))
    # the pair-loop path with a callable the native path does not know: the reference's final dict
    S, R = _dicts(z["q100_pred_boxes"], z["q100_pred_present"]), _dicts(z["q100_ref_boxes"], z["q100_ref_present"])
    func = lambda A, B, accelerated=False: ev.part_l2(4, A, B)  # noqa: E731
    got = ev.compute_all_metrics_cust_func(S, R, func, "bbox_l2", accelerated_cd=True, thresh=100)
    want = {k[len("q100_l2_res_bbox_"):]: float(z[k]) for k in z.files if k.startswith("q100_l2_res_")}
    assert set(got) == set(want)
    for k, v in want.items():
        assert float(got[k]) == pytest.approx(v, rel=1e-6, abs=1e-7), k


def test_part_metrics_golden_manifest():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import manifest
    want = {}
    for line in open(os.path.join(PM, "MANIFEST.sha256")):
        if line.strip() and not line.startswith("#"):
            h, name = line.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(PM, f)) for f in sorted(os.listdir(PM)) if f.endswith(".npz")}
    assert want == have
    assert all(os.path.getsize(os.path.join(PM, f)) < 1 << 20 for f in have)
