"""GPU checks of the part-level generation metrics (part_metrics.hip through difffacto_amd.evaluation) against the reference's
recorded values (tests/golden/partmetrics/, make_golden_partmetrics.py), numpy brute force and torch.quantile."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PM = os.path.join(ROOT, "tests", "golden", "partmetrics")


@pytest.fixture(scope="module")
def ev():
    from difffacto_amd import build
    build.build(verbose=False)
    from difffacto_amd import evaluation
    return evaluation


def _z(name):
    return np.load(os.path.join(PM, name))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("cls", ["Chair", "Airplane"])
def test_snapping_matches_reference(ev, cls):
    z = _z("snapping.npz")
    xyz, lab = _cuda(z["xyz"]), _cuda(z["labels"])
    for k in range(3):
        got = ev.compute_snapping_metric(xyz[k:k + 1], lab[k:k + 1], cls=cls)
        want = {key[len(f"{cls}_shape{k}_"):]: float(z[key]) for key in z.files if key.startswith(f"{cls}_shape{k}_")}
        assert list(got) == list(want)
        for key, v in want.items():
            assert abs(float(got[key]) - v) < 1e-6, (k, key, float(got[key]), v)
    got = ev.compute_snapping_metric(xyz, lab, cls=cls)
    want = {key[len(f"{cls}_mean_"):]: float(z[key]) for key in z.files if key.startswith(f"{cls}_mean_")}
    assert list(got) == list(want)
    for key, v in want.items():
        assert abs(float(got[key]) - v) < 1e-6, (key, float(got[key]), v)
    # the shape without part 1: pairs naming it are skipped (status 0)
    _, st = ev.part_snapping(xyz, lab, [(0, 1), (0, 2)])
    assert st[3].tolist() == [0, 1] and bool((st[:3] == 1).all())


def _snap_brute(x, l, a, b, k):
    A, B = x[l == a], x[l == b]
    if len(A) == 0 or len(B) == 0:
        return np.nan, 0
    if len(A) < k or len(B) < k:
        return np.nan, 2
    d = (A[:, None] - B[None]) ** 2
    d = (d[..., 0] + d[..., 1]) + d[..., 2]
    ia = np.lexsort((np.arange(len(A)), d.min(1)))[:k]
    ib = np.lexsort((np.arange(len(B)), d.min(0)))[:k]
    e = ((A[ia][:, None] - B[ib][None]) ** 2).sum(-1)
    return float(e.min(1).mean() + e.min(0).mean()), 1


@pytest.mark.parametrize("N", [64, 2048, 8192])
def test_snapping_against_brute_force(ev, N):
    rng = np.random.default_rng(N)
    B = 3
    x = rng.standard_normal((B, N, 3)).astype(np.float32)
    lab = rng.integers(0, 4, (B, N)).astype(np.int32)
    if N == 64:
        lab[:] = rng.choice([0, 1, 5], (B, N)).astype(np.int32)   # parts 0 / 1 have ~21 points: status 2; parts 2 / 3 absent
    else:
        lab[1][lab[1] == 2] = 3
        keep = np.flatnonzero(lab[1] == 3)[:49]
        lab[1][lab[1] == 3] = 0
        lab[1][keep] = 3                                          # shape 1: part 2 absent, part 3 has 49 points
    pairs = [(0, 1), (1, 2), (3, 0), (0, 0)]
    dist, st = ev.part_snapping(_cuda(x), _cuda(lab), pairs)
    dist, st = dist.cpu().numpy(), st.cpu().numpy()
    for b in range(B):
        for p, (i, j) in enumerate(pairs):
            want, ws = _snap_brute(x[b].astype(np.float32), lab[b], i, j, 50)
            assert st[b, p] == ws, (b, p, st[b, p], ws)
            if ws == 1:
                assert abs(dist[b, p] - want) <= 1e-6 * max(1.0, abs(want)), (b, p, dist[b, p], want)
    if N != 64:
        with pytest.raises(ValueError, match="shape 1"):
            ev.compute_snapping_metric(_cuda(x), _cuda(lab), cls="Chair")


@pytest.mark.parametrize("tag,q", [("q100", 1.0), ("q095", 0.95)])
def test_boxes_match_reference(ev, tag, q):
    z = _z("boxes.npz")
    for side in ("pred", "ref"):
        xyz, lab = _cuda(z[f"{side}s"]), _cuda(z[f"{side}s_mask"])
        boxes, count = ev.part_boxes(xyz, lab, 4, q)
        present = (count > 100).int().cpu().numpy()
        assert np.array_equal(present, z[f"{tag}_{side}_present"])
        got, want = boxes.cpu().numpy()[present == 1], z[f"{tag}_{side}_boxes"][present == 1]
        if q == 1.0:
            assert np.array_equal(got, want)
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
        assert np.isnan(boxes.cpu().numpy()[present == 0]).all()


def test_boxes_against_torch_quantile(ev):
    rng = np.random.default_rng(5)
    B, N = 4, 3000
    x = rng.standard_normal((B, N, 3)).astype(np.float32)
    lab = rng.integers(0, 6, (B, N)).astype(np.int32)
    for q in (0.95, 0.9, 0.5, 0.0, 1.0):
        for norm in (False, True):
            boxes, count = ev.part_boxes(_cuda(x), _cuda(lab), 4, q, normalize=norm, min_points=10)
            boxes, count = boxes.cpu(), count.cpu()
            for b in range(B):
                t = torch.from_numpy(x[b])
                if norm:
                    mx, mn = t.max(0)[0], t.min(0)[0]
                    t = (t - (mn + mx) / 2) / ((mx - mn).max() / 2)
                for j in range(4):
                    pts = t[torch.from_numpy(lab[b] == j)]
                    assert count[b, j] == len(pts)
                    lo, hi = torch.quantile(pts, 1 - q, dim=0), torch.quantile(pts, q, dim=0)
                    np.testing.assert_allclose(boxes[b, j, 0].numpy(), lo.numpy(), rtol=0, atol=1e-6)
                    np.testing.assert_allclose(boxes[b, j, 1].numpy(), hi.numpy(), rtol=0, atol=1e-6)


def test_part_clouds_match_reference(ev):
    z = _z("clouds.npz")
    P = ev._class_parts(*ev.part_clouds(_cuda(z["preds"]), _cuda(z["preds_mask"]), 4), 4)
    R = ev._class_parts(*ev.part_clouds(_cuda(z["refs"]), _cuda(z["refs_mask"]), 4), 4)
    for j in range(4):
        assert np.array_equal(P[j][0].cpu().numpy(), z[f"pred_{j}"]), j
        assert np.array_equal(P[j][1].cpu().numpy(), z[f"mask_{j}"]), j
        assert np.array_equal(R[j][0].cpu().numpy(), z[f"ref_{j}"]), j
    counts = [R[j][0].shape[0] for j in range(4)]
    assert np.array_equal(np.asarray([c / sum(counts) for c in counts], np.float32), z["weights"].astype(np.float32))   # recorded via fp32


def _boxset(ev, z, pre):
    return ev.BoxSet(_cuda(z[f"{pre}_boxes"]), _cuda(z[f"{pre}_present"]))


@pytest.mark.parametrize("tag", ["q100", "q095"])
@pytest.mark.parametrize("metric", ["l2", "iou"])
def test_l2_iou_matrices_and_dicts(ev, tag, metric):
    z = _z("boxes.npz")
    S, R = _boxset(ev, z, f"{tag}_pred"), _boxset(ev, z, f"{tag}_ref")
    for name, (X, Y) in (("rs", (R, S)), ("rr", (R, R)), ("ss", (S, S))):
        got, want = ev.box_pairwise(X, Y, metric).cpu().numpy(), z[f"{tag}_{metric}_{name}"].copy()
        if metric == "iou" and name != "rs":   # the reference's IoU of a box with itself can exceed 1 (see the CPU test)
            assert np.all(np.diag(got) == 0)
            np.fill_diagonal(want, 0)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=name)
    res = ev.compute_bbox_metric(_cuda(z["preds"]), _cuda(z["preds_mask"]), _cuda(z["refs"]), _cuda(z["refs_mask"]), 32,
                                 thresh=1.0 if tag == "q100" else 0.95, metric=metric)
    want = {k[len(f"{tag}_{metric}_res_"):]: float(z[k]) for k in z.files if k.startswith(f"{tag}_{metric}_res_")}
    assert list(res) == list(want)
    for k, v in want.items():
        assert float(res[k]) == pytest.approx(v, rel=1e-6, abs=1e-6), k


def test_chamfer_replay_matches_reference(ev):
    z = _z("chamfer.npz")
    S, R = _boxset(ev, z, "pred"), _boxset(ev, z, "ref")
    for name, (X, Y) in (("rs", (R, S)), ("rr", (R, R)), ("ss", (S, S))):
        got = ev.box_pairwise(X, Y, "chamfer", units=_cuda(z[f"units_{name}"])).cpu().numpy()
        np.testing.assert_allclose(got, z[name], rtol=0, atol=1e-6, err_msg=name)


def test_chamfer_philox_stream(ev):
    from difffacto_amd import _ffi
    rng = np.random.default_rng(3)
    M, C = 6, 4
    lo = rng.uniform(-1, 0, (M, C, 1, 3)).astype(np.float32)
    boxes = np.concatenate([lo, lo + rng.uniform(0.2, 1, (M, C, 1, 3)).astype(np.float32)], 2)
    present = np.ones((M, C), np.int32)
    present[1, 2] = present[4, 2] = 0
    A = ev.BoxSet(_cuda(boxes), _cuda(present))
    full = ev.box_pairwise(A, A, "chamfer", seed=11)
    top = ev.box_pairwise(ev.BoxSet(A.boxes[:2], A.present[:2]), A, "chamfer", seed=11, row0=0)
    bot = ev.box_pairwise(ev.BoxSet(A.boxes[2:], A.present[2:]), A, "chamfer", seed=11, row0=2)
    assert torch.equal(full, torch.cat([top, bot]))
    assert not torch.equal(full, ev.box_pairwise(A, A, "chamfer", seed=12))
    # the stream's own draws replayed through `units` give the same matrix
    units = torch.empty(M * M, C, 2, 512, 3, device="cuda")
    _ffi.check(_ffi.lib().dfx_debug_part_box_units(11, 0, M * M, C, _ffi.ptr(units), _ffi.current_stream()), "units")
    assert torch.equal(full, ev.box_pairwise(A, A, "chamfer", units=units))
    assert float(units.min()) >= 0 and float(units.max()) < 1
    # 4096 comparisons of two identical unit boxes: mean within 1 % of torch.rand draws through the replay path
    one = ev.BoxSet(_cuda(np.array([[[[0, 0, 0], [1, 1, 1]]]], np.float32)).expand(64, 1, 2, 3).contiguous(),
                    torch.ones(64, 1, dtype=torch.int32, device="cuda"))
    ph = float(ev.box_pairwise(one, one, "chamfer", seed=5).mean())
    g = torch.Generator().manual_seed(0)
    rp = float(ev.box_pairwise(one, one, "chamfer", units=torch.rand(4096, 1, 2, 512, 3, generator=g).cuda()).mean())
    assert abs(ph / rp - 1) < 0.01, (ph, rp)


def test_evaluate_gen_part_equals_merged_mirrors(ev):
    rng = np.random.default_rng(9)
    # two batches of forward dicts with 2500 points per shape (FPS down to 2048), four parts of 625 points
    lab = torch.from_numpy(np.repeat(np.arange(4), 625)[None].repeat(2, 0).astype(np.int64))
    centre = torch.from_numpy(np.asarray([[0, 0, 0], [0, .5, 0], [.5, 0, 0], [0, -.5, 0]], np.float32))[lab]
    results = []
    for _ in range(2):
        pred = torch.from_numpy(rng.standard_normal((2, 2500, 3)).astype(np.float32)) * 0.1 + centre
        ref = torch.from_numpy(rng.standard_normal((2, 2500, 3)).astype(np.float32)) * 0.1 + centre
        results.append(dict(pred=pred, pred_seg_mask=lab, input_ref=ref.flip(1), ref_seg_mask=lab.flip(1)))
    got = ev.evaluate_gen_part(results, "Chair", seed=4)
    p, pmk, r, rmk = ev.gen_part_inputs(results)
    assert p.shape == r.shape == (4, 2048, 3)
    want = ev.compute_all_metrics(p, r, 32)
    want.update(ev.compute_snapping_metric(p, pmk, cls="Chair"))
    want.update({f"oracle_{k}": v for k, v in ev.compute_snapping_metric(r, rmk, cls="Chair").items()})
    want.update(ev.compute_part_metric(p, pmk, r, rmk, 32))
    want.update(ev.compute_bbox_metric(p, pmk, r, rmk, 32, metric="chamfer", seed=4))
    keys = [f"{k}-{d}" for d in ("CD", "EMD") for k in ("lgan_mmd", "lgan_cov", "lgan_mmd_smp")]
    keys += [f"1-NN-{d}-{k}" for d in ("CD", "EMD") for k in ("acc_t", "acc_f", "acc")]
    keys += [f"snapping_Chair_{i}" for i in (0, 1, 3)] + [f"oracle_snapping_Chair_{i}" for i in (0, 1, 3)]
    keys += [f"part_weighted_{k}" for k in keys[:12]]
    keys += [f"bbox_{k}-bbox_chamfer" for k in ("lgan_mmd", "lgan_cov", "lgan_mmd_smp")]
    keys += [f"bbox_1-NN-bbox_chamfer-{k}" for k in ("acc_t", "acc_f", "acc")]
    assert list(got) == keys == list(want)
    for k in keys:
        assert torch.equal(torch.as_tensor(got[k]).cpu(), torch.as_tensor(want[k]).cpu()), k
