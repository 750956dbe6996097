"""GPU checks of the occupancy-grid JSD (occupancy.hip through difffacto_amd.evaluation): exact equality with the reference's recorded
cells and counters (tests/golden/jsd/, make_golden_jsd.py), a numpy float64 brute force over all kept cells with the lower-index tie
rule, the labelled rows, chunked accumulation, reproducibility and the non-finite convention."""
import numpy as np
import pytest
import torch

import _jsd_case as jc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ev():
    from difffacto_amd import build
    build.build(verbose=False)
    from difffacto_amd import evaluation
    return evaluation


@pytest.fixture(scope="module")
def clouds():
    return jc.load_clouds()


def _np(t):
    return t.cpu().numpy()


def _grid(ev, x, R, sphere, labels=None, n_class=0, out=None):
    c, b, i, bad = ev.occupancy_grid(torch.from_numpy(np.ascontiguousarray(x)).cuda(), None if labels is None else torch.from_numpy(labels).cuda(),
                                     n_class, R, sphere, return_index=True, out=out)
    return c, b, i, bad


@pytest.mark.parametrize("R,sphere", jc.CASES)
def test_cells_and_counters_equal_reference(ev, clouds, R, sphere):
    z = jc.load_case(R, sphere)
    dev = {}
    for name, pcs in clouds.items():
        c, b, i, bad = _grid(ev, pcs, R, sphere)
        dev[name] = c
        assert int(bad) == 0 and c.dtype == torch.int64 and b.dtype == torch.int32 and c.shape == (1, int(z["cells"]))
        assert np.array_equal(_np(i), z[f"index_{name}"])
        assert np.array_equal(_np(c[0]), z[f"counters_{name}"].astype(np.int64))
        assert np.array_equal(_np(b[0]), z[f"bernoulli_{name}"])
        ent, counters = ev.entropy_of_occupancy_grid(pcs, R, sphere)
        assert type(ent).__name__ == str(z[f"type_entropy_{name}"])
        assert f"{type(counters).__name__}:{counters.dtype}" == str(z[f"type_counters_{name}"])
        assert np.array_equal(counters, z[f"counters_{name}"])
        assert abs(ent - float(z[f"entropy_{name}"])) < 1e-11, (ent, float(z[f"entropy_{name}"]))
    jab = ev.jensen_shannon_divergence(dev["a"][0], dev["b"][0])
    assert type(jab).__name__ == str(z["type_jsd"])
    assert abs(jab - float(z["jsd_ab"])) < 1e-11, (jab, float(z["jsd_ab"]))
    assert ev.jensen_shannon_divergence(dev["a"][0], dev["a"][0]) == 0.0
    if sphere:
        got = ev.jsd_between_point_cloud_sets(clouds["a"], torch.from_numpy(clouds["b"]), R)
        assert type(got).__name__ == str(z["type_jsd"]) and abs(got - float(z["jsd_ab"])) < 1e-11
        assert ev.jsd_between_point_cloud_sets(clouds["a"], clouds["a"], R) == 0.0


def _special_points(rng, R, n):
    """Cell centres, midpoints of two and of eight cells (exact ties), points at distance 1e3."""
    a = jc.grid_axis(R)
    ii, jj, ax = rng.integers(0, R, (n, 3)), rng.integers(0, R - 1, (n, 3)), rng.integers(0, 3, n)
    mid8 = (a[jj].astype(np.float64) + a[jj + 1]) / 2
    mid2 = a[ii].astype(np.float64)
    mid2[np.arange(n), ax] = mid8[np.arange(n), ax]
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([a[ii], mid2, mid8, 1e3 * d]).astype(np.float32)


@pytest.mark.parametrize("R,sphere,B,N", [(2, False, 1, 1), (28, True, 1, 1), (2, False, 3, 65), (3, True, 3, 63), (3, False, 3, 65),
                                          (28, True, 3, 63), (28, False, 3, 65), (28, True, 3, 2048), (28, False, 3, 2048),
                                          (40, True, 3, 65), (40, False, 3, 63), (40, True, 3, 2048)])
def test_against_float64_brute_force(ev, R, sphere, B, N):
    rng = np.random.default_rng(1000 * R + 10 * N + sphere)
    x = jc.mixed_points(rng, B * N).reshape(B, N, 3)
    if N >= 63:   # sixteen points of each cloud: centres, ties, far points
        for b in range(B):
            x[b, :16] = _special_points(rng, R, 4)
    want = jc.brute_force(x, R, sphere).reshape(B, N)
    c, bern, i, bad = _grid(ev, x, R, sphere)
    cells = ev.occupancy_num_cells(R, sphere)
    assert int(bad) == 0 and np.array_equal(_np(i), want)
    wc, wb = jc.count(want, cells)
    assert np.array_equal(_np(c), wc) and np.array_equal(_np(bern), wb)
    assert int(c.sum()) == B * N


@pytest.mark.parametrize("R,sphere", [(28, True), (40, False)])
def test_all_points_identical(ev, R, sphere):
    B, N = 3, 65
    x = np.tile(np.array([0.113, -0.2, 0.31], np.float32), (B, N, 1))
    c, bern, i, _ = _grid(ev, x, R, sphere)
    cell = int(jc.brute_force(x[0, :1], R, sphere)[0])
    assert bool((i == cell).all())
    assert int(c[0, cell]) == B * N and int(c.sum()) == B * N
    assert int(bern[0, cell]) == B and int(bern.sum()) == B          # one Bernoulli count per shape


@pytest.mark.parametrize("R,sphere,C", [(28, True, 4), (40, False, 16)])   # C = 16 at R = 40: 17 rows of 8000 bytes, three passes
def test_labelled_rows(ev, R, sphere, C):
    rng = np.random.default_rng(R + C)
    B, N = 3, 257
    x = jc.mixed_points(rng, B * N).reshape(B, N, 3)
    lab = rng.integers(0, C, (B, N)).astype(np.int32)
    lab[lab == 2] = 0                                               # part 2 is absent
    c0, b0, i0, _ = _grid(ev, x, R, sphere)
    c, b, i, bad = _grid(ev, x, R, sphere, lab, C)
    cells = ev.occupancy_num_cells(R, sphere)
    assert c.shape == (C + 1, cells) and int(bad) == 0
    assert torch.equal(c[0], c0[0]) and torch.equal(b[0], b0[0]) and torch.equal(i, i0)     # row 0 = the unlabelled call
    assert torch.equal(c[1:].sum(0), c[0])                          # all labels in range: the rows sum to row 0
    assert int(c[3].sum()) == 0 and int(b[3].sum()) == 0            # the absent part: a zero row
    wc, wb = jc.count(_np(i), cells, lab, C)
    assert np.array_equal(_np(c), wc) and np.array_equal(_np(b), wb)
    # out-of-range labels land in row 0 only
    lab2 = lab.copy()
    lab2[:, ::5], lab2[:, 1::7] = C, -1
    c2, b2, _, _ = _grid(ev, x, R, sphere, lab2, C)
    wc2, wb2 = jc.count(_np(i), cells, lab2, C)
    assert torch.equal(c2[0], c0[0]) and np.array_equal(_np(c2), wc2) and np.array_equal(_np(b2), wb2)
    assert int(c2[1:].sum()) == int(((lab2 >= 0) & (lab2 < C)).sum()) < B * N


def test_part_jsd(ev):
    rng = np.random.default_rng(5)
    x, y = jc.mixed_points(rng, 4 * 300).reshape(4, 300, 3) * 0.5, jc.mixed_points(rng, 3 * 300).reshape(3, 300, 3) * 0.5
    lx, ly = rng.integers(0, 4, (4, 300)).astype(np.int32), rng.integers(0, 4, (3, 300)).astype(np.int32)
    lx[lx == 1] = 0                                                 # part 1 has no sample point
    res = ev.part_jsd(x, lx, torch.from_numpy(y).cuda(), ly, n_class=4)
    assert list(res) == ["jsd", "part_0_jsd", "part_1_jsd", "part_2_jsd", "part_3_jsd"]
    assert np.isnan(res["part_1_jsd"]) and all(type(v).__name__ == "float64" for v in res.values())
    assert res["jsd"] == ev.jsd_between_point_cloud_sets(x, y)
    for p in (0, 2, 3):
        xp = [x[b][lx[b] == p] for b in range(4)]
        yp = [y[b][ly[b] == p] for b in range(3)]
        cx = sum(np.bincount(jc.brute_force(q, 28, True), minlength=10144) for q in xp)
        cy = sum(np.bincount(jc.brute_force(q, 28, True), minlength=10144) for q in yp)
        assert abs(res[f"part_{p}_jsd"] - ev.jensen_shannon_divergence(cx, cy)) < 1e-11
        assert 0.0 < res[f"part_{p}_jsd"] <= 1.0


def test_accumulate_and_reproducibility(ev, clouds):
    x = clouds["a"]
    whole = _grid(ev, x, 28, True)
    again = _grid(ev, x, 28, True)
    for u, v in zip(whole, again):
        assert torch.equal(u, v)                                    # two runs are bit-equal
    c, b, _, bad = _grid(ev, x[:4], 28, True)
    c2, b2, _, bad2 = _grid(ev, x[4:], 28, True, out=(c, b, bad))
    assert c2 is c and b2 is b
    assert torch.equal(c, whole[0]) and torch.equal(b, whole[1]) and int(bad) == 0
    j1 = ev.jsd_between_point_cloud_sets(x, clouds["b"])
    assert j1 == ev.jsd_between_point_cloud_sets(x, clouds["b"])


def test_non_finite_points(ev, clouds):
    x = clouds["b"].copy()
    x[1, 7, 2], x[4, 200], x[0, 0, 0] = np.nan, np.inf, -np.inf
    c, b, i, bad = _grid(ev, x, 28, True)
    ok = np.isfinite(x).all(2)
    assert int(bad) == 3 and int(c.sum()) == int(ok.sum())
    assert np.array_equal(_np(i) == -1, ~ok)
    assert np.array_equal(_np(i)[ok], jc.load_case(28, True)["index_b"][ok])
    c, b, _, bad = _grid(ev, x[:2], 28, True)
    _grid(ev, x[2:], 28, True, out=(c, b, bad))
    assert int(bad) == 3                                            # n_bad accumulates with the counters
    for call in (lambda: ev.jsd_between_point_cloud_sets(x, clouds["a"]), lambda: ev.jsd_between_point_cloud_sets(clouds["a"], x),
                 lambda: ev.entropy_of_occupancy_grid(x, 28, True),
                 lambda: ev.part_jsd(x, np.zeros(x.shape[:2], np.int32), clouds["a"], np.zeros(clouds["a"].shape[:2], np.int32))):
        with pytest.raises(ValueError, match="NaN or infinity"):
            call()
