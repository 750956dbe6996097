"""CPU checks of the occupancy-grid JSD: the dfx_occupancy_* entry points are exported and bound and reject bad arguments before touching
a GPU; the host grid (cell counts, keep mask) and the kernel's per-point search, compiled for the host, against the reference's recorded
values (tests/golden/jsd/, make_golden_jsd.py) and a float64 brute force; jensen_shannon_divergence on recorded counters; the
fixtures' manifest."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _jsd_case as jc

NEW = ("dfx_occupancy_num_cells", "dfx_occupancy_cell_mask", "dfx_occupancy_grid_f32", "dfx_occupancy_jsd_f64",
       "dfx_occupancy_entropy_f64")


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_occupancy_symbols_are_exported_and_bound(L):
    from difffacto_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert L.dfx_version() >= 104 and L.dfx_abi_version() == 5 == _ffi.DFX_ABI_VERSION


FAKE = ctypes.c_void_p(0x1000)   # a non-null "device pointer": never dereferenced, the checks fail first


def _err(L, rc):
    return rc, (L.dfx_last_error() or b"").decode()


def test_occupancy_grid_rejects_bad_arguments_without_a_gpu(L):
    def grid(xyz=FAKE, lab=None, B=2, N=64, C=0, R=28, sphere=1, counters=FAKE, bern=FAKE, index=None, n_bad=FAKE):
        return _err(L, L.dfx_occupancy_grid_f32(xyz, lab, B, N, C, R, sphere, 0, counters, bern, index, n_bad, None))
    for kw, msg in [(dict(xyz=None), "null"), (dict(counters=None), "null"), (dict(bern=None), "null"), (dict(n_bad=None), "null"),
                    (dict(B=0), "positive"), (dict(B=-1), "positive"), (dict(N=0), "positive"), (dict(R=1), "outside"),
                    (dict(R=41), "outside"), (dict(R=0), "outside"), (dict(lab=FAKE, C=17), "outside"), (dict(lab=FAKE, C=-1), "outside"),
                    (dict(R=2, sphere=1), "keeps no cell")]:
        rc, m = grid(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)


def test_reductions_and_host_entries_reject_bad_arguments(L):
    for args, msg in [((None, FAKE, 10, FAKE), "null"), ((FAKE, None, 10, FAKE), "null"), ((FAKE, FAKE, 10, None), "null"),
                      ((FAKE, FAKE, 0, FAKE), "positive")]:
        rc, m = _err(L, L.dfx_occupancy_jsd_f64(*args, None))
        assert rc == -1 and msg in m, (args, rc, m)
    for args, msg in [((None, 10, 3, FAKE), "null"), ((FAKE, 10, 3, None), "null"), ((FAKE, 0, 3, FAKE), "positive"),
                      ((FAKE, 10, 0, FAKE), "positive")]:
        rc, m = _err(L, L.dfx_occupancy_entropy_f64(*args, None))
        assert rc == -1 and msg in m, (args, rc, m)
    for R in (1, 41, -3):
        assert L.dfx_occupancy_num_cells(R, 1) < 0 and "outside" in _err(L, 0)[1]
        rc, m = _err(L, L.dfx_occupancy_cell_mask(R, 1, FAKE))
        assert rc == -1 and "outside" in m
    rc, m = _err(L, L.dfx_occupancy_cell_mask(8, 1, None))
    assert rc == -1 and "null" in m


def test_cell_counts(L):
    assert L.dfx_occupancy_num_cells(28, 1) == 10144 and L.dfx_occupancy_num_cells(28, 0) == 21952
    assert L.dfx_occupancy_num_cells(2, 1) == 0 and L.dfx_occupancy_num_cells(2, 0) == 8
    assert L.dfx_occupancy_num_cells(3, 1) == 7 and L.dfx_occupancy_num_cells(40, 0) == 64000


@pytest.mark.parametrize("R,sphere", jc.CASES)
def test_cell_mask_and_grid_match_reference(L, R, sphere):
    from difffacto_amd import evaluation as ev
    z = jc.load_case(R, sphere)
    want = jc.recorded_mask(z, R)
    mask = np.zeros((R, R, R), np.uint8)
    assert L.dfx_occupancy_cell_mask(R, int(sphere), mask.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(mask.astype(bool), want)
    assert L.dfx_occupancy_num_cells(R, int(sphere)) == int(z["cells"]) == int(want.sum())
    assert np.array_equal(jc.keep_mask(R, sphere), want)          # the brute force of the GPU tests stands on the same grid
    grid, spacing = ev.unit_cube_grid_point_cloud(R, sphere)
    assert grid.dtype == np.float32 and spacing == 1.0 / float(R - 1)
    a = jc.grid_axis(R)
    full = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1)
    assert grid.shape == ((int(z["cells"]), 3) if sphere else (R, R, R, 3))
    assert np.array_equal(grid.reshape(-1, 3), full.reshape(-1, 3)[want.reshape(-1)])


def _host_search(L, pts, R, sphere):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), np.int32)
    rc = L.dfx_debug_occupancy_host(pts.ctypes.data_as(ctypes.c_void_p), len(pts), R, int(sphere), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.dfx_last_error()
    return out


@pytest.mark.parametrize("R,sphere", jc.CASES)
def test_host_compiled_search_matches_reference_indices(L, R, sphere):
    """The kernel's per-point functions, compiled for the host, give the reference's kneighbors index for every fixture point."""
    z = jc.load_case(R, sphere)
    for name, pcs in jc.load_clouds().items():
        assert np.array_equal(_host_search(L, pcs, R, sphere).reshape(pcs.shape[:2]), z[f"index_{name}"]), name


@pytest.mark.parametrize("R,sphere", [(2, False), (3, True), (5, True), (28, True), (40, False), (40, True)])
def test_host_compiled_search_against_brute_force_on_ties_and_far_points(L, R, sphere):
    rng = np.random.default_rng(100 * R + sphere)
    a = jc.grid_axis(R)
    n = 64
    ii, jj, ax = rng.integers(0, R, (n, 3)), rng.integers(0, R - 1, (n, 3)), rng.integers(0, 3, n)
    mid8 = (a[jj].astype(np.float64) + a[jj + 1]) / 2                                  # midpoint of eight cells
    mid2 = a[ii].astype(np.float64)
    mid2[np.arange(n), ax] = mid8[np.arange(n), ax]                                   # midpoint of two cells
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    near_mid = np.zeros((n, 3))                                                       # far in y, x a hair off a midpoint or the centre:
    near_mid[:, 0], near_mid[:, 1], near_mid[:, 2] = rng.uniform(-1e-9, 1e-9, n), 1e3, rng.uniform(-0.5, 0.5, n)   # equal after rounding
    pts = np.concatenate([jc.mixed_points(rng, 600), a[ii], mid8, mid2, 1e3 * d, 1e7 * d, 1e20 * d, near_mid]).astype(np.float32)
    pts[3], pts[11, 1] = np.nan, np.inf
    got = _host_search(L, pts, R, sphere)
    assert got[3] == -1 and got[11] == -1
    assert np.array_equal(got, jc.brute_force(pts, R, sphere))


@pytest.mark.parametrize("R,sphere", jc.CASES)
def test_jensen_shannon_divergence_on_recorded_counters(R, sphere):
    from difffacto_amd import evaluation as ev
    z = jc.load_case(R, sphere)
    got = ev.jensen_shannon_divergence(z["counters_a"], z["counters_b"])
    assert type(got).__name__ == str(z["type_jsd"])
    assert abs(got - float(z["jsd_ab"])) < 1e-11, (got, float(z["jsd_ab"]))
    assert ev.jensen_shannon_divergence(z["counters_a"], z["counters_a"]) == 0.0 == float(z["jsd_aa"])
    assert 0.0 < got <= 1.0


def test_jensen_shannon_divergence_value_errors():
    from difffacto_amd import evaluation as ev
    with pytest.raises(ValueError, match="Negative values"):
        ev.jensen_shannon_divergence(np.array([1.0, -1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="Negative values"):
        ev.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([-2.0, 1.0]))
    with pytest.raises(ValueError, match="Non equal size"):
        ev.jensen_shannon_divergence(np.array([1.0, 1.0, 0.0]), np.array([1.0, 1.0]))


def test_jsd_golden_manifest():
    sys.path.insert(0, os.path.join(jc.ROOT, "tests", "golden"))
    import manifest
    want = {}
    for line in open(os.path.join(jc.JSD, "MANIFEST.sha256")):
        if line.strip() and not line.startswith("#"):
            h, name = line.split()
            want[name] = h
    files = sorted(os.listdir(jc.JSD))
    assert all(f.endswith(".npz") or f == "MANIFEST.sha256" for f in files), files
    have = {f: manifest.content_hash(os.path.join(jc.JSD, f)) for f in files if f.endswith(".npz")}
    assert want == have and set(have) == {"clouds.npz"} | {jc.case_name(R, s) for R, s in jc.CASES}
    assert all(os.path.getsize(os.path.join(jc.JSD, f)) < 200 * 1024 for f in have)
