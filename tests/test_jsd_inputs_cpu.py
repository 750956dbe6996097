"""CPU checks of the occupancy-JSD front door: jensen_shannon_divergence on host tensors of any dtype (float weights are normalised,
not truncated), and the column walk compiled for the host on points far outside the grid in every direction, where the walk starts
at a clamped slab and an outer column must win."""
import ctypes

import numpy as np
import pytest
import torch

import _jsd_case as jc


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _scipy_free_jsd(P, Q):
    def bits(v):
        v = v[v > 0]
        return -np.sum(v * np.log2(v))
    P, Q = P / P.sum(), Q / Q.sum()
    return bits((P + Q) / 2) - (bits(P) + bits(Q)) / 2


def test_jsd_of_host_tensors_and_float_weights():
    from difffacto_amd import evaluation as ev
    rng = np.random.default_rng(3)
    P, Q = rng.uniform(0, 1, 257), rng.uniform(0, 1, 257)            # weights below 1: an integer cast would give 0 / 0
    want = _scipy_free_jsd(P, Q)
    for a, b in ((P, Q), (torch.from_numpy(P), torch.from_numpy(Q)), (torch.from_numpy(P), Q), (P.tolist(), torch.from_numpy(Q))):
        got = ev.jensen_shannon_divergence(a, b)
        assert type(got).__name__ == "float64" and abs(got - want) < 1e-11 and 0.0 < got <= 1.0   # 257 fp64 terms of size <= 1
    c, d = rng.integers(0, 50, 300), rng.integers(0, 50, 300)
    assert ev.jensen_shannon_divergence(torch.from_numpy(c), torch.from_numpy(d).int()) == ev.jensen_shannon_divergence(c, d)


@pytest.mark.parametrize("R,sphere", [(3, True), (28, True), (40, True), (28, False)])
def test_host_compiled_walk_from_every_side(L, R, sphere):
    rng = np.random.default_rng(7 * R + sphere)
    sign = np.array([[sx, sy, sz] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)], np.float64)
    pts = [sign * s + rng.uniform(-0.3, 0.3, sign.shape) for s in (0.45, 0.6, 1.0, 3.0, 1e3, 1e7)]
    pts = np.concatenate(pts + [rng.uniform(-0.7, 0.7, (2000, 3))]).astype(np.float32)
    out = np.zeros(len(pts), np.int32)
    rc = L.dfx_debug_occupancy_host(pts.ctypes.data_as(ctypes.c_void_p), len(pts), R, int(sphere), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.dfx_last_error()
    assert np.array_equal(out, jc.brute_force(pts, R, sphere))
