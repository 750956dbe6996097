"""CPU: FPS and the auction EMD pinned to the reference's own CUDA kernels.

tests/golden/refk_*.npz hold what sampling_gpu.cu:59-173 and emd_cuda.cu:10-226,284-300 compute when their unmodified text is run
on the CPU through oracle/cuda_on_cpu.h (one block at a time, every CUDA thread a fibre that yields at __syncthreads();
tests/golden/make_golden_refkernels.py).  Here:

  * the C oracle (oracle/pointnet2.c) equals every fixture: FPS indices, EMD assignment and the EMD backward bit for bit; EMD
    distance bit for bit on lattice clouds and within 2^-21 d of the float64 distance of the fixture's assignment on random ones
    (oracle.refk_fixtures.check_emd_forward);
  * where a checkout of the reference is present, the recipe is rebuilt from scratch and reproduces every FPS fixture and every EMD
    fixture of at most 30 iterations bit for bit (skipped where there is no reference: the fixtures are the record);
  * the shim itself is held to its contract on toy kernels written for this test.

What the fixtures leave open on purpose is stated in their generator: the order of GetMax's racing writes (lattice fixtures carry
`race_rule`; random ones are kept only if the order does not matter) and the contraction of the three-term sums of squares.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from oracle import pointnet2 as opn
from oracle import refk_fixtures as fxs
from oracle import refkernels as rk

FPS, EMD, EMDBWD = fxs.names("fps"), fxs.names("emd"), fxs.names("emdbwd")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_refkernels", os.path.join(fxs.GOLDEN, "make_golden_refkernels.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_set_is_the_one_the_generator_writes():
    """Nothing missing, nothing stale; the sizes the HIP launch table switches at are all there; flags are what the tests rely on."""
    gen = _generator()
    assert sorted(n for n, _ in gen.all_cases()) == sorted(FPS + EMD + EMDBWD)
    sizes = {fxs.load(n)["xyz"].shape[1] for n in FPS}
    assert sizes >= {1, 5, 33, 512, 513, 700, 1024, 1025, 2048, 2049, 3000, 4096, 4097, 8192, 8193, 16384, 16385, 600, 1500, 40}
    tails, batched_tails, emd_sizes = 0, 0, set()
    for n in EMD:
        fx = fxs.load(n)
        assert str(fx["race_rule"]) == fxs.RACE_RULE and fx["a"].shape[1] % 1024 == 0
        if str(fx["kind"]) == "random":   # kept only because no schedule and no contraction changes them
            assert int(fx["race_moved"]) == 0 and np.array_equal(fx["assignment"], fx["assignment_desc"])
        tails += 1 <= int(fx["last_bidders"]) <= 8
        emd_sizes.add(fx["a"].shape[1])
        if fx["a"].shape[1] > 2048:
            # more than one 2048-target batch of Bid: ties follow its thread-major scan order once a bidder has two or more threads
            assert str(fx["kind"]) == "lattice" and int(fx["tie_iters"]) > 0
            hist = opn.emd_unassigned_per_iteration(fx["a"], fx["b"], float(fx["eps"]), int(fx["iters"]))
            blocks = fx["a"].shape[1] // 1024
            assert sum(1 for u in hist if u and 1024 // -(-int(u) // blocks) >= 2) >= 5, n
            batched_tails += 1 <= int(fx["last_bidders"]) <= 8
    assert emd_sizes >= {1024, 2048, 3072, 4096} and batched_tails >= 1
    assert tails >= 2 and sum(str(fxs.load(n)["kind"]) == "random" for n in EMD) >= 4


@pytest.mark.parametrize("name", FPS)
def test_oracle_fps_equals_reference_kernel(name):
    fx = fxs.load(name)
    got = opn.furthest_point_sampling(fx["xyz"], int(fx["npoint"]))
    assert got.dtype == np.int32 and np.array_equal(got, fx["idx"]), np.argwhere(got != fx["idx"])[:5]


@pytest.mark.parametrize("name", EMD)
def test_oracle_emd_forward_equals_reference_kernels(name):
    fx = fxs.load(name)
    dist, asg = opn.emd_forward(fx["a"], fx["b"], float(fx["eps"]), int(fx["iters"]))
    ratio = fxs.check_emd_forward(fx, dist, asg)
    print(f"{name}: worst |dist - d64| = {ratio:.3f} of the 2^-21 d bound; stored dist {fxs.emd_dist_error(fx, fx['dist']):.3f}")
    assert fxs.emd_dist_error(fx, fx["dist"]) <= 1.0   # the reference's own uncontracted distance obeys the same bound
    # the trace the tail fixtures were chosen by is the oracle's as well
    assert int(opn.emd_unassigned_per_iteration(fx["a"], fx["b"], float(fx["eps"]), int(fx["iters"]))[-1]) == int(fx["last_bidders"])


@pytest.mark.parametrize("name", EMDBWD)
def test_oracle_emd_backward_equals_reference_kernel(name):
    fx = fxs.load(name)
    got = opn.emd_backward(fx["a"], fx["b"], fx["grad_dist"], fx["assignment"])
    assert np.array_equal(got, fx["grad_xyz1"])
    assert np.abs(fx["grad_xyz1"]).max() > 0


# ------------------------------------------------------------------------------------------- the recipe, where the reference is
@pytest.fixture(scope="module")
def rebuilt():
    if not rk.available():
        pytest.skip("no checkout of the reference: the committed fixtures are the record")
    rk.build(force=True)
    return _generator()


def test_recipe_reproduces_fixtures(rebuilt):
    for name, maker in rebuilt.regeneration_subset():
        new, old = maker(), dict(np.load(os.path.join(fxs.GOLDEN, name), allow_pickle=False))
        assert sorted(new) == sorted(old), name
        for k in old:
            a = np.asarray(new[k])
            assert a.dtype == old[k].dtype and np.array_equal(a, old[k]), (name, k)


def test_recipe_refuses_another_revision_of_the_reference(rebuilt, monkeypatch):
    rel, first, last, out, digest = rk.SPANS[0]
    monkeypatch.setattr(rk, "SPANS", ((rel, first + 1, last, out, digest),) + rk.SPANS[1:])
    with pytest.raises(RuntimeError, match="sha256"):
        rk.extract()


def test_fps_hazard_of_the_reference_shows_on_the_ascending_schedule(rebuilt):
    """dists_i[0] is read after the last barrier of a step (:170) and overwritten by thread 0 in the next scan (:112): with thread 0
    first the later threads read the wrong winner; with thread 0 last (descending) nobody does.  One thread has no hazard."""
    fx = fxs.load("refk_fps_N33.npz")
    assert np.array_equal(rk.fps(fx["xyz"], 33, order=rk.DESCENDING), fx["idx"])
    assert not np.array_equal(rk.fps(fx["xyz"], 33, order=rk.ASCENDING), fx["idx"])
    one = fxs.load("refk_fps_N1.npz")
    assert np.array_equal(rk.fps(one["xyz"], 1, order=rk.ASCENDING), one["idx"])


# ------------------------------------------------------------------------------------------- the shim on its own
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def toy():
    return rk.selftest_lib()


@pytest.mark.parametrize("order", [rk.ASCENDING, rk.DESCENDING])
def test_shim_tree_reduction_with_barriers(toy, order):
    toy.selftest_schedule(order)
    rng = np.random.default_rng(1)
    for n, block in ((1000, 256), (64, 64), (7, 1), (300, 128)):
        x = rng.integers(-100, 100, n).astype(np.int32)
        out = np.full((n + block - 1) // block, -7, np.int32)
        toy.selftest_tree_sum(_p(x), n, block, _p(out))
        want = [int(x[i:i + block].sum()) for i in range(0, n, block)]
        assert out.tolist() == want


@pytest.mark.parametrize("order", [rk.ASCENDING, rk.DESCENDING])
def test_shim_threads_that_return_before_a_barrier(toy, order):
    toy.selftest_schedule(order)
    out = np.zeros(64, np.int32)
    toy.selftest_early_return(64, _p(out))
    want = [-1 if t & 1 else 100 + (t + 2) % 64 for t in range(64)]
    assert out.tolist() == want


@pytest.mark.parametrize("order", [rk.ASCENDING, rk.DESCENDING])
def test_shim_shared_array_is_static_and_blocks_run_in_order(toy, order):
    """Block (x, y) sees the stamp of the block before it in the documented order (y outer, x inner); the first block of a second
    launch sees the last block of the first."""
    toy.selftest_schedule(order)
    gx, gy = 3, 2
    seen = np.zeros(gx * gy, np.int32)
    toy.selftest_shared_reuse(gx, gy, 8, _p(seen))
    stamps = [1000 * (y + 1) + x + 1 for y in range(gy) for x in range(gx)]
    assert seen.tolist()[1:] == stamps[:-1]
    toy.selftest_shared_reuse(gx, gy, 8, _p(seen))
    assert seen.tolist() == [stamps[-1]] + stamps[:-1]


def test_shim_last_writer_follows_the_schedule(toy):
    slot = np.zeros(3, np.int32)
    toy.selftest_schedule(rk.ASCENDING)
    toy.selftest_last_writer(3, 200, _p(slot))
    assert slot.tolist() == [199] * 3
    toy.selftest_schedule(rk.DESCENDING)
    toy.selftest_last_writer(3, 200, _p(slot))
    assert slot.tolist() == [0] * 3
    toy.selftest_schedule(rk.ASCENDING)


@pytest.mark.parametrize("order", [rk.ASCENDING, rk.DESCENDING])
def test_shim_index_variables(toy, order):
    toy.selftest_schedule(order)
    gx, gy, bx, by = 3, 2, 4, 5
    out = np.zeros(gx * gy * bx * by, np.int32)
    toy.selftest_indices(gx, gy, bx, by, _p(out))
    want = [((Y * 16 + X) * 16 + y) * 16 + x for Y in range(gy) for X in range(gx) for y in range(by) for x in range(bx)]
    assert out.tolist() == want


def test_shim_atomics_and_bit_casts(toy):
    toy.selftest_schedule(rk.ASCENDING)
    x = np.array([0.5, -3.0, 7.25, 7.0, 1.0, 2.5, -0.0, 0.25], np.float32)
    fmax, count, fsum = np.array([-1e9], np.float32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    toy.selftest_atomics(_p(x), 8, _p(fmax), _p(count), _p(fsum))
    assert float(fmax[0]) == 7.25 and int(count[0]) == 8 and float(fsum[0]) == float(np.clip(x, 0, 2).sum())
