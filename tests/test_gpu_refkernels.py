"""GPU: the HIP FPS and auction-EMD kernels against what the reference's own CUDA kernels compute (tests/golden/refk_*.npz: their
unmodified text run on the CPU, see tests/golden/make_golden_refkernels.py and tests/test_refkernels_cpu.py).  Fixtures only — neither
the emulator nor the reference is used here.

FPS: indices bit for bit, through the production launch table and through every register-resident instantiation that the debug hook
can select and that holds the cloud (seven of the thirteen are reachable through the hook alone, and the production table is chosen
among them by tools/experiments/sweep_fps_shape.py).  EMD: assignment bit for bit; distance bit for bit on lattice clouds, within
2^-21 d of the float64 distance of the fixture's assignment on random ones; with the auction's state in LDS and in the workspace.
Lattice EMD fixtures carry the reference's GetMax write race resolved as "last writer = largest bidder"; the random ones and every
FPS fixture do not depend on any schedule."""
import numpy as np
import pytest
import torch

from oracle import refk_fixtures as fxs

pytestmark = pytest.mark.gpu

FPS, EMD, EMDBWD = fxs.names("fps"), fxs.names("emd"), fxs.names("emdbwd")
FPS_SHAPES = [(256, 2), (256, 4), (256, 8), (256, 16), (256, 32), (512, 2), (512, 4), (512, 8), (512, 16),
              (1024, 2), (1024, 4), (1024, 8), (1024, 16)]


@pytest.fixture(scope="module")
def pu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from difffacto_amd.pointnet2_ops import pointnet2_utils
    return pointnet2_utils


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_fixtures_present():
    assert len(FPS) >= 20 and len(EMD) >= 19 and len(EMDBWD) >= 1


@pytest.mark.parametrize("name", FPS)
def test_fps_equals_reference_kernel(pu, name):
    fx = fxs.load(name)
    got = pu.furthest_point_sample(dev(fx["xyz"]), int(fx["npoint"])).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, fx["idx"]), np.argwhere(got != fx["idx"])[:5]


FPS_STREAMING = ["refk_fps_N16385.npz"]   # more points than any register-resident shape holds: the production launch alone (above)


def test_fps_launch_shape_cases_leave_out_only_the_streaming_size():
    assert set(FPS_STREAMING) <= set(FPS)
    for name in FPS:
        N = fxs.load(name)["xyz"].shape[1]
        assert (name in FPS_STREAMING) == (N > max(nt * ppt for nt, ppt in FPS_SHAPES)), name


@pytest.mark.parametrize("name", [n for n in FPS if n not in FPS_STREAMING])
def test_fps_every_launch_shape_equals_reference_kernel(pu, name):
    from difffacto_amd import _ffi
    fx = fxs.load(name)
    xyz, M, N = dev(fx["xyz"]), int(fx["npoint"]), fx["xyz"].shape[1]
    shapes = [s for s in FPS_SHAPES if s[0] * s[1] >= N]
    assert shapes, N
    try:
        for nt, ppt in shapes:
            _ffi.lib().dfx_debug_fps_shape(nt, ppt)
            got = pu.furthest_point_sample(xyz, M).cpu().numpy()
            assert np.array_equal(got, fx["idx"]), (nt, ppt, np.argwhere(got != fx["idx"])[:5])
    finally:
        _ffi.lib().dfx_debug_fps_shape(0, 0)


@pytest.mark.parametrize("state_global", [0, 1])
@pytest.mark.parametrize("name", EMD)
def test_emd_forward_equals_reference_kernels(pu, name, state_global):
    from difffacto_amd import _ffi
    from difffacto_amd.metrics import emdFunction
    fx = fxs.load(name)
    _ffi.lib().dfx_debug_emd_state_global(state_global)
    try:
        d, asg = emdFunction.apply(dev(fx["a"]), dev(fx["b"]), float(fx["eps"]), int(fx["iters"]))
        d, asg = d.cpu().numpy(), asg.cpu().numpy()
    finally:
        _ffi.lib().dfx_debug_emd_state_global(0)
    ratio = fxs.check_emd_forward(fx, d, asg)
    print(f"{name} state_global={state_global}: worst |dist - d64| = {ratio:.3f} of the 2^-21 d bound")


@pytest.mark.parametrize("name", EMDBWD)
def test_emd_backward_equals_reference_kernel(pu, name):
    from difffacto_amd.metrics import emdFunction
    fx = fxs.load(name)
    x1, x2 = dev(fx["a"]).requires_grad_(True), dev(fx["b"]).requires_grad_(True)
    d, asg = emdFunction.apply(x1, x2, float(fx["eps"]), int(fx["iters"]))
    assert np.array_equal(asg.cpu().numpy(), fx["assignment"])
    (d * dev(fx["grad_dist"])).sum().backward()
    assert np.array_equal(x1.grad.cpu().numpy(), fx["grad_xyz1"])
    assert float(x2.grad.abs().max()) == 0.0   # emd_module.py:70-73: the second cloud gets zeros
