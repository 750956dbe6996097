"""GPU parity of the auction EMD through the C-ABI vs the C oracle (oracle/pointnet2.c: a sequential
restatement of emd_cuda.cu): assignment and squared distances bit-exact — integer work and correctly-rounded fp32 /
fp64 scalar arithmetic in the same order.  The oracle itself is pinned to the reference's own kernels run on the CPU
(tests/test_refkernels_cpu.py; the HIP kernel directly in tests/test_gpu_refkernels.py); its rule for GetMax's data race, which the
reference leaves undefined (largest bidder index = last writer in ascending thread order), is shared by both sides."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _clouds(B, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(0, 1, (B, n, 3)).astype(np.float32), rng.uniform(0, 1, (B, n, 3)).astype(np.float32)


@pytest.mark.parametrize("B,n,iters", [(3, 1024, 300), (2, 2048, 60), (2, 1000, 200), (1, 64, 5000), (2, 8192, 3)])
def test_emd_forward_bit_exact_vs_oracle(B, n, iters):
    from difffacto_amd.metrics import emdFunction
    from oracle import pointnet2 as o
    a, b = _clouds(B, n, n + iters)
    d_ref, as_ref = o.emd_forward(a, b, 0.002, iters)
    d, asg = emdFunction.apply(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 0.002, iters)
    assert np.array_equal(asg.cpu().numpy(), as_ref)
    assert np.array_equal(d.cpu().numpy(), d_ref)


def test_emd_converged_is_a_permutation_and_near_optimal():
    """Size-independent property: once the auction has converged (no unassigned point left before the last iteration) the
    assignment is a permutation and its cost is within n * eps of the optimal transport cost."""
    from difffacto_amd.metrics import EMD
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist
    a, b = _clouds(2, 512, 7)
    dist, asg = EMD(0.002, 20000)(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    cost = EMD(0.002, 20000, dist_only=True)(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    for i in range(2):
        assert sorted(asg[i].cpu().tolist()) == list(range(512))
        C = cdist(a[i], b[i])
        r, c = linear_sum_assignment(C)
        assert C[r, c].mean() - 1e-6 <= cost[i] <= C[r, c].mean() + 0.002 + 1e-6


def test_emd_backward_vs_oracle():
    from difffacto_amd.metrics import emdFunction
    from oracle import pointnet2 as o
    a, b = _clouds(2, 256, 3)
    x1 = torch.from_numpy(a).cuda().requires_grad_(True)
    x2 = torch.from_numpy(b).cuda().requires_grad_(True)
    d, asg = emdFunction.apply(x1, x2, 0.005, 50)
    w = torch.linspace(0.5, 1.5, 256, device="cuda")[None].expand(2, -1)
    (d * w).sum().backward()
    ref = o.emd_backward(a, b, w.cpu().numpy(), asg.cpu().numpy())
    assert np.abs(x1.grad.cpu().numpy() - ref).max() < 1e-6
    assert float(x2.grad.abs().max()) == 0.0


_BATCHED = {}


def _batched_cases():
    """Lattice clouds (k/16: constant exact ties) of more than 2048 points, eps 0.1 so that the tail is reached: (a, b, iters, oracle
    distance, oracle assignment, bidders of the last iteration), computed once."""
    if not _BATCHED:
        from oracle import pointnet2 as o
        for n, its in ((2500, (3, 20, 75, 120, 300)), (3000, (3, 40, 160, 300))):
            rng = np.random.Generator(np.random.PCG64(n))
            lat = (rng.integers(0, 17, (2, n, 3)) / 16).astype(np.float32)
            a, b = lat[:1], lat[1:]
            hist = o.emd_unassigned_per_iteration(a, b, 0.1, max(its))
            _BATCHED[n] = [(a, b, it) + tuple(o.emd_forward(a, b, 0.1, it)) + (int(hist[it - 1]),) for it in its]
    return _BATCHED


@pytest.mark.parametrize("state_global", [0, 1])
@pytest.mark.parametrize("n", [2500, 3000])
def test_emd_more_than_one_target_batch_ties_bit_exact(n, state_global):
    """n > 2048: the reference's Bid walks the targets in batches of 2048, every thread of a bidder its chunk of each batch, so among
    equal values the first in (thread, batch, k) order wins, not the first k (the oracle is pinned to that by the n = 3072 and 4096
    fixtures of tests/test_gpu_refkernels.py; the reference itself takes multiples of 1024 only).  Ragged sizes, whose last batch has
    a chunk length of its own: 2500 keeps the auction's state in LDS, 3000 in the workspace; stopped among many bidders and inside
    the tail path (the keys then travel through the partial merges of wavefront 0)."""
    from difffacto_amd import _ffi
    from difffacto_amd.metrics import emdFunction
    cases = _batched_cases()[n]
    assert sum(1 <= c[5] <= 8 for c in cases) >= 2 and sum(c[5] > 16 for c in cases) >= 2
    _ffi.lib().dfx_debug_emd_state_global(state_global)
    try:
        for a, b, it, d_ref, as_ref, _ in cases:
            d, asg = emdFunction.apply(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 0.1, it)
            assert np.array_equal(asg.cpu().numpy(), as_ref), (n, it, int((asg.cpu().numpy() != as_ref).sum()))
            assert np.array_equal(d.cpu().numpy(), d_ref), (n, it)
    finally:
        _ffi.lib().dfx_debug_emd_state_global(0)


@pytest.mark.parametrize("state_global", [0, 1])
def test_emd_tail_iterations_and_ties_bit_exact(state_global):
    """The auction's tail (<= 8 unassigned points: a separate path of the kernel — eight wavefronts share the scans, one finishes the
    iteration in registers) stopped at many different iterations, so that the last, non-evicting iteration (:209-211) falls on 1, 2,
    .. bidders as well as on many; ragged n; and lattice clouds: exact ties between targets (first index wins), equal increments on
    one target (largest bidder index wins) and coincident points (distance 0).  With the state in LDS and in the workspace."""
    from difffacto_amd import _ffi
    from difffacto_amd.metrics import emdFunction
    from oracle import pointnet2 as o
    rng = np.random.Generator(np.random.PCG64(11))
    cases = []
    for n in (257, 96):
        a, b = _clouds(1, n, n)
        cases += [(a, b, it) for it in (1, 2, 3, 17, 40, 80, 120, 160, 200, 250, 300, 400, 600, 900)]
    lat = (rng.integers(0, 5, (2, 200, 3)) / 4).astype(np.float32)
    cases += [(lat[:1], lat[1:], it) for it in (5, 50, 500, 3000)] + [(lat[:1], lat[:1].copy(), 50)]
    # squared distances in (0, 2^-96) (the kernel's square root takes its library path for such a scan), alone and mixed with ordinary ones
    a, b = _clouds(1, 130, 3)
    mixed_a, mixed_b = a.copy(), b.copy()
    mixed_a[0, :40] *= np.float32(1e-17)
    mixed_b[0, 20:70] *= np.float32(1e-17)
    cases += [(a * np.float32(1e-16), b * np.float32(1e-16), 30), (mixed_a, mixed_b, 40), (mixed_a, mixed_b, 700)]
    _ffi.lib().dfx_debug_emd_state_global(state_global)
    try:
        tails = 0
        for a, b, it in cases:
            d_ref, as_ref = o.emd_forward(a, b, 0.002, it)
            d, asg = emdFunction.apply(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 0.002, it)
            assert np.array_equal(asg.cpu().numpy(), as_ref), (a.shape, it)
            assert np.array_equal(d.cpu().numpy(), d_ref), (a.shape, it)
            tails += 0 < int(o.emd_unassigned_per_iteration(a, b, 0.002, it)[-1]) <= 8
        assert tails >= 6   # the sweep does stop inside the tail (the last iteration has 1..8 bidders)
    finally:
        _ffi.lib().dfx_debug_emd_state_global(0)
