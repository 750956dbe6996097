"""GPU parity of the Chamfer-L2 kernels (csrc/chamfer_kernels.hip) through the C-ABI vs the C oracle (oracle/pointnet2.c: the same
`k == 0 || d < best` rule and the same mul, fma, fma order as chamfer.cu), on the launch path the evaluation takes.

dfx_chamfer_forward_f32 picks chamfer_nn_kernel<2> (two queries per thread, 512-query workgroups) when B * ceil(n / 512) >= 256 and <1>
otherwise.  The evaluation (PAIRS_PER_LAUNCH = 1024 pairs) and bench.py (B = 128, N = 2048) both take <2>; here both instantiations are held
bit-exact against the oracle — distances AND indices, which ChamferFunction.forward never returns — through the launcher's own rule and through
dfx_debug_chamfer_queries, across the CD_TILE = 1024 boundary, on exact ties and on non-finite input.  The backward is held against a float64
reference with a bound derived from its arithmetic (see _grad_bound), including its grid-stride loop (more than 8192 x 256 points)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of fp32


def _dev(x):
    return torch.tensor(x, device="cuda")


@contextlib.contextmanager
def _queries(q):
    """dfx_debug_chamfer_queries(q) for the duration of the block; the launcher's own rule (0) afterwards, whatever happens."""
    from difffacto_amd import _ffi
    _ffi.lib().dfx_debug_chamfer_queries(q)
    try:
        yield
    finally:
        _ffi.lib().dfx_debug_chamfer_queries(0)


def _forward(a, b):
    """dfx_chamfer_forward_f32 directly: d1 (B,N), d2 (B,M), i1, i2 as numpy.  The outputs start out poisoned (-1), so a store the kernel
    skips shows."""
    from difffacto_amd import _ffi
    B, N, _ = a.shape
    M = b.shape[1]
    ta, tb = _dev(a), _dev(b)
    d1, d2 = torch.full((B, N), -1.0, device="cuda"), torch.full((B, M), -1.0, device="cuda")
    i1 = torch.full((B, N), -1, dtype=torch.int32, device="cuda")
    i2 = torch.full((B, M), -1, dtype=torch.int32, device="cuda")
    _ffi.check(_ffi.lib().dfx_chamfer_forward_f32(_ffi.ptr(ta), _ffi.ptr(tb), _ffi.ptr(d1), _ffi.ptr(d2), _ffi.ptr(i1), _ffi.ptr(i2),
                                                  B, N, M, _ffi.current_stream()), "dfx_chamfer_forward_f32")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (d1, d2, i1, i2))


def _backward(a, b, i1, i2, g1, g2):
    """dfx_chamfer_backward_f32 directly: grad_xyz1 (B,N,3), grad_xyz2 (B,M,3) as numpy (poisoned with NaN: the launcher's memset shows)."""
    from difffacto_amd import _ffi
    B, N, _ = a.shape
    M = b.shape[1]
    t = [_dev(x) for x in (a, b, i1, i2, g1, g2)]
    gx1, gx2 = torch.full((B, N, 3), float("nan"), device="cuda"), torch.full((B, M, 3), float("nan"), device="cuda")
    _ffi.check(_ffi.lib().dfx_chamfer_backward_f32(*map(_ffi.ptr, t), _ffi.ptr(gx1), _ffi.ptr(gx2), B, N, M, _ffi.current_stream()),
               "dfx_chamfer_backward_f32")
    torch.cuda.synchronize()
    return gx1.cpu().numpy(), gx2.cpu().numpy()


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _normal_case(B, N, M):
    """Standard-normal clouds with a duplicated reference point (strict '<' keeps the first index) and the oracle's forward: computed once per
    shape, shared by the tests, read-only."""
    from oracle import pointnet2 as o
    rng = np.random.Generator(np.random.PCG64(1000003 * B + 1009 * N + M))
    a = rng.standard_normal((B, N, 3)).astype(np.float32)
    b = rng.standard_normal((B, M, 3)).astype(np.float32)
    if M > 2:
        b[:, 1] = b[:, 0]
    return _frozen(a, b, *o.chamfer_forward(a, b))


def _assert_forward_exact(got, ref, what, equal_nan=False):
    for name, g, r in zip(("dist1", "dist2", "idx1", "idx2"), got, ref):
        same = np.array_equal(g, r, equal_nan=True) if equal_nan and g.dtype.kind == "f" else np.array_equal(g, r)
        assert same, (what, name, int((g != r).sum()), np.argwhere(g != r)[:4].tolist())


# ---- (a) the launcher's own rule --------------------------------------------------------------------------------------------------------
# (256, 300, 1030): both directions take <2>; N = 300 leaves 44 live second queries and 212 clamped ones, M = 1030 crosses the tile with a 6-point tail
# (128, 600, 500):  N takes <2> at two workgroups per cloud, M takes <1>: one call mixes the two
# (255, 512, 512):  one workgroup short of the threshold: <1>
LAUNCHER_SHAPES = [(256, 300, 1030), (128, 600, 500), (255, 512, 512)]


@pytest.mark.parametrize("B,N,M", LAUNCHER_SHAPES)
def test_forward_bit_exact_under_the_launchers_rule(B, N, M):
    a, b, *ref = _normal_case(B, N, M)
    _assert_forward_exact(_forward(a, b), ref, (B, N, M))


# ---- (b) both instantiations at every edge shape ----------------------------------------------------------------------------------------
EDGE_SHAPES = [(1, 7), (7, 1), (255, 1024), (256, 1025), (257, 1023), (511, 2049), (512, 2048), (513, 3000), (1025, 33)]


@pytest.mark.parametrize("N,M", EDGE_SHAPES)
def test_forward_bit_exact_with_one_and_two_queries_per_thread(N, M):
    a, b, *ref = _normal_case(2, N, M)
    got = {}
    for q in (1, 2):
        with _queries(q):
            got[q] = _forward(a, b)
        _assert_forward_exact(got[q], ref, (N, M, q))
    _assert_forward_exact(got[2], got[1], (N, M, "<2> vs <1>"))


# ---- (c) ties across tiles ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice_case(M):
    """Lattice clouds (coordinates in {0, 1/4, .., 1}: exact ties everywhere) with hand-planted duplicates across the CD_TILE = 1024 boundary.  The
    planted points sit on odd eighths, so no lattice point equals them and the lower index of each pair is known:
      reference 1024 = reference 0     (first slot of tile 1 vs the point the kernel takes outside its loop)
      reference 1029 = reference 5
      reference 2048 = reference 1023  (first slot of tile 2 vs the last slot of tile 0; M = 2050 only)
    plus one-off points at 1030 and 2049, the only zero-distance match of their queries (a minimum found in a later tile keeps its tile's base),
    and queries coincident with each of these, in the first (j < 256) and in the second (256 <= j < 512) query slot of a <2> workgroup and in a later
    workgroup.  Returns (a, b, oracle outputs, [(query index, expected reference index)])."""
    from oracle import pointnet2 as o
    rng = np.random.Generator(np.random.PCG64(77 + M))
    N = 1100   # > CD_TILE: the second direction crosses the boundary too
    a = (rng.integers(0, 5, (2, N, 3)) / 4).astype(np.float32)
    b = (rng.integers(0, 5, (2, M, 3)) / 4).astype(np.float32)
    pairs = [(0, 1024, (0.125, 0.375, 0.625)), (5, 1029, (0.375, 0.125, 0.875)), (1023, 2048, (0.875, 0.625, 0.125))]
    planted = []
    for n, (low, high, p) in enumerate(pairs):
        if high >= M:
            continue
        b[:, low] = b[:, high] = p
        for j in (n, 300 + n, 1090 + n):
            a[:, j] = p
            planted.append((j, low))
    for n, (k, p) in enumerate([(1030, (0.625, 0.875, 0.375)), (2049, (0.125, 0.875, 0.625))]):
        if k >= M:
            continue
        b[:, k] = p
        for j in (10 + n, 310 + n):
            a[:, j] = p
            planted.append((j, k))
    return _frozen(a, b, *o.chamfer_forward(a, b)) + (planted,)


@pytest.mark.parametrize("M", [1500, 2050])
@pytest.mark.parametrize("q", [1, 2])
def test_first_minimum_wins_across_tiles(q, M):
    a, b, r1, r2, ri1, ri2, planted = _lattice_case(M)
    assert len(planted) == (13 if M > 2049 else 8)
    with _queries(q):
        d1, d2, i1, i2 = _forward(a, b)
    _assert_forward_exact((d1, d2, i1, i2), (r1, r2, ri1, ri2), (M, q))
    for j, k in planted:
        assert np.all(i1[:, j] == k) and np.all(d1[:, j] == 0), (M, q, j, k, i1[:, j], d1[:, j])
    # the lattice did produce ties beyond the planted ones: many queries at distance 0 from a reference that has a later twin
    assert int((d1 == 0).sum()) > 100


# ---- (d) non-finite input ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2])
def test_non_finite_input_follows_the_reference_rule(q):
    """chamfer.cu:47,:132,:137: the first point is taken unconditionally and every later one through a strict '<' (a tile's best replaces the
    running one through a strict '>'), so a NaN distance to reference 0 sticks and a NaN distance to a later reference never wins; an infinite
    query is at distance inf from everything and keeps index 0.  (The later NaN sits at 700, not on a multiple of the reference's own 512-point
    tile, whose first slot it also takes unconditionally.)"""
    from oracle import pointnet2 as o
    rng = np.random.Generator(np.random.PCG64(4))
    a = rng.standard_normal((3, 600, 3)).astype(np.float32)
    b = rng.standard_normal((3, 1500, 3)).astype(np.float32)
    b[0, 0, 1] = np.nan        # cloud 0: NaN in the first reference point
    b[1, 700, 0] = np.nan      # cloud 1: NaN in a middle reference point ..
    a[1, 3, 2] = np.inf        # .. and an infinite query (a later reference point in the other direction)
    a[1, 300, 0] = -np.inf     # (second query slot of a <2> workgroup)
    ref = r1, r2, ri1, ri2 = o.chamfer_forward(a, b)
    assert np.isnan(r1[0]).all() and (ri1[0] == 0).all()                                          # a NaN first point sticks
    finite = np.setdiff1d(np.arange(600), [3, 300])
    assert np.isfinite(r1[1][finite]).all() and not (ri1[1] == 700).any()                          # a later NaN never wins
    assert np.isinf(r1[1][[3, 300]]).all() and (ri1[1][[3, 300]] == 0).all()                       # an infinite query: inf, index 0
    assert not np.isin(ri2[1], [3, 300]).any() and np.isfinite(np.delete(r2[1], 700)).all()        # an infinite later point never wins
    assert np.isnan(r2[0][0]) and ri2[0][0] == 0 and np.isnan(r2[1][700]) and ri2[1][700] == 0     # a NaN query: NaN, index 0
    assert np.isfinite(r1[2]).all() and np.isfinite(r2[2]).all()
    with _queries(q):
        got = _forward(a, b)
    _assert_forward_exact(got, ref, q, equal_nan=True)


# ---- (e) backward against float64 with a derived bound ----------------------------------------------------------------------------------
def _grad_ref(a, b, i1, i2, g1, g2):
    """float64 gradients of both directions (g = None leaves a direction out), and per output row k = the number of terms added into it and per
    element S = the sum of the terms' absolute values.  Returns ((ref1, k1, S1), (ref2, k2, S2))."""
    B, N, _ = a.shape
    M = b.shape[1]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    out1 = [np.zeros((B * N * 3,)), np.zeros((B * N * 3,)), np.zeros((B * N * 3,))]
    out2 = [np.zeros((B * M * 3,)), np.zeros((B * M * 3,)), np.zeros((B * M * 3,))]
    bi = np.arange(B)[:, None]
    for q, r, idx, g, oq, orf, m in ((a64, b64, i1, g1, out1, out2, M), (b64, a64, i2, g2, out2, out1, N)):
        if g is None:
            continue
        idx = idx.astype(np.int64)
        t = (2.0 * g.astype(np.float64))[..., None] * (q - r[bi, idx])   # (B,n,3): the term grad_xyz[query] += t, grad_xyz[ref[idx]] -= t
        t = t.ravel()
        oq[0] += t
        oq[1] += 1
        oq[2] += np.abs(t)
        flat = (((bi * m + idx) * 3)[..., None] + np.arange(3)).ravel()
        np.add.at(orf[0], flat, -t)
        np.add.at(orf[1], flat, 1)
        np.add.at(orf[2], flat, np.abs(t))
    return tuple(tuple(x.reshape(B, n, 3) for x in o) for o, n in ((out1, N), (out2, M)))


def _grad_bound(k, S):
    """The kernel forms each term as fl(g2 * fl(p1 - p2)) with g2 = 2 g exact: two roundings, |term - exact| <= (2 u + u^2) |exact|.  It then adds
    the k terms of an element with fp32 atomics in some order: k - 1 roundings (the first add into the memset's 0 is exact), each at most u times a
    partial sum, itself at most the sum of the rounded terms' magnitudes.  Together (k + 1) u S to first order; (k + 2) with 1.01 for the second-order
    terms is the asserted bound, plus the smallest normal for a flushed or gradually underflowed term."""
    return (k + 2) * U * S * 1.01 + 2.0 ** -126


def _assert_grad_within_bound(got, ref_k_S, what):
    """Element-wise |got - ref64| <= bound; returns the largest |err| / bound."""
    ref, k, S = ref_k_S
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - ref)
    bound = _grad_bound(k, S)
    ratio = float((err / bound).max())
    print(f"chamfer backward {what}: max |err| / bound = {ratio:.4f} (k up to {int(k.max())})")
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert ratio <= 1.0, (what, ratio, worst, float(err[worst]), float(bound[worst]))
    return ratio


@functools.lru_cache(maxsize=None)
def _funnel_case():
    """Every query's nearest neighbour is reference 0: k = N + 1 on that row of grad_xyz2 (N terms of the first direction, one of its own)."""
    from oracle import pointnet2 as o
    rng = np.random.Generator(np.random.PCG64(9))
    a = (0.1 * rng.standard_normal((2, 700, 3))).astype(np.float32)
    b = (100 + rng.standard_normal((2, 40, 3))).astype(np.float32)
    b[:, 0] = 0.01
    out = o.chamfer_forward(a, b)
    assert (out[2] == 0).all()
    return _frozen(a, b, *out)


@pytest.mark.parametrize("case", ["2x500x3000", "256x300x1030", "funnel"])
def test_backward_within_the_derived_bound_of_float64(case):
    a, b, _, _, i1, i2 = {"2x500x3000": lambda: _normal_case(2, 500, 3000), "256x300x1030": lambda: _normal_case(256, 300, 1030),
                          "funnel": _funnel_case}[case]()
    rng = np.random.Generator(np.random.PCG64(len(case)))
    g1 = rng.standard_normal(i1.shape).astype(np.float32)
    g2 = rng.standard_normal(i2.shape).astype(np.float32)
    gx1, gx2 = _backward(a, b, i1, i2, g1, g2)
    ref1, ref2 = _grad_ref(a, b, i1, i2, g1, g2)
    if case == "funnel":
        assert int(ref2[1].max()) == a.shape[1] + 1
    _assert_grad_within_bound(gx1, ref1, case + " grad_xyz1")
    _assert_grad_within_bound(gx2, ref2, case + " grad_xyz2")


# ---- (f) the backward's grid-stride loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stride_case():
    """One cloud of 8192 x 256 + 300 points (the backward's grid is capped at 8192 workgroups of 256: the last 300 points are reached only by the
    second trip of the stride loop) against one of 4096, with synthetic valid indices."""
    rng = np.random.Generator(np.random.PCG64(31))
    big, small = 8192 * 256 + 300, 4096
    x_big = rng.standard_normal((1, big, 3), dtype=np.float32)
    x_small = rng.standard_normal((1, small, 3), dtype=np.float32)
    i_big = rng.integers(0, small, (1, big), dtype=np.int32)    # of every big point: a small point
    i_small = rng.integers(0, big, (1, small), dtype=np.int32)  # of every small point: a big point
    g_big = rng.standard_normal((1, big), dtype=np.float32)
    return _frozen(x_big, x_small, i_big, i_small, g_big)


@pytest.mark.parametrize("big_side", [1, 2])
def test_backward_grid_stride_loop(big_side):
    """big_side = 1: xyz1 is the long cloud and grad_dist2 = 0 (the first launch strides); 2: the roles swapped (the second launch strides)."""
    x_big, x_small, i_big, i_small, g_big = _stride_case()
    zeros = np.zeros(i_small.shape, np.float32)
    if big_side == 1:
        gx_big, gx_small = _backward(x_big, x_small, i_big, i_small, g_big, zeros)
        ref_big, ref_small = _grad_ref(x_big, x_small, i_big, i_small, g_big, None)
    else:
        gx_small, gx_big = _backward(x_small, x_big, i_small, i_big, zeros, g_big)
        ref_small, ref_big = _grad_ref(x_small, x_big, i_small, i_big, None, g_big)
    _assert_grad_within_bound(gx_big, ref_big, f"stride side {big_side}, long cloud")
    _assert_grad_within_bound(gx_small, ref_small, f"stride side {big_side}, short cloud")
    # without the stride loop these rows stay at the memset's zero
    tail = gx_big[0, -300:]
    assert np.all(np.any(tail != 0, axis=1))
    _assert_grad_within_bound(tail, tuple(x[0, -300:] for x in ref_big), f"stride side {big_side}, last 300 points")


# ---- (g) the evaluation on the <2> path -------------------------------------------------------------------------------------------------
def test_pairwise_cd_on_the_evaluations_launch_path(monkeypatch):
    """17 x 17 clouds of 96 points = 289 pairs in one launch of the default PAIRS_PER_LAUNCH: 289 x ceil(96 / 512) >= 256 workgroups, <2>.
    Bound against float64: coordinates in [0, 1], so each of the three squared terms is at most 1 and rounded once and the mean of 96 fp32 values
    adds rounding of the same order: 4 x 2^-24 x 3 absolute covers both (nearest-neighbour distances of 96 uniform points are far below 1).
    Launches of 64 pairs take <1> (64 workgroups): the matrix must not depend on it."""
    from difffacto_amd import evaluation as ev
    from oracle import pointnet2 as o
    rng = np.random.Generator(np.random.PCG64(17))
    smp = rng.uniform(0, 1, (17, 96, 3)).astype(np.float32)
    ref = rng.uniform(0, 1, (17, 96, 3)).astype(np.float32)
    S, R = _dev(smp), _dev(ref)
    assert ev.PAIRS_PER_LAUNCH >= 289
    cd = ev._pairwise_EMD_CD_(S, R, batch_size=32)[0]
    s64, r64 = smp.astype(np.float64), ref.astype(np.float64)
    brute = np.zeros((17, 17))
    for i in range(17):
        d = ((s64[i][None, :, None] - r64[:, None]) ** 2).sum(-1)   # (17 refs, 96 sample points, 96 ref points)
        brute[i] = d.min(2).mean(1) + d.min(1).mean(1)
    err = np.abs(cd.cpu().numpy().astype(np.float64) - brute).max()
    print(f"pairwise CD vs float64 brute force: max abs err = {err:.3e} (bound {4 * U * 3:.3e})")
    assert err <= 4 * U * 3
    # the per-point distances of that very launch, bit-exact
    i, r = np.divmod(np.arange(289), 17)
    pa, pb = np.ascontiguousarray(smp[i]), np.ascontiguousarray(ref[r])
    _assert_forward_exact(_forward(pa, pb), o.chamfer_forward(pa, pb), "289 pairs")
    monkeypatch.setattr(ev, "PAIRS_PER_LAUNCH", 64)
    assert torch.equal(ev._pairwise_EMD_CD_(S, R, batch_size=32)[0], cd)
