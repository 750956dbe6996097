"""Layout algebra of the bf16 chain kernels' feed-forward on v_mfma_f32_16x16x32 (csrc/denoiser_ff16.h), on the host: numpy emulates the lane
semantics of both MFMA shapes and of the 16-lane row swap, packs small integer weights with the library's own pack functions
(dfx_debug_ff16_pack_w1 / _w2, the lines k_pack_w1 / k_pack_w2 compile) and walks the fragments in the order and with the accumulators the
kernels use (dfx_debug_ff16_slot_ops, the lines ff_m compiles).  Everything is exact in fp32, so every check is an equality:
  (a) GEMM1 and GEMM2 equal the plain matrix products, element by element;
  (b) swap, feed-forward, swap back leaves every channel of every point of h in its old register and lane;
  (c) no output of a point depends on another point's input;
  (d) the packs with and without the W1 bias fold hold what the 32x32x16 pack held, tile by tile, up to the stated permutation.
The reading of the swap instruction itself (odd rows of the first operand <-> even rows of the second) is from the ISA text; that the hardware
does this is checked on the GPU (tests/test_gpu_ff16_points.py)."""
import ctypes

import numpy as np
import pytest

CH, HID, CHUNKS, REC_TILES = 128, 512, 16, 12
L = np.arange(64)
HF, PT = L >> 5, L & 31          # one point per lane: half-wave, point
ROW, LI = L >> 4, L & 15         # 16-lane row, lane in the row


def rho(r, hf):
    return (r & 3) + 8 * (r >> 2) + 4 * hf


@pytest.fixture(scope="module")
def lib():
    from difffacto_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lib.dfx_debug_ff16_pack_w1.restype = None
    lib.dfx_debug_ff16_pack_w1.argtypes = [fp, fp, fp, fp, ctypes.c_int, ctypes.c_int, fp]
    lib.dfx_debug_ff16_pack_w2.restype = None
    lib.dfx_debug_ff16_pack_w2.argtypes = [fp, ctypes.c_int, fp]
    lib.dfx_debug_ff16_slot_ops.restype = None
    lib.dfx_debug_ff16_slot_ops.argtypes = [ip]
    return lib


def _fp(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def pack_w1(lib, W1, g3, b1, be3, fold, layout):
    out = np.full(((CHUNKS + 1) * REC_TILES * 1024,), np.nan, np.float32)
    lib.dfx_debug_ff16_pack_w1(_fp(W1), _fp(g3), _fp(b1), _fp(be3), fold, layout, _fp(out))
    return out.reshape(CHUNKS + 1, REC_TILES, 2, 64, 8)   # record, tile, unit, lane, element


def pack_w2(lib, W2, layout):
    out = np.full(((CHUNKS + 1) * REC_TILES * 1024,), np.nan, np.float32)
    lib.dfx_debug_ff16_pack_w2(_fp(W2), layout, _fp(out))
    return out.reshape(CHUNKS + 1, REC_TILES, 2, 64, 8)


def slot_ops(lib):
    o = np.zeros((24, 5), np.int32)
    lib.dfx_debug_ff16_slot_ops(o.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return o


# ---- lane semantics (programming guide section 3) ----
def mfma32(A, B, C):
    """v_mfma_f32_32x32x16: A, B (64 lanes, 8), C (16, 64) -> D"""
    Am, Bm = np.zeros((32, 16), np.float32), np.zeros((16, 32), np.float32)
    for j in range(8):
        Am[L & 31, 8 * (L >> 5) + j] = A[:, j]
        Bm[8 * (L >> 5) + j, L & 31] = B[:, j]
    D = Am @ Bm
    r = np.arange(16)[:, None]
    return C + D[(r & 3) + 8 * (r >> 2) + 4 * (L >> 5)[None, :], (L & 31)[None, :]]


def mfma16(A, B, C):
    """v_mfma_f32_16x16x32: A, B (64 lanes, 8), C (4, 64) -> D"""
    Am, Bm = np.zeros((16, 32), np.float32), np.zeros((32, 16), np.float32)
    for j in range(8):
        Am[L & 15, 8 * (L >> 4) + j] = A[:, j]
        Bm[8 * (L >> 4) + j, L & 15] = B[:, j]
    D = Am @ Bm
    r = np.arange(4)[:, None]
    return C + D[4 * (L >> 4)[None, :] + r, (L & 15)[None, :]]


def row_swap(x, y):
    """v_permlane16_swap_b32 x, y: the odd 16-lane rows of x <-> the even rows of y"""
    x, y = x.copy(), y.copy()
    for k in (0, 2):
        odd, even = slice(16 * (k + 1), 16 * (k + 2)), slice(16 * k, 16 * (k + 1))
        x[..., odd], y[..., even] = y[..., even].copy(), x[..., odd].copy()
    return x, y


def test_row_swap_is_its_own_inverse_and_sorts_points_into_n_tiles():
    x, y = L.astype(np.float32), 100 + L.astype(np.float32)
    xs, ys = row_swap(x, y)
    assert np.array_equal(xs, np.concatenate([x[0:16], y[0:16], x[32:48], y[32:48]]))
    assert np.array_equal(ys, np.concatenate([x[16:32], y[16:32], x[48:64], y[48:64]]))
    xb, yb = row_swap(xs, ys)
    assert np.array_equal(xb, x) and np.array_equal(yb, y)


# ---- register images of the kernels' state, one point per lane (denoiser_internal.h) ----
def h_regs(H):
    """H (128 channels, 32 points) -> h[c][r][lane]"""
    h = np.zeros((4, 16, 64), np.float32)
    for c in range(4):
        for r in range(16):
            h[c, r] = H[32 * c + rho(r, HF), PT]
    return h


def xn_regs(X):
    """LayerNorm output X (128, 32) -> Act xn[c].f[q][lane][e] (register 8q + e of tile c)"""
    xn = np.zeros((4, 2, 64, 8), np.float32)
    for c in range(4):
        for q in range(2):
            for e in range(8):
                xn[c, q, :, e] = X[32 * c + rho(8 * q + e, HF), PT]
    return xn


def ff16_rows_xn(xn):
    out = xn.copy()
    for c in range(4):
        for e in range(8):   # (the instruction moves 32-bit registers = element pairs; element by element is the same movement)
            out[c, 0, :, e], out[c, 1, :, e] = row_swap(xn[c, 0, :, e], xn[c, 1, :, e])
    return out


def ff16_rows_h(h):
    out = h.copy()
    for c in range(4):
        for t in range(2):
            for r in range(4):
                out[c, 8 * t + r], out[c, 8 * t + 4 + r] = row_swap(h[c, 8 * t + r], h[c, 8 * t + 4 + r])
    return out


def frag(rec, off):
    """fragment at uint4 offset `off` from the lane's record pointer: (64 lanes, 8)"""
    return rec[off // 128, (off % 128) // 64]


def feed_forward(lib, P1, P2, X, H, act):
    """The feed-forward of one block as k_denoise_pipe runs it on the packed records P1 (W1 tiles) / P2 (W2 tiles): returns (h registers back in
    the one-point-per-lane form, per chunk the a / g registers).  `act` stands in for the (elementwise) GEGLU."""
    ops = slot_ops(lib)
    xn = ff16_rows_xn(xn_regs(X))
    h = ff16_rows_h(h_regs(H))
    acc = np.zeros((2, 16, 64), np.float32)   # a, g: quad 2n + m
    hid = None
    seen = []
    for j in range(CHUNKS + 1):               # record j: GEMM2 of chunk j-1 | GEMM1 of chunk j, in the M slot's fragment order
        new = np.zeros_like(acc)
        started = set()
        for off, gemm, part, mt, c in ops:
            if gemm == 2 and j > 0:
                for n in range(2):
                    q = 2 * mt + n
                    h[c, 4 * q:4 * q + 4] = mfma16(frag(P2[j], off), hid[n], h[c, 4 * q:4 * q + 4])
            if gemm == 1 and j < CHUNKS:
                for n in range(2):
                    q = 2 * n + mt
                    assert (c == 0) == ((part, q) not in started), "K steps in order, the first one starts from C = 0"
                    started.add((part, q))
                    new[part, 4 * q:4 * q + 4] = mfma16(frag(P1[j], off), xn[c, n], 0 if c == 0 else new[part, 4 * q:4 * q + 4])
        if j < CHUNKS:
            acc = new
            seen.append(acc.copy())
            y = act(acc[0], acc[1])                                   # elementwise on the 16 registers, like the GELU
            hid = [y[8 * n:8 * n + 8].T.copy() for n in range(2)]     # hid.f[n] = registers 8n .. 8n+7 in order: (64 lanes, 8)
    return ff16_rows_h(h), seen


def _weights(seed, fold):
    rng = np.random.default_rng(seed)
    W1 = rng.integers(-2, 3, (2 * HID, CH)).astype(np.float32)
    W2 = rng.integers(-2, 3, (CH, HID)).astype(np.float32)
    g3 = rng.integers(1, 3, CH).astype(np.float32)
    b1 = rng.integers(-2, 3, 2 * HID).astype(np.float32)
    be3 = rng.integers(-1, 2, CH).astype(np.float32)
    W1p = W1 * g3[None, :]                                            # what GEMM1 multiplies xn by, written down independently of the pack
    if fold:
        W1p = W1p - W1p[:, CH - 1:CH]
        W1p[:, CH - 1] = b1 + W1 @ be3
    return W1, W2, g3, b1, be3, W1p


def ACT(a, g):
    """integer-valued stand-in for a * gelu(g): elementwise and not symmetric in (a, g); small enough that GEMM2 stays exact in fp32"""
    return a + 3 * g


@pytest.mark.parametrize("fold", [1, 0])
def test_feed_forward_on_16x16x32_equals_the_matrix_products(lib, fold):
    W1, W2, g3, b1, be3, W1p = _weights(1 + fold, fold)
    rng = np.random.default_rng(7)
    X = rng.integers(-2, 3, (CH, 32)).astype(np.float32)
    if fold:
        X[CH - 1] = 1.0    # bias_slot_one
    H = rng.integers(-50, 51, (CH, 32)).astype(np.float32)
    P1, P2 = pack_w1(lib, W1, g3, b1, be3, fold, 1), pack_w2(lib, W2, 1)
    h_out, seen = feed_forward(lib, P1, P2, X, H, ACT)
    AG = W1p @ X                                                      # (1024, 32)
    for u, acc in enumerate(seen):                                    # (a) GEMM1: quad 2n + m, register r of lane row R = hidden unit 16m + 4R + r, point 16n + lane
        for part in range(2):
            for n in range(2):
                for m in range(2):
                    for r in range(4):
                        want = AG[part * HID + 32 * u + 16 * m + 4 * ROW + r, 16 * n + LI]
                        assert np.array_equal(acc[part, 4 * (2 * n + m) + r], want), (u, part, n, m, r)
    hidden = ACT(AG[:HID], AG[HID:])
    assert np.abs(W2).sum(1).max() * np.abs(hidden).max() < 2 ** 24   # exact in fp32
    want_h = h_regs(H + W2 @ hidden)                                  # (a) GEMM2 and (b): every channel of every point back in its register and lane
    assert np.array_equal(h_out, want_h)


def test_the_32x32x16_pack_and_shape_give_the_same_products(lib):
    """The form the kernels had: both units of a tile as the A operands of two K = 16 steps, one point per lane."""
    W1, W2, g3, b1, be3, W1p = _weights(5, 1)
    X = np.random.default_rng(9).integers(-2, 3, (CH, 32)).astype(np.float32)
    P1, xn, AG = pack_w1(lib, W1, g3, b1, be3, 1, 0), xn_regs(X), W1p @ X
    for u, part in ((0, 0), (9, 1)):
        acc = np.zeros((16, 64), np.float32)
        for c in range(4):
            for q in range(2):
                acc = mfma32(P1[u, part * 4 + c, q], xn[c, q], acc)
        for r in range(16):
            assert np.array_equal(acc[r], AG[part * HID + 32 * u + rho(r, HF), PT])


def test_swap_zero_feed_forward_swap_returns_h(lib):
    z = np.zeros
    P1 = pack_w1(lib, z((2 * HID, CH), np.float32), np.ones(CH, np.float32), z(2 * HID, np.float32), z(CH, np.float32), 0, 1)
    P2 = pack_w2(lib, z((CH, HID), np.float32), 1)
    H = np.arange(CH * 32, dtype=np.float32).reshape(CH, 32)
    h_out, _ = feed_forward(lib, P1, P2, np.ones((CH, 32), np.float32), H, ACT)
    assert np.array_equal(h_out, h_regs(H))


def test_no_point_sees_another_points_input(lib):
    W1, W2, g3, b1, be3, _ = _weights(3, 1)
    P1, P2 = pack_w1(lib, W1, g3, b1, be3, 1, 1), pack_w2(lib, W2, 1)
    rng = np.random.default_rng(8)
    X = rng.integers(-2, 3, (CH, 32)).astype(np.float32)
    H = rng.integers(-50, 51, (CH, 32)).astype(np.float32)
    base, _ = feed_forward(lib, P1, P2, X, H, ACT)
    for p in (0, 15, 16, 31):
        X2, H2 = X.copy(), H.copy()
        X2[:, p] += rng.integers(1, 4, CH)
        H2[:, p] += 1000
        out, _ = feed_forward(lib, P1, P2, X2, H2, ACT)
        changed = (out != base).any(axis=(0, 1))
        assert np.array_equal(changed, PT == p), p   # both half-waves' lanes of point p, and nothing else


@pytest.mark.parametrize("fold", [0, 1])
def test_packs_hold_what_the_32x32x16_pack_held_up_to_the_permutation(lib, fold):
    rng = np.random.default_rng(11)
    W1 = rng.standard_normal((2 * HID, CH)).astype(np.float32)
    W2 = rng.standard_normal((CH, HID)).astype(np.float32)
    g3, b1, be3 = (rng.standard_normal(n).astype(np.float32) for n in (CH, 2 * HID, CH))
    old1, new1 = pack_w1(lib, W1, g3, b1, be3, fold, 0), pack_w1(lib, W1, g3, b1, be3, fold, 1)
    old2, new2 = pack_w2(lib, W2, 0), pack_w2(lib, W2, 1)
    assert np.array_equal(np.isnan(old1), np.isnan(new1)) and np.array_equal(np.isnan(old2), np.isnan(new2))   # same tiles, same offsets
    assert not np.isnan(new1[:CHUNKS, :8]).any() and np.isnan(new1[CHUNKS]).all() and np.isnan(new1[:, 8:]).all()
    assert not np.isnan(new2[1:, 8:]).any() and np.isnan(new2[0]).all() and np.isnan(new2[:, :8]).all()
    # the old pack is the documented one (denoiser_internal.h): unit q, lane (i, hf), element e = W[row0 + i][k0 + (e&3) + 16q + 8(e>>2) + 4hf]
    e = np.arange(8)
    if not fold:
        for u, part, c in ((0, 0, 0), (5, 1, 2), (15, 1, 3)):
            for q in range(2):
                k = (e & 3)[None, :] + 16 * q + 8 * (e >> 2)[None, :] + 4 * HF[:, None]
                want = (W1 * g3[None, :])[part * HID + 32 * u + PT[:, None], 32 * c + k]
                assert np.array_equal(old1[u, part * 4 + c, q], want)
    for u, ct in ((0, 0), (7, 3), (15, 1)):
        for q in range(2):
            k = (e & 3)[None, :] + 16 * q + 8 * (e >> 2)[None, :] + 4 * HF[:, None]
            assert np.array_equal(old2[u + 1, 8 + ct, q], W2[32 * ct + PT[:, None], 32 * u + k])
    # W1: the fragment of M-tile m holds, lane row R, what unit R&1 of the old tile held for half-wave R>>1 and rows 16m .. 16m+15
    for m in range(2):
        src_lane = 32 * (ROW >> 1) + 16 * m + LI
        assert np.array_equal(new1[:CHUNKS, :8, m], old1[:CHUNKS, :8][:, :, ROW & 1, src_lane])
    # W2: row 16t + rowperm(lane & 15), k = 16(j>>2) + 4R + (j&3) of the tile, wherever the old pack kept that element
    rowperm = (LI & 3) + 8 * ((LI >> 2) & 1) + 4 * (LI >> 3)
    for t in range(2):
        i = (16 * t + rowperm)[:, None]
        kk = 16 * (e >> 2)[None, :] + 4 * ROW[:, None] + (e & 3)[None, :]
        o_unit, o_lane, o_e = kk >> 4, i + 32 * ((kk >> 2) & 1), (kk & 3) + 4 * ((kk >> 3) & 1)
        assert np.array_equal(new2[1:, 8:, t], old2[1:, 8:][:, :, o_unit, o_lane, o_e])
