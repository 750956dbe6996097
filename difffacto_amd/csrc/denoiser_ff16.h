// Layout algebra of the bf16 chain kernels' feed-forward on v_mfma_f32_16x16x32_{bf16,f16}: where every weight element sits in a
// streaming record, which fragment every MFMA of an M slot takes, and which accumulator it feeds.  Plain C++17, no HIP includes
// (like denoiser_plan.h): the pack kernels (denoiser_setup.hip), the device fragment functions (denoiser_kernel.hip) and the host
// test (tests/test_ff16_layout_cpu.py through dfx_debug_ff16_*) all compile these lines.
//
// Lane semantics (l = lane, j = 0..7 the element of a 4-VGPR operand, r the accumulator register):
//                   v_mfma_f32_32x32x16                              v_mfma_f32_16x16x32
//     A   row l&31, k 8(l>>5)+j                         row l&15, k 8(l>>4)+j
//     B   k 8(l>>5)+j, col l&31                         k 8(l>>4)+j, col l&15
//     C/D col l&31, row (r&3)+8(r>>2)+4(l>>5), r < 16   col l&15, row 4(l>>4)+r, r < 4
//
// The chain kernels hold one point per lane, l&31, with the half-wave hf = l>>5 selecting the channels (denoiser_internal.h).  The
// feed-forward works on two N-tiles of 16 points instead.  v_permlane16_swap_b32 X, Y exchanges the odd 16-lane rows of X with the
// even rows of Y: X' = (X0, Y0, X2, Y2) holds points 0..15 and Y' = (X1, Y1, X3, Y3) points 16..31; lane row R of either holds what
// register (R&1 ? Y : X) held for half-wave R>>1.  The swap is its own inverse.
//
//   xn (GEMM1's B):  X = unit 0, Y = unit 1 of channel tile c, VGPR by VGPR.  Unit n then IS the B operand of N-tile n for K step c,
//       and K slot 8R+j carries channel 32c + (j&3) + 8(j>>2) + 16(R&1) + 4(R>>1): W1's A fragment for M-tile m (hidden units
//       16m..16m+15 of the chunk) is, lane for lane, what unit R&1 of the 32x32x16 tile held for half-wave R>>1 (w1_decode).
//   a, g (GEMM1's D): 16 registers each as now: quad 2n+m = N-tile n, M-tile m; register r of lane row R = hidden unit 16m+4R+r.
//       The GELU is elementwise and packs pairs in register order, so hid.f[n] = quads (n, 0), (n, 1) is GEMM2's B operand of N-tile
//       n with K slot 8R+j = hidden unit 16(j>>2) + 4R + (j&3) (w2_decode's k).
//   h (GEMM2's C/D): X = h[c][8t+r], Y = h[c][8t+4+r] (r < 4, t < 2).  X' / Y' = quads 2t / 2t+1 of h[c] are the accumulators of
//       M-tile (c, t) for N-tile 0 / 1, and output row i = 4R+r is channel 32c + 16t + rowperm(i) (w2_decode's row).  The same
//       swaps bring h back.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DFX_FF16_HD __host__ __device__
#else
#define DFX_FF16_HD
#endif

namespace dfx {
namespace ff16 {

constexpr int CH = 128, HID = 512, CHUNKS = 16, REC_TILES = 12, SKEW = 1;   // (static_asserted against denoiser_internal.h where both are seen)
enum { LAYOUT_32X32X16 = 0, LAYOUT_16X16X32 = 1 };

DFX_FF16_HD constexpr int rowperm(int i) { return (i & 3) + 8 * ((i >> 2) & 1) + 4 * (i >> 3); }

// position idx (unit * 512 + lane * 8 + element) of a 32 x 32 bf16 / fp16 weight tile -> row i, column kk of the tile
// v_mfma_f32_32x32x16 A operand: unit = K half
DFX_FF16_HD inline void tile32_decode(int idx, int &i, int &kk) {
  const int unit = idx >> 9, lane = (idx >> 3) & 63, e = idx & 7;
  i = lane & 31;
  kk = (e & 3) + 16 * unit + 8 * (e >> 2) + 4 * (lane >> 5);
}
// W1, v_mfma_f32_16x16x32_bf16 A operand: unit = M-tile, K slot 8R+j = the channel xn's swapped registers carry there
DFX_FF16_HD inline void w1_decode(int idx, int &i, int &kk) {
  const int unit = idx >> 9, lane = (idx >> 3) & 63, j = idx & 7, R = lane >> 4;
  i = 16 * unit + (lane & 15);
  kk = (j & 3) + 8 * (j >> 2) + 16 * (R & 1) + 4 * (R >> 1);
}
// W2, v_mfma_f32_16x16x32_f16 A operand: unit = M-tile (half of the 32 output channels), rows in the order h's swapped quads hold them
DFX_FF16_HD inline void w2_decode(int idx, int &i, int &kk) {
  const int unit = idx >> 9, lane = (idx >> 3) & 63, j = idx & 7, R = lane >> 4;
  i = 16 * unit + rowperm(lane & 15);
  kk = 16 * (j >> 2) + 4 * R + (j & 3);
}

// Destination (element index into a block's FF_STAGES records) and source (row, column of the parameter) of pack thread gi
struct Src {
  long long di;
  int row, col;
};
// W1 (1024 x 128): tiles part*4 + c of record u
DFX_FF16_HD inline Src w1_source(long long gi, int layout) {
  const int tile = (int)(gi >> 10), idx = (int)(gi & 1023);
  int i, kk;
  if (layout == LAYOUT_16X16X32) w1_decode(idx, i, kk);
  else tile32_decode(idx, i, kk);
  const int c = tile & 3, part = (tile >> 2) & 1, u = tile >> 3;
  return Src{((long long)(u * REC_TILES + part * 4 + c) << 10) + idx, part * HID + 32 * u + i, 32 * c + kk};
}
// W2 (128 x 512): tiles 8 + ct of record u + SKEW
DFX_FF16_HD inline Src w2_source(long long gi, int layout) {
  const int tile = (int)(gi >> 10), idx = (int)(gi & 1023);
  int i, kk;
  if (layout == LAYOUT_16X16X32) w2_decode(idx, i, kk);
  else tile32_decode(idx, i, kk);
  const int ct = tile & 3, u = tile >> 2;
  return Src{((long long)((u + SKEW) * REC_TILES + 8 + ct) << 10) + idx, 32 * ct + i, 32 * u + kk};
}
constexpr long long W1_PACK_THREADS = (long long)CHUNKS * 8 * 1024, W2_PACK_THREADS = (long long)CHUNKS * 4 * 1024;

// The packed value of W1' = W1 diag(gamma3) at (row, col), before the scale and the rounding.  fold: channel 127's K slot carries the constant 1
// and the weight there is b1' = b1 + W1 beta3; every other weight has W1'[.][127] subtracted (denoiser_kernel.hip: bias_slot_one).
DFX_FF16_HD inline float w1_value(const float *W1, const float *g3, const float *b1, const float *be3, int row, int col, int fold) {
  if (!fold) return W1[(size_t)row * CH + col] * g3[col];
  if (col == CH - 1) {
    float acc = 0.f;
    for (int k = 0; k < CH; ++k) acc = fmaf(W1[(size_t)row * CH + k], be3[k], acc);
    return b1[row] + acc;
  }
  const float w127 = W1[(size_t)row * CH + (CH - 1)] * g3[CH - 1];
  return W1[(size_t)row * CH + col] * g3[col] - w127;
}

// ---- fragments (uint4 units relative to a lane's record pointer; a tile = 128, a unit = 64) ----
// W2 tile ct = i&3, unit i>>2: consecutive MFMAs go to different tiles of h.  W1 unit order (c, unit, part) -> tile part*4 + c
// (half 0: c = 0, 1; half 1: c = 2, 3).
DFX_FF16_HD constexpr int w2_frag(int i) { return (8 + (i & 3)) * 128 + (i >> 2) * 64; }
DFX_FF16_HD constexpr int w1_frag(int i, int half) { return ((i & 1) * 4 + 2 * half + (i >> 2)) * 128 + ((i >> 1) & 1) * 64; }
// m-th fragment of a full FF record: eight groups of  GEMM2 fragment k | GEMM1 fragments 2k, 2k+1
DFX_FF16_HD constexpr int ff_frag(int m) {
  const int k = m / 3, r = m % 3;
  if (r == 0) return w2_frag(k);
  const int e = 2 * k + r - 1;
  return w1_frag(e & 7, e >> 3);
}
// What the two MFMAs (N-tile 0, 1) of a fragment do.  GEMM1 fragment e = 0..15: accumulator part (0 = a, 1 = g), M-tile mt, K step c
// (= channel tile of xn): quads 2n + mt of a / g.  GEMM2 fragment i = 0..7: output tile ct of h, M-tile mt: quads 2 mt + n of h[ct].
struct Op {
  int frag, part, mt, c;
};
DFX_FF16_HD constexpr Op gemm1_op(int e) { return Op{w1_frag(e & 7, e >> 3), e & 1, (e >> 1) & 1, 2 * (e >> 3) + ((e & 7) >> 2)}; }
DFX_FF16_HD constexpr Op gemm2_op(int i) { return Op{w2_frag(i), -1, i >> 2, i & 3}; }

}  // namespace ff16
}  // namespace dfx
