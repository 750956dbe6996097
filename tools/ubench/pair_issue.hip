// Micro-benchmark of an MFMA stream with two point tiles per wavefront (the schedule of a since-retired chain kernel): ONE wavefront per SIMD (256 threads, 512 registers) issuing pairs of
// v_mfma_f32_32x32x16 that share their A fragment (two point tiles), the fragment refilled in place from LDS behind the pair.
// Variants: C/D in the accumulator file or in VGPRs, B from the accumulator file or VGPRs, with / without the refill, NV packed
// fp16 VALU fillers per MFMA.  Prints shader cycles per MFMA (floor: 32).
// F32 rows: on top of the stream "refill per MFMA, 5 v_pk per MFMA", the same fp32 arithmetic (four fused multiply-adds on random operands
// per MFMA) issued as 4 v_fma_f32 or as 2 v_pk_fma_f32 — what a packed fp32 instruction costs the full chip against the two scalar ones
// it replaces.  M16 rows: every v_mfma_f32_32x32x16 replaced by the two v_mfma_f32_16x16x32 (one per 16-point N-tile, same A fragment)
// of the chain kernels' feed-forward; "per MFMA" then means per such pair.
// ORDER rows (pair_issue <iters> order): the 16x16x32 stream with the feed-forward's mix (one refill and 5 v_pk per fragment, two MFMAs per fragment: one per
// N-tile b0 / b1), the SAME MFMAs and accumulators in three issue orders — what the order of operand changes costs the full chip:
//   (a) today's:        (A1,N0) (A1,N1) (A2,N0) (A2,N1)             A held for two MFMAs, B changes at every one: 1.5 operand changes per MFMA
//   (b) boustrophedon:  (A1,N0) (A2,N0) (A2,N1) (A1,N1) (A3,N1) ... exactly one operand changes per MFMA
//   (c) upper bracket:  (A1,N0) (A2,N1) (A3,N0) (A4,N1) (A1,N1) ... both operands change at every MFMA
// Every row three times in one process, the rows interleaved, with each run's time and the row's spread.
// Usage: pair_issue [iters = 2000] [order]
// Build: hipcc --offload-arch=gfx950 -O3 pair_issue.hip -o _build/pair_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

#define FILL "v_pk_fma_f16 %[t0], %[g0], %[g1], %[t0]\n v_pk_mul_f16 %[t1], %[g0], %[t1]\n v_pk_fma_f16 %[t2], %[g1], %[g0], %[t2]\n v_pk_add_f16 %[t3], %[g1], %[t3]\n v_pk_fma_f16 %[t4], %[g0], %[g1], %[t4]\n"
#define FILL3 "v_pk_fma_f16 %[t0], %[g0], %[g1], %[t0]\n v_pk_mul_f16 %[t1], %[g0], %[t1]\n v_pk_fma_f16 %[t2], %[g1], %[g0], %[t2]\n"

// ACC: 0 = C/D in VGPRs, 1 = accumulator file.  BA: B operand from the accumulator file.  LDS: refill behind every pair.
// NV: 0, 3 or 5 fillers behind every MFMA.  PAIR: 1 = the two MFMAs of a pair share A; 0 = every MFMA its own A (+ its own refill)
// F32: 0 = none, 1 = 4 v_fma_f32, 2 = 2 v_pk_fma_f32 behind every MFMA.  M16: 1 = pairs of 16x16x32 (C/D in the accumulator file)
typedef float v2f __attribute__((ext_vector_type(2)));
template <int ACC, int BA, int LDS, int NV, int PAIR, int F32 = 0, int M16 = 0, int ORD = 0>
__global__ void __launch_bounds__(256, 1) k(unsigned long long *out, int iters) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  for (int i = threadIdx.x; i < 32 * 1024 / 4; i += blockDim.x) {
    unsigned hsh = (i * 2654435761u) ^ (i >> 3) * 40503u;
    reinterpret_cast<unsigned *>(smem)[i] = (hsh & 0x807f807fu) | 0x3f003f00u | ((hsh >> 9) & 0x00800080u);
  }
  __syncthreads();
  const unsigned lane = threadIdx.x & 63;
  unsigned la = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem + lane * 16;
  v16f c0 = {0}, c1 = c0, c2 = c0, c3 = c0;
  const v4f *fs = reinterpret_cast<const v4f *>(smem) + lane;
  v4f f0 = fs[64], f1 = fs[128], f2 = fs[192], f3 = fs[256], f4 = fs[320], f5 = fs[384], f6 = fs[448], f7 = fs[512], b0 = fs[0], b1 = fs[576];
  unsigned g0 = 0x3c003c00u ^ (threadIdx.x * 0x01230123u & 0x03ff03ffu), g1 = 0x38003800u ^ (threadIdx.x * 0x04560457u & 0x03ff03ffu), t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
  // fp32 fillers: x <- x * u + w with |u| < 1, two (u, w) sets alternating between the two filler sites of a pair, so that x keeps moving
  const unsigned hs = (threadIdx.x + 1) * 2654435761u;
  auto rnd = [&](int i, float lo, float span) { return lo + span * (float)((hs >> (i * 3)) & 1023u) * (1.0f / 1024.0f); };
  const v2f ua = {rnd(0, 0.5f, 0.45f), rnd(1, -0.95f, 0.45f)}, wa = {rnd(2, -1.f, 2.f), rnd(3, -1.f, 2.f)};
  const v2f ub = {rnd(4, -0.95f, 0.45f), rnd(5, 0.5f, 0.45f)}, wb = {rnd(6, -1.f, 2.f), rnd(7, -1.f, 2.f)};
  v2f x0 = {rnd(1, -1.f, 2.f), rnd(4, -1.f, 2.f)}, x1 = {rnd(3, -1.f, 2.f), rnd(6, -1.f, 2.f)};
  float y0 = x0[0], y1 = x0[1], y2 = x1[0], y3 = x1[1];
  v4f d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0, d2 = d0, d3 = d0, d4 = d0, d5 = d0, d6 = d0, d7 = d0;
#define FILL32(u, w)                                                                                                                        \
  do {                                                                                                                                      \
    if (F32 == 1)                                                                                                                           \
      asm volatile("v_fma_f32 %0, %0, %4, %6\n v_fma_f32 %1, %1, %5, %7\n v_fma_f32 %2, %2, %4, %6\n v_fma_f32 %3, %3, %5, %7\n"             \
                   : "+v"(y0), "+v"(y1), "+v"(y2), "+v"(y3) : "v"(u[0]), "v"(u[1]), "v"(w[0]), "v"(w[1]));                                  \
    if (F32 == 2) asm volatile("v_pk_fma_f32 %0, %0, %2, %3\n v_pk_fma_f32 %1, %1, %2, %3\n" : "+v"(x0), "+v"(x1) : "v"(u), "v"(w));        \
  } while (0)
  const unsigned long long tA = __builtin_readcyclecounter();
#define OPSV : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [f0] "+v"(f0), [f1] "+v"(f1), [f2] "+v"(f2), [f3] "+v"(f3), [f4] "+v"(f4), [f5] "+v"(f5), \
               [f6] "+v"(f6), [f7] "+v"(f7), [t0] "+v"(t0), [t1] "+v"(t1), [t2] "+v"(t2), [t3] "+v"(t3), [t4] "+v"(t4) : [la] "v"(la), [b0] "v"(b0), [b1] "v"(b1), [g0] "v"(g0), [g1] "v"(g1)
#define OPSA : [c0] "+a"(c0), [c1] "+a"(c1), [c2] "+a"(c2), [c3] "+a"(c3), [f0] "+v"(f0), [f1] "+v"(f1), [f2] "+v"(f2), [f3] "+v"(f3), [f4] "+v"(f4), [f5] "+v"(f5), \
               [f6] "+v"(f6), [f7] "+v"(f7), [t0] "+v"(t0), [t1] "+v"(t1), [t2] "+v"(t2), [t3] "+v"(t3), [t4] "+v"(t4) : [la] "v"(la), [b0] "v"(b0), [b1] "v"(b1), [g0] "v"(g0), [g1] "v"(g1)
#define OPSVB : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [f0] "+v"(f0), [f1] "+v"(f1), [f2] "+v"(f2), [f3] "+v"(f3), [f4] "+v"(f4), [f5] "+v"(f5), \
               [f6] "+v"(f6), [f7] "+v"(f7), [t0] "+v"(t0), [t1] "+v"(t1), [t2] "+v"(t2), [t3] "+v"(t3), [t4] "+v"(t4) : [la] "v"(la), [b0] "a"(b0), [b1] "a"(b1), [g0] "v"(g0), [g1] "v"(g1)
#define EMIT(str) do { if (ACC) asm volatile(str OPSA); else if (BA) asm volatile(str OPSVB); else asm volatile(str OPSV); } while (0)
#define GRP(ca, cb, fr, fr2, off)                                                                     \
    EMIT("s_waitcnt lgkmcnt(7)\n v_mfma_f32_32x32x16_bf16 %[" ca "], %[" fr "], %[b0], %[" ca "]\n");  \
    if (NV == 5) EMIT(FILL); if (NV == 3) EMIT(FILL3); FILL32(ua, wa);                                \
    EMIT("v_mfma_f32_32x32x16_bf16 %[" cb "], %[" fr2 "], %[b1], %[" cb "]\n");                        \
    if (LDS) EMIT("ds_read_b128 %[" fr "], %[la] offset:" #off "\n");                                 \
    if (LDS && !PAIR) EMIT("ds_read_b128 %[" fr2 "], %[la] offset:" #off "+16384\n");                  \
    if (NV == 5) EMIT(FILL); if (NV == 3) EMIT(FILL3); FILL32(ub, wb);
  // the same group on v_mfma_f32_16x16x32_bf16: accumulators d0..d7 (accumulator file), two MFMAs per fragment (b0 / b1 = the two N-tiles)
#define OPS16 : [d0] "+a"(d0), [d1] "+a"(d1), [d2] "+a"(d2), [d3] "+a"(d3), [d4] "+a"(d4), [d5] "+a"(d5), [d6] "+a"(d6), [d7] "+a"(d7), [f0] "+v"(f0), [f1] "+v"(f1), \
                [f2] "+v"(f2), [f3] "+v"(f3), [f4] "+v"(f4), [f5] "+v"(f5), [f6] "+v"(f6), [f7] "+v"(f7), [t0] "+v"(t0), [t1] "+v"(t1), [t2] "+v"(t2), [t3] "+v"(t3), \
                [t4] "+v"(t4) : [la] "v"(la), [b0] "v"(b0), [b1] "v"(b1), [g0] "v"(g0), [g1] "v"(g1)
#define EMIT16(str) asm volatile(str OPS16)
#define GRP16(da, db, dc, dd, fr, fr2, off)                                                                                             \
    EMIT16("s_waitcnt lgkmcnt(7)\n v_mfma_f32_16x16x32_bf16 %[" da "], %[" fr "], %[b0], %[" da "]\n"                                    \
           " v_mfma_f32_16x16x32_bf16 %[" db "], %[" fr "], %[b1], %[" db "]\n");                                                        \
    if (NV == 5) EMIT16(FILL); FILL32(ua, wa);                                                                                          \
    EMIT16("v_mfma_f32_16x16x32_bf16 %[" dc "], %[" fr2 "], %[b0], %[" dc "]\n v_mfma_f32_16x16x32_bf16 %[" dd "], %[" fr2 "], %[b1], %[" dd "]\n"); \
    if (LDS) EMIT16("ds_read_b128 %[" fr "], %[la] offset:" #off "\n");                                                                  \
    if (LDS && !PAIR) EMIT16("ds_read_b128 %[" fr2 "], %[la] offset:" #off "+16384\n");                                                  \
    if (NV == 5) EMIT16(FILL); FILL32(ub, wb);
  // ORDER rows: one MFMA / one refill / one counted wait per statement (the LDS returns in order: eight refills are in flight at a group's start)
#define MF(d, f, b) EMIT16("v_mfma_f32_16x16x32_bf16 %[" d "], %[" f "], %[" b "], %[" d "]\n");
#define RD(f, off) EMIT16("ds_read_b128 %[" f "], %[la] offset:" #off "\n");
#define WT(n) EMIT16("s_waitcnt lgkmcnt(" #n ")\n");
#define FL EMIT16(FILL);
  // (a): accumulators (fr, b0) (fr, b1) (fr2, b0) (fr2, b1) = da db dc dd; every fragment refilled in place behind its second MFMA
#define GA(da, db, dc, dd, fr, fr2, off) WT(7) MF(da, fr, "b0") MF(db, fr, "b1") RD(fr, off) FL WT(7) MF(dc, fr2, "b0") MF(dd, fr2, "b1") RD(fr2, off + 16384) FL
  // (b): X / Y = the N-tile the group starts / ends with; ax = accumulator of (fr, X), ay of (fr, Y), cx of (fr2, X), cy of (fr2, Y); fr2 is refilled first
#define GB(ax, ay, cx, cy, fr, fr2, X, Y, off) WT(6) MF(ax, fr, X) MF(cx, fr2, X) FL MF(cy, fr2, Y) RD(fr2, off + 16384) MF(ay, fr, Y) RD(fr, off) FL
  // (c): four fragments, pX / pY = accumulator of (fragment p, X / Y)
#define GC(fa, fb, fc, fd, aX, aY, bX, bY, cX, cY, dX, dY, X, Y, o1, o2)                                              \
    WT(7) MF(aX, fa, X) WT(6) MF(bY, fb, Y) FL WT(5) MF(cX, fc, X) WT(4) MF(dY, fd, Y) FL                             \
    MF(aY, fa, Y) RD(fa, o1) MF(bX, fb, X) RD(fb, o1 + 16384) FL MF(cY, fc, Y) RD(fc, o2) MF(dX, fd, X) RD(fd, o2 + 16384) FL
  for (int it = 0; it < iters; ++it) {
    if (ORD == 1) {
      GA("d0", "d1", "d2", "d3", "f0", "f1", 1024) GA("d4", "d5", "d6", "d7", "f2", "f3", 2048) GA("d0", "d1", "d2", "d3", "f4", "f5", 3072)
      GA("d4", "d5", "d6", "d7", "f6", "f7", 4096) GA("d0", "d1", "d2", "d3", "f0", "f1", 5120) GA("d4", "d5", "d6", "d7", "f2", "f3", 6144)
      GA("d0", "d1", "d2", "d3", "f4", "f5", 7168) GA("d4", "d5", "d6", "d7", "f6", "f7", 8192)
    } else if (ORD == 2) {
      GB("d0", "d1", "d2", "d3", "f0", "f1", "b0", "b1", 1024) GB("d5", "d4", "d7", "d6", "f2", "f3", "b1", "b0", 2048)
      GB("d0", "d1", "d2", "d3", "f4", "f5", "b0", "b1", 3072) GB("d5", "d4", "d7", "d6", "f6", "f7", "b1", "b0", 4096)
      GB("d0", "d1", "d2", "d3", "f0", "f1", "b0", "b1", 5120) GB("d5", "d4", "d7", "d6", "f2", "f3", "b1", "b0", 6144)
      GB("d0", "d1", "d2", "d3", "f4", "f5", "b0", "b1", 7168) GB("d5", "d4", "d7", "d6", "f6", "f7", "b1", "b0", 8192)
    } else if (ORD == 3) {
      GC("f0", "f1", "f2", "f3", "d0", "d1", "d2", "d3", "d4", "d5", "d6", "d7", "b0", "b1", 1024, 2048)
      GC("f4", "f5", "f6", "f7", "d1", "d0", "d3", "d2", "d5", "d4", "d7", "d6", "b1", "b0", 3072, 4096)
      GC("f0", "f1", "f2", "f3", "d0", "d1", "d2", "d3", "d4", "d5", "d6", "d7", "b0", "b1", 5120, 6144)
      GC("f4", "f5", "f6", "f7", "d1", "d0", "d3", "d2", "d5", "d4", "d7", "d6", "b1", "b0", 7168, 8192)
    } else if (M16) {
      GRP16("d0", "d1", "d2", "d3", "f0", "f1", 1024) GRP16("d4", "d5", "d6", "d7", "f2", "f3", 2048) GRP16("d0", "d1", "d2", "d3", "f4", "f5", 3072)
      GRP16("d4", "d5", "d6", "d7", "f6", "f7", 4096) GRP16("d0", "d1", "d2", "d3", "f0", "f1", 5120) GRP16("d4", "d5", "d6", "d7", "f2", "f3", 6144)
      GRP16("d0", "d1", "d2", "d3", "f4", "f5", 7168) GRP16("d4", "d5", "d6", "d7", "f6", "f7", 8192)
    } else if (PAIR) {
      GRP("c0", "c1", "f0", "f0", 1024) GRP("c2", "c3", "f1", "f1", 2048) GRP("c0", "c1", "f2", "f2", 3072) GRP("c2", "c3", "f3", "f3", 4096)
      GRP("c0", "c1", "f4", "f4", 5120) GRP("c2", "c3", "f5", "f5", 6144) GRP("c0", "c1", "f6", "f6", 7168) GRP("c2", "c3", "f7", "f7", 8192)
    } else {
      GRP("c0", "c1", "f0", "f1", 1024) GRP("c2", "c3", "f2", "f3", 2048) GRP("c0", "c1", "f4", "f5", 3072) GRP("c2", "c3", "f6", "f7", 4096)
      GRP("c0", "c1", "f0", "f1", 5120) GRP("c2", "c3", "f2", "f3", 6144) GRP("c0", "c1", "f4", "f5", 7168) GRP("c2", "c3", "f6", "f7", 8192)
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n s_nop 15\n s_nop 15" ::: "memory");
  const unsigned long long tB = __builtin_readcyclecounter();
  float s = 0;
  for (int i = 0; i < 16; ++i) s += c0[i] + c1[i] + c2[i] + c3[i];
  s += y0 + y1 + y2 + y3 + x0[0] + x0[1] + x1[0] + x1[1];
  for (int i = 0; i < 4; ++i) s += d0[i] + d1[i] + d2[i] + d3[i] + d4[i] + d5[i] + d6[i] + d7[i];
  s += f0[0] + f1[0] + f2[0] + f3[0] + f4[0] + f5[0] + f6[0] + f7[0] + __uint_as_float(t0 ^ t1 ^ t2 ^ t3 ^ t4);
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = tB - tA;
  if (s == 12345.678f) out[1] = 1;
}

int g_iters = 2000;
template <int ACC, int BA, int LDS, int NV, int PAIR, int F32 = 0, int M16 = 0>
void run(const char *name, int blocks) {
  unsigned long long *d;
  hipMalloc(&d, 16);
  const int iters = g_iters;
  hipFuncSetAttribute(reinterpret_cast<const void *>(k<ACC, BA, LDS, NV, PAIR, F32, M16>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  k<ACC, BA, LDS, NV, PAIR, F32, M16><<<blocks, 256, 64 * 1024>>>(d, 10);
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  hipEventRecord(a);
  k<ACC, BA, LDS, NV, PAIR, F32, M16><<<blocks, 256, 64 * 1024>>>(d, iters);
  hipEventRecord(b);
  hipDeviceSynchronize();
  float ms; hipEventElapsedTime(&ms, a, b);
  unsigned long long h[2];
  hipMemcpy(h, d, 16, hipMemcpyDeviceToHost);
  printf("%-58s blocks %4d: %6.1f cycles / MFMA   (%.3f ms -> %.0f TFLOP/s)\n", name, blocks, (double)h[0] / (iters * 16.0), ms,
         blocks * 4.0 * iters * 16 * 32768.0 / (ms * 1e-3) / 1e12);
  hipFree(d);
}

// ORDER rows: one timed launch -> milliseconds and block 0's shader cycles per fragment (pair of MFMAs)
template <int ORD>
void run_order(int blocks, float &ms, double &cyc) {
  unsigned long long *d;
  hipMalloc(&d, 16);
  auto kern = k<1, 0, 1, 5, 0, 0, 1, ORD>;
  hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  kern<<<blocks, 256, 64 * 1024>>>(d, 10);
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  hipEventRecord(a);
  kern<<<blocks, 256, 64 * 1024>>>(d, g_iters);
  hipEventRecord(b);
  hipDeviceSynchronize();
  hipEventElapsedTime(&ms, a, b);
  unsigned long long h[2];
  hipMemcpy(h, d, 16, hipMemcpyDeviceToHost);
  cyc = (double)h[0] / (g_iters * 16.0);
  hipEventDestroy(a); hipEventDestroy(b);
  hipFree(d);
}

int order_rows() {
  const char *names[3] = {"(a) A held for two, B alternating (today)", "(b) boustrophedon: one operand change per MFMA", "(c) both operands change at every MFMA"};
  float ms[3][3];
  double cyc[3];
  for (int r = 0; r < 3; ++r) {   // rows interleaved: a drift of the box falls on all three alike
    run_order<1>(256, ms[0][r], cyc[0]);
    run_order<2>(256, ms[1][r], cyc[1]);
    run_order<3>(256, ms[2][r], cyc[2]);
  }
  printf("# 16x16x32 pairs, refill per pair, 5 v_pk per pair; %d iterations x 16 fragments, 256 blocks; cycles per fragment of block 0 (last run)\n", g_iters);
  printf("# %-50s cycles  ms (3 runs)                 TFLOP/s (3 runs)      spread   GHz (last run)\n", "row");
  for (int o = 0; o < 3; ++o) {
    float lo = ms[o][0], hi = ms[o][0];
    double tf[3];
    for (int r = 0; r < 3; ++r) {
      lo = ms[o][r] < lo ? ms[o][r] : lo, hi = ms[o][r] > hi ? ms[o][r] : hi;
      tf[r] = 256 * 4.0 * g_iters * 16 * 32768.0 / (ms[o][r] * 1e-3) / 1e12;
    }
    printf("%-52s %6.1f  %9.3f %9.3f %9.3f   %6.0f %6.0f %6.0f  %6.2f %%   %.3f\n", names[o], cyc[o], ms[o][0], ms[o][1], ms[o][2], tf[0], tf[1], tf[2],
           100.0 * (hi - lo) / lo, cyc[o] * 16.0 * g_iters / (ms[o][2] * 1e-3) / 1e9);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1) g_iters = atoi(argv[1]);
  if (argc > 2 && argv[2][0] == 'o') return order_rows();
  for (int blocks : {1, 256}) {
    run<0, 0, 0, 0, 1>("C/D VGPR, B VGPR, no refill, no filler", blocks);
    run<1, 0, 0, 0, 1>("C/D AGPR, B VGPR, no refill, no filler", blocks);
    run<0, 1, 0, 0, 1>("C/D VGPR, B AGPR, no refill, no filler", blocks);
    run<1, 0, 1, 0, 1>("C/D AGPR, refill per pair (shared A)", blocks);
    run<1, 0, 1, 0, 0>("C/D AGPR, refill per MFMA (own A)", blocks);
    run<0, 1, 1, 0, 1>("C/D VGPR, B AGPR, refill per pair", blocks);
    run<1, 0, 1, 3, 1>("C/D AGPR, refill per pair, 3 v_pk per MFMA", blocks);
    run<1, 0, 1, 5, 1>("C/D AGPR, refill per pair, 5 v_pk per MFMA", blocks);
    run<0, 1, 1, 5, 1>("C/D VGPR, B AGPR, refill per pair, 5 v_pk per MFMA", blocks);
    run<1, 0, 1, 5, 0>("C/D AGPR, refill per MFMA, 5 v_pk per MFMA", blocks);
    run<1, 0, 1, 5, 0, 1>("... + 4 v_fma_f32 per MFMA", blocks);
    run<1, 0, 1, 5, 0, 2>("... + 2 v_pk_fma_f32 per MFMA", blocks);
    run<1, 0, 0, 0, 0, 0, 1>("16x16x32 pairs, no refill, no filler", blocks);
    run<1, 0, 1, 0, 0, 0, 1>("16x16x32 pairs, refill per pair (own A)", blocks);
    run<1, 0, 1, 5, 0, 0, 1>("16x16x32 pairs, refill per pair, 5 v_pk per pair", blocks);
    run<1, 0, 1, 5, 0, 1, 1>("... + 4 v_fma_f32 per pair", blocks);
    run<1, 0, 1, 5, 0, 2, 1>("... + 2 v_pk_fma_f32 per pair", blocks);
  }
  return 0;
}
