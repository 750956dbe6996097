// libdfx hot path: the cross-diffusion denoiser eps_theta(x_t, t) fused with the anchored-DDPM
// posterior update, as ONE kernel that can run a single evaluation, a single p_sample step, or the
// whole T-step reverse chain with x_t resident in registers (no HBM round trip per step).
//
// Replaces TransformerNet.forward (python/difffacto/models/diffusions/nets/attention.py:385-440) and
// AnchoredDiffusion.p_mean_variance / p_sample / p_sample_loop_progressive
// (python/difffacto/models/diffusions/anchored_diffusion.py:227-395, 450-484, 528-588).
//
// Mapping (see denoiser_internal.h): one wavefront = 32 points; the residual stream h^T
// (128 channels x 32 points) stays in 64 accumulator VGPRs for the whole chain; every dense
// contraction is a v_mfma_f32_32x32x16_bf16 (or the exact v_mfma_f32_32x32x2_f32) with the WEIGHT
// tile as the A operand and the register-resident activation as the B operand, so consecutive GEMMs
// chain register-to-register.  The bf16 feed-forward (384 of a block's 400 MFMA tiles) runs on
// v_mfma_f32_16x16x32_{bf16,f16} instead, two 16-point N-tiles per wavefront, between two sets of
// 16-lane row swaps (denoiser_ff16.h).  LayerNorm / softmax / GELU / posterior are fp32 VALU on the same
// registers; the 4-key attention needs no q/k/v at run time (folded into A_s / M_s at prepare time).
#include <cmath>
#include <type_traits>

#include "denoiser_ff16.h"
#include "denoiser_internal.h"
#include "denoiser_plan.h"   // (ahead of the pragma: the planner's cost arithmetic is not contracted)

#pragma clang fp contract(fast)

using namespace dfx;

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v8f __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

enum { MODE_EPS = 0, MODE_PSAMPLE = 1, MODE_CHAIN = 2 };
// where a MODE_CHAIN launch takes its first state from: x_T = a + L z (generation), the caller's x_in (a snapshot, a noisy cloud),
// or q_sample of the caller's clean x_in at the first executed timestep, computed in the prologue
enum { START_NOISE = 0, START_GIVEN = 1, START_QSAMPLE = 2 };   // (START_NOISE: the generation kernels; the others: their FROM instantiations)
constexpr int DDIM_MAX_STEPS = 128;
// Instantiations of the bf16 chain kernels.  GENERAL: every entry point, every mode select of KParams tested at run time.  FROM: partial chains.
// PLAIN: plain generation — MODE_CHAIN, DDPM over the whole chain (t = t0 - step), in-kernel Philox for x_T and for the step noise, no t_shape, no
// xstart, no snapshots, no x_in, no hold mask — with all of that fixed at compile time: the launcher (launch(), plain_launch()) takes it exactly
// when the launch is of that kind.  What is left of every function is what GENERAL runs for such a launch, expression for expression, in the same
// order: the two are bit-identical (tests/test_gpu_chain_plain_bits.py).  The exact-fp32 and the direct kernels have GENERAL and FROM only.
enum ChainKind { CHAIN_GENERAL = 0, CHAIN_FROM = 1, CHAIN_PLAIN = 2 };

struct KParams {
  DenoiserDev d;
  const float *part;     // shape ctx regions
  const float *cpart;
  const uint4 *as_ms;
  const float *x_in;     // (B,3,N)        eps / p_sample | chain, START_GIVEN: first state, START_QSAMPLE: clean cloud
  const int32_t *seg;    // (B,N)
  const float *noise;    // p_sample: (B,3,N) | chain: (nsteps,B,3,N) | null -> Philox
  const float *xT_noise; // chain: (B,3,N) | null -> Philox (START_NOISE: the x_T draw; START_QSAMPLE: the forward-noising draw)
  float *out;            // eps: (B,3,N) | p_sample: (B,3,N) | chain: pred (B,N,3)
  float *traj;           // chain snapshots (n_keep,B,N,3) or null
  float *xstart;         // p_sample: optional pred_xstart (B,3,N)
  unsigned long long seed;
  unsigned long long shape0;   // global index of this launch's shape 0 (Philox counters are keyed by the GLOBAL point id)
  int B, N, t0, nsteps, ret_interval, mode;
  // DDIM branch (anchored_diffusion.py:114-124, :368-377, :480-481): ddim_n > 0 = the executed timestep list
  // (descending, e.g. 'quad' [32,23,16,10,5,2,0,0]) and xt_dir_coeff[t] = sqrt(1 - acp[t] - eta^2 posterior_variance[t])
  const int32_t *t_shape;  // MODE_EPS only: per-shape timestep (B,), training-style evaluation (anchored_diffusion.py:760-853)
  int ddim_n;
  float ddim_eta;
  int ddim_t[DDIM_MAX_STEPS];
  float ddim_xdc[DDIM_MAX_STEPS];
  unsigned long long *trace;  // debug: s_memtime stamps of waves 0 and 4 of workgroup 0 at every slot boundary
  int trace_cap;
  int start;              // chain: START_*
  const int32_t *hold;    // chain, START_GIVEN / START_QSAMPLE: (B,) bit j = the points of part j keep their x_in coordinates | null
};

// ----------------------------------------------------------------------------------------------
// Activation fragments: the B operand view of one 32-channel accumulator tile.
template <int PREC>
struct Act;
template <>
struct Act<DFX_PREC_BF16> {
  v8bf f[2];
  __device__ __forceinline__ void set(const v16f &x) {
    v8f lo = __builtin_shufflevector(x, x, 0, 1, 2, 3, 4, 5, 6, 7);
    v8f hi = __builtin_shufflevector(x, x, 8, 9, 10, 11, 12, 13, 14, 15);
    f[0] = __builtin_convertvector(lo, v8bf);
    f[1] = __builtin_convertvector(hi, v8bf);
  }
};
template <>
struct Act<DFX_PREC_F32> {
  v16f x;
  __device__ __forceinline__ void set(const v16f &v) { x = v; }
};

// acc += Wtile (32 rows x 32 k)  *  act (32 k x 32 points).   `w` already includes the lane offset.
template <int PREC>
__device__ __forceinline__ void mma_tile(v16f &acc, const uint4 *__restrict__ w, const Act<PREC> &a);

template <>
__device__ __forceinline__ void mma_tile<DFX_PREC_BF16>(v16f &acc, const uint4 *__restrict__ w,
                                                        const Act<DFX_PREC_BF16> &a) {
  const uint4 u0 = w[0], u1 = w[64];
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, u0), a.f[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, u1), a.f[1], acc, 0, 0, 0);
}

template <>
__device__ __forceinline__ void mma_tile<DFX_PREC_F32>(v16f &acc, const uint4 *__restrict__ w,
                                                       const Act<DFX_PREC_F32> &a) {
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const v4f u = __builtin_bit_cast(v4f, w[r4 * 64]);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u[e], a.x[4 * r4 + e], acc, 0, 0, 0);
  }
}

__device__ __forceinline__ float xhalf(float v) { return __shfl_xor(v, 32, 64); }

// LayerNorm statistics over the 128 channels of each point (64 in-lane + the partner half-wave).
__device__ __forceinline__ void ln_stats(const v16f (&h)[4], float &mean, float &rstd) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += h[c][r];
  s += xhalf(s);
  mean = s * (1.0f / 128.0f);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float dlt = h[c][r] - mean;
      q = fmaf(dlt, dlt, q);
    }
  q += xhalf(q);
  rstd = 1.0f / sqrtf(q * (1.0f / 128.0f) + 1e-5f);  // nn.LayerNorm eps (attention.py:348-349, 286-287)
}

// bf16 path: single pass over the registers (sum and sum of squares on four independent chains each), variance as
// E[x^2] - mean^2 in fp32 — the normalised value is rounded to bf16 right after, so the cancellation error
// (<= 2^-24 E[x^2] / var relative) is far below the operand rounding — and one FMA per element for the normalisation.
//
// Packed fp32 (v_pk_add_f32 / v_pk_fma_f32: two IEEE operations per instruction, at the issue cost of one): the fp32 work of the bf16 kernels
// outside the feed-forward loop is written on register PAIRS — chains (0, 1) and (2, 3) here take registers (4k, 4k+1) and (4k+2, 4k+3) in
// the order they always did, so every half is the operation it was and the bits are the same (tests/test_gpu_chain_bits.py).  The library is
// built with -fno-slp-vectorize: only what is spelled on v2f is packed, and none of it sits in an M or V slot of the feed-forward.
__device__ __forceinline__ v2f pair(const v16f &x, int i) { return v2f{x[2 * i], x[2 * i + 1]}; }
__device__ __forceinline__ void set_pair(v16f &x, int i, const v2f &v) { x[2 * i] = v[0], x[2 * i + 1] = v[1]; }
__device__ __forceinline__ v2f splat2(float v) { return v2f{v, v}; }
__device__ __forceinline__ void ln_stats_fast(const v16f (&h)[4], float &mean, float &rstd) {
  v2f s01 = {0.f, 0.f}, s23 = s01, q01 = s01, q23 = s01;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const v2f a = pair(h[c], 2 * k), b = pair(h[c], 2 * k + 1);
      s01 += a;
      s23 += b;
      q01 = __builtin_elementwise_fma(a, a, q01);
      q23 = __builtin_elementwise_fma(b, b, q23);
    }
  float st = (s01[0] + s01[1]) + (s23[0] + s23[1]), qt = (q01[0] + q01[1]) + (q23[0] + q23[1]);
  st += xhalf(st);
  qt += xhalf(qt);
  mean = st * (1.0f / 128.0f);
  const float var = fmaxf(fmaf(-mean, mean, qt * (1.0f / 128.0f)), 0.f);
  rstd = __builtin_amdgcn_rsqf(var + 1e-5f);
}

template <int PREC>
__device__ __forceinline__ void ln_to_act(const v16f (&h)[4], Act<PREC> (&xn)[4]) {
  float mean, rstd;
  if (PREC == DFX_PREC_BF16) {
    ln_stats_fast(h, mean, rstd);
    const float nmr = -mean * rstd;
    const v2f rstd2 = splat2(rstd), nmr2 = splat2(nmr);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v16f t;
#pragma unroll
      for (int i = 0; i < 8; ++i) set_pair(t, i, __builtin_elementwise_fma(pair(h[c], i), rstd2, nmr2));
      xn[c].set(t);
    }
    return;
  }
  ln_stats(h, mean, rstd);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    v16f t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = (h[c][r] - mean) * rstd;
    xn[c].set(t);
  }
}

__device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
// bf16 path, GEMM1 of the feed-forward: LayerNorm3's output xhat sums to zero over its 128 channels, so channel 127 is redundant
// (xhat_127 = - sum of the others).  denoiser_setup.hip packs W1'' = W1'[., k] - W1'[., 127] for k < 127 and puts b1' into column 127;
// here channel 127's K slot — register 15 of tile 3 in the upper half-wave (rho(15, 1) = 31) — carries the constant 1, so
// [a | g] = W1'' xhat'' comes out of the MFMAs WITH its bias, started from C = 0: the 8 ds_read_b128 of accumulator initialisers per
// record are gone (2.1 % of a record's energy, profiles/r02_energy_budget.txt; measured +2.5 %, profiles/r04_headline_experiments.txt).
// Exact in real arithmetic; in bf16 the weight differences round ~1.4x coarser and the implicit channel carries the rounding noise of
// the other 127: one evaluation deviates from fp32 by rms 8.1e-4 instead of 6.6e-4 (same file).  fp32 kernels keep the plain form.
__device__ __forceinline__ void bias_slot_one(Act<DFX_PREC_BF16> (&xn)[4], int hf) {
  if (hf) xn[3].f[1][7] = (__bf16)1.0f;
}
__device__ __forceinline__ void bias_slot_one(Act<DFX_PREC_F32> (&)[4], int) {}

__device__ __forceinline__ float gelu_erf(float x) {  // F.gelu default (attention.py:57)
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

template <bool PK = false>   // PK: the bf16 kernels' form, two adds per instruction (ln_stats_fast)
__device__ __forceinline__ void add_cvec(v16f (&h)[4], const float *__restrict__ v /* + hf*64 applied */) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      if (PK) {
        const v4f t = *reinterpret_cast<const v4f *>(v + c * 16 + r4 * 4);
        set_pair(h[c], 2 * r4, pair(h[c], 2 * r4) + v2f{t[0], t[1]});
        set_pair(h[c], 2 * r4 + 1, pair(h[c], 2 * r4 + 1) + v2f{t[2], t[3]});
        continue;
      }
      const float4 t = *reinterpret_cast<const float4 *>(v + c * 16 + r4 * 4);
      h[c][r4 * 4 + 0] += t.x;
      h[c][r4 * 4 + 1] += t.y;
      h[c][r4 * 4 + 2] += t.z;
      h[c][r4 * 4 + 3] += t.w;
    }
}

// ----------------------------------------------------------------------------------------------
// Philox4x32-10 counter RNG + Box-Muller (perf runs; parity runs feed explicit noise).  Counter = (gid lo, gid hi, t, stream), key = (seed lo,
// seed hi); gid = (shape_offset + b) N + n with the N of the launch (the engine's padded one); stream 0 = the noise of timestep t, stream 1 = a
// start draw (x_T keyed by T, the refine start keyed by n_steps).  Three normals from four 24-bit uniforms ((w >> 8) + 0.5) 2^-24: (r(u0) cos, r(u0) sin)
// of 2 pi u1 and r(u2) cos 2 pi u3.  DESIGN.md "Random streams" lists the layout; tests/test_gpu_random_streams.py judges every entry point and
// kernel variant against oracle/philox.py in units of z.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ void philox_normal3(unsigned long long seed, unsigned long long gid, unsigned t,
                                               unsigned stream, float (&z)[3]) {
  const uint4 r = philox4x32_10(make_uint4((unsigned)gid, (unsigned)(gid >> 32), t, stream),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  const float u0 = ((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u1 = ((float)(r.y >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(r.z >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u3 = ((float)(r.w >> 8) + 0.5f) * (1.0f / 16777216.0f);
  // hardware transcendentals (v_log_f32; v_sin_f32 / v_cos_f32 take revolutions): plenty for a noise source and
  // far fewer instructions than the libm versions in the persistent kernel's step epilogue
  const float ra = sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u0));  // -2 ln(u) = -2 ln2 log2(u)
  const float rb = sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u2));
  z[0] = ra * __builtin_amdgcn_cosf(u1);
  z[1] = ra * __builtin_amdgcn_sinf(u1);
  z[2] = rb * __builtin_amdgcn_cosf(u3);
}

// ----------------------------------------------------------------------------------------------
// Building blocks shared by the direct (v0) and the LDS-pipelined kernels.  Pointers may be global
// or LDS: after inlining the compiler infers the address space from the call site.

// proj_in (13 -> 128) + pre_norm.  x-columns on the VALU; the 10 per-part-constant inputs
// (anchors | variances | onehot, attention.py:398-408) are pre-folded into cpart[seg].
__device__ __forceinline__ void proj_in_prenorm(v16f (&h)[4], const float (&x)[3], const float *cpart,
                                                const float4 *winx, const float2 *pregb) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 cp = *reinterpret_cast<const float4 *>(cpart + c * 16 + r4 * 4);
      const float cpv[4] = {cp.x, cp.y, cp.z, cp.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 w = winx[c * 16 + r4 * 4 + e];
        h[c][r4 * 4 + e] = fmaf(w.z, x[2], fmaf(w.y, x[1], fmaf(w.x, x[0], cpv[e])));
      }
    }
  float mean, rstd;
  ln_stats(h, mean, rstd);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float2 gb = pregb[c * 16 + r];
      h[c][r] = fmaf((h[c][r] - mean) * rstd, gb.x, gb.y);  // affine kept: h is the residual stream
    }
}

// The bf16 chain kernels' step-boundary tables, as their prologues lay them out in LDS (pair_tables): per PAIR of channels (2i, 2i+1) — the
// registers (2i, 2i+1) of a tile of h — the operands of one packed instruction side by side and no padding word:
//     W_in x-columns  6 floats  wx(2i) wx(2i+1) | wy(2i) wy(2i+1) | wz(2i) wz(2i+1)
//     pre_norm        4 floats  gamma(2i) gamma(2i+1) | beta(2i) beta(2i+1)
//     W_out           6 floats  wx(2i) wy(2i) | wx(2i+1) wy(2i+1) | wz(2i) wz(2i+1)      (eps_x and eps_y are one packed chain, eps_z a scalar one)
// Two pairs = three ds_read_b128 for W_in and for W_out (four before, one float4 per channel with a padding word).
constexpr int PAIR_WIN = 6, PAIR_PREGB = 4, PAIR_WOUT = 6;
// channel pair `i` (0..63) of the engine's tables -> the three pair tables; the caller's barrier publishes them
__device__ __forceinline__ void pair_tables(const DenoiserDev &d, int i, float *winp, float *pregp, float *woutp) {
  const float4 wa = d.win_x[2 * i], wb = d.win_x[2 * i + 1], oa = d.wout[2 * i], ob = d.wout[2 * i + 1];
  const float2 ga = d.pre_gb[2 * i], gb = d.pre_gb[2 * i + 1];
  float *w = winp + i * PAIR_WIN, *g = pregp + i * PAIR_PREGB, *o = woutp + i * PAIR_WOUT;
  w[0] = wa.x, w[1] = wb.x, w[2] = wa.y, w[3] = wb.y, w[4] = wa.z, w[5] = wb.z;
  g[0] = ga.x, g[1] = gb.x, g[2] = ga.y, g[3] = gb.y;
  o[0] = oa.x, o[1] = oa.y, o[2] = ob.x, o[3] = ob.y, o[4] = oa.z, o[5] = ob.z;
}
// 12 floats = two pairs' W_in / W_out entries, as three 16-byte reads
struct Pair2 {
  v4f q[3];
  __device__ __forceinline__ v2f at(int k) const { return v2f{q[k >> 1][2 * (k & 1)], q[k >> 1][2 * (k & 1) + 1]}; }   // k-th 64-bit operand, 0..5
};
__device__ __forceinline__ Pair2 load_pair2(const float *t) {
  const v4f *q = reinterpret_cast<const v4f *>(t);
  return Pair2{{q[0], q[1], q[2]}};
}
// proj_in of four channels = registers 4j .. 4j+3 of one tile: the three-FMA chain of every channel, two channels per instruction
__device__ __forceinline__ void proj_in4_pk(v16f &ht, int j, const v2f (&x2)[3], const v4f &cp, const Pair2 &w) {
  set_pair(ht, 2 * j, __builtin_elementwise_fma(w.at(2), x2[2], __builtin_elementwise_fma(w.at(1), x2[1], __builtin_elementwise_fma(w.at(0), x2[0], v2f{cp[0], cp[1]}))));
  set_pair(ht, 2 * j + 1, __builtin_elementwise_fma(w.at(5), x2[2], __builtin_elementwise_fma(w.at(4), x2[1], __builtin_elementwise_fma(w.at(3), x2[0], v2f{cp[2], cp[3]}))));
}
// proj_in_prenorm of the bf16 chain kernels (single-pass statistics), on the pair tables of this half-wave (`winp`, `pregp`: + hf * 32 pairs)
__device__ __forceinline__ void proj_in_prenorm_pk(v16f (&h)[4], const float (&x)[3], const float *cpart, const float *winp, const float *pregp) {
  const v2f x2[3] = {splat2(x[0]), splat2(x[1]), splat2(x[2])};
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      proj_in4_pk(h[c], j, x2, *reinterpret_cast<const v4f *>(cpart + c * 16 + j * 4), load_pair2(winp + (c * 4 + j) * 2 * PAIR_WIN));
  float mean, rstd;
  ln_stats_fast(h, mean, rstd);
  const v2f mean2 = splat2(mean), rstd2 = splat2(rstd);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const v4f gb = *reinterpret_cast<const v4f *>(pregp + (c * 8 + i) * PAIR_PREGB);
      set_pair(h[c], i, __builtin_elementwise_fma((pair(h[c], i) - mean2) * rstd2, v2f{gb[0], gb[1]}, v2f{gb[2], gb[3]}));  // affine kept: h is the residual stream
    }
}

__device__ __forceinline__ void load16(v16f &v, const float *src) {
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const float4 t4 = *reinterpret_cast<const float4 *>(src + r4 * 4);
    v[r4 * 4 + 0] = t4.x; v[r4 * 4 + 1] = t4.y; v[r4 * 4 + 2] = t4.z; v[r4 * 4 + 3] = t4.w;
  }
}

// Masked softmax over the 4 keys of each head, in place (registers 4g..4g+3 = keys 0..3 of head 2g+hf; attention.py:195-198).
// bf16 kernels (softmax4<true>, every one of them through this function): on register pairs, as ln_stats_fast.  The max-subtract and the exp's scale
// (__expf = v_exp_f32 of x * log2(e)) take the pairs (0, 1) and (2, 3) of a head; the sum and the multiply by the reciprocal take the SAME key of two
// neighbouring heads side by side, so that every half is the operation it always was, in the order it always was (0 + e0 + e1 + e2 + e3), and the bits
// hold for every key mask (tests/test_gpu_softmax_masks_bits.py).  The max, v_exp_f32 and v_rcp_f32 have no packed form.  The
// hardware reciprocal (1 ulp) stands for the correctly rounded division (~10 VALU instructions, four per block).
// There is no mask select here: a bf16 attention record carries the key mask in sbias (dfx_shape_ctx_prepare writes -FLT_MAX into the rows of absent
// parts), sbias is the C operand of the A_s MFMAs, and -FLT_MAX plus products below half its ulp (1e31) is -FLT_MAX: `sim` arrives with the value the
// select used to put there (:195-197).  Every bf16 kernel relies on it, through this function: the chain kernels, dfx_denoise_eps(_t), dfx_p_sample(_ddim)
// and the partial chains, on every context of a bf16 engine — the editing paths prepare a new context whenever they change `valid`.
__device__ __forceinline__ void softmax4_pk(v16f &sim) {
  const v2f l2e = splat2(1.44269504088896340736f);
#pragma unroll
  for (int gp = 0; gp < 2; ++gp) {   // heads 2gp and 2gp + 1 of this half-wave
    float e[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int g = 2 * gp + u;
      float sj[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) sj[j] = sim[4 * g + j];
      const v2f m2 = splat2(fmaxf(fmaxf(sj[0], sj[1]), fmaxf(sj[2], sj[3])));
      const v2f t01 = (v2f{sj[0], sj[1]} - m2) * l2e, t23 = (v2f{sj[2], sj[3]} - m2) * l2e;
      e[u][0] = __builtin_amdgcn_exp2f(t01[0]), e[u][1] = __builtin_amdgcn_exp2f(t01[1]);
      e[u][2] = __builtin_amdgcn_exp2f(t23[0]), e[u][3] = __builtin_amdgcn_exp2f(t23[1]);
    }
    v2f sum = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += v2f{e[0][j], e[1][j]};
    const v2f inv = {__builtin_amdgcn_rcpf(sum[0]), __builtin_amdgcn_rcpf(sum[1])};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const v2f pr = v2f{e[0][j], e[1][j]} * inv;
      sim[8 * gp + j] = pr[0], sim[8 * gp + 4 + j] = pr[1];
    }
  }
}
template <bool FAST_RCP = false>   // true: the bf16 kernels (softmax4_pk)
__device__ __forceinline__ void softmax4(v16f &sim, unsigned vmask) {
  if constexpr (FAST_RCP) {
    softmax4_pk(sim);   // (the mask is in sim already: sbias)
    return;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float sj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sj[j] = (vmask >> j) & 1u ? sim[4 * g + j] : -3.402823466e38f;  // :195-197
    const float m = fmaxf(fmaxf(sj[0], sj[1]), fmaxf(sj[2], sj[3]));
    float e[4], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j] = __expf(sj[j] - m);
      sum += e[j];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) sim[4 * g + j] = e[j] * inv;
  }
}

// Cross attention to the 4 part tokens (attention.py:179-204 with q/k/v folded away, see denoiser_setup.hip):
//   sim = A_s LN2(h) + sbias;  P = softmax over the 4 keys of each head (masked);  h += M_s P + c_t
// `rec` = this lane's view of the attention record (tiles 0..3 = A_s, 4..7 = M_s).
template <int PREC>
__device__ __forceinline__ void attention(v16f (&h)[4], const uint4 *rec, const float *sbias, const float *ct,
                                          unsigned vmask) {
  constexpr int TSTRIDE = tile_units(PREC) * 64;
  Act<PREC> xn[4];
  ln_to_act<PREC>(h, xn);
  v16f sim;
  load16(sim, sbias);
#pragma unroll
  for (int c = 0; c < 4; ++c) mma_tile<PREC>(sim, rec + c * TSTRIDE, xn[c]);
  softmax4<PREC == DFX_PREC_BF16>(sim, vmask);
  Act<PREC> pa;
  pa.set(sim);
#pragma unroll
  for (int t = 0; t < 4; ++t) mma_tile<PREC>(h[t], rec + (4 + t) * TSTRIDE, pa);
  add_cvec<PREC == DFX_PREC_BF16>(h, ct);
}

// GELU for the bf16 path: x * sigmoid(x (c1 + c3 x^2)) with (c1, c3) = (1.60031416, 0.06940179) fitted to the
// exact erf form (max abs error 2.7e-4 over all x, below the bf16 rounding of the hidden activation it
// feeds; the standard tanh constants give 4.7e-4).  The argument is monotone in x, so no clamp is needed:
// +-inf / huge inputs give sigmoid = 1 / 0 exactly.  6 plain VALU + v_exp_f32 + v_rcp_f32 per element.
__device__ __forceinline__ float gelu_sigmoid_arg(float x) {
  const float x2 = x * x;
  return x * fmaf(-0.100125614f, x2, -2.30876530f);  // -log2(e) * x (c1 + c3 x^2)
}
__device__ __forceinline__ float gelu_fast(float x) {
  const float e = __builtin_amdgcn_exp2f(gelu_sigmoid_arg(x));
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

template <int PREC>
__device__ __forceinline__ float gelu_for(float x) {
  return PREC == DFX_PREC_BF16 ? gelu_fast(x) : gelu_erf(x);
}

// ---- packed-fp16 GELU (bf16 path; see denoiser_internal.h) ----------------------------------------------------------
// B operand of GEMM2: 16 hidden values of this lane as fp16, same element order as Act.
struct HidAct {
  uint4 f[2];
};
__device__ __forceinline__ h2 pk_f16(float lo, float hi) { return __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(lo, hi)); }
// gelu(g) = g Phi(g),  Phi(g) ~ 1/2 + u R(z),  u = g / 2,  z = min(u^2 - m, L^2 - m),  R of degree 5 (minimax fit of g Phi(g) on
// [-6, 6]: 3.9e-4 in exact arithmetic; evaluated in fp16 with the centred argument z the error of a * gelu(g) is rms 8.5e-4 for
// a, g ~ N(0, 1.5), tools/experiments/fit_gelu_poly.py).  Ten packed instructions per PAIR of values and no transcendental (an exp / rcp
// pair is quarter rate and not packed: the sigmoid form cost 6 packed + 4 transcendental instructions per pair = 2.2x the
// VALU cycles).  g arrives as g / 2 (FF_G_SCALE), a as a / 16 (FF_A_SCALE); fp16 overflow is benign: z saturates at the
// min, the clamp modifier saturates Phi to [0, 1].
__device__ __forceinline__ h2 h2c(float v) { return h2{(_Float16)v, (_Float16)v}; }
// (a, g) -> packed fp16 first: after these sixteen conversions the accumulators are dead and their next initialisers
// (b1 of the next chunk) can be fetched from LDS underneath the GELU arithmetic instead of after it.
__device__ __forceinline__ void gelu16_f16_cvt(const v16f &a, const v16f &g, h2 (&aa)[8], h2 (&gg)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) gg[i] = pk_f16(g[2 * i], g[2 * i + 1]);
#pragma unroll
  for (int i = 0; i < 8; ++i) aa[i] = pk_f16(a[2 * i], a[2 * i + 1]);
}
__device__ __forceinline__ void gelu16_f16_math(const h2 (&aa)[8], const h2 (&gg)[8], HidAct &hid) {
  // Stage by stage over the eight packed pairs: eight independent instructions between any two dependent ones (a
  // dependent v_pk_* costs a wait state on gfx950; written pair by pair hipcc serialises the whole chain through three
  // registers: 88 dependent instructions + 53 s_nop, 1176 cycles per slot against 984 like this).
  h2 y[8], z[8], r[8];
#define DFX_STAGE(expr)                                   \
  _Pragma("unroll") for (int i = 0; i < 8; ++i) { expr; } \
  __builtin_amdgcn_sched_barrier(0)
  __builtin_amdgcn_sched_barrier(0);
  DFX_STAGE(z[i] = __builtin_elementwise_fma(gg[i], gg[i], h2c(-1.62f)));
  DFX_STAGE(y[i] = aa[i] * gg[i]);
  DFX_STAGE(z[i] = __builtin_elementwise_min(z[i], h2c(1.62f)));
  DFX_STAGE(r[i] = __builtin_elementwise_fma(z[i], h2c(-0.0011402554f), h2c(0.0057853916f)));
  DFX_STAGE(r[i] = __builtin_elementwise_fma(r[i], z[i], h2c(-0.0158536041f)));
  DFX_STAGE(r[i] = __builtin_elementwise_fma(r[i], z[i], h2c(0.0409006897f)));
  DFX_STAGE(r[i] = __builtin_elementwise_fma(r[i], z[i], h2c(-0.1098130657f)));
  DFX_STAGE(r[i] = __builtin_elementwise_fma(r[i], z[i], h2c(0.3885767652f)));
  DFX_STAGE(asm("v_pk_fma_f16 %0, %1, %2, 0.5 op_sel_hi:[1,1,0] clamp" : "=v"(z[i]) : "v"(gg[i]), "v"(r[i])));   // Phi
  DFX_STAGE(y[i] = y[i] * z[i]);
#undef DFX_STAGE
  hid.f[0] = make_uint4(__builtin_bit_cast(unsigned, y[0]), __builtin_bit_cast(unsigned, y[1]), __builtin_bit_cast(unsigned, y[2]),
                        __builtin_bit_cast(unsigned, y[3]));
  hid.f[1] = make_uint4(__builtin_bit_cast(unsigned, y[4]), __builtin_bit_cast(unsigned, y[5]), __builtin_bit_cast(unsigned, y[6]),
                        __builtin_bit_cast(unsigned, y[7]));
}
// ---- the bf16 feed-forward on v_mfma_f32_16x16x32 (layout algebra: denoiser_ff16.h) --------------------------------------
// The smaller shape costs the same cycles per FLOP and the same LDS bytes per FLOP (every fragment feeds two MFMAs, one per
// 16-point N-tile), and the chip holds a higher clock on it under the power cap.  Everything outside GEMM1 / GELU / GEMM2 keeps
// one point per lane; 16-lane row swaps move xn and h between the two forms, exactly (they move bits).
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
// x, y -> (x0, y0, x2, y2), (x1, y1, x3, y3) by 16-lane rows; its own inverse
__device__ __forceinline__ void row_swap(unsigned &x, unsigned &y) {
  const v2u r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
  x = r[0], y = r[1];
}
// LayerNorm3's output (one point per lane) -> xn[c].f[n] = GEMM1's B operand of N-tile n, K step c: 16 swaps
__device__ __forceinline__ void ff16_rows(Act<DFX_PREC_BF16> (&xn)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    v4u x = __builtin_bit_cast(v4u, xn[c].f[0]), y = __builtin_bit_cast(v4u, xn[c].f[1]);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      unsigned a = x[v], b = y[v];
      row_swap(a, b);
      x[v] = a, y[v] = b;
    }
    xn[c].f[0] = __builtin_bit_cast(v8bf, x), xn[c].f[1] = __builtin_bit_cast(v8bf, y);
  }
}
__device__ __forceinline__ void ff16_rows(Act<DFX_PREC_F32> (&)[4]) {}
// one 32-channel tile of h: quads 2t + n <-> the accumulators of M-tile t, N-tile n (8 swaps, in place; the same call brings it back)
__device__ __forceinline__ void ff16_rows(v16f &h) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned a = __float_as_uint(h[8 * t + r]), b = __float_as_uint(h[8 * t + 4 + r]);
      row_swap(a, b);
      h[8 * t + r] = __uint_as_float(a), h[8 * t + 4 + r] = __uint_as_float(b);
    }
}
__device__ __forceinline__ void ff16_rows(v16f (&h)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) ff16_rows(h[c]);
}
__device__ __forceinline__ v4f quad(const v16f &x, int q) { return v4f{x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]}; }
__device__ __forceinline__ void set_quad(v16f &x, int q, const v4f &v) { x[4 * q] = v[0], x[4 * q + 1] = v[1], x[4 * q + 2] = v[2], x[4 * q + 3] = v[3]; }
// GEMM1: quads 2n + mt of acc (a or g) += W1 fragment of M-tile mt (A) x xn unit n (B), n = 0, 1; first: C = 0
__device__ __forceinline__ void mma16_w1(v16f &acc, int mt, const uint4 &w, const Act<DFX_PREC_BF16> &x, bool first) {
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const v4f c = first ? v4f{0.f, 0.f, 0.f, 0.f} : quad(acc, 2 * n + mt);
    set_quad(acc, 2 * n + mt, __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, w), x.f[n], c, 0, 0, 0));
  }
}
// GEMM2: quads 2 mt + n of one tile of h (after ff16_rows) += W2 fragment of M-tile mt (A, fp16) x hid unit n (B)
__device__ __forceinline__ void mma16_w2(v16f &ht, int mt, const uint4 &w, const uint4 &hid0, const uint4 &hid1) {
  set_quad(ht, 2 * mt, __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, w), __builtin_bit_cast(v8h, hid0), quad(ht, 2 * mt), 0, 0, 0));
  set_quad(ht, 2 * mt + 1, __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, w), __builtin_bit_cast(v8h, hid1), quad(ht, 2 * mt + 1), 0, 0, 0));
}

// One hidden chunk (32 units) of the GEGLU feed-forward (attention.py:50-57,77-94):
//   a = W1a xn + b1a; g = W1g xn + b1g; hid = a * gelu(g); h += W2[:, chunk] hid.  Hidden stays in registers.
// bf16 (direct kernel): xn and h in the 16x16x32 form (ff16_rows), `b1` = this lane row's eight initialisers of a (g: + 32)
__device__ __forceinline__ void ff_chunk(v16f (&h)[4], const Act<DFX_PREC_BF16> (&xn)[4], const uint4 *ck, const uint4 *ck2,
                                         const float *b1, bool fold) {
  v16f a = zero16(), g = zero16();   // fold: b1' rides on the constant-one K slot (bias_slot_one)
  if (!fold) {                       // engines whose weights ruled the fold out (DenoiserDev::w1_fold = 0): plain W1', b1' initialisers
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const v4f ia = *reinterpret_cast<const v4f *>(b1 + 4 * m), ig = *reinterpret_cast<const v4f *>(b1 + 32 + 4 * m);
      set_quad(a, m, ia), set_quad(a, 2 + m, ia), set_quad(g, m, ig), set_quad(g, 2 + m, ig);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      mma16_w1(a, m, ck[(0 + c) * 128 + m * 64], xn[c], false);
      mma16_w1(g, m, ck[(4 + c) * 128 + m * 64], xn[c], false);
    }
  v16f hid;
#pragma unroll
  for (int r = 0; r < 16; ++r)   // g and `a` arrive pre-scaled, hid carries the same factors, W2 is fp16 (denoiser_internal.h)
    hid[r] = a[r] * gelu_fast(g[r] * (1.0f / FF_G_SCALE)) * FF_G_SCALE;
  HidAct hf16;
  h2 y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = pk_f16(hid[2 * i], hid[2 * i + 1]);
  hf16.f[0] = make_uint4(__builtin_bit_cast(unsigned, y[0]), __builtin_bit_cast(unsigned, y[1]), __builtin_bit_cast(unsigned, y[2]),
                         __builtin_bit_cast(unsigned, y[3]));
  hf16.f[1] = make_uint4(__builtin_bit_cast(unsigned, y[4]), __builtin_bit_cast(unsigned, y[5]), __builtin_bit_cast(unsigned, y[6]),
                         __builtin_bit_cast(unsigned, y[7]));
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int m = 0; m < 2; ++m) mma16_w2(h[t], m, ck2[(8 + t) * 128 + m * 64], hf16.f[0], hf16.f[1]);
}
// fp32 (direct kernel)
__device__ __forceinline__ void ff_chunk(v16f (&h)[4], const Act<DFX_PREC_F32> (&xn)[4], const uint4 *ck, const uint4 *ck2,
                                         const float *b1, bool) {
  constexpr int PREC = DFX_PREC_F32, TSTRIDE = tile_units(PREC) * 64;
  v16f a, g;
  load16(a, b1);
  load16(g, b1 + 32);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mma_tile<PREC>(a, ck + (0 + c) * TSTRIDE, xn[c]);
    mma_tile<PREC>(g, ck + (4 + c) * TSTRIDE, xn[c]);
  }
  v16f hid;
#pragma unroll
  for (int r = 0; r < 16; ++r) hid[r] = a[r] * gelu_erf(g[r]);
  Act<PREC> ha;
  ha.set(hid);
#pragma unroll
  for (int t = 0; t < 4; ++t) mma_tile<PREC>(h[t], ck2 + (8 + t) * TSTRIDE, ha);
}

// ---- building blocks of the LDS-pipelined bf16 kernel ---------------------------------------------------
// Every wavefront's stream is cut into pure MFMA bursts ("M slots") and pure VALU bursts ("V slots"), and the two
// wavefronts of a SIMD run them in anti-phase (k_denoise_pipe), so that the matrix pipe of a SIMD always has one
// wavefront feeding it while the other one does the fp32 work.  Measured rules behind the structure
// (tools/ubench/agpr_overlap.hip, stage_mix.hip, lds_bw.hip):
//   * a VALU instruction next to MFMAs costs ~3.1 cycles of SIMD issue (transcendentals ~10), every MFMA takes
//     ~18 cycles of VALU issue away: T(SIMD) ~ max(32.6 nMFMA, 3.1 nVALU + 10 nTRANS + 18 nMFMA);
//   * packed fp32 VALU (v_pk_mul/fma/add_f32) serialises against the matrix pipe: never in an M or V slot of the feed-forward
//     (the library is built with -fno-slp-vectorize, +10 %); the V0 / V1 / V2 slots and the step boundary do use it (ln_stats_fast, softmax4_pk);
//   * LDS delivers ~240 B/clk/CU with eight wavefronts reading; one wavefront sustains ~32 B/clk (latency bound).
__device__ __forceinline__ v8bf as_bf(const uint4 &u) { return __builtin_bit_cast(v8bf, u); }

constexpr int MFMA_PRIO = 0, VALU_PRIO = 3;   // s_setprio inside M / V slots

// M slot of FF record j: h += W2[:, chunk j-1] hid (S3: 8 MFMAs) then a,g = b1[j] + W1[chunk j] xn (S1: 16 MFMAs).
// The 24 A-fragment units are fetched in batches of eight ds_read_b128 running one batch ahead of the MFMAs.
// Slot-boundary clock stamps for tools/experiments/trace_slots.py; compiled in only with -DDFX_TRACE (the bookkeeping costs
// ~10 scalar instructions per stamp site even when switched off at run time).
struct Tracer {
#ifdef DFX_TRACE
  unsigned long long *buf;  // nullptr = off
  int cap, count;
  __device__ __forceinline__ void stamp(int tag) {
    if (buf && count < cap) {
      if ((threadIdx.x & 63) == 0) buf[count] = ((unsigned long long)tag << 56) | (__builtin_readcyclecounter() & 0xffffffffffffffull);
      ++count;
    }
  }
#else
  __device__ __forceinline__ void stamp(int) {}
#endif
};

// Fragment indices (uint4 units relative to this lane's record pointer).  FF record: W2 tile ct = i&3, unit q = i>>2 (a tile's
// two MFMAs are four MFMAs apart: a dependent accumulate right behind its predecessor waits for it when the wave is alone on its SIMD);
// W1 unit order (c, q, part) -> tile part*4 + c, unit q (half 0: c = 0,1; half 1: c = 2,3).  Attention record: A_s tiles
// 0..3, M_s tiles 4..7.
// (FF: denoiser_ff16.h — a W1 / W2 unit is the 16-row A fragment of one M-tile over all 32 K slots, used for both N-tiles)
using ff16::w1_frag;
using ff16::w2_frag;
using ff16::ff_frag;
__device__ __forceinline__ constexpr int as_frag(int i) { return (i >> 1) * 128 + (i & 1) * 64; }
__device__ __forceinline__ constexpr int ms_frag(int i) { return (4 + (i & 3)) * 128 + (i >> 2) * 64; }

// Tail prefetch: every M slot finds the A fragments of its first eight MFMAs in registers (P): they are read at the
// TAIL of the previous M slot of the same wavefront — after its last MFMA has been issued, while the matrix pipe drains
// and the wave has nothing else to issue — so the burst starts without the LDS round trip (~300 cycles per slot) and the
// VALU-bound V slot in between carries no extra LDS instructions.  Needs the next record complete in LDS one management
// barrier earlier: the ring runs three records ahead in five slots.
// Interleaved M slots: every fragment's MFMAs (one in the attention slots, the two N-tiles' in the feed-forward's) are followed by ONE
// LDS read that refills the fragment register they have just consumed with the fragment needed eight fragments later (in place:
// an MFMA reads its A operand at issue), so the wavefront's read
// instructions issue while the matrix pipe works instead of in bursts during which it drains.  The last eight refills are
// the tail prefetch for the next M slot.  `issue.at(i, n)` issues the wave's ring-DMA pieces between the MFMAs.

// Fragment order of a full FF record (GEMM2 of chunk j-1 and GEMM1 of chunk j are independent; ff16::ff_frag): eight groups of
//     GEMM2 fragment k (tile h[k & 3])  |  GEMM1 fragment 2k (a)  |  GEMM1 fragment 2k+1 (g)
// so that an accumulator is touched every third fragment at the earliest (the r01 order — 8 x GEMM2, then 16 x GEMM1 with its two
// accumulators alternating — made every GEMM1 MFMA depend on the one two before it).  Measured on the 32x32x16 form, one MFMA per
// fragment: no difference (B = 1: 87.7 vs
// 87.0 ms per chain, B = 128: within box noise) — a lone wavefront's M slot takes 41 cycles per MFMA in either order (slot trace:
// 984 cycles), so the accumulate latency is not what stretches it; the order stays because it costs nothing and one ring loop
// is simpler than three.
// what the next M slot of this wavefront starts with (tail prefetch): a full record (mixed order), the block's last record
// (GEMM2 only) or the next block's attention record (A_s)
enum { NEXT_FULL = 0, NEXT_LAST = 1, NEXT_AS = 2 };
template <int NEXT>
__device__ __forceinline__ constexpr int next_frag(int i) { return NEXT == NEXT_FULL ? ff_frag(i) : NEXT == NEXT_LAST ? w2_frag(i) : as_frag(i); }

// On 16x16x32 tiles (denoiser_ff16.h): every fragment m = 0..23 of a full record feeds TWO MFMAs back to back, one per 16-point N-tile —
// 48 MFMAs of 8 passes for the 24 of 16 passes before, still 24 ds_read_b128 and the same LDS bytes per FLOP; P[m & 7] is refilled behind
// the second MFMA of its pair.  GEMM1: 2 (a, g) x 2 M-tiles x 4 K steps (K steps 0..3 in order per accumulator quad); GEMM2: 8 M-tiles
// of h, one K = 32 instruction per quad and chunk (v_mfma_f32_16x16x32_f16), chunks 0..15 in order — the order of every kernel on this pack.
template <bool S3, bool S1, int NEXT, class Issue>
__device__ __forceinline__ void ff_m(v16f (&h)[4], const Act<DFX_PREC_BF16> (&xn)[4], v16f &a, v16f &g,
                                     const HidAct &hid, const uint4 *ck, uint4 (&P)[8], const uint4 *ck_next, Tracer &tr,
                                     Issue &issue) {
  __builtin_amdgcn_sched_barrier(0);
  tr.stamp(4);
  if (MFMA_PRIO) __builtin_amdgcn_s_setprio(MFMA_PRIO);
  auto gemm1 = [&](int e, const uint4 &w) {   // GEMM1 fragment e = 0..15; K step 0 starts from C = 0 (inline constant): b1' rides on the constant-one K slot (bias_slot_one), no initialiser reads
    const ff16::Op op = ff16::gemm1_op(e);
    mma16_w1(op.part ? g : a, op.mt, w, xn[op.c], op.c == 0);
  };
  auto gemm2 = [&](int i, const uint4 &w) {   // GEMM2 fragment i = 0..7
    const ff16::Op op = ff16::gemm2_op(i);
    mma16_w2(h[op.c], op.mt, w, hid.f[0], hid.f[1]);
  };
  if (S3 && S1) {
#pragma unroll
    for (int m = 0; m < 24; ++m) {   // P is a ring of eight fragment registers: fragment m sits in P[m & 7], refilled in place with fragment m + 8
      const int k = m / 3, r = m % 3;
      if (r == 0) gemm2(k, P[m & 7]);
      else gemm1(2 * k + r - 1, P[m & 7]);
      issue.at(m, 24);
      P[m & 7] = m + 8 < 24 ? ck[ff_frag(m + 8)] : ck_next[next_frag<NEXT>(m + 8 - 24)];
    }
  } else if (S1) {                  // first FF record of a block: GEMM1 only; P holds its first eight fragments
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      gemm1(m, P[m & 7]);
      issue.at(m, 16);
      P[m & 7] = m + 8 < 16 ? ck[w1_frag((m + 8) & 7, (m + 8) >> 3)] : ck_next[next_frag<NEXT>(m + 8 - 16)];
    }
  } else {                          // last FF record of a block: GEMM2 only
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      gemm2(i, P[i]);
      issue.at(i, 8);
      P[i] = ck_next[next_frag<NEXT>(i)];
    }
  }
  // keep the program order MFMA, MFMA, read, MFMA, MFMA, read, ...
#pragma unroll
  for (int i = 0; i < (S3 && S1 ? 24 : S1 ? 16 : 8); ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  if (MFMA_PRIO) __builtin_amdgcn_s_setprio(0);
}

// V slot of the feed-forward: hid = a * gelu(g) as the fp16 B operand of GEMM2.
__device__ __forceinline__ void ff_v(v16f &a, v16f &g, HidAct &hid, Tracer &tr) {
  if (VALU_PRIO) __builtin_amdgcn_s_setprio(VALU_PRIO);
  h2 aa[8], gg[8];
  gelu16_f16_cvt(a, g, aa, gg);
  gelu16_f16_math(aa, gg, hid);
  // Pin the result here: without a use in this slot LLVM sinks the whole GELU past the record barrier into the
  // consumer's M slot, and the two groups' VALU bursts collide instead of running in anti-phase.
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    v4u w = __builtin_bit_cast(v4u, hid.f[q]);
    asm volatile("" : "+v"(w));
    hid.f[q] = __builtin_bit_cast(uint4, w);
  }
  tr.stamp(8);
  if (VALU_PRIO) __builtin_amdgcn_s_setprio(0);
}

// attention M slots: sim = sbias + A_s xn (8 MFMAs);  h += M_s P (8 MFMAs)
template <class Issue>
__device__ __forceinline__ void attn_m0(v16f &sim, const Act<DFX_PREC_BF16> (&xn)[4], const uint4 *rec, const float *sbias,
                                        uint4 (&P)[8], bool have_p, Issue &issue) {
  if (!have_p) {
#pragma unroll
    for (int i = 0; i < 8; ++i) P[i] = rec[as_frag(i)];
  }
  load16(sim, sbias);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sim = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(P[i]), xn[i >> 1].f[i & 1], sim, 0, 0, 0);
    issue.at(i, 8);
    P[i] = rec[ms_frag(i)];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void attn_m1(v16f (&h)[4], const Act<DFX_PREC_BF16> &pa, const uint4 *rec, uint4 (&P)[8],
                                        const uint4 *ck_next) {
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    h[i & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(P[i]), pa.f[i >> 2], h[i & 3], 0, 0, 0);
    P[i] = ck_next[w1_frag(i, 0)];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// attention V slot: softmax over the 4 keys of each head (registers 4g..4g+3 = keys of head 2g+hf; masked through sbias), on register pairs
__device__ __forceinline__ void attn_softmax(v16f &sim, Act<DFX_PREC_BF16> &pa) {
  softmax4_pk(sim);   // (every bf16 kernel takes the same reciprocal; +0.25 % in a same-box A/B)
  pa.set(sim);
}

// post_norm (affine folded into W_out) + proj_out (128 -> 3) on the VALU.
__device__ __forceinline__ void post_eps(const v16f (&h)[4], const float4 *wout, const float (&bout)[4],
                                         float (&eps)[3]) {
  float mean, rstd;
  ln_stats(h, mean, rstd);
  float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float4 w = wout[c * 16 + r];
      const float v = (h[c][r] - mean) * rstd;
      e0 = fmaf(w.x, v, e0);
      e1 = fmaf(w.y, v, e1);
      e2 = fmaf(w.z, v, e2);
    }
  eps[0] = e0 + xhalf(e0) + bout[0];
  eps[1] = e1 + xhalf(e1) + bout[1];
  eps[2] = e2 + xhalf(e2) + bout[2];
}
// four channels (registers 4j .. 4j+3 of a tile, normalised two at a time) of the three eps chains: (e_x, e_y) packed, e_z scalar, channel after
// channel as ever
__device__ __forceinline__ void post_eps4_pk(const v16f &ht, int j, const v2f &rstd2, const v2f &nmr2, const Pair2 &w, v2f &e01, float &e2) {
  const v2f va = __builtin_elementwise_fma(pair(ht, 2 * j), rstd2, nmr2), vb = __builtin_elementwise_fma(pair(ht, 2 * j + 1), rstd2, nmr2);
  e01 = __builtin_elementwise_fma(w.at(0), splat2(va[0]), e01);
  e2 = fmaf(w.at(2)[0], va[0], e2);
  e01 = __builtin_elementwise_fma(w.at(1), splat2(va[1]), e01);
  e2 = fmaf(w.at(2)[1], va[1], e2);
  e01 = __builtin_elementwise_fma(w.at(3), splat2(vb[0]), e01);
  e2 = fmaf(w.at(5)[0], vb[0], e2);
  e01 = __builtin_elementwise_fma(w.at(4), splat2(vb[1]), e01);
  e2 = fmaf(w.at(5)[1], vb[1], e2);
}
// post_eps of the bf16 chain kernels, on the W_out pair table of this half-wave (`woutp`: + hf * 32 pairs)
__device__ __forceinline__ void post_eps_pk(const v16f (&h)[4], const float *woutp, const float (&bout)[4], float (&eps)[3]) {
  float mean, rstd;
  ln_stats_fast(h, mean, rstd);
  const float nmr = -mean * rstd;
  const v2f rstd2 = splat2(rstd), nmr2 = splat2(nmr);
  v2f e01 = {0.f, 0.f};
  float e2 = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) post_eps4_pk(h[c], j, rstd2, nmr2, load_pair2(woutp + (c * 4 + j) * 2 * PAIR_WOUT), e01, e2);
  eps[0] = e01[0] + xhalf(e01[0]) + bout[0];
  eps[1] = e01[1] + xhalf(e01[1]) + bout[1];
  eps[2] = e2 + xhalf(e2) + bout[2];
}

// Timestep of the step-th executed step (wave-uniform): T-1, T-2, ... for DDPM, the list for DDIM.
template <int KIND = CHAIN_GENERAL>
__device__ __forceinline__ int step_t(const KParams &p, int step, int s) {
  if constexpr (KIND == CHAIN_PLAIN) return p.t0 - step;
  if (p.t_shape) return __builtin_amdgcn_readfirstlane(p.t_shape[s]);   // wave-uniform (one shape per wave)
  if (p.ddim_n > 0) return p.ddim_t[step < p.ddim_n ? step : p.ddim_n - 1];
  return p.t0 - step;
}

// Per-point state that lives in registers for the whole chain.
struct PointState {
  float x[3], anc[3], var[3], L[3];
  int s, n, sg;
  unsigned long long gid;
  bool live = true;   // false: a wavefront past the end of its shape's last (partial) 256-point tile recomputes that shape's last 32 points and stores nothing
};

// Partial chains (the FROM instantiations of the kernels; MODE_CHAIN only).  ps.x holds the caller's x_in.  START_GIVEN: that is the state entering
// the first executed timestep (a DDPM launch over the whole chain, nsteps == T, also records it as the t = T snapshot).  START_QSAMPLE: x_in is a
// clean cloud, forward-noised here to the first executed timestep t = nsteps-1 in k_q_sample's expression order, no contraction — bit-identical to
// dfx_q_sample_f32 followed by START_GIVEN.  Its noise is the caller's xT_noise or the Philox stream of the x_T draw (stream 1) keyed by nsteps:
// the step noise (stream 0) never meets it.
__device__ __forceinline__ void chain_start_from(const KParams &p, PointState &ps, int hf) {
  if (p.start == START_QSAMPLE) {
#pragma clang fp contract(off)
    float z[3];
    if (p.xT_noise) {
#pragma unroll
      for (int i = 0; i < 3; ++i) z[i] = p.xT_noise[((size_t)ps.s * 3 + i) * p.N + ps.n];
    } else {
      philox_normal3(p.seed, ps.gid, (unsigned)p.nsteps, 1u, z);
    }
    const float qa = p.d.qtab[(p.nsteps - 1) * 2], qb = p.d.qtab[(p.nsteps - 1) * 2 + 1];
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.x[i] = qa * (ps.x[i] - ps.anc[i]) + ps.anc[i] + qb * ps.L[i] * z[i];
  } else if (p.traj && p.ddim_n == 0 && p.nsteps == p.d.T && p.d.T % p.ret_interval == 0 && hf == 0 && ps.live) {
    float *o = p.traj + ((size_t)ps.s * p.N + ps.n) * 3;  // snapshot 0 <-> t = T
    o[0] = ps.x[0]; o[1] = ps.x[1]; o[2] = ps.x[2];
  }
}

// One point of `pred` or of a snapshot.  In a partial chain a point of a held part (hold bit of its part id) is written as the caller's x_in:
// decided here, from the part id and the shape's mask, and re-read from global memory — nothing of it travels through the step loop.
template <int KIND>
__device__ __forceinline__ void chain_store(const KParams &p, const PointState &ps, float *o) {
  if constexpr (KIND == CHAIN_FROM) {
    if (p.hold && ((p.hold[ps.s] >> ps.sg) & 1)) {
#pragma unroll
      for (int i = 0; i < 3; ++i) o[i] = p.x_in[((size_t)ps.s * 3 + i) * p.N + ps.n];
      return;
    }
  }
  o[0] = ps.x[0]; o[1] = ps.x[1]; o[2] = ps.x[2];
}

// FROM: the instantiation for partial chains (dfx_sample_chain_from / dfx_refine_chain / dfx_sample_chain_ddim_from).  Every kernel exists twice,
// and the generation kernels (FROM = false) compile to what they were before partial chains existed.
template <int KIND = CHAIN_GENERAL>
__device__ __forceinline__ void point_init(const KParams &p, PointState &ps, int s, int n, unsigned long long gid,
                                           unsigned &vmask) {
  ps.s = s; ps.n = n; ps.gid = gid;
  const float *part = p.part + (size_t)s * 32;
  ps.sg = p.seg[(size_t)s * p.N + n];  // replaces gather_operation (part_encoders.py:417-428)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ps.anc[i] = part[i * 4 + ps.sg];
    ps.var[i] = part[12 + i * 4 + ps.sg];
    ps.L[i] = sqrtf(ps.var[i]);  // anchored_diffusion.py:306 / :562
  }
  vmask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) vmask |= (part[24 + j] != 0.f ? 1u : 0u) << j;  // mask.to(bool), attention.py:196
  vmask = __builtin_amdgcn_readfirstlane(vmask);
  const int hf = (threadIdx.x >> 5) & 1;
  if constexpr (KIND == CHAIN_PLAIN) {   // x_T = a + L z, z from the Philox stream of the x_T draw
    float z[3];
    philox_normal3(p.seed, gid, (unsigned)p.d.T, 1u, z);
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.x[i] = ps.L[i] * z[i] + ps.anc[i];  // anchored_diffusion.py:563-564
  } else if constexpr (KIND == CHAIN_FROM) {
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.x[i] = p.x_in[((size_t)s * 3 + i) * p.N + n];
    chain_start_from(p, ps, hf);
  } else if (p.mode == MODE_CHAIN) {
    float z[3];
    if (p.xT_noise) {
#pragma unroll
      for (int i = 0; i < 3; ++i) z[i] = p.xT_noise[((size_t)s * 3 + i) * p.N + n];
    } else {
      philox_normal3(p.seed, gid, (unsigned)p.d.T, 1u, z);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.x[i] = ps.L[i] * z[i] + ps.anc[i];  // anchored_diffusion.py:563-564
    if (p.traj && p.d.T % p.ret_interval == 0 && hf == 0 && ps.live) {
      float *o = p.traj + ((size_t)s * p.N + n) * 3;  // snapshot 0 <-> t = T
      o[0] = ps.x[0]; o[1] = ps.x[1]; o[2] = ps.x[2];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.x[i] = p.x_in[((size_t)s * 3 + i) * p.N + n];
  }
}

// What happens to eps after the network: store it (MODE_EPS), or the anchored posterior update
// (anchored_diffusion.py:306-319,365-367,378-380,401-409,175-213,476-483; reference op order, no contraction)
// plus the bookkeeping of AnchorDiffAE.decode (anchor_gen.py:160-167).  Returns true when the kernel is done.
// PLAIN: the DDPM posterior of a MODE_CHAIN launch and nothing else; `tab_row` is the table row of t, fetched by the caller (one scalar load at the top
// of the step boundary in the pipelined kernels, the idle wavefront's copy in LDS in the co-operative ones).  The store of `pred` at t = 0 is the one
// place that writes global memory.
template <int KIND = CHAIN_GENERAL>
__device__ __forceinline__ bool step_epilogue(const KParams &p, PointState &ps, const float (&eps)[3], int step, int t,
                                              const float *z_ready = nullptr, const float *tab_row = nullptr) {
  const int hf = ps.live ? (threadIdx.x >> 5) & 1 : 1;   // stores are done by half-wave 0 of live wavefronts
  const int s = ps.s, n = ps.n;
  if constexpr (KIND == CHAIN_PLAIN) {
    float z[3];
    if (z_ready) {
#pragma unroll
      for (int i = 0; i < 3; ++i) z[i] = z_ready[i];
    } else {
      philox_normal3(p.seed, ps.gid, (unsigned)t, 0u, z);
    }
    {
#pragma clang fp contract(off)
      const float *tb = tab_row;
      const float sra = tb[0], srm1 = tb[1], c1 = tb[2], c2 = tb[3], c3 = tb[4], pv = tb[5];
      const float nz = t != 0 ? 1.0f : 0.0f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float x0 = sra * (ps.x[i] - ps.anc[i]) + ps.anc[i] - srm1 * ps.L[i] * eps[i];
        const float mv = pv * ps.var[i];
        const float mu = c1 * x0 + c2 * ps.x[i] + c3 * ps.anc[i];
        ps.x[i] = mu + nz * sqrtf(mv) * z[i];
      }
    }
    if (hf == 0 && t == 0) chain_store<KIND>(p, ps, p.out + ((size_t)s * p.N + n) * 3);
    return false;
  }
  if (p.mode == MODE_EPS) {
    if (hf == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) p.out[((size_t)s * 3 + i) * p.N + n] = eps[i];
    }
    return true;
  }
  float z[3];
  if (z_ready) {   // (co-operative kernel: an idle wavefront has drawn the noise and fetched the table row already)
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i] = z_ready[i];
  } else if (p.noise) {
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i] = p.noise[(((size_t)step * p.B + s) * 3 + i) * p.N + n];
  } else {
    philox_normal3(p.seed, ps.gid, (unsigned)t, 0u, z);
  }
  {
#pragma clang fp contract(off)
    const float *tb = tab_row ? tab_row : p.d.tab + (size_t)t * 8;
    const float sra = tb[0], srm1 = tb[1], c1 = tb[2], c2 = tb[3], c3 = tb[4], pv = tb[5];
    const float nz = t != 0 ? 1.0f : 0.0f;
    const bool ddim = p.ddim_n > 0;
    const float sap = sqrtf(tb[6]);   // torch.sqrt of the fp32 alphas_cumprod_prev[t] (:481)
    const float xdc = ddim ? p.ddim_xdc[step < p.ddim_n ? step : p.ddim_n - 1] : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float x0 = sra * (ps.x[i] - ps.anc[i]) + ps.anc[i] - srm1 * ps.L[i] * eps[i];
      if (p.xstart && hf == 0) p.xstart[((size_t)s * 3 + i) * p.N + n] = x0;
      const float mv = pv * ps.var[i];
      if (ddim) {   // (x0 - a) sqrt(acp_prev) + a + L xt_dir_coeff eps + eta 1[t != 0] sqrt(var) z
        const float xt_dir = ps.L[i] * xdc * eps[i];
        ps.x[i] = (x0 - ps.anc[i]) * sap + ps.anc[i] + xt_dir + p.ddim_eta * nz * sqrtf(mv) * z[i];
      } else {
        const float mu = c1 * x0 + c2 * ps.x[i] + c3 * ps.anc[i];
        ps.x[i] = mu + nz * sqrtf(mv) * z[i];
      }
    }
  }
  if (p.mode == MODE_PSAMPLE) {
    if (hf == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) p.out[((size_t)s * 3 + i) * p.N + n] = ps.x[i];
    }
    return true;
  }
  if (hf == 0) {
    if (t == 0) {
      chain_store<KIND>(p, ps, p.out + ((size_t)s * p.N + n) * 3);
    } else if (p.traj && t % p.ret_interval == 0) {
      const int k = p.d.T / p.ret_interval - t / p.ret_interval;
      chain_store<KIND>(p, ps, p.traj + (((size_t)k * p.B + s) * p.N + n) * 3);
    }
  }
  return false;
}

// ----------------------------------------------------------------------------------------------
// v0 "direct" kernel: every operand comes straight from global memory (L2-resident).  Any N % 32 == 0,
// both precisions.  It is the general fallback and the exact-fp32 parity path.
template <int PREC, int NW, bool FROM = false>
__global__ void __launch_bounds__(NW * 64) k_denoise(const KParams p) {
  constexpr int TSTRIDE = tile_units(PREC) * 64;  // uint4 elements per 32x32 weight tile
  constexpr int AREC = asms_bytes(PREC) / 16;     // uint4 per attention record
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hf = lane >> 5, pj = lane & 31;
  const long long g0 = ((long long)blockIdx.x * NW + wave) * 32;
  if (g0 >= (long long)p.B * p.N) return;
  const int s = __builtin_amdgcn_readfirstlane((int)(g0 / p.N));
  const int n = (int)(g0 - (long long)s * p.N) + pj;
  const int depth = p.d.depth;
  PointState ps;
  unsigned vmask;
  point_init<FROM>(p, ps, s, n, ((unsigned long long)p.shape0 + (unsigned)s) * (unsigned)p.N + (unsigned)n, vmask);
  const float *cpart = p.cpart + ((size_t)s * NCLS + ps.sg) * INNER + hf * 64;
  const uint4 *asms_s = p.as_ms + (size_t)s * depth * AREC + lane;

  for (int step = 0; step < p.nsteps; ++step) {
    const int t = step_t(p, step, s);
    v16f h[4];
    proj_in_prenorm(h, ps.x, cpart, p.d.win_x + hf * 64, p.d.pre_gb + hf * 64);
    for (int b = 0; b < depth; ++b) {
      const BlockPack &bp = p.d.blk[b];
      const uint4 *rec = asms_s + (size_t)b * AREC;
      attention<PREC>(h, rec, reinterpret_cast<const float *>(rec - lane + 8 * TSTRIDE) + hf * 16,
                      bp.ct + (size_t)t * CT_ROW + hf * 64, vmask);
      Act<PREC> xn[4];
      ln_to_act<PREC>(h, xn);
      const bool fold = p.d.w1_fold != 0;   // (wave-uniform)
      if (fold) bias_slot_one(xn, hf);
      constexpr bool FF16 = PREC == DFX_PREC_BF16;   // the bf16 feed-forward runs on 16x16x32 tiles: b1' in that order (k_pack_b1)
      if (FF16) ff16_rows(xn), ff16_rows(h);
#pragma unroll 1
      for (int u = 0; u < FF_CHUNKS; ++u)
        ff_chunk(h, xn, bp.chunks + (size_t)u * CHUNK_TILES * TSTRIDE + lane,
                 bp.chunks + (size_t)(u + FF_SKEW) * CHUNK_TILES * TSTRIDE + lane, bp.bconst + u * 64 + (FF16 ? (lane >> 4) * 8 : hf * 16), fold);
      if (FF16) ff16_rows(h);
      add_cvec<FF16>(h, bp.bconst + BCONST_B2_OFF + hf * 64);
    }
    float eps[3];
    post_eps(h, p.d.wout + hf * 64, p.d.bout, eps);
    if (step_epilogue<FROM>(p, ps, eps, step, t)) return;
  }
}

// ----------------------------------------------------------------------------------------------
// LDS-pipelined kernel (bf16): one workgroup = 8 wavefronts = 256 points of ONE shape (a partial last tile idles wavefronts).
//
// Weight streaming.  All weights stream L2 -> LDS through a 5-slot ring of 24 KiB records filled by LDS-DMA
// (global_load_lds_dwordx4: 1 KiB per wavefront-instruction, 3 per wave per record), three records ahead of the
// compute, with a counted s_waitcnt vmcnt (never 0 in steady state).  Record sequence per transformer block:
// [attention record] then 17 x [FF record j = W1 of chunk j | W2 of chunk j-1].  The DMA is issued from inline asm so
// that hipcc does not serialise the ring behind vmcnt(0) waits (it cannot prove that a ds_read does not alias an
// in-flight LDS-DMA); the data hazards are handled by the slot protocol below.
//
// Slots.  Each wavefront alternates pure-VALU slots (V) and pure-MFMA slots (M).  Group B (waves 4-7) runs one
// slot behind group A (waves 0-3): each record's management barrier (below) is in front of A's M slot but in
// front of B's preceding V slot, and waves w / w+4 share a SIMD, so after every barrier one wavefront of each
// SIMD starts an MFMA burst while its partner starts a VALU burst:
//     block:  V0 (b2 of the previous block | step boundary | LN2)  M0 (A_s)  V1 (softmax)  M1 (M_s)  V2 (+c_t, LN3)
//             M(F0: GEMM1 0)  V (GELU 0)  M(F1: GEMM2 0 + GEMM1 1)  V (GELU 1) ... M(F16: GEMM2 15)
// One barrier per record per wavefront; both groups execute the same number of barriers.  Every M slot ends by reading
// the first eight A fragments of the wave's NEXT M slot (tail prefetch, ff_m / attn_m0 / attn_m1).
//
// Ring protocol.  The barrier in front of the M slot that first reads record r (for group A; for B it is the
// barrier in front of the preceding V slot — the SAME global barrier) is r's management barrier:
//     before it  every wave waits for its own DMA pieces of r+1 (vmcnt(its pieces per record): r+2 may still be in flight)
//     after it   every wave issues its pieces of record r+3 into slot (r+3)%5
//   RAW: the issuing waves' vmcnt + the barrier precede every read of r and every tail-prefetch read of r+1.
//   WAR: slot (r+3)%5 held record r-2, whose last reader (B; for an attention record B's V2, which ends before the
//        management barrier of r) finished at least one barrier earlier.
// Wavefronts per workgroup: 8 (256 points) when that fills the chip; 4 or 2 for small batches, so that a single shape still
// spreads over 16 / 32 CUs (same per-wave instruction stream, bit-identical results; the ring then takes 6 / 12 pieces per wave).
constexpr int SLOT_BYTES = 24 * 1024;
constexpr int NSLOT = 5;   // records in flight ahead of the compute: NSLOT - 2

// Ring DMA: 24 pieces of 1 KiB per record, 24 / NW per wavefront.
constexpr int RING_PIECES = SLOT_BYTES / 1024;
constexpr int RECORDS_PER_BLOCK = 1 + FF_STAGES;
// LDS map (bytes)
constexpr int L_RING = 0;
constexpr int L_BCONST = L_RING + NSLOT * SLOT_BYTES;  // 2 x block-constant record (b1', b2)
constexpr int L_WINX = L_BCONST + 2 * BCONST_BYTES;    // float4[128]; bf16 kernel: pair table (pair_tables), 1.5 KiB of it
constexpr int L_PREGB = L_WINX + 2048;                 // float2[128]; bf16 kernel: pair table
constexpr int L_WOUT = L_PREGB + 1024;                 // float4[128]; bf16 kernel: pair table, 1.5 KiB of it
constexpr int L_CPART = L_WOUT + 2048;                 // float[4][128]
constexpr int L_DUMMY = L_CPART + 2048;                // sink for padding DMAs (one wave's pieces)
constexpr int PSTATE_FIELDS = 13;                      // x[3] anc[3] var[3] L[3] seg
template <int NW>
struct PipeCfg {
  static_assert(NW == 8 || NW == 4 || NW == 2, "wavefronts per workgroup");
  static constexpr int CALLS = RING_PIECES / NW;                       // ring pieces per wave and record
  static constexpr int PTS = NW * 32;                                  // points per workgroup
  static constexpr int L_PSTATE = L_DUMMY + CALLS * 1024;              // per-point chain state parked between steps: float[13][PTS]
  static constexpr int L_TOTAL = L_PSTATE + PSTATE_FIELDS * PTS * 4;
  static_assert(L_TOTAL <= 160 * 1024, "LDS budget");
};
static_assert(asms_bytes(DFX_PREC_BF16) + 1024 <= SLOT_BYTES && chunk_bytes(DFX_PREC_BF16) == SLOT_BYTES, "slot layout");

extern __shared__ __attribute__((aligned(1024))) unsigned char pipe_smem[];

// one 1 KiB LDS-DMA: lane l copies 16 B from gbase + voff(l) to LDS byte address lds_addr + 16 l
__device__ __forceinline__ void dma1k(const void *gbase, unsigned voff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(gbase), "s"(lds_addr)
               : "memory");  // m0 is reserved: hipcc re-materialises it before each of its own uses
}
__device__ __forceinline__ const char *pin_ptr(const char *q) {   // wave-uniform pointer -> scalar registers
  const unsigned long long g = (unsigned long long)(uintptr_t)q;
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(g >> 32)), lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)g);
  return (const char *)(uintptr_t)(((unsigned long long)hi << 32) | lo);   // (the builtin returns int: no sign extension of `lo`)
}
// the same with the (wave-uniform by construction) operands pinned to scalar registers: behind a chain of uniform selects hipcc
// may hold them in VGPRs, which the "s" constraints reject
__device__ __forceinline__ void dma1k_pinned(const void *gbase, unsigned voff, unsigned lds_addr) {
  dma1k(pin_ptr(reinterpret_cast<const char *>(gbase)), voff, (unsigned)__builtin_amdgcn_readfirstlane(lds_addr));
}

// N consecutive 1 KiB pieces: the instruction's immediate offset applies to BOTH the global and the LDS address
// (checked on gfx950: tools/ubench/dma_offset.hip), so one M0 / one SGPR base serve all of them
#define DFX_DMA_HEAD "s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
#define DFX_DMA_MORE(off) "\n\tglobal_load_lds_dwordx4 %0, %1 offset:" #off
#define DFX_DMA_ASM(str) asm volatile(str ::"v"(voff), "s"(gbase), "s"(lds_addr) : "memory")
template <int N>
__device__ __forceinline__ void dma_nk(const void *gbase, unsigned voff, unsigned lds_addr) {   // ONE asm block per four pieces: M0 stays ours
  static_assert(N >= 0 && N <= 12, "pieces per wave");
  if constexpr (N > 4) {   // the immediate offset has 12 bits
    dma_nk<4>(gbase, voff, lds_addr);
    dma_nk<N - 4>(reinterpret_cast<const char *>(gbase) + 4096, voff, lds_addr + 4096);
  } else {
    if (N == 1) DFX_DMA_ASM(DFX_DMA_HEAD);
    if (N == 2) DFX_DMA_ASM(DFX_DMA_HEAD DFX_DMA_MORE(1024));
    if (N == 3) DFX_DMA_ASM(DFX_DMA_HEAD DFX_DMA_MORE(1024) DFX_DMA_MORE(2048));
    if (N == 4) DFX_DMA_ASM(DFX_DMA_HEAD DFX_DMA_MORE(1024) DFX_DMA_MORE(2048) DFX_DMA_MORE(3072));
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Block b's pack = block 0's + b * stride: plain scalar arithmetic instead of a look-up in the kernel-argument table
// (an s_load whose s_waitcnt lgkmcnt(0) also drains every LDS read in flight, once per record).
__device__ __forceinline__ BlockPack block_pack(const KParams &p, int b) {
  const long long off = (long long)b * p.d.blk_stride;
  return BlockPack{reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(p.d.blk[0].chunks) + off),
                   reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.d.blk[0].bconst) + off),
                   reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.d.blk[0].ct) + off)};
}

// Next record to fetch (all wave-uniform).
struct DmaState {
  int step, b, k, seq, slot;  // k: 0 = attention record, 1..17 = FF record k-1; seq = running block number
  const char *ff_src;         // this wave's window of the next FF record
};

// The attention record of block st.b for shape s: 17 KiB shape record | 5 KiB block constants | 1 KiB c_t row | 1 padding piece.  Everything here is
// wave-uniform, and it is spelled so that it STAYS on the scalar unit (the record is prepared right in front of a V slot, whose issue slots are the
// wavefront's critical path): the shape record's offset is one 32 x 32 -> 64-bit product of scalar registers (written as (size_t)s * depth it shared the
// 64-bit copy of `s` that the per-lane addresses keep in a VGPR pair, and the product, the pointer and the selects behind it all ran on the VALU), and the
// timestep is looked up once, by the one wavefront whose pieces include the c_t row, not once per piece.
struct AttnRecord {
  const char *as, *bconst, *ct_row;
  unsigned ring, bc, dummy;   // LDS: the ring slot, this block's block-constant buffer, the padding sink
  __device__ __forceinline__ void piece(int q, const char *&src, unsigned &dst) const {
    src = bconst, dst = dummy;
    if (q < 17) src = as + q * 1024, dst = ring + q * 1024;
    else if (q < 22) src = bconst + (q - 17) * 1024, dst = bc + (q - 17) * 1024;
    else if (q == 22) src = ct_row, dst = ring + 17 * 1024;
  }
};
template <int KIND>
__device__ __forceinline__ AttnRecord attn_record(const KParams &p, const DmaState &st, const BlockPack &bp, int q0, int nc, unsigned ring, unsigned lds0, int s) {
  AttnRecord r;
  const unsigned rec = (unsigned)__builtin_amdgcn_readfirstlane(s * p.d.depth + st.b);
  r.as = reinterpret_cast<const char *>(p.as_ms) + (unsigned long long)rec * (unsigned)asms_bytes(DFX_PREC_BF16);
  r.bconst = reinterpret_cast<const char *>(bp.bconst);
  r.ct_row = r.bconst;
  if (q0 <= 22 && 22 < q0 + nc) r.ct_row = reinterpret_cast<const char *>(bp.ct + (size_t)step_t<KIND>(p, st.step, s) * CT_ROW);
  r.ring = ring, r.bc = lds0 + L_BCONST + (st.seq & 1) * BCONST_BYTES, r.dummy = lds0 + L_DUMMY;
  return r;
}

// Issue this wave's pieces (CALLS_A / CALLS_B of them, starting at piece q0) of the next record and advance the state.
template <int NC, int KIND>
__device__ __forceinline__ void issue_pieces(const KParams &p, DmaState &st, int q0, unsigned voff, unsigned lds0, int s) {
  const unsigned ring = lds0 + L_RING + st.slot * SLOT_BYTES;
  if (NC == 0) {
  } else if (st.step >= p.nsteps) {  // past the end: padding pieces keep the vmcnt bookkeeping uniform
    dma_nk<NC>(p.d.blk[0].chunks, voff, lds0 + L_DUMMY);
  } else if (st.k > 0) {  // FF record: 24 contiguous KiB (the common case: keep it lean)
    dma_nk<NC>(st.ff_src, voff, ring + q0 * 1024);
    st.ff_src += SLOT_BYTES;
  } else {  // attention record: 17 KiB shape record | 5 KiB block constants | 1 KiB c_t row | 1 padding piece
    const BlockPack bp = block_pack(p, st.b);
    const AttnRecord ar = attn_record<KIND>(p, st, bp, q0, NC, ring, lds0, s);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const char *src;
      unsigned dst;
      ar.piece(q0 + j, src, dst);
      dma1k_pinned(src, voff, dst);
    }
    st.ff_src = reinterpret_cast<const char *>(bp.chunks) + q0 * 1024;
  }
}

// The same bookkeeping, but only the (wave-uniform) source / destination of this wave's pieces: the loads themselves are
// issued one at a time from inside the wave's next M slot (Issuer).
template <int NC>
struct Pieces {
  const char *src[NC];
  unsigned dst[NC];
};
template <int NC, int KIND>
__device__ __forceinline__ void prepare_pieces(const KParams &p, DmaState &st, int q0, unsigned lds0, int s, Pieces<NC> &pc) {
  const unsigned ring = lds0 + L_RING + st.slot * SLOT_BYTES;
  if (st.step >= p.nsteps) {
#pragma unroll
    for (int j = 0; j < NC; ++j) pc.src[j] = reinterpret_cast<const char *>(p.d.blk[0].chunks), pc.dst[j] = lds0 + L_DUMMY;
  } else if (st.k > 0) {
#pragma unroll
    for (int j = 0; j < NC; ++j) pc.src[j] = st.ff_src + j * 1024, pc.dst[j] = ring + (q0 + j) * 1024;
    st.ff_src += SLOT_BYTES;
  } else {
    const BlockPack bp = block_pack(p, st.b);
    const AttnRecord ar = attn_record<KIND>(p, st, bp, q0, NC, ring, lds0, s);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const char *src;
      unsigned dst;
      ar.piece(q0 + j, src, dst);
      pc.src[j] = pin_ptr(src), pc.dst[j] = (unsigned)__builtin_amdgcn_readfirstlane(dst);   // (the "s" operands of the DMA: no-ops on scalar registers)
    }
    st.ff_src = reinterpret_cast<const char *>(bp.chunks) + q0 * 1024;
  }
}

__device__ __forceinline__ void advance_record(const KParams &p, DmaState &st) {
  st.slot = st.slot + 1 == NSLOT ? 0 : st.slot + 1;
  if (++st.k == RECORDS_PER_BLOCK) {
    st.k = 0;
    ++st.seq;
    if (++st.b == p.d.depth) {
      st.b = 0;
      ++st.step;
    }
  }
}

template <int NW, int KIND>
__device__ __forceinline__ void issue_record(const KParams &p, DmaState &st, int wave, unsigned voff, unsigned lds0, int s) {
  issue_pieces<PipeCfg<NW>::CALLS, KIND>(p, st, wave * PipeCfg<NW>::CALLS, voff, lds0, s);
  advance_record(p, st);
}

// The DMA of the record three ahead is issued one piece at a time from inside the wave's own M slot, between MFMAs (the two
// groups' M slots are in anti-phase, so at most four waves issue at a time, one KiB per ~250 cycles).  Issued all at once
// behind the record's management barrier, the eight waves' 24 KiB hit the texture-address path (64 B/clk) together and
// every wave sits ~400 cycles in the issue stall on the critical path of the record (slot trace, tools/experiments/run_trace.sh).
template <int NW, int KIND>
struct Issuer {
  static constexpr int CALLS = PipeCfg<NW>::CALLS;
  // 8-wave workgroups fill the chip: their pieces are spread over the M slot (comment above).  The 4- and 2-wave workgroups of
  // small batches (<= 32 workgroups in flight, no contention on the texture-address path) issue theirs at once behind the
  // record's management barrier: 6 / 12 (source, destination) pairs would not fit the scalar registers of the M slot.
  static constexpr bool SPREAD = NW == 8;
  const KParams &p;
  DmaState &st;
  int wave;
  unsigned voff, lds0;
  int s;
  Pieces<SPREAD ? CALLS : 1> pc;
  // (scalar) source / destination bookkeeping of the pieces of the next M slot; runs in the V slot before it
  __device__ __forceinline__ void m_begin() {
    if constexpr (SPREAD) {
      prepare_pieces<CALLS, KIND>(p, st, wave * CALLS, lds0, s, pc);
      advance_record(p, st);
    }
  }
  // right behind a record's management barrier
  __device__ __forceinline__ void after_barrier() {
    if constexpr (!SPREAD) issue_record<NW, KIND>(p, st, wave, voff, lds0, s);
  }
  // after MFMA i of the n of an M slot
  __device__ __forceinline__ void at(int i, int n) {
    if constexpr (SPREAD) {
#pragma unroll
      for (int k = 0; k < CALLS; ++k)
        if (i == (k * n) / CALLS) dma1k(pc.src[k], voff, pc.dst[k]);
    }
  }
};

// One row of the posterior table ([T][8] floats, 32-byte rows of a 256-byte-aligned array that no kernel writes) through the scalar unit: the address is
// wave-uniform, and read through the constant address space the row is ONE s_load_dwordx8 — as a plain global pointer hipcc cannot prove that the
// kernel's own stores leave it alone and fetches it per lane.
struct TabRow {
  float v[8];
  __device__ __forceinline__ void fetch(const float *tab, int t) {
    typedef __attribute__((address_space(4))) const v8f *cv8;
    const v8f r = *(cv8)(uintptr_t)(tab + (size_t)t * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = r[i];
  }
};

// The per-point state (x_t, anchor, variance, sqrt(variance), part id) is touched once per diffusion step; parked in LDS
// in between (13 KiB per workgroup) it costs no VGPRs during the 90 record slots of a step — hipcc would otherwise keep
// it in scratch memory (80 B per lane: ~8 MB of write-back traffic per step and launch).
__device__ __forceinline__ void pstate_store(float *ps_lds, int pt, int PTS, const PointState &ps, bool all) {
#pragma unroll
  for (int i = 0; i < 3; ++i) ps_lds[i * PTS + pt] = ps.x[i];
  if (all) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ps_lds[(3 + i) * PTS + pt] = ps.anc[i];
      ps_lds[(6 + i) * PTS + pt] = ps.var[i];
      ps_lds[(9 + i) * PTS + pt] = ps.L[i];
    }
    ps_lds[12 * PTS + pt] = __int_as_float(ps.sg);
  }
}
__device__ __forceinline__ void pstate_load(const float *ps_lds, int pt, int PTS, PointState &ps, bool all) {
#pragma unroll
  for (int i = 0; i < 3; ++i) ps.x[i] = ps_lds[i * PTS + pt];
  if (all) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ps.anc[i] = ps_lds[(3 + i) * PTS + pt];
      ps.var[i] = ps_lds[(6 + i) * PTS + pt];
      ps.L[i] = ps_lds[(9 + i) * PTS + pt];
    }
  }
  ps.sg = __float_as_int(ps_lds[12 * PTS + pt]);
}

template <int NW, int KIND = CHAIN_GENERAL>
__global__ void __launch_bounds__(NW * 64, 2) k_denoise_pipe(const KParams p) {
  constexpr int PREC = DFX_PREC_BF16;
  constexpr int PIPE_NW = NW, PTS = PipeCfg<NW>::PTS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hf = lane >> 5, pj = lane & 31;
  // XCD-aware placement: workgroups are handed to the 8 XCDs round-robin by blockIdx, and every XCD has its own 4 MiB
  // L2.  All workgroups stream the same block weights (2 MiB per step), but the attention records are per shape
  // (85 KiB each): with the natural order the wpg workgroups of one shape land on wpg different XCDs and every L2 sees
  // every shape.  Remap so that consecutive workgroups of ONE XCD walk through the workgroups of one shape.
  const int wpg = (p.N + PIPE_NW * 32 - 1) / (PIPE_NW * 32);   // workgroups per shape (the last one may be partial)
  int bid = blockIdx.x;
  {
    const int per = 8 * wpg;                        // workgroups of 8 shapes = one remap period
    const int full = ((int)gridDim.x / per) * per;  // the tail (B % 8 shapes) keeps the natural order
    if (bid < full) {
      const int x = bid & 7, q = (bid % per) >> 3;  // XCD, position on that XCD within the period (0 .. wpg-1)
      bid = (bid / per) * per + x * wpg + q;        // shape (period*8 + x), workgroup q of it
    }
  }
  // one shape per workgroup; N % 32 == 0, so whole wavefronts fall off the end of a shape's last tile: those recompute the
  // shape's last 32 points (same barriers, same DMA duties) and store nothing
  const int s = __builtin_amdgcn_readfirstlane(bid / wpg);
  int n0 = __builtin_amdgcn_readfirstlane((bid - s * wpg) * (PIPE_NW * 32) + wave * 32);
  const bool live = n0 < p.N;
  if (!live) n0 = p.N - 32;
  const int n = n0 + pj;
  const unsigned long long gid = ((unsigned long long)p.shape0 + (unsigned)s) * (unsigned)p.N + (unsigned)n;   // Philox key: GLOBAL point id
  const int depth = p.d.depth;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)pipe_smem);
  const unsigned voff = lane * 16;
  const bool grpA = wave < PIPE_NW / 2;

  // ---- prologue DMA: records 0, 1, 2 in flight while the per-point state is set up ----
  DmaState dma{0, 0, 0, 0, 0, nullptr};
  issue_record<NW, KIND>(p, dma, wave, voff, lds0, s);
  issue_record<NW, KIND>(p, dma, wave, voff, lds0, s);
  issue_record<NW, KIND>(p, dma, wave, voff, lds0, s);

  // ---- chain-invariant small operands -> LDS (plain loads; not part of the ring) ----
  {   // (W_in, pre_norm, W_out: the pair tables of proj_in_prenorm_pk / post_eps_pk, inside the regions of the one-float4-per-channel form)
    float *cp = reinterpret_cast<float *>(pipe_smem + L_CPART);
    const int tid = threadIdx.x;
    if (tid < 64)
      pair_tables(p.d, tid, reinterpret_cast<float *>(pipe_smem + L_WINX), reinterpret_cast<float *>(pipe_smem + L_PREGB), reinterpret_cast<float *>(pipe_smem + L_WOUT));
    for (int i = tid; i < NCLS * INNER; i += NW * 64) cp[i] = p.cpart[(size_t)s * NCLS * INNER + i];
  }
  unsigned vmask;
  float *ps_lds = reinterpret_cast<float *>(pipe_smem + PipeCfg<NW>::L_PSTATE);
  const int pt = wave * 32 + pj;   // point slot inside the workgroup (both half-waves hold the same point)
  {
    PointState ps0;
    ps0.live = live;
    point_init<KIND>(p, ps0, s, n, gid, vmask);
    pstate_store(ps_lds, pt, PTS, ps0, true);   // both half-waves hold the same point: identical values
  }
  __syncthreads();

  const float *winx = reinterpret_cast<const float *>(pipe_smem + L_WINX) + hf * 32 * PAIR_WIN;
  const float *pregb = reinterpret_cast<const float *>(pipe_smem + L_PREGB) + hf * 32 * PAIR_PREGB;
  const float *wout = reinterpret_cast<const float *>(pipe_smem + L_WOUT) + hf * 32 * PAIR_WOUT;

  Issuer<NW, KIND> issue_in_m{p, dma, wave, voff, lds0, s, {}};
  // slot boundary; `mgmt` = this barrier is a record's management barrier for this wave's group
#define DFX_SLOT(mgmt)                   \
  do {                                   \
    __builtin_amdgcn_sched_barrier(0);   \
    if (mgmt) {                          \
      tr.stamp(1);                       \
      wait_vmcnt<PipeCfg<NW>::CALLS>();  \
      __builtin_amdgcn_s_barrier();      \
      tr.stamp(2);                       \
      issue_in_m.after_barrier();        \
    } else {                             \
      tr.stamp(3);                       \
    }                                    \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)
  // pointer to this lane's view of the record in ring slot `cur`, then advance
#define DFX_NEXT_RECORD()                                                               \
  do {                                                                                  \
    ck = reinterpret_cast<const uint4 *>(pipe_smem + L_RING + cur * SLOT_BYTES) + lane; \
    cur = cur + 1 == NSLOT ? 0 : cur + 1;                                               \
  } while (0)
  // the record that the next DFX_NEXT_RECORD() will hand out (complete in LDS since the previous management barrier)
#define DFX_PEEK_RECORD() (reinterpret_cast<const uint4 *>(pipe_smem + L_RING + cur * SLOT_BYTES) + lane)

#ifdef DFX_TRACE
  Tracer tr{(p.trace != nullptr && bid == 0 && (wave & 3) == 0) ? p.trace + (size_t)(wave >> 2) * p.trace_cap : nullptr,
            p.trace_cap, 0};
#else
  Tracer tr;
#endif

  uint4 P[8];   // first MFMA batch of the next M slot (tail prefetch)
  int cur = 0;  // ring slot of the next record to be consumed
  int seq = 0;  // running block number (parity selects the block-constant buffer)
  v16f h[4];
  bool done = false;
  for (int step = 0; step <= p.nsteps && !done; ++step) {
    for (int b = 0; b < depth; ++b, ++seq) {
      const uint4 *ck;
      Act<PREC> xn[4];
      // ---- V0: finish the previous block / step, start this one ----
      DFX_SLOT(!grpA && step < p.nsteps);
      issue_in_m.m_begin();
      if (seq > 0) {  // the previous block's h back to one point per lane (32 swaps), + its b2 (other block-constant buffer)
        ff16_rows(h);
        add_cvec<true>(h, reinterpret_cast<const float *>(pipe_smem + L_BCONST + ((seq - 1) & 1) * BCONST_BYTES) +
                              BCONST_B2_OFF + hf * 64);
      }
      if (b == 0) {
        PointState ps;
        ps.s = s, ps.n = n, ps.gid = gid, ps.live = live;
        TabRow row;
        if constexpr (KIND == CHAIN_PLAIN) {   // the posterior's table row: one scalar load, under the state's LDS reads and post_eps
          if (step > 0) row.fetch(p.d.tab, step_t<KIND>(p, step - 1, s));
        }
        pstate_load(ps_lds, pt, PTS, ps, step > 0);
        if (step > 0) {
          float eps[3];
          post_eps_pk(h, wout, p.d.bout, eps);
          if constexpr (KIND == CHAIN_PLAIN) {
            step_epilogue<KIND>(p, ps, eps, step - 1, step_t<KIND>(p, step - 1, s), nullptr, row.v);
          } else {
            done = step_epilogue<KIND>(p, ps, eps, step - 1, step_t(p, step - 1, s));
          }
          if (!done) pstate_store(ps_lds, pt, PTS, ps, false);   // both half-waves hold the same point and write the same x
        }
        if (step == p.nsteps) done = true;
        if (!done) {
          const float *cpart = reinterpret_cast<const float *>(pipe_smem + L_CPART) + ps.sg * INNER + hf * 64;
          proj_in_prenorm_pk(h, ps.x, cpart, winx, pregb);
        }
      }
      if (done) break;
      ln_to_act<PREC>(h, xn);
      // ---- M0: sim = sbias + A_s xn ----
      DFX_SLOT(grpA);
      DFX_NEXT_RECORD();
      const uint4 *rec = ck;
      v16f sim;
      attn_m0(sim, xn, rec, reinterpret_cast<const float *>(rec - lane + 1024) + hf * 16, P, seq > 0, issue_in_m);
      // ---- V1: softmax ----
      DFX_SLOT(false);
      Act<PREC> pa;
      attn_softmax(sim, pa);
      // ---- M1: h += M_s P ----
      DFX_SLOT(false);
      attn_m1(h, pa, rec, P, DFX_PEEK_RECORD());
      // ---- V2: + c_t, LN3 ----
      DFX_SLOT(!grpA);
      issue_in_m.m_begin();
      add_cvec<true>(h, reinterpret_cast<const float *>(rec - lane + 1088) + hf * 64);
      ln_to_act<PREC>(h, xn);
      // ---- feed-forward: M(F0) V M(F1) V ... M(F16) ----
      v16f a, g;
      HidAct hid;
      bias_slot_one(xn, hf);   // b1' enters GEMM1 through channel 127's K slot: no accumulator initialisers
      ff16_rows(xn);           // 16 + 32 row swaps: xn and h in the feed-forward's 16x16x32 form until the next V0
      ff16_rows(h);
      DFX_SLOT(grpA);
      DFX_NEXT_RECORD();
      ff_m<false, true, NEXT_FULL>(h, xn, a, g, hid, ck, P, DFX_PEEK_RECORD(), tr, issue_in_m);
#pragma unroll 1
      for (int j = 1; j < FF_CHUNKS - 1; ++j) {
        DFX_SLOT(!grpA);
        issue_in_m.m_begin();
        ff_v(a, g, hid, tr);
        DFX_SLOT(grpA);
        DFX_NEXT_RECORD();
        ff_m<true, true, NEXT_FULL>(h, xn, a, g, hid, ck, P, DFX_PEEK_RECORD(), tr, issue_in_m);
      }
      DFX_SLOT(!grpA);   // record F15: the next one is the block's last (GEMM2 only): its tail prefetch differs
      issue_in_m.m_begin();
      ff_v(a, g, hid, tr);
      DFX_SLOT(grpA);
      DFX_NEXT_RECORD();
      ff_m<true, true, NEXT_LAST>(h, xn, a, g, hid, ck, P, DFX_PEEK_RECORD(), tr, issue_in_m);
      DFX_SLOT(!grpA);
      issue_in_m.m_begin();
      ff_v(a, g, hid, tr);
      DFX_SLOT(grpA);
      DFX_NEXT_RECORD();
      ff_m<true, false, NEXT_AS>(h, xn, a, g, hid, ck, P, DFX_PEEK_RECORD(), tr, issue_in_m);
    }
  }
#undef DFX_SLOT
#undef DFX_NEXT_RECORD
#undef DFX_PEEK_RECORD
  wait_vmcnt<0>();  // drain padding DMAs before the LDS allocation is released
}

// ----------------------------------------------------------------------------------------------
// LDS-pipelined kernel, exact fp32 (v_mfma_f32_32x32x2_f32): the reference-precision sampler.  The reference computes in
// fp32 end to end (attention.py:296-306, anchored_diffusion.py:227-395); this is that arithmetic at the structure of the bf16
// chain kernel — one workgroup = NW wavefronts x 32 points of one shape, the residual stream in registers for the whole chain,
// the posterior fused, and every weight streamed L2 -> LDS through the same 5-slot ring of 24 KiB records by LDS-DMA three
// records ahead, one workgroup barrier per record.  Same device functions and the same MFMA order per accumulator as the direct
// kernel k_denoise<DFX_PREC_F32>: the results are bit-identical (tested), so every golden of the fp32 path holds for it.
//
// What differs from the bf16 kernel is the balance: an fp32 MFMA is 64 cycles of matrix pipe for 4 bytes of A operand per lane
// (the bf16 one: 32 cycles for 16 bytes), so operand delivery is a twentieth of the bf16 kernel's — one ds_read_b128 feeds four
// MFMAs — and the fp32 VALU work (LayerNorm, softmax, erf-GELU, posterior) is ~15 % of the matrix time of one wavefront, hidden by
// the other wavefront of the SIMD without any slot choreography.  The direct kernel takes every fragment from L2 (~600 cycles
// away, 4 KiB tiles, two or three requests in flight per wavefront) and idles the matrix pipe 70 % of the time; here the pipe waits only
// at the record barriers.
//
// Ring records (24 KiB = six fp32 tiles = 24 DMA pieces of 1 KiB; RECORDS_F32 = 2 + 2 x 17 per transformer block):
//     k = 0      A_s tiles 0..3 | sbias piece (+16 KiB) | c_t row (+17 KiB); block constants -> their own double buffer
//     k = 1      M_s tiles 0..3
//     k = 2 + 2j FF record j, first half:  W1 g-rows x k-tiles 0..3 (tiles 4..7 of the packed record) | W1 a-rows x k-tiles 0, 1
//     k = 3 + 2j FF record j, second half: W1 a-rows x k-tiles 2, 3 | W2 row tiles 0..3 x hidden chunk j-1 (tiles 8..11)
// so g is complete after the first half and the second half ends with the MFMAs that do not feed the GELU (GEMM2 of the chunk before).
// Second half of FF record j of the fp32 chain: `a` x k-tiles 2, 3 (tiles 0, 1 of the half-record) and GEMM2 of chunk j - 1 (tiles 2..5),
// with the erf of chunk j's g BEHIND the MFMAs: g is complete since the first half, an fp32 MFMA keeps the matrix pipe busy for 64
// cycles after its issue, and the wave spends them on the VALU — gelu_erf(g[r]) overwrites g[r], one element per NM / 16 MFMAs
// (erff branches per lane; that only cuts basic blocks, the MFMAs in flight do not care).  Before this the two wavefronts of a SIMD
// reached the GELU together and the pipe idled for its whole length (80 % busy).  Same MFMA order per accumulator, same GELU
// function on the same values: bit-identical to the direct kernel.
template <bool FIRST, bool LAST>
__device__ __forceinline__ void ff_f32_second_half(v16f (&h)[4], const Act<DFX_PREC_F32> (&xn)[4], v16f &a, v16f &g, Act<DFX_PREC_F32> &hid,
                                                   const uint4 *rl) {
  constexpr int TS = tile_units(DFX_PREC_F32) * 64;
  constexpr int T0 = LAST ? 2 : 0, T1 = FIRST ? 2 : 6;   // tiles of the half-record that carry MFMAs here
  constexpr int NM = (T1 - T0) * 16, PER = NM / 16;
  v4f w = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const int t = T0 + m / 16, r4 = (m % 16) / 4, e = m % 4;
    if (e == 0) w = __builtin_bit_cast(v4f, rl[t * TS + r4 * 64]);
    if (t < 2) a = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], xn[2 + t].x[4 * r4 + e], a, 0, 0, 0);
    else h[t - 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], hid.x[4 * r4 + e], h[t - 2], 0, 0, 0);
    if constexpr (!LAST) {
      if ((m + 1) % PER == 0) {
        const int r = (m + 1) / PER - 1;
        g[r] = gelu_erf(g[r]);
      }
    }
  }
  if constexpr (!LAST) {
#pragma unroll
    for (int r = 0; r < 16; ++r) hid.x[r] = a[r] * g[r];
  }
}

constexpr int RECORDS_F32 = 2 + 2 * FF_STAGES;
static_assert(tile_bytes(DFX_PREC_F32) * 6 == SLOT_BYTES && asms_bytes(DFX_PREC_F32) == 33 * 1024, "fp32 ring records");

struct DmaStateF {
  int step, b, k, seq, slot;
};

template <int NC>
__device__ __forceinline__ void issue_pieces_f32(const KParams &p, const DmaStateF &st, int q0, unsigned voff, unsigned lds0, int s) {
  const unsigned ring = lds0 + L_RING + st.slot * SLOT_BYTES;
  if (st.step >= p.nsteps) {  // past the end: padding pieces keep the vmcnt bookkeeping uniform
    dma_nk<NC>(p.d.blk[0].chunks, voff, lds0 + L_DUMMY);
    return;
  }
  const BlockPack bp = block_pack(p, st.b);
  const char *asms = reinterpret_cast<const char *>(p.as_ms) + ((size_t)s * p.d.depth + st.b) * asms_bytes(DFX_PREC_F32);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int q = q0 + j;
    const char *src = reinterpret_cast<const char *>(bp.bconst);   // padding piece
    unsigned dst = lds0 + L_DUMMY;
    if (st.k == 0) {
      if (q < 16) src = asms + q * 1024, dst = ring + q * 1024;
      else if (q == 16) src = asms + 32 * 1024, dst = ring + 16 * 1024;
      else if (q < 22) src = reinterpret_cast<const char *>(bp.bconst) + (q - 17) * 1024, dst = lds0 + L_BCONST + (st.seq & 1) * BCONST_BYTES + (q - 17) * 1024;
      else if (q == 22) src = reinterpret_cast<const char *>(bp.ct + (size_t)step_t(p, st.step, s) * CT_ROW), dst = ring + 17 * 1024;
    } else if (st.k == 1) {
      if (q < 16) src = asms + (16 + q) * 1024, dst = ring + q * 1024;
    } else {
      const char *rec = reinterpret_cast<const char *>(bp.chunks) + (size_t)((st.k - 2) >> 1) * chunk_bytes(DFX_PREC_F32);
      if (((st.k - 2) & 1) == 0) src = rec + (q < 16 ? (16 + q) * 1024 : (q - 16) * 1024);
      else src = rec + (q < 8 ? (8 + q) * 1024 : (32 + q - 8) * 1024);
      dst = ring + q * 1024;
    }
    dma1k_pinned(src, voff, dst);
  }
}

template <int NW>
__device__ __forceinline__ void issue_record_f32(const KParams &p, DmaStateF &st, int wave, unsigned voff, unsigned lds0, int s) {
  issue_pieces_f32<PipeCfg<NW>::CALLS>(p, st, wave * PipeCfg<NW>::CALLS, voff, lds0, s);
  st.slot = st.slot + 1 == NSLOT ? 0 : st.slot + 1;
  if (++st.k == RECORDS_F32) {
    st.k = 0;
    ++st.seq;
    if (++st.b == p.d.depth) {
      st.b = 0;
      ++st.step;
    }
  }
}

template <int NW, bool FROM = false>
__global__ void __launch_bounds__(NW * 64, 2) k_denoise_pipe_f32(const KParams p) {
  constexpr int PREC = DFX_PREC_F32;
  constexpr int PTS = PipeCfg<NW>::PTS, TS = tile_units(PREC) * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hf = lane >> 5, pj = lane & 31;
  // XCD-aware placement and tile bookkeeping: as in k_denoise_pipe
  const int wpg = (p.N + NW * 32 - 1) / (NW * 32);
  int bid = blockIdx.x;
  {
    const int per = 8 * wpg;
    const int full = ((int)gridDim.x / per) * per;
    if (bid < full) {
      const int x = bid & 7, q = (bid % per) >> 3;
      bid = (bid / per) * per + x * wpg + q;
    }
  }
  const int s = __builtin_amdgcn_readfirstlane(bid / wpg);
  int n0 = __builtin_amdgcn_readfirstlane((bid - s * wpg) * (NW * 32) + wave * 32);
  const bool live = n0 < p.N;
  if (!live) n0 = p.N - 32;
  const int n = n0 + pj;
  const unsigned long long gid = ((unsigned long long)p.shape0 + (unsigned)s) * (unsigned)p.N + (unsigned)n;
  const int depth = p.d.depth;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)pipe_smem);
  const unsigned voff = lane * 16;

  DmaStateF dma{0, 0, 0, 0, 0};
  issue_record_f32<NW>(p, dma, wave, voff, lds0, s);
  issue_record_f32<NW>(p, dma, wave, voff, lds0, s);
  issue_record_f32<NW>(p, dma, wave, voff, lds0, s);
  {
    float4 *winx = reinterpret_cast<float4 *>(pipe_smem + L_WINX);
    float2 *pregb = reinterpret_cast<float2 *>(pipe_smem + L_PREGB);
    float4 *wout = reinterpret_cast<float4 *>(pipe_smem + L_WOUT);
    float *cp = reinterpret_cast<float *>(pipe_smem + L_CPART);
    const int tid = threadIdx.x;
    if (tid < 128) {
      winx[tid] = p.d.win_x[tid];
      pregb[tid] = p.d.pre_gb[tid];
      wout[tid] = p.d.wout[tid];
    }
    for (int i = tid; i < NCLS * INNER; i += NW * 64) cp[i] = p.cpart[(size_t)s * NCLS * INNER + i];
  }
  unsigned vmask;
  float *ps_lds = reinterpret_cast<float *>(pipe_smem + PipeCfg<NW>::L_PSTATE);
  const int pt = wave * 32 + pj;
  {
    PointState ps0;
    ps0.live = live;
    point_init<FROM>(p, ps0, s, n, gid, vmask);
    pstate_store(ps_lds, pt, PTS, ps0, true);
  }
  __syncthreads();
  const float4 *winx = reinterpret_cast<const float4 *>(pipe_smem + L_WINX) + hf * 64;
  const float2 *pregb = reinterpret_cast<const float2 *>(pipe_smem + L_PREGB) + hf * 64;
  const float4 *wout = reinterpret_cast<const float4 *>(pipe_smem + L_WOUT) + hf * 64;

  // record boundary: this wave's pieces of the record after next have landed, everybody is done with the slot that is refilled next
  // (ring protocol of k_denoise_pipe), then the pieces of the record three ahead are issued
#ifdef DFX_TRACE   // phase stamps of waves 0 and 4 (one SIMD) of workgroup 0: tools/experiments/trace_f32.py
  Tracer tr{(p.trace != nullptr && bid == 0 && (wave & 3) == 0) ? p.trace + (size_t)(wave >> 2) * p.trace_cap : nullptr, p.trace_cap, 0};
#else
  Tracer tr;
#endif
#define DFX_RECORD(ptr)                                                                      \
  do {                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    tr.stamp(1);                                                                             \
    wait_vmcnt<PipeCfg<NW>::CALLS>();                                                        \
    __builtin_amdgcn_s_barrier();                                                            \
    tr.stamp(2);                                                                             \
    issue_record_f32<NW>(p, dma, wave, voff, lds0, s);                                       \
    tr.stamp(3);                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    ptr = reinterpret_cast<const uint4 *>(pipe_smem + L_RING + cur * SLOT_BYTES);            \
    cur = cur + 1 == NSLOT ? 0 : cur + 1;                                                    \
  } while (0)

  int cur = 0, seq = 0;
  v16f h[4];
  bool done = false;
  for (int step = 0; step <= p.nsteps && !done; ++step) {
    for (int b = 0; b < depth; ++b, ++seq) {
      const float *bc = reinterpret_cast<const float *>(pipe_smem + L_BCONST + (seq & 1) * BCONST_BYTES);
      if (seq > 0)  // b2 of the previous block (other block-constant buffer)
        add_cvec(h, reinterpret_cast<const float *>(pipe_smem + L_BCONST + ((seq - 1) & 1) * BCONST_BYTES) + BCONST_B2_OFF + hf * 64);
      if (b == 0) {
        PointState ps;
        ps.s = s, ps.n = n, ps.gid = gid, ps.live = live;
        pstate_load(ps_lds, pt, PTS, ps, step > 0);
        if (step > 0) {
          float eps[3];
          post_eps(h, wout, p.d.bout, eps);
          done = step_epilogue<FROM>(p, ps, eps, step - 1, step_t(p, step - 1, s));
          if (!done) pstate_store(ps_lds, pt, PTS, ps, false);
        }
        if (step == p.nsteps) done = true;
        if (!done) proj_in_prenorm(h, ps.x, reinterpret_cast<const float *>(pipe_smem + L_CPART) + ps.sg * INNER + hf * 64, winx, pregb);
      }
      if (done) break;
      const uint4 *rec;
      Act<PREC> xn[4];
      ln_to_act<PREC>(h, xn);
      // ---- attention: sim = sbias + A_s LN2(h);  P = softmax4;  h += M_s P + c_t ----
      DFX_RECORD(rec);
      const float *ct = reinterpret_cast<const float *>(rec) + 17 * 256 + hf * 64;   // (read during the NEXT record: its slot is refilled one barrier later)
      v16f sim;
      load16(sim, reinterpret_cast<const float *>(rec) + 16 * 256 + hf * 16);
#pragma unroll
      for (int c = 0; c < 4; ++c) mma_tile<PREC>(sim, rec + lane + c * TS, xn[c]);
      softmax4(sim, vmask);
      Act<PREC> pa;
      pa.set(sim);
      DFX_RECORD(rec);
#pragma unroll
      for (int t = 0; t < 4; ++t) mma_tile<PREC>(h[t], rec + lane + t * TS, pa);
      add_cvec(h, ct);
      ln_to_act<PREC>(h, xn);
      // ---- feed-forward: 17 records of two halves; GEMM2 of chunk j-1 rides in the second half of record j ----
      Act<PREC> hid;
      v16f a, g;
      auto first_half = [&](int j) {   // g x k-tiles 0..3, a x k-tiles 0, 1
        load16(a, bc + j * 64 + hf * 16);
        load16(g, bc + j * 64 + hf * 16 + 32);
#pragma unroll
        for (int c = 0; c < 4; ++c) mma_tile<PREC>(g, rec + lane + c * TS, xn[c]);
#pragma unroll
        for (int c = 0; c < 2; ++c) mma_tile<PREC>(a, rec + lane + (4 + c) * TS, xn[c]);
      };
      DFX_RECORD(rec);
      first_half(0);
      DFX_RECORD(rec);
      ff_f32_second_half<true, false>(h, xn, a, g, hid, rec + lane);
#pragma unroll 1
      for (int j = 1; j < FF_CHUNKS; ++j) {
        DFX_RECORD(rec);
        first_half(j);
        DFX_RECORD(rec);
        ff_f32_second_half<false, false>(h, xn, a, g, hid, rec + lane);
      }
      DFX_RECORD(rec);   // (record 16, first half: zero tiles of the packed layout — consumed to keep the ring uniform)
      DFX_RECORD(rec);
      ff_f32_second_half<false, true>(h, xn, a, g, hid, rec + lane);
    }
  }
#undef DFX_RECORD
  wait_vmcnt<0>();  // drain padding DMAs before the LDS allocation is released
}

// The step boundary runs on one wavefront with nobody to hide its LDS latency behind: the same arithmetic as post_eps /
// proj_in_prenorm_pk (operation for operation — the results are bit-identical), with the operand reads of half a 16-channel tile
// issued ahead of the half before's arithmetic (hipcc, short of registers over the whole kernel, otherwise reads one operand at a time).
// (fences: an empty asm that consumes the batch's results and clobbers memory — reads cannot cross it, the arithmetic is tied to it by its
// data; a sched_barrier alone orders only what instruction selection has already laid out, and that is every read first.)
#define DFX_TIE4(a) asm volatile("" : "+v"((a)[0]), "+v"((a)[1]), "+v"((a)[2]), "+v"((a)[3]) :: "memory")   // (four register pairs)
__device__ __forceinline__ void post_eps_tiles(const v16f (&h)[4], const float *woutp, const float (&bout)[4], float (&eps)[3]) {
  float mean, rstd;
  ln_stats_fast(h, mean, rstd);
  const float nmr = -mean * rstd;
  const v2f rstd2 = splat2(rstd), nmr2 = splat2(nmr);
  v2f e01 = {0.f, 0.f};
  float e2 = 0.f;
  Pair2 w[2][2];   // half a tile per batch
#pragma unroll
  for (int j = 0; j < 2; ++j) w[0][j] = load_pair2(woutp + j * 2 * PAIR_WOUT);
  asm volatile("" : "+v"(e01), "+v"(e2) :: "memory");
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < 7) {
#pragma unroll
      for (int j = 0; j < 2; ++j) w[(k + 1) & 1][j] = load_pair2(woutp + ((k + 1) * 2 + j) * 2 * PAIR_WOUT);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) post_eps4_pk(h[k >> 1], (k & 1) * 2 + j, rstd2, nmr2, w[k & 1][j], e01, e2);
    asm volatile("" : "+v"(e01), "+v"(e2) :: "memory");
  }
  eps[0] = e01[0] + xhalf(e01[0]) + bout[0];
  eps[1] = e01[1] + xhalf(e01[1]) + bout[1];
  eps[2] = e2 + xhalf(e2) + bout[2];
}

__device__ __forceinline__ void proj_in_prenorm_tiles(v16f (&h)[4], const float (&x)[3], const float *cpart, const float *winp, const float *pregp) {
  const v2f x2[3] = {splat2(x[0]), splat2(x[1]), splat2(x[2])};
  Pair2 w[2][2];
  v4f cp[2][2];
  auto fetch = [&](int k) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      cp[k & 1][j] = *reinterpret_cast<const v4f *>(cpart + k * 8 + j * 4);
      w[k & 1][j] = load_pair2(winp + (k * 2 + j) * 2 * PAIR_WIN);
    }
  };
  fetch(0);
  asm volatile("" ::: "memory");
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < 7) fetch(k + 1);
    v16f &ht = h[k >> 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) proj_in4_pk(ht, (k & 1) * 2 + j, x2, cp[k & 1][j], w[k & 1][j]);
    v2f o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pair(ht, (k & 1) * 4 + i);
    DFX_TIE4(o);
#pragma unroll
    for (int i = 0; i < 4; ++i) set_pair(ht, (k & 1) * 4 + i, o[i]);
  }
  v4f gb[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) gb[0][i] = *reinterpret_cast<const v4f *>(pregp + i * PAIR_PREGB);
  float mean, rstd;
  ln_stats_fast(h, mean, rstd);
  asm volatile("" : "+v"(mean), "+v"(rstd) :: "memory");
  const v2f mean2 = splat2(mean), rstd2 = splat2(rstd);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < 7) {
#pragma unroll
      for (int i = 0; i < 4; ++i) gb[(k + 1) & 1][i] = *reinterpret_cast<const v4f *>(pregp + ((k + 1) * 4 + i) * PAIR_PREGB);
    }
    v2f o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const v4f g = gb[k & 1][i];
      o[i] = __builtin_elementwise_fma((pair(h[k >> 1], (k & 1) * 4 + i) - mean2) * rstd2, v2f{g[0], g[1]}, v2f{g[2], g[3]});
    }
    DFX_TIE4(o);
#pragma unroll
    for (int i = 0; i < 4; ++i) set_pair(h[k >> 1], (k & 1) * 4 + i, o[i]);
  }
}

// ---- Shared by k_denoise_coop and k_denoise_coop2: what happens inside a phase.  Each kernel keeps its own schedule (its barriers, which wave does
// what, where W2 lives); what differs inside a phase comes in as an argument: an LDS pointer, a tile index, n.
constexpr int COOP_NW = 8, COOP_TILES = 4;
static_assert(FF_CHUNKS == 2 * COOP_NW, "two rounds of one chunk per wavefront");
constexpr int COOP_TSTRIDE = tile_units(DFX_PREC_BF16) * 64, COOP_AREC = asms_bytes(DFX_PREC_BF16) / 16;
// chain-invariant operands in LDS (7 KiB): pair tables of W_in x-columns (1.5 of 2 KiB) | pre_norm (1 KiB) | W_out (1.5 of 2 KiB); cpart of the workgroup's shape (2 KiB)
constexpr int CC_WINX = 0, CC_PREGB = 2048, CC_WOUT = 3072, CC_CPART = 5120, CC_BYTES = 7 * 1024;

__device__ __forceinline__ void coop_stage_consts(unsigned char *cc, const KParams &p, int s) {   // (the caller's barrier publishes them)
  float *c_cp = reinterpret_cast<float *>(cc + CC_CPART);
  const int tid = threadIdx.x;
  if (tid < 64) pair_tables(p.d, tid, reinterpret_cast<float *>(cc + CC_WINX), reinterpret_cast<float *>(cc + CC_PREGB), reinterpret_cast<float *>(cc + CC_WOUT));
  c_cp[tid] = p.cpart[(size_t)s * NCLS * INNER + tid];
}

// The 32 points of tile (s, n - pj): initial chain state -> its LDS home between step boundaries
// (the state would otherwise sit in scratch memory for the whole chain: a global-memory round trip per field at every step boundary)
template <int KIND>
__device__ __forceinline__ void coop_point_init(const KParams &p, float *ps_lds, int s, int n, int pj, unsigned &vmask) {
  PointState ps0;
  point_init<KIND>(p, ps0, s, n, ((unsigned long long)p.shape0 + (unsigned)s) * (unsigned)p.N + (unsigned)n, vmask);
  pstate_store(ps_lds, pj, 32, ps0, true);
}

// GEMM1 fragments of chunk u -> R[base .. base + 15], in the accumulation order a(c,0) a(c,1) g(c,0) g(c,1), c = 0..3
// (scalar base + lane offset: with the base pinned to SGPRs the sixteen loads share one address VGPR; left to itself hipcc keeps
// 64-bit per-lane addresses, spills them, and every scratch reload — a vector-memory operation like the prefetches in flight —
// drains the whole prefetch with s_waitcnt vmcnt(0))
__device__ __forceinline__ void coop_load_w1(uint4 (&R)[32], int base, const uint4 *chunks, int u, int lane) {
  constexpr int TSTRIDE = COOP_TSTRIDE;
  const uint4 *ck = reinterpret_cast<const uint4 *>(pin_ptr(reinterpret_cast<const char *>(chunks + (size_t)u * CHUNK_TILES * TSTRIDE))) + lane;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    R[base + 4 * c + 0] = ck[(0 + c) * TSTRIDE], R[base + 4 * c + 1] = ck[(0 + c) * TSTRIDE + 64];
    R[base + 4 * c + 2] = ck[(4 + c) * TSTRIDE], R[base + 4 * c + 3] = ck[(4 + c) * TSTRIDE + 64];
  }
}
// W2 fragments of chunks first .. first + 7, output tile ct -> R[2 u], R[2 u + 1] (W2 of chunk u sits in FF record u + FF_SKEW, tiles 8..11)
__device__ __forceinline__ void coop_load_w2(uint4 (&R)[32], int first, const uint4 *chunks, int ct, int lane) {
  constexpr int TSTRIDE = COOP_TSTRIDE;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint4 *ck = reinterpret_cast<const uint4 *>(pin_ptr(reinterpret_cast<const char *>(chunks + (size_t)(first + c + FF_SKEW) * CHUNK_TILES * TSTRIDE + (8 + ct) * TSTRIDE))) + lane;
    R[2 * (first + c)] = ck[0], R[2 * (first + c) + 1] = ck[64];
  }
}

// h's LDS home of one 32-point tile (16 KiB): channel tile c, quad q of lane l at float4 index (4 c + q) * 64 + l.  `home` = the tile's home + lane,
// `hc` = home + 256 c, one channel tile of it.
__device__ __forceinline__ void hs_load(v16f &h, const v4f *hc) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const v4f x = hc[q * 64];
    h[4 * q] = x[0], h[4 * q + 1] = x[1], h[4 * q + 2] = x[2], h[4 * q + 3] = x[3];
  }
}
__device__ __forceinline__ void hs_store(v4f *hc, const v16f &h) {
#pragma unroll
  for (int q = 0; q < 4; ++q) hc[q * 64] = v4f{h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]};
}
__device__ __forceinline__ void hs_store_plus(v4f *hc, const v16f &h, const float *b) {   // h + b: the 16 values of b follow the accumulator's order
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const v4f bb = *reinterpret_cast<const v4f *>(b + 4 * q);
    const v2f lo = pair(h, 2 * q) + v2f{bb[0], bb[1]}, hi = pair(h, 2 * q + 1) + v2f{bb[2], bb[3]};   // (packed, as add_cvec<true>)
    hc[q * 64] = v4f{lo[0], lo[1], hi[0], hi[1]};
  }
}
__device__ __forceinline__ void hs_load4(v16f (&h)[4], const v4f *home) {
#pragma unroll
  for (int c = 0; c < 4; ++c) hs_load(h[c], home + c * 256);
}
__device__ __forceinline__ void hs_store4(v4f *home, const v16f (&h)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) hs_store(home + c * 256, h[c]);
}

// Attention record of a block (`arec`: 17 pieces of 1 KiB) | its c_t row at time t (1) | its block constants (5) -> LDS by LDS-DMA: the 23 pieces go
// round NWAVES issuing wavefronts, `slot` = this wave's place among them
template <int NWAVES>
__device__ __forceinline__ void coop_stage_block(const BlockPack &bp, const uint4 *arec, int t, int slot, unsigned voff, unsigned lds_at, unsigned lds_bc) {
  constexpr int NA = asms_bytes(DFX_PREC_BF16) / 1024, NB = BCONST_BYTES / 1024;
#pragma unroll
  for (int i = 0; i < (NA + 1 + NB + NWAVES - 1) / NWAVES; ++i) {
    const int k = i * NWAVES + slot;
    if (k < NA) dma1k_pinned(reinterpret_cast<const char *>(arec) + k * 1024, voff, lds_at + k * 1024);
    else if (k == NA) dma1k_pinned(reinterpret_cast<const char *>(bp.ct + (size_t)t * CT_ROW), voff, lds_at + NA * 1024);
    else if (k < NA + 1 + NB) dma1k_pinned(reinterpret_cast<const char *>(bp.bconst) + (k - NA - 1) * 1024, voff, lds_bc + (k - NA - 1) * 1024);
  }
}

// Phase A of one tile: attention and LayerNorm 3 on h (from its home and back), xn3 -> s_xn as the B operand of GEMM1 (k-th uint4: tile k >> 1, unit k & 1)
__device__ __forceinline__ void coop_phase_a(v4f *home, const uint4 *s_at, uint4 (*s_xn)[64], int lane, unsigned vmask) {
  constexpr int PREC = DFX_PREC_BF16;
  const int hf = lane >> 5;
  v16f h[4];
  hs_load4(h, home);
  attention<PREC>(h, s_at + lane, reinterpret_cast<const float *>(s_at + 8 * COOP_TSTRIDE) + hf * 16, reinterpret_cast<const float *>(s_at + COOP_AREC) + hf * 64, vmask);
  Act<PREC> xo[4];
  ln_to_act<PREC>(h, xo);
  bias_slot_one(xo, hf);
  ff16_rows(xo);   // unit n of tile c = GEMM1's B operand of N-tile n, K step c
#pragma unroll
  for (int c = 0; c < 4; ++c) s_xn[2 * c][lane] = __builtin_bit_cast(uint4, xo[c].f[0]), s_xn[2 * c + 1][lane] = __builtin_bit_cast(uint4, xo[c].f[1]);
  hs_store4(home, h);
}

// The step's noise for the tile's 32 points (n = this lane's) and the posterior table row -> s_z, ready for the step boundary: z[3][32] | row at float 128
template <int KIND>
__device__ __forceinline__ void coop_draw_noise(const KParams &p, float *s_z, int step, int t, int s, int n, int lane) {
  const int hf = lane >> 5, pj = lane & 31;
  float z[3];
  if (KIND != CHAIN_PLAIN && p.noise) {
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i] = p.noise[(((size_t)step * p.B + s) * 3 + i) * p.N + n];
  } else {
    philox_normal3(p.seed, ((unsigned long long)p.shape0 + (unsigned)s) * (unsigned)p.N + (unsigned)n, (unsigned)t, 0u, z);
  }
  if (hf == 0) s_z[pj] = z[0], s_z[32 + pj] = z[1], s_z[64 + pj] = z[2];
  if (lane < 8) s_z[128 + lane] = p.d.tab[(size_t)t * 8 + lane];
}

// GEMM1 of one chunk on one tile: (a, g) = W1 fragments R[cur .. cur + 15] (coop_load_w1's order: M-tiles 0, 1 of a, of g, per K step c) x xn3
__device__ __forceinline__ void coop_gemm1(v16f &a, v16f &g, const uint4 (&R)[32], int cur, const uint4 (*s_xn)[64], int lane) {
  a = zero16(), g = zero16();   // b1' rides on the constant-one K slot (bias_slot_one)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    Act<DFX_PREC_BF16> x;
    x.f[0] = __builtin_bit_cast(v8bf, s_xn[2 * c][lane]), x.f[1] = __builtin_bit_cast(v8bf, s_xn[2 * c + 1][lane]);
    mma16_w1(a, 0, R[cur + 4 * c + 0], x, c == 0);
    mma16_w1(g, 0, R[cur + 4 * c + 2], x, c == 0);
    mma16_w1(a, 1, R[cur + 4 * c + 1], x, c == 0);
    mma16_w1(g, 1, R[cur + 4 * c + 3], x, c == 0);
  }
}
// ... and its GELU: hid = a gelu(g) -> the chunk's two uint4 rows of the GELU output
__device__ __forceinline__ void coop_gelu_store(const v16f &a, const v16f &g, uint4 (*hid_u)[64], int lane) {
  h2 aa[8], gg[8];
  HidAct hid;
  gelu16_f16_cvt(a, g, aa, gg);
  gelu16_f16_math(aa, gg, hid);
  hid_u[0][lane] = hid.f[0], hid_u[1][lane] = hid.f[1];
}

// Step boundary of one tile, on the wave that runs its phase A: eps from the last block's h ...
__device__ __forceinline__ void coop_eps(float (&eps)[3], const v4f *home, const unsigned char *cc, const KParams &p, int lane) {
  v16f h[4];
  hs_load4(h, home);
  post_eps_tiles(h, reinterpret_cast<const float *>(cc + CC_WOUT) + (lane >> 5) * 32 * PAIR_WOUT, p.d.bout, eps);
}
// ... the posterior update of the chain state parked at ps_lds, with the noise coop_draw_noise left in s_z (true: the kernel is done) ...
template <int KIND>
__device__ __forceinline__ bool coop_posterior(const KParams &p, PointState &ps, const float (&eps)[3], const float *ps_lds, const float *s_z, int s, int n,
                                               int step, int t, int pj) {
  ps.s = s, ps.n = n, ps.gid = 0;   // (gid: the noise was drawn by another wave)
  pstate_load(ps_lds, pj, 32, ps, true);
  const float zr[3] = {s_z[pj], s_z[32 + pj], s_z[64 + pj]};
  const bool zok = KIND == CHAIN_PLAIN || p.mode != MODE_EPS;
  return step_epilogue<KIND>(p, ps, eps, step, t, zok ? zr : nullptr, zok ? s_z + 128 : nullptr);
}
// ... and proj_in + pre_norm of the new state -> h's home (also before the first step)
__device__ __forceinline__ void coop_enter_step(const PointState &ps, v4f *home, const unsigned char *cc, int lane) {
  const int hf = lane >> 5;
  v16f h[4];
  proj_in_prenorm_tiles(h, ps.x, reinterpret_cast<const float *>(cc + CC_CPART) + ps.sg * INNER + hf * 64, reinterpret_cast<const float *>(cc + CC_WINX) + hf * 32 * PAIR_WIN,
                        reinterpret_cast<const float *>(cc + CC_PREGB) + hf * 32 * PAIR_PREGB);
  hs_store4(home, h);
}

// ---- k_denoise_coop: eight wavefronts on ONE 32-point tile
constexpr int COOP_W2_FIRST = 8;                                  // first W2 chunk staged in LDS (the LDS budget holds eight; chunks 0..7: one coop_load_w2)
constexpr int CL_XN = 0;                                          // 8 x 64 uint4: LN3 output as the B operand of GEMM1
constexpr int CL_HID = CL_XN + 8 * 1024;                          // [16][2][64] uint4: GELU output of every chunk
constexpr int CL_BC = CL_HID + FF_CHUNKS * 2048;                  // 2 x block constants (b1', b2), by block parity
constexpr int CL_AT = CL_BC + 2 * BCONST_BYTES;                   // attention record (17 KiB) + c_t row (1 KiB)
constexpr int CL_HS = CL_AT + asms_bytes(DFX_PREC_BF16) + 1024;   // home of the residual stream h: 4 tiles x 4 KiB, [tile][q][lane] float4
constexpr int CL_CONST = CL_HS + 16 * 1024;                       // chain-invariant operands (CC_*)
constexpr int CL_W2 = CL_CONST + CC_BYTES;                        // W2 tiles of chunks 8..15 (8 KiB each)
constexpr int CL_Z = CL_W2 + (FF_CHUNKS - COOP_W2_FIRST) * 8192;   // this step's noise z[3][32] (384 B) | posterior table row (32 B at +512)
constexpr int CL_PS = CL_Z + 1024;                                 // per-point chain state (x, anchor, variance, L, part id: 13 x 32 floats), home between step boundaries
constexpr int CL_TOTAL = CL_PS + 2048;
static_assert(CL_TOTAL <= 160 * 1024, "LDS budget of the co-operative kernel");

template <int KIND>
__global__ void __launch_bounds__(COOP_NW * 64, 2) k_denoise_coop(const KParams p) {
  constexpr int TSTRIDE = COOP_TSTRIDE, AREC = COOP_AREC;
  uint4 (*s_xn)[64] = reinterpret_cast<uint4 (*)[64]>(pipe_smem + CL_XN);
  uint4 (*s_hid)[2][64] = reinterpret_cast<uint4 (*)[2][64]>(pipe_smem + CL_HID);
  uint4 *s_at = reinterpret_cast<uint4 *>(pipe_smem + CL_AT);
  unsigned char *cc = pipe_smem + CL_CONST;
  float *s_z = reinterpret_cast<float *>(pipe_smem + CL_Z);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hf = lane >> 5, pj = lane & 31;
  const long long g0 = (long long)blockIdx.x * 32;
  const int s = __builtin_amdgcn_readfirstlane((int)(g0 / p.N));
  const int n = (int)(g0 - (long long)s * p.N) + pj;
  const int depth = p.d.depth;
  const bool w0 = wave == 0, tile_owner = wave < COOP_TILES;
  float *ps_lds = reinterpret_cast<float *>(pipe_smem + CL_PS);
  v4f *home = reinterpret_cast<v4f *>(pipe_smem + CL_HS) + lane;
  unsigned vmask = 0;
  if (w0) coop_point_init<KIND>(p, ps_lds, s, n, pj, vmask);
  const uint4 *asms_s = p.as_ms + (size_t)s * depth * AREC;
  coop_stage_consts(cc, p, s);   // (wave 0 reads them at every step boundary)
  __syncthreads();
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)pipe_smem);
  const unsigned voff = lane * 16;

  // One register file for every role (one kernel = one register allocation):
  //   R[32]   phase H: GEMM1 fragments of round 0 (R[0..15]) / round 1 (R[16..31]), in the accumulation order a(c,0) a(c,1) g(c,0)
  //           g(c,1), c = 0..3;   phase G (tile owners): W2 fragments of chunks 0..7 of the own tile, R[2 u + q]
  //   h[4]    wave 0, phase A only;   ht   tile owners, phase G only — in between h lives in LDS
  uint4 R[32];

#ifdef DFX_TRACE   // phase stamps of wave 0 (row 0 of the trace buffer) and of wave 5 (row 1) of workgroup 0
  Tracer tr{(p.trace != nullptr && blockIdx.x == 0 && (wave == 0 || wave == 5)) ? p.trace + (size_t)(wave ? 1 : 0) * p.trace_cap : nullptr, p.trace_cap, 0};
#else
  Tracer tr;
#endif
  if (w0) {
    PointState ps;
    pstate_load(ps_lds, pj, 32, ps, false);
    coop_enter_step(ps, home, cc, lane);
  }
  int seq = 0;
  for (int step = 0; step < p.nsteps; ++step) {
    const int t = step_t<KIND>(p, step, s);
    for (int b = 0; b < depth; ++b, ++seq) {
      const BlockPack bp = block_pack(p, b);
      float *s_bc = reinterpret_cast<float *>(pipe_smem + CL_BC + (seq & 1) * BCONST_BYTES);
      // ---- top of the block: operands of phase A -> LDS (waves 4..7, which left phase G's barrier first), round-0 fragments requested
      if (!tile_owner) {
        coop_stage_block<COOP_NW - COOP_TILES>(bp, asms_s + (size_t)b * AREC, t, wave - COOP_TILES, voff, lds0 + CL_AT, lds0 + CL_BC + (seq & 1) * BCONST_BYTES);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      coop_load_w1(R, 0, bp.chunks, wave, lane);   // round 0: in flight through phase A
      tr.stamp(10);
      __syncthreads();   // 0: attention record, c_t, block constants of this block are in LDS; h's home holds the previous block's result
      tr.stamp(11);
      if (!w0) {         // ---- phase A for the idle waves: W2 tiles of chunks 8..15 -> LDS
        constexpr int NP = (FF_CHUNKS - COOP_W2_FIRST) * 8, NH = COOP_NW - 1;   // 64 pieces over 7 waves
#pragma unroll
        for (int i = 0; i < (NP + NH - 1) / NH; ++i) {
          const int k = i * NH + wave - 1;
          if (k < NP)
            dma1k_pinned(reinterpret_cast<const char *>(bp.chunks + (size_t)(COOP_W2_FIRST + (k >> 3) + FF_SKEW) * CHUNK_TILES * TSTRIDE + 8 * TSTRIDE) + (k & 7) * 1024,
                         voff, lds0 + CL_W2 + k * 1024);
        }
        // the step's noise and posterior coefficients, ready for wave 0's epilogue
        if (wave == COOP_NW - 1 && b == depth - 1 && (KIND == CHAIN_PLAIN || p.mode != MODE_EPS)) coop_draw_noise<KIND>(p, s_z, step, t, s, n, lane);
      } else {           // ---- phase A: wave 0
        coop_phase_a(home, s_at, s_xn, lane, vmask);
      }
      tr.stamp(12);
      __syncthreads();   // 1: xn3 of this block and h are in LDS
      tr.stamp(13);
      // ---- phase H: every wave, chunks `wave` and `wave + 8`
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int u = r * COOP_NW + wave, cur = r * 16;
        if (r == 0) coop_load_w1(R, 16, bp.chunks, u + COOP_NW, lane);
        else if (tile_owner) coop_load_w2(R, 0, bp.chunks, wave, lane);   // round 0's registers are free: the own tile's W2 fragments of chunks 0..7
        v16f a, g;
        coop_gemm1(a, g, R, cur, s_xn, lane);
        coop_gelu_store(a, g, s_hid[u], lane);
      }
      if (!w0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's W2 pieces have landed (long ago: loads complete in order)
      tr.stamp(14);
      __syncthreads();   // 2: hid of all chunks and the W2 copies are in LDS
      tr.stamp(15);
      // ---- phase G: wave t accumulates tile t of h, chunk after chunk (the accumulation order of the pipelined kernel), + b2
      if (tile_owner) {
        v16f ht;
        hs_load(ht, home + wave * 256);
        ff16_rows(ht);   // quads = the accumulators of the tile's two M-tiles x two N-tiles; back before the store
        // hid / LDS-resident W2 fragments: a ring three chunks deep (one chunk = two dependent MFMAs = less than one LDS round trip),
        // fenced per chunk — left alone hipcc sinks every read next to its MFMA and the chain runs at LDS latency
        uint4 hq[4][2], wq[4][2];
        unsigned hoff = CL_HID + lane * 16, woff = CL_W2 + (wave * TSTRIDE + lane) * 16;
        asm volatile("" : "+v"(hoff), "+v"(woff));   // one base register each, chunk offsets as immediates
        const uint4 *hidb = reinterpret_cast<const uint4 *>(pipe_smem + hoff), *w2b = reinterpret_cast<const uint4 *>(pipe_smem + woff);
        auto fetch = [&](int u) {
          hq[u & 3][0] = hidb[u * 128], hq[u & 3][1] = hidb[u * 128 + 64];
          if (u >= COOP_W2_FIRST) wq[u & 3][0] = w2b[(u - COOP_W2_FIRST) * 4 * TSTRIDE], wq[u & 3][1] = w2b[(u - COOP_W2_FIRST) * 4 * TSTRIDE + 64];
        };
        fetch(0), fetch(1), fetch(2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < FF_CHUNKS; ++u) {
          if (u + 3 < FF_CHUNKS) fetch(u + 3);
          const uint4 f0 = u < COOP_W2_FIRST ? R[2 * u] : wq[u & 3][0], f1 = u < COOP_W2_FIRST ? R[2 * u + 1] : wq[u & 3][1];
          mma16_w2(ht, 0, f0, hq[u & 3][0], hq[u & 3][1]);
          mma16_w2(ht, 1, f1, hq[u & 3][0], hq[u & 3][1]);
          __builtin_amdgcn_sched_barrier(0);
        }
        ff16_rows(ht);
        hs_store_plus(home + wave * 256, ht, s_bc + BCONST_B2_OFF + hf * 64 + wave * 16);
      }
    }
    tr.stamp(16);
    __syncthreads();   // the last block's tiles are in h's home
    tr.stamp(17);
    if (w0) {
      float eps[3];
      coop_eps(eps, home, cc, p, lane);
      tr.stamp(18);
      PointState ps;
      if (coop_posterior<KIND>(p, ps, eps, ps_lds, s_z, s, n, step, t, pj)) break;   // (the other waves leave through the loop bound: nsteps = 1 in these modes)
      tr.stamp(19);
      pstate_store(ps_lds, pj, 32, ps, false);
      if (step + 1 < p.nsteps) coop_enter_step(ps, home, cc, lane);
      tr.stamp(20);
    }
  }
}

// ---- k_denoise_coop2: the co-operative kernel with TWO 32-point tiles per workgroup (round 4; batches of 5 .. 8 shapes at N = 2048, i.e. one to two
// tiles per CU, where k_denoise_coop needs two rounds of workgroups and k_denoise_pipe<2> leaves half of every CU idle).  Same phases, same device
// functions, same MFMA order per accumulator as k_denoise_coop — bit-identical results — with the work of a block cut this way:
//   phase A   waves 0 and 1 (different SIMDs): attention + LayerNorms on tile 0 / tile 1, side by side
//   phase H   all 8 waves, chunks w and w + 8: every GEMM1 fragment (registers) feeds BOTH tiles' MFMAs; two GELUs per chunk
//   phase G   waves 0..3 own the four output tiles of tile 0, waves 4..7 those of tile 1 — the eight waves carry all of W2 for their output tile in
//             the 32 fragment registers phase H has freed (chunks 0..7 requested behind round 0, chunks 8..15 behind round 1's MFMAs: the second
//             tile's GELU covers their latency), so k_denoise_coop's 64 KiB LDS copy of W2 is gone and the second tile's h home, xn3 and GELU
//             outputs take its place (153 KiB)
// The next block's attention record, c_t row and block constants are requested behind barrier 2 (the record is only read in phase A) by all waves,
// four chunks into phase G: the address arithmetic of the pieces needs registers, and right behind the barrier all 32 fragment registers are live.
constexpr int C2_XN = 0;                                           // 2 tiles x 8 x 64 uint4
constexpr int C2_HID = C2_XN + 2 * 8 * 1024;                       // 2 tiles x [16][2][64] uint4
constexpr int C2_BC = C2_HID + 2 * FF_CHUNKS * 2048;               // 2 x block constants, by block parity
constexpr int C2_AT = C2_BC + 2 * BCONST_BYTES;                    // attention record + c_t row (one shape per workgroup)
constexpr int C2_HS = C2_AT + asms_bytes(DFX_PREC_BF16) + 1024;    // 2 tiles x 16 KiB: h's home
constexpr int C2_CONST = C2_HS + 2 * 16 * 1024;                    // chain-invariant operands (CC_*)
constexpr int C2_Z = C2_CONST + CC_BYTES;                          // 2 tiles x (noise z[3][32] | posterior table row at +512)
constexpr int C2_PS = C2_Z + 2 * 1024;                             // 2 tiles x per-point chain state
constexpr int C2_TOTAL = C2_PS + 2 * 2048;
static_assert(C2_TOTAL <= 160 * 1024, "LDS budget of the two-tile co-operative kernel");

template <int KIND>
__global__ void __launch_bounds__(COOP_NW * 64, 2) k_denoise_coop2(const KParams p) {
  constexpr int AREC = COOP_AREC;
  uint4 *s_at = reinterpret_cast<uint4 *>(pipe_smem + C2_AT);
  unsigned char *cc = pipe_smem + C2_CONST;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hf = lane >> 5, pj = lane & 31;
  const long long g0 = (long long)blockIdx.x * 64;
  const int s = __builtin_amdgcn_readfirstlane((int)(g0 / p.N));        // both tiles belong to shape s (N % 64 == 0: launch())
  const int nbase = (int)(g0 - (long long)s * p.N);
  const int depth = p.d.depth;
  const bool arole = wave < 2;                 // phase A / step boundary: wave w works on tile w
  const int gt = wave >> 2, ct = wave & 3;     // phase G: output tile ct of tile gt
  auto xn_base = [&](int t) { return reinterpret_cast<uint4 (*)[64]>(pipe_smem + C2_XN + t * 8 * 1024); };
  auto hid_base = [&](int t) { return reinterpret_cast<uint4 (*)[2][64]>(pipe_smem + C2_HID + t * FF_CHUNKS * 2048); };
  auto home = [&](int t) { return reinterpret_cast<v4f *>(pipe_smem + C2_HS + t * 16 * 1024) + lane; };
  auto z_base = [&](int t) { return reinterpret_cast<float *>(pipe_smem + C2_Z + t * 1024); };
  float *ps_lds = reinterpret_cast<float *>(pipe_smem + C2_PS + (wave & 1) * 2048);   // (waves 0, 1)
  const int n_a = nbase + wave * 32 + pj;                                             // (waves 0, 1: this lane's point)
  unsigned vmask = 0;
  if (arole) coop_point_init<KIND>(p, ps_lds, s, n_a, pj, vmask);
  const uint4 *asms_s = p.as_ms + (size_t)s * depth * AREC;
  coop_stage_consts(cc, p, s);
  __syncthreads();
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)pipe_smem);
  const unsigned voff = lane * 16;

  uint4 R[32];   // phase H: GEMM1 fragments of round 0 (R[0..15]) / round 1 (R[16..31]); phase G: W2 fragments of the own output tile, chunk u in R[2 u], R[2 u + 1]
  // attention record, c_t row and block constants of block b at time t -> LDS: 23 pieces over the 8 waves
  auto stage_block = [&](int b, int t, int parity) {
    coop_stage_block<COOP_NW>(block_pack(p, b), asms_s + (size_t)b * AREC, t, wave, voff, lds0 + C2_AT, lds0 + C2_BC + parity * BCONST_BYTES);
  };
  if (arole) {
    PointState ps;
    pstate_load(ps_lds, pj, 32, ps, false);
    coop_enter_step(ps, home(wave), cc, lane);
  }
  int seq = 0;
  if (p.nsteps > 0) stage_block(0, step_t<KIND>(p, 0, s), 0);
  for (int step = 0; step < p.nsteps; ++step) {
    const int t = step_t<KIND>(p, step, s);
    for (int b = 0; b < depth; ++b, ++seq) {
      const BlockPack bp = block_pack(p, b);
      float *s_bc = reinterpret_cast<float *>(pipe_smem + C2_BC + (seq & 1) * BCONST_BYTES);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the block's operands (requested a phase G ago)
      coop_load_w1(R, 0, bp.chunks, wave, lane);   // round 0: in flight through phase A
      __syncthreads();   // 0: attention record, c_t, block constants of this block are in LDS; h's homes hold the previous block's result
      if (arole) {       // ---- phase A: wave w on tile w
        coop_phase_a(home(wave), s_at, xn_base(wave), lane, vmask);
      } else if (wave >= COOP_NW - 2 && b == depth - 1 && (KIND == CHAIN_PLAIN || p.mode != MODE_EPS)) {   // the step's noise and posterior coefficients: wave 6 for tile 0, wave 7 for tile 1
        const int tz = wave - (COOP_NW - 2);
        coop_draw_noise<KIND>(p, z_base(tz), step, t, s, nbase + tz * 32 + pj, lane);
      }
      __syncthreads();   // 1: xn3 of both tiles and h are in LDS
      // ---- phase H: every wave, chunks `wave` and `wave + 8`, both tiles per fragment set
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int u = r * COOP_NW + wave, cur = r * 16;
        if (r == 0) coop_load_w1(R, 16, bp.chunks, u + COOP_NW, lane);
        else coop_load_w2(R, 0, bp.chunks, ct, lane);   // round 0's registers are free: W2 of chunks 0..7
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
          v16f a, g;
          coop_gemm1(a, g, R, cur, xn_base(tl), lane);
          if (r == 1 && tl == 1) {   // round 1's fragments are done with: W2 of chunks 8..15 travels under the last GELU
            __builtin_amdgcn_sched_barrier(0);
            coop_load_w2(R, 8, bp.chunks, ct, lane);
            __builtin_amdgcn_sched_barrier(0);
          }
          coop_gelu_store(a, g, hid_base(tl)[u], lane);
        }
      }
      __syncthreads();   // 2: hid of all chunks of both tiles is in LDS; nobody reads the attention record any more
      // the next block's operands (next step's c_t row behind the last block)
      auto stage_next = [&] {
        if (b + 1 < depth) stage_block(b + 1, t, (seq + 1) & 1);
        else if (step + 1 < p.nsteps) stage_block(0, step_t<KIND>(p, step + 1, s), (seq + 1) & 1);
      };
      // ---- phase G: wave (gt, ct) accumulates output tile ct of tile gt, chunk after chunk (the accumulation order of the pipelined kernel), + b2
      {
        v16f ht;
        hs_load(ht, home(gt) + ct * 256);
        ff16_rows(ht);
        uint4 hq[4][2];   // hid fragments: a ring three chunks deep, fenced per chunk (see k_denoise_coop)
        unsigned hoff = C2_HID + gt * FF_CHUNKS * 2048 + lane * 16;
        asm volatile("" : "+v"(hoff));
        const uint4 *hidb = reinterpret_cast<const uint4 *>(pipe_smem + hoff);
        auto fetch = [&](int u) { hq[u & 3][0] = hidb[u * 128], hq[u & 3][1] = hidb[u * 128 + 64]; };
        fetch(0), fetch(1), fetch(2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < FF_CHUNKS; ++u) {
          if (u + 3 < FF_CHUNKS) fetch(u + 3);
          mma16_w2(ht, 0, R[2 * u], hq[u & 3][0], hq[u & 3][1]);
          mma16_w2(ht, 1, R[2 * u + 1], hq[u & 3][0], hq[u & 3][1]);
          __builtin_amdgcn_sched_barrier(0);
          if (u == 3) {   // (here and not at the barrier: the address arithmetic of the pieces needs registers, and the first chunks' fragments have just freed some)
            stage_next();
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        ff16_rows(ht);
        hs_store_plus(home(gt) + ct * 256, ht, s_bc + BCONST_B2_OFF + hf * 64 + ct * 16);
      }
    }
    __syncthreads();   // the last block's tiles are in h's homes
    if (arole) {
      float eps[3];
      coop_eps(eps, home(wave), cc, p, lane);
      PointState ps;
      if (coop_posterior<KIND>(p, ps, eps, ps_lds, z_base(wave), s, n_a, step, t, pj)) break;   // (the other waves leave through the loop bound: nsteps = 1 in these modes)
      pstate_store(ps_lds, pj, 32, ps, false);
      if (step + 1 < p.nsteps) coop_enter_step(ps, home(wave), cc, lane);
    }
  }
}

// q_sample (anchored_diffusion.py:148-173): x_t = sqrt_acp[t] (x0 - a) + a + sqrt_1m_acp[t] L noise, per-shape t,
// anchors / variances of the point's part from the shape context (learn_anchor, learn_variance)
__global__ void k_q_sample(const float *__restrict__ part, const float *__restrict__ qtab, const int32_t *__restrict__ seg,
                           const int32_t *__restrict__ t, const float *__restrict__ x0, const float *__restrict__ noise,
                           float *__restrict__ out, int N, int T, long long total) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int n = i % N, c = (i / N) % 3;
  const long long b = i / ((long long)3 * N);
  const int sg = seg[b * N + n];
  int tt = t[b];
  tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
  const float a = part[b * 32 + c * 4 + sg], L = sqrtf(part[b * 32 + 12 + c * 4 + sg]);
  out[i] = qtab[tt * 2] * (x0[i] - a) + a + qtab[tt * 2 + 1] * L * noise[i];
}

// ((target - pred)^2 * flags).mean(1).sum() / flags.sum()  (anchored_diffusion.py:840-847); float64 accumulation
__global__ void k_masked_mse(const float *__restrict__ target, const float *__restrict__ pred, const float *__restrict__ flags,
                             double *__restrict__ acc, int N, long long total) {
  double s = 0.0, f = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / N;
    const int n = i % N;
    float m = 0.f;
    const float fl = flags ? flags[i] : 1.f;
    for (int c = 0; c < 3; ++c) {
      const float dlt = target[(b * 3 + c) * N + n] - pred[(b * 3 + c) * N + n];
      m += dlt * dlt * fl;
    }
    s += (double)(flags ? m / 3.0f : m);
    f += (double)fl;
  }
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o), f += __shfl_xor(f, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(acc, s), atomicAdd(acc + 1, f);
}
__global__ void k_mse_finish(const double *acc, float *loss, int has_flags, double count) {
  *loss = (float)(has_flags ? acc[0] / acc[1] : acc[0] / count);
}

bool g_force_direct = false;
int g_force_nw = 0;       // debug: code of dfx_debug_pipe_waves (denoiser_plan.h: force_from_code)
int g_num_cus = 256;      // the MI355X's; never read from the device
unsigned long long *g_trace = nullptr;
int g_trace_cap = 0;

// The kernels in the order of denoiser_plan.h's Variant, with their dynamic LDS bytes
struct VariantKernel {
  void (*kernel)(KParams);
  int lds;
};
const VariantKernel KERNELS[NUM_VARIANTS] = {
    {k_denoise_pipe<8>, PipeCfg<8>::L_TOTAL},     {k_denoise_pipe<4>, PipeCfg<4>::L_TOTAL},     {k_denoise_pipe<2>, PipeCfg<2>::L_TOTAL},
    {k_denoise_coop<CHAIN_GENERAL>, CL_TOTAL},    {k_denoise_coop2<CHAIN_GENERAL>, C2_TOTAL},   {k_denoise_pipe_f32<8>, PipeCfg<8>::L_TOTAL},
    {k_denoise_pipe_f32<4>, PipeCfg<4>::L_TOTAL}, {k_denoise_pipe_f32<2>, PipeCfg<2>::L_TOTAL}, {k_denoise<DFX_PREC_BF16, 4>, 0},
    {k_denoise<DFX_PREC_F32, 4>, 0},
};
// ... and their instantiations for partial chains (KParams::start != START_NOISE): the same plan, the same launch shape
const VariantKernel KERNELS_FROM[NUM_VARIANTS] = {
    {k_denoise_pipe<8, CHAIN_FROM>, PipeCfg<8>::L_TOTAL}, {k_denoise_pipe<4, CHAIN_FROM>, PipeCfg<4>::L_TOTAL}, {k_denoise_pipe<2, CHAIN_FROM>, PipeCfg<2>::L_TOTAL},
    {k_denoise_coop<CHAIN_FROM>, CL_TOTAL},             {k_denoise_coop2<CHAIN_FROM>, C2_TOTAL},            {k_denoise_pipe_f32<8, true>, PipeCfg<8>::L_TOTAL},
    {k_denoise_pipe_f32<4, true>, PipeCfg<4>::L_TOTAL}, {k_denoise_pipe_f32<2, true>, PipeCfg<2>::L_TOTAL}, {k_denoise<DFX_PREC_BF16, 4, true>, 0},
    {k_denoise<DFX_PREC_F32, 4, true>, 0},
};
// ... and the plain-generation instantiations of the five bf16 chain kernels (ChainKind): the same plan, the same launch shape, the same name in
// dfx_last_kernel_variant.  The other variants have none (nullptr): a plain launch that the planner gives to one of them takes its GENERAL form.
const VariantKernel KERNELS_PLAIN[NUM_VARIANTS] = {
    {k_denoise_pipe<8, CHAIN_PLAIN>, PipeCfg<8>::L_TOTAL}, {k_denoise_pipe<4, CHAIN_PLAIN>, PipeCfg<4>::L_TOTAL}, {k_denoise_pipe<2, CHAIN_PLAIN>, PipeCfg<2>::L_TOTAL},
    {k_denoise_coop<CHAIN_PLAIN>, CL_TOTAL},               {k_denoise_coop2<CHAIN_PLAIN>, C2_TOTAL},              {nullptr, 0},
    {nullptr, 0},                                          {nullptr, 0},                                          {nullptr, 0},
    {nullptr, 0},
};
static_assert((int)Variant::Pipe8 == 0 && (int)Variant::Pipe4 == 1 && (int)Variant::Pipe2 == 2 && (int)Variant::Coop == 3 && (int)Variant::Coop2 == 4,
              "KERNELS_PLAIN's rows against denoiser_plan.h's Variant");
bool g_force_general = false;          // debug: dfx_debug_chain_general
const char *g_last_chain_kind = "";    // "general" | "from" | "plain": the instantiation the last launch() took (dfx_debug_last_chain_kind)

// Plain generation: everything that the PLAIN instantiations fix at compile time (ChainKind).  dfx_sample_chain without explicit noise and without
// snapshots is such a launch — bench.py's timed call, AnchorDiffAE.decode when it asks for no trajectory.
bool plain_launch(const KParams &p) {
  return p.mode == MODE_CHAIN && p.start == START_NOISE && p.ddim_n == 0 && !p.t_shape && !p.noise && !p.xT_noise && !p.xstart && !p.traj && !p.x_in && !p.hold &&
         p.nsteps == p.d.T && p.t0 == p.d.T - 1;
}

static_assert(info(Variant::Coop).threads == COOP_NW * 64 && info(Variant::Coop2).threads == COOP_NW * 64 && info(Variant::Pipe8).points == PipeCfg<8>::PTS,
              "denoiser_plan.h's table against the kernels' launch bounds");

int launch(const dfx_denoiser *d, const void *shape_ctx, KParams &p, hipStream_t st) {
  ShapeCtxView v;
  shape_ctx_view(&v, const_cast<void *>(shape_ctx), p.B, d->dev.depth, d->dev.prec);
  p.d = d->dev;
  p.part = v.part;
  p.cpart = v.cpart;
  p.as_ms = v.as_ms;
  p.trace = g_trace;
  p.trace_cap = g_trace_cap;
  // (the size check stays here, on the direct kernels' workgroup count as before; the planner itself takes any B, N)
  if (((long long)p.B * p.N / 32 + 3) / 4 > 0x7fffffffLL) return set_error(DFX_ERR_INVALID_ARG, "denoiser: B*N too large");
  const Plan plan = plan_launch({d->dev.prec, d->dev.w1_fold != 0, g_force_direct, force_from_code(g_force_nw), p.B, p.N, g_num_cus});
  const bool plain = !g_force_general && plain_launch(p) && KERNELS_PLAIN[(int)plan.v].kernel != nullptr;
  const VariantKernel &k = (plain ? KERNELS_PLAIN : p.start != START_NOISE ? KERNELS_FROM : KERNELS)[(int)plan.v];
  if (k.lds > 0) {
    static PerDeviceOnce attrs;
    DFX_HIP_TRY(attrs.run([] {
      hipError_t e = hipSuccess;
      for (const VariantKernel &vk : KERNELS)
        if (e == hipSuccess && vk.lds > 0) e = set_max_lds(reinterpret_cast<const void *>(vk.kernel), vk.lds);
      for (const VariantKernel &vk : KERNELS_FROM)
        if (e == hipSuccess && vk.lds > 0) e = set_max_lds(reinterpret_cast<const void *>(vk.kernel), vk.lds);
      for (const VariantKernel &vk : KERNELS_PLAIN)
        if (e == hipSuccess && vk.lds > 0) e = set_max_lds(reinterpret_cast<const void *>(vk.kernel), vk.lds);
      return e;
    }));
  }
  EventTimer tm;
  tm.begin(st);
  hipLaunchKernelGGL(k.kernel, dim3((unsigned)plan.grid), dim3(info(plan.v).threads), k.lds, st, p);
  g_last_variant = info(plan.v).name;
  g_last_chain_kind = plain ? "plain" : p.start != START_NOISE ? "from" : "general";
  const int rc = check_launch("denoiser kernel");
  tm.end();
  return rc;
}

int check_common(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, int B, int N, const char *who) {
  DFX_REQUIRE(d, "%s: null denoiser", who);
  DFX_REQUIRE(B >= 0 && N >= 0, "%s: negative size", who);
  DFX_REQUIRE(N % 32 == 0, "%s: N=%d must be a multiple of 32 (one wavefront = 32 points of one shape)", who, N);
  if ((long long)B * N == 0) return 1;
  DFX_REQUIRE(shape_ctx && seg, "%s: null pointer", who);
  return DFX_OK;
}

}  // namespace

extern "C" {

int dfx_denoise_eps(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, int t,
                    float *eps, int B, int N, dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "denoise_eps");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(x && eps, "denoise_eps: null pointer");
  DFX_REQUIRE(t >= 0 && t < d->dev.T, "denoise_eps: t=%d outside [0,%d)", t, d->dev.T);
  KParams p{};
  p.x_in = x; p.seg = seg; p.out = eps;
  p.B = B; p.N = N; p.t0 = t; p.nsteps = 1; p.ret_interval = 1; p.mode = MODE_EPS;
  return launch(d, shape_ctx, p, as_stream(stream));
}

int dfx_p_sample(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, int t,
                 const float *noise, uint64_t seed, uint64_t shape_offset, float *x_prev, float *pred_xstart, int B, int N,
                 dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "p_sample");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(x && x_prev, "p_sample: null pointer");
  DFX_REQUIRE(t >= 0 && t < d->dev.T, "p_sample: t=%d outside [0,%d)", t, d->dev.T);
  KParams p{};
  p.x_in = x; p.seg = seg; p.noise = noise; p.out = x_prev; p.xstart = pred_xstart; p.seed = seed; p.shape0 = shape_offset;
  p.B = B; p.N = N; p.t0 = t; p.nsteps = 1; p.ret_interval = 1; p.mode = MODE_PSAMPLE;
  return launch(d, shape_ctx, p, as_stream(stream));
}

// DDIM coefficient list of a launch: steps are given ASCENDING like the reference's `self.steps` (:117-122) and
// executed in reverse (:566); xt_dir_coeff in float64 like numpy (:116), cast to fp32 at use (extract_into_tensor).
static int fill_ddim(const dfx_denoiser *d, KParams &p, const int32_t *steps, int n_steps, float eta, const char *who) {
  DFX_REQUIRE(steps && n_steps >= 1 && n_steps <= DDIM_MAX_STEPS, "%s: 1..%d DDIM steps", who, DDIM_MAX_STEPS);
  const int T = d->dev.T;
  p.ddim_n = n_steps;
  p.ddim_eta = eta;
  for (int i = 0; i < n_steps; ++i) {
    const int t = steps[n_steps - 1 - i];
    DFX_REQUIRE(t >= 0 && t < T, "%s: step %d outside [0,%d)", who, t, T);
    p.ddim_t[i] = t;
    p.ddim_xdc[i] = (float)std::sqrt(1.0 - d->host_ac_pv[t] - (double)eta * (double)eta * d->host_ac_pv[(size_t)T + t]);
  }
  return DFX_OK;
}

int dfx_p_sample_ddim(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, int t, float eta,
                      const float *noise, uint64_t seed, uint64_t shape_offset, float *x_prev, float *pred_xstart, int B, int N,
                      dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "p_sample_ddim");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(x && x_prev, "p_sample_ddim: null pointer");
  KParams p{};
  const int32_t one[1] = {t};
  if (int e = fill_ddim(d, p, one, 1, eta, "p_sample_ddim")) return e;
  p.x_in = x; p.seg = seg; p.noise = noise; p.out = x_prev; p.xstart = pred_xstart; p.seed = seed; p.shape0 = shape_offset;
  p.B = B; p.N = N; p.t0 = t; p.nsteps = 1; p.ret_interval = 1; p.mode = MODE_PSAMPLE;
  return launch(d, shape_ctx, p, as_stream(stream));
}

int dfx_sample_chain_ddim(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const int32_t *steps,
                          int n_steps, float eta, const float *x_T_noise, const float *step_noise, uint64_t seed,
                          uint64_t shape_offset, int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "sample_chain_ddim");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(pred, "sample_chain_ddim: null pred");
  DFX_REQUIRE(!traj || ret_interval >= 1, "sample_chain_ddim: ret_interval must be >= 1 when traj is given");
  KParams p{};
  if (int e = fill_ddim(d, p, steps, n_steps, eta, "sample_chain_ddim")) return e;
  DFX_REQUIRE(steps[0] == 0, "sample_chain_ddim: the step list must start at 0 (decode keeps the t == 0 sample as 'pred')");
  p.seg = seg; p.noise = step_noise; p.xT_noise = x_T_noise; p.out = pred; p.traj = traj; p.seed = seed; p.shape0 = shape_offset;
  p.B = B; p.N = N; p.t0 = p.ddim_t[0]; p.nsteps = n_steps; p.ret_interval = ret_interval >= 1 ? ret_interval : 1;
  p.mode = MODE_CHAIN;
  return launch(d, shape_ctx, p, as_stream(stream));
}

int dfx_denoise_eps_t(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, const int32_t *t,
                      float *eps, int B, int N, dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "denoise_eps_t");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(x && eps && t, "denoise_eps_t: null pointer");
  KParams p{};
  p.x_in = x; p.seg = seg; p.out = eps; p.t_shape = t;
  p.B = B; p.N = N; p.t0 = 0; p.nsteps = 1; p.ret_interval = 1; p.mode = MODE_EPS;
  return launch(d, shape_ctx, p, as_stream(stream));
}

int dfx_q_sample_f32(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const int32_t *t, const float *x_start,
                     const float *noise, float *x_t, int B, int N, dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "q_sample");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(t && x_start && noise && x_t, "q_sample: null pointer");
  ShapeCtxView v;
  shape_ctx_view(&v, const_cast<void *>(shape_ctx), B, d->dev.depth, d->dev.prec);
  const long long total = (long long)B * 3 * N;
  k_q_sample<<<(int)((total + 255) / 256), 256, 0, as_stream(stream)>>>(v.part, d->dev.qtab, seg, t, x_start, noise, x_t, N, d->dev.T, total);
  return check_launch("q_sample");
}

int dfx_masked_mse_f32(const float *target, const float *pred, const float *flags, double *workspace2, float *loss, int B,
                       int N, dfx_stream_t stream) {
  DFX_REQUIRE(B >= 1 && N >= 1 && target && pred && workspace2 && loss, "masked_mse: bad argument");
  hipStream_t st = as_stream(stream);
  DFX_HIP_TRY(hipMemsetAsync(workspace2, 0, 2 * sizeof(double), st));
  const long long total = (long long)B * N;
  long long blocks = (total + 255) / 256;
  if (blocks > 64) blocks = 64;   // every wavefront ends with two float64 atomics on the same two addresses: 256 of them, not 16384 (100 us of serialised L2 atomics)
  k_masked_mse<<<(int)blocks, 256, 0, st>>>(target, pred, flags, workspace2, N, total);
  k_mse_finish<<<1, 1, 0, st>>>(workspace2, loss, flags != nullptr, (double)B * 3.0 * N);
  return check_launch("masked_mse");
}

void dfx_debug_force_direct(int on) { g_force_direct = on != 0; }
void dfx_debug_pipe_waves(int nw) { g_force_nw = nw; }
void dfx_debug_chain_general(int on) { g_force_general = on != 0; }
const char *dfx_debug_last_chain_kind(void) { return g_last_chain_kind; }
const char *dfx_debug_plan_variant(int prec, int w1_fold, int force_direct, int pipe_waves_code, int B, int N, long long *grid_out) {
  const Plan plan = plan_launch({prec, w1_fold != 0, force_direct != 0, force_from_code(pipe_waves_code), B, N, g_num_cus});
  if (grid_out) *grid_out = plan.grid;
  return info(plan.v).name;
}
void dfx_debug_trace(void *device_buf, int capacity) {
  g_trace = static_cast<unsigned long long *>(device_buf);
  g_trace_cap = capacity;
}

int dfx_chain_num_snapshots(int num_timesteps, int ret_interval) {
  if (num_timesteps <= 0 || ret_interval <= 0) return 0;
  return num_timesteps / ret_interval;
}

int dfx_sample_chain(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x_T_noise,
                     const float *step_noise, uint64_t seed, uint64_t shape_offset, int ret_interval, float *traj, float *pred,
                     int B, int N, dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "sample_chain");
  if (rc) return rc < 0 ? rc : DFX_OK;
  DFX_REQUIRE(pred, "sample_chain: null pred");
  DFX_REQUIRE(!traj || ret_interval >= 1, "sample_chain: ret_interval must be >= 1 when traj is given");
  KParams p{};
  p.seg = seg; p.noise = step_noise; p.xT_noise = x_T_noise; p.out = pred; p.traj = traj; p.seed = seed; p.shape0 = shape_offset;
  p.B = B; p.N = N; p.t0 = d->dev.T - 1; p.nsteps = d->dev.T; p.ret_interval = ret_interval >= 1 ? ret_interval : 1;
  p.mode = MODE_CHAIN;
  return launch(d, shape_ctx, p, as_stream(stream));
}

// Partial chains: the last n_steps timesteps (n_steps-1 .. 0) from a caller's state, or from q_sample of a caller's clean cloud at t = n_steps-1
static int chain_from(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x, int n_steps, int start,
                      const float *start_noise, const float *step_noise, uint64_t seed, uint64_t shape_offset, const int32_t *hold,
                      int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream, const char *who) {
  const int rc = check_common(d, shape_ctx, seg, B, N, who);
  if (rc < 0) return rc;
  DFX_REQUIRE(n_steps >= 1 && n_steps <= d->dev.T, "%s: n_steps=%d outside [1,%d]", who, n_steps, d->dev.T);
  if (rc) return DFX_OK;
  DFX_REQUIRE(x, "%s: null start cloud", who);
  DFX_REQUIRE(pred, "%s: null pred", who);
  DFX_REQUIRE(!traj || ret_interval >= 1, "%s: ret_interval must be >= 1 when traj is given", who);
  KParams p{};
  p.x_in = x; p.seg = seg; p.noise = step_noise; p.xT_noise = start_noise; p.out = pred; p.traj = traj; p.seed = seed; p.shape0 = shape_offset;
  p.B = B; p.N = N; p.t0 = n_steps - 1; p.nsteps = n_steps; p.ret_interval = ret_interval >= 1 ? ret_interval : 1;
  p.mode = MODE_CHAIN; p.start = start; p.hold = hold;
  return launch(d, shape_ctx, p, as_stream(stream));
}

int dfx_sample_chain_from(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x_init, int n_steps,
                          const float *step_noise, uint64_t seed, uint64_t shape_offset, const int32_t *hold, int ret_interval,
                          float *traj, float *pred, int B, int N, dfx_stream_t stream) {
  return chain_from(d, shape_ctx, seg, x_init, n_steps, START_GIVEN, nullptr, step_noise, seed, shape_offset, hold, ret_interval, traj, pred,
                    B, N, stream, "sample_chain_from");
}

int dfx_refine_chain(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x_start, int n_steps,
                     const float *start_noise, const float *step_noise, uint64_t seed, uint64_t shape_offset, const int32_t *hold,
                     int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream) {
  return chain_from(d, shape_ctx, seg, x_start, n_steps, START_QSAMPLE, start_noise, step_noise, seed, shape_offset, hold, ret_interval, traj,
                    pred, B, N, stream, "refine_chain");
}

int dfx_sample_chain_ddim_from(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const int32_t *steps, int n_steps,
                               float eta, const float *x_init, const float *step_noise, uint64_t seed, uint64_t shape_offset,
                               const int32_t *hold, int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream) {
  const int rc = check_common(d, shape_ctx, seg, B, N, "sample_chain_ddim_from");
  if (rc < 0) return rc;
  KParams p{};
  if (int e = fill_ddim(d, p, steps, n_steps, eta, "sample_chain_ddim_from")) return e;
  DFX_REQUIRE(steps[0] == 0, "sample_chain_ddim_from: the step list must start at 0 (the t == 0 sample is 'pred')");
  if (rc) return DFX_OK;
  DFX_REQUIRE(x_init, "sample_chain_ddim_from: null start cloud");
  DFX_REQUIRE(pred, "sample_chain_ddim_from: null pred");
  DFX_REQUIRE(!traj || ret_interval >= 1, "sample_chain_ddim_from: ret_interval must be >= 1 when traj is given");
  p.x_in = x_init; p.seg = seg; p.noise = step_noise; p.out = pred; p.traj = traj; p.seed = seed; p.shape0 = shape_offset;
  p.B = B; p.N = N; p.t0 = p.ddim_t[0]; p.nsteps = n_steps; p.ret_interval = ret_interval >= 1 ? ret_interval : 1;
  p.mode = MODE_CHAIN; p.start = START_GIVEN; p.hold = hold;
  return launch(d, shape_ctx, p, as_stream(stream));
}

}  // extern "C"
