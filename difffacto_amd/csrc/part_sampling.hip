// Candidate selection for part-level sampling on gfx950 (include/dfx.h "Part-level sampling").
//
// Semantics of PartEncoder.subsample_params (part_encoders.py:545-589) and of the fit arg-min of sample_with_fixed_latents (:678-682):
//   draws     u ~ N(0,1) of shape (n_draws,3,J) per candidate (:555), reduced to (mean, unbiased std, min, max) per (axis, part): with
//             sigma > 0 every quantity the reference derives from mu + sigma u is a function of those four numbers
//   scores    the bounding-box-normalised per-part mean and 2 log std of those points (:555-560), in closed form
//   diverse   greedy farthest-candidate selection on the scores (:562-585)
//   fit       arg-min of the masked squared parameter distance to a target (:678-682)
//
// Mapping: draws and scores are one thread per (row, axis, part) / per row (fp64 arithmetic, one rounding to fp32); the selections
// are one 256-thread workgroup per group with the per-candidate state in LDS.  Everything discrete is decided by score_row /
// diverse_group / fit_group, written once over an execution context: BlockCtx (the kernels) and SerialCtx (the dfx_debug_*_host twins:
// one "thread", plain loops).  A candidate's distance is an fp64 sum in a fixed (c, j) order inside one thread, so the host twin and the
// kernel compute the same bits; the reductions across threads only compare.  Compiled with -ffp-contract=off (build.py).
#include "part_sampling.h"
#include "dfx_dropout.h"

#include <cmath>
#include <vector>

namespace {

using dfx::psel::MAX_DRAWS;
using dfx::psel::MAX_K;

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int MAX_J = 8;

// the best candidate so far: cls 1 = finite, 0 = non-finite, -1 = none; larger v wins, of equal ones the lowest index
struct Best {
  int cls;
  double v;
  int idx;
};
__host__ __device__ inline bool better(const Best &a, const Best &b) {
  if (a.cls != b.cls) return a.cls > b.cls;
  if (a.cls < 0) return false;
  if (a.v != b.v) return a.v > b.v;
  return a.idx < b.idx;
}

// ---- execution contexts ----
struct SerialCtx {
  int tid = 0, nt = 1;
  __host__ __device__ void sync() {}
  __host__ __device__ int sum_i(int v) { return v; }
  __host__ __device__ void best(Best &) {}
  __host__ __device__ void add(int32_t *p, int v) { *p += v; }
};

struct BlockCtx {
  int tid, nt;
  Best *red_b;   // NW
  int *red_i;    // NW
  __device__ void sync() { __syncthreads(); }
  __device__ int sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) red_i[tid >> 6] = v;
    __syncthreads();
    const int r = (red_i[0] + red_i[1]) + (red_i[2] + red_i[3]);
    __syncthreads();
    return r;
  }
  // all-reduce: every thread leaves with the workgroup's best
  __device__ void best(Best &b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const Best other{__shfl_down(b.cls, o), __shfl_down(b.v, o), __shfl_down(b.idx, o)};
      if (better(other, b)) b = other;
    }
    if ((tid & 63) == 0) red_b[tid >> 6] = b;
    __syncthreads();
    b = red_b[0];
    for (int w = 1; w < NW; ++w)
      if (better(red_b[w], b)) b = red_b[w];
    __syncthreads();
  }
  __device__ void add(int32_t *p, int v) { atomicAdd(p, v); }
};

// ---- scores of one candidate (part_encoders.py:555-560 in closed form) ----
// mean, logvar (3,J); valid (J); st (4,3,J) = mean, unbiased std, min, max of the candidate's unit draws; out (6,J).
// fp64 throughout, one rounding to fp32.  The box is taken over the valid parts; every part gets a score.
__host__ __device__ inline void score_row(const float *mean, const float *logvar, const float *valid, const float *st, int J, float *out) {
  const float *ubar = st, *ustd = st + 3 * J, *umin = st + 6 * J, *umax = st + 9 * J;
  double shift[3], scale = -INFINITY;
  for (int c = 0; c < 3; ++c) {
    double hi = -INFINITY, lo = INFINITY;
    for (int j = 0; j < J; ++j) {
      if (valid[j] == 0.0f) continue;
      const double mu = (double)mean[c * J + j], sg = exp(0.5 * (double)logvar[c * J + j]);
      hi = fmax(hi, mu + sg * (double)umax[c * J + j]);
      lo = fmin(lo, mu + sg * (double)umin[c * J + j]);
    }
    shift[c] = (hi + lo) / 2.0;
    scale = fmax(scale, hi - lo);
  }
  scale = scale / 2.0;
  for (int c = 0; c < 3; ++c)
    for (int j = 0; j < J; ++j) {
      const double mu = (double)mean[c * J + j], sg = exp(0.5 * (double)logvar[c * J + j]);
      out[c * J + j] = (float)((mu + sg * (double)ubar[c * J + j] - shift[c]) / scale);
      out[(3 + c) * J + j] = (float)(2.0 * log(sg * (double)ustd[c * J + j] / scale));
    }
}

// distance of two candidates' scores (6,J): sum over c < 6, valid j of (a - b)^2, in that order, over the number of valid parts;
// 0 for a group without a valid part (nothing counts: every candidate is as good as any other, and the picks are 0 .. P-1)
__host__ __device__ inline double score_dist(const float *a, const float *b, const float *valid, int J, double nv) {
  if (nv == 0.0) return 0.0;
  double acc = 0.0;
  for (int c = 0; c < 6; ++c)
    for (int j = 0; j < J; ++j) {
      if (valid[j] == 0.0f) continue;
      const double d = (double)a[c * J + j] - (double)b[c * J + j];
      acc += (double)valid[j] * (d * d);
    }
  return acc / nv;
}

// ---- greedy diverse selection of one group (:562-585) ----
// sc (K,6,J), valid (J); mind (K) and state (K) are staging: the smallest distance to the selected set, and 0 = free, 1 = selected,
// 2 = non-finite (on a valid part), 3 = non-finite and selected.  Starts from the lowest finite candidate (candidate 0 in the
// reference), then adds the free candidate whose smallest distance to the selected set is largest; non-finite ones, lowest index
// first, only once no finite one is free.  pick_dist (P) or null: every pick's smallest distance to the picks before it (0 for the
// first and for a non-finite one).
template <class Ctx>
__host__ __device__ void diverse_group(Ctx &cx, const float *sc, const float *valid, int K, int J, int P, double *mind,
                                       unsigned char *state, int32_t *idx, double *pick_dist, int32_t *n_bad) {
  double nv = 0.0;
  for (int j = 0; j < J; ++j) nv += (double)valid[j];
  int bad = 0;
  for (int i = cx.tid; i < K; i += cx.nt) {
    bool ok = true;
    for (int c = 0; c < 6; ++c)
      for (int j = 0; j < J; ++j)
        if (valid[j] != 0.0f && !__builtin_isfinite(sc[((size_t)i * 6 + c) * J + j])) ok = false;
    state[i] = ok ? 0 : 2;
    mind[i] = INFINITY;
    bad += !ok;
  }
  cx.sync();
  bad = cx.sum_i(bad);
  if (cx.tid == 0 && bad) cx.add(n_bad, bad);
  int last = -1;   // the finite candidate selected in the step before
  for (int p = 0; p < P; ++p) {
    Best b{-1, 0.0, -1};
    for (int i = cx.tid; i < K; i += cx.nt) {
      const unsigned char s = state[i];
      if (s == 1 || s == 3) continue;
      Best cand{0, 0.0, i};
      if (s == 0) {
        if (last >= 0) {
          const double d = score_dist(sc + (size_t)i * 6 * J, sc + (size_t)last * 6 * J, valid, J, nv);
          if (d < mind[i]) mind[i] = d;
        }
        cand.cls = 1;
        cand.v = p == 0 ? 0.0 : mind[i];
      }
      if (better(cand, b)) b = cand;
    }
    cx.best(b);
    if (cx.tid == 0) {
      idx[p] = b.idx, state[b.idx] = b.cls == 1 ? 1 : 3;
      if (pick_dist) pick_dist[p] = b.v;
    }
    last = b.cls == 1 ? b.idx : -1;
    cx.sync();
  }
}

// ---- fit selection of one group (:678-682) ----
// mean, logvar (K,3,J); tm, tl (3,J); w (J) = valid with the resampled part zeroed.  score_k = sum_j w_j sum_c [(mean - tm)^2, then
// (logvar - tl)^2], fp64 in that order; the smallest wins, of equal ones the lowest index; a non-finite score only when all are.
template <class Ctx>
__host__ __device__ void fit_group(Ctx &cx, const float *mean, const float *logvar, const float *tm, const float *tl, const float *w, int K,
                                   int J, int32_t *idx, float *fit, int32_t *n_bad) {
  Best b{-1, 0.0, -1};
  int bad = 0;
  for (int k = cx.tid; k < K; k += cx.nt) {
    const float *m = mean + (size_t)k * 3 * J, *l = logvar + (size_t)k * 3 * J;
    double acc = 0.0;
    for (int j = 0; j < J; ++j) {
      if (w[j] == 0.0f) continue;
      double inner = 0.0;
      for (int c = 0; c < 3; ++c) {
        const double d = (double)m[c * J + j] - (double)tm[c * J + j];
        inner += d * d;
      }
      for (int c = 0; c < 3; ++c) {
        const double d = (double)l[c * J + j] - (double)tl[c * J + j];
        inner += d * d;
      }
      acc += (double)w[j] * inner;
    }
    if (fit) fit[k] = (float)acc;
    const bool ok = __builtin_isfinite(acc);
    bad += !ok;
    const Best cand{ok ? 1 : 0, ok ? -acc : 0.0, k};
    if (better(cand, b)) b = cand;
  }
  cx.best(b);
  bad = cx.sum_i(bad);
  if (cx.tid == 0) {
    idx[0] = b.idx;
    if (bad) cx.add(n_bad, bad);
  }
}

// ---- draws: Philox4x32-7 (dfx_dropout.h), key = seed, counter = (group of four draws, purpose | axis * 8 + part, global row) ----
constexpr unsigned DRAW_PART = 0x9A570000u;

// two standard normals from two words (Box-Muller on 24-bit uniforms; u1 in (0,1])
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float *n0, float *n1) {
  const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = (float)(b >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1)), t = 6.283185307179586f * u2;
  *n0 = r * cosf(t), *n1 = r * sinf(t);
}
// draws 4 g .. 4 g + 3 of (row, axis c, part j)
__device__ __forceinline__ void normals4(unsigned long long seed, unsigned long long row, int c, int j, int g, float *n) {
  const uint4 r = dfx::philox4x32_7((unsigned)g, DRAW_PART | (unsigned)(c * 8 + j), (unsigned)row, (unsigned)(row >> 32), (unsigned)seed,
                                    (unsigned)(seed >> 32));
  box_muller(r.x, r.y, n, n + 1);
  box_muller(r.z, r.w, n + 2, n + 3);
}
// mean, unbiased std, min, max of the n_draws normals of (row, c, j): fp64 sums in draw order, one rounding
__device__ inline void draw_stats(unsigned long long seed, unsigned long long row, int c, int j, int n_draws, float *o_mean, float *o_std,
                                  float *o_min, float *o_max) {
  double s = 0.0, q = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int g = 0; g < n_draws / 4; ++g) {
    float n[4];
    normals4(seed, row, c, j, g, n);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s += (double)n[e];
      q += (double)n[e] * (double)n[e];
      lo = fminf(lo, n[e]);
      hi = fmaxf(hi, n[e]);
    }
  }
  const double nd = (double)n_draws;
  *o_mean = (float)(s / nd);
  *o_std = (float)sqrt(fmax(q - s * s / nd, 0.0) / (nd - 1.0));
  *o_min = lo, *o_max = hi;
}

__global__ void __launch_bounds__(NT) k_draw_stats(unsigned long long seed, long long row0, long long R, int J, int n_draws,
                                                   float *__restrict__ stats) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;   // (row, c, j)
  if (t >= R * 3 * J) return;
  const int j = (int)(t % J), c = (int)((t / J) % 3);
  const long long r = t / (3 * J);
  float *o = stats + (size_t)r * 12 * J + c * J + j;
  draw_stats(seed, (unsigned long long)(row0 + r), c, j, n_draws, o, o + 3 * J, o + 6 * J, o + 9 * J);
}

__global__ void __launch_bounds__(NT) k_draw_normals(unsigned long long seed, long long row0, long long total, int J, int n_draws,
                                                     float *__restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;   // (row, group of four draws, c, j)
  if (t >= total) return;
  const int j = (int)(t % J), c = (int)((t / J) % 3), g = (int)((t / (3 * J)) % (n_draws / 4));
  const long long r = t / ((long long)3 * J * (n_draws / 4));
  float n[4];
  normals4(seed, (unsigned long long)(row0 + r), c, j, g, n);
  for (int e = 0; e < 4; ++e) out[(((size_t)r * n_draws + 4 * g + e) * 3 + c) * J + j] = n[e];
}

__global__ void __launch_bounds__(NT) k_scores(const float *__restrict__ mean, const float *__restrict__ logvar,
                                               const float *__restrict__ valid, const float *__restrict__ stats, long long R, int K, int J,
                                               float *__restrict__ scores) {
  const long long r = (long long)blockIdx.x * NT + threadIdx.x;
  if (r >= R) return;
  score_row(mean + (size_t)r * 3 * J, logvar + (size_t)r * 3 * J, valid + (size_t)(r / K) * J, stats + (size_t)r * 12 * J, J,
            scores + (size_t)r * 6 * J);
}

__global__ void __launch_bounds__(NT) k_select_diverse(const float *__restrict__ scores, const float *__restrict__ valid, int K, int J, int P,
                                                       int32_t *__restrict__ idx, int32_t *__restrict__ n_bad) {
  __shared__ double mind[MAX_K];
  __shared__ unsigned char state[MAX_K];
  __shared__ Best red_b[NW];
  __shared__ int red_i[NW];
  const size_t g = blockIdx.x;
  BlockCtx cx{(int)threadIdx.x, NT, red_b, red_i};
  diverse_group(cx, scores + g * K * 6 * J, valid + g * J, K, J, P, mind, state, idx + g * P, nullptr, n_bad);
}

__global__ void __launch_bounds__(NT) k_select_fit(const float *__restrict__ mean, const float *__restrict__ logvar,
                                                   const float *__restrict__ tm, const float *__restrict__ tl, const float *__restrict__ w,
                                                   int K, int J, int32_t *__restrict__ idx, float *__restrict__ fit,
                                                   int32_t *__restrict__ n_bad) {
  __shared__ Best red_b[NW];
  __shared__ int red_i[NW];
  const size_t g = blockIdx.x;
  BlockCtx cx{(int)threadIdx.x, NT, red_b, red_i};
  fit_group(cx, mean + g * K * 3 * J, logvar + g * K * 3 * J, tm + g * 3 * J, tl + g * 3 * J, w + g * J, K, J, idx + g,
            fit ? fit + g * K : nullptr, n_bad);
}

__global__ void __launch_bounds__(NT) k_select_first(int total, int P, int32_t *__restrict__ idx) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t < total) idx[t] = t % P;
}

// idx (G P) holds picks in [0,K): written by the selection kernels of the same call, which write nothing else
__global__ void __launch_bounds__(NT) k_gather_picks(const int32_t *__restrict__ idx, const float *__restrict__ noise,
                                                     const float *__restrict__ mean, const float *__restrict__ logvar, long long GP, int K,
                                                     int Kc, int P, int ND, int J, float *__restrict__ noise_o, float *__restrict__ mean_o,
                                                     float *__restrict__ logvar_o) {
  const int per = ND + 6 * J;
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= GP * per) return;
  const long long o = t / per;
  const int e = (int)(t % per);
  const size_t src = (size_t)(o / P) * Kc + idx[o];   // among the Kc candidates per group the aligner saw; the noise holds K
  if (e < ND) {
    noise_o[(size_t)o * ND + e] = noise[((size_t)(o / P) * K + idx[o]) * ND + e];
  } else if (e < ND + 3 * J) {
    mean_o[(size_t)o * 3 * J + (e - ND)] = mean[src * 3 * J + (e - ND)];
  } else {
    logvar_o[(size_t)o * 3 * J + (e - ND - 3 * J)] = logvar[src * 3 * J + (e - ND - 3 * J)];
  }
}

inline unsigned grid_of(long long n) { return (unsigned)((n + NT - 1) / NT); }

int check_draws(const char *who, long long row0, long long R, int J, int n_draws) {
  DFX_REQUIRE(row0 >= 0 && R > 0, "%s: row0 = %lld, rows = %lld", who, row0, R);
  DFX_REQUIRE(J >= 1 && J <= MAX_J, "%s: n_class = %d outside [1,%d]", who, J, MAX_J);
  DFX_REQUIRE(n_draws >= 4 && n_draws % 4 == 0 && n_draws <= MAX_DRAWS, "%s: n_draws = %d must be a multiple of 4 in [4,%d]", who, n_draws,
              MAX_DRAWS);
  DFX_REQUIRE(R * 3 * J * (long long)(n_draws / 4) <= 0x7fffffffLL * NT, "%s: %lld rows in one launch", who, R);
  return DFX_OK;
}

}  // namespace

namespace dfx {
namespace psel {

int check_shape(const char *who, long long G, int K, int J) {
  DFX_REQUIRE(G > 0 && K > 0, "%s: G = %lld, K = %d must be positive", who, G, K);
  DFX_REQUIRE(K <= MAX_K, "%s: K = %d above %d", who, K, MAX_K);
  DFX_REQUIRE(J >= 1 && J <= MAX_J, "%s: n_class = %d outside [1,%d]", who, J, MAX_J);
  DFX_REQUIRE(G * K <= 0x7fffffffLL, "%s: %lld candidate rows in one call", who, G * K);
  return DFX_OK;
}

int launch_draw_stats(uint64_t seed, long long row0, long long R, int J, int n_draws, float *stats, hipStream_t st) {
  k_draw_stats<<<grid_of(R * 3 * J), NT, 0, st>>>((unsigned long long)seed, row0, R, J, n_draws, stats);
  return check_launch("part_draw_stats");
}

int launch_scores(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int J, float *scores,
                  hipStream_t st) {
  const long long R = (long long)G * K;
  k_scores<<<grid_of(R), NT, 0, st>>>(mean, logvar, valid, stats, R, K, J, scores);
  return check_launch("part_param_scores");
}

int launch_diverse(const float *scores, const float *valid, int G, int K, int J, int P, int32_t *idx, int32_t *n_bad, hipStream_t st) {
  k_select_diverse<<<G, NT, 0, st>>>(scores, valid, K, J, P, idx, n_bad);
  return check_launch("select_diverse");
}

int launch_fit(const float *mean, const float *logvar, const float *target_mean, const float *target_logvar, const float *weight, int G,
               int K, int J, int32_t *idx, float *fit, int32_t *n_bad, hipStream_t st) {
  k_select_fit<<<G, NT, 0, st>>>(mean, logvar, target_mean, target_logvar, weight, K, J, idx, fit, n_bad);
  return check_launch("select_fit");
}

int launch_first(int G, int P, int32_t *idx, hipStream_t st) {
  k_select_first<<<grid_of((long long)G * P), NT, 0, st>>>(G * P, P, idx);
  return check_launch("select_first");
}

int launch_gather(const int32_t *idx, const float *noise, const float *mean, const float *logvar, int G, int K, int Kc, int P, int ND, int J,
                  float *noise_o, float *mean_o, float *logvar_o, hipStream_t st) {
  const long long GP = (long long)G * P;
  k_gather_picks<<<grid_of(GP * (ND + 6 * J)), NT, 0, st>>>(idx, noise, mean, logvar, GP, K, Kc, P, ND, J, noise_o, mean_o, logvar_o);
  return check_launch("gather_picks");
}

}  // namespace psel
}  // namespace dfx

extern "C" {

int dfx_part_draw_stats(uint64_t seed, long long row0, long long rows, int n_class, int n_draws, float *stats, dfx_stream_t stream) {
  if (int rc = check_draws("part_draw_stats", row0, rows, n_class, n_draws)) return rc;
  DFX_REQUIRE(stats, "part_draw_stats: null pointer");
  return dfx::psel::launch_draw_stats(seed, row0, rows, n_class, n_draws, stats, dfx::as_stream(stream));
}

int dfx_debug_part_draw_normals(uint64_t seed, long long row0, int rows, int n_class, int n_draws, float *normals, dfx_stream_t stream) {
  if (int rc = check_draws("debug_part_draw_normals", row0, rows, n_class, n_draws)) return rc;
  DFX_REQUIRE(normals, "debug_part_draw_normals: null pointer");
  const long long total = (long long)rows * 3 * n_class * (n_draws / 4);
  k_draw_normals<<<grid_of(total), NT, 0, dfx::as_stream(stream)>>>((unsigned long long)seed, row0, total, n_class, n_draws, normals);
  return dfx::check_launch("debug_part_draw_normals");
}

int dfx_select_diverse(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int n_class, int P,
                       int32_t *idx, float *scores, int32_t *n_bad, dfx_stream_t stream) {
  if (int rc = dfx::psel::check_shape("select_diverse", G, K, n_class)) return rc;
  DFX_REQUIRE(P >= 1 && P <= K, "select_diverse: P = %d outside [1,K = %d]", P, K);
  DFX_REQUIRE(mean && logvar && valid && stats && idx && scores && n_bad, "select_diverse: null pointer");
  hipStream_t st = dfx::as_stream(stream);
  DFX_HIP_TRY(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  if (int rc = dfx::psel::launch_scores(mean, logvar, valid, stats, G, K, n_class, scores, st)) return rc;
  return dfx::psel::launch_diverse(scores, valid, G, K, n_class, P, idx, n_bad, st);
}

int dfx_select_fit(const float *mean, const float *logvar, const float *target_mean, const float *target_logvar, const float *weight, int G,
                   int K, int n_class, int32_t *idx, float *fit, int32_t *n_bad, dfx_stream_t stream) {
  if (int rc = dfx::psel::check_shape("select_fit", G, K, n_class)) return rc;
  DFX_REQUIRE(mean && logvar && target_mean && target_logvar && weight && idx && n_bad, "select_fit: null pointer");
  hipStream_t st = dfx::as_stream(stream);
  DFX_HIP_TRY(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  return dfx::psel::launch_fit(mean, logvar, target_mean, target_logvar, weight, G, K, n_class, idx, fit, n_bad, st);
}

// ---- host twins: the same routines on host pointers, groups one after the other ----
int dfx_debug_part_scores_host(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int n_class,
                               float *scores) {
  if (int rc = dfx::psel::check_shape("debug_part_scores_host", G, K, n_class)) return rc;
  DFX_REQUIRE(mean && logvar && valid && stats && scores, "debug_part_scores_host: null pointer");
  const int J = n_class;
  for (size_t r = 0; r < (size_t)G * K; ++r)
    score_row(mean + r * 3 * J, logvar + r * 3 * J, valid + (r / K) * J, stats + r * 12 * J, J, scores + r * 6 * J);
  return DFX_OK;
}

int dfx_debug_select_diverse_host(const float *scores, const float *valid, int G, int K, int n_class, int P, int32_t *idx, double *pick_dist,
                                  int32_t *n_bad) {
  if (int rc = dfx::psel::check_shape("debug_select_diverse_host", G, K, n_class)) return rc;
  DFX_REQUIRE(P >= 1 && P <= K, "debug_select_diverse_host: P = %d outside [1,K = %d]", P, K);
  DFX_REQUIRE(scores && valid && idx && n_bad, "debug_select_diverse_host: null pointer");
  std::vector<double> mind((size_t)K);
  std::vector<unsigned char> state((size_t)K);
  *n_bad = 0;
  for (size_t g = 0; g < (size_t)G; ++g) {
    SerialCtx cx;
    diverse_group(cx, scores + g * K * 6 * n_class, valid + g * n_class, K, n_class, P, mind.data(), state.data(), idx + g * P,
                  pick_dist ? pick_dist + g * P : nullptr, n_bad);
  }
  return DFX_OK;
}

int dfx_debug_select_fit_host(const float *mean, const float *logvar, const float *target_mean, const float *target_logvar,
                              const float *weight, int G, int K, int n_class, int32_t *idx, float *fit, int32_t *n_bad) {
  if (int rc = dfx::psel::check_shape("debug_select_fit_host", G, K, n_class)) return rc;
  DFX_REQUIRE(mean && logvar && target_mean && target_logvar && weight && idx && n_bad, "debug_select_fit_host: null pointer");
  const int J = n_class;
  *n_bad = 0;
  for (size_t g = 0; g < (size_t)G; ++g) {
    SerialCtx cx;
    fit_group(cx, mean + g * K * 3 * J, logvar + g * K * 3 * J, target_mean + g * 3 * J, target_logvar + g * 3 * J, weight + g * J, K, J,
              idx + g, fit ? fit + g * K : nullptr, n_bad);
  }
  return DFX_OK;
}

}  // extern "C"
