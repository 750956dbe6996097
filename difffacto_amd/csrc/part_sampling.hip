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
// are one 256-thread workgroup per group with the per-candidate state in LDS; the selection over all rows of a call
// (dfx_select_diverse_global) is one 512-thread workgroup up to 512 rows and one launch per pick above.  Everything discrete is decided by score_row /
// diverse_group / diverse_global / fit_group, written once over an execution context: BlockCtx (the kernels) and SerialCtx (the dfx_debug_*_host twins:
// one "thread", plain loops).  A candidate's distance is an fp64 sum in a fixed (c, j) order inside one thread, so the host twin and the
// kernel compute the same bits; the reductions across threads only compare.  Compiled with -ffp-contract=off (build.py).
#include "part_sampling.h"
#include "dfx_dropout.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {

using dfx::psel::MAX_DRAWS;
using dfx::psel::MAX_K;
using dfx::psel::MAX_GLOBAL_ROWS;

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

// a workgroup of NWV wavefronts
template <int NWV>
struct BlockCtxT {
  int tid, nt;
  Best *red_b;   // NWV
  int *red_i;    // NWV
  __device__ void sync() { __syncthreads(); }
  __device__ int sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) red_i[tid >> 6] = v;
    __syncthreads();
    int r = 0;
    for (int w = 0; w < NWV; ++w) r += red_i[w];
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
    for (int w = 1; w < NWV; ++w)
      if (better(red_b[w], b)) b = red_b[w];
    __syncthreads();
  }
  __device__ void add(int32_t *p, int v) { atomicAdd(p, v); }
};
using BlockCtx = BlockCtxT<NW>;

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

// ---- greedy diverse selection over all rows of a call (subsample_params_global, part_encoders.py:591-621, as intended) ----
// sc (R,6,J), valid (G,J): the mask of row i is valid[i / K].  Two rows are compared on the parts valid in both:
//   n(i,s) = sum_j m_i[j] m_s[j],  d(i,s) = sum over c < 6, j valid in both of (s_i - s_s)^2 / n(i,s), fp64 in (c, j) order.
// A pair without a common part (n = 0; the reference divides 0 by 0 there and its arg-max goes to NaN) puts no constraint on the
// candidate: it is skipped in the minimum, so a candidate that shares no part with any pick keeps mind = +inf and is picked next.
// mind (R), state (R) as in diverse_group; a row is finite when it has a valid part and every score on its valid parts is finite.
// cur (7 J) is staging for the newest pick's scores and mask, written once per step and read by every thread.
// rule 0 (farthest): mind follows every pick; rule 1 (first pick): mind follows pick 0 only, which is what the reference executes
// (its out_score is never appended to, :603-619) when all rows share one mask.  A row is never picked twice (the reference can
// repeat a row once every distance is 0).  pick_dist (P) or null: the winner's mind; 0 for pick 0 and for a non-finite pick.
// The pieces below are shared by diverse_global (one context runs the whole call: the host twin and the one-workgroup kernel) and
// k_select_diverse_global_step (one launch per pick).

// a row is finite when it has a valid part and every score on its own valid parts is finite
__host__ __device__ inline bool global_row_ok(const float *sc, const float *valid, int i, int K, int J) {
  const float *m = valid + (size_t)(i / K) * J;
  bool any = false, fin = true;
  for (int j = 0; j < J; ++j) any = any || m[j] != 0.0f;
  for (int c = 0; c < 6; ++c)
    for (int j = 0; j < J; ++j)
      if (m[j] != 0.0f && !__builtin_isfinite(sc[((size_t)i * 6 + c) * J + j])) fin = false;
  return any && fin;
}
// free finite row i as a candidate of step p; with `fresh`, mind[i] first follows the pick staged in cur (scores, then mask)
__host__ __device__ inline Best global_candidate(const float *sc, const float *valid, int i, int K, int J, int p, bool fresh, const float *cur,
                                                 double *mind) {
  if (fresh) {
    const float *a = sc + (size_t)i * 6 * J, *m = valid + (size_t)(i / K) * J, *ms = cur + 6 * J;
    double n = 0.0;
    for (int j = 0; j < J; ++j) n += (double)(m[j] * ms[j]);
    if (n != 0.0) {
      double acc = 0.0;
      for (int c = 0; c < 6; ++c)
        for (int j = 0; j < J; ++j) {
          const float w = m[j] * ms[j];
          if (w == 0.0f) continue;
          const double d = (double)a[c * J + j] - (double)cur[c * J + j];
          acc += (double)w * (d * d);
        }
      const double d = acc / n;
      if (d < mind[i]) mind[i] = d;
    }
  }
  return Best{1, p == 0 ? 0.0 : mind[i], i};
}
// does mind follow the pick b of step p?
__host__ __device__ inline bool global_fresh(const Best &b, int rule, int p) { return b.cls == 1 && (rule == DFX_DIVERSE_FARTHEST || p == 0); }
// stage pick `row` for the next step
template <class Ctx>
__host__ __device__ inline void global_stage(Ctx &cx, const float *sc, const float *valid, int row, int K, int J, float *cur) {
  for (int t = cx.tid; t < 7 * J; t += cx.nt) cur[t] = t < 6 * J ? sc[(size_t)row * 6 * J + t] : valid[(size_t)(row / K) * J + (t - 6 * J)];
}

template <class Ctx>
__host__ __device__ void diverse_global(Ctx &cx, const float *sc, const float *valid, int R, int K, int J, int P, int rule, double *mind,
                                        unsigned char *state, float *cur, int32_t *idx, double *pick_dist, int32_t *n_bad) {
  int bad = 0;
  for (int i = cx.tid; i < R; i += cx.nt) {
    const bool ok = global_row_ok(sc, valid, i, K, J);
    state[i] = ok ? 0 : 2;
    mind[i] = INFINITY;
    bad += !ok;
  }
  cx.sync();
  bad = cx.sum_i(bad);
  if (cx.tid == 0 && bad) cx.add(n_bad, bad);
  bool fresh = false;   // cur holds a finite pick that mind has not seen yet
  for (int p = 0; p < P; ++p) {
    Best b{-1, 0.0, -1};
    for (int i = cx.tid; i < R; i += cx.nt) {
      const unsigned char s = state[i];
      if (s == 1 || s == 3) continue;
      const Best cand = s == 0 ? global_candidate(sc, valid, i, K, J, p, fresh, cur, mind) : Best{0, 0.0, i};
      if (better(cand, b)) b = cand;
    }
    cx.best(b);
    fresh = global_fresh(b, rule, p);
    if (cx.tid == 0) {
      idx[p] = b.idx, state[b.idx] = b.cls == 1 ? 1 : 3;
      if (pick_dist) pick_dist[p] = b.v;
    }
    if (fresh) global_stage(cx, sc, valid, b.idx, K, J, cur);
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

// ---- draws: Philox4x32-7 (dfx_dropout.h), key = seed, counter = (group of four draws, purpose | axis * 8 + part, global row lo, hi) ----
// DESIGN.md "Random streams" lists the layout; tests/test_gpu_random_streams.py judges the normals against oracle/philox.py in units of z.
constexpr unsigned DRAW_PART = 0x9A570000u;

// two standard normals from two words (Box-Muller on 24-bit uniforms; u1 in (0,1), u2 in [0,1)).  The angle 2 pi u2 goes through cospif / sinpif
// on the exact 2 u2: the float32 2 pi is 2.8e-8 too large, which as `cosf(6.2831855f * u2)` shifted the mean of the even draws by +3.5e-8
// (E[r] E[t sin t] / 2 pi times that) — 24 standard errors in tests/test_gpu_random_streams.py's comparison with the float64 statement.
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float *n0, float *n1) {
  const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = (float)(b >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1)), t = 2.0f * u2;
  *n0 = r * cospif(t), *n1 = r * sinpif(t);
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

// One workgroup for the whole call, for at most GLOBAL_ONE_WG_ROWS rows (one per thread): no launch between picks, per-row state
// (mind fp64, one state byte) in LDS.
constexpr int GLOBAL_ONE_WG_ROWS = 512;
constexpr int GNT = GLOBAL_ONE_WG_ROWS;
constexpr int GNW = GNT / 64;
__global__ void __launch_bounds__(GNT) k_select_diverse_global(const float *__restrict__ scores, const float *__restrict__ valid, int R, int K,
                                                               int J, int P, int rule, int32_t *__restrict__ idx, int32_t *__restrict__ n_bad) {
  __shared__ double mind[GLOBAL_ONE_WG_ROWS];
  __shared__ unsigned char state[GLOBAL_ONE_WG_ROWS];
  __shared__ Best red_b[GNW];
  __shared__ int red_i[GNW];
  __shared__ float cur[7 * MAX_J];
  BlockCtxT<GNW> cx{(int)threadIdx.x, GNT, red_b, red_i};
  diverse_global(cx, scores, valid, R, K, J, P, rule, mind, state, cur, idx, nullptr, n_bad);
}

// The same selection with one stream-ordered launch per pick, for more rows than one workgroup handles well: launch p first reduces
// the per-block bests of launch p - 1 (every block, redundantly, with the same total order: one result) into pick p - 1, then lets
// mind follow it and writes its own per-block best of step p.  A row always belongs to the same thread of the same block, which alone
// writes its mind and state (in the workspace), the previous pick's state included; blk holds two sets of gridDim.x bests, used in
// turn.  Launch P only reduces and writes the last pick.  No workgroup waits for another one inside a launch.
constexpr int GLOBAL_GRID_BLOCKS = 256;
__global__ void __launch_bounds__(NT) k_select_diverse_global_step(const float *__restrict__ scores, const float *__restrict__ valid, int R, int K,
                                                                    int J, int P, int p, int rule, double *__restrict__ mind,
                                                                    unsigned char *__restrict__ state, Best *__restrict__ blk,
                                                                    int32_t *__restrict__ idx, int32_t *__restrict__ n_bad) {
  __shared__ Best red_b[NW];
  __shared__ int red_i[NW];
  __shared__ float cur[7 * MAX_J];
  BlockCtx cx{(int)threadIdx.x, NT, red_b, red_i};
  const int nb = gridDim.x;
  Best prev{-1, 0.0, -1};
  bool fresh = false;
  if (p > 0) {
    const Best *src = blk + (size_t)((p - 1) & 1) * nb;
    for (int k = cx.tid; k < nb; k += NT)
      if (better(src[k], prev)) prev = src[k];
    cx.best(prev);
    fresh = global_fresh(prev, rule, p - 1);
    if (blockIdx.x == 0 && cx.tid == 0) idx[p - 1] = prev.idx;
    if (fresh) global_stage(cx, scores, valid, prev.idx, K, J, cur);
    cx.sync();
  }
  if (p == P) return;
  Best b{-1, 0.0, -1};
  int bad = 0;
  for (int i = blockIdx.x * NT + cx.tid; i < R; i += nb * NT) {
    unsigned char s;
    if (p == 0) {
      const bool ok = global_row_ok(scores, valid, i, K, J);
      s = ok ? 0 : 2;
      state[i] = s, mind[i] = INFINITY;
      bad += !ok;
    } else {
      s = state[i];
      if (i == prev.idx) state[i] = s = prev.cls == 1 ? 1 : 3;
    }
    if (s == 1 || s == 3) continue;
    const Best cand = s == 0 ? global_candidate(scores, valid, i, K, J, p, fresh, cur, mind) : Best{0, 0.0, i};
    if (better(cand, b)) b = cand;
  }
  cx.best(b);
  if (cx.tid == 0) blk[(size_t)(p & 1) * nb + blockIdx.x] = b;
  if (p == 0) {
    bad = cx.sum_i(bad);
    if (cx.tid == 0 && bad) cx.add(n_bad, bad);
  }
}

// idx (P) holds global rows in [0,R): written by k_select_diverse_global of the same call
__global__ void __launch_bounds__(NT) k_gather_rows(const int32_t *__restrict__ idx, const float *__restrict__ noise,
                                                    const float *__restrict__ mean, const float *__restrict__ logvar, long long P, int ND, int J,
                                                    float *__restrict__ noise_o, float *__restrict__ mean_o, float *__restrict__ logvar_o) {
  const int per = ND + 6 * J;
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= P * per) return;
  const long long o = t / per;
  const int e = (int)(t % per);
  const size_t src = (size_t)idx[o];
  if (e < ND) {
    noise_o[(size_t)o * ND + e] = noise[src * ND + e];
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

int check_shape_global(const char *who, long long G, int K, int J, int P, int rule) {
  if (int rc = check_shape(who, G, K, J)) return rc;
  DFX_REQUIRE(G * K <= MAX_GLOBAL_ROWS, "%s: %lld candidate rows above %d", who, G * K, MAX_GLOBAL_ROWS);
  DFX_REQUIRE(P >= 1 && P <= G * K, "%s: P = %d outside [1,G K = %lld]", who, P, G * K);
  DFX_REQUIRE(rule == DFX_DIVERSE_FARTHEST || rule == DFX_DIVERSE_FIRST_PICK, "%s: rule %d not in {0 farthest, 1 first pick}", who, rule);
  return DFX_OK;
}

// mind (rows fp64) | two sets of per-block bests | state (rows bytes)
size_t diverse_global_state_bytes(long long rows) {
  return ((size_t)rows * 8 + 2 * GLOBAL_GRID_BLOCKS * sizeof(Best) + (size_t)rows + 15) & ~(size_t)15;
}

bool g_diverse_global_launches = false;   // dfx_debug_diverse_global_path

int launch_diverse_global(const float *scores, const float *valid, int G, int K, int J, int P, int rule, int32_t *idx, int32_t *n_bad,
                          void *state, hipStream_t st) {
  const int R = G * K;
  // one workgroup up to GLOBAL_ONE_WG_ROWS rows; above that one launch per pick over many CUs (where the two meet)
  if (R <= GLOBAL_ONE_WG_ROWS && !g_diverse_global_launches) {
    k_select_diverse_global<<<1, GNT, 0, st>>>(scores, valid, R, K, J, P, rule, idx, n_bad);
    return check_launch("select_diverse_global");
  }
  double *mind = static_cast<double *>(state);
  Best *blk = reinterpret_cast<Best *>(mind + R);
  unsigned char *state_b = reinterpret_cast<unsigned char *>(blk + 2 * GLOBAL_GRID_BLOCKS);
  const int need = (R + NT - 1) / NT, nb = need < GLOBAL_GRID_BLOCKS ? need : GLOBAL_GRID_BLOCKS;
  for (int p = 0; p <= P; ++p)
    k_select_diverse_global_step<<<nb, NT, 0, st>>>(scores, valid, R, K, J, P, p, rule, mind, state_b, blk, idx, n_bad);
  return check_launch("select_diverse_global (one launch per pick)");
}

int launch_gather_rows(const int32_t *idx, const float *noise, const float *mean, const float *logvar, int P, int ND, int J, float *noise_o,
                       float *mean_o, float *logvar_o, hipStream_t st) {
  k_gather_rows<<<grid_of((long long)P * (ND + 6 * J)), NT, 0, st>>>(idx, noise, mean, logvar, P, ND, J, noise_o, mean_o, logvar_o);
  return check_launch("gather_rows");
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

size_t dfx_select_diverse_global_workspace_bytes(long long rows) {
  if (rows <= 0) return 0;
  return dfx::psel::diverse_global_state_bytes(rows) + (size_t)rows * 6 * MAX_J * sizeof(float);
}

int dfx_select_diverse_global(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int n_class, int P,
                              int rule, int32_t *idx, float *scores, int32_t *n_bad, void *workspace, size_t workspace_bytes,
                              dfx_stream_t stream) {
  if (int rc = dfx::psel::check_shape_global("select_diverse_global", G, K, n_class, P, rule)) return rc;
  DFX_REQUIRE(mean && logvar && valid && stats && idx && n_bad && workspace, "select_diverse_global: null pointer");
  const long long R = (long long)G * K;
  DFX_REQUIRE(workspace_bytes >= dfx_select_diverse_global_workspace_bytes(R), "select_diverse_global: workspace of %zu bytes, %zu needed",
              workspace_bytes, dfx_select_diverse_global_workspace_bytes(R));
  DFX_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "select_diverse_global: workspace is not 16-byte aligned");
  hipStream_t st = dfx::as_stream(stream);
  float *sc = scores ? scores : reinterpret_cast<float *>(static_cast<char *>(workspace) + dfx::psel::diverse_global_state_bytes(R));
  DFX_HIP_TRY(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  if (int rc = dfx::psel::launch_scores(mean, logvar, valid, stats, G, K, n_class, sc, st)) return rc;
  return dfx::psel::launch_diverse_global(sc, valid, G, K, n_class, P, rule, idx, n_bad, workspace, st);
}

void dfx_debug_diverse_global_path(int path) { dfx::psel::g_diverse_global_launches = path == 1; }

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

int dfx_debug_select_diverse_global_host(const float *scores, const float *valid, int G, int K, int n_class, int P, int rule, int32_t *idx,
                                         double *pick_dist, int32_t *n_bad) {
  if (int rc = dfx::psel::check_shape_global("debug_select_diverse_global_host", G, K, n_class, P, rule)) return rc;
  DFX_REQUIRE(scores && valid && idx && n_bad, "debug_select_diverse_global_host: null pointer");
  const int R = G * K;
  std::vector<double> mind((size_t)R);
  std::vector<unsigned char> state((size_t)R);
  float cur[7 * MAX_J];
  *n_bad = 0;
  SerialCtx cx;
  diverse_global(cx, scores, valid, R, K, n_class, P, rule, mind.data(), state.data(), cur, idx, pick_dist, n_bad);
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
