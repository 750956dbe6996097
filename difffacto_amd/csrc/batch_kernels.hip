// Training-batch assembly for gfx950 from a device-resident ragged set of labelled clouds (include/dfx.h).
//
// Semantics of _ShapeNetSegParts.__getitem__ (python/difffacto/datasets/shapenet_seg.py:436-543) with pc_norm
// (dataset_utils.py:55-95), in the reference's order: resample with replacement, shape normalisation, the parts one after the other
// on the CURRENT labels (statistics and per-part normalisation from 10 points on, relabelling to the nearest other point below),
// part dropout, augmentation of ref / shift / scale.  Every random input (choice, drop_u, aug_u) is an argument; k_batch_draw
// writes them from Philox for callers that have none.
//
// Mapping: one 256-thread workgroup per shape; the sampled cloud lives in LDS as x / y / z / label arrays (16 N bytes) and every
// later pass reads it there.  Statistics are fp64 sums (per-thread strided, wave shuffle, LDS tree over the four waves: a fixed
// order, no floating-point atomics) rounded once to float32.  The per-shape routine build_item is written once over an execution
// context: BlockCtx (the kernel) and SerialCtx (dfx_debug_batch_build_host: one "thread", plain loops), so the host twin runs the
// kernel's own decisions and element arithmetic; only the order of the fp64 sums differs.
// This file is compiled with -ffp-contract=off (build.py): float32 expressions round after every operation, as numpy's do.
#include "dfx_common.h"
#include "dfx_dropout.h"

#include <cmath>
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int BATCH_MAX_C = 8;
constexpr int BATCH_MIN_N = 10;
constexpr int BATCH_MAX_N = 8192;
constexpr int SMALL_PART = 10;   // a part of fewer points is relabelled (shapenet_seg.py:474)

enum ScaleMode { SM_NONE = 0, SM_UNIT = 1, SM_HALF = 2, SM_34 = 3, SM_BBOX = 4, SM_CANONICAL = 5, SM_CANONICAL_BBOX = 6 };

struct Item {
  // the cloud and the item's draws
  const float *pts;        // (M,3)
  const int32_t *plab;     // (M)
  long long M;
  const int32_t *choice;   // (N)
  const float *drop_u;     // (C)
  const float *aug_u;      // (6)
  int N, C, scale_mode, part_scale_mode, clip, aug_shift, aug_scale;
  double dropout_part;
  // the item's outputs
  float *ref, *input;              // (N,3)
  int64_t *seg, *attn;             // (N), (N,C)
  float *present, *dp_present;     // (C)
  float *part_shift, *part_scale;  // (3,C)
  float *shift, *scale;            // (3), (3)
  int32_t *status;                 // [0] sampled labels outside [0,C), [1] items with a bad index / cloud / choice
  // staging: the sampled cloud
  float *x, *y, *z;
  int32_t *lab;
  int *scratch;                    // [0] list length, [1..9] list, [10..18] new labels
};

struct Stats {
  int cnt;
  double mean[3], sd[3], flat_sd;
  float mn[3], mx[3];
};

// ---- execution contexts ----
struct SerialCtx {
  int tid = 0, nt = 1;
  __host__ __device__ void sync() {}
  __host__ __device__ void sum(double *, int) {}
  __host__ __device__ int sum_i(int v) { return v; }
  __host__ __device__ void minmax3(float *, float *) {}
  __host__ __device__ void argmin(float &, int &) {}
  __host__ __device__ int append(int *count) { return (*count)++; }
  __host__ __device__ void add_status(int32_t *p, int v) { *p += v; }
};

struct BlockCtx {
  int tid, nt;
  double *red_d;   // NW * 4
  float *red_f;    // NW * 6
  int *red_i;      // NW * 2
  __device__ void sync() { __syncthreads(); }
  // all-reduce of k <= 4 doubles: shuffle inside the wave, then ((w0 + w1) + (w2 + w3)) from LDS
  __device__ void sum(double *v, int k) {
    for (int j = 0; j < k; ++j) {
      double s = v[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s = __dadd_rn(s, __shfl_down(s, o));
      if ((tid & 63) == 0) red_d[(tid >> 6) * 4 + j] = s;
    }
    __syncthreads();
    for (int j = 0; j < k; ++j) v[j] = __dadd_rn(__dadd_rn(red_d[j], red_d[4 + j]), __dadd_rn(red_d[8 + j], red_d[12 + j]));
    __syncthreads();
  }
  __device__ int sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) red_i[tid >> 6] = v;
    __syncthreads();
    const int r = (red_i[0] + red_i[1]) + (red_i[2] + red_i[3]);
    __syncthreads();
    return r;
  }
  __device__ void minmax3(float *lo, float *hi) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float l = lo[a], h = hi[a];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) l = fminf(l, __shfl_down(l, o)), h = fmaxf(h, __shfl_down(h, o));
      if ((tid & 63) == 0) red_f[(tid >> 6) * 6 + a] = l, red_f[(tid >> 6) * 6 + 3 + a] = h;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(fminf(red_f[a], red_f[6 + a]), fminf(red_f[12 + a], red_f[18 + a]));
      hi[a] = fmaxf(fmaxf(red_f[3 + a], red_f[9 + a]), fmaxf(red_f[15 + a], red_f[21 + a]));
    }
    __syncthreads();
  }
  // the smallest distance, of equal ones the lowest index
  __device__ void argmin(float &d, int &idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_down(d, o);
      const int oi = __shfl_down(idx, o);
      if (oi >= 0 && (idx < 0 || od < d || (od == d && oi < idx))) d = od, idx = oi;
    }
    if ((tid & 63) == 0) red_f[tid >> 6] = d, red_i[tid >> 6] = idx;
    __syncthreads();
    d = red_f[0], idx = red_i[0];
    for (int w = 1; w < NW; ++w) {
      const float od = red_f[w];
      const int oi = red_i[w];
      if (oi >= 0 && (idx < 0 || od < d || (od == d && oi < idx))) d = od, idx = oi;
    }
    __syncthreads();
  }
  __device__ int append(int *count) { return atomicAdd(count, 1); }
  __device__ void add_status(int32_t *p, int v) { atomicAdd(p, v); }
};

// ---- statistics of the points labelled `part` (part < 0: every point): count, fp64 mean / std(0) / std of all coordinates, bounds ----
template <class Ctx>
__host__ __device__ Stats part_stats(Ctx &cx, const Item &it, int part) {
  Stats s;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int cnt = 0;
  for (int n = cx.tid; n < it.N; n += cx.nt) {
    if (part >= 0 && it.lab[n] != part) continue;
    const float v[3] = {it.x[n], it.y[n], it.z[n]};
    ++cnt;
    for (int a = 0; a < 3; ++a) {
      acc[a] += (double)v[a];
      lo[a] = fminf(lo[a], v[a]);
      hi[a] = fmaxf(hi[a], v[a]);
    }
  }
  s.cnt = cx.sum_i(cnt);
  cx.sum(acc, 3);
  cx.minmax3(lo, hi);
  const double inv = 1.0 / (double)s.cnt;
  const double flat_mean = ((acc[0] + acc[1]) + acc[2]) / (3.0 * (double)s.cnt);
  for (int a = 0; a < 3; ++a) s.mean[a] = acc[a] * inv, s.mn[a] = lo[a], s.mx[a] = hi[a];
  double dev[4] = {0.0, 0.0, 0.0, 0.0};
  for (int n = cx.tid; n < it.N; n += cx.nt) {
    if (part >= 0 && it.lab[n] != part) continue;
    const double v[3] = {(double)it.x[n], (double)it.y[n], (double)it.z[n]};
    for (int a = 0; a < 3; ++a) {
      const double d = v[a] - s.mean[a], f = v[a] - flat_mean;
      dev[a] += d * d;
      dev[3] += f * f;
    }
  }
  cx.sum(dev, 4);
  for (int a = 0; a < 3; ++a) s.sd[a] = sqrt(dev[a] * inv);
  s.flat_sd = sqrt(dev[3] / (3.0 * (double)s.cnt));
  return s;
}

// pc_norm's shift and scale (dataset_utils.py:55-91), float32 as numpy holds them
__host__ __device__ inline void norm_params(int mode, int clip, const Stats &s, float *shift, float *scale) {
  const bool bbox = mode == SM_BBOX || mode == SM_CANONICAL_BBOX;
  for (int a = 0; a < 3; ++a) {
    if (mode == SM_NONE) shift[a] = 0.0f;
    else if (bbox) shift[a] = (s.mn[a] + s.mx[a]) / 2.0f;
    else shift[a] = (float)s.mean[a];
  }
  if (mode == SM_CANONICAL || mode == SM_CANONICAL_BBOX) {
    for (int a = 0; a < 3; ++a) {
      float v = mode == SM_CANONICAL ? (float)s.sd[a] : (s.mx[a] - s.mn[a]) / 2.0f;
      if (clip) v = fminf(fmaxf(v, 1e-2f), 1.0f);
      if (v == 0.0f) v = 1.0f;
      scale[a] = v;
    }
    return;
  }
  float v = 1.0f;
  if (mode == SM_UNIT) v = (float)s.flat_sd;
  else if (mode == SM_HALF) v = (float)s.flat_sd / 0.5f;
  else if (mode == SM_34) v = (float)s.flat_sd / 0.75f;
  else if (mode == SM_BBOX) v = fmaxf(fmaxf(s.mx[0] - s.mn[0], s.mx[1] - s.mn[1]), s.mx[2] - s.mn[2]) / 2.0f;
  scale[0] = scale[1] = scale[2] = v;
}

// ---- one item ----
template <class Ctx>
__host__ __device__ void build_item(Ctx &cx, const Item &it) {
  const int N = it.N, C = it.C;
  // (a) gather; input rows start as zeros (a thread owns the same rows n = tid + k nt in every pass below)
  int bad = 0, bad_choice = 0;
  for (int n = cx.tid; n < N; n += cx.nt) {
    long long c = (long long)it.choice[n];
    if (c < 0 || c >= it.M) c = 0, bad_choice = 1;
    it.x[n] = it.pts[3 * c], it.y[n] = it.pts[3 * c + 1], it.z[n] = it.pts[3 * c + 2];
    const int32_t l = it.plab[c];
    it.lab[n] = l;
    if (l < 0 || l >= C) ++bad;
    it.input[3 * n] = it.input[3 * n + 1] = it.input[3 * n + 2] = 0.0f;
  }
  if (cx.tid == 0) it.scratch[0] = 0;
  cx.sync();
  bad = cx.sum_i(bad);
  bad_choice = cx.sum_i(bad_choice);
  if (cx.tid == 0) {
    if (bad) cx.add_status(it.status, bad);
    if (bad_choice) cx.add_status(it.status + 1, 1);
  }

  // (b) shape normalisation
  float shift[3], scale[3];
  {
    const Stats s = part_stats(cx, it, -1);
    norm_params(it.scale_mode, 0, s, shift, scale);
    if (it.scale_mode != SM_NONE)
      for (int n = cx.tid; n < N; n += cx.nt) {
        it.x[n] = (it.x[n] - shift[0]) / scale[0];
        it.y[n] = (it.y[n] - shift[1]) / scale[1];
        it.z[n] = (it.z[n] - shift[2]) / scale[2];
      }
    cx.sync();
  }

  // (c) the parts, in order, on the current labels
  for (int i = 0; i < C; ++i) {
    int cnt = 0;
    for (int n = cx.tid; n < N; n += cx.nt) cnt += it.lab[n] == i;
    cnt = cx.sum_i(cnt);
    float present = 0.0f, pshift[3] = {0.0f, 0.0f, 0.0f}, pscale[3] = {1.0f, 1.0f, 1.0f};
    if (cnt >= SMALL_PART) {
      const Stats s = part_stats(cx, it, i);
      present = (s.sd[0] == 0.0 || s.sd[1] == 0.0 || s.sd[2] == 0.0) ? 0.0f : 1.0f;
      norm_params(it.part_scale_mode, it.clip, s, pshift, pscale);
      for (int n = cx.tid; n < N; n += cx.nt) {
        if (it.lab[n] != i) continue;
        if (it.part_scale_mode == SM_NONE) {
          it.input[3 * n] = it.x[n], it.input[3 * n + 1] = it.y[n], it.input[3 * n + 2] = it.z[n];
        } else {
          it.input[3 * n] = (it.x[n] - pshift[0]) / pscale[0];
          it.input[3 * n + 1] = (it.y[n] - pshift[1]) / pscale[1];
          it.input[3 * n + 2] = (it.z[n] - pshift[2]) / pscale[2];
        }
      }
    } else if (cnt > 0) {
      // every point of the part takes the label of its nearest point outside the part; the new labels are applied together
      int *len = it.scratch, *list = it.scratch + 1, *newlab = it.scratch + 10;
      for (int n = cx.tid; n < N; n += cx.nt)
        if (it.lab[n] == i) list[cx.append(len)] = n;
      cx.sync();
      for (int k = 0; k < cnt; ++k) {
        const int p = list[k];
        const float px = it.x[p], py = it.y[p], pz = it.z[p];
        float best = INFINITY;
        int found = -1;
        for (int n = cx.tid; n < N; n += cx.nt) {
          if (it.lab[n] == i) continue;
          const float dx = px - it.x[n], dy = py - it.y[n], dz = pz - it.z[n];
          const float d = ((dx * dx) + dy * dy) + dz * dz;
          if (found < 0 || d < best) best = d, found = n;
        }
        cx.argmin(best, found);
        if (cx.tid == 0) newlab[k] = it.lab[found];   // N >= 10 > cnt: a point outside the part exists
      }
      cx.sync();
      if (cx.tid == 0) {
        for (int k = 0; k < cnt; ++k) it.lab[list[k]] = newlab[k];
        *len = 0;
      }
      cx.sync();
    }
    if (cx.tid == 0) {
      it.present[i] = present;
      it.dp_present[i] = ((double)it.drop_u[i] < it.dropout_part) ? 0.0f : present;   // (d)
      for (int a = 0; a < 3; ++a) it.part_shift[a * C + i] = pshift[a], it.part_scale[a * C + i] = pscale[a];
    }
  }

  // (e) augmentation of ref / shift / scale, (f) the remaining outputs
  float rs[3] = {1.0f, 1.0f, 1.0f}, rt[3] = {0.0f, 0.0f, 0.0f};
  const bool aug = it.aug_shift || it.aug_scale;
  for (int a = 0; a < 3; ++a) {
    if (it.aug_scale) rs[a] = it.aug_u[a] / 2.0f + 0.7f;
    if (it.aug_shift) rt[a] = it.aug_u[3 + a] - 0.5f;
  }
  for (int n = cx.tid; n < N; n += cx.nt) {
    float v[3] = {it.x[n], it.y[n], it.z[n]};
    if (aug)
      for (int a = 0; a < 3; ++a) v[a] = (v[a] + rt[a]) * rs[a];
    it.ref[3 * n] = v[0], it.ref[3 * n + 1] = v[1], it.ref[3 * n + 2] = v[2];
    it.seg[n] = (int64_t)it.lab[n];
  }
  for (int e = cx.tid; e < N * C; e += cx.nt) it.attn[e] = it.lab[e / C] == e % C ? 1 : 0;
  if (cx.tid == 0)
    for (int a = 0; a < 3; ++a) {
      it.shift[a] = aug ? shift[a] + scale[a] * rt[a] : shift[a];
      it.scale[a] = aug ? rs[a] * scale[a] : scale[a];
    }
}

struct BuildArgs {
  const float *points;
  const int32_t *labels;
  const int64_t *offsets, *index;
  int S;
  const int32_t *choice;
  const float *drop_u, *aug_u;
  int N, C, scale_mode, part_scale_mode, clip, aug_shift, aug_scale;
  double dropout_part;
  float *ref, *input;
  int64_t *seg, *attn;
  float *present, *dp_present, *part_shift, *part_scale, *shift, *scale;
  int32_t *status;
};

// the item of batch row b; false (and status[1] counted by the caller) when its index or cloud is unusable
__host__ __device__ inline bool make_item(const BuildArgs &a, int b, Item *it) {
  const long long s = (long long)a.index[b];
  if (s < 0 || s >= a.S) return false;
  const long long off = (long long)a.offsets[s], M = (long long)a.offsets[s + 1] - off;
  if (off < 0 || M <= 0) return false;
  const size_t N = (size_t)a.N, C = (size_t)a.C;
  it->pts = a.points + 3 * off, it->plab = a.labels + off, it->M = M;
  it->choice = a.choice + b * N, it->drop_u = a.drop_u + b * C, it->aug_u = a.aug_u + (size_t)b * 6;
  it->N = a.N, it->C = a.C, it->scale_mode = a.scale_mode, it->part_scale_mode = a.part_scale_mode, it->clip = a.clip;
  it->aug_shift = a.aug_shift, it->aug_scale = a.aug_scale, it->dropout_part = a.dropout_part;
  it->ref = a.ref + b * N * 3, it->input = a.input + b * N * 3, it->seg = a.seg + b * N, it->attn = a.attn + b * N * C;
  it->present = a.present + b * C, it->dp_present = a.dp_present + b * C;
  it->part_shift = a.part_shift + b * 3 * C, it->part_scale = a.part_scale + b * 3 * C;
  it->shift = a.shift + (size_t)b * 3, it->scale = a.scale + (size_t)b * 3;
  it->status = a.status;
  return true;
}

__global__ void __launch_bounds__(NT) k_batch_build(BuildArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red_d[NW * 4];
  __shared__ float red_f[NW * 6];
  __shared__ int red_i[NW * 2];
  __shared__ int scratch[20];
  Item it;
  if (!make_item(a, blockIdx.x, &it)) {   // uniform over the workgroup
    if (threadIdx.x == 0) atomicAdd(a.status + 1, 1);
    return;
  }
  it.x = reinterpret_cast<float *>(smem);
  it.y = it.x + a.N;
  it.z = it.y + a.N;
  it.lab = reinterpret_cast<int32_t *>(it.z + a.N);
  it.scratch = scratch;
  BlockCtx cx{(int)threadIdx.x, NT, red_d, red_f, red_i};
  build_item(cx, it);
}

// ---- draws: Philox4x32-7 (dfx_dropout.h), key = seed, counter = (group of four values, purpose, sample_id lo, sample_id hi) ----
// choice = (word * M) >> 32, unit floats = (word >> 8) 2^-24; value i of an item is word i & 3 of group i >> 2.  DESIGN.md "Random streams" lists the
// layout; tests/test_gpu_random_streams.py holds the draws to oracle/philox.py bit for bit.
constexpr unsigned DRAW_CHOICE = 0xBA7C0u, DRAW_DROP = 0xBA7C1u, DRAW_AUG = 0xBA7C2u;
__device__ __forceinline__ float unit_float(unsigned w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }   // 24 bits: [0,1)

__global__ void __launch_bounds__(NT) k_batch_draw(const int64_t *__restrict__ offsets, int S, const int64_t *__restrict__ index,
                                                   const int64_t *__restrict__ sample_id, int N, int C, unsigned long long seed,
                                                   int32_t *__restrict__ choice, float *__restrict__ drop_u, float *__restrict__ aug_u) {
  const int b = blockIdx.x;   // B can exceed the 65535 of grid.y; the groups of four values (at most 8 blocks) go there
  const unsigned long long id = (unsigned long long)sample_id[b];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), id0 = (unsigned)id, id1 = (unsigned)(id >> 32);
  const long long s = (long long)index[b];
  unsigned long long M = 0;
  if (s >= 0 && s < S) {
    const long long m = (long long)offsets[s + 1] - (long long)offsets[s];
    if (m > 0) M = (unsigned long long)m;   // else every choice is 0 and dfx_batch_build_f32 reports the item
  }
  const int g = blockIdx.y * NT + threadIdx.x;
  if (4 * g < N) {
    const uint4 r = dfx::philox4x32_7((unsigned)g, DRAW_CHOICE, id0, id1, k0, k1);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
    for (int e = 0; e < 4 && 4 * g + e < N; ++e) choice[(size_t)b * N + 4 * g + e] = (int32_t)(((unsigned long long)w[e] * M) >> 32);
  }
  if (blockIdx.y == 0 && threadIdx.x < 4) {
    const int t = threadIdx.x, grp = t & 1;
    const bool drop = t < 2;
    const uint4 r = dfx::philox4x32_7((unsigned)grp, drop ? DRAW_DROP : DRAW_AUG, id0, id1, k0, k1);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
    const int len = drop ? C : 6;
    float *out = drop ? drop_u + (size_t)b * C : aug_u + (size_t)b * 6;
    for (int e = 0; e < 4 && 4 * grp + e < len; ++e) out[4 * grp + e] = unit_float(w[e]);
  }
}

int check_config(const char *who, int S, int B, int C, int N, int scale_mode, int part_scale_mode) {
  DFX_REQUIRE(S > 0 && B > 0, "%s: S = %d, B = %d must be positive", who, S, B);
  DFX_REQUIRE(C >= 1 && C <= BATCH_MAX_C, "%s: n_class = %d outside [1,%d]", who, C, BATCH_MAX_C);
  DFX_REQUIRE(N >= BATCH_MIN_N && N <= BATCH_MAX_N, "%s: npoints = %d outside [%d,%d]", who, N, BATCH_MIN_N, BATCH_MAX_N);
  DFX_REQUIRE(scale_mode >= SM_NONE && scale_mode <= SM_BBOX, "%s: scale_mode = %d is not one of none, shape_unit, shape_half, shape_34, shape_bbox",
              who, scale_mode);
  DFX_REQUIRE(part_scale_mode >= SM_NONE && part_scale_mode <= SM_CANONICAL_BBOX, "%s: part_scale_mode = %d unknown", who, part_scale_mode);
  return DFX_OK;
}

dfx::PerDeviceOnce g_build_lds;

}  // namespace

extern "C" {

int dfx_batch_draw(const int64_t *offsets, int S, const int64_t *index, const int64_t *sample_id, int B, int N, int C, uint64_t seed,
                   int32_t *choice, float *drop_u, float *aug_u, dfx_stream_t stream) {
  DFX_REQUIRE(offsets && index && sample_id && choice && drop_u && aug_u, "batch_draw: null pointer");
  if (int rc = check_config("batch_draw", S, B, C, N, SM_UNIT, SM_CANONICAL)) return rc;
  const dim3 grid((unsigned)B, (unsigned)(((N + 3) / 4 + NT - 1) / NT));
  k_batch_draw<<<grid, NT, 0, dfx::as_stream(stream)>>>(offsets, S, index, sample_id, N, C, (unsigned long long)seed, choice, drop_u, aug_u);
  return dfx::check_launch("batch_draw");
}

int dfx_batch_build_f32(const float *points, const int32_t *labels, const int64_t *offsets, int S, const int64_t *index, int B,
                        const int32_t *choice, const float *drop_u, const float *aug_u, int n_class, int npoints, int scale_mode,
                        int part_scale_mode, int clip, double dropout_part, int augment_shift, int augment_scale, float *ref,
                        float *input, int64_t *seg, int64_t *attn_map, float *present, float *dp_present, float *part_shift,
                        float *part_scale, float *shift, float *scale, int32_t *n_bad, dfx_stream_t stream) {
  DFX_REQUIRE(points && labels && offsets && index && choice && drop_u && aug_u, "batch_build: null input pointer");
  DFX_REQUIRE(ref && input && seg && attn_map && present && dp_present && part_shift && part_scale && shift && scale && n_bad,
              "batch_build: null output pointer");
  if (int rc = check_config("batch_build", S, B, n_class, npoints, scale_mode, part_scale_mode)) return rc;
  hipStream_t st = dfx::as_stream(stream);
  const int lds = npoints * 16;
  if (lds > 48 * 1024)
    DFX_HIP_TRY(g_build_lds.run([] { return dfx::set_max_lds(reinterpret_cast<const void *>(k_batch_build), BATCH_MAX_N * 16); }));
  DFX_HIP_TRY(hipMemsetAsync(n_bad, 0, 2 * sizeof(int32_t), st));
  const BuildArgs a{points, labels, offsets, index, S, choice, drop_u, aug_u, npoints, n_class, scale_mode, part_scale_mode, clip != 0,
                    augment_shift != 0, augment_scale != 0, dropout_part, ref, input, seg, attn_map, present, dp_present, part_shift,
                    part_scale, shift, scale, n_bad};
  k_batch_build<<<B, NT, lds, st>>>(a);
  return dfx::check_launch("batch_build");
}

int dfx_debug_batch_build_host(const float *points, const int32_t *labels, const int64_t *offsets, int S, const int64_t *index, int B,
                               const int32_t *choice, const float *drop_u, const float *aug_u, int n_class, int npoints, int scale_mode,
                               int part_scale_mode, int clip, double dropout_part, int augment_shift, int augment_scale, float *ref,
                               float *input, int64_t *seg, int64_t *attn_map, float *present, float *dp_present, float *part_shift,
                               float *part_scale, float *shift, float *scale, int32_t *n_bad) {
  DFX_REQUIRE(points && labels && offsets && index && choice && drop_u && aug_u, "debug_batch_build_host: null input pointer");
  DFX_REQUIRE(ref && input && seg && attn_map && present && dp_present && part_shift && part_scale && shift && scale && n_bad,
              "debug_batch_build_host: null output pointer");
  if (int rc = check_config("debug_batch_build_host", S, B, n_class, npoints, scale_mode, part_scale_mode)) return rc;
  for (int b = 0; b < B; ++b) {
    const long long s = (long long)index[b];
    DFX_REQUIRE(s >= 0 && s < S, "debug_batch_build_host: index[%d] = %lld outside [0,%d)", b, s, S);
    DFX_REQUIRE(offsets[s + 1] > offsets[s] && offsets[s] >= 0, "debug_batch_build_host: cloud %lld is empty", s);
  }
  const BuildArgs a{points, labels, offsets, index, S, choice, drop_u, aug_u, npoints, n_class, scale_mode, part_scale_mode, clip != 0,
                    augment_shift != 0, augment_scale != 0, dropout_part, ref, input, seg, attn_map, present, dp_present, part_shift,
                    part_scale, shift, scale, n_bad};
  n_bad[0] = n_bad[1] = 0;
  std::vector<float> xyz((size_t)npoints * 3);
  std::vector<int32_t> lab((size_t)npoints);
  int scratch[20];
  for (int b = 0; b < B; ++b) {
    Item it;
    if (!make_item(a, b, &it)) return dfx::set_error(DFX_ERR_INVALID_ARG, "debug_batch_build_host: item %d", b);
    it.x = xyz.data(), it.y = it.x + npoints, it.z = it.y + npoints, it.lab = lab.data(), it.scratch = scratch;
    SerialCtx cx;
    build_item(cx, it);
  }
  return DFX_OK;
}

}  // extern "C"
