// Part-level generation metrics for gfx950: snapping, part boxes, part clouds, box-set distance matrices (include/dfx.h).
//
// Semantics of python/difffacto/datasets/evaluation_utils.py (compute_snapping_metric :385-421, compute_bbox_metric :287-333 with
// part_chamfer / part_l2 / part_miou :23-82, compute_part_metric :423-486), restated in DESIGN.md "Part-level metrics".
// Mapping: one 256-thread workgroup per (shape, pair) / (shape, part) / box pair.  Parts are compacted in index order with a
// ballot + prefix popcount per 64-lane wave; nearest-neighbour scans run from LDS tiles of 16-byte records (broadcast reads, as
// chamfer_kernels.hip); order statistics come from a bitwise radix select (snapping) or an LDS bitonic sort (quantiles).
#include "dfx_common.h"

#include <cmath>

namespace {

constexpr int NT = 256, WAVE = 64, NWAVE = NT / WAVE;
constexpr int PM_MAX_N = 8192;     // uint16 point ids in LDS
constexpr int PM_MAX_PAIRS = 64;
constexpr int PM_TILE = 1024;      // float4 records per LDS tile (16 KiB)
constexpr int BOX_PTS = 512;       // points drawn per box (part_chamfer, :32-33)

struct PairList {
  int a[PM_MAX_PAIRS], b[PM_MAX_PAIRS];
};

// (dx*dx + dy*dy) + dz*dz, each operation rounded: torch's CPU ((A[:,None]-B[None])**2).sum(-1)
__device__ __forceinline__ float sqd_plain(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
// mul, fma, fma (chamfer_kernels.hip's evaluation order; the box Chamfer has no bit-level reference to follow)
__device__ __forceinline__ float sqd_fma(float dx, float dy, float dz) {
  return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Block-wide reductions through NWAVE slots of LDS (every thread gets the result).
__device__ float block_sum(float v, float *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ int block_sum_i(int v, int *red) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ float block_min(float v, float *red) {
  v = wave_min(v);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}
__device__ float block_max(float v, float *red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// Index-order compaction of [0,n): write(pos, i) for every i with flag(i), pos = number of flagged indices before i.  All flags of
// a 256-index chunk are evaluated before any write of that chunk, and a chunk's writes land below the next chunk's first index, so
// an in-place compaction of an LDS array is safe.  Returns the count.
template <class Flag, class Write>
__device__ int block_compact(int n, Flag flag, Write write, int *wcnt) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  int total = 0;
  for (int base = 0; base < n; base += NT) {
    const int i = base + threadIdx.x;
    int val = 0;
    const bool f = i < n && flag(i, val);
    const unsigned long long m = __ballot(f);
    __syncthreads();
    if (lane == 0) wcnt[w] = __popcll(m);
    __syncthreads();
    int off = total;
    for (int v = 0; v < w; ++v) off += wcnt[v];
    if (f) write(off + __popcll(m & ((1ull << lane) - 1ull)), i, val);
    total += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  }
  __syncthreads();
  return total;
}

// For every query q < nq (point X[qi[q]]) the minimum plain squared distance to the targets X[ti[t]], t < nt: out(q, min).
// Two queries per thread; targets stream through the LDS tile.  nt >= 1.
template <class Out>
__device__ void nn_scan(const float *__restrict__ X, const uint16_t *qi, int nq, const uint16_t *ti, int nt, float4 *tile, Out out) {
  for (int q0 = 0; q0 < nq; q0 += 2 * NT) {
    const int qa = q0 + threadIdx.x, qb = qa + NT;
    const int pa = qi[min(qa, nq - 1)], pb = qi[min(qb, nq - 1)];
    const float ax = X[pa * 3], ay = X[pa * 3 + 1], az = X[pa * 3 + 2];
    const float bx = X[pb * 3], by = X[pb * 3 + 1], bz = X[pb * 3 + 2];
    float ma = INFINITY, mb = INFINITY;
    for (int t0 = 0; t0 < nt; t0 += PM_TILE) {
      const int cnt = min(PM_TILE, nt - t0);
      __syncthreads();
      for (int t = threadIdx.x; t < cnt; t += NT) {
        const int p = ti[t0 + t];
        tile[t] = make_float4(X[p * 3], X[p * 3 + 1], X[p * 3 + 2], 0.f);
      }
      __syncthreads();
#pragma unroll 4
      for (int t = 0; t < cnt; ++t) {
        const float4 r = tile[t];
        ma = fminf(ma, sqd_plain(ax, ay, az, r.x, r.y, r.z));
        mb = fminf(mb, sqd_plain(bx, by, bz, r.x, r.y, r.z));
      }
    }
    if (qa < nq) out(qa, ma);
    if (qb < nq) out(qb, mb);
  }
  __syncthreads();
}

// 45-bit selection key: the bits of a minimum (>= +0: integer order = value order) above the 13-bit point id (ties: lower id first)
__device__ __forceinline__ unsigned long long sel_key(const float *m, int t) {
  return ((unsigned long long)__float_as_uint(m[t]) << 13) | (unsigned)t;
}
// The k-th smallest key of m[0..n) (1 <= k <= n), bit by bit from the top: bit b of the answer is 0 iff at least k keys lie at or
// below the largest key with the bits found so far and bit b clear.
__device__ unsigned long long kth_key(const float *m, int n, int k, int *red) {
  unsigned long long P = 0;
  for (int b = 44; b >= 0; --b) {
    const unsigned long long cand = P | ((1ull << b) - 1ull);
    int c = 0;
    for (int t = threadIdx.x; t < n; t += NT) c += sel_key(m, t) <= cand;
    if (block_sum_i(c, red) < k) P |= 1ull << b;
  }
  return P;
}

// ---- snapping: one workgroup per (shape, pair) ----
// LDS: ia, ib (uint16 N): the parts' point ids in index order, later the kept ids; ma, mb (fp32 N): nearest distances; tile.
__global__ void __launch_bounds__(NT) k_snapping(const float *__restrict__ xyz, const int32_t *__restrict__ lab, PairList pl, int N,
                                                 int P, int k, float *__restrict__ dist, int32_t *__restrict__ status) {
  extern __shared__ __align__(16) unsigned char smem[];
  float4 *tile = reinterpret_cast<float4 *>(smem);
  float *ma = reinterpret_cast<float *>(tile + PM_TILE), *mb = ma + N;
  uint16_t *ia = reinterpret_cast<uint16_t *>(mb + N), *ib = ia + N;
  __shared__ int red[NWAVE];
  __shared__ float redf[NWAVE];
  const int b = blockIdx.x / P, pr = blockIdx.x % P;
  const int pa = pl.a[pr], pb = pl.b[pr];
  const float *X = xyz + (size_t)b * N * 3;
  const int32_t *L = lab + (size_t)b * N;
  const int na = block_compact(
      N, [&](int i, int &) { return L[i] == pa; }, [&](int pos, int i, int) { ia[pos] = (uint16_t)i; }, red);
  const int nb = block_compact(
      N, [&](int i, int &) { return L[i] == pb; }, [&](int pos, int i, int) { ib[pos] = (uint16_t)i; }, red);
  const size_t o = (size_t)b * P + pr;
  if (na == 0 || nb == 0 || na < k || nb < k) {
    if (threadIdx.x == 0) dist[o] = NAN, status[o] = (na == 0 || nb == 0) ? 0 : 2;
    return;
  }
  nn_scan(X, ia, na, ib, nb, tile, [&](int q, float v) { ma[q] = v; });
  nn_scan(X, ib, nb, ia, na, tile, [&](int q, float v) { mb[q] = v; });
  // keep the k smallest of each side (in index order, in place)
  const unsigned long long KA = kth_key(ma, na, k, red), KB = kth_key(mb, nb, k, red);
  block_compact(
      na, [&](int i, int &v) { v = ia[i]; return sel_key(ma, i) <= KA; }, [&](int pos, int, int v) { ia[pos] = (uint16_t)v; }, red);
  block_compact(
      nb, [&](int i, int &v) { v = ib[i]; return sel_key(mb, i) <= KB; }, [&](int pos, int, int v) { ib[pos] = (uint16_t)v; }, red);
  // Chamfer of the two k-point sets
  float sa = 0.f, sb = 0.f;
  nn_scan(X, ia, k, ib, k, tile, [&](int, float v) { sa += v; });
  nn_scan(X, ib, k, ia, k, tile, [&](int, float v) { sb += v; });
  sa = block_sum(sa, redf);
  sb = block_sum(sb, redf);
  if (threadIdx.x == 0) dist[o] = sa / (float)k + sb / (float)k, status[o] = 1;
}

// ---- part boxes: one workgroup per (shape, part), one axis at a time through an LDS bitonic sort ----
__device__ __forceinline__ float quantile_sorted(const float *s, int n, float q) {
  // torch.quantile, linear: rank = q (n-1) in fp32, lerp(s[floor], s[ceil], rank - floor) as torch's vectorised lerp evaluates it
  const float rank = __fmul_rn(q, (float)(n - 1));
  const int lo = (int)rank, hi = min((int)ceilf(rank), n - 1);
  const float w = __fsub_rn(rank, (float)lo);
  const float a = s[lo], c = s[hi], d = __fsub_rn(c, a);
  return fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(__fsub_rn(w, 1.0f), d, c);
}

__device__ void bitonic_sort(float *v, int n2) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < n2 / 2; t += NT) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const float x = v[i], y = v[j];
        if ((x > y) == up) v[i] = y, v[j] = x;
      }
    }
  }
  __syncthreads();
}

struct ShapeNorm {
  float sx, sy, sz, scale;
};

// whole-shape normalisation (compute_bbox_metric :297-301): shift = (min + max) / 2, scale = largest extent / 2
__device__ ShapeNorm shape_norm(const float *X, int N, float *redf) {
  float lo[3], hi[3];
  for (int c = 0; c < 3; ++c) lo[c] = INFINITY, hi[c] = -INFINITY;
  for (int i = threadIdx.x; i < N; i += NT)
    for (int c = 0; c < 3; ++c) lo[c] = fminf(lo[c], X[i * 3 + c]), hi[c] = fmaxf(hi[c], X[i * 3 + c]);
  for (int c = 0; c < 3; ++c) lo[c] = block_min(lo[c], redf), hi[c] = block_max(hi[c], redf);
  const float e = fmaxf(fmaxf(__fsub_rn(hi[0], lo[0]), __fsub_rn(hi[1], lo[1])), __fsub_rn(hi[2], lo[2]));
  return ShapeNorm{__fadd_rn(lo[0], hi[0]) * 0.5f, __fadd_rn(lo[1], hi[1]) * 0.5f, __fadd_rn(lo[2], hi[2]) * 0.5f, e * 0.5f};
}

__global__ void __launch_bounds__(NT) k_boxes(const float *__restrict__ xyz, const int32_t *__restrict__ lab, int N, int C, int normalize,
                                              int min_points, float qlo, float qhi, float *__restrict__ boxes,
                                              int32_t *__restrict__ count) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *v = reinterpret_cast<float *>(smem);
  __shared__ float redf[NWAVE];
  __shared__ int cnt;
  const int b = blockIdx.x / C, j = blockIdx.x % C;
  const float *X = xyz + (size_t)b * N * 3;
  const int32_t *L = lab + (size_t)b * N;
  float *out = boxes + ((size_t)b * C + j) * 6;
  ShapeNorm sn{0.f, 0.f, 0.f, 1.f};
  if (normalize) sn = shape_norm(X, N, redf);
  const float shift[3] = {sn.sx, sn.sy, sn.sz};
  for (int c = 0; c < 3; ++c) {
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += NT) {
      if (L[i] != j) continue;
      const float x = X[i * 3 + c];
      v[atomicAdd(&cnt, 1)] = normalize ? __fdiv_rn(__fsub_rn(x, shift[c]), sn.scale) : x;   // any order: sorted below
    }
    __syncthreads();
    const int n = cnt;
    if (n <= min_points) {
      if (threadIdx.x == 0) count[(size_t)b * C + j] = n;
      if (threadIdx.x < 6) out[threadIdx.x] = NAN;
      return;
    }
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + threadIdx.x; i < n2; i += NT) v[i] = INFINITY;
    bitonic_sort(v, n2);
    if (threadIdx.x == 0) {
      out[c] = quantile_sorted(v, n, qlo);
      out[3 + c] = quantile_sorted(v, n, qhi);
      if (c == 0) count[(size_t)b * C + j] = n;
    }
    __syncthreads();
  }
}

// ---- part clouds: one workgroup per (shape, part) ----
__global__ void __launch_bounds__(NT) k_clouds(const float *__restrict__ xyz, const int32_t *__restrict__ lab, int N, int C, int min_points,
                                               int n_out, float *__restrict__ clouds, float *__restrict__ masks,
                                               int32_t *__restrict__ count) {
  extern __shared__ __align__(16) unsigned char smem[];
  float4 *cl = reinterpret_cast<float4 *>(smem);
  __shared__ int red[NWAVE];
  __shared__ float redf[NWAVE];
  const int b = blockIdx.x / C, j = blockIdx.x % C;
  const float *X = xyz + (size_t)b * N * 3;
  const int32_t *L = lab + (size_t)b * N;
  float *co = clouds + ((size_t)b * C + j) * n_out * 3;
  float *mo = masks + ((size_t)b * C + j) * n_out;
  const int n = block_compact(
      N, [&](int i, int &) { return L[i] == j; },
      [&](int pos, int i, int) {
        if (pos < n_out) cl[pos] = make_float4(X[i * 3], X[i * 3 + 1], X[i * 3 + 2], 0.f);
      },
      red);
  if (threadIdx.x == 0) count[(size_t)b * C + j] = n;
  if (n <= min_points) {
    for (int p = threadIdx.x; p < n_out; p += NT) co[p * 3] = co[p * 3 + 1] = co[p * 3 + 2] = 0.f, mo[p] = 0.f;
    return;
  }
  const int m = min(n, n_out);
  float lo[3], hi[3];
  for (int c = 0; c < 3; ++c) lo[c] = INFINITY, hi[c] = -INFINITY;
  for (int p = threadIdx.x; p < m; p += NT) {
    const float4 q = cl[p];
    lo[0] = fminf(lo[0], q.x), lo[1] = fminf(lo[1], q.y), lo[2] = fminf(lo[2], q.z);
    hi[0] = fmaxf(hi[0], q.x), hi[1] = fmaxf(hi[1], q.y), hi[2] = fmaxf(hi[2], q.z);
  }
  float sh[3], sc[3];
  for (int c = 0; c < 3; ++c) {
    lo[c] = block_min(lo[c], redf), hi[c] = block_max(hi[c], redf);
    sh[c] = __fadd_rn(lo[c], hi[c]) * 0.5f, sc[c] = __fsub_rn(hi[c], lo[c]) * 0.5f;
  }
  for (int p = threadIdx.x; p < n_out; p += NT) {
    const float4 q = cl[p % n];
    co[p * 3] = __fdiv_rn(__fsub_rn(q.x, sh[0]), sc[0]);
    co[p * 3 + 1] = __fdiv_rn(__fsub_rn(q.y, sh[1]), sc[1]);
    co[p * 3 + 2] = __fdiv_rn(__fsub_rn(q.z, sh[2]), sc[2]);
    mo[p] = p < n ? 1.f : 0.f;
  }
}

// ---- box-set distances ----
__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}
// unit draw in [0,1) with 24 random bits, as torch.rand's float32
__device__ __forceinline__ float unit24(unsigned w) { return (float)(w >> 8) * 0x1p-24f; }

// Counter = (point, DRAW_BOX | class * 2 + side, pair lo, pair hi), key = seed; words 0..2 are used, word 3 is discarded (DESIGN.md "Random
// streams").  The tag keeps this layout apart from the chain noise's (gid lo, gid hi, t, stream), the other Philox4x32-10 stream: without it
// (p, 0, pair, 0) was the chain's counter of point p at t = pair under the same seed.
constexpr unsigned DRAW_BOX = 0xB0C50000u;
__device__ __forceinline__ float3 box_unit(unsigned long long seed, unsigned long long gpair, int c, int side, int p) {
  const uint4 r = philox4x32_10((unsigned)p, DRAW_BOX | (unsigned)(c * 2 + side), (unsigned)gpair, (unsigned)(gpair >> 32), (unsigned)seed,
                                (unsigned)(seed >> 32));
  return make_float3(unit24(r.x), unit24(r.y), unit24(r.z));
}

// l2 / iou: one thread per pair
__global__ void __launch_bounds__(NT) k_box_pair(const float *__restrict__ ba, const int32_t *__restrict__ pa, const float *__restrict__ bb,
                                                 const int32_t *__restrict__ pb, int Ma, int Mb, int C, int metric, float *__restrict__ D) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= (long long)Ma * Mb) return;
  const int i = (int)(t / Mb), j = (int)(t % Mb);
  float sf = 0.f;
  double sd = 0.0;
  int terms = 0;
  for (int c = 0; c < C; ++c) {
    const bool ha = pa[(size_t)i * C + c] != 0, hb = pb[(size_t)j * C + c] != 0;
    if (ha != hb) {
      D[t] = INFINITY;
      return;
    }
    if (!ha) continue;
    const float *A = ba + ((size_t)i * C + c) * 6, *B = bb + ((size_t)j * C + c) * 6;
    if (metric == 0) {   // part_l2 (:42-62): mse of [scale, shift]
      float s = 0.f;
      for (int h = 0; h < 2; ++h)
        for (int a = 0; a < 3; ++a) {
          const float va = h == 0 ? __fsub_rn(A[3 + a], A[a]) * 0.5f : __fadd_rn(A[3 + a], A[a]) * 0.5f;
          const float vb = h == 0 ? __fsub_rn(B[3 + a], B[a]) * 0.5f : __fadd_rn(B[3 + a], B[a]) * 0.5f;
          const float d = __fsub_rn(va, vb);
          s = __fadd_rn(s, __fmul_rn(d, d));
        }
      sf = __fadd_rn(sf, s / 6.0f);
    } else {   // part_miou (:64-82): get_3d_box reads (dx,dy,dz) as (l,w,h): x-extent dx, y-extent dz, z-extent dy
      double lo_a[3], hi_a[3], lo_b[3], hi_b[3], ea[3], eb[3];
      for (int a = 0; a < 3; ++a) {
        ea[a] = (double)__fsub_rn(A[3 + a], A[a]), eb[a] = (double)__fsub_rn(B[3 + a], B[a]);
      }
      const int ext[3] = {0, 2, 1};   // extent used along x, y, z
      for (int a = 0; a < 3; ++a) {
        const double ca = (double)(__fadd_rn(A[3 + a], A[a]) * 0.5f), cb = (double)(__fadd_rn(B[3 + a], B[a]) * 0.5f);
        const double ha2 = (double)((float)ea[ext[a]] * 0.5f), hb2 = (double)((float)eb[ext[a]] * 0.5f);
        lo_a[a] = ca - ha2, hi_a[a] = ca + ha2, lo_b[a] = cb - hb2, hi_b[a] = cb + hb2;
      }
      double inter = 1.0;
      for (int a = 0; a < 3; ++a) inter *= fmax(0.0, fmin(hi_a[a], hi_b[a]) - fmax(lo_a[a], lo_b[a]));
      const double va = ea[0] * ea[1] * ea[2], vb = eb[0] * eb[1] * eb[2];
      sd += inter / (va + vb - inter);
    }
    ++terms;
  }
  if (terms == 0) D[t] = NAN;
  else D[t] = metric == 0 ? sf / (float)terms : (float)(1.0 - sd / (double)terms);
}

// chamfer: one workgroup per pair, the classes in order; 512 + 512 points in LDS, two queries per thread per direction
__global__ void __launch_bounds__(NT) k_box_chamfer(const float *__restrict__ ba, const int32_t *__restrict__ pa, const float *__restrict__ bb,
                                                    const int32_t *__restrict__ pb, int Mb, int C, unsigned long long seed,
                                                    long long row0, const float *__restrict__ units, float *__restrict__ D) {
  __shared__ float4 pts[2 * BOX_PTS];
  __shared__ float redf[NWAVE];
  const long long t = blockIdx.x;
  const int i = (int)(t / Mb), j = (int)(t % Mb);
  const unsigned long long gpair = (unsigned long long)(row0 + i) * Mb + j;
  float s = 0.f;
  int terms = 0;
  for (int c = 0; c < C; ++c) {
    const bool ha = pa[(size_t)i * C + c] != 0, hb = pb[(size_t)j * C + c] != 0;
    if (ha != hb) {
      if (threadIdx.x == 0) D[t] = INFINITY;
      return;
    }
    if (!ha) continue;
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * BOX_PTS; e += NT) {
      const int side = e / BOX_PTS, p = e % BOX_PTS;
      const float *bx = (side == 0 ? ba + ((size_t)i * C + c) * 6 : bb + ((size_t)j * C + c) * 6);
      float3 u;
      if (units) {
        const float *up = units + ((((size_t)t * C + c) * 2 + side) * BOX_PTS + p) * 3;
        u = make_float3(up[0], up[1], up[2]);
      } else {
        u = box_unit(seed, gpair, c, side, p);
      }
      // u * (hi - lo) + lo, two roundings (torch.rand(...) * (hi - lo) + lo)
      pts[e] = make_float4(__fadd_rn(__fmul_rn(u.x, __fsub_rn(bx[3], bx[0])), bx[0]),
                           __fadd_rn(__fmul_rn(u.y, __fsub_rn(bx[4], bx[1])), bx[1]),
                           __fadd_rn(__fmul_rn(u.z, __fsub_rn(bx[5], bx[2])), bx[2]), 0.f);
    }
    __syncthreads();
    float sum[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const float4 q0 = pts[side * BOX_PTS + threadIdx.x], q1 = pts[side * BOX_PTS + threadIdx.x + NT];
      const float4 *R = pts + (1 - side) * BOX_PTS;
      float m0 = INFINITY, m1 = INFINITY;
#pragma unroll 8
      for (int r = 0; r < BOX_PTS; ++r) {
        const float4 x = R[r];
        m0 = fminf(m0, sqd_fma(x.x - q0.x, x.y - q0.y, x.z - q0.z));
        m1 = fminf(m1, sqd_fma(x.x - q1.x, x.y - q1.y, x.z - q1.z));
      }
      sum[side] = m0 + m1;
    }
    const float sa = block_sum(sum[0], redf), sb = block_sum(sum[1], redf);
    s = __fadd_rn(s, sa / (float)BOX_PTS + sb / (float)BOX_PTS);
    ++terms;
  }
  if (threadIdx.x == 0) D[t] = terms ? s / (float)terms : NAN;
}

__global__ void __launch_bounds__(NT) k_box_units(unsigned long long seed, long long pair0, long long total, int C, float *__restrict__ units) {
  const long long e = (long long)blockIdx.x * NT + threadIdx.x;   // (pair, class, side, point)
  if (e >= total) return;
  const int p = (int)(e % BOX_PTS), side = (int)((e / BOX_PTS) % 2), c = (int)((e / (2 * BOX_PTS)) % C);
  const long long pr = e / (2LL * BOX_PTS * C);
  const float3 u = box_unit(seed, (unsigned long long)(pair0 + pr), c, side, p);
  units[e * 3] = u.x, units[e * 3 + 1] = u.y, units[e * 3 + 2] = u.z;
}

int check_cloud_args(const char *what, const float *xyz, const int32_t *labels, int B, int N, int C) {
  DFX_REQUIRE(xyz && labels, "%s: null pointer", what);
  DFX_REQUIRE(B > 0 && N > 0 && C > 0, "%s: B = %d, N = %d, C = %d must be positive", what, B, N, C);
  DFX_REQUIRE(N <= PM_MAX_N, "%s: N = %d above %d", what, N, PM_MAX_N);
  return DFX_OK;
}

int grid_of(long long n) { return (int)((n + NT - 1) / NT); }

}  // namespace

extern "C" {

int dfx_part_snapping_f32(const float *xyz, const int32_t *labels, int B, int N, int C, const int32_t *pairs, int P, int k,
                          float *dist, int32_t *status, dfx_stream_t stream) {
  if (int rc = check_cloud_args("part_snapping", xyz, labels, B, N, C)) return rc;
  DFX_REQUIRE(pairs && dist && status, "part_snapping: null pointer");
  DFX_REQUIRE(P > 0 && P <= PM_MAX_PAIRS, "part_snapping: P = %d not in [1,%d]", P, PM_MAX_PAIRS);
  DFX_REQUIRE(k > 0, "part_snapping: k = %d must be positive", k);
  PairList pl{};
  for (int p = 0; p < P; ++p) {
    for (int s = 0; s < 2; ++s)
      DFX_REQUIRE(pairs[2 * p + s] >= 0 && pairs[2 * p + s] < C, "part_snapping: pair %d names part %d outside [0,%d)", p,
                  pairs[2 * p + s], C);
    pl.a[p] = pairs[2 * p], pl.b[p] = pairs[2 * p + 1];
  }
  const int lds = PM_TILE * 16 + N * 12;
  static dfx::PerDeviceOnce attrs;
  DFX_HIP_TRY(attrs.run([] { return dfx::set_max_lds(reinterpret_cast<const void *>(k_snapping), PM_TILE * 16 + PM_MAX_N * 12); }));
  k_snapping<<<B * P, NT, lds, dfx::as_stream(stream)>>>(xyz, labels, pl, N, P, k, dist, status);
  return dfx::check_launch("part_snapping");
}

int dfx_part_boxes_f32(const float *xyz, const int32_t *labels, int B, int N, int C, int normalize, int min_points, double q,
                       float *boxes, int32_t *count, dfx_stream_t stream) {
  if (int rc = check_cloud_args("part_boxes", xyz, labels, B, N, C)) return rc;
  DFX_REQUIRE(boxes && count, "part_boxes: null pointer");
  DFX_REQUIRE(q >= 0.0 && q <= 1.0, "part_boxes: q = %g outside [0,1]", q);
  DFX_REQUIRE(min_points >= 0, "part_boxes: min_points = %d is negative", min_points);
  int n2 = 1;
  while (n2 < N) n2 <<= 1;
  k_boxes<<<B * C, NT, n2 * 4, dfx::as_stream(stream)>>>(xyz, labels, N, C, normalize, min_points, (float)(1.0 - q), (float)q, boxes,
                                                        count);
  return dfx::check_launch("part_boxes");
}

int dfx_part_clouds_f32(const float *xyz, const int32_t *labels, int B, int N, int C, int min_points, int n_out, float *clouds,
                        float *masks, int32_t *count, dfx_stream_t stream) {
  if (int rc = check_cloud_args("part_clouds", xyz, labels, B, N, C)) return rc;
  DFX_REQUIRE(clouds && masks && count, "part_clouds: null pointer");
  DFX_REQUIRE(n_out > 0 && n_out <= 4096, "part_clouds: n_out = %d not in [1,4096]", n_out);
  DFX_REQUIRE(min_points >= 0, "part_clouds: min_points = %d is negative", min_points);
  k_clouds<<<B * C, NT, n_out * 16, dfx::as_stream(stream)>>>(xyz, labels, N, C, min_points, n_out, clouds, masks, count);
  return dfx::check_launch("part_clouds");
}

int dfx_part_box_pairwise_f32(const float *boxes_a, const int32_t *present_a, int Ma, const float *boxes_b,
                              const int32_t *present_b, int Mb, int C, int metric, uint64_t seed, long long row0,
                              const float *units, float *D, dfx_stream_t stream) {
  DFX_REQUIRE(boxes_a && present_a && boxes_b && present_b && D, "part_box_pairwise: null pointer");
  DFX_REQUIRE(Ma > 0 && Mb > 0 && C > 0, "part_box_pairwise: Ma = %d, Mb = %d, C = %d must be positive", Ma, Mb, C);
  DFX_REQUIRE(metric >= 0 && metric <= 2, "part_box_pairwise: unknown metric %d (0 l2, 1 iou, 2 chamfer)", metric);
  DFX_REQUIRE(row0 >= 0, "part_box_pairwise: row0 = %lld is negative", row0);
  const long long P = (long long)Ma * Mb;
  DFX_REQUIRE(P <= 0x7fffffffLL, "part_box_pairwise: %lld pairs in one launch", P);
  hipStream_t st = dfx::as_stream(stream);
  if (metric == 2)
    k_box_chamfer<<<(int)P, NT, 0, st>>>(boxes_a, present_a, boxes_b, present_b, Mb, C, seed, row0, units, D);
  else
    k_box_pair<<<grid_of(P), NT, 0, st>>>(boxes_a, present_a, boxes_b, present_b, Ma, Mb, C, metric, D);
  return dfx::check_launch("part_box_pairwise");
}

int dfx_debug_part_box_units(uint64_t seed, long long pair0, int P, int C, float *units, dfx_stream_t stream) {
  DFX_REQUIRE(units && P > 0 && C > 0 && pair0 >= 0, "debug_part_box_units: bad arguments");
  const long long total = (long long)P * C * 2 * BOX_PTS;
  k_box_units<<<grid_of(total), NT, 0, dfx::as_stream(stream)>>>(seed, pair0, total, C, units);
  return dfx::check_launch("debug_part_box_units");
}

}  // extern "C"
