// Occupancy-grid JSD for gfx950: nearest kept grid cell per point, per-cell counters, the JSD / entropy reductions (include/dfx.h).
//
// Semantics of python/difffacto/datasets/evaluation_utils.py (unit_cube_grid_point_cloud :547-565, entropy_of_occupancy_grid
// :586-626, jensen_shannon_divergence :629-648), restated in DESIGN.md §5.9.  The grid is built on the host once per
// (resolution, in_sphere): the keep mask and, per (i,j) column, the interval [k_lo,k_hi] of kept k with the compact index of its
// first cell (a sphere cuts every column in an interval).  Mapping: one 256-thread workgroup per cloud, a point per thread.
//   (a) the eight cells around the point (floor / ceil per axis, clamped to the grid) hold the nearest of ALL cells; if one of the
//       nearest among them is kept it is the answer;
//   (b) else the point queues in LDS and the queue is worked off a point per thread: a walk over the (i,j) columns, the nearest kept
//       cell of a column being floor / ceil of the k coordinate clamped to [k_lo,k_hi], pruned by the (x,y) distance.
// Distances are (dx*dx + dy*dy) + dz*dz in double, every operation rounded; ties go to the lower compact index (cells are visited in
// ascending order and replaced on a strictly smaller distance only).  Points beyond 1e5, where cells further than one step away
// could round to the same distance, take the walk with every k of a column visited: a plain scan of all kept cells.
// Counting: integer atomics on the HBM counters; a per-cloud LDS bitmap (cells bits per row) makes the Bernoulli counters count a
// cell once per cloud.  Labelled rows that do not fit the LDS budget run in passes (row ranges) over the same points.
#include "dfx_common.h"

#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int OCC_MAX_R = 40;
constexpr int OCC_MAX_C = 16;
constexpr int OCC_CHUNK = 2048;            // points per round: uint16 ids in the LDS queue
constexpr int OCC_LDS_BUDGET = 60 * 1024;  // dynamic LDS per workgroup: no attribute needed, two workgroups per CU at the largest grid
constexpr double OCC_FAR = 1e5;
constexpr unsigned COL_EMPTY = 0x00ffu;    // k_lo = 255 > k_hi = 0

// column entry: k_lo | k_hi << 8 | first compact index << 16 (at most 40^3 - 40 = 63960)
__host__ __device__ inline int col_lo(unsigned e) { return (int)(e & 255u); }
__host__ __device__ inline int col_hi(unsigned e) { return (int)((e >> 8) & 255u); }
__host__ __device__ inline int col_first(unsigned e) { return (int)(e >> 16); }

struct Grid {
  int R = 0, cells = 0;
  std::vector<uint8_t> mask;    // (R,R,R)
  std::vector<unsigned> col;    // (R,R)
  double axis[OCC_MAX_R] = {};
  bool intervals = true;        // every column's kept set is an interval
};

// Host grid per (R, in_sphere); entries live for the life of the process.  This file is compiled with -ffp-contract=off (build.py),
// so the float32 expressions below round after every operation, as numpy's do.
const Grid *host_grid(int R, int in_sphere) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<Grid>> cache;
  std::lock_guard<std::mutex> lock(mu);
  std::unique_ptr<Grid> &slot = cache[R * 2 + (in_sphere ? 1 : 0)];
  if (slot) return slot.get();
  auto g = std::make_unique<Grid>();
  g->R = R;
  const double spacing = 1.0 / (double)(R - 1);
  float ax[OCC_MAX_R];
  for (int i = 0; i < R; ++i) {
    ax[i] = (float)((double)i * spacing - 0.5);
    g->axis[i] = (double)ax[i];
  }
  g->mask.assign((size_t)R * R * R, 1);
  g->col.assign((size_t)R * R, COL_EMPTY);
  int cells = 0;
  for (int i = 0; i < R; ++i)
    for (int j = 0; j < R; ++j) {
      int lo = -1, hi = -1, n = 0;
      for (int k = 0; k < R; ++k) {
        bool keep = true;
        if (in_sphere) {
          const float xx = ax[i] * ax[i], yy = ax[j] * ax[j], zz = ax[k] * ax[k];
          keep = sqrtf((xx + yy) + zz) <= 0.5f;
        }
        g->mask[((size_t)i * R + j) * R + k] = keep ? 1 : 0;
        if (keep) {
          if (lo < 0) lo = k;
          hi = k;
          ++n;
        }
      }
      if (n == 0) continue;
      if (n != hi - lo + 1) g->intervals = false;
      g->col[(size_t)i * R + j] = (unsigned)lo | ((unsigned)hi << 8) | ((unsigned)cells << 16);
      cells += n;
    }
  g->cells = cells;
  slot = std::move(g);
  return slot.get();
}

// Device copy of a grid's tables per (device, R, in_sphere): 40 doubles of axis values, then the (R,R) column entries.
struct DevTable {
  const double *axis = nullptr;
  const unsigned *col = nullptr;
};
// The first call per key allocates and uploads with a blocking copy, which a capturing stream does not allow: it is refused with a
// text that says what to do instead of failing inside the allocation or the copy.  A table is at most 6.7 KB and there are at most
// 78 keys per device, so the cache is kept for the life of the process like the host grids.
int device_table(const Grid *g, int in_sphere, hipStream_t st, DevTable *out) {
  static std::mutex mu;
  static std::map<long long, void *> cache;
  int dev = 0;
  DFX_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  void *&slot = cache[((long long)dev << 8) | (long long)(g->R * 2 + (in_sphere ? 1 : 0))];
  if (!slot) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    DFX_HIP_TRY(hipStreamIsCapturing(st, &cap));
    DFX_REQUIRE(cap == hipStreamCaptureStatusNone,
                "occupancy_grid: the first call for resolution %d%s on device %d uploads the grid table and cannot be captured: "
                "call once outside the capture", g->R, in_sphere ? " (sphere)" : "", dev);
    const size_t bytes = OCC_MAX_R * sizeof(double) + (size_t)g->R * g->R * sizeof(unsigned);
    std::vector<unsigned char> host(bytes);
    memcpy(host.data(), g->axis, OCC_MAX_R * sizeof(double));
    memcpy(host.data() + OCC_MAX_R * sizeof(double), g->col.data(), (size_t)g->R * g->R * sizeof(unsigned));
    void *d = nullptr;
    DFX_HIP_TRY(hipMalloc(&d, bytes));
    hipError_t e = hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return dfx::set_error(DFX_ERR_HIP, "occupancy_grid: table upload: %s", hipGetErrorString(e));
    }
    slot = d;
  }
  out->axis = static_cast<const double *>(slot);
  out->col = reinterpret_cast<const unsigned *>(static_cast<const unsigned char *>(slot) + OCC_MAX_R * sizeof(double));
  return DFX_OK;
}

// Rounded double operations: explicit on the device; the host build of this file has contraction off (build.py).
__host__ __device__ inline double mul_rn(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
__host__ __device__ inline double add_rn(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
__host__ __device__ inline double sq_xy(double dx, double dy) { return add_rn(mul_rn(dx, dx), mul_rn(dy, dy)); }
__host__ __device__ inline double sq_add_z(double dxy, double dz) { return add_rn(dxy, mul_rn(dz, dz)); }

// floor of the grid coordinate of p, in [-1, R]; one off at most near a grid point, where the other candidate is the answer anyway
__host__ __device__ inline int grid_floor(double p, int R) {
  const double t = fmin(fmax((p + 0.5) * (double)(R - 1), -1.0), (double)R);
  return (int)floor(t);
}
__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ inline bool is_far(double px, double py, double pz) {
  return !(fmax(fmax(fabs(px), fabs(py)), fabs(pz)) <= OCC_FAR);
}

// (a) The eight cells around a finite point: the compact index of the nearest cell if it is kept (of several equally near ones: the
// first kept one in ascending order), else -1: the point needs the walk.
__host__ __device__ inline int nearest_around(const double *axis, const unsigned *col, int R, double px, double py, double pz) {
  if (is_far(px, py, pz)) return -1;
  const int fi = grid_floor(px, R), fj = grid_floor(py, R), fk = grid_floor(pz, R);
  const int ci[2] = {clampi(fi, 0, R - 1), clampi(fi + 1, 0, R - 1)};
  const int cj[2] = {clampi(fj, 0, R - 1), clampi(fj + 1, 0, R - 1)};
  const int ck[2] = {clampi(fk, 0, R - 1), clampi(fk + 1, 0, R - 1)};
  double best = INFINITY;
  int found = -1;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const unsigned e = col[ci[a] * R + cj[c]];
      const double dxy = sq_xy(px - axis[ci[a]], py - axis[cj[c]]);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int k = ck[d];
        const double dist = sq_add_z(dxy, pz - axis[k]);
        const bool kept = k >= col_lo(e) && k <= col_hi(e);
        const int idx = kept ? col_first(e) + (k - col_lo(e)) : -1;
        if (dist < best) best = dist, found = idx;          // a nearer cell, kept or not
        else if (dist == best && found < 0) found = idx;    // a tie: the first kept one
      }
    }
  return found;
}

// (b) The column walk: the nearest kept cell of a finite point, columns in ascending order, replaced on a strictly smaller distance.
__host__ __device__ inline int nearest_walk(const double *axis, const unsigned *col, int R, double px, double py, double pz) {
  const bool far = is_far(px, py, pz);
  const int fk = grid_floor(pz, R);
  double best = INFINITY;
  int found = -1;
  for (int i = 0; i < R; ++i) {
    const double dx = px - axis[i], dx2 = mul_rn(dx, dx);
    if (!(dx2 < best)) continue;   // the distance is at least dx2: it cannot be strictly smaller
    for (int j = 0; j < R; ++j) {
      const unsigned e = col[i * R + j];
      const int lo = col_lo(e), hi = col_hi(e);
      if (lo > hi) continue;
      const double dy = py - axis[j], dxy = add_rn(dx2, mul_rn(dy, dy));
      if (!(dxy < best)) continue;
      const int k0 = far ? lo : clampi(fk, lo, hi), k1 = far ? hi : clampi(fk + 1, lo, hi);
      for (int k = k0; k <= k1; ++k) {
        const double dist = sq_add_z(dxy, pz - axis[k]);
        if (dist < best) best = dist, found = col_first(e) + (k - lo);
      }
    }
  }
  return found;   // >= 0: the grid keeps a cell and the point is finite
}

// ---- one workgroup per cloud; rows [row0, row0 + nrows) of the counters ----
__global__ void __launch_bounds__(NT) k_occupancy(const float *__restrict__ xyz, const int32_t *__restrict__ labels, int N, int C, int R,
                                                  int cells, const double *__restrict__ g_axis, const unsigned *__restrict__ g_col,
                                                  int row0, int nrows, unsigned long long *__restrict__ counters,
                                                  int *__restrict__ bernoulli, int32_t *__restrict__ cell_index,
                                                  int *__restrict__ n_bad) {
  extern __shared__ __align__(16) unsigned char smem[];
  double *axis = reinterpret_cast<double *>(smem);
  unsigned *col = reinterpret_cast<unsigned *>(axis + OCC_MAX_R);
  const int words = (cells + 31) >> 5;
  unsigned *bitmap = col + R * R;
  uint16_t *queue = reinterpret_cast<uint16_t *>(bitmap + (size_t)nrows * words);
  __shared__ int qn;

  const int b = blockIdx.x;
  const float *X = xyz + (size_t)b * N * 3;
  const int32_t *L = labels ? labels + (size_t)b * N : nullptr;
  int32_t *CI = (cell_index && row0 == 0) ? cell_index + (size_t)b * N : nullptr;

  for (int i = threadIdx.x; i < OCC_MAX_R; i += NT) axis[i] = i < R ? g_axis[i] : 0.0;
  for (int i = threadIdx.x; i < R * R; i += NT) col[i] = g_col[i];
  for (int i = threadIdx.x; i < nrows * words; i += NT) bitmap[i] = 0u;

  // a point's cell is known: the counters of row 0 and of its label's row, where this pass owns them
  auto commit = [&](int n, int cell) {
    if (CI) CI[n] = cell;
    if (cell < 0) return;
    int rows[2] = {0, -1};
    if (L) {
      const int l = L[n];
      if (l >= 0 && l < C) rows[1] = 1 + l;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int r = rows[s] - row0;
      if (rows[s] < 0 || r < 0 || r >= nrows) continue;
      atomicAdd(&counters[(size_t)rows[s] * cells + cell], 1ull);
      const unsigned bit = 1u << (cell & 31);
      const unsigned old = atomicOr(&bitmap[(size_t)r * words + (cell >> 5)], bit);
      if (!(old & bit)) atomicAdd(&bernoulli[(size_t)rows[s] * cells + cell], 1);
    }
  };

  for (int base = 0; base < N; base += OCC_CHUNK) {
    const int cnt = min(OCC_CHUNK, N - base);
    __syncthreads();   // tables and bitmap written; the previous round's queue read
    if (threadIdx.x == 0) qn = 0;
    __syncthreads();
    // (a) the eight cells around the point
    for (int t = threadIdx.x; t < cnt; t += NT) {
      const int n = base + t;
      const float fx = X[(size_t)n * 3], fy = X[(size_t)n * 3 + 1], fz = X[(size_t)n * 3 + 2];
      if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) {
        if (row0 == 0) {
          atomicAdd(n_bad, 1);
          if (CI) CI[n] = -1;
        }
        continue;
      }
      const int found = nearest_around(axis, col, R, (double)fx, (double)fy, (double)fz);
      if (found >= 0) commit(n, found);
      else queue[atomicAdd(&qn, 1)] = (uint16_t)t;
    }
    __syncthreads();
    // (b) the column walk
    const int nq = qn;
    for (int q = threadIdx.x; q < nq; q += NT) {
      const int n = base + queue[q];
      const double px = (double)X[(size_t)n * 3], py = (double)X[(size_t)n * 3 + 1], pz = (double)X[(size_t)n * 3 + 2];
      commit(n, nearest_walk(axis, col, R, px, py, pz));
    }
  }
}

// ---- reductions: one workgroup, per-thread strided sums, then a fixed LDS tree ----
__device__ double block_sum_d(double v, double *red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = __dadd_rn(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}
__device__ long long block_sum_ll(long long v, long long *red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ double entr(double x) { return x > 0.0 ? -__dmul_rn(x, log(x)) : 0.0; }

// mode 0: JSD of two counter rows; mode 1: accumulated Bernoulli entropy
__global__ void __launch_bounds__(NT) k_jsd_reduce(int mode, const long long *__restrict__ P, const long long *__restrict__ Q,
                                                   const int *__restrict__ bern, int cells, long long n_shapes, double *__restrict__ out) {
  __shared__ double red[NT];
  __shared__ long long redl[NT];
  if (mode == 0) {
    long long sp = 0, sq = 0;
    for (int c = threadIdx.x; c < cells; c += NT) sp += P[c], sq += Q[c];
    sp = block_sum_ll(sp, redl);
    sq = block_sum_ll(sq, redl);
    const double np = (double)sp, nq = (double)sq;
    double ep = 0.0, eq = 0.0, em = 0.0;
    for (int c = threadIdx.x; c < cells; c += NT) {
      const double p = (double)P[c] / np, q = (double)Q[c] / nq;
      ep = __dadd_rn(ep, entr(p));
      eq = __dadd_rn(eq, entr(q));
      em = __dadd_rn(em, entr(__dadd_rn(p, q) / 2.0));
    }
    ep = block_sum_d(ep, red);
    eq = block_sum_d(eq, red);
    em = block_sum_d(em, red);
    if (threadIdx.x == 0) out[0] = (em - __dadd_rn(ep, eq) / 2.0) / log(2.0);
  } else {
    const double n = (double)n_shapes;
    double acc = 0.0;
    for (int c = threadIdx.x; c < cells; c += NT) {
      const int g = bern[c];
      if (g > 0) {
        const double p = (double)g / n;
        acc = __dadd_rn(acc, __dadd_rn(entr(p), entr(1.0 - p)));
      }
    }
    acc = block_sum_d(acc, red);
    if (threadIdx.x == 0) out[0] = acc / (double)cells;
  }
}

int check_resolution(const char *what, int R) {
  DFX_REQUIRE(R >= 2 && R <= OCC_MAX_R, "%s: resolution = %d outside [2,%d]", what, R, OCC_MAX_R);
  return DFX_OK;
}

}  // namespace

extern "C" {

int dfx_occupancy_num_cells(int resolution, int in_sphere) {
  if (int rc = check_resolution("occupancy_num_cells", resolution)) return rc;
  return host_grid(resolution, in_sphere != 0)->cells;
}

int dfx_occupancy_cell_mask(int resolution, int in_sphere, uint8_t *host_mask) {
  if (int rc = check_resolution("occupancy_cell_mask", resolution)) return rc;
  DFX_REQUIRE(host_mask, "occupancy_cell_mask: null pointer");
  const Grid *g = host_grid(resolution, in_sphere != 0);
  memcpy(host_mask, g->mask.data(), g->mask.size());
  return DFX_OK;
}

int dfx_debug_occupancy_host(const float *host_xyz, int n, int resolution, int in_sphere, int32_t *host_cell_index) {
  if (int rc = check_resolution("debug_occupancy_host", resolution)) return rc;
  DFX_REQUIRE(host_xyz && host_cell_index && n > 0, "debug_occupancy_host: bad arguments");
  const Grid *g = host_grid(resolution, in_sphere != 0);
  DFX_REQUIRE(g->cells > 0 && g->intervals, "debug_occupancy_host: resolution %d: no usable grid", resolution);
  for (int p = 0; p < n; ++p) {
    const float fx = host_xyz[3 * p], fy = host_xyz[3 * p + 1], fz = host_xyz[3 * p + 2];
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(fz))) {
      host_cell_index[p] = -1;
      continue;
    }
    int c = nearest_around(g->axis, g->col.data(), g->R, (double)fx, (double)fy, (double)fz);
    if (c < 0) c = nearest_walk(g->axis, g->col.data(), g->R, (double)fx, (double)fy, (double)fz);
    host_cell_index[p] = c;
  }
  return DFX_OK;
}

int dfx_occupancy_grid_f32(const float *xyz, const int32_t *labels, int B, int N, int C, int resolution, int in_sphere,
                           int accumulate, int64_t *counters, int32_t *bernoulli, int32_t *cell_index, int32_t *n_bad,
                           dfx_stream_t stream) {
  DFX_REQUIRE(xyz && counters && bernoulli && n_bad, "occupancy_grid: null pointer");
  DFX_REQUIRE(B > 0 && N > 0, "occupancy_grid: B = %d, N = %d must be positive", B, N);
  if (int rc = check_resolution("occupancy_grid", resolution)) return rc;
  if (labels) DFX_REQUIRE(C >= 0 && C <= OCC_MAX_C, "occupancy_grid: C = %d outside [0,%d]", C, OCC_MAX_C);
  const int R = resolution, sph = in_sphere != 0;
  const Grid *g = host_grid(R, sph);
  DFX_REQUIRE(g->cells > 0, "occupancy_grid: the grid of resolution %d%s keeps no cell", R, sph ? " in the sphere" : "");
  DFX_REQUIRE(g->intervals, "occupancy_grid: resolution %d: a column's kept cells are not an interval", R);
  const int cells = g->cells, rows = labels ? C + 1 : 1, words = (cells + 31) >> 5;
  const int fixed = OCC_MAX_R * 8 + R * R * 4 + OCC_CHUNK * 2;
  const int rows_per_pass = (OCC_LDS_BUDGET - fixed) / (words * 4);   // >= 6: words * 4 <= 8000, fixed <= 10816
  hipStream_t st = dfx::as_stream(stream);
  DevTable tab;
  if (int rc = device_table(g, sph, st, &tab)) return rc;
  if (!accumulate) {
    DFX_HIP_TRY(hipMemsetAsync(counters, 0, (size_t)rows * cells * sizeof(int64_t), st));
    DFX_HIP_TRY(hipMemsetAsync(bernoulli, 0, (size_t)rows * cells * sizeof(int32_t), st));
    DFX_HIP_TRY(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  }
  for (int row0 = 0; row0 < rows; row0 += rows_per_pass) {
    const int nrows = rows - row0 < rows_per_pass ? rows - row0 : rows_per_pass;
    const int lds = fixed + nrows * words * 4;
    k_occupancy<<<B, NT, lds, st>>>(xyz, labels, N, labels ? C : 0, R, cells, tab.axis, tab.col, row0, nrows,
                                    reinterpret_cast<unsigned long long *>(counters), bernoulli, cell_index, n_bad);
    if (int rc = dfx::check_launch("occupancy_grid")) return rc;
  }
  return DFX_OK;
}

int dfx_occupancy_jsd_f64(const int64_t *counters_p, const int64_t *counters_q, int cells, double *jsd, dfx_stream_t stream) {
  DFX_REQUIRE(counters_p && counters_q && jsd, "occupancy_jsd: null pointer");
  DFX_REQUIRE(cells > 0, "occupancy_jsd: cells = %d must be positive", cells);
  k_jsd_reduce<<<1, NT, 0, dfx::as_stream(stream)>>>(0, reinterpret_cast<const long long *>(counters_p),
                                                     reinterpret_cast<const long long *>(counters_q), nullptr, cells, 0, jsd);
  return dfx::check_launch("occupancy_jsd");
}

int dfx_occupancy_entropy_f64(const int32_t *bernoulli, int cells, int64_t n_shapes, double *entropy, dfx_stream_t stream) {
  DFX_REQUIRE(bernoulli && entropy, "occupancy_entropy: null pointer");
  DFX_REQUIRE(cells > 0 && n_shapes > 0, "occupancy_entropy: cells = %d, n_shapes = %lld must be positive", cells, (long long)n_shapes);
  k_jsd_reduce<<<1, NT, 0, dfx::as_stream(stream)>>>(1, nullptr, nullptr, bernoulli, cells, (long long)n_shapes, entropy);
  return dfx::check_launch("occupancy_entropy");
}

}  // extern "C"
