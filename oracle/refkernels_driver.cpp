/* Driver for the reference's own FPS and auction-EMD kernels run on the CPU (ORACLE — test infrastructure only).
 *
 * The *.inc files included below are NOT part of this repository: oracle/refkernels.py cuts them, by line range and
 * checked SHA-256, out of a checkout of the reference into oracle/_ref/ and compiles this file next to them.  They hold the
 * unmodified text of
 *     pointnet2_ops_lib/pointnet2_ops/_ext-src/include/cuda_utils.h:13-19   (TOTAL_THREADS, opt_n_threads)
 *     pointnet2_ops_lib/pointnet2_ops/_ext-src/src/sampling_gpu.cu:59-173   (__update, furthest_point_sampling_kernel)
 *     python/difffacto/metrics/emd/emd_cuda.cu:10-226 and :284-300          (atomicMax .. CalcDist, NmDistanceGradKernel)
 * This file restates only what surrounds the kernels: the host wrappers' launch shapes and buffer initialisation.
 */
#include "cuda_on_cpu.h"

#include <cmath>

#include "ref_cuda_utils_13_19.inc"   /* the block-size rule, cut out like the kernels */
#include "ref_sampling_gpu_59_173.inc"
#include "ref_emd_cuda_10_226.inc"
#include "ref_emd_cuda_284_300.inc"

using cuda_on_cpu::launch;

namespace {

/* The kernel instance whose block size equals the launch's thread count (the block-size rule only gives powers of two up to 512). */
template <unsigned int BS>
void fps_launch(unsigned threads, int b, int n, int m, const float *dataset, float *temp, int *idxs) {
  if constexpr (BS > 1) {
    if (threads != BS) return fps_launch<BS / 2>(threads, b, n, m, dataset, temp, idxs);
  }
  launch(dim3(b), dim3(threads), [=] { furthest_point_sampling_kernel<BS>(b, n, m, dataset, temp, idxs); });
}

}  // namespace

extern "C" {

/* 0 = ascending fibre order, 1 = descending */
void ref_schedule(int order) { cuda_on_cpu::set_order(order); }

/* What the reference's host wrapper (sampling_gpu.cu:175-229) does: one block per cloud, the block size from the block-size rule
 * of the span above, the template instance of that size.  temp: (b, n) pre-filled with 1e10 by the caller (sampling.cpp:74-76);
 * idxs: (b, m).  -1 where the rule gives something no instance has (it cannot). */
int ref_fps(int b, int n, int m, const float *dataset, float *temp, int *idxs) {
  const unsigned threads = opt_n_threads(n);
  if (threads == 0 || threads > 512 || (threads & (threads - 1))) return -1;
  fps_launch<512>(threads, b, n, m, dataset, temp, idxs);
  return 1;
}

/* emdFunction.forward (emd_module.py:46-57: buffer shapes and fills) + emd_cuda_forward (emd_cuda.cu:228-282: checks and the
 * launch sequence :256-269).  dist, assignment: (b, n) outputs.  Two optional observers, filled by this host code from the
 * buffers between launches (the kernels are not touched): unassigned, iters ints, the first pair's number of unassigned points
 * at the start of each iteration; ties, 2 ints, [0] the iterations in which some target had two or more bidders inside GetMax's
 * 1e-6 window (:188) — where its write race decides — and [1] the number of such (iteration, target) pairs.
 * Returns 1, or -1 where the reference refuses the input. */
int ref_emd_forward(int b, int n, const float *xyz1_in, const float *xyz2_in, float eps, int iters, float *dist_out,
                    int *assignment_out, int *unassigned, int *ties) {
  if (b > 512 || n % 1024 != 0 || n <= 0 || b <= 0) return -1;
  const size_t bn = (size_t)b * n;
  std::vector<float> xyz1(xyz1_in, xyz1_in + bn * 3), xyz2(xyz2_in, xyz2_in + bn * 3);
  std::vector<float> dist(bn, 0.f), price(bn, 0.f), bid_increments(bn, 0.f), max_increments(bn, 0.f);
  std::vector<int> assignment(bn, -1), assignment_inv(bn, -1), bid(bn, 0), unass_idx(bn, 0), max_idx(bn, 0);
  std::vector<int> unass_cnt(512, 0), unass_cnt_sum(512, 0), cnt_tmp(512, 0);
  const dim3 grid(b, n / 1024, 1);
  float *x1 = xyz1.data(), *x2 = xyz2.data(), *pr = price.data(), *bi = bid_increments.data(), *mi = max_increments.data(),
        *di = dist.data();
  int *as = assignment.data(), *ai = assignment_inv.data(), *bd = bid.data(), *ui = unass_idx.data(), *mx = max_idx.data(),
      *uc = unass_cnt.data(), *us = unass_cnt_sum.data(), *ct = cnt_tmp.data();
  for (int i = 0; i < iters; i++) {
    const bool last = i == iters - 1;
    launch(dim3(1), dim3(b), [=] { clear(b, ct, uc); });
    launch(grid, dim3(1024), [=] { calc_unass_cnt(b, n, as, uc); });
    if (unassigned) unassigned[i] = uc[0];
    launch(dim3(1), dim3(b), [=] { calc_unass_cnt_sum(b, uc, us); });
    launch(grid, dim3(1024), [=] { calc_unass_idx(b, n, as, ui, uc, us, ct); });
    launch(grid, dim3(1024), [=] { Bid(b, n, x1, x2, eps, as, ai, pr, bd, bi, mi, uc, us, ui); });
    if (ties && !last) { /* the last iteration assigns every bidder whatever max_idx says (:201) */
      std::vector<int> winners(bn, 0);
      int tied = 0;
      for (size_t j = 0; j < bn; ++j)
        if (as[j] == -1) {
          const size_t k = j / n * n + bd[j];
          if (bi[j] - 1e-6 <= mi[k] && mi[k] <= bi[j] + 1e-6) tied += ++winners[k] == 2;
        }
      ties[0] += tied > 0;
      ties[1] += tied;
    }
    launch(grid, dim3(1024), [=] { GetMax(b, n, as, bd, bi, mi, mx); });
    launch(grid, dim3(1024), [=] { Assign(b, n, as, ai, pr, bd, bi, mi, mx, last); });
  }
  launch(grid, dim3(1024), [=] { CalcDist(b, n, x1, x2, di, as); });
  memcpy(dist_out, di, bn * sizeof(float));
  memcpy(assignment_out, as, bn * sizeof(int));
  return 1;
}

/* emdFunction.backward (emd_module.py:69-72) + emd_cuda_backward (emd_cuda.cu:302-307).  grad_xyz: (b, n, 3), zero-filled here. */
int ref_emd_backward(int b, int n, const float *xyz1, const float *xyz2, const float *grad_dist, const int *idx, float *grad_xyz) {
  if (n % 1024 != 0 || n <= 0 || b <= 0) return -1;
  memset(grad_xyz, 0, (size_t)b * n * 3 * sizeof(float));
  launch(dim3(b, n / 1024, 1), dim3(1024), [=] { NmDistanceGradKernel(b, n, xyz1, xyz2, grad_dist, idx, grad_xyz); });
  return 1;
}

}  // extern "C"
