// Launchers of csrc/part_sampling.hip for the candidate search of latents_kernels.hip (dfx_part_search): every pointer is a device
// pointer, nothing allocates, nothing zeroes n_bad (the entry points do), errors are reported through dfx::check_launch.
#pragma once
#include "dfx_common.h"

namespace dfx {
namespace psel {

constexpr int MAX_K = 4096;        // candidates per group (selection state lives in LDS)
constexpr int MAX_DRAWS = 65536;   // normals per (candidate, axis, part)
constexpr int MAX_GLOBAL_ROWS = 262144;   // candidate rows of one global selection

int check_shape(const char *who, long long G, int K, int J);
// stats (R,4,3,J) of rows row0 .. row0+R-1
int launch_draw_stats(uint64_t seed, long long row0, long long R, int J, int n_draws, float *stats, hipStream_t st);
// scores (G K,6,J) from stats (G K,4,3,J); valid (G,J)
int launch_scores(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int J, float *scores,
                  hipStream_t st);
int launch_diverse(const float *scores, const float *valid, int G, int K, int J, int P, int32_t *idx, int32_t *n_bad, hipStream_t st);
int launch_fit(const float *mean, const float *logvar, const float *target_mean, const float *target_logvar, const float *weight, int G,
               int K, int J, int32_t *idx, float *fit, int32_t *n_bad, hipStream_t st);
// FIRST: idx[g,p] = p
int launch_first(int G, int P, int32_t *idx, hipStream_t st);
// rows idx[g,p] of group g of noise (G K,ND) and of mean / logvar (G Kc,3,J: the first Kc candidates of every group) -> (G P, ..)
int launch_gather(const int32_t *idx, const float *noise, const float *mean, const float *logvar, int G, int K, int Kc, int P, int ND, int J,
                  float *noise_o, float *mean_o, float *logvar_o, hipStream_t st);

// the global selection: check_shape plus 1 <= P <= G K <= MAX_GLOBAL_ROWS and the rule
int check_shape_global(const char *who, long long G, int K, int J, int P, int rule);
// bytes of the selection's state (per row mind fp64 and one byte; the per-block bests of the launch-per-pick path), a multiple of 16
size_t diverse_global_state_bytes(long long rows);
// idx (P): global rows; state: diverse_global_state_bytes(G K) device bytes, 8-byte aligned (used by the launch-per-pick path).  One workgroup
// up to 512 rows, one launch per pick above (dfx_debug_diverse_global_path(1): at every size)
int launch_diverse_global(const float *scores, const float *valid, int G, int K, int J, int P, int rule, int32_t *idx, int32_t *n_bad,
                          void *state, hipStream_t st);
// rows idx[p] of noise (R,ND), mean / logvar (R,3,J) -> (P, ..)
int launch_gather_rows(const int32_t *idx, const float *noise, const float *mean, const float *logvar, int P, int ND, int J, float *noise_o,
                       float *mean_o, float *logvar_o, hipStream_t st);

}  // namespace psel
}  // namespace dfx
