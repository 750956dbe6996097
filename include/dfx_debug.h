/* libdfx test and tuning hooks — NOT part of the drop-in ABI of include/dfx.h.
 *
 * Nothing here replaces a reference interface: these are the switches tests/ and tools/ use to run two implementations of the
 * same entry point against each other (A/B), to sweep a launch shape, or to replay random factors into the oracle.  They are
 * process-global and not thread-safe; a product binding never includes this header.  Results are valid under
 * every setting (all variants are parity-tested against each other); only the choice of kernel changes.
 */
#ifndef DFX_DEBUG_H
#define DFX_DEBUG_H
#include "dfx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Dropout factors (0 or 1/(1-p)) of n consecutive elements of a site: 2 i = behind to_out of block i over (B N, 128),
 * 2 i + 1 = behind the GEGLU of block i over (B N, 512), 1000 = time_embed over (B, 1024).  n % 4 == 0. */
int dfx_debug_dropout_factors(uint64_t seed, int site, float p, float *out, long long n, dfx_stream_t stream);
/* Debug / A-B switch: 0 routes the bf16 training path through the layer-by-layer kernels instead of the fused ones (default 1: the fused
 * path, for DFX_PREC_BF16 from 256 rows, with or without dropout).  Any non-zero value selects the fused path (2 once kept the attention
 * forward and its input gradient as kernels of their own; it is now the same as 1). */
void dfx_debug_train_fused(int on);
/* The kernel family the calling thread's most recent dfx_denoiser_train_forward took (its backward follows the same record):
 * "fused_bf16", "fused_bf16_dropout" (k_ff_fwd_chain / k_ff_bwd / k_ff_wgrad), "layer_bf16(_dropout)" (layer-by-layer kernels, bf16
 * products), "layer_f32(_dropout)" (exact fp32; also what DFX_PREC_BF16 takes below 256 rows), "none" before the first call. */
const char *dfx_debug_last_train_path(void);
/* Host-side run (no GPU) of the training step's planner (csrc/train_plan.h): the name dfx_debug_last_train_path() would report after a
 * dfx_denoiser_train_forward of B shapes of N points with `prec` (DFX_PREC_*) and dropout_p under dfx_debug_train_fused(fused_switch) and
 * dfx_debug_train_streams(streams_switch); NULL for arguments the entry points reject.  *bits_out (may be NULL): bits 0-1 the path (0 layer
 * by layer with fp32-stored activations, 1 layer by layer with bf16-stored product operands, 3 fused; 2 was the fused path with the attention
 * as kernels of its own: retired, never reported), 4 = bf16-stored product operands, 8 = dropout on; what goes to the side stream: 16 the forward's context branch, 32 the backward
 * uses the side stream at all, 64 the head's sums right behind k_head_bwd, 128 the stem's backward behind block 0, 256 the finishing kernels'
 * leaves, 512 the stem's backward beside the finishing kernels.  A pure function of its arguments: the process-global switches are not read. */
const char *dfx_debug_plan_train(int prec, float dropout_p, int fused_switch, int streams_switch, int B, int N, int *bits_out);
/* Debug / A-B switch: 0 keeps every launch of the fused training path on the caller's stream (default 1: the context branch of the forward
 * and the parameter-gradient reductions of the backward run on a per-device side stream, forked from and joined into the caller's stream
 * inside the call).  Same kernels and operands either way: bit-identical results. */
void dfx_debug_train_streams(int on);
/* Debug / A-B switch: 0 = the PointNetV2 training forward computes its BatchNorm batch statistics with two passes over each layer's output
 * (mean, then centred sum of squares); default 1 = from (count, mean, M2) partials the fp32 product kernels leave in their epilogues
 * (>= 8192 rows), equal up to fp32 rounding of the statistics; and BatchNorm over at most 512 rows (the per-part heads: over the B shapes) as one
 * launch per direction instead of seven / four, bit-identical to the multi-launch passes. */
void dfx_debug_bn_fused_stats(int on);
/* Test hook: the branch dfx_pointnet_v2_train_backward will derive from this workspace, copied out between the forward and the backward (the
 * workspace is only read).  trunk_masks[3]: one byte per unit of the three ReLU trunk layers, (B N, 128 / 128 / 256); head_masks[4]: the heads'
 * ReLU sites mlp_m.1, mlp_m.4, mlp_v.1, mlp_v.4, (B, 4 x 256) and (B, 4 x 128) per head; 1 = the gradient passes, from the backward's own test
 * (the BatchNorm affine of z > 0).  arg: the max-pool's selected point per (shape, part, channel), (B, 4, 512) int32.  Device pointers. */
int dfx_debug_pointnet_v2_branch(const dfx_pointnet_v2_weights *wt, const void *workspace, size_t workspace_bytes, int B, int N,
                                 uint8_t *const *trunk_masks, uint8_t *const *head_masks, int32_t *arg, dfx_stream_t stream);
/* Test hook: the same for dfx_prior_loss_backward: the ReLU masks h1 > 0 and h2 > 0 of every coupling layer, (flow_depth, 4 B, flow_hidden)
 * bytes each, rows part-major (part * B + shape). */
int dfx_debug_prior_loss_branch(const void *workspace, size_t workspace_bytes, int flow_depth, int flow_hidden, int B, uint8_t *h1_masks,
                                uint8_t *h2_masks, dfx_stream_t stream);
/* Host-side run (no GPU) of that statistics arithmetic: n values in pieces of `chunk`, each piece as (count, mean, M2), merged left to right with
 * the kernels' own merge function; out3 = (count, mean, sum of squared deviations). */
void dfx_debug_stats_merge(const float *values, int n, int chunk, float *out3);
/* Host-side table of the fused training kernels' row addressing inside a 32-point tile (tiled = 1: the tile-major layout between the fused
 * kernels; 0: row-major): float offset of (point, channel) through the B-operand-layout and the accumulator-layout accessors; [32][128] int32 each. */
void dfx_debug_rowmap(int tiled, int *out_b, int *out_a);
/* The few-row fp32 products (latent front end, time-embedding MLP; mfma_linear.h) split their sum over K across four wavefronts when the call has at
 * most 256 output tiles — a different grouping of the same fp32 terms, chosen by the call's row count.  mode 1: split whenever K >= 128 (one grouping for
 * every batch size: sharded runs reproduce a single-process run's latents bit for bit whatever the shard size); 0: never; -1: automatic (default). */
void dfx_debug_lin_split_k(int mode);
/* Debug / A-B switch: 1 keeps the EMD auction's state in global memory for every n (default 0: in LDS when n <= 2688). */
void dfx_debug_emd_state_global(int on);
/* Debug / A-B switch: query points per thread of the Chamfer nearest-neighbour kernel in both directions of dfx_chamfer_forward_f32: 1 or 2 force
 * chamfer_nn_kernel<1> / <2> with ceil(n / (256 q)) workgroups per cloud; 0 (default, and any other value) = the launcher's own rule (<2> when
 * B * ceil(n / 512) >= 256).  Bit-identical results either way. */
void dfx_debug_chamfer_queries(int q);
/* Debug / sweep: workgroup shape of the register-resident FPS kernel (threads in {256, 512, 1024} x points per thread in {2..32},
 * used when threads * points >= N; 0, 0 = automatic). */
void dfx_debug_fps_shape(int threads, int points_per_thread);
/* Test hook for the bf16 product kernels of the training path (csrc/gemm_bf16.h): tn = 0: C (M,N) = A (M,K) B (N,K)^T + bias +
 * resid; tn = 1: C (M,N) = A (K,M)^T B (K,N) and db (M) = column sums of A, workspace >= (K/64 + 1) (M N + M) floats.
 * a_bf16 / b_bf16: the operand is stored as bf16 (lda / ldb in elements).  N % 128 == 0 (and M % 128 == 0 for tn = 1). */
int dfx_debug_gemm_bf16(int tn, const void *A, int lda, int a_bf16, const void *B, int ldb, int b_bf16, const float *bias,
                        const float *resid, float *C, float *db, float *workspace, size_t workspace_floats, int M, int N, int K,
                        dfx_stream_t stream);
/* Box calibration for bench.py: a bare v_mfma_f32_32x32x16_bf16 stream (one wavefront per SIMD on every CU, pseudo-random operands, nothing
 * else) of `iters` x 16 MFMAs per wavefront; *ms_out = HIP-event duration, *tflops_out = executed MFMA TFLOP/s — what this chip sustains on the
 * matrix pipe at its power cap and clocks (iters = 150000 runs ~50 ms).  Synchronises `stream`. */
int dfx_debug_bare_mfma(int iters, float *ms_out, double *tflops_out, dfx_stream_t stream);
/* Debug/A-B switch: force the direct (non LDS-pipelined) kernel for every launch. */
void dfx_debug_force_direct(int on);
/* dfx_denoiser_create's decision about the W1 bias fold of bf16 engines (dfx_denoiser_w1_fold): -1 = from the weights (default: channel 127
 * while its column of W1 diag(gamma3) is ordinary, else the hidden channel with the smallest column over all blocks, exchanged with 127 at
 * pack time), 0 = never (plain pack, direct kernel), 1 = always on channel 127 (round 5's form).  Applies to engines created afterwards. */
void dfx_debug_w1_fold(int mode);
/* The hidden channel whose K slot of the packed W1 carries b1' (127 unless create relabelled the channels; -1 = engine without the fold). */
int dfx_debug_w1_fold_channel(const dfx_denoiser *d);
/* Debug: force one chain-kernel variant of the denoiser launches (csrc/denoiser_plan.h: force_from_code).  The codes:
 *     0 = automatic: chosen from the batch shape by the cost model (the default); any value not listed here is treated as 0 - among them
 *       64, 160 and 161, which selected two since-retired kernels (bench.py's --pipe-waves help still lists 64: it now means automatic);
 *     8, 4, 2 = wavefronts per workgroup of the pipelined chain kernel (k_denoise_pipe<NW>, for an fp32 denoiser k_denoise_pipe_f32<NW>);
 *       tiles of NW x 32 points that would pad a shape by more than 3x fall back to the direct kernel;
 *     1 = the co-operative latency kernel k_denoise_coop (one 32-point tile per workgroup, eight wavefronts on it); for an fp32 denoiser: the
 *       direct kernel;
 *    16 = k_denoise_coop2 (bf16 only: the co-operative kernel with two 32-point tiles per workgroup; N % 64 != 0 falls back to k_denoise_coop).
 * An fp32 denoiser ignores 16; a bf16 engine without the W1 bias fold, or under dfx_debug_force_direct, takes the direct kernel
 * whatever the code.  All variants of one precision are bit-identical.
 * dfx_last_kernel_variant() (dfx.h) names the kernel a launch actually took. */
void dfx_debug_pipe_waves(int nw);
/* Debug / A-B switch: 1 makes a plain generation launch (dfx_sample_chain of a bf16 engine with in-kernel noise and no snapshots) take the
 * GENERAL instantiation of its chain kernel, whose mode selects are tested at run time, where it would take the PLAIN one, which has them
 * fixed at compile time (csrc/denoiser_kernel.hip: ChainKind); 0 = automatic (the default).  The two are bit-identical.
 * dfx_debug_last_chain_kind: "plain", "general" or "from" (partial chains) for the instantiation the last denoiser launch took, "" before
 * the first; dfx_last_kernel_variant() reports the same kernel name for all three. */
void dfx_debug_chain_general(int on);
const char *dfx_debug_last_chain_kind(void);
/* Host-side run (no GPU) of the launcher's planner (csrc/denoiser_plan.h): the name dfx_last_kernel_variant() would report after a denoiser
 * launch of B shapes of N points on an engine of precision `prec` (DFX_PREC_*) with / without the W1 bias fold, under dfx_debug_force_direct(force_direct)
 * and dfx_debug_pipe_waves(pipe_waves_code); *grid_out (may be NULL) = its workgroups.  A pure function of its arguments: the process-global
 * switches are not read. */
const char *dfx_debug_plan_variant(int prec, int w1_fold, int force_direct, int pipe_waves_code, int B, int N, long long *grid_out);
/* Host-side views (no GPU) of the bf16 feed-forward layout (csrc/denoiser_ff16.h).  dfx_debug_ff16_pack_w1 / _w2: what the pack kernels write
 * into a block's 17 x 12 x 1024-element streaming records for W1 (1024 x 128; gamma3, b1, beta3 as in the engine, fold = the W1 bias fold) and W2
 * (128 x 512), as fp32 before scale and rounding; layout 0 = the 32x32x16 A-operand order (the pack before the 16x16x32 feed-forward), 1 = the
 * 16x16x32 order the bf16 kernels read.  Elements that carry no weight are left untouched.  dfx_debug_ff16_slot_ops: the 24 fragments of a full
 * record's M slot in issue order, 5 ints each: {offset in 16-byte units from the lane's record pointer, GEMM (1 | 2), accumulator (0 = a,
 * 1 = g, -1 = h), M-tile, K step (GEMM1) or output tile of h (GEMM2)}. */
void dfx_debug_ff16_pack_w1(const float *W1, const float *g3, const float *b1, const float *be3, int fold, int layout, float *out);
void dfx_debug_ff16_pack_w2(const float *W2, int layout, float *out);
void dfx_debug_ff16_slot_ops(int32_t *out);
/* Slot-boundary clock stamps of two wavefronts of workgroup 0 (device buffer of 2*capacity uint64; NULL = off).
 * Only effective in a library built with -DDFX_TRACE (tools/experiments/trace_slots.py builds one). */
void dfx_debug_trace(void *device_buf, int capacity);
/* A dfx_latents handle with n_class / zdim / cimle / noise_dim set and no device memory (free with dfx_latents_destroy): the argument
 * checks of dfx_compose_latents run against it on a machine without a GPU; a call that passes them fails with "holds no weights". */
int dfx_debug_latents_stub(dfx_latents **out, int n_class, int zdim, int cimle, int noise_dim);
/* The unit draws dfx_part_box_pairwise_f32 makes without `units` for global pairs pair0 .. pair0+P-1: units (P,C,2,512,3) device. */
int dfx_debug_part_box_units(uint64_t seed, long long pair0, int P, int C, float *units, dfx_stream_t stream);
/* Host-side run (no GPU) of k_occupancy's per-point search, compiled from the kernel's own functions: the compact cell index of n HOST
 * points (n,3) on the grid of dfx_occupancy_grid_f32, -1 for a non-finite point. */
int dfx_debug_occupancy_host(const float *host_xyz, int n, int resolution, int in_sphere, int32_t *host_cell_index);
/* Host-side run (no GPU) of dfx_batch_build_f32, compiled from the kernel's own per-item routine: the same arguments as HOST
 * pointers, items one after the other, sums in index order.  An index outside [0,S) or an empty cloud is an error here. */
int dfx_debug_batch_build_host(const float *points, const int32_t *labels, const int64_t *offsets, int S, const int64_t *index, int B,
                               const int32_t *choice, const float *drop_u, const float *aug_u, int n_class, int npoints, int scale_mode,
                               int part_scale_mode, int clip, double dropout_part, int augment_shift, int augment_scale, float *ref,
                               float *input, int64_t *seg, int64_t *attn_map, float *present, float *dp_present, float *part_shift,
                               float *part_scale, float *shift, float *scale, int32_t *n_bad);
/* The normals dfx_part_draw_stats reduces, for global rows row0 .. row0+rows-1: normals (rows,n_draws,3,n_class) device. */
int dfx_debug_part_draw_normals(uint64_t seed, long long row0, int rows, int n_class, int n_draws, float *normals, dfx_stream_t stream);
/* Host-side runs (no GPU) of the selection routines of csrc/part_sampling.hip, compiled from the kernels' own functions, on HOST
 * pointers, groups one after the other: the scores of dfx_select_diverse from given stats; its greedy selection on given scores
 * (G K,6,n_class), with pick_dist (G,P) float64 or NULL = every pick's smallest distance to the picks before it; dfx_select_fit. */
int dfx_debug_part_scores_host(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int n_class,
                               float *scores);
int dfx_debug_select_diverse_host(const float *scores, const float *valid, int G, int K, int n_class, int P, int32_t *idx, double *pick_dist,
                                  int32_t *n_bad);
int dfx_debug_select_fit_host(const float *mean, const float *logvar, const float *target_mean, const float *target_logvar,
                              const float *weight, int G, int K, int n_class, int32_t *idx, float *fit, int32_t *n_bad);
/* The same for dfx_select_diverse_global's selection on given scores (G K,6,n_class): idx (P) global rows, pick_dist (P) float64 or
 * NULL = the winner's smallest distance to the picks before it (0 for pick 0 and for a non-finite pick, +inf for a pick that shares
 * no part with any earlier one). */
int dfx_debug_select_diverse_global_host(const float *scores, const float *valid, int G, int K, int n_class, int P, int rule, int32_t *idx,
                                         double *pick_dist, int32_t *n_bad);
/* Debug / A-B switch: 1 makes dfx_select_diverse_global (and dfx_part_search_global) run their selection as one launch per pick at every
 * size; any other value: automatic (default: one workgroup for the whole call up to 512 rows).  The picks are the same. */
void dfx_debug_diverse_global_path(int path);

#ifdef __cplusplus
}
#endif
#endif /* DFX_DEBUG_H */
