/* libdfx — MI355X-native (gfx950) kernels for DiffFacto's reverse-diffusion sampling hot path.
 *
 * C-ABI drop-in boundary.  Plain pointers and sizes only; every pointer is a
 * DEVICE pointer unless stated otherwise; every launch goes on the caller's HIP stream
 * (`stream` is a hipStream_t passed as void*; NULL = the default stream), no hidden syncs.
 * Inputs are borrowed, outputs are caller-allocated and fully written by the call (no
 * dependence on pre-zeroed outputs unless stated).  Return value: 0 = DFX_OK, negative =
 * error (never exit(), unlike the reference's CUDA_CHECK_ERRORS,
 * pointnet2_ops_lib/pointnet2_ops/_ext-src/include/cuda_utils.h:30-39); dfx_last_error() gives the
 * message for the calling thread.  Single caller thread per device.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repo root; SRC = pointnet2_ops_lib/pointnet2_ops/_ext-src/src).
 */
#ifndef DFX_H
#define DFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_OK 0
#define DFX_ERR_INVALID_ARG (-1)
#define DFX_ERR_HIP (-2)
#define DFX_ERR_UNSUPPORTED (-3)
#define DFX_ERR_ALLOC (-4)

#define DFX_MAX_DEPTH 8

/* arithmetic of the dense contraction (LayerNorm, softmax, GELU, posterior are fp32 in both) */
#define DFX_PREC_F32 0  /* v_mfma_f32_32x32x2_f32: exact fp32, the parity gate            */
#define DFX_PREC_BF16 1 /* v_mfma_f32_32x32x16 / 16x16x32: bf16 operands, fp32 accumulate */

typedef void *dfx_stream_t;
#define DFX_MAX_SIDE_STREAMS 64   /* see dfx_denoiser_train_forward */

int dfx_version(void);
/* Bumped whenever an existing entry point changes its argument list (round 2 inserted `shape_offset` into the four sampling
 * calls: 2; round 4 added dfx_last_kernel_variant: 3 — additive, bumped so that a binding written against 3 does not load a library without it;
 * round 5: d_x / d_variances of the denoiser backward: 4; round 6 added dfx_shared_mlp_train_*: 5).
 * Bindings compare dfx_abi_version() with the DFX_ABI_VERSION they were written against at load time (_ffi.py does)
 * instead of shifting arguments silently. */
#define DFX_ABI_VERSION 5
int dfx_abi_version(void);
const char *dfx_last_error(void);

/* ------------------------------------------------------------------------------------------
 * pointnet2_ops primitives — replace the pybind module `pointnet2_ops._ext`
 * (SRC/bindings.cpp:6-19); fp32 + int32, contiguous.
 * ------------------------------------------------------------------------------------------ */

/* _ext.gather_points  (SRC/sampling.cpp:15-38 -> SRC/sampling_gpu.cu:8-30)
 * out[b,c,j] = points[b,c,idx[b,j]];  points (B,C,N), idx (B,M) -> out (B,C,M) */
int dfx_gather_points_f32(const float *points, const int32_t *idx, float *out, int B, int C, int N, int M,
                          dfx_stream_t stream);

/* _ext.gather_points_grad  (SRC/sampling.cpp:40-64 -> SRC/sampling_gpu.cu:34-57)
 * grad_points (B,C,N) is ZEROED by the call, then scatter-added from grad_out (B,C,M). */
int dfx_gather_points_grad_f32(const float *grad_out, const int32_t *idx, float *grad_points, int B, int C, int N,
                               int M, dfx_stream_t stream);

/* _ext.furthest_point_sampling  (SRC/sampling.cpp:66-87 -> SRC/sampling_gpu.cu:69-229)
 * xyz (B,N,3) -> idx (B,M).  Starts at index 0, skips points with |p|^2 <= 1e-3, reproduces the
 * reference block-reduction tie rule for opt_n_threads(N) threads.  `tmp` (B,N) floats is scratch
 * (the reference's `temp`, filled with 1e10 by the call); may be NULL when N <= dfx_fps_max_resident(). */
int dfx_furthest_point_sampling_f32(const float *xyz, float *tmp, int32_t *idx, int B, int N, int M,
                                    dfx_stream_t stream);
int dfx_fps_max_resident(void);

/* _ext.ball_query  (SRC/ball_query.cpp:8-32 -> SRC/ball_query_gpu.cu:9-54)
 * new_xyz (B,M,3), xyz (B,N,3) -> idx (B,M,nsample): first `nsample` indices k (ascending) with
 * d2 < radius^2; first hit pre-fills all slots; no hit -> zeros.  Argument order is the C++ op's. */
int dfx_ball_query_f32(const float *new_xyz, const float *xyz, int32_t *idx, int B, int N, int M, float radius,
                       int nsample, dfx_stream_t stream);

/* _ext.group_points  (SRC/group_points.cpp:12-36 -> SRC/group_points_gpu.cu:8-39)
 * out[b,c,j,k] = points[b,c,idx[b,j,k]];  points (B,C,N), idx (B,npoints,nsample). */
int dfx_group_points_f32(const float *points, const int32_t *idx, float *out, int B, int C, int N, int npoints,
                         int nsample, dfx_stream_t stream);

/* _ext.group_points_grad  (SRC/group_points.cpp:38-62 -> SRC/group_points_gpu.cu:43-75); zeroes grad_points. */
int dfx_group_points_grad_f32(const float *grad_out, const int32_t *idx, float *grad_points, int B, int C, int N,
                              int npoints, int nsample, dfx_stream_t stream);

/* _ext.three_nn  (SRC/interpolate.cpp:14-40 -> SRC/interpolate_gpu.cu:9-68)
 * unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3) SQUARED distances, idx (B,n,3). */
int dfx_three_nn_f32(const float *unknown, const float *known, float *dist2, int32_t *idx, int B, int n, int m,
                     dfx_stream_t stream);

/* _ext.three_interpolate (SRC/interpolate.cpp:42-70 -> SRC/interpolate_gpu.cu:72-111)
 * points (B,c,m), idx (B,n,3), weight (B,n,3) -> out (B,c,n). */
int dfx_three_interpolate_f32(const float *points, const int32_t *idx, const float *weight, float *out, int B,
                              int c, int m, int n, dfx_stream_t stream);

/* _ext.three_interpolate_grad (SRC/interpolate.cpp:72-99 -> SRC/interpolate_gpu.cu:116-154); zeroes grad_points (B,c,m). */
int dfx_three_interpolate_grad_f32(const float *grad_out, const int32_t *idx, const float *weight,
                                   float *grad_points, int B, int c, int n, int m, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Cross-diffusion denoiser + anchored DDPM reverse process.
 * Replaces, for the shipped gen_* configs (inner 128 = 8 heads x 16, n_class 4, ctx 522,
 * GEGLU FF 128 -> 2*512 -> 128, single cross-attention per block):
 *   TransformerNet.forward        python/difffacto/models/diffusions/nets/attention.py:385-440
 *   AnchoredDiffusion.p_mean_variance / p_sample / p_sample_loop_progressive
 *                                 python/difffacto/models/diffusions/anchored_diffusion.py:227-395,450-484,528-588
 *   gather_operation of the per-part params (part_encoders.py:417-428) — folded in: the kernels
 *   index the (B,3,4) part params by `seg` instead of materialising (B,3,N) tensors.
 * ------------------------------------------------------------------------------------------ */

/* fp32 device pointers to the reference parameters (torch Linear layout: weight (out,in)),
 * named by their state_dict keys relative to `diffusion.model.`. */
typedef struct dfx_block_weights {
  const float *norm2_w, *norm2_b;   /* transformer_blocks.i.norm2.{weight,bias}      (128)     */
  const float *to_q;                /* ...attn2.to_q.weight                          (128,128) */
  const float *to_k, *to_v;         /* ...attn2.to_{k,v}.weight                      (128,522) */
  const float *to_out_w, *to_out_b; /* ...attn2.to_out.0.{weight,bias}               (128,128),(128) */
  const float *norm3_w, *norm3_b;   /* ...norm3.{weight,bias}                        (128)     */
  const float *ff0_w, *ff0_b;       /* ...ff.net.0.proj.{weight,bias}                (1024,128),(1024) */
  const float *ff2_w, *ff2_b;       /* ...ff.net.2.{weight,bias}                     (128,512),(128) */
} dfx_block_weights;

typedef struct dfx_denoiser_weights {
  int depth;                          /* number of transformer blocks (<= DFX_MAX_DEPTH)  */
  const float *proj_in_w, *proj_in_b; /* proj_in.{weight,bias}            (128,13),(128)  */
  const float *pre_norm_w, *pre_norm_b;
  const float *post_norm_w, *post_norm_b;
  const float *proj_out_w, *proj_out_b; /* proj_out.{weight,bias}         (3,128),(3)     */
  const float *te0_w, *te0_b;           /* time_embed.net.0.proj.{weight,bias} (2048,256),(2048) */
  const float *te2_w, *te2_b;           /* time_embed.net.2.{weight,bias}      (256,1024),(256)  */
  dfx_block_weights blk[DFX_MAX_DEPTH];
} dfx_denoiser_weights;

typedef struct dfx_denoiser dfx_denoiser; /* opaque; owns repacked weights + per-t tables on the device */

/* Build the frozen denoiser for one diffusion schedule (AnchoredDiffusion.__init__,
 * anchored_diffusion.py:62-112, mode='linear'): repacks weights into MFMA fragment order for
 * `precision`, tabulates the time-embedding MLP and the per-t attention/posterior constants for
 * t = 0..num_timesteps-1.  The source parameters are only read during this call (stream-ordered:
 * keep them alive until the stream has passed it). */
int dfx_denoiser_create(dfx_denoiser **out, const dfx_denoiser_weights *w, int num_timesteps, double beta_1,
                        double beta_T, int precision, dfx_stream_t stream);
void dfx_denoiser_destroy(dfx_denoiser *d);
int dfx_denoiser_num_timesteps(const dfx_denoiser *d);
int dfx_denoiser_precision(const dfx_denoiser *d);
/* DFX_PREC_BF16 engines: 1 if b1' = b1 + W1 beta3 rides in one hidden channel's K slot of the packed W1 (no accumulator initialisers in the chain
 * kernels; exact in real arithmetic — a LayerNorm output sums to zero, so one channel is redundant — and every weight of a row then rounds with a
 * step that follows that channel's column of W1 diag(gamma3)).  Create picks the channel from the weights: 127, or — when 127's column is an
 * outlier (ratio > 4 of its row's mean magnitude) — the channel with the smallest column over all blocks, exchanged with 127 in a private copy
 * of the parameters (a relabelling of the hidden channels: the same function).  0 only if every channel is an outlier of some block (ratio > 8):
 * the engine then has the plain pack and runs the direct kernel (~3x slower).  *ratio (may be NULL) receives the chosen channel's ratio.
 * fp32 engines: 0. */
int dfx_denoiser_w1_fold(const dfx_denoiser *d, float *ratio);

/* Copies the 8 fp32 schedule tables the kernels use to HOST memory, each `num_timesteps` long, in the
 * order: sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, _coef2, _coef3,
 * posterior_variance, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod  (out: host float[8*T]). */
int dfx_denoiser_get_tables(const dfx_denoiser *d, float *host_out);

/* Per-batch static context (once per batch of shapes, before the T-loop): the 4 part tokens'
 * K/V projections folded with to_q / to_out and the per-part proj_in constants.
 *   part_code (B,256,4)  mean (B,3,4)  var (B,3,4) = exp(logvar)   [ctx list of prepare_ctx,
 *   part_encoders.py:1317-1326]   valid (B,4) floats (mask of attention.py:192-197)
 * `ctx_out` is a caller-allocated device buffer of dfx_shape_ctx_bytes(d, B) bytes.
 * The context is opaque: it is consumed by the library that prepared it, with the `valid` it was prepared with.  The context of a bf16
 * engine carries the key mask inside its attention operands (the similarity bias of an absent part is -FLT_MAX) and its kernels no longer
 * read `valid` for the softmax, so a context written by an earlier library version must be prepared again, and a change of `valid` means
 * a new dfx_shape_ctx_prepare, as it always did.  The context of an fp32 engine is what it was. */
size_t dfx_shape_ctx_bytes(const dfx_denoiser *d, int B);
int dfx_shape_ctx_prepare(const dfx_denoiser *d, const float *part_code, const float *mean, const float *var,
                          const float *valid, void *ctx_out, int B, dfx_stream_t stream);

/* One TransformerNet.forward: eps (B,3,N) = eps_theta(x (B,3,N), t) with anchors/variances/one-hot
 * taken from the shape context through seg (B,N) int32 in [0,4).  N % 32 == 0.  `t` is the same for
 * the whole batch (anchored_diffusion.py:576). */
int dfx_denoise_eps(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, int t,
                    float *eps, int B, int N, dfx_stream_t stream);

/* One p_sample (anchored_diffusion.py:450-484): x_prev = mean + 1[t!=0] sqrt(var) z.
 * noise (B,3,N) = the z of :476, or NULL -> in-kernel Philox4x32-10 normals keyed by
 * (seed, global point id, t), global point id = (shape_offset + b) * N + n: `shape_offset` is the global index of this
 * call's shape 0, so a batch that is split over several calls or GPUs draws exactly the normals of
 * the unsplit call, whatever the split.  x_prev may alias x.  pred_xstart (B,3,N) is optional (NULL to skip):
 * the x_0 prediction p_sample returns next to the sample (:484). */
int dfx_p_sample(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, int t,
                 const float *noise, uint64_t seed, uint64_t shape_offset, float *x_prev, float *pred_xstart, int B, int N,
                 dfx_stream_t stream);

/* The whole reverse chain in ONE persistent launch (p_sample_loop_progressive :528-588 driven by
 * AnchorDiffAE.decode, python/difffacto/models/networks/anchor_gen.py:145-169): x_t stays in registers
 * for all T steps.
 *   x_T_noise  (B,3,N) the randn of :564, or NULL -> Philox
 *   step_noise (T,B,3,N), step_noise[i] = z of the i-th executed step (t = T-1-i), or NULL -> Philox
 *   seed, shape_offset  Philox key and global index of shape 0 (see dfx_p_sample): rank r of a sharded run passes the
 *              index of its first shape, and the clouds do not depend on the number of GPUs
 *   pred       (B,N,3)  final cloud, already transposed like decode's 'pred'
 *   traj       NULL, or (n_keep,B,N,3) snapshots for t = T, then every t>0 with t % ret_interval == 0 in
 *              descending order (decode's ret_traj entries); n_keep = dfx_chain_num_snapshots(T, ret_interval). */
int dfx_chain_num_snapshots(int num_timesteps, int ret_interval);
int dfx_sample_chain(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x_T_noise,
                     const float *step_noise, uint64_t seed, uint64_t shape_offset, int ret_interval, float *traj, float *pred,
                     int B, int N, dfx_stream_t stream);

/* Training-style forward evaluation (forward only; anchored_diffusion.py:760-853 in eval mode):
 *   dfx_q_sample_f32    x_t = sqrt_acp[t_b] (x0 - a) + a + sqrt(1 - acp[t_b]) L noise   (:148-173), t (B,) int32 on the device
 *   dfx_denoise_eps_t   dfx_denoise_eps with one timestep per shape
 *   dfx_masked_mse_f32  ((target - pred)^2 * flags).mean(1).sum() / flags.sum()  (:840-847; flags (B,N) or NULL = plain mean);
 *                       workspace2 = 2 doubles on the device, loss = 1 float on the device
 * Dropout and gradients are not part of this path. */
int dfx_q_sample_f32(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const int32_t *t, const float *x_start,
                     const float *noise, float *x_t, int B, int N, dfx_stream_t stream);
int dfx_denoise_eps_t(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, const int32_t *t,
                      float *eps, int B, int N, dfx_stream_t stream);
int dfx_masked_mse_f32(const float *target, const float *pred, const float *flags, double *workspace2, float *loss, int B,
                       int N, dfx_stream_t stream);

/* DDIM branch (anchored_diffusion.py:114-124 step lists, :368-377 xt_dir, :480-481 update):
 *   x_prev = (x0 - a) sqrt(acp_prev[t]) + a + L xt_dir_coeff[t] eps + eta 1[t != 0] sqrt(variance) z,
 *   xt_dir_coeff = sqrt(1 - acp - eta^2 posterior_variance) (float64 on the host).
 * `steps` is a HOST array, ascending like the reference's self.steps (e.g. 'quad': [0,0,2,5,10,16,23,32]); it is
 * executed in reverse; n_steps <= 128; steps[0] must be 0 for the chain.  step_noise is (n_steps,B,3,N) or NULL.
 * traj slot k still means t = (T / ret_interval - k) * ret_interval; slots of timesteps that are not visited are
 * left untouched. */
int dfx_p_sample_ddim(const dfx_denoiser *d, const void *shape_ctx, const float *x, const int32_t *seg, int t, float eta,
                      const float *noise, uint64_t seed, uint64_t shape_offset, float *x_prev, float *pred_xstart, int B, int N,
                      dfx_stream_t stream);
int dfx_sample_chain_ddim(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const int32_t *steps,
                          int n_steps, float eta, const float *x_T_noise, const float *step_noise, uint64_t seed,
                          uint64_t shape_offset, int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream);

/* Partial reverse chains (dfx_version() >= 108): the LAST n_steps timesteps, n_steps-1 .. 0, from a caller's cloud instead of from pure noise —
 * variations of a cloud at a chosen strength, cleaning a noisy cloud, resuming from a snapshot.  1 <= n_steps <= T.  The step arithmetic is
 * dfx_sample_chain's (the same kernels, instantiated with another prologue), so resuming a chain from one of its own snapshots with the same
 * seed continues it bit for bit.
 *   dfx_sample_chain_from       x_init (B,3,N) is the state entering timestep n_steps-1.  Snapshots are labelled by the timestep that has just
 *                               run: traj slot k holds the state AFTER timestep t = (T / ret_interval - k) * ret_interval, so resuming from the
 *                               slot labelled t takes n_steps = t; slot 0 (t = T, when ret_interval divides T) is the first state and takes n_steps = T.
 *   dfx_refine_chain            x_start (B,3,N) is a CLEAN cloud: the prologue forward-noises it to t = n_steps-1,
 *                               x = sqrt_acp[t] (x0 - a) + a + sqrt(1 - acp[t]) L z, in dfx_q_sample_f32's operation order — the result is bit-identical
 *                               to dfx_q_sample_f32 followed by dfx_sample_chain_from.  start_noise (B,3,N) = z, or NULL -> Philox.
 *   dfx_sample_chain_ddim_from  DDIM over the ascending HOST list `steps` (steps[0] == 0, every entry < T), executed in reverse from
 *                               x_init, the state entering timestep steps[n-1]: the tail of a longer DDIM chain's list resumes that chain.
 *   step_noise  (n_steps,B,3,N) / (n,B,3,N), step_noise[i] = z of the i-th EXECUTED step (t = n_steps-1-i), or NULL -> Philox
 *   hold        NULL, or (B,) int32 on the device: bit j set = the points of part j (seg == j) are HELD — wherever the chain writes such a
 *               point, in pred and in every snapshot, it writes the caller's x_init / x_start coordinates.  Held points still run through
 *               the network (a point's update does not depend on other points, so the others are what they are without `hold`).
 *   traj        NULL, or the (n_keep,B,N,3) buffer of dfx_sample_chain with the same slot meaning; only the slots of executed timesteps are written
 *               (t <= n_steps-1, or the list's entries), the others are left untouched.  The t = T slot is written by dfx_sample_chain_from with
 *               n_steps == T only; never by dfx_refine_chain (its first state is not a snapshot of anything) or the DDIM form.
 * Philox keys, (seed, global point id, counter word, stream), global point id = (shape_offset + b) * N + n:
 *     step noise of timestep t            (t, 0)          every chain entry point
 *     x_T draw of dfx_sample_chain[_ddim] (T, 1)
 *     start noise of dfx_refine_chain     (n_steps, 1)    stream 1 like the x_T draw (n_steps = T is that draw): never a step-noise counter */
int dfx_sample_chain_from(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x_init, int n_steps,
                          const float *step_noise, uint64_t seed, uint64_t shape_offset, const int32_t *hold, int ret_interval,
                          float *traj, float *pred, int B, int N, dfx_stream_t stream);
int dfx_refine_chain(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const float *x_start, int n_steps,
                     const float *start_noise, const float *step_noise, uint64_t seed, uint64_t shape_offset, const int32_t *hold,
                     int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream);
int dfx_sample_chain_ddim_from(const dfx_denoiser *d, const void *shape_ctx, const int32_t *seg, const int32_t *steps, int n_steps,
                               float eta, const float *x_init, const float *step_noise, uint64_t seed, uint64_t shape_offset,
                               const int32_t *hold, int ret_interval, float *traj, float *pred, int B, int N, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Chamfer-L2 — replaces the `chamfer` extension
 * (python/difffacto/metrics/chamfer_dist/chamfer.cu: forward :15-170, backward :173-230; bound in
 * python/difffacto/metrics/chamfer_dist/__init__.py:14-27).
 * ------------------------------------------------------------------------------------------ */

/* chamfer.forward(xyz1 (B,N,3), xyz2 (B,M,3)) -> dist1 (B,N), dist2 (B,M) squared NN distances, idx1, idx2 int32 */
int dfx_chamfer_forward_f32(const float *xyz1, const float *xyz2, float *dist1, float *dist2, int32_t *idx1,
                            int32_t *idx2, int B, int N, int M, dfx_stream_t stream);

/* chamfer.backward(...) -> grad_xyz1 (B,N,3), grad_xyz2 (B,M,3); both zeroed by the call, atomics like the reference */
int dfx_chamfer_backward_f32(const float *xyz1, const float *xyz2, const int32_t *idx1, const int32_t *idx2,
                             const float *grad_dist1, const float *grad_dist2, float *grad_xyz1, float *grad_xyz2,
                             int B, int N, int M, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Part-level generation metrics — the gen_part evaluation of python/difffacto/datasets/evaluation_utils.py
 * (compute_snapping_metric :385-421, the box step of compute_bbox_metric :287-333 and its part_l2 / part_miou /
 * part_chamfer distances :23-82, the extraction step of compute_part_metric :423-486).  part_metrics.hip.
 * xyz (B,N,3) fp32, labels (B,N) int32 with 1 <= N <= 8192; a label outside [0,C) belongs to no part.  Every argument is
 * checked on the host before the first HIP call.
 * ------------------------------------------------------------------------------------------ */

/* Snapping distance of P part pairs per shape (k = 50 in the reference).  pairs: HOST int32 (P,2) = (a,b) in [0,C), 1 <= P <= 64.
 * Per (shape, pair): d(p,q) = (dx*dx + dy*dy) + dz*dz, no contraction (torch's CPU sum of squares); every point of part a gets its
 * minimum d to part b and vice versa; the k points of each part with the smallest minima are kept (equal minima: the lower point
 * index wins; torch's topk leaves the order of ties unspecified); dist = Chamfer of the two k-point sets (mean nearest-neighbour d in
 * each direction, summed).  Outputs dist (B,P) fp32, status (B,P) int32: 0 = part a or b has no point (dist NaN), 1 = computed,
 * 2 = a present part has fewer than k points (dist NaN; the reference's topk raises). */
int dfx_part_snapping_f32(const float *xyz, const int32_t *labels, int B, int N, int C, const int32_t *pairs, int P, int k,
                          float *dist, int32_t *status, dfx_stream_t stream);

/* Part bounding boxes.  normalize != 0: the shape is first mapped to (x - (min+max)/2) / (largest extent / 2).  Per part with
 * count > min_points (>= 0): lo = quantile(1 - q), hi = quantile(q) per axis with torch.quantile's linear interpolation (q and 1 - q
 * rounded to fp32 from double; pos = q (n-1), lerp between the floor and ceil order statistics); q = 1 gives the exact min / max.
 * q in [0,1].  Outputs boxes (B,C,2,3) = (lo, hi) (NaN for parts not kept), count (B,C) = points per part. */
int dfx_part_boxes_f32(const float *xyz, const int32_t *labels, int B, int N, int C, int normalize, int min_points, double q,
                       float *boxes, int32_t *count, dfx_stream_t stream);

/* Part clouds.  Per part with count n > min_points: point p < n_out is part point (p mod n) in index order (the reference's "repeat
 * until >= n_out, truncate"), then per axis x <- (x - (min+max)/2) / ((max-min)/2) over those n_out points.  mask[p] = p < n.
 * 1 <= n_out <= 4096 (512 in the reference).  Outputs clouds (B,C,n_out,3), masks (B,C,n_out) (zeros for parts not kept), count (B,C). */
int dfx_part_clouds_f32(const float *xyz, const int32_t *labels, int B, int N, int C, int min_points, int n_out, float *clouds,
                        float *masks, int32_t *count, dfx_stream_t stream);

/* Box-set distance matrix D (Ma,Mb), D[i,j] = dist(A_i, B_j): boxes (M,C,2,3) as dfx_part_boxes_f32 writes them, present (M,C) int32
 * (nonzero = the part has a box).  Per pair the classes are walked in order: presence differs -> +inf; both absent -> skipped;
 * else a term; D = fp32 mean of the terms (NaN without any).  metric 0 = l2 (mean squared difference of [(hi-lo)/2, (hi+lo)/2]),
 * 1 = iou (1 - mean IoU in double, boxes read as the reference's get_3d_box at heading 0 reads (l,w,h): x-extent dx, y-extent dz,
 * z-extent dy), 2 = chamfer (512 points uniform in each box, u (hi-lo) + lo, then Chamfer-L2).  Chamfer draws: units (P,C,2,512,3)
 * device, P = Ma*Mb local pairs i*Mb + j, side 0 = A; or units NULL = Philox4x32-10 keyed by seed, counter (point, 0xB0C50000 | class*2 + side,
 * global pair (row0 + i)*Mb + j, low word first; DESIGN.md "Random streams"): any split of the rows into launches gives the same matrix. */
int dfx_part_box_pairwise_f32(const float *boxes_a, const int32_t *present_a, int Ma, const float *boxes_b,
                              const int32_t *present_b, int Mb, int C, int metric, uint64_t seed, long long row0,
                              const float *units, float *D, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Occupancy-grid JSD — unit_cube_grid_point_cloud, entropy_of_occupancy_grid, jensen_shannon_divergence and
 * jsd_between_point_cloud_sets of python/difffacto/datasets/evaluation_utils.py:544-648.  occupancy.hip, DESIGN.md §5.9.
 * The grid: R = resolution in [2,40] cells per axis, axis value a[i] = float32(i * (1.0 / (R - 1)) - 0.5) (product and
 * difference in double); with in_sphere a cell (i,j,k) is kept when the float32 sqrt((x*x + y*y) + z*z) <= 0.5f (numpy's norm of a
 * float32 row, no contraction); kept cells are numbered in C order over (i,j,k): the compact index.  A point belongs to the
 * kept cell with the smallest (dx*dx + dy*dy) + dz*dz, coordinates widened to double and every operation rounded to double
 * (sklearn's KD-tree on the same grid); an exact tie goes to the lower compact index.
 * ------------------------------------------------------------------------------------------ */

/* Number of kept cells (host only; no GPU call).  < 0 on error (resolution outside [2,40]). */
int dfx_occupancy_num_cells(int resolution, int in_sphere);

/* The keep mask, HOST uint8 (R,R,R) in C order: 1 = kept (host only; no GPU call). */
int dfx_occupancy_cell_mask(int resolution, int in_sphere, uint8_t *host_mask);

/* Counts the points of B clouds xyz (B,N,3) into the grid.  rows = C + 1 with labels (int32 (B,N), 0 <= C <= 16), else 1 (labels
 * NULL, C ignored): row 0 takes every point, row 1 + c the points labelled c; a label outside [0,C) counts in row 0 only.
 * counters int64 (rows,cells): points per cell.  bernoulli int32 (rows,cells): clouds with at least one point in the cell.
 * cell_index int32 (B,N), nullable: the compact index per point.  A point with a non-finite coordinate is counted nowhere but in
 * n_bad (int32, 1) and gets cell_index -1.  accumulate == 0: counters, bernoulli and n_bad are zeroed first; != 0: added to, so
 * a large set can be fed in chunks.  Integer counting: the result does not depend on scheduling.  The first call per
 * (device, resolution, in_sphere) allocates the grid's column table (at most 6.7 KB, kept for the life of the process) and uploads
 * it with a blocking copy; on a capturing stream that first call is refused (make one call outside the capture first).  Fails for
 * a grid without kept cells (R = 2 with in_sphere). */
int dfx_occupancy_grid_f32(const float *xyz, const int32_t *labels, int B, int N, int C, int resolution, int in_sphere,
                           int accumulate, int64_t *counters, int32_t *bernoulli, int32_t *cell_index, int32_t *n_bad,
                           dfx_stream_t stream);

/* jsd (double, 1) = H((P+Q)/2) - (H(P) + H(Q))/2 in bits, P = counters_p / sum, Q = counters_q / sum (rows of `cells` int64);
 * fixed-order fp64 sums: bit-reproducible, and exactly 0 for equal rows.  NaN when a row sums to 0. */
int dfx_occupancy_jsd_f64(const int64_t *counters_p, const int64_t *counters_q, int cells, double *jsd, dfx_stream_t stream);

/* entropy (double, 1) = sum over cells with bernoulli > 0 of H([p, 1 - p]) in nats, p = bernoulli / n_shapes, divided by cells. */
int dfx_occupancy_entropy_f64(const int32_t *bernoulli, int cells, int64_t n_shapes, double *entropy, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-batch assembly — _ShapeNetSegParts.__getitem__ (python/difffacto/datasets/shapenet_seg.py:436-543) with pc_norm
 * (dataset_utils.py:55-95), over a device-resident ragged set: points (P,3) float32, labels (P) int32, offsets (S+1) int64 (cloud s
 * is rows offsets[s] .. offsets[s+1]-1).  batch_kernels.hip, DESIGN.md §5.10.  index (B) int64 picks the clouds.
 * Scale modes: 0 none, 1 shape_unit, 2 shape_half, 3 shape_34, 4 shape_bbox (scale_mode and part_scale_mode), 5 shape_canonical,
 * 6 shape_canonical_bbox (part_scale_mode only).  1 <= n_class <= 8, 10 <= npoints <= 8192.
 * ------------------------------------------------------------------------------------------ */

/* The random inputs of a batch from Philox4x32-7: key = seed, counter = (group of four values, purpose, sample_id[b]), so an item's
 * draws depend on (seed, sample_id[b]) only, not on its row or on B.  choice int32 (B,N) = (u32 * M) >> 32 with M the size of cloud
 * index[b] (bias < M / 2^32 per value; all 0 for an index outside [0,S) or an empty cloud, which dfx_batch_build_f32 reports);
 * drop_u float32 (B,C) and aug_u float32 (B,6): 24-bit uniforms in [0,1). */
int dfx_batch_draw(const int64_t *offsets, int S, const int64_t *index, const int64_t *sample_id, int B, int N, int C, uint64_t seed,
                   int32_t *choice, float *drop_u, float *aug_u, dfx_stream_t stream);

/* Assembles B items, one 256-thread workgroup each, 16 * npoints bytes of LDS.  Per item: gather points / labels at choice; shape
 * normalisation (fp64 mean, two-pass variance and bounds, rounded once; ref = (x - shift) / scale in float32); for part i = 0..C-1
 * on the CURRENT labels: with >= 10 points its statistics, present = 0 when an axis std is exactly zero, pc_norm with
 * part_scale_mode (clip to [1e-2,1] when clip, then a zero scale becomes 1) and the part's input rows; with 1..9 points every point
 * takes the label of its nearest point outside the part (float32 ((dx*dx) + dy*dy) + dz*dz, first minimum), present 0, shift 0,
 * scale 1.  dp_present = present, 0 where drop_u < dropout_part.  With augment_shift / augment_scale: rand_scale = aug_u[0:3] / 2 + 0.7,
 * rand_shift = aug_u[3:6] - 0.5 (ones / zeros for the one that is off), ref = (ref + rand_shift) * rand_scale,
 * shift += scale * rand_shift, scale = rand_scale * scale.
 * Outputs: ref, input float32 (B,N,3); seg int64 (B,N); attn_map int64 (B,N,C) one-hot; present, dp_present float32 (B,C);
 * part_shift, part_scale float32 (B,3,C); shift float32 (B,3); scale float32 (B,3) (three equal values without augmentation).
 * n_bad int32 (2), zeroed first: [0] sampled labels outside [0,C) (their one-hot row is zero), [1] items whose index is outside
 * [0,S), whose cloud is empty (their output rows are not written) or that hold a choice outside [0,M) (read as 0).
 * Bit-reproducible: fixed-order fp64 sums, no floating-point atomics. */
int dfx_batch_build_f32(const float *points, const int32_t *labels, const int64_t *offsets, int S, const int64_t *index, int B,
                        const int32_t *choice, const float *drop_u, const float *aug_u, int n_class, int npoints, int scale_mode,
                        int part_scale_mode, int clip, double dropout_part, int augment_shift, int augment_scale, float *ref,
                        float *input, int64_t *seg, int64_t *attn_map, float *present, float *dp_present, float *part_shift,
                        float *part_scale, float *shift, float *scale, int32_t *n_bad, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Latent sampler — the once-per-batch producer of decode's inputs:
 * PartEncoder.sample_latents (python/difffacto/models/encoders/part_encoders.py:1052-1110) =
 * per-part normalising flows run in reverse (python/difffacto/models/encoders/flow.py:21-47,58-72)
 * + PartAlignerTransformer (part_encoders.py:20-143) + seg-mask ids / per-point gathers
 * (part_encoders.py:1105-1108, :417-428) + PartEncoderForTransformerDecoder.prepare_ctx (:1317-1326).
 * fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32); supported configuration = the shipped gen configs
 * (class_cond + add_class_cond, use_linear, single_attn, cimle with cond_noise_type 0, or no cimle).
 * ------------------------------------------------------------------------------------------ */
typedef struct dfx_aligner_block_weights { /* BasicTransformerBlock(single_attn) of the aligner, device pointers */
  const float *norm2_w, *norm2_b;   /* (inner) */
  const float *to_q, *to_k, *to_v;  /* (inner, inner), bias-free */
  const float *to_out_w, *to_out_b; /* (inner, inner), (inner) */
  const float *norm3_w, *norm3_b;
  const float *ff_proj_w, *ff_proj_b; /* (8*inner, inner), (8*inner): GEGLU */
  const float *ff_out_w, *ff_out_b;   /* (inner, 4*inner), (inner) */
} dfx_aligner_block_weights;

typedef struct dfx_latent_weights {
  int32_t n_class, zdim;                /* 4, 256 */
  int32_t flow_depth, flow_hidden;      /* 14, 256; flow_depth 0 = use_flow False */
  /* host array of n_class*flow_depth*6 device pointers, [part][layer][w0,b0,w1,b1,w2,b2] = net_s_t.{0,2,4} */
  const float *const *flow;
  int32_t depth, n_heads, d_head;       /* 5, 8, 32 */
  int32_t cimle, noise_dim;             /* 1, 32 (cond_noise_type 0: noise*noise_scale concatenated per token) */
  float noise_scale, prior_var, log_scale_var;
  const float *proj_in_w, *proj_in_b;   /* (inner, zdim + cimle*noise_dim) */
  const float *class_emb;               /* (n_class, inner) */
  const float *pre_norm_w, *pre_norm_b; /* applied only when !cimle (part_encoders.py:115-131) */
  const float *post_norm_w, *post_norm_b;
  const float *proj_out_w, *proj_out_b; /* (6, inner) */
  dfx_aligner_block_weights blocks[DFX_MAX_DEPTH];
} dfx_latent_weights;

typedef struct dfx_latents dfx_latents; /* opaque; owns a copy of the weights + a grow-only workspace */

int dfx_latents_create(dfx_latents **out, const dfx_latent_weights *w, dfx_stream_t stream);
void dfx_latents_destroy(dfx_latents *h);

/* flow[i](w[..., i], reverse=True) for every part (part_encoders.py:1054-1060):
 * w (S,zdim,n_class) standard normal -> part_code (S,zdim,n_class); w is scaled by sqrt(prior_var) first. */
int dfx_flow_reverse(dfx_latents *h, const float *w, float *part_code, int S, dfx_stream_t stream);

/* PartAlignerTransformer.forward (part_encoders.py:88-109): part_code (B,zdim,n_class), valid_id (B,n_class)
 * {0,1} floats = the key mask, noise (B,noise_dim) (NULL iff !cimle) -> mean (B,3,n_class), logvar (B,3,n_class). */
int dfx_part_aligner(dfx_latents *h, const float *part_code, const float *valid_id, const float *noise, float *mean,
                     float *logvar, int B, dfx_stream_t stream);

/* The whole sample_latents after the random draws (part_encoders.py:1052-1110; no selective sampling):
 *   w_noise (S,zdim,n_class) randn of :1054, or part_code_in (S,zdim,n_class) given codes (then w_noise NULL)
 *   aligner_noise (S*K,noise_dim) randn of :1065 (NULL iff !cimle; then K must be 1)
 *   valid_id (S,n_class); fixed_id: HOST array of n_class 0/1 flags (:1072-1082)
 * outputs, R = S*K rows (any may be NULL to skip, except those the chain needs):
 *   part_code (R,zdim,n_class), valid_out (R,n_class), noise_out (R,noise_dim), mean/logvar (R,3,n_class),
 *   params (R,6,n_class) = [mean | exp(logvar + log_scale_var)] (= ctx[1]), seg (R,npoints) int32,
 *   mean_per_point / logvar_per_point (R,3,npoints) (logvar_per_point includes log_scale_var). */
int dfx_sample_latents(dfx_latents *h, const float *w_noise, const float *part_code_in, const float *aligner_noise,
                       const float *valid_id, const int32_t *fixed_id, int S, int K, int npoints, float *part_code,
                       float *valid_out, float *noise_out, float *mean, float *logvar, float *params, int32_t *seg,
                       float *mean_per_point, float *logvar_per_point, dfx_stream_t stream);

/* Editing front end (shape interpolation, part mixing, anchor drift; anchor_gen.py:206-532): dfx_sample_latents' outputs from an
 * explicit recipe instead of a sampling rule, R output rows over S source shapes.
 *   code_src (S,zdim,n_class) device: source part codes
 *   code_a, code_b: HOST int32 (R,n_class): source rows per output row and part.  code_b NULL (then alpha NULL too) or an entry
 *     -1 = copy src[a] with no arithmetic (-0 stays -0); else code[r,:,j] = src[a] + (src[b] - src[a]) * alpha[r,j], three
 *     separately rounded fp32 operations (anchor_gen.py:244): the bits of torch's three elementwise ops.
 *   alpha (R,n_class) device or NULL; valid (R,n_class) device: the final key mask of every row (built by the caller)
 *   noise_src (Sn,noise_dim) device + noise_row HOST int32 (R) or NULL = identity (then Sn >= R); both NULL iff !cimle
 *   mean_scale / logvar_shift (R,3,n_class) device or NULL: after the aligner, mean <- mean * s and logvar <- logvar + l, before
 *     params and the per-point gathers are written (interpolate_params, anchor_gen.py:369-370)
 *   seg_mode 0: ids = arange*valid + argmax(valid)*(1-valid) (as dfx_sample_latents); 1: ids = arange*valid
 *     (combine_latent_specific, :437); 2: seg[r] = seg_src[seg_row[r]] with seg_src (Ss,npoints) device int32 ids in
 *     [0,n_class) and seg_row HOST int32 (R) (both NULL for modes 0 / 1)
 * outputs as dfx_sample_latents (no valid_out: the caller's `valid` is the mask): part_code (R,zdim,n_class), noise_out
 * (R,noise_dim), mean / logvar (R,3,n_class), params (R,6,n_class), seg (R,npoints), mean_per_point / logvar_per_point
 * (R,3,npoints).  Every argument, index maps included, is checked before the first HIP call. */
int dfx_compose_latents(dfx_latents *h, const float *code_src, int S, const int32_t *code_a, const int32_t *code_b,
                        const float *alpha, const float *valid, const float *noise_src, int Sn, const int32_t *noise_row,
                        const float *mean_scale, const float *logvar_shift, int seg_mode, const int32_t *seg_src, int Ss,
                        const int32_t *seg_row, int R, int npoints, float *part_code, float *noise_out, float *mean,
                        float *logvar, float *params, int32_t *seg, float *mean_per_point, float *logvar_per_point,
                        dfx_stream_t stream);

/* ---- Part-level sampling (AnchorDiffAE.sample_one_part, anchor_gen.py:307-337; PartEncoder.sample_with_fixed_latents,
 * part_encoders.py:623-710; subsample_params :545-589): new styles for one part, and a search over K aligner noises
 * per style for configurations to go with them.  Candidate row g K + k is candidate k of group g; all data pointers are device
 * pointers; n_bad (one int32, device) counts the candidates whose score is not finite: such a candidate is never picked while a
 * finite one remains. ---- */

/* flow[part](w, reverse=True) (part_encoders.py:655-659): w (R,zdim) standard normal -> code (R,zdim), the flow of that part alone.
 * scale_prior != 0: w is scaled by sqrt(prior_var) first, which gives column `part` of dfx_flow_reverse; 0: w as it is (the
 * reference's :655 does not scale; the same at the shipped prior_var = 1). */
int dfx_flow_reverse_part(dfx_latents *h, int part, const float *w, int scale_prior, float *code, int R, dfx_stream_t stream);

/* Statistics of the unit draws of subsample_params :555 without storing them: for the global candidate rows row0 .. row0+rows-1,
 * n_draws (a multiple of 4; the reference draws 512) standard normals per (axis, part) from Philox keyed by (seed, global row,
 * axis, part, draw), reduced in draw order in fp64 to stats (rows,4,3,n_class) = mean, unbiased std, min, max.  A call split over
 * row0 gives the same numbers. */
int dfx_part_draw_stats(uint64_t seed, long long row0, long long rows, int n_class, int n_draws, float *stats, dfx_stream_t stream);

/* Greedy diverse selection (subsample_params): mean, logvar (G K,3,n_class), valid (G,n_class) {0,1} floats.
 *   scores (G K,6,n_class), an output: the reference's param_score in closed form, fp64 rounded once.  With sigma = exp(logvar / 2)
 *     and the draw statistics (ubar, ustd, umin, umax): hi_c = max over valid j of mu + sigma umax, lo_c = min of mu + sigma umin,
 *     shift_c = (hi_c + lo_c) / 2, scale = max_c (hi_c - lo_c) / 2, scores[:3] = (mu + sigma ubar - shift) / scale,
 *     scores[3:] = 2 log(sigma ustd / scale).
 *   stats (G K,4,3,n_class) as dfx_part_draw_stats writes them (or the statistics of draws of the caller's own).
 *   idx (G,P) int32, 1 <= P <= K <= 4096: the group's lowest finite candidate (candidate 0 in the reference), then repeatedly the
 *     unselected candidate whose smallest distance to the selected ones is largest, distance = sum over c < 6 and valid j of
 *     (s_i - s_k)^2 / sum(valid), fp64 in (c, j) order; of equal ones the lowest index (torch.argmax).  A group without any valid
 *     part has nothing to compare: every distance is 0 and the picks are 0 .. P-1. */
int dfx_select_diverse(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int n_class, int P,
                       int32_t *idx, float *scores, int32_t *n_bad, dfx_stream_t stream);

/* Fit selection (part_encoders.py:678-682): idx (G) int32 = arg-min over k of sum_j weight[g,j] sum_c [(mean - target_mean)^2 +
 * (logvar - target_logvar)^2], fp64 in that order, the lowest index of equal ones.  mean, logvar (G K,3,n_class); target_mean,
 * target_logvar (G,3,n_class); weight (G,n_class) = the validity mask with the resampled part zeroed (a part of weight 0 is not
 * read); fit (G,K) or NULL: the sums, rounded once. */
int dfx_select_fit(const float *mean, const float *logvar, const float *target_mean, const float *target_logvar, const float *weight, int G,
                   int K, int n_class, int32_t *idx, float *fit, int32_t *n_bad, dfx_stream_t stream);

/* Greedy diverse selection over ALL rows of a call (the intent of subsample_params_global, part_encoders.py:591-621):
 * P picks out of the R = G K candidate rows, whatever group they belong to.  Layouts are dfx_select_diverse's: candidate row
 * r = g K + k, valid (G,n_class) with the mask of row r = valid[r / K], stats (R,4,3,n_class); scores (R,6,n_class) is an output and
 * may be NULL (it then lives in the workspace); idx (P) int32 holds GLOBAL row numbers.  1 <= P <= R, K <= 4096, R <= 262144.
 *   scores: dfx_select_diverse's, each row with its own mask.
 *   distance: rows i and s are compared on the parts valid in both: n = sum_j m_i[j] m_s[j],
 *     d(i,s) = sum over c < 6 and j valid in both of (s_i - s_s)^2 / n, fp64 in (c, j) order (part_encoders.py:611-612).  A pair
 *     without a common part (n = 0) puts no constraint on the candidate: it is skipped in the minimum (the reference divides 0 by 0
 *     and its arg-max goes to NaN), so a candidate that shares no part with any pick keeps mind = +inf and is picked next.
 *   selection: a row is finite when it has a valid part and every score on its own valid parts is finite; n_bad counts the others.
 *     Pick 0 is the lowest finite row, every later pick the free finite row whose smallest distance to the picks (mind) is largest,
 *     of equal ones the lowest index; non-finite rows by ascending index, only when no finite row is free.  A row is never picked
 *     twice (the reference can repeat a row once every distance is 0).
 *   rule DFX_DIVERSE_FARTHEST: mind follows every pick (farthest-point selection).  DFX_DIVERSE_FIRST_PICK: mind follows pick 0
 *     only: what the reference executes, because its out_score is never appended to (:603-619), when all rows share one mask.
 *   workspace: dfx_select_diverse_global_workspace_bytes(R) device bytes (sized for n_class = 8 and scores = NULL), 16-byte aligned.
 * No host round trip between picks and no workgroup that waits for another: up to 512 rows one workgroup runs the whole call;
 * above, one stream-ordered launch per pick spreads the rows over many workgroups and the next launch reduces their bests. */
#define DFX_DIVERSE_FARTHEST 0
#define DFX_DIVERSE_FIRST_PICK 1
size_t dfx_select_diverse_global_workspace_bytes(long long rows);
int dfx_select_diverse_global(const float *mean, const float *logvar, const float *valid, const float *stats, int G, int K, int n_class, int P,
                              int rule, int32_t *idx, float *scores, int32_t *n_bad, void *workspace, size_t workspace_bytes,
                              dfx_stream_t stream);

#define DFX_SEARCH_FIT 0     /* dfx_select_fit; P = 1 */
#define DFX_SEARCH_FIRST 1   /* candidates 0 .. P-1 (the intent of part_encoders.py:687); the aligner runs on those only */
#define DFX_SEARCH_DIVERSE 2 /* dfx_select_diverse */
#define DFX_SEARCH_DEFAULT_ROWS 16384

/* The candidate search of sample_with_fixed_latents (:664-695) for G groups (one per shape and new style) of K aligner noises each,
 * without materialising the G K candidate codes: the aligner runs over chunks of whole groups of at most row_budget candidate rows
 * (0 = DFX_SEARCH_DEFAULT_ROWS; at least K), each chunk is reduced by the selection, and only the P winners per group are kept.
 *   the codes of group g: part j from code_src[code_a[g,j]][:, j] (code_src (S,zdim,n_class) device, code_a HOST int32 (G,n_class),
 *     as dfx_compose_latents), except part new_part, which is new_code[g] (new_code (G,zdim) device; NULL with new_part -1)
 *   valid (G,n_class): the key mask of every candidate of the group; noise (G K,noise_dim): the aligner noises, an input
 *   mode DFX_SEARCH_*; target_mean / target_logvar / weight: dfx_select_fit's (FIT only, else NULL);
 *   stats (G K,4,3,n_class): dfx_select_diverse's, or NULL: dfx_part_draw_stats(seed, row0 + row, n_draws) per chunk (DIVERSE only)
 *   outputs: idx (G,P) int32; noise_sel (G P,noise_dim), mean_sel / logvar_sel (G P,3,n_class): the picked candidates' rows;
 *     scores or NULL: (G K,6,n_class) for DIVERSE, (G,K) for FIT.
 * The result does not depend on row_budget when the fp32 products keep one grouping of their K sums (dfx_debug_lin_split_k(1));
 * with the automatic grouping the parameters can differ in the last bits between budgets.  Every argument, code_a included, is
 * checked before the first HIP call. */
int dfx_part_search(dfx_latents *h, const float *code_src, int S, const int32_t *code_a, const float *new_code, int new_part,
                    const float *valid, const float *noise, int G, int K, int mode, int P, const float *target_mean,
                    const float *target_logvar, const float *weight, const float *stats, uint64_t seed, long long row0, int n_draws,
                    int row_budget, int32_t *idx, float *noise_sel, float *mean_sel, float *logvar_sel, float *scores, int32_t *n_bad,
                    dfx_stream_t stream);

/* dfx_part_search with the global selection: the same chunked aligner pass over G groups of K noises (no new part; the G K candidate
 * codes are never held), but mean, logvar and scores of ALL R = G K rows stay in the handle's workspace (R x 12 n_class floats),
 * dfx_select_diverse_global runs once after the last chunk, and the P winners' rows are gathered: idx (P) int32 global rows,
 * noise_sel (P,noise_dim), mean_sel / logvar_sel (P,3,n_class); scores (R,6,n_class) or NULL.  stats / seed / row0 / n_draws /
 * row_budget as dfx_part_search (DIVERSE); rule DFX_DIVERSE_*.  The result does not depend on row_budget under
 * dfx_debug_lin_split_k(1).  Every argument, code_a included, is checked before the first HIP call. */
int dfx_part_search_global(dfx_latents *h, const float *code_src, int S, const int32_t *code_a, const float *valid, const float *noise,
                           int G, int K, int P, int rule, const float *stats, uint64_t seed, long long row0, int n_draws, int row_budget,
                           int32_t *idx, float *noise_sel, float *mean_sel, float *logvar_sel, float *scores, int32_t *n_bad,
                           dfx_stream_t stream);

/* Training forward / backward of the part aligner (stage 2: configs/train_*_stage2.py and gen_*.py with train_aligner; replaces torch autograd through
 * PartAlignerTransformer, part_encoders.py:88-143, for the shipped options: cimle with cond_noise_type 0, class_cond + add_class_cond, single_attn,
 * mask_out_unreferenced_code, dropout 0).  Exact fp32, no atomics (aligner_train.hip).  `w` holds the parameter pointers (flow fields unused), `grads` the
 * gradient buffers in the same struct (overwritten; pre_norm_* untouched: unused by this configuration).
 *   part_code (B,zdim,n_class), valid (B,n_class) 0/1 = the key mask, noise (B,noise_dim) -> mean / logvar (B,3,n_class)
 *   backward: d_mean / d_logvar (B,3,n_class) (either may be NULL = zero) -> grads, d_part_code (B,zdim,n_class) or NULL
 *   workspace: dfx_aligner_train_workspace_bytes(...) device bytes, shared by the forward and the backward of a step. */
size_t dfx_aligner_train_workspace_bytes(int B, int n_class, int zdim, int noise_dim, int n_heads, int d_head, int depth);
int dfx_aligner_train_forward(const dfx_latent_weights *w, void *workspace, size_t workspace_bytes, const float *part_code, const float *valid,
                              const float *noise, float *mean, float *logvar, int B, dfx_stream_t stream);
int dfx_aligner_train_backward(const dfx_latent_weights *w, void *workspace, size_t workspace_bytes, const float *valid, const float *d_mean,
                               const float *d_logvar, const dfx_latent_weights *grads, float *d_part_code, int B, dfx_stream_t stream);

/* The data-gradient half of dfx_aligner_train_backward, for callers that differentiate in the INPUTS only (frozen weights; the noise optimization
 * below): runs after dfx_aligner_train_forward on the same workspace, the same dH chain (same kernels, same order: d_part_code has the bits
 * dfx_aligner_train_backward writes), no weight-gradient product, column sum or LayerNorm-parameter launch and no `grads` struct.
 *   d_noise (B,noise_dim) or NULL: d_noise[r,c] = noise_scale * sum_j dX0[(r,j), zdim + c], j ascending (the transpose of the token build; no atomics)
 *   d_part_code (B,zdim,n_class) or NULL; at least one of the two is given.  Arguments are checked before the first HIP call. */
int dfx_aligner_input_backward(const dfx_latent_weights *w, void *workspace, size_t workspace_bytes, const float *valid, const float *d_mean,
                               const float *d_logvar, float *d_noise, float *d_part_code, int B, dfx_stream_t stream);

/* Part re-configuration editing: gradient descent on the aligner's cIMLE noise z (tools/shape_edit.py:80-129 around AnchorDiffAE.edit_latent,
 * anchor_gen.py:872-893, + parse_losses; tools/optimize_noise.py / optimize_latent :895-913 with both selectors zero and fix = valid), R independent
 * problems per call (noise_opt.hip).  Per row r, J = n_class:
 *   fit  = sum_{c<3,j} fix[r,j] ((mean - fit_mean)^2 + (logvar - fit_logvar)^2)[r,c,j] / sum_j fix[r,j]      fix = valid * fix_ids, not all zero
 *   edit = sum_j edit_mean_sel[r,j] (1/3) sum_c (mean - edit_mean)^2[r,c,j] + sum_j edit_var_sel[r,j] (1/3) sum_c (logvar - edit_logvar)^2[r,c,j]
 *   reg  = sum_c z[r,c]^2;     L = fit_weight fit + edit + reg_weight reg
 * Every row has its own torch.optim.Adam state (amsgrad off), ReduceLROnPlateau (mode min, threshold mode rel, cooldown 0) on L and stop flag
 * (|L - prev| <= stop_atol + stop_rtol |prev|, prev starting at 0, as torch.allclose); a stopped row is never written again.  UNLIKE the reference,
 * whose batch mean couples the rows of a batch, no row sees another one: a row gives the same bits alone and inside any batch.
 * All pointers are device pointers; (R,3,J) targets, (R,J) masks; a selector and its target are NULL together (= that term is absent). */
typedef struct {
  const float *fit_mean, *fit_logvar, *fix;
  const float *edit_mean, *edit_mean_sel;
  const float *edit_logvar, *edit_var_sel;
  double fit_weight, reg_weight;
  double lr0, beta1, beta2, adam_eps;                 /* reference: 1, 0.9, 0.999, 1e-8 */
  double factor, threshold, min_lr, lr_eps;           /* reference: 0.5, 1e-4, 5e-2, 1e-8 */
  double stop_atol, stop_rtol;                        /* reference: 1e-8, 1e-5 */
  int32_t patience;                                   /* reference: 10 */
} dfx_noise_opt_problem;

/*   workspace: dfx_noise_opt_workspace_bytes(w, R) device bytes (0 for a configuration the training kernels do not take)
 *   part_code (R,zdim,J), valid (R,J); z (R,noise_dim): in = the start, out = the result; mean / logvar (R,3,J): the aligner's output at the
 *   RETURNED z; iters_done (R): iterations a row took part in (a row that stops at iteration s: s + 1)
 *   trace (max_iter,R,5 + 2 noise_dim) or NULL: L, fit, edit, reg, the learning rate of this iteration's Adam step, z before the step, the total
 *   gradient (d_noise + 2 reg_weight z); zeros for the iterations after a row stopped.
 * Enqueues max_iter x [aligner forward, loss, input backward, step] and a final forward on `stream`, with no host synchronization except one
 * read of the stopped-row count every 32 iterations (to stop enqueuing once every row is frozen; no result depends on it). */
size_t dfx_noise_opt_workspace_bytes(const dfx_latent_weights *w, int R);
int dfx_noise_opt_run(const dfx_latent_weights *w, void *workspace, size_t workspace_bytes, const dfx_noise_opt_problem *p, const float *part_code,
                      const float *valid, float *z, float *mean, float *logvar, int32_t *iters_done, float *trace, int R, int max_iter,
                      dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PointNet++ set-abstraction / feature-propagation layers, eval mode — the part of
 * pointnet2_ops the reference leaves to PyTorch: QueryAndGroup / GroupAll
 * (pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py:296-333, :349-381) + build_shared_mlp's Conv2d 1x1 +
 * BatchNorm2d + ReLU stack (pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py:9-19) + max_pool2d over nsample
 * (:62-70), and PointnetFPModule.forward (:170-209).  BatchNorm uses its running statistics (folded into the
 * convolution at create time); training mode: dfx_shared_mlp_train_* below.
 * ------------------------------------------------------------------------------------------ */
typedef struct dfx_shared_mlp dfx_shared_mlp; /* opaque; owns folded/packed weights + a grow-only workspace */

/* n_layers <= 4; channels[n_layers+1]; per layer device pointers: conv_w (Cout,Cin) [Conv2d weight (Cout,Cin,1,1)],
 * conv_b (Cout) or NULL, and either all of bn_w/bn_b/bn_mean/bn_var (Cout) or bn_w[l] == NULL (no BatchNorm). */
int dfx_shared_mlp_create(dfx_shared_mlp **out, int n_layers, const int32_t *channels, const float *const *conv_w,
                          const float *const *conv_b, const float *const *bn_w, const float *const *bn_b,
                          const float *const *bn_mean, const float *const *bn_var, float eps, uint32_t relu_mask,
                          dfx_stream_t stream); /* relu_mask bit l: ReLU after layer l (build_shared_mlp: all ones) */
void dfx_shared_mlp_destroy(dfx_shared_mlp *h);
int dfx_shared_mlp_is_fused(const dfx_shared_mlp *h); /* 1: the gather+MLP+max-pool kernel serves this MLP in one launch */

/* _PointnetSAModuleBase.forward after the centres are known: grouper -> mlp -> max over nsample.
 *   xyz (B,N,3); new_xyz (B,M,3) centres (NULL: no centring, GroupAll); features (B,C,N) or NULL (C = 0);
 *   idx (B,M,ns) int32 from ball_query, or NULL = GroupAll (M = 1, ns = N, every point);
 *   out (B, C_out, M).  force_general != 0 selects the layer-by-layer path (A/B and parity of the two paths). */
int dfx_sa_forward_f32(dfx_shared_mlp *h, const float *xyz, const float *new_xyz, const float *features,
                       const int32_t *idx, int use_xyz, float *out, int B, int N, int M, int ns, int C, int force_general,
                       dfx_stream_t stream);

/* PointnetFPModule.forward: unknown (B,n,3), known (B,m,3) or NULL, unknow_feats (B,C1,n) or NULL (C1 = 0),
 * known_feats (B,C2,m) [(B,C2,1) when known is NULL] -> out (B, C_out, n). */
int dfx_fp_forward_f32(dfx_shared_mlp *h, const float *unknown, const float *known, const float *unknow_feats,
                       const float *known_feats, float *out, int B, int n, int m, int C1, int C2, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same shared MLP in TRAINING mode (round 6): build_shared_mlp's Conv2d 1x1 [+ BatchNorm2d with BATCH statistics and the running-
 * statistics update of nn.BatchNorm2d: momentum, unbiased variance] + ReLU stack over a grouped tensor, + max over nsample
 * (pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py:9-19, :62-70; PointnetFPModule's mlp :170-209 with pool = 0), forward with saved
 * activations and backward — what autograd through nn.Conv2d / nn.BatchNorm2d / F.max_pool2d computes in the reference.  Exact fp32.
 *   x (B, ch[0], M, ns) = the grouper's output (QueryAndGroup / GroupAll through dfx_group_points, or the interpolated + skip features with
 *   ns = 1; a Linear + BatchNorm1d head over a batch of rows, e.g. PointNet2SSG.fc_layer (models/encoders/pointnet2.py:47-56): B = 1, M = rows, ns = 1); out (B, ch[layers], M) when pool != 0, else (B, ch[layers], M, ns).  ch[l] % 8 == 0 and 8 <= ch[l] <= 1024 for l >= 1 (each is the K of
 *   two fp32 MFMA products, consumed eight at a time; ch[0] is free: it is padded to a multiple of 8 internally); layers <= DFX_MLP_MAX_LAYERS.
 *   conv_b[l] == NULL when the layer has BatchNorm (bn_w[l] != NULL); bn_mean / bn_var: running statistics, updated IN PLACE by the forward
 *   when momentum >= 0.  grads: the same struct whose conv_w / conv_b / bn_w / bn_b name WRITABLE buffers of the parameters' shapes.
 *   batch_stats = 1: BatchNorm of train() mode; 0: eval() mode under autograd (the running statistics normalise, nothing is updated); the same value
 *   for the forward and its backward.  d_x (B, ch[0], M, ns) or NULL.  workspace: dfx_shared_mlp_train_workspace_bytes, 256-byte aligned; the backward reads what the forward of
 *   the SAME (B, M, ns) call left in it.
 * ------------------------------------------------------------------------------------------ */
#define DFX_MLP_MAX_LAYERS 4
typedef struct dfx_shared_mlp_train {
  int layers;
  int ch[DFX_MLP_MAX_LAYERS + 1];
  const float *conv_w[DFX_MLP_MAX_LAYERS], *conv_b[DFX_MLP_MAX_LAYERS];
  const float *bn_w[DFX_MLP_MAX_LAYERS], *bn_b[DFX_MLP_MAX_LAYERS];
  float *bn_mean[DFX_MLP_MAX_LAYERS], *bn_var[DFX_MLP_MAX_LAYERS];
  float bn_eps;
  uint32_t relu_mask; /* bit l: ReLU behind layer l (build_shared_mlp: all ones; a Linear head's last layer: 0) */
} dfx_shared_mlp_train;
size_t dfx_shared_mlp_train_workspace_bytes(const dfx_shared_mlp_train *w, int B, int M, int ns);
int dfx_shared_mlp_train_forward(const dfx_shared_mlp_train *w, void *workspace, size_t workspace_bytes, const float *x, float *out, int B, int M,
                                 int ns, int pool, int batch_stats, float momentum, dfx_stream_t stream);
int dfx_shared_mlp_train_backward(const dfx_shared_mlp_train *w, void *workspace, size_t workspace_bytes, const float *d_out,
                                  const dfx_shared_mlp_train *grads, float *d_x, int B, int M, int ns, int pool, int batch_stats, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PointNetV2 masked max-pool part encoder, eval mode — python/difffacto/models/encoders/pointnet.py:124-213
 * with per_part_mlp=True: conv1..4 + BN (ReLU after the first three) over the points, x * attn_weight (* num_anchors)
 * max-pooled over N per part (:194-198), per-part grouped-Conv1d heads 512 -> 256 -> 128 -> zdim for m and v (:200-203).
 * ------------------------------------------------------------------------------------------ */
typedef struct dfx_pointnet_v2_weights { /* fp32 device pointers, reference state_dict tensors */
  int32_t num_anchors, zdim, reweight_by_anchor;
  float bn_eps;
  const float *conv_w[4], *conv_b[4];                           /* conv{1..4}.weight (Cout,Cin,1), .bias */
  const float *bn_w[4], *bn_b[4], *bn_mean[4], *bn_var[4];      /* bn{1..4} */
  const float *head_w[2][3], *head_b[2][3];                     /* [0] = mlp_m, [1] = mlp_v: .0 / .3 / .6 weight (A*Cout,Cin,1), bias */
  const float *head_bn_w[2][2], *head_bn_b[2][2], *head_bn_mean[2][2], *head_bn_var[2][2]; /* .1 / .4 */
} dfx_pointnet_v2_weights;
typedef struct dfx_pointnet_v2 dfx_pointnet_v2;
int dfx_pointnet_v2_create(dfx_pointnet_v2 **out, const dfx_pointnet_v2_weights *w, dfx_stream_t stream);
void dfx_pointnet_v2_destroy(dfx_pointnet_v2 *h);
/* x (B,N,3), attn_weight (B,N,num_anchors) -> m, v (B,num_anchors,zdim) */
int dfx_pointnet_v2_forward_f32(dfx_pointnet_v2 *h, const float *x, const float *attn, float *m, float *v, int B, int N,
                                dfx_stream_t stream);

/* The same encoder in TRAIN mode (nn.BatchNorm1d with batch statistics over the B N points / over the B shapes in the heads) and
 * its backward (encoder side): m, v as above; the backward takes d m, d v (B,num_anchors,zdim) and writes the
 * gradients of conv / BatchNorm / head weights and biases into `grads` (same struct, writable pointers; its running-statistics
 * pointers are ignored).  momentum >= 0 updates the running statistics in place like nn.BatchNorm1d (unbiased variance),
 * momentum < 0 leaves them alone.  workspace: dfx_pointnet_v2_train_workspace_bytes(B, N, 4, zdim), 256-byte aligned, shared
 * by the forward and the backward of one step.  num_anchors = 4, B >= 2, zdim % 8 == 0 (the K of the last head layer's input-gradient
 * products; the eval handle has the same rule).  precision as for the denoiser. */
size_t dfx_pointnet_v2_train_workspace_bytes(int B, int N, int num_anchors, int zdim);
int dfx_pointnet_v2_train_forward(const dfx_pointnet_v2_weights *w, void *workspace, size_t workspace_bytes, const float *x,
                                  const float *attn, float *m, float *v, float momentum, int B, int N, int precision,
                                  dfx_stream_t stream);
int dfx_pointnet_v2_train_backward(const dfx_pointnet_v2_weights *w, void *workspace, size_t workspace_bytes, const float *attn,
                                   const float *dm, const float *dv, const dfx_pointnet_v2_weights *grads, int B, int N,
                                   int precision, dfx_stream_t stream);

/* Prior loss of the part encoder with use_flow (PartEncoder.get_prior_loss, part_encoders.py:1143-1182) and its backward
 * (encoder side): per part, the latents go FORWARD through that part's coupling layers (flow.py:21-41,
 * logpx - log det), log N(w; 0, prior_var) with the reference's normalisation (misc.py:301-317 called with dim = zdim and summed
 * over the zdim elements), minus the posterior's Gaussian entropy (misc.py:292-295), averaged over the valid parts of a shape
 * and over the batch, times kl_weight.  n_class = 4, zdim = 256.
 *   flow / flow_grads: HOST arrays of 4 * flow_depth * 6 device pointers, [part][layer][w0,b0,w1,b1,w2,b2] = net_s_t.{0,2,4}
 *   (as in dfx_latent_weights); flow_grads buffers are overwritten.  part_code (B,256,4), logvar (B,4,256), valid (B,4) 0/1.
 *   loss: one float on the device; log_p_part / entropy (B,4) or NULL.  d_part_code (B,256,4) / d_logvar (B,4,256) or NULL.
 *   workspace: dfx_prior_loss_workspace_bytes(B, flow_depth, flow_hidden), shared by the forward and the backward of a step. */
#define DFX_MAX_FLOW_DEPTH 16
size_t dfx_prior_loss_workspace_bytes(int B, int flow_depth, int flow_hidden);
int dfx_prior_loss_forward(const float *const *flow, int flow_depth, int flow_hidden, void *workspace, size_t workspace_bytes,
                           const float *part_code, const float *logvar, const float *valid, float prior_var, float kl_weight,
                           float *loss, float *log_p_part, float *entropy, int B, dfx_stream_t stream);
int dfx_prior_loss_backward(const float *const *flow, int flow_depth, int flow_hidden, void *workspace, size_t workspace_bytes,
                            const float *valid, float prior_var, float grad_scale, float *const *flow_grads, float *d_part_code,
                            float *d_logvar, int B, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Approximate EMD by auction — replaces the `emd` extension
 * (python/difffacto/metrics/emd/emd_cuda.cu: forward :236-284, backward :286-316; bound in emd_module.py:17-51).
 * xyz1, xyz2 (B,n,3) in [0,1]^3 -> dist (B,n) squared distance of point j to its matched target, assignment (B,n) int32.
 * One persistent workgroup per cloud pair; n <= 8192 (any n, not only multiples of 1024; B unbounded).
 * workspace: dfx_emd_workspace_bytes(B, n) device bytes.  emd_backward: grad_xyz1 (B,n,3) (grad_xyz2 is zero in the reference).
 * ------------------------------------------------------------------------------------------ */
size_t dfx_emd_workspace_bytes(int B, int n);
int dfx_emd_forward_f32(const float *xyz1, const float *xyz2, float *dist, int32_t *assignment, void *workspace, int B, int n,
                        float eps, int iters, dfx_stream_t stream);
int dfx_emd_backward_f32(const float *xyz1, const float *xyz2, const float *grad_dist, const int32_t *assignment,
                         float *grad_xyz1, int B, int n, dfx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode denoiser: forward with saved activations, backward, loss gradient, optimizer.
 * Replaces autograd through TransformerNet.forward / _forward_attn (python/difffacto/models/diffusions/nets/attention.py:385-440;
 * BasicTransformerBlock :296-306, CrossAttention :179-204, FeedForward/GEGLU :50-57,77-94; nn.Dropout optional, see below), the
 * mse_loss of AnchoredDiffusion.training_losses (anchored_diffusion.py:840-847), and Runner.train's
 * clip_grad_norm_ + Adam.step (runner.py:312-316, optimizers.py:4-16).
 *   precision DFX_PREC_F32: exact fp32 throughout (the parity gate).  DFX_PREC_BF16: the large matrix products (every
 *   linear layer over the B*N points: forward, dX, dW) round their operands to bf16 on the way into LDS and accumulate
 *   in fp32 (v_mfma_f32_32x32x16_bf16); activations, gradients, LayerNorm / softmax / GELU and the optimiser stay fp32.
 *   The same value must be passed to the forward and the backward of one step.
 *   dropout_p in [0, 1): nn.Dropout of train() mode behind every to_out (attention.py:177) and GEGLU (:84, time_embed
 *   included); factor(seed, site, element i) = 0 when a 16-bit draw is below round(p 2^16), else 1 / (1 - p); the draw is 16 bits of
 *   Philox4x32-7 keyed by the 64-bit dropout_seed, counter = (i >> 3 = group of EIGHT consecutive elements of the site's row-major
 *   tensor, site, 0xD20F0), element i & 7 = half (i & 1) of word (i & 7) >> 1 (csrc/dfx_dropout.h is the one definition); sites: 2 b =
 *   behind to_out of block b over (B N, 128), 2 b + 1 = behind the GEGLU of block b over (B N, 512), 1000 = time_embed over (B, 1024).
 *   The backward regenerates / re-reads them (pass the same p and seed); torch's own CUDA dropout stream is launch-geometry dependent
 *   and not reproducible, so this is libdfx's contract, checked against torch autograd by replaying the factors
 *   (dfx_debug_dropout_factors, include/dfx_debug.h).
 *   x (B,3,N); t (B,) int32; ctx_code (B,256,4) and ctx_mv (B,6,4) = the two tensors of the reference's ctx list;
 *   anchors, variances (B,N,3) per point (the caller's gather, as at anchored_diffusion.py:261); valid (B,4) 0/1 or
 *   NULL; assignment (B,N) int32; eps (B,3,N).
 *   workspace: dfx_denoiser_train_workspace_bytes(B, N, depth) device bytes, 256-byte aligned; the backward reads what
 *   the forward of the SAME (B, N) call left in it.
 *   Streams: the bf16 path forks small-grid work (context branch, parameter-gradient reductions) onto an internal side stream per
 *   (device, caller stream) pair and joins it before returning — stream-ordered, capturable.  A process gets at most
 *   DFX_MAX_SIDE_STREAMS such pairs (never evicted); callers beyond that run everything on their own stream (same results).
 *   grads: a dfx_denoiser_weights whose pointers name WRITABLE device buffers of the parameters' shapes; every one of
 *   them is overwritten (not accumulated).  d_ctx_code / d_ctx_mv: (B,256,4) / (B,6,4) or NULL.
 *   d_x (B,3,N) / d_variances (B,N,3) or NULL (ABI 4): the gradient at the input x and at the per-point variance feature columns — stage 2 of the
 *   reference differentiates `variance` (it reaches training_losses undetached, anchor_gen.py:1002-1020), through q_sample and through these columns.
 * ------------------------------------------------------------------------------------------ */
size_t dfx_denoiser_train_workspace_bytes(int B, int N, int depth);
int dfx_denoiser_train_forward(const dfx_denoiser_weights *w, void *workspace, size_t workspace_bytes, const float *x,
                               const int32_t *t, const float *ctx_code, const float *ctx_mv, const float *anchors,
                               const float *variances, const float *valid, const int32_t *assignment, float *eps, int B,
                               int N, int precision, float dropout_p, uint64_t dropout_seed, dfx_stream_t stream);
int dfx_denoiser_train_backward(const dfx_denoiser_weights *w, void *workspace, size_t workspace_bytes,
                                const float *d_eps, const dfx_denoiser_weights *grads, float *d_ctx_code, float *d_ctx_mv,
                                float *d_x, float *d_variances, int B, int N, int precision, float dropout_p, uint64_t dropout_seed,
                                dfx_stream_t stream);
/* d loss / d pred of dfx_masked_mse_f32, times grad_scale; workspace2 = the two doubles its forward left behind */
int dfx_masked_mse_backward_f32(const float *target, const float *pred, const float *flags, const double *workspace2,
                                float grad_scale, float *d_pred, int B, int N, dfx_stream_t stream);
/* *sumsq += sum(g^2) (zero it before the first tensor); workspace1024 = 1024 doubles on the device */
int dfx_grad_sumsq_accumulate(const float *g, long long n, double *workspace1024, double *sumsq, dfx_stream_t stream);
/* torch.optim.Adam step on one tensor, gradient scaled by min(1, max_norm / (sqrt(*sumsq) + 1e-6)) if max_norm > 0 */
int dfx_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long n, const double *sumsq,
                      float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      dfx_stream_t stream);

/* Name + average duration bookkeeping for bench.py: duration in ms of the last dfx_sample_chain /
 * dfx_p_sample / dfx_denoise_eps launch measured with HIP events on `stream` when profiling is enabled. */
void dfx_set_event_timing(int enable);
float dfx_last_kernel_ms(void);
/* Which kernel the last dfx_sample_chain / dfx_p_sample / dfx_denoise_eps (and their _ddim / _t forms) launched on this host
 * thread's process: "k_denoise_pipe<8>", "k_denoise_pipe<4>", "k_denoise_pipe<2>", "k_denoise_coop", "k_denoise_coop2",
 * "k_denoise_pipe_f32<8|4|2>", "k_denoise<bf16>", "k_denoise<f32>" ("" before the first launch).  The choice is made from the
 * batch shape; every variant of one precision produces the same bits.  Static storage, never NULL. */
const char *dfx_last_kernel_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* DFX_H */
