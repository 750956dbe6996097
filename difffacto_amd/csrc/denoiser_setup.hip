// libdfx: one-off preparation of the frozen denoiser (not on the hot path).
//
//  dfx_denoiser_create   schedule tables (anchored_diffusion.py:62-112), time-embedding MLP for every
//                        t (nets/utils.py:7-24 + attention.py:357,393), per-t attention constants,
//                        weight repacking into MFMA A-fragment order (denoiser_internal.h)
//  dfx_shape_ctx_prepare per-batch static attention operands (attention.py:386-397 context, :179-204)
//
// Algebra used (exact in real arithmetic):
//   ctx_j = [s_j | t_emb(t)]  =>  k_j = Wk_s s_j + Wk_t t_emb,  v_j = Wv_s s_j + Wv_t t_emb.
//   * The Wk_t t_emb term is identical for the 4 keys of a head, so it cancels in the softmax.
//   * softmax weights sum to 1, so the Wv_t t_emb term passes through as a per-(t,block) constant
//     c_t = Wo (Wv_t t_emb) + b_o.
//   * q.k_j = LN(h) . (Wq_h^T k_j): the to_q projection folds into A_s[(head,j), :] (32 x 128 per shape),
//     the to_out projection into M_s[:, (head,j)] = Wo[:, head] v_j (128 x 32 per shape).
//   * LayerNorm affine of norm2 / norm3 / post_norm fold into A_s / W1 / W_out.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "denoiser_ff16.h"
#include "denoiser_internal.h"

using namespace dfx;

namespace {

static_assert(ff16::CH == INNER && ff16::HID == FF_HID && ff16::CHUNKS == FF_CHUNKS && ff16::REC_TILES == CHUNK_TILES && ff16::SKEW == FF_SKEW,
              "denoiser_ff16.h against denoiser_internal.h");

int g_w1_fold_mode = -1;                       // dfx_debug_w1_fold: -1 = decide per engine from its weights, 0 = never, 1 = always
constexpr float W1_FOLD_KEEP_127 = 4.0f;       // channel 127 stays the folded one while its column's ratio is at most this (bit-compatible with round 5's packs)
constexpr float W1_FOLD_MAX_RATIO = 8.0f;      // (random-init and unit-gamma weights: ~1-3; the fold's extra rounding scales with the ratio)

// ---------------------------------------------------------------------------------------------
// small fp32 helper kernels (setup only: one thread per output, no tuning)

// Y[m][n] = sum_k X[m*ldx + k] * W[n*ldw + koff + k] + (b ? b[n] : 0)
__global__ void k_linear(const float *__restrict__ X, int ldx, const float *__restrict__ W, int ldw, int koff,
                         const float *__restrict__ b, float *__restrict__ Y, int M, int N, int K) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  const float *x = X + (size_t)m * ldx;
  const float *w = W + (size_t)n * ldw + koff;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(x[k], w[k], acc);
  Y[i] = acc + (b ? b[n] : 0.f);
}

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// GEGLU: out[m][j] = in[m][j] * gelu(in[m][H + j])   (attention.py:50-57)
__global__ void k_geglu(const float *__restrict__ in, float *__restrict__ out, int M, int H) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)M * H) return;
  const int m = (int)(i / H), j = (int)(i % H);
  out[i] = in[(size_t)m * 2 * H + j] * gelu_exact(in[(size_t)m * 2 * H + H + j]);
}

// rows of Y (M x 128, natural channel order) -> cvec order, optional bias add
__global__ void k_to_cvec(const float *__restrict__ Y, const float *__restrict__ bias, float *__restrict__ out,
                          int M, int out_stride) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)M * 128) return;
  const int m = (int)(i >> 7), ch = (int)(i & 127);
  out[(size_t)m * out_stride + cvec_index(ch)] = Y[i] + (bias ? bias[ch] : 0.f);
}

template <int PREC>
__device__ __forceinline__ void tile_decode(int idx, int &i, int &kk) {
  if (PREC == DFX_PREC_BF16) {
    const int unit = idx >> 9, lane = (idx >> 3) & 63, e = idx & 7;
    i = lane & 31;
    kk = (e & 3) + 16 * unit + 8 * (e >> 2) + 4 * (lane >> 5);
  } else {
    const int unit = idx >> 8, lane = (idx >> 2) & 63, e = idx & 3;
    i = lane & 31;
    kk = e + 8 * unit + 4 * (lane >> 5);
  }
}

// inverse of tile_decode: position of element (row i, column kk) inside its 32 x 32 tile
template <int PREC>
__device__ __forceinline__ int tile_index(int i, int kk) {
  const int lane = i + 32 * ((kk >> 2) & 1);
  if (PREC == DFX_PREC_BF16) return (kk >> 4) * 512 + lane * 8 + (kk & 3) + 4 * ((kk >> 3) & 1);
  return (kk >> 3) * 256 + lane * 4 + (kk & 3);
}

template <int PREC>
__device__ __forceinline__ void tile_store(void *dst, long long gi, float v) {
  if (PREC == DFX_PREC_BF16) reinterpret_cast<__bf16 *>(dst)[gi] = (__bf16)v;
  else reinterpret_cast<float *>(dst)[gi] = v;
}

// W1 (1024 x 128) with norm3.weight folded in -> tiles part*4+c of chunk record u.  bf16: element order (the A operand of
// v_mfma_f32_16x16x32_bf16, for every kernel of the engine) and value from denoiser_ff16.h
template <int PREC>
__global__ void k_pack_w1(const float *__restrict__ W1, const float *__restrict__ g3, void *__restrict__ dst, const float *__restrict__ b1,
                          const float *__restrict__ be3, int fold) {
  const long long gi = blockIdx.x * 256LL + threadIdx.x;
  if (gi >= ff16::W1_PACK_THREADS) return;
  if (PREC == DFX_PREC_BF16) {
    // fold (denoiser_kernel.hip: bias_slot_one): the normalised row sums to zero, so channel 127 is redundant (xhat_127 = - sum of the
    // others): its K slot carries the constant 1 and the weight there is b1' = b1 + W1 beta3, every other weight has W1'[.][127] subtracted.
    // Exact in real arithmetic; GEMM1 then needs no accumulator initialisers.
    const ff16::Src s = ff16::w1_source(gi, ff16::LAYOUT_16X16X32);
    const float sc = s.row < FF_HID ? FF_A_SCALE : FF_G_SCALE;   // (denoiser_internal.h)
    tile_store<PREC>(dst, s.di, ff16::w1_value(W1, g3, b1, be3, s.row, s.col, fold) * sc);
    return;
  }
  const int tile = (int)(gi >> 10);
  int i, kk;
  tile_decode<PREC>((int)(gi & 1023), i, kk);
  const int c = tile & 3, part = (tile >> 2) & 1, u = tile >> 3;
  const int row = part * FF_HID + 32 * u + i, col = 32 * c + kk;
  const long long di = ((long long)(u * CHUNK_TILES + part * 4 + c) << 10) + (gi & 1023);
  tile_store<PREC>(dst, di, W1[(size_t)row * INNER + col] * g3[col]);
}

// How much coarser the fold makes a row of W1' = W1 diag(gamma3) when channel k is the redundant one: every weight of row r becomes
// W1'[r][c] - W1'[r][k], so its bf16 rounding step follows |W1'[r][k]| instead of |W1'[r][c]|.  out[k] = max over the rows of
// |W1'[r][k]| / mean_{c != k} |W1'[r][c]| (about 1-3 for weights of one scale; a LayerNorm outlier gamma3[k] shows up as itself).
// One workgroup of 1024 threads = one row each.
__global__ void __launch_bounds__(1024) k_w1_fold_scores(const float *__restrict__ W1, const float *__restrict__ g3, float *__restrict__ out) {
  __shared__ unsigned best[INNER];   // non-negative floats order like their bit patterns
  const int row = threadIdx.x;
  if (row < INNER) best[row] = 0u;
  __syncthreads();
  float s = 0.f;
  for (int c = 0; c < INNER; ++c) s += fabsf(W1[(size_t)row * INNER + c] * g3[c]);
  for (int c = 0; c < INNER; ++c) {
    const float w = fabsf(W1[(size_t)row * INNER + c] * g3[c]);
    atomicMax(&best[c], __float_as_uint(w / fmaxf((s - w) / (INNER - 1), 1e-30f)));
  }
  __syncthreads();
  if (row < INNER) out[row] = __uint_as_float(best[row]);
}

// A copy of a (rows x cols) parameter with hidden channels ka and kb exchanged along its rows (by_col = 0) or its columns (by_col = 1)
__global__ void k_swap_channels(const float *__restrict__ src, float *__restrict__ dst, int rows, int cols, int by_col, int ka, int kb) {
  const long long gi = blockIdx.x * 256LL + threadIdx.x;
  if (gi >= (long long)rows * cols) return;
  int r = (int)(gi / cols), c = (int)(gi % cols);
  int &k = by_col ? c : r;
  k = k == ka ? kb : k == kb ? ka : k;
  dst[gi] = src[(size_t)r * cols + c];
}

// b1' = b1 + W1 beta3, stored [u][part][hf][16]; quads16 (bf16 engines): [u][part][R][m][4] = hidden unit 16m + 4R + r, the order of a lane row's
// two accumulator quads under v_mfma_f32_16x16x32 (denoiser_ff16.h)
__global__ void k_pack_b1(const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ be3,
                          float *__restrict__ dst, float a_scale, float g_scale, int quads16) {
  const int gi = blockIdx.x * 256 + threadIdx.x;
  if (gi >= FF_CHUNKS * 2 * 32) return;
  const int r = gi & 15, hf = (gi >> 4) & 1, part = (gi >> 5) & 1, u = gi >> 6;
  const int unit = quads16 ? 16 * ((gi >> 2) & 1) + 4 * ((gi >> 3) & 3) + (gi & 3) : rho(r, hf);
  const int row = part * FF_HID + 32 * u + unit;
  float acc = 0.f;
  for (int k = 0; k < INNER; ++k) acc = fmaf(W1[(size_t)row * INNER + k], be3[k], acc);
  dst[gi] = (b1[row] + acc) * (part == 0 ? a_scale : g_scale);
}

// W2 (128 x 512) -> tiles 8+ct of stage record u+FF_SKEW (see denoiser_internal.h; bf16: fp16 in the order of denoiser_ff16.h)
template <int PREC>
__global__ void k_pack_w2(const float *__restrict__ W2, void *__restrict__ dst) {
  const long long gi = blockIdx.x * 256LL + threadIdx.x;
  if (gi >= ff16::W2_PACK_THREADS) return;
  if (PREC == DFX_PREC_BF16) {
    const ff16::Src s = ff16::w2_source(gi, ff16::LAYOUT_16X16X32);
    reinterpret_cast<_Float16 *>(dst)[s.di] = (_Float16)(W2[(size_t)s.row * FF_HID + s.col] * (1.0f / (FF_A_SCALE * FF_G_SCALE)));
    return;
  }
  const int tile = (int)(gi >> 10);
  int i, kk;
  tile_decode<PREC>((int)(gi & 1023), i, kk);
  const int ct = tile & 3, u = tile >> 2;
  const long long di = ((long long)((u + FF_SKEW) * CHUNK_TILES + 8 + ct) << 10) + (gi & 1023);
  tile_store<PREC>(dst, di, W2[(size_t)(32 * ct + i) * FF_HID + 32 * u + kk]);
}

// proj_in x-columns, pre_norm affine, post_norm-folded proj_out, all in cvec order
__global__ void k_pack_misc(const float *__restrict__ win, const float *__restrict__ pre_g,
                            const float *__restrict__ pre_b, const float *__restrict__ post_g,
                            const float *__restrict__ wout, float4 *__restrict__ win_x, float2 *__restrict__ pre_gb,
                            float4 *__restrict__ wout_f) {
  const int ch = threadIdx.x;  // 128 threads
  const int p = cvec_index(ch);
  win_x[p] = make_float4(win[ch * IN_CH + 0], win[ch * IN_CH + 1], win[ch * IN_CH + 2], 0.f);
  pre_gb[p] = make_float2(pre_g[ch], pre_b[ch]);
  wout_f[p] = make_float4(wout[0 * INNER + ch] * post_g[ch], wout[1 * INNER + ch] * post_g[ch],
                          wout[2 * INNER + ch] * post_g[ch], 0.f);
}

// to_k / to_v (128, 522) -> the static columns transposed, [266][128] (k_shape_ctx reads them with thread = row)
__global__ void k_transpose_static(const float *__restrict__ W, float *__restrict__ WT) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= CTX_STATIC * INNER) return;
  const int k = idx / INNER, row = idx % INNER;
  WT[idx] = W[(size_t)row * CTX_DIM + k];
}

// Wq beta2 (the LayerNorm2 shift folded into the similarity bias): one thread per row, summed over k in order
__global__ void k_wq_beta(const float *__restrict__ Wq, const float *__restrict__ be2, float *__restrict__ out) {
  const int row = threadIdx.x;
  float acc = 0.f;
  for (int k = 0; k < INNER; ++k) acc = fmaf(Wq[(size_t)row * INNER + k], be2[k], acc);
  out[row] = acc;
}
__global__ void k_transpose_sq(const float *__restrict__ W, float *__restrict__ WT) {   // (128, 128)
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < INNER * INNER) WT[idx] = W[(size_t)(idx % INNER) * INNER + idx / INNER];
}

// ---------------------------------------------------------------------------------------------
// Per-(shape, block) static attention operands.  One 256-thread workgroup per (s, b).
template <int PREC>
__global__ void __launch_bounds__(256) k_shape_ctx(const float *__restrict__ part_code, const float *__restrict__ mean,
                                                   const float *__restrict__ var, const float *__restrict__ valid,
                                                   const float *const *__restrict__ wptrs /* [depth][7] */,
                                                   const float *__restrict__ win, const float *__restrict__ bin,
                                                   ShapeCtxView out, int depth) {
  // token-minor LDS tables: one ds_read_b128 hands a thread the value of all four tokens (the reads are broadcasts: every lane the same address)
  __shared__ __attribute__((aligned(16))) float s_ctx[CTX_STATIC + 2][NCLS];
  __shared__ __attribute__((aligned(16))) float s_k[INNER][NCLS], s_v[INNER][NCLS];
  __shared__ float s_wqb[INNER];
  __shared__ float s_out[8 * 1024];   // the record's eight tiles in fragment order
  const int s = blockIdx.x / depth, b = blockIdx.x % depth;
  const int tid = threadIdx.x;
  const float *Wq = wptrs[b * 7 + 0], *Wk = wptrs[b * 7 + 1], *Wv = wptrs[b * 7 + 2], *Wo = wptrs[b * 7 + 3];
  const float *g2 = wptrs[b * 7 + 4], *wqb = wptrs[b * 7 + 6];   // (Wk, Wv: static columns transposed; Wo transposed; wqb = Wq beta2, from create)
  // static context rows: [part_code(256) | mean(3) | var(3) | onehot(4)]   (attention.py:386-391)
  for (int i = tid; i < NCLS * CTX_STATIC; i += 256) {
    const int j = i / CTX_STATIC, k = i % CTX_STATIC;
    float v;
    if (k < ZDIM) v = part_code[((size_t)s * ZDIM + k) * NCLS + j];
    else if (k < ZDIM + 3) v = mean[((size_t)s * 3 + (k - ZDIM)) * NCLS + j];
    else if (k < ZDIM + 6) v = var[((size_t)s * 3 + (k - ZDIM - 3)) * NCLS + j];
    else v = (k - ZDIM - 6) == j ? 1.f : 0.f;
    s_ctx[k][j] = v;
  }
  __syncthreads();
  // k_static / v_static = W[:, :266] ctx_j.  Wk / Wv arrive TRANSPOSED ([266][128], k_transpose_static at create): thread = output row, so every
  // load instruction of a wavefront reads 256 contiguous bytes (one thread per output walking its own row of the (128, 522) matrix touched 64 cache
  // lines per instruction: 86 us per batch of 128 shapes; a wavefront per row with a lane reduction was a serial chain of round trips: 127 us);
  // the sum runs over k in order, as before: the same bits
  static_assert(NCLS == 4 && INNER == 128, "256 threads = 2 matrices x 128 rows, four context tokens per shape");
  {
    const int which = tid >> 7, row = tid & (INNER - 1);
    const float *wT = (which ? Wv : Wk) + row;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    // 38 loads in flight per thread: seven round trips to the L2 instead of one per unrolled group of eight (the kernel is a chain of round trips)
    constexpr int KB = 38;
    static_assert(CTX_STATIC % KB == 0, "266 = 7 x 38");
#pragma unroll 1
    for (int kb = 0; kb < CTX_STATIC; kb += KB) {
      float wv[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) wv[u] = wT[(size_t)(kb + u) * INNER];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const float4 cx = *reinterpret_cast<const float4 *>(s_ctx[kb + u]);
        a0 = fmaf(wv[u], cx.x, a0), a1 = fmaf(wv[u], cx.y, a1), a2 = fmaf(wv[u], cx.z, a2), a3 = fmaf(wv[u], cx.w, a3);
      }
    }
    *reinterpret_cast<float4 *>((which ? s_v : s_k)[row]) = make_float4(a0, a1, a2, a3);
  }
  if (tid < INNER) s_wqb[tid] = wqb[tid];
  __syncthreads();
  const float scale = 0.25f;  // dim_head ** -0.5 (attention.py:167)
  const size_t sb = (size_t)s * depth + b;
  char *rec = reinterpret_cast<char *>(out.as_ms) + sb * asms_bytes(PREC);
  void *tiles = rec;
  float *sbias = reinterpret_cast<float *>(rec + 8 * tile_bytes(PREC));
  // A_s (threads 0..127: channel = thread) and M_s (threads 128..255: output row = thread, Wo arrives TRANSPOSED): every weight load of a
  // wavefront is 256 contiguous bytes and serves the four tokens; the sums run over d in order (the same bits as one thread per output, which
  // read Wq / Wo with a 512-byte stride between lanes).  The 8 tiles are put together in LDS in fragment order and leave as whole lines.
  {
    const int c = tid & (INNER - 1);
    const bool ms = tid >= INNER;
    const float *wsrc = (ms ? Wo : Wq) + c;
    const float(*kv)[NCLS] = ms ? s_v : s_k;
    const float post = ms ? 1.f : scale * g2[c];
#pragma unroll 1
    for (int h0 = 0; h0 < INNER / DHEAD; h0 += 4) {   // four heads' weights (64 loads) in flight
      float wv[4 * DHEAD];
#pragma unroll
      for (int u = 0; u < 4 * DHEAD; ++u) wv[u] = wsrc[(size_t)(h0 * DHEAD + u) * INNER];
#pragma unroll
      for (int hh = 0; hh < 4; ++hh) {
      const int head = h0 + hh;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
      for (int d = 0; d < DHEAD; ++d) {
        const float w1 = wv[hh * DHEAD + d];
        const float4 t4 = *reinterpret_cast<const float4 *>(kv[head * DHEAD + d]);
        a0 = fmaf(w1, t4.x, a0), a1 = fmaf(w1, t4.y, a1), a2 = fmaf(w1, t4.z, a2), a3 = fmaf(w1, t4.w, a3);
      }
      const float av[4] = {a0, a1, a2, a3};
#pragma unroll
      for (int j = 0; j < NCLS; ++j) {
        // A_s: tile c / 32, row i = 4 head + j, column kk = c % 32;  M_s: tile 4 + c / 32, row i = c % 32, column kk = 4 head + j
        const int tile = (ms ? 4 : 0) + (c >> 5), i = ms ? (c & 31) : 4 * head + j, kk = ms ? 4 * head + j : (c & 31);
        s_out[tile * 1024 + tile_index<PREC>(i, kk)] = av[j] * post;
      }
      }
    }
  }
  __syncthreads();
  for (int gi = tid; gi < 8 * 1024; gi += 256) tile_store<PREC>(tiles, gi, s_out[gi]);
  if (tid < 32) {  // sbias in C-layout [hf][16]
    const int hf = tid >> 4, r = tid & 15, R = rho(r, hf), head = R >> 2, j = R & 3;
    float acc = 0.f;
    for (int d = 0; d < DHEAD; ++d) acc = fmaf(s_wqb[head * DHEAD + d], s_k[head * DHEAD + d][j], acc);
    // bf16 records carry the key mask here (denoiser_internal.h, "key mask"): the rows of an absent part start the A_s MFMAs from -FLT_MAX and leave
    // them as -FLT_MAX, the value the masked softmax used to select.  fp32 records keep the plain bias: the exact kernels select (softmax4<false>).
    sbias[tid] = PREC == DFX_PREC_BF16 && valid[(size_t)s * 4 + j] == 0.f ? -3.402823466e38f : acc * scale;
  } else if (tid < 256) {
    sbias[tid] = 0.f;  // pad of the 1 KiB piece
  }
  if (b == 0) {
    if (tid < 32) {
      float v = 0.f;
      if (tid < 12) v = mean[(size_t)s * 12 + tid];
      else if (tid < 24) v = var[(size_t)s * 12 + (tid - 12)];
      else if (tid < 28) v = valid[(size_t)s * 4 + (tid - 24)];
      out.part[(size_t)s * 32 + tid] = v;
    }
    // proj_in of the per-part constant inputs: [anchors | variances | onehot] + bias (attention.py:398-408)
    for (int o = tid; o < NCLS * INNER; o += 256) {
      const int j = o / INNER, ch = o % INNER;
      const float *w = win + (size_t)ch * IN_CH;
      float acc = bin[ch];
      for (int i = 0; i < 3; ++i) acc = fmaf(w[3 + i], s_ctx[ZDIM + i][j], acc);
      for (int i = 0; i < 3; ++i) acc = fmaf(w[6 + i], s_ctx[ZDIM + 3 + i][j], acc);
      acc += w[9 + j];
      out.cpart[((size_t)s * NCLS + j) * INNER + cvec_index(ch)] = acc;
    }
  }
}

struct Bump {
  char *base;
  size_t off = 0;
  template <typename T>
  T *take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

inline int nblk(long long total) { return (int)((total + 255) / 256); }

// anchored_diffusion.py:62-112, float64, then .float() as diffusion_utils.py:42-66 does at every use
void host_tables(int T, double beta_1, double beta_T, std::vector<float> &tabs /* [8][T] */, std::vector<float> &acp_f32,
                 std::vector<double> &ac_pv /* [2][T] */) {
  std::vector<double> betas(T), ac(T), acp(T);
  // np.linspace(beta_1, beta_T, num=T): arange(T) * step + start, last element forced to stop
  const double step = T > 1 ? (beta_T - beta_1) / (double)(T - 1) : 0.0;
  for (int i = 0; i < T; ++i) {
    volatile double prod = (double)i * step;  // keep mul and add separate (numpy does not fuse)
    betas[i] = prod + beta_1;
  }
  if (T > 1) betas[T - 1] = beta_T;
  double run = 1.0;
  for (int i = 0; i < T; ++i) {
    run *= (1.0 - betas[i]);
    ac[i] = run;
    acp[i] = i ? ac[i - 1] : 1.0;
  }
  tabs.assign((size_t)8 * T, 0.f);
  acp_f32.assign(T, 0.f);
  ac_pv.assign((size_t)2 * T, 0.0);
  for (int i = 0; i < T; ++i) {
    acp_f32[i] = (float)acp[i];
    ac_pv[i] = ac[i];
    ac_pv[(size_t)T + i] = betas[i] * (1.0 - acp[i]) / (1.0 - ac[i]);
    const double alpha = 1.0 - betas[i];
    const double sra = std::sqrt(1.0 / ac[i]);
    const double srm1 = std::sqrt(1.0 / ac[i] - 1);
    const double c1 = betas[i] * std::sqrt(acp[i]) / (1.0 - ac[i]);
    const double c2 = (1.0 - acp[i]) * std::sqrt(alpha) / (1.0 - ac[i]);
    const double c3 = 1.0 + ((std::sqrt(ac[i]) - 1.) * (std::sqrt(acp[i]) + std::sqrt(alpha))) / (1.0 - ac[i]);
    const double pv = betas[i] * (1.0 - acp[i]) / (1.0 - ac[i]);
    tabs[0 * (size_t)T + i] = (float)sra;
    tabs[1 * (size_t)T + i] = (float)srm1;
    tabs[2 * (size_t)T + i] = (float)c1;
    tabs[3 * (size_t)T + i] = (float)c2;
    tabs[4 * (size_t)T + i] = (float)c3;
    tabs[5 * (size_t)T + i] = (float)pv;
    tabs[6 * (size_t)T + i] = (float)std::sqrt(ac[i]);
    tabs[7 * (size_t)T + i] = (float)std::sqrt(1.0 - ac[i]);
  }
}

}  // namespace

extern "C" {

int dfx_denoiser_create(dfx_denoiser **out, const dfx_denoiser_weights *w, int T, double beta_1, double beta_T,
                        int precision, dfx_stream_t stream) {
  DFX_REQUIRE(out && w, "denoiser_create: null argument");
  *out = nullptr;
  DFX_REQUIRE(w->depth >= 1 && w->depth <= DFX_MAX_DEPTH, "denoiser_create: depth %d not in [1,%d]", w->depth,
              DFX_MAX_DEPTH);
  DFX_REQUIRE(T >= 1, "denoiser_create: num_timesteps must be >= 1");
  DFX_REQUIRE(precision == DFX_PREC_F32 || precision == DFX_PREC_BF16, "denoiser_create: unknown precision %d",
              precision);
  DFX_REQUIRE(beta_1 > 0 && beta_T <= 1 && beta_1 <= 1 && beta_T > 0, "denoiser_create: betas must lie in (0,1]");
  DFX_REQUIRE(w->proj_in_w && w->proj_in_b && w->pre_norm_w && w->pre_norm_b && w->post_norm_w && w->post_norm_b &&
                  w->proj_out_w && w->proj_out_b && w->te0_w && w->te0_b && w->te2_w && w->te2_b,
              "denoiser_create: null parameter pointer");
  const int depth = w->depth;
  for (int b = 0; b < depth; ++b) {
    const dfx_block_weights &k = w->blk[b];
    DFX_REQUIRE(k.norm2_w && k.norm2_b && k.to_q && k.to_k && k.to_v && k.to_out_w && k.to_out_b && k.norm3_w &&
                    k.norm3_b && k.ff0_w && k.ff0_b && k.ff2_w && k.ff2_b,
                "denoiser_create: null parameter pointer in block %d", b);
  }
  hipStream_t st = as_stream(stream);
  dfx_denoiser *d = new (std::nothrow) dfx_denoiser();
  if (!d) return set_error(DFX_ERR_ALLOC, "denoiser_create: host allocation failed");

  // two passes over the same carving code: measure, then place
  struct Carve {
    float *sinus, *h1, *h2, *temb, *vt, *y, *tab, *qtab;
    float4 *win_x, *wout;
    float2 *pre_gb;
    float *win, *bin;
    const float **wptrs;
    struct {
      uint4 *chunks;
      float *bconst, *ct, *wq, *wk, *wv, *wo, *g2, *be2, *wqb;
    } blk[DFX_MAX_DEPTH];
  } cv;
  auto carve = [&](char *base) {
    Bump bp{base};
    cv.sinus = bp.take<float>((size_t)T * TEMB);
    cv.h1 = bp.take<float>((size_t)T * 2048);
    cv.h2 = bp.take<float>((size_t)T * 1024);
    cv.temb = bp.take<float>((size_t)T * TEMB);
    cv.vt = bp.take<float>((size_t)T * INNER);
    cv.y = bp.take<float>((size_t)T * INNER);
    cv.tab = bp.take<float>((size_t)T * 8);
    cv.qtab = bp.take<float>((size_t)T * 2);
    cv.win_x = bp.take<float4>(INNER);
    cv.wout = bp.take<float4>(INNER);
    cv.pre_gb = bp.take<float2>(INNER);
    cv.win = bp.take<float>(INNER * IN_CH);
    cv.bin = bp.take<float>(INNER);
    cv.wptrs = bp.take<const float *>(DFX_MAX_DEPTH * 7);
    for (int b = 0; b < depth; ++b) {
      cv.blk[b].chunks = reinterpret_cast<uint4 *>(bp.take<char>((size_t)FF_STAGES * chunk_bytes(precision)));
      cv.blk[b].bconst = bp.take<float>(BCONST_BYTES / 4);
      cv.blk[b].ct = bp.take<float>((size_t)(T + 1) * CT_ROW);
      cv.blk[b].wq = bp.take<float>(INNER * INNER);
      cv.blk[b].wk = bp.take<float>(CTX_STATIC * INNER);   // static columns of to_k / to_v, transposed
      cv.blk[b].wv = bp.take<float>(CTX_STATIC * INNER);
      cv.blk[b].wo = bp.take<float>(INNER * INNER);
      cv.blk[b].g2 = bp.take<float>(INNER);
      cv.blk[b].be2 = bp.take<float>(INNER);
      cv.blk[b].wqb = bp.take<float>(INNER);
    }
    return bp.off;
  };
  d->pool_bytes = carve(nullptr);
  hipError_t e = hipMalloc(&d->pool, d->pool_bytes);
  if (e != hipSuccess) {
    delete d;
    return set_error(DFX_ERR_ALLOC, "denoiser_create: hipMalloc(%zu): %s", d->pool_bytes, hipGetErrorString(e));
  }
  carve(static_cast<char *>(d->pool));

  int rc = DFX_OK;
  void *swap_pool = nullptr;   // bf16 engines whose W1 bias fold moves to another channel: channel-exchanged copies of the parameters (freed below)
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(st);
    if (swap_pool) (void)hipFree(swap_pool);
    (void)hipFree(d->pool);
    delete[] d->host_tables;
    delete[] d->host_ac_pv;
    delete d;
    return code;
  };
#define TRY_HIP(expr)                                                                            \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) return fail(set_error(DFX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e))); \
  } while (0)
#define TRY_LAUNCH(what)                                   \
  do {                                                     \
    if ((rc = check_launch(what)) != DFX_OK) return fail(rc); \
  } while (0)

  // ---- schedule tables (host, float64) ----
  std::vector<float> tabs, acp_f32;
  std::vector<double> ac_pv;
  host_tables(T, beta_1, beta_T, tabs, acp_f32, ac_pv);
  d->host_tables = new float[(size_t)8 * T];
  std::memcpy(d->host_tables, tabs.data(), sizeof(float) * 8 * T);
  d->host_ac_pv = new double[(size_t)2 * T];
  std::memcpy(d->host_ac_pv, ac_pv.data(), sizeof(double) * 2 * T);
  std::vector<float> tab_dev((size_t)T * 8, 0.f);
  for (int i = 0; i < T; ++i) {
    for (int k = 0; k < 5; ++k) tab_dev[(size_t)i * 8 + k] = tabs[(size_t)k * T + i];
    tab_dev[(size_t)i * 8 + 5] = tabs[(size_t)5 * T + i];  // posterior_variance (sqrt taken with the point variance in-kernel)
    tab_dev[(size_t)i * 8 + 6] = acp_f32[i];               // alphas_cumprod_prev (DDIM, anchored_diffusion.py:481)
  }
  TRY_HIP(hipMemcpyAsync(cv.tab, tab_dev.data(), sizeof(float) * T * 8, hipMemcpyHostToDevice, st));
  std::vector<float> qtab_dev((size_t)T * 2);
  for (int i = 0; i < T; ++i) qtab_dev[(size_t)i * 2] = tabs[(size_t)6 * T + i], qtab_dev[(size_t)i * 2 + 1] = tabs[(size_t)7 * T + i];
  TRY_HIP(hipMemcpyAsync(cv.qtab, qtab_dev.data(), sizeof(float) * T * 2, hipMemcpyHostToDevice, st));

  // ---- sinusoidal embedding (host; nets/utils.py:7-24) ----
  std::vector<float> sinus((size_t)T * TEMB);
  {
    const int half = TEMB / 2;
    std::vector<float> freqs(half);
    const float neglog = (float)(-std::log(10000.0));
    for (int k = 0; k < half; ++k) freqs[k] = std::exp((neglog * (float)k) / (float)half);
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < half; ++k) {
        const float a = (float)t * freqs[k];
        sinus[(size_t)t * TEMB + k] = std::cos(a);
        sinus[(size_t)t * TEMB + half + k] = std::sin(a);
      }
  }
  TRY_HIP(hipMemcpyAsync(cv.sinus, sinus.data(), sizeof(float) * T * TEMB, hipMemcpyHostToDevice, st));

  // ---- bf16: b1' rides in ONE hidden channel's K slot of W1 (k_pack_w1; the kernels put the constant 1 into slot 127).  Any channel can be the
  // redundant one (the normalised row sums to zero), and the fold costs precision in proportion to that channel's column of W1' = W1 diag(gamma3)
  // (ADVICE r4): channel 127 is taken as it is while its column is ordinary (ratio <= W1_FOLD_KEEP_127); otherwise the channel whose column is
  // the smallest over all blocks is EXCHANGED with 127 in every parameter that touches the residual stream — a relabelling of the 128 hidden
  // channels, under which the network is the same function (LayerNorm, the residual adds and the matrix products commute with it) — and the
  // engine is packed from those copies (an outlier gamma3[127] used to send the engine to the ~3x slower direct kernel).  Only
  // when EVERY channel is an outlier of some block (> W1_FOLD_MAX_RATIO), or dfx_debug_w1_fold(0), the plain pack + direct kernel remain. ----
  int w1_fold = 0, fold_ch = -1;
  d->w1_fold_ratio = 0.f;
  dfx_denoiser_weights wswap;
  if (precision == DFX_PREC_BF16) {
    static_assert(FF_HID * 2 == 1024, "k_w1_fold_scores: one thread per row of W1");
    std::vector<float> sc((size_t)depth * INNER), score(INNER, 0.f);
    for (int b = 0; b < depth; ++b) {
      k_w1_fold_scores<<<1, 1024, 0, st>>>(w->blk[b].ff0_w, w->blk[b].norm3_w, cv.h1 + (size_t)b * INNER);   // (cv.h1: >= 2048 floats, not yet in use)
      TRY_LAUNCH("w1_fold_scores");
    }
    TRY_HIP(hipMemcpyAsync(sc.data(), cv.h1, sizeof(float) * depth * INNER, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < depth; ++b)
      for (int k = 0; k < INNER; ++k) score[k] = std::max(score[k], sc[(size_t)b * INNER + k]);
    int kmin = INNER - 1;
    for (int k = 0; k < INNER; ++k)
      if (score[k] < score[kmin]) kmin = k;
    if (g_w1_fold_mode == 1) fold_ch = INNER - 1;                                   // forced: the round-5 form
    else if (g_w1_fold_mode < 0) fold_ch = score[INNER - 1] <= W1_FOLD_KEEP_127 ? INNER - 1 : (score[kmin] <= W1_FOLD_MAX_RATIO ? kmin : -1);
    w1_fold = fold_ch >= 0;
    d->w1_fold_ratio = score[w1_fold ? fold_ch : INNER - 1];
    if (w1_fold && fold_ch != INNER - 1) {
      size_t floats = (size_t)INNER * IN_CH + 5 * INNER + 3 * INNER + (size_t)depth * (7 * INNER + 2 * (size_t)INNER * INNER + 2 * FF_HID * INNER + (size_t)INNER * FF_HID);
      TRY_HIP(hipMalloc(&swap_pool, floats * sizeof(float)));
      float *next = static_cast<float *>(swap_pool);
      bool bad = false;
      auto ex = [&](const float *src, int rows, int cols, int by_col) -> const float * {
        float *dst = next;
        next += (size_t)rows * cols;
        k_swap_channels<<<nblk((long long)rows * cols), 256, 0, st>>>(src, dst, rows, cols, by_col, fold_ch, INNER - 1);
        bad = bad || hipGetLastError() != hipSuccess;
        return dst;
      };
      wswap = *w;
      wswap.proj_in_w = ex(w->proj_in_w, INNER, IN_CH, 0), wswap.proj_in_b = ex(w->proj_in_b, INNER, 1, 0);
      wswap.pre_norm_w = ex(w->pre_norm_w, INNER, 1, 0), wswap.pre_norm_b = ex(w->pre_norm_b, INNER, 1, 0);
      wswap.post_norm_w = ex(w->post_norm_w, INNER, 1, 0), wswap.post_norm_b = ex(w->post_norm_b, INNER, 1, 0);
      wswap.proj_out_w = ex(w->proj_out_w, 3, INNER, 1);
      for (int b = 0; b < depth; ++b) {
        const dfx_block_weights &k = w->blk[b];
        dfx_block_weights &o = wswap.blk[b];
        o.norm2_w = ex(k.norm2_w, INNER, 1, 0), o.norm2_b = ex(k.norm2_b, INNER, 1, 0);
        o.to_q = ex(k.to_q, INNER, INNER, 1);                                              // (inner, hidden): the hidden channels are its columns
        o.to_out_w = ex(k.to_out_w, INNER, INNER, 0), o.to_out_b = ex(k.to_out_b, INNER, 1, 0);   // (hidden, inner)
        o.norm3_w = ex(k.norm3_w, INNER, 1, 0), o.norm3_b = ex(k.norm3_b, INNER, 1, 0);
        o.ff0_w = ex(k.ff0_w, 2 * FF_HID, INNER, 1);
        o.ff2_w = ex(k.ff2_w, INNER, FF_HID, 0), o.ff2_b = ex(k.ff2_b, INNER, 1, 0);
      }
      if (bad || (size_t)(next - static_cast<float *>(swap_pool)) > floats) return fail(set_error(DFX_ERR_HIP, "denoiser_create: channel exchange failed"));
      w = &wswap;   // everything below packs the relabelled network
    }
  }
  d->dev.w1_fold = w1_fold;
  d->w1_fold_channel = fold_ch;

  // ---- time_embed MLP for all t: Linear(256->2048) GEGLU Linear(1024->256) ----
  k_linear<<<nblk((long long)T * 2048), 256, 0, st>>>(cv.sinus, TEMB, w->te0_w, TEMB, 0, w->te0_b, cv.h1, T, 2048, TEMB);
  TRY_LAUNCH("time_embed.0");
  k_geglu<<<nblk((long long)T * 1024), 256, 0, st>>>(cv.h1, cv.h2, T, 1024);
  TRY_LAUNCH("time_embed.geglu");
  k_linear<<<nblk((long long)T * TEMB), 256, 0, st>>>(cv.h2, 1024, w->te2_w, 1024, 0, w->te2_b, cv.temb, T, TEMB, 1024);
  TRY_LAUNCH("time_embed.2");

  // ---- misc vectors ----
  TRY_HIP(hipMemcpyAsync(cv.win, w->proj_in_w, sizeof(float) * INNER * IN_CH, hipMemcpyDeviceToDevice, st));
  TRY_HIP(hipMemcpyAsync(cv.bin, w->proj_in_b, sizeof(float) * INNER, hipMemcpyDeviceToDevice, st));
  k_pack_misc<<<1, 128, 0, st>>>(w->proj_in_w, w->pre_norm_w, w->pre_norm_b, w->post_norm_w, w->proj_out_w, cv.win_x,
                                 cv.pre_gb, cv.wout);
  TRY_LAUNCH("pack_misc");
  {  // bout = proj_out.bias + W_out beta_post  (tiny: do it on the host)
    std::vector<float> wo(3 * INNER), bp(INNER), bo(3);
    TRY_HIP(hipMemcpyAsync(wo.data(), w->proj_out_w, sizeof(float) * 3 * INNER, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipMemcpyAsync(bp.data(), w->post_norm_b, sizeof(float) * INNER, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipMemcpyAsync(bo.data(), w->proj_out_b, sizeof(float) * 3, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) {
      float acc = 0.f;
      for (int k = 0; k < INNER; ++k) acc = std::fmaf(wo[(size_t)i * INNER + k], bp[k], acc);
      d->dev.bout[i] = bo[i] + acc;
    }
    d->dev.bout[3] = 0.f;
  }

  // ---- per block ----
  std::vector<const float *> wptrs((size_t)DFX_MAX_DEPTH * 7, nullptr);
  for (int b = 0; b < depth; ++b) {
    const dfx_block_weights &k = w->blk[b];
    auto &c = cv.blk[b];
    TRY_HIP(hipMemcpyAsync(c.wq, k.to_q, sizeof(float) * INNER * INNER, hipMemcpyDeviceToDevice, st));
    k_transpose_static<<<nblk((long long)CTX_STATIC * INNER), 256, 0, st>>>(k.to_k, c.wk);
    k_transpose_static<<<nblk((long long)CTX_STATIC * INNER), 256, 0, st>>>(k.to_v, c.wv);
    TRY_LAUNCH("transpose_static");
    k_transpose_sq<<<nblk((long long)INNER * INNER), 256, 0, st>>>(k.to_out_w, c.wo);   // Wo^T: k_shape_ctx reads it with thread = output row
    TRY_LAUNCH("transpose_wo");
    TRY_HIP(hipMemcpyAsync(c.g2, k.norm2_w, sizeof(float) * INNER, hipMemcpyDeviceToDevice, st));
    TRY_HIP(hipMemcpyAsync(c.be2, k.norm2_b, sizeof(float) * INNER, hipMemcpyDeviceToDevice, st));
    // c_t = Wo (Wv[:,266:] t_emb(t)) + b_o, cvec order
    k_linear<<<nblk((long long)T * INNER), 256, 0, st>>>(cv.temb, TEMB, k.to_v, CTX_DIM, CTX_STATIC, nullptr, cv.vt, T,
                                                       INNER, TEMB);
    TRY_LAUNCH("vt");
    k_linear<<<nblk((long long)T * INNER), 256, 0, st>>>(cv.vt, INNER, k.to_out_w, INNER, 0, nullptr, cv.y, T, INNER,
                                                       INNER);
    TRY_LAUNCH("ct");
    TRY_HIP(hipMemsetAsync(c.ct, 0, sizeof(float) * (size_t)(T + 1) * CT_ROW, st));
    TRY_HIP(hipMemsetAsync(c.bconst, 0, BCONST_BYTES, st));
    TRY_HIP(hipMemsetAsync(c.chunks, 0, (size_t)FF_STAGES * chunk_bytes(precision), st));
    k_to_cvec<<<nblk((long long)T * INNER), 256, 0, st>>>(cv.y, k.to_out_b, c.ct, T, CT_ROW);
    TRY_LAUNCH("ct_cvec");
    k_to_cvec<<<1, 256, 0, st>>>(k.ff2_b, nullptr, c.bconst + BCONST_B2_OFF, 1, INNER);
    TRY_LAUNCH("b2_cvec");
    k_pack_b1<<<nblk(FF_CHUNKS * 2 * 32), 256, 0, st>>>(k.ff0_w, k.ff0_b, k.norm3_b, c.bconst,
                                                        precision == DFX_PREC_BF16 ? FF_A_SCALE : 1.0f,
                                                        precision == DFX_PREC_BF16 ? FF_G_SCALE : 1.0f, precision == DFX_PREC_BF16);
    TRY_LAUNCH("pack_b1");
    if (precision == DFX_PREC_BF16) {
      k_pack_w1<DFX_PREC_BF16><<<nblk((long long)FF_CHUNKS * 8 * 1024), 256, 0, st>>>(k.ff0_w, k.norm3_w, c.chunks, k.ff0_b, k.norm3_b, w1_fold);
      k_pack_w2<DFX_PREC_BF16><<<nblk((long long)FF_CHUNKS * 4 * 1024), 256, 0, st>>>(k.ff2_w, c.chunks);
    } else {
      k_pack_w1<DFX_PREC_F32><<<nblk((long long)FF_CHUNKS * 8 * 1024), 256, 0, st>>>(k.ff0_w, k.norm3_w, c.chunks, k.ff0_b, k.norm3_b, 0);
      k_pack_w2<DFX_PREC_F32><<<nblk((long long)FF_CHUNKS * 4 * 1024), 256, 0, st>>>(k.ff2_w, c.chunks);
    }
    TRY_LAUNCH("pack_w1w2");
    d->dev.blk[b] = BlockPack{c.chunks, c.bconst, c.ct};
    d->wq[b] = c.wq; d->wk[b] = c.wk; d->wv[b] = c.wv; d->wo[b] = c.wo; d->g2[b] = c.g2; d->be2[b] = c.be2;
    k_wq_beta<<<1, INNER, 0, st>>>(k.to_q, k.norm2_b, c.wqb);
    TRY_LAUNCH("wq_beta");
    wptrs[(size_t)b * 7 + 0] = c.wq; wptrs[(size_t)b * 7 + 1] = c.wk; wptrs[(size_t)b * 7 + 2] = c.wv;
    wptrs[(size_t)b * 7 + 3] = c.wo; wptrs[(size_t)b * 7 + 4] = c.g2; wptrs[(size_t)b * 7 + 5] = c.be2; wptrs[(size_t)b * 7 + 6] = c.wqb;
  }
  TRY_HIP(hipMemcpyAsync(cv.wptrs, wptrs.data(), sizeof(const float *) * DFX_MAX_DEPTH * 7, hipMemcpyHostToDevice, st));
  TRY_HIP(hipStreamSynchronize(st));  // host staging vectors die here; user parameters no longer needed
  if (swap_pool) (void)hipFree(swap_pool), swap_pool = nullptr;
#undef TRY_HIP
#undef TRY_LAUNCH

  d->dev.depth = depth;
  d->dev.blk_stride = depth > 1 ? reinterpret_cast<const char *>(d->dev.blk[1].chunks) - reinterpret_cast<const char *>(d->dev.blk[0].chunks) : 0;
  for (int b = 1; b < depth; ++b) {   // the pipelined kernel addresses block b as block 0 + b * stride (no table look-up)
    const long long off = (long long)b * d->dev.blk_stride;
    if (reinterpret_cast<const char *>(d->dev.blk[b].chunks) != reinterpret_cast<const char *>(d->dev.blk[0].chunks) + off ||
        reinterpret_cast<const char *>(d->dev.blk[b].bconst) != reinterpret_cast<const char *>(d->dev.blk[0].bconst) + off ||
        reinterpret_cast<const char *>(d->dev.blk[b].ct) != reinterpret_cast<const char *>(d->dev.blk[0].ct) + off) {
      return fail(set_error(DFX_ERR_UNSUPPORTED, "denoiser_create: block packs are not uniformly strided"));
    }
  }
  d->dev.T = T;
  d->dev.prec = precision;
  d->dev.win_x = cv.win_x;
  d->dev.pre_gb = cv.pre_gb;
  d->dev.wout = cv.wout;
  d->dev.tab = cv.tab;
  d->dev.qtab = cv.qtab;
  d->win = cv.win;
  d->bin = cv.bin;
  d->wptrs_dev = cv.wptrs;
  *out = d;
  return DFX_OK;
}

void dfx_denoiser_destroy(dfx_denoiser *d) {
  if (!d) return;
  if (d->pool) (void)hipFree(d->pool);
  delete[] d->host_tables;
  delete[] d->host_ac_pv;
  delete d;
}

int dfx_denoiser_num_timesteps(const dfx_denoiser *d) { return d ? d->dev.T : 0; }
int dfx_denoiser_precision(const dfx_denoiser *d) { return d ? d->dev.prec : -1; }
int dfx_denoiser_w1_fold(const dfx_denoiser *d, float *ratio) {
  if (d && ratio) *ratio = d->w1_fold_ratio;
  return d ? d->dev.w1_fold : -1;
}
void dfx_debug_w1_fold(int mode) { g_w1_fold_mode = mode < 0 ? -1 : mode != 0; }
int dfx_debug_w1_fold_channel(const dfx_denoiser *d) { return d ? d->w1_fold_channel : -1; }

// Host-only views of denoiser_ff16.h (no GPU): what k_pack_w1 / k_pack_w2 write for a bf16 engine, as fp32 before the scale and the rounding,
// into `out` (FF_STAGES x CHUNK_TILES x 1024 floats, untouched where nothing is packed); layout = ff16::LAYOUT_*
void dfx_debug_ff16_pack_w1(const float *W1, const float *g3, const float *b1, const float *be3, int fold, int layout, float *out) {
  for (long long gi = 0; gi < ff16::W1_PACK_THREADS; ++gi) {
    const ff16::Src s = ff16::w1_source(gi, layout);
    out[s.di] = ff16::w1_value(W1, g3, b1, be3, s.row, s.col, fold);
  }
}
void dfx_debug_ff16_pack_w2(const float *W2, int layout, float *out) {
  for (long long gi = 0; gi < ff16::W2_PACK_THREADS; ++gi) {
    const ff16::Src s = ff16::w2_source(gi, layout);
    out[s.di] = W2[(size_t)s.row * FF_HID + s.col];
  }
}
// The fragments of a full FF record's M slot in issue order (24 rows of {uint4 offset, gemm (1 | 2), part (0 = a, 1 = g | -1), M-tile, K step | output tile})
void dfx_debug_ff16_slot_ops(int32_t *out) {
  for (int m = 0; m < 24; ++m) {
    const int k = m / 3, r = m % 3;
    const ff16::Op op = r == 0 ? ff16::gemm2_op(k) : ff16::gemm1_op(2 * k + r - 1);
    out[5 * m + 0] = ff16::ff_frag(m), out[5 * m + 1] = r == 0 ? 2 : 1, out[5 * m + 2] = op.part, out[5 * m + 3] = op.mt, out[5 * m + 4] = op.c;
  }
}

int dfx_denoiser_get_tables(const dfx_denoiser *d, float *host_out) {
  DFX_REQUIRE(d && host_out, "get_tables: null argument");
  std::memcpy(host_out, d->host_tables, sizeof(float) * 8 * (size_t)d->dev.T);
  return DFX_OK;
}

size_t dfx_shape_ctx_bytes(const dfx_denoiser *d, int B) {
  if (!d || B <= 0) return 0;
  return shape_ctx_view(nullptr, nullptr, B, d->dev.depth, d->dev.prec);
}

int dfx_shape_ctx_prepare(const dfx_denoiser *d, const float *part_code, const float *mean, const float *var,
                          const float *valid, void *ctx_out, int B, dfx_stream_t stream) {
  DFX_REQUIRE(d, "shape_ctx_prepare: null denoiser");
  DFX_REQUIRE(B >= 0, "shape_ctx_prepare: negative batch");
  if (B == 0) return DFX_OK;
  DFX_REQUIRE(part_code && mean && var && valid && ctx_out, "shape_ctx_prepare: null pointer");
  DFX_REQUIRE((reinterpret_cast<uintptr_t>(ctx_out) & 255) == 0, "shape_ctx_prepare: ctx_out must be 256-byte aligned");
  ShapeCtxView v;
  shape_ctx_view(&v, ctx_out, B, d->dev.depth, d->dev.prec);
  const float *const *wptrs = d->wptrs_dev;
  if (d->dev.prec == DFX_PREC_BF16)
    k_shape_ctx<DFX_PREC_BF16><<<B * d->dev.depth, 256, 0, as_stream(stream)>>>(part_code, mean, var, valid, wptrs,
                                                                              d->win, d->bin, v, d->dev.depth);
  else
    k_shape_ctx<DFX_PREC_F32><<<B * d->dev.depth, 256, 0, as_stream(stream)>>>(part_code, mean, var, valid, wptrs,
                                                                             d->win, d->bin, v, d->dev.depth);
  return check_launch("shape_ctx_prepare");
}

}  // extern "C"
