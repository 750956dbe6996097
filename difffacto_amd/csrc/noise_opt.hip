// libdfx: part re-configuration editing = gradient descent on the part aligner's cIMLE noise, many independent problems per call.
//
// Reference: tools/shape_edit.py:80-129 (Adam([z], lr 1) + ReduceLROnPlateau(factor 0.5, patience 10, min_lr 5e-2) + the torch.allclose stop) around
// AnchorDiffAE.edit_latent (python/difffacto/models/networks/anchor_gen.py:872-893) and parse_losses (utils/misc.py:120-132); tools/optimize_noise.py /
// optimize_latent (:895-913) is the same loop without the edit term.  The reference runs ONE shape per process with three host round trips per
// iteration; here every row r of the batch is a problem of its own (own Adam moments, learning rate, plateau counter, stop flag), and an iteration is
//   dfx_aligner_train_forward -> k_edit_loss -> dfx_aligner_input_backward -> k_noise_step
// enqueued back to back.  Exact fp32 like aligner_train.hip; nothing in a row's arithmetic depends on the other rows or on R.
#include <cmath>

#include "dfx_common.h"

namespace {

// per-row optimizer state (doubles where torch keeps Python floats: the learning rate, the scheduler's best, the previous loss)
struct RowState {
  double lr, best, prev;
  int num_bad, stopped;
};

struct St {
  float *d_mean, *d_logvar, *d_noise, *m, *v, *loss;   // loss (R, 4): L, fit, edit, reg
  RowState *row;
  int *n_stopped;
};
size_t carve(St &s, char *base, size_t off, int R, int J, int ND) {
  auto take = [&](size_t bytes) {
    off = (off + 255) & ~size_t(255);
    char *p = base ? base + off : nullptr;
    off += bytes;
    return p;
  };
  s.d_mean = reinterpret_cast<float *>(take((size_t)R * 3 * J * sizeof(float)));
  s.d_logvar = reinterpret_cast<float *>(take((size_t)R * 3 * J * sizeof(float)));
  s.d_noise = reinterpret_cast<float *>(take((size_t)R * ND * sizeof(float)));
  s.m = reinterpret_cast<float *>(take((size_t)R * ND * sizeof(float)));
  s.v = reinterpret_cast<float *>(take((size_t)R * ND * sizeof(float)));
  s.loss = reinterpret_cast<float *>(take((size_t)R * 4 * sizeof(float)));
  s.row = reinterpret_cast<RowState *>(take((size_t)R * sizeof(RowState)));
  s.n_stopped = reinterpret_cast<int *>(take(sizeof(int)));
  return off;
}

__global__ void k_noise_init(St s, int32_t *__restrict__ iters_done, int R, int ND, double lr0) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *s.n_stopped = 0;
  if (r >= R) return;
  for (int c = 0; c < ND; ++c) s.m[(size_t)r * ND + c] = 0.f, s.v[(size_t)r * ND + c] = 0.f;
  s.row[r] = RowState{lr0, INFINITY, 0.0, 0, 0};
  iters_done[r] = 0;
}

// One thread per row: the four loss values and d L_r / d mean, d L_r / d logvar (R, 3, J) (the reg term's gradient is added by k_noise_step).
//   fit  = sum_{c, j} f_j ((mean - fit_mean)^2 + (logvar - fit_logvar)^2) / sum_j f_j        (anchor_gen.py:877-879)
//   edit = sum_j em_j mean_c (mean - edit_mean)^2 + sum_j ev_j mean_c (logvar - edit_logvar)^2  (:880-888)
//   reg  = sum_c z_c^2                                                                          (:891-892)
__global__ void k_edit_loss(const float *__restrict__ mean, const float *__restrict__ logvar, const float *__restrict__ z, dfx_noise_opt_problem p, St s, int R,
                            int J, int ND) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float third = 1.0f / 3.0f, fw = (float)p.fit_weight;
  float fsum = 0.f;
  for (int j = 0; j < J; ++j) fsum += p.fix[(size_t)r * J + j];
  float fit = 0.f, edit = 0.f, reg = 0.f;
  for (int c = 0; c < 3; ++c)
    for (int j = 0; j < J; ++j) {
      const size_t i = ((size_t)r * 3 + c) * J + j;
      const float f = p.fix[(size_t)r * J + j];
      const float em = p.edit_mean_sel ? p.edit_mean_sel[(size_t)r * J + j] : 0.f, ev = p.edit_var_sel ? p.edit_var_sel[(size_t)r * J + j] : 0.f;
      const float am = mean[i] - p.fit_mean[i], al = logvar[i] - p.fit_logvar[i];
      fit += f * (am * am + al * al);
      float gm = fw * f * 2.0f * am / fsum, gl = fw * f * 2.0f * al / fsum;
      if (em != 0.f) {
        const float e = mean[i] - p.edit_mean[i];
        edit += em * third * e * e;
        gm += em * third * 2.0f * e;
      }
      if (ev != 0.f) {
        const float e = logvar[i] - p.edit_logvar[i];
        edit += ev * third * e * e;
        gl += ev * third * 2.0f * e;
      }
      s.d_mean[i] = gm, s.d_logvar[i] = gl;
    }
  fit /= fsum;
  for (int c = 0; c < ND; ++c) reg += z[(size_t)r * ND + c] * z[(size_t)r * ND + c];
  float *L = s.loss + (size_t)r * 4;
  L[0] = fw * fit + edit + (float)p.reg_weight * reg, L[1] = fit, L[2] = edit, L[3] = reg;
}

// One thread per row: g = d_noise + 2 reg_weight z; torch.optim.Adam (amsgrad off, no weight decay) with the learning rate in force before this
// iteration's scheduler step; ReduceLROnPlateau(mode min, threshold mode rel, cooldown 0) on L; the torch.allclose stop test against the previous L.
// A stopped row is never written again.  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step from the host (step = it + 1: every live row has stepped each iteration).
__global__ void k_noise_step(float *__restrict__ z, dfx_noise_opt_problem p, St s, int32_t *__restrict__ iters_done, float *__restrict__ trace, int R, int ND,
                             int it, double bc1, double bc2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  RowState st = s.row[r];
  if (st.stopped) return;
  const float L = s.loss[(size_t)r * 4];
  float *tr = trace ? trace + ((size_t)it * R + r) * (5 + 2 * ND) : nullptr;
  if (tr) {
    for (int k = 0; k < 4; ++k) tr[k] = s.loss[(size_t)r * 4 + k];
    tr[4] = (float)st.lr;
  }
  const float step_size = (float)(st.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const float w1 = (float)(1.0 - p.beta1), w2 = (float)(1.0 - p.beta2), beta2 = (float)p.beta2, eps = (float)p.adam_eps, reg2 = 2.0f * (float)p.reg_weight;
  for (int c = 0; c < ND; ++c) {
    const size_t i = (size_t)r * ND + c;
    const float zc = z[i], g = s.d_noise[i] + reg2 * zc;
    if (tr) tr[5 + c] = zc, tr[5 + ND + c] = g;
    const float m = s.m[i] + w1 * (g - s.m[i]);          // exp_avg.lerp_(grad, 1 - beta1)
    const float v = s.v[i] * beta2 + w2 * g * g;       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    s.m[i] = m, s.v[i] = v;
    z[i] = zc - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
  }
  // ReduceLROnPlateau.step(L)
  if ((double)L < st.best * (1.0 - p.threshold)) st.best = L, st.num_bad = 0;
  else ++st.num_bad;
  if (st.num_bad > p.patience) {
    const double nl = fmax(st.lr * p.factor, p.min_lr);
    if (st.lr - nl > p.lr_eps) st.lr = nl;
    st.num_bad = 0;
  }
  // torch.allclose(L, prev), prev starting at 0
  if (fabs((double)L - st.prev) <= p.stop_atol + p.stop_rtol * fabs(st.prev)) {
    st.stopped = 1;
    atomicAdd(s.n_stopped, 1);   // an integer count of stopped rows for the host's coarse early exit: no result depends on it
  }
  st.prev = L;
  s.row[r] = st;
  iters_done[r] = it + 1;
}

int check_problem(const dfx_latent_weights *w, int R, const char *who) {
  int rc = dfx::aligner_train_check(w, who);
  if (rc) return rc;
  DFX_REQUIRE(R > 0, "%s: R = %d", who, R);
  return DFX_OK;
}

constexpr int POLL_EVERY = 32;   // iterations between two reads of the stopped-row count

}  // namespace

extern "C" {

size_t dfx_noise_opt_workspace_bytes(const dfx_latent_weights *w, int R) {
  if (!w || R <= 0 || !w->cimle || w->noise_dim <= 0) return 0;
  const size_t a = dfx_aligner_train_workspace_bytes(R, w->n_class, w->zdim, w->noise_dim, w->n_heads, w->d_head, w->depth);
  if (!a) return 0;
  St s;
  return carve(s, nullptr, a, R, w->n_class, w->noise_dim);
}

int dfx_noise_opt_run(const dfx_latent_weights *w, void *workspace, size_t workspace_bytes, const dfx_noise_opt_problem *p, const float *part_code,
                      const float *valid, float *z, float *mean, float *logvar, int32_t *iters_done, float *trace, int R, int max_iter,
                      dfx_stream_t stream) {
  int rc = check_problem(w, R, "noise_opt_run");
  if (rc) return rc;
  DFX_REQUIRE(max_iter >= 0, "noise_opt_run: max_iter = %d", max_iter);
  DFX_REQUIRE(p && workspace && part_code && valid && z && mean && logvar && iters_done, "noise_opt_run: null argument");
  DFX_REQUIRE(p->fit_mean && p->fit_logvar && p->fix, "noise_opt_run: null fit target or mask");
  DFX_REQUIRE(!p->edit_mean_sel == !p->edit_mean && !p->edit_var_sel == !p->edit_logvar, "noise_opt_run: an edit selector and its target come together");
  DFX_REQUIRE(p->lr0 > 0 && p->beta1 >= 0 && p->beta1 < 1 && p->beta2 >= 0 && p->beta2 < 1 && p->adam_eps >= 0 && p->factor > 0 && p->factor < 1 &&
                  p->patience >= 0 && p->min_lr >= 0,
              "noise_opt_run: optimizer constants out of range");
  const size_t a = dfx_aligner_train_workspace_bytes(R, w->n_class, w->zdim, w->noise_dim, w->n_heads, w->d_head, w->depth);
  St s;
  DFX_REQUIRE(a && carve(s, static_cast<char *>(workspace), a, R, w->n_class, w->noise_dim) <= workspace_bytes, "noise_opt_run: workspace too small");
  hipStream_t st = dfx::as_stream(stream);
  const int J = w->n_class, ND = w->noise_dim, nb = (R + 63) / 64;
  if (trace && max_iter) DFX_HIP_TRY(hipMemsetAsync(trace, 0, (size_t)max_iter * R * (5 + 2 * ND) * sizeof(float), st));   // rows that stop early: zeros
  k_noise_init<<<nb, 64, 0, st>>>(s, iters_done, R, ND, p->lr0);
  for (int it = 0; it < max_iter; ++it) {
    if ((rc = dfx_aligner_train_forward(w, workspace, a, part_code, valid, z, mean, logvar, R, stream))) return rc;
    k_edit_loss<<<nb, 64, 0, st>>>(mean, logvar, z, *p, s, R, J, ND);
    if ((rc = dfx_aligner_input_backward(w, workspace, a, valid, s.d_mean, s.d_logvar, s.d_noise, nullptr, R, stream))) return rc;
    k_noise_step<<<nb, 64, 0, st>>>(z, *p, s, iters_done, trace, R, ND, it, 1.0 - pow(p->beta1, it + 1), 1.0 - pow(p->beta2, it + 1));
    if ((it + 1) % POLL_EVERY == 0 && it + 1 < max_iter) {
      int stopped = 0;
      DFX_HIP_TRY(hipMemcpyAsync(&stopped, s.n_stopped, sizeof(int), hipMemcpyDeviceToHost, st));
      DFX_HIP_TRY(hipStreamSynchronize(st));
      if (stopped == R) break;   // every row is frozen: further iterations would write nothing
    }
  }
  if ((rc = dfx_aligner_train_forward(w, workspace, a, part_code, valid, z, mean, logvar, R, stream))) return rc;
  return dfx::check_launch("noise_opt_run");
}

}  // extern "C"
