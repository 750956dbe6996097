// libdfx: error plumbing, version, event timing.
#include "dfx_common.h"

#include <cstring>
#include <map>
#include <mutex>
#include <utility>

namespace dfx {

static thread_local char t_err[512] = "";

char *err_buf() { return t_err; }

int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(t_err, sizeof(t_err), fmt, ap);
  va_end(ap);
  return code;
}

bool g_event_timing = false;
namespace lin {
int g_lin_split_k = -1;
}
float g_last_ms = -1.0f;
const char *g_last_variant = "";

void EventTimer::begin(hipStream_t s) {
  active = g_event_timing;
  if (!active) return;
  st = s;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
    active = false;
    return;
  }
  (void)hipEventRecord(a, st);
}

void EventTimer::end() {
  if (!active) return;
  (void)hipEventRecord(b, st);
  (void)hipEventSynchronize(b);
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, a, b) == hipSuccess) g_last_ms = ms;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  active = false;
}

namespace {
struct DevSide {
  hipStream_t st = nullptr;
  hipEvent_t ev[64] = {};
  std::atomic<unsigned> next{0};
};
std::mutex g_side_mu;
// One side stream + event ring per (device, caller's stream) — ADVICE r4: with one per device, independent calls on different streams or host threads were
// serialised through it, and a caller under stream capture put the shared stream into capture mode under everybody else's launches.  At most
// DFX_MAX_SIDE_STREAMS (64, dfx.h) pairs get one — entries are never evicted (a destroyed caller stream's handle may be reused by the runtime, and
// a side stream may sit inside somebody's captured graph) — and a caller beyond that runs WITHOUT a side stream (everything on its own stream:
// the same results, no overlap; ADVICE r5: sharing the first pair's stream brought back exactly the hazards above).
std::map<std::pair<int, hipStream_t>, DevSide *> g_side;

DevSide *dev_side(hipStream_t caller, bool &capped) {
  int dev = 0;
  capped = false;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) return nullptr;
  std::lock_guard<std::mutex> lk(g_side_mu);
  const auto key = std::make_pair(dev, caller);
  const auto it = g_side.find(key);
  if (it != g_side.end()) return it->second;
  if (g_side.size() >= 64) {
    capped = true;
    return nullptr;
  }
  DevSide *d = new DevSide;
  if (hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking) != hipSuccess) {
    delete d;
    return nullptr;
  }
  for (hipEvent_t &e : d->ev)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;   // (leaks a few handles on a broken device)
  g_side[key] = d;
  return d;
}
hipEvent_t next_event(DevSide *d) { return d->ev[d->next.fetch_add(1, std::memory_order_relaxed) & 63]; }
}  // namespace

int SideStream::open(hipStream_t caller, bool enable) {
  main = side = caller;
  on = false;
  if (!enable) return DFX_OK;
  bool capped = false;
  DevSide *d = dev_side(caller, capped);
  if (!d && capped) return DFX_OK;   // more than 64 (device, stream) pairs in this process: this caller gets no side stream (on == false)
  if (!d) return set_error(DFX_ERR_HIP, "side stream: cannot create the side stream / events");
  impl = d;
  side = d->st;
  on = true;
  return DFX_OK;
}
int SideStream::fork() {
  if (!on) return DFX_OK;
  hipEvent_t e = next_event(static_cast<DevSide *>(impl));
  DFX_HIP_TRY(hipEventRecord(e, main));
  DFX_HIP_TRY(hipStreamWaitEvent(side, e, 0));
  pending = true;
  return DFX_OK;
}
int SideStream::join() {
  if (!on) return DFX_OK;
  hipEvent_t e = next_event(static_cast<DevSide *>(impl));
  pending = false;
  DFX_HIP_TRY(hipEventRecord(e, side));
  DFX_HIP_TRY(hipStreamWaitEvent(main, e, 0));
  return DFX_OK;
}

}  // namespace dfx

// ---- box calibration (bench.py's `roofline.box_bare_mfma_tflops`): a bare stream of v_mfma_f32_32x32x16_bf16 with pseudo-random operands, one
// wavefront per SIMD on every CU, four independent accumulators (back-to-back issue), nothing else — what THIS chip sustains on the matrix pipe at
// its power cap and clocks right now (tools/ubench/pair_issue.hip's first row, inside the library so that the driver's bench line can normalise
// itself: boxes of this pool differ by several percent) ----
namespace dfx {
typedef float cal_v16f __attribute__((ext_vector_type(16)));
typedef __bf16 cal_v8bf __attribute__((ext_vector_type(8)));
__global__ void __launch_bounds__(256, 1) k_bare_mfma(float *out, int iters) {
  auto frag = [](unsigned seed) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned h = (seed + 0x9E3779B9u * (i + 1)) * 2654435761u;
      h ^= h >> 15;
      w[i] = (h & 0x807f807fu) | 0x3f003f00u | ((h >> 9) & 0x00800080u);   // two bf16 of magnitude 0.5 .. 2, random sign and mantissa
    }
    return __builtin_bit_cast(cal_v8bf, w);
  };
  const unsigned tid = threadIdx.x + 256u * blockIdx.x;
  const cal_v8bf a0 = frag(tid * 8 + 0), a1 = frag(tid * 8 + 1), a2 = frag(tid * 8 + 2), a3 = frag(tid * 8 + 3);
  const cal_v8bf b0 = frag(tid * 8 + 4), b1 = frag(tid * 8 + 5);
  cal_v16f c0, c1, c2, c3;
#pragma unroll
  for (int r = 0; r < 16; ++r) c0[r] = c1[r] = c2[r] = c3[r] = 0.f;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c1, 0, 0, 0);
      c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c2, 0, 0, 0);
      c3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, c3, 0, 0, 0);
      c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c1, 0, 0, 0);
      c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, c2, 0, 0, 0);
      c3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c3, 0, 0, 0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += c0[r] + c1[r] + c2[r] + c3[r];
  if (s == 12345.678f) out[0] = s;   // (keeps the accumulators alive)
}
}  // namespace dfx

extern "C" {

int dfx_debug_bare_mfma(int iters, float *ms_out, double *tflops_out, dfx_stream_t stream) {
  DFX_REQUIRE(iters > 0 && ms_out && tflops_out, "debug_bare_mfma: bad argument");
  hipStream_t st = dfx::as_stream(stream);
  int dev = 0, cus = 0;
  DFX_HIP_TRY(hipGetDevice(&dev));
  DFX_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  float *scratch = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  float ms = -1.f;
  // every exit passes the clean-up below: bench.py calls this several times per run
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&scratch), 256);
  if (e == hipSuccess) e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  if (e == hipSuccess) {
    dfx::k_bare_mfma<<<cus, 256, 0, st>>>(scratch, 16);   // code load
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(a, st);
  if (e == hipSuccess) {
    dfx::k_bare_mfma<<<cus, 256, 0, st>>>(scratch, iters);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(b, st);
  if (e == hipSuccess) e = hipEventSynchronize(b);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  if (scratch) (void)hipFree(scratch);
  if (e != hipSuccess || ms <= 0.f) return dfx::set_error(DFX_ERR_HIP, "debug_bare_mfma: %s", hipGetErrorString(e));
  *ms_out = ms;
  *tflops_out = (double)cus * 4.0 * iters * 16.0 * 32768.0 / (ms * 1e-3) / 1e12;   // executed MFMA flops: 2 x 32 x 32 x 16 each
  return DFX_OK;
}

int dfx_version(void) { return 108; }
int dfx_abi_version(void) { return DFX_ABI_VERSION; }

const char *dfx_last_error(void) { return dfx::err_buf(); }

void dfx_set_event_timing(int enable) { dfx::g_event_timing = enable != 0; }
void dfx_debug_lin_split_k(int mode) { dfx::lin::g_lin_split_k = mode < 0 ? -1 : (mode > 0 ? 1 : 0); }

float dfx_last_kernel_ms(void) { return dfx::g_last_ms; }

const char *dfx_last_kernel_variant(void) { return dfx::g_last_variant; }

}  // extern "C"
