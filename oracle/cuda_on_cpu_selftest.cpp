/* Toy kernels that hold oracle/cuda_on_cpu.h to its contract (ORACLE — test infrastructure only; written for the test, nothing
 * here comes from the reference).  Built by oracle/refkernels.py, called by tests/test_refkernels_cpu.py. */
#include "cuda_on_cpu.h"

namespace {

/* block-wide tree sum with a barrier per level; every block writes its sum */
__global__ void tree_sum(const int *in, int n, int *out) {
  __shared__ int buf[256];
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  buf[threadIdx.x] = gid < n ? in[gid] : 0;
  __syncthreads();
  for (unsigned s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) buf[threadIdx.x] += buf[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = buf[0];
}

/* odd threads leave before the first barrier; the even ones go through two more and see each other's writes */
__global__ void early_return(int *out) {
  __shared__ int buf[64];
  out[threadIdx.x] = -1;
  if (threadIdx.x & 1) return;
  buf[threadIdx.x] = 100 + threadIdx.x;
  __syncthreads();
  const int other = buf[(threadIdx.x + 2) % blockDim.x];
  __syncthreads();
  buf[threadIdx.x] = other;
  __syncthreads();
  out[threadIdx.x] = buf[threadIdx.x];
}

/* a __shared__ array is one static object: block k sees what block k-1 left (never cleared), a second launch what the first left */
__global__ void shared_reuse(int *seen) {
  __shared__ int stamp[1];
  if (threadIdx.x == 0) seen[blockIdx.y * gridDim.x + blockIdx.x] = stamp[0];
  __syncthreads();
  if (threadIdx.x == blockDim.x - 1) stamp[0] = 1000 * (blockIdx.y + 1) + blockIdx.x + 1;
}

/* every thread writes its index to one word without a barrier: the schedule decides who is last */
__global__ void last_writer(int *slot) {
  __syncthreads();
  slot[blockIdx.x] = threadIdx.x;
}

/* the index variables, 2-D block and grid: out[linear block][linear thread] = packed indices */
__global__ void indices(int *out) {
  const unsigned nt = blockDim.x * blockDim.y, t = threadIdx.y * blockDim.x + threadIdx.x;
  const unsigned blk = blockIdx.y * gridDim.x + blockIdx.x;
  __syncthreads();
  out[blk * nt + t] = (int)(((blockIdx.y * 16 + blockIdx.x) * 16 + threadIdx.y) * 16 + threadIdx.x);
}

/* atomics and bit casts: a float maximum by compare-and-swap, an int and a float sum */
__global__ void atomics(const float *in, float *fmax, int *count, float *fsum) {
  const float v = in[threadIdx.x];
  int ret = __float_as_int(*fmax);
  while (v > __int_as_float(ret)) {
    const int old = ret;
    if ((ret = atomicCAS((int *)fmax, old, __float_as_int(v))) == old) break;
  }
  atomicAdd(count, 1);
  __syncthreads();
  atomicAdd(fsum, min(max(v, 0.f), 2.f));
}

}  // namespace

extern "C" {
void selftest_schedule(int order) { cuda_on_cpu::set_order(order); }
void selftest_tree_sum(const int *in, int n, int block, int *out) {
  cuda_on_cpu::launch(dim3((n + block - 1) / block), dim3(block), [=] { tree_sum(in, n, out); });
}
void selftest_early_return(int block, int *out) { cuda_on_cpu::launch(dim3(1), dim3(block), [=] { early_return(out); }); }
void selftest_shared_reuse(int gx, int gy, int block, int *seen) {
  cuda_on_cpu::launch(dim3(gx, gy), dim3(block), [=] { shared_reuse(seen); });
}
void selftest_last_writer(int blocks, int block, int *slot) {
  cuda_on_cpu::launch(dim3(blocks), dim3(block), [=] { last_writer(slot); });
}
void selftest_indices(int gx, int gy, int bx, int by, int *out) {
  cuda_on_cpu::launch(dim3(gx, gy), dim3(bx, by), [=] { indices(out); });
}
void selftest_atomics(const float *in, int block, float *fmax, int *count, float *fsum) {
  cuda_on_cpu::launch(dim3(1), dim3(block), [=] { atomics(in, fmax, count, fsum); });
}
}
