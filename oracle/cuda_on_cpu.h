/* CUDA-on-CPU shim (ORACLE — test infrastructure only).
 *
 * Runs a CUDA kernel that synchronises only through __syncthreads() (no warp intrinsics, no cooperative groups) as plain
 * C++ on one OS thread: one block at a time, every CUDA thread of the block a ucontext fibre that yields to the scheduler
 * at each barrier.  Deterministic by construction.
 *
 *   blocks    run one after the other, blockIdx.z outermost, then blockIdx.y, blockIdx.x innermost;
 *   threads   between two barriers the scheduler resumes every unfinished fibre of the block once, in ASCENDING linear
 *             thread index (x fastest) or in DESCENDING index — cuda_on_cpu::set_order(), read at each launch.  A fibre
 *             runs until its next __syncthreads() or until the kernel returns; a thread that has returned simply stops
 *             taking part (the remaining ones go on through their barriers);
 *   __shared__  is `static`: one array per kernel (per template instance), reused by every block and every launch —
 *             legitimate because blocks never overlap in time.  Like real shared memory it is NOT cleared between blocks;
 *   atomics   are plain read-modify-writes (one OS thread).
 *
 * The order is the only freedom a race-free kernel cannot observe; a kernel WITH a race observes it, which is what the
 * two orders are for: ascending = "last writer is the largest thread index", descending = "the smallest".
 *
 * Launch:  cuda_on_cpu::launch(dim3(gx, gy), dim3(bx), [&] { kernel<...>(args...); });
 */
#ifndef ORACLE_CUDA_ON_CPU_H
#define ORACLE_CUDA_ON_CPU_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <algorithm>
#include <functional>
#include <vector>

struct uint3 {
  unsigned x, y, z;
};
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

inline uint3 threadIdx, blockIdx;
inline dim3 blockDim, gridDim;

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static

using std::max;
using std::min;

namespace cuda_on_cpu {

enum { ASCENDING = 0, DESCENDING = 1 };
constexpr size_t STACK_BYTES = 64 * 1024;

struct Fibre {
  ucontext_t ctx;
  bool done;
};

inline int g_order = ASCENDING;
inline ucontext_t g_main;
inline std::vector<Fibre> g_fibres;
inline std::vector<char> g_stacks;
inline unsigned g_cur = 0;
inline bool g_inside = false;
inline const std::function<void()> *g_body = nullptr;

inline void set_order(int order) { g_order = order == DESCENDING ? DESCENDING : ASCENDING; }
inline int order() { return g_order; }

inline void trampoline() {
  (*g_body)();
  g_fibres[g_cur].done = true; /* uc_link takes control back to the scheduler */
}

inline void yield() { swapcontext(&g_fibres[g_cur].ctx, &g_main); }

inline void launch(dim3 grid, dim3 block, const std::function<void()> &body) {
  const unsigned nt = block.x * block.y * block.z;
  if (g_inside || nt == 0 || nt > 1024) {
    fprintf(stderr, "cuda_on_cpu: bad launch (%u threads%s)\n", nt, g_inside ? ", nested" : "");
    abort();
  }
  if (g_fibres.size() < nt) g_fibres.resize(nt);
  if (g_stacks.size() < (size_t)nt * STACK_BYTES) g_stacks.resize((size_t)nt * STACK_BYTES);
  g_inside = true;
  g_body = &body;
  const int ord = g_order;
  gridDim = grid;
  blockDim = block;
  for (unsigned bz = 0; bz < grid.z; ++bz)
    for (unsigned by = 0; by < grid.y; ++by)
      for (unsigned bx = 0; bx < grid.x; ++bx) {
        blockIdx = uint3{bx, by, bz};
        for (unsigned t = 0; t < nt; ++t) {
          Fibre &f = g_fibres[t];
          getcontext(&f.ctx);
          f.ctx.uc_stack.ss_sp = g_stacks.data() + (size_t)t * STACK_BYTES;
          f.ctx.uc_stack.ss_size = STACK_BYTES;
          f.ctx.uc_link = &g_main;
          makecontext(&f.ctx, trampoline, 0);
          f.done = false;
        }
        unsigned live = nt;
        while (live) { /* one pass = the stretch of code between two barriers */
          for (unsigned i = 0; i < nt; ++i) {
            const unsigned t = ord == ASCENDING ? i : nt - 1 - i;
            Fibre &f = g_fibres[t];
            if (f.done) continue;
            g_cur = t;
            threadIdx = uint3{t % block.x, (t / block.x) % block.y, t / (block.x * block.y)};
            swapcontext(&g_main, &f.ctx);
            if (f.done) --live;
          }
        }
      }
  g_body = nullptr;
  g_inside = false;
}

}  // namespace cuda_on_cpu

inline void __syncthreads() { cuda_on_cpu::yield(); }

inline int __float_as_int(float f) {
  int i;
  memcpy(&i, &f, sizeof i);
  return i;
}
inline float __int_as_float(int i) {
  float f;
  memcpy(&f, &i, sizeof f);
  return f;
}

inline int atomicCAS(int *address, int compare, int val) {
  const int old = *address;
  if (old == compare) *address = val;
  return old;
}
inline int atomicAdd(int *address, int val) {
  const int old = *address;
  *address = old + val;
  return old;
}
inline float atomicAdd(float *address, float val) {
  const float old = *address;
  *address = old + val;
  return old;
}

#endif
