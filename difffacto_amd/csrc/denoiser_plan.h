// Which chain kernel a denoiser launch takes, and with how many workgroups: pure host arithmetic on the engine's precision and W1 pack,
// the batch shape and the debug switches.  Plain C++17 without HIP headers, so a host-only program can compile it; denoiser_kernel.hip holds
// the kernels and their LDS sizes in an array of the same order (launch()), dfx_debug_plan_variant runs the planner without a GPU
// (tests/test_launch_plan_cpu.py pins it to a table recorded from the launcher it replaced).
#pragma once
#include "../../include/dfx.h"   // DFX_PREC_*

namespace dfx {

enum class Variant { Pipe8, Pipe4, Pipe2, Coop, Coop2, PipeF32_8, PipeF32_4, PipeF32_2, DirectBf16, DirectF32, COUNT };
constexpr int NUM_VARIANTS = (int)Variant::COUNT;

struct VariantInfo {
  const char *name;   // what dfx_last_kernel_variant() returns
  int threads;        // workgroup size
  int points;         // points of one workgroup
};
constexpr VariantInfo VARIANTS[NUM_VARIANTS] = {
    {"k_denoise_pipe<8>", 512, 256},     {"k_denoise_pipe<4>", 256, 128},     {"k_denoise_pipe<2>", 128, 64},
    {"k_denoise_coop", 512, 32},         {"k_denoise_coop2", 512, 64},        {"k_denoise_pipe_f32<8>", 512, 256},
    {"k_denoise_pipe_f32<4>", 256, 128}, {"k_denoise_pipe_f32<2>", 128, 64},  {"k_denoise<bf16>", 256, 128},
    {"k_denoise<f32>", 256, 128},
};
constexpr const VariantInfo &info(Variant v) { return VARIANTS[(int)v]; }

// dfx_debug_pipe_waves: the integer codes are the external interface (bench.py --pipe-waves, tools, tests), this is what they mean
enum class Force { Auto, Pipe8, Pipe4, Pipe2, CoopOrDirect, Coop2 };
constexpr Force force_from_code(int code) {
  switch (code) {
    case 8: return Force::Pipe8;
    case 4: return Force::Pipe4;
    case 2: return Force::Pipe2;
    case 1: return Force::CoopOrDirect;     // bf16: k_denoise_coop; fp32: the direct kernel
    case 16: return Force::Coop2;           // N % 64 != 0: k_denoise_coop
    default: return Force::Auto;            // (every other code, the retired 64, 160 and 161 among them)
  }
}

// ms per round of num_cus workgroups at N = 2048, T = 1000 (only the ratios matter).  Pipelined kernels by wavefronts per workgroup and the
// co-operative kernel: profiles/r02_small_batch_sweep.txt; k_denoise_coop2: between one and two rounds of k_denoise_coop (B = 5 .. 8 shapes of
// 2048 points) the cheapest.
constexpr double PIPE8_ROUND_MS = 93.5, PIPE4_ROUND_MS = 88.5, PIPE2_ROUND_MS = 86.5, COOP_ROUND_MS = 32.7, COOP2_ROUND_MS = 48.2;

struct PlanInput {
  int prec;            // DFX_PREC_F32 / DFX_PREC_BF16
  bool w1_fold;        // bf16 engine: b1' rides in the packed W1 (DenoiserDev::w1_fold)
  bool force_direct;   // dfx_debug_force_direct
  Force force;
  int B, N;
  int num_cus;
};
struct Plan {
  Variant v;
  long long grid;
};

// One workgroup per CU, so a launch runs in rounds of num_cus workgroups and the cheapest estimate wins.  The pipelined kernels work on tiles
// of nw x 32 points of one shape (a partial last tile idles whole wavefronts) with nw = 8, 4 or 2 wavefronts per workgroup — fewer wavefronts
// spread a small batch over more CUs; the co-operative ones put eight wavefronts on one (k_denoise_coop) or two (coop2)
// 32-point tiles.  Every variant of one precision produces the same bits.
inline Plan plan_launch(const PlanInput &in) {
  const int N = in.N, num_cus = in.num_cus;
  const long long waves = ((long long)in.B * N) / 32;
  auto tiles = [&](int nw) { return (long long)((N + nw * 32 - 1) / (nw * 32)); };
  auto fits = [&](int nw) { return tiles(nw) * nw * 32 <= 3LL * N; };   // ~3x faster per point than the direct kernels: unless the padding of a small shape eats that factor
  // a round that fills the fraction L of the chip's wavefront slots costs 1 + 0.36 L^4 times the base (the power cap)
  auto rounds_cost = [&](long long wgs, double base, double fill_per_wg) {
    const long long full = wgs / num_cus, rest = wgs % num_cus;
    auto f = [](double L) { return 1.0 + 0.36 * L * L * L * L; };
    return base * (full * f(num_cus * fill_per_wg) + (rest ? f(rest * fill_per_wg) : 0.0));
  };
  auto flat = [&](Variant v) { return Plan{v, ((long long)in.B * N + info(v).points - 1) / info(v).points}; };
  auto tiled = [&](Variant first, int nw) { return Plan{(Variant)((int)first + (nw == 8 ? 0 : nw == 4 ? 1 : 2)), tiles(nw) * in.B}; };

  // Eligibility.  A bf16 engine without the W1 bias fold (every hidden channel is an outlier of some block's W1', or dfx_debug_w1_fold(0)) has
  // the plain pack, which only the direct kernel reads: the chain kernels take b1' from slot 127.
  const bool bf16 = in.prec == DFX_PREC_BF16 && !in.force_direct && in.w1_fold, f32 = in.prec == DFX_PREC_F32 && !in.force_direct;
  const Force force = in.force;
  const bool automatic = force == Force::Auto;

  // Cost comparison: the pipelined kernel's cheapest nw (a forced one replaces it, its estimate `best` stays the automatic one) ...
  int nw = 8;
  double best = 1e300;
  for (int c = 8; c >= 2; c >>= 1) {
    if (!fits(c) && c > 2) continue;
    const double cost = rounds_cost(tiles(c) * in.B, c == 8 ? PIPE8_ROUND_MS : c == 4 ? PIPE4_ROUND_MS : PIPE2_ROUND_MS, c / (8.0 * num_cus));
    if (cost < best) best = cost, nw = c;
  }
  if (const int forced_nw = force == Force::Pipe8 ? 8 : force == Force::Pipe4 ? 4 : force == Force::Pipe2 ? 2 : 0) nw = forced_nw;
  const bool pipe = bf16 && fits(nw), pipe_f32 = f32 && force != Force::CoopOrDirect && fits(nw);   // (fp32 ignores Coop2)
  // ... against the co-operative kernels (coop2 needs N % 64 == 0; without a pipelined candidate k_denoise_coop takes up to one round)
  const double coop_cost = rounds_cost(waves, COOP_ROUND_MS, 0.0), coop2_cost = rounds_cost((waves + 1) / 2, COOP2_ROUND_MS, 0.0);
  const bool coop = bf16 && (force == Force::CoopOrDirect || (force == Force::Coop2 && N % 64 != 0) || (automatic && (pipe ? coop_cost < best : waves <= num_cus)));
  const bool coop2 = bf16 && N % 64 == 0 && (force == Force::Coop2 || (automatic && coop2_cost < coop_cost && (!pipe || coop2_cost < best)));

  // The first that applies; the direct kernels are the fallback of everything above.
  if (coop2) return flat(Variant::Coop2);
  if (coop) return flat(Variant::Coop);
  if (pipe) return tiled(Variant::Pipe8, nw);
  if (pipe_f32) return tiled(Variant::PipeF32_8, nw);
  return flat(in.prec == DFX_PREC_BF16 ? Variant::DirectBf16 : Variant::DirectF32);
}

}  // namespace dfx
