// Which launch sequence a denoiser training step takes, and what of it goes to the side stream: pure host arithmetic on the precision, the
// dropout rate, the batch shape and the debug switches.  Plain C++17 without HIP headers, so a host-only program can compile it;
// train_kernels.hip holds one forward and one backward function per family of paths (forward_layered / forward_fused, backward_layered /
// backward_fused), dfx_debug_plan_train runs the planner without a GPU (tests/test_train_plan_cpu.py pins it to a table recorded from the
// predicates it replaced).
#pragma once
#include "../../include/dfx.h"   // DFX_PREC_*

namespace dfx {

enum class TrainPath {
  LayerF32,         // layer-by-layer kernels, fp32-stored activations
  LayerBf16,        // layer-by-layer kernels, product-only tensors stored as bf16
  Fused = 3,        // the default: the attention sub-block inside the feed-forward kernels, all blocks' forward in one launch
                    // (3: dfx_debug_plan_train reports the value; 2 was the split-attention path, retired)
};

// dfx_debug_train_streams: 0 = one stream, 1 = the default set, other values = explicit set of these bits (A/B)
enum { SS_FWD_CTX = 2, SS_HEAD_EARLY = 4, SS_STEM_EARLY = 8, SS_LEAVES = 16, SS_STEM_END = 32, SS_DEFAULT = SS_HEAD_EARLY | SS_STEM_EARLY | SS_LEAVES };

struct TrainSwitches {   // what dfx_debug_train_fused and dfx_debug_train_streams set
  bool fused = true;
  int streams = 1;
};
constexpr TrainSwitches train_switches_from_codes(int fused_code, int streams_code) {
  return TrainSwitches{fused_code != 0, streams_code < 0 ? 0 : streams_code};
}

struct TrainPlan {
  TrainPath path;
  int prec;              // what the products are asked for: a bf16 step below 256 rows is LayerF32 whose products still take the bf16 kernel where its shape rules allow
  bool bf_store;         // product-only tensors stored as bf16: every product over the points takes the bf16 kernel
  bool dropout;
  const char *record;    // dfx_debug_last_train_path()
  bool fused() const { return path == TrainPath::Fused; }
};

// The plan of a known path: what the backward rebuilds from the forward's record (same precision and dropout rate, checked there).
inline TrainPlan train_plan_of(TrainPath path, int prec, float dropout_p) {
  const bool dropout = dropout_p > 0.f;
  const char *record = path == TrainPath::LayerF32    ? (dropout ? "layer_f32_dropout" : "layer_f32")
                       : path == TrainPath::LayerBf16 ? (dropout ? "layer_bf16_dropout" : "layer_bf16")
                                                      : (dropout ? "fused_bf16_dropout" : "fused_bf16");
  return TrainPlan{path, prec, path != TrainPath::LayerF32, dropout, record};
}

// (B >= 1, N >= 32 and N % 32 == 0 are the entry points' argument checks: every row count is a multiple of the fused kernels' 32-point tile)
inline TrainPlan plan_train(int prec, float dropout_p, int B, int N, const TrainSwitches &sw) {
  const bool bf = prec == DFX_PREC_BF16 && (long long)B * N >= 256;   // fewer rows: no product over the points is sure of the bf16 kernel
  return train_plan_of(sw.fused && bf ? TrainPath::Fused : bf ? TrainPath::LayerBf16 : TrainPath::LayerF32, prec, dropout_p);
}

// What runs beside the caller's stream (fused path only; every launch keeps its kernel and operands, so the results are the same bits).
struct TrainStreams {
  bool fwd_ctx;      // forward: the context branch (time embedding -> context rows -> keys / values -> attention folds) on the side stream
  bool bwd_open;     // backward: the side stream is in use at all
  bool head_early;   // the head's partial sums right behind k_head_bwd (else: with the leaves, or on the caller's stream when !bwd_open)
  bool stem_early;   // pre_norm / proj_in backward right behind block 0's k_ff_bwd (its fp32 rows are final there)
  bool leaves;       // the finishing kernels behind the block loop that nothing on the way to the context gradient waits for
  bool stem_end;     // pre_norm / proj_in backward beside the finishing kernels (when not already done early)
};
inline TrainStreams plan_train_streams(TrainPath path, int streams_switch) {
  const int m = streams_switch == 1 ? SS_DEFAULT : streams_switch;
  const bool fused = path == TrainPath::Fused;
  TrainStreams s{};
  s.fwd_ctx = fused && (m & SS_FWD_CTX);
  s.bwd_open = fused && (m & ~SS_FWD_CTX);
  s.head_early = s.bwd_open && (m & SS_HEAD_EARLY);
  s.stem_early = s.bwd_open && (m & SS_STEM_EARLY);
  s.leaves = s.bwd_open && (m & SS_LEAVES);
  s.stem_end = s.bwd_open && !s.stem_early && (m & SS_STEM_END);
  return s;
}

}  // namespace dfx
