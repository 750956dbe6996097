"""The training step's path and side-stream choice (csrc/train_plan.h: plan_train, plan_train_streams) through its host-only hook
dfx_debug_plan_train, against tests/golden/train_plan.npz: the decisions of the predicates this planner replaced (ff_fused, bf_store, the
dfx_debug_last_train_path expression, ss_mask, the two SideStream::open conditions and the SS_* tests behind them), recorded from those
lines compiled as a host program over precision x dropout x dfx_debug_train_fused x dfx_debug_train_streams x batch shapes.  Equality
on every row: changing a rule means regenerating the fixture on purpose.  (dfx_debug_train_fused(2) once kept the attention as kernels of
its own; since that path was retired the switch-2 rows hold the decisions of their switch-1 twins, copied inside the fixture by
tools/retire_split_attn_plan_fixture.py, not re-recorded.)"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "train_plan.npz")
F32, BF16 = 0, 1   # DFX_PREC_*
PATHS = ["LayerF32", "LayerBf16", "Fused"]
PATH_OF_CODE = {0: "LayerF32", 1: "LayerBf16", 3: "Fused"}   # 2 is retired and never reported
# dfx_debug_plan_train's bits (include/dfx_debug.h)
BITS = {"bf_store": 4, "dropout": 8, "fwd_ctx": 16, "bwd_open": 32, "head_early": 64, "stem_early": 128, "leaves": 256, "stem_end": 512}


@pytest.fixture(scope="module")
def plan():
    from difffacto_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.dfx_debug_plan_train.restype = ctypes.c_char_p
    lib.dfx_debug_plan_train.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)]

    def call(prec, p, fused_sw, streams, B, N):
        bits = ctypes.c_int(-1)
        name = lib.dfx_debug_plan_train(int(prec), float(p), int(fused_sw), int(streams), int(B), int(N), ctypes.byref(bits))
        d = {k: bool(bits.value & m) for k, m in BITS.items()}
        d["path"] = PATH_OF_CODE[bits.value & 3]
        d["record"] = name.decode()
        return d
    return call


def test_every_recorded_decision(plan):
    g = np.load(FIXTURE)
    names, paths = [str(n) for n in g["names"]], [str(n) for n in g["paths"]]
    assert paths == PATHS and len(names) == 6
    keys = ("prec", "p", "fused_sw", "streams", "B", "N")
    flags = ("bf_store", "fwd_ctx", "bwd_open", "head_early", "stem_early", "leaves", "stem_end")
    n = len(g["prec"])
    # the sweep: both precisions, p in {0, 0.2}, the three fused switches, streams off / default / every single bit, R = 32, 224, 256, 288 and large
    assert set(g["prec"]) == {F32, BF16} and set(g["p"].astype(np.float64).round(3)) == {0.0, 0.2} and set(g["fused_sw"]) == {0, 1, 2}
    assert {0, 1, 2, 4, 8, 16, 32} <= set(g["streams"]) and {32, 96, 2048} <= set(g["N"])
    assert {32, 224, 256, 288, 64 * 2048} <= set(g["B"].astype(np.int64) * g["N"])
    seen_records, seen_paths, wrong = set(), set(), []
    for r in range(n):
        args = tuple(g[k][r] for k in keys)
        got = plan(*args)
        want = {f: bool(g[f][r]) for f in flags}
        want.update(path=paths[g["path"][r]], record=names[g["record_index"][r]], dropout=bool(g["p"][r] > 0))
        seen_records.add(got["record"])
        seen_paths.add(got["path"])
        if got != want:
            wrong.append((args, got, want))
    assert not wrong, (len(wrong), wrong[:5])
    assert seen_records == set(names) and seen_paths == set(PATHS)


def test_bf16_below_256_rows_reports_layer_f32_and_keeps_its_precision(plan):
    """A bf16 step with fewer than 256 rows is the fp32-stored layer-by-layer path by name; its products are still asked for bf16 (they take
    the bf16 kernel where its shape rules allow), which is why the plan carries the precision beside the path."""
    for B, N in ((1, 32), (7, 32), (2, 96)):
        for sw in (0, 1, 2):
            d = plan(BF16, 0.0, sw, 1, B, N)
            assert (d["path"], d["record"], d["bf_store"]) == ("LayerF32", "layer_f32", False), (B, N, sw)
    assert plan(BF16, 0.0, 1, 1, 8, 32)["path"] == "Fused" and plan(BF16, 0.0, 1, 1, 2, 128)["path"] == "Fused"   # R = 256: the first fused shape
    assert plan(BF16, 0.2, 1, 1, 7, 32)["record"] == "layer_f32_dropout"


def test_switch_2_equals_switch_1(plan):
    """Any non-zero dfx_debug_train_fused selects the fused path: 2 (once the fused path with the attention as kernels of its own, layer by
    layer under dropout) gives the plan of 1 on every field, with and without dropout."""
    for p in (0.0, 0.2):
        for prec, B, N in ((BF16, 3, 2048), (BF16, 8, 32), (BF16, 7, 32), (F32, 3, 2048)):
            for streams in (0, 1, 2, 8 | 32):
                assert plan(prec, p, 2, streams, B, N) == plan(prec, p, 1, streams, B, N), (p, prec, B, N, streams)
    d = plan(BF16, 0.2, 2, 1, 3, 2048)
    assert (d["path"], d["record"], d["bf_store"], d["bwd_open"], d["stem_early"]) == ("Fused", "fused_bf16_dropout", True, True, True)
    assert plan(BF16, 0.0, 2, 1, 3, 2048)["record"] == "fused_bf16"
    assert plan(BF16, 0.2, 1, 1, 3, 2048)["record"] == "fused_bf16_dropout"
    assert plan(F32, 0.0, 1, 1, 3, 2048)["record"] == "layer_f32" and plan(BF16, 0.0, 0, 1, 3, 2048)["record"] == "layer_bf16"


def test_default_streams_and_explicit_masks(plan):
    d = plan(BF16, 0.0, 1, 1, 3, 2048)   # SS_DEFAULT = head early | stem early | leaves
    assert [d[k] for k in ("fwd_ctx", "bwd_open", "head_early", "stem_early", "leaves", "stem_end")] == [False, True, True, True, True, False]
    assert not any(plan(BF16, 0.0, 1, 0, 3, 2048)[k] for k in ("fwd_ctx", "bwd_open", "head_early", "stem_early", "leaves", "stem_end"))
    assert plan(BF16, 0.0, 1, -5, 3, 2048) == plan(BF16, 0.0, 1, 0, 3, 2048)   # dfx_debug_train_streams clamps negatives to off
    d = plan(BF16, 0.0, 1, 2, 3, 2048)   # the forward's context branch alone: the backward opens no side stream
    assert d["fwd_ctx"] and not d["bwd_open"]
    d = plan(BF16, 0.0, 1, 8 | 32, 3, 2048)   # early wins over end
    assert d["stem_early"] and not d["stem_end"]


def test_rejected_arguments_and_optional_pointer(plan):
    from difffacto_amd import _ffi
    L = _ffi.lib()
    assert L.dfx_debug_plan_train(BF16, 0.0, 1, 1, 3, 2048, None) == b"fused_bf16"
    for bad in ((2, 0.0, 1, 1, 3, 2048), (BF16, 1.0, 1, 1, 3, 2048), (BF16, -0.1, 1, 1, 3, 2048), (BF16, 0.0, 1, 1, 0, 2048), (BF16, 0.0, 1, 1, 3, 16),
                (BF16, 0.0, 1, 1, 3, 100)):
        assert L.dfx_debug_plan_train(*bad, None) is None, bad


def test_planner_header_compiles_alone_with_the_host_compiler(tmp_path):
    """train_plan.h is plain C++17 without HIP headers (like denoiser_plan.h): a host-only program that includes nothing else compiles."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler found"
    src = tmp_path / "plan_only.cpp"
    src.write_text('#include "difffacto_amd/csrc/train_plan.h"\n'
                   "int main() {\n"
                   "  const dfx::TrainPlan p = dfx::plan_train(DFX_PREC_BF16, 0.f, 2, 128, dfx::TrainSwitches{});\n"
                   "  return p.path == dfx::TrainPath::Fused && dfx::plan_train_streams(p.path, 1).leaves ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "plan_only"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    assert subprocess.run([str(exe)], timeout=30).returncode == 0


def test_no_hidden_parameters_left_in_the_training_host_code():
    src = open(os.path.join(ROOT, "difffacto_amd", "csrc", "train_kernels.hip")).read()
    for word in ("g_prec", "t_ff_fused", "t_attn_in_ff", "std::function", "ff_fused(", "ss_mask", "g_attn_in_ff", "attn_in_ff"):
        assert word not in src, word
