#!/usr/bin/env python
"""The decision table of DESIGN.md 5.1b, read off the launcher's planner (csrc/denoiser_plan.h) through its host-only hook
dfx_debug_plan_variant — no GPU needed:

    python tools/launch_plan_table.py          # markdown: the automatic choice by batch size B, one row per N and engine
    python tools/launch_plan_table.py --train  # markdown: the training step's path table of DESIGN.md 5.6 (csrc/train_plan.h, dfx_debug_plan_train)

Paste the output over the table in DESIGN.md after re-measuring a cost constant or adding a variant."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difffacto_amd import _ffi, build   # noqa: E402

NS = (32, 64, 96, 128, 256, 512, 1024, 2048, 8192)
ENGINES = (("bf16", 1, 1), ("bf16, no W1 fold", 1, 0), ("fp32", 0, 0))
BMAX = 512


def bands(prec, fold, N, code=0):
    """[(B_lo, B_hi, name)] of the choice for B = 1 .. BMAX."""
    out = []
    for B in range(1, BMAX + 1):
        name = _ffi.lib().dfx_debug_plan_variant(prec, fold, 0, code, B, N, None).decode()
        if out and out[-1][2] == name:
            out[-1][1] = B
        else:
            out.append([B, B, name])
    return out


def train_table():
    """path, record and side-stream use of a denoiser training step by precision, row count, dropout and dfx_debug_train_fused."""
    paths = {0: "layer by layer, fp32-stored", 1: "layer by layer, bf16-stored operands", 3: "fused"}   # (2: retired, never reported)
    side = ((16, "forward: context branch"), (64, "head sums early"), (128, "stem early"), (256, "leaves"), (512, "stem at the end"))

    def cells(prec, p, sw, B, N):
        bits = ctypes.c_int(0)
        rec = _ffi.lib().dfx_debug_plan_train(prec, p, sw, 1, B, N, ctypes.byref(bits)).decode()
        return paths[bits.value & 3], f"`{rec}`", ", ".join(n for m, n in side if bits.value & m) or "-"

    print("| precision | rows B N | dropout p | `dfx_debug_train_fused` | path | `dfx_debug_last_train_path` | beside the caller's stream (default `dfx_debug_train_streams`) |")
    print("|---|---|---|---|---|---|---|")
    for prec, B, N, label in ((0, 2, 128, "fp32 | any"), (1, 7, 32, "bf16 | < 256"), (1, 2, 128, "bf16 | >= 256")):
        for p in (0.0, 0.2):
            by_cells = {}   # switches that give the same plan share a row
            for sw in (1, 2, 0):
                by_cells.setdefault(cells(prec, p, sw, B, N), []).append(sw)
            for c, sws in by_cells.items():
                print(f"| {label} | {'0' if p == 0 else '> 0'} | {'any' if len(sws) == 3 else ', '.join(map(str, sws))} | {' | '.join(c)} |")


def main():
    build.build(verbose=False)
    if "--train" in sys.argv:
        return train_table()
    print(f"| engine | N | automatic choice for B = 1 .. {BMAX} |\n|---|---|---|")
    auto = set()
    for label, prec, fold in ENGINES:
        rows = []   # [N list, cells]: consecutive N with the same bands share a row
        for N in NS:
            bs = bands(prec, fold, N)
            auto |= {b[2] for b in bs}
            cells = "; ".join(f"{lo}{'' if lo == hi else ' ..' if hi == BMAX else f'-{hi}'}: `{name}`" for lo, hi, name in bs)
            if rows and rows[-1][1] == cells:
                rows[-1][0].append(N)
            else:
                rows.append([[N], cells])
        for ns, cells in rows:
            print(f"| {label} | {', '.join(map(str, ns))} | {cells} |")
    forced = {_ffi.lib().dfx_debug_plan_variant(prec, 1, 0, code, 3, 2048, None).decode() for prec in (0, 1) for code in (1, 2, 4, 8, 16)}
    print("\nOnly when forced (`dfx_debug_pipe_waves`, `dfx_debug_force_direct`):", ", ".join(f"`{n}`" for n in sorted(forced - auto)))


if __name__ == "__main__":
    main()
