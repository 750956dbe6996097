#!/usr/bin/env python
"""The decision table of DESIGN.md 5.1b, read off the launcher's planner (csrc/denoiser_plan.h) through its host-only hook
dfx_debug_plan_variant — no GPU needed:

    python tools/launch_plan_table.py        # markdown: the automatic choice by batch size B, one row per N and engine

Paste the output over the table in DESIGN.md after re-measuring a cost constant or adding a variant."""
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


def main():
    build.build(verbose=False)
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
