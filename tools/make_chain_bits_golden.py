#!/usr/bin/env python
"""Writes tests/golden/chain_bits/chain_bits_parent.npz, the fixture of tests/test_gpu_chain_bits.py: the outputs of every bf16 denoiser kernel at its
smallest shape.  Run it on the GPU with the library of the PARENT of the commit under test in difffacto_amd/libdfx.so (the scheme of
tools/experiments/ab_so.sh: two prebuilt libraries copied over it in turn) — never with the code the test is to judge.

    python tools/make_chain_bits_golden.py [--out tests/golden/chain_bits/chain_bits_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "chain_bits", "chain_bits_parent.npz"))
    args = ap.parse_args()
    import test_gpu_chain_bits as t
    e = t.make_engine()
    ent = {}
    for case in t.CASES:
        out = t.run_case(e, case)
        for k, a in out.items():
            assert np.isfinite(a).all(), (case[0], k)
            print(f"{case[0]}.{k}: shape {a.shape}, |max| {np.abs(a).max():.4f}, sha256 {bytes(t.digest(a)).hex()[:16]}")
        ent.update(t.fixture_entries(case, out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez(args.out, **ent)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
