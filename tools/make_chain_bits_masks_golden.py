#!/usr/bin/env python
"""Writes tests/golden/chain_bits_masks/chain_bits_masks_parent.npz, the fixture of tests/test_gpu_softmax_masks_bits.py: the outputs of the bf16
denoiser kernels for one shape per presence pattern of the 4 parts.  Run it on the GPU with the library of the PARENT of the commit under test in
difffacto_amd/libdfx.so (the scheme of tools/make_chain_bits_golden.py and tools/experiments/ab_so.sh: two prebuilt libraries copied over it in
turn) — never with the code the test is to judge.

    python tools/make_chain_bits_masks_golden.py [--out tests/golden/chain_bits_masks/chain_bits_masks_parent.npz]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "chain_bits_masks", "chain_bits_masks_parent.npz"))
    args = ap.parse_args()
    import test_gpu_softmax_masks_bits as t
    e = t.make_engine()
    ent = {}
    for case in t.CASES:
        out = t.run_case(e, case)
        for k, a in out.items():
            assert np.isfinite(a).all(), k
            print(f"{k}: shape {a.shape}, |max| {np.abs(a).max():.4f}, sha256 {hashlib.sha256(a.tobytes()).hexdigest()[:16]}")
        ent.update(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez(args.out, **ent)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
