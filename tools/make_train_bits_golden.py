#!/usr/bin/env python
"""Writes tests/golden/train_bits/parent.json, the fixture of tests/test_gpu_train_bits.py: the SHA-256 of every output of one denoiser training
iteration per case of tests/_train_bits_case.py.  Run it once on the GPU with the library of the PARENT of the commit under test in
difffacto_amd/libdfx.so (the scheme of tools/make_chain_bits_golden.py) — never with the code the test is to judge.

    python tools/make_train_bits_golden.py [--out tests/golden/train_bits/parent.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import _train_bits_case as t
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=t.GOLDEN)
    args = ap.parse_args()
    ent = {}
    for case in t.CASES:
        ent[case[0]] = t.run_case(case)
        again = t.run_case(case)
        assert again == ent[case[0]], (case[0], sorted(k for k in again if again[k] != ent[case[0]][k]))
        print(f"{case[0]}: {len(ent[case[0]])} outputs, loss {ent[case[0]]['loss'][:16]}, eps {ent[case[0]]['eps'][:16]}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(ent, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
