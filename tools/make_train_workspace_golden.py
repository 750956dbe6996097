#!/usr/bin/env python
"""Writes tests/golden/train_workspace_bytes.json, the fixture of tests/test_train_workspace_cpu.py: what the four training `*_workspace_bytes`
functions return at the shapes of tests/_train_workspace_case.py.  Run it with the library of the PARENT of the commit under test (the scheme of
tools/make_train_bits_golden.py) — never with the code the test is to judge.  No GPU needed.

    python tools/make_train_workspace_golden.py --lib path/to/the/parent's/libdfx.so [--out tests/golden/train_workspace_bytes.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import _train_workspace_case as t
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=t.GOLDEN)
    args = ap.parse_args()
    ent = t.sizes(t.load(args.lib))
    assert all(v > 0 for d in ent.values() for v in d.values()), ent
    with open(args.out, "w") as f:
        json.dump(ent, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, sum(len(d) for d in ent.values()), "sizes")


if __name__ == "__main__":
    main()
