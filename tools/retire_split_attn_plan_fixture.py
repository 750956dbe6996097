#!/usr/bin/env python
"""How tests/golden/train_plan.npz followed the retirement of the split-attention training path (dfx_debug_train_fused(2) = 1): derived from the
recorded fixture itself, not from a run of the planner.  Every row with fused_sw == 2 takes the decisions of the row that differs from it only
in fused_sw == 1, and the path table loses FusedSplitAttn.

    python tools/retire_split_attn_plan_fixture.py OLD.npz NEW.npz
"""
import sys

import numpy as np

g = dict(np.load(sys.argv[1]))
keys = ("prec", "p", "streams", "B", "N")
decisions = ("path", "record_index", "bf_store", "fwd_ctx", "bwd_open", "head_early", "stem_early", "leaves", "stem_end")
row_of = {tuple(g[k][r].item() for k in keys): r for r in range(len(g["prec"])) if g["fused_sw"][r] == 1}
for r in np.flatnonzero(g["fused_sw"] == 2):
    for d in decisions:
        g[d][r] = g[d][row_of[tuple(g[k][r].item() for k in keys)]]
old = [str(n) for n in g["paths"]]
assert "FusedSplitAttn" not in {old[i] for i in g["path"]}
g["paths"] = np.array([n for n in old if n != "FusedSplitAttn"])
g["path"] = np.array([list(g["paths"]).index(old[i]) for i in g["path"]], dtype=g["path"].dtype)
np.savez_compressed(sys.argv[2], **g)
