#!/usr/bin/env python
"""What a partial reverse chain costs on the flagship shape (B = 128 x 2048 points, T = 1000, bf16):

    python tools/bench_refine.py [--batch 128] [--npoints 2048] [--timesteps 1000] [--runs 5] [--warmup 1] [--steps 100 250 500 1000]

times, device-synchronised, after --warmup calls, the median of --runs (>= 5) calls of
    sample_chain_from(n_steps)                  the last n_steps steps from a given state
    refine_chain(n_steps)                       q_sample fused into the prologue, then the same steps
    q_sample + sample_chain_from(n_steps)       the two-kernel composition
    sample_chain                                the whole generation chain
and prints, per entry and n_steps, ms and ms / n_steps, the fixed cost left by a least-squares line ms = a + b n_steps, and one JSON line.
Two facts are checked, nothing else is asserted: the whole chain through sample_chain_from (n_steps = T, from sample_chain's own first state: the same
trajectory, the same step loop behind another prologue), timed alternately with sample_chain, lies within sample_chain's run-to-run spread and gives
its bits; and every result is finite."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difffacto_amd import synth  # noqa: E402
from difffacto_amd.engine import DenoiserEngine, last_kernel_variant  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, nargs="*", default=None, help="n_steps to time (default: T/10, T/4, T/2, T)")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: a median of at least 5")
    T, B, N = a.timesteps, a.batch, a.npoints
    steps = sorted(set(a.steps)) if a.steps else sorted({max(1, T // 10), max(1, T // 4), max(1, T // 2), T})
    eng = DenoiserEngine({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()}, num_timesteps=T, precision=a.precision)
    part_code, mean, logvar, valid = synth.make_latents(B, seed=1)
    ctx = eng.prepare_shapes(*(torch.from_numpy(x) for x in (part_code, mean, np.exp(logvar).astype(np.float32), valid)))
    seg = torch.from_numpy(synth.make_seg_mask(valid, N)).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, 3, N, device="cuda", generator=g) * 0.2
    z = torch.randn(B, 3, N, device="cuda", generator=g)

    res = {"B": B, "N": N, "T": T, "precision": a.precision, "runs": a.runs, "n_steps": steps, "entries": {}}
    full_ms, (pred, _) = timed(lambda: eng.sample_chain(ctx, seg, seed=1), a.runs, a.warmup)
    res["kernel"] = last_kernel_variant()
    finite = bool(torch.isfinite(pred).all())
    res["sample_chain_ms"] = {"median": statistics.median(full_ms), "min": min(full_ms), "max": max(full_ms)}
    print(f"sample_chain ({res['kernel']}, B={B} N={N} T={T} {a.precision}): median {statistics.median(full_ms):.2f} ms "
          f"(min {min(full_ms):.2f}, max {max(full_ms):.2f}) = {statistics.median(full_ms) / T:.4f} ms/step")
    entries = {
        "sample_chain_from": lambda n: eng.sample_chain_from(ctx, seg, x, n, seed=1),
        "refine_chain": lambda n: eng.refine_chain(ctx, seg, x, n, seed=1),
        "q_sample+sample_chain_from": lambda n: eng.sample_chain_from(ctx, seg, eng.q_sample(ctx, seg, x, torch.full((B,), n - 1, dtype=torch.int32, device="cuda"), z), n, seed=1),
    }
    for name, call in entries.items():
        med = []
        res["entries"][name] = {}
        for n in steps:
            ms, (pred, _) = timed(lambda: call(n), a.runs, a.warmup)
            finite = finite and bool(torch.isfinite(pred).all())
            m = statistics.median(ms)
            med.append(m)
            res["entries"][name][str(n)] = {"median": m, "min": min(ms), "max": max(ms), "ms_per_step": m / n}
            print(f"{name:<28} n_steps {n:>5}: median {m:9.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}) = {m / n:.4f} ms/step")
        if len(steps) >= 2:
            slope, fixed = np.polyfit(np.asarray(steps, np.float64), np.asarray(med, np.float64), 1)
            res["entries"][name]["fit"] = {"fixed_ms": float(fixed), "ms_per_step": float(slope)}
            print(f"{name:<28} fit ms = {fixed:.2f} + {slope:.4f} n_steps")
    # the same step loop behind another prologue: the whole chain from sample_chain's own first state (the t = T snapshot, so both walk the same
    # trajectory, bit for bit), timed alternately with sample_chain
    _, first = eng.sample_chain(ctx, seg, seed=1, ret_interval=T)
    x_T = first[0].transpose(1, 2).contiguous()
    del first
    pair = {"sample_chain": [], "sample_chain_from": []}
    same = True
    for i in range(a.warmup + a.runs):
        for name, call in (("sample_chain", lambda: eng.sample_chain(ctx, seg, seed=1)), ("sample_chain_from", lambda: eng.sample_chain_from(ctx, seg, x_T, T, seed=1))):
            ms, (p, _) = timed(call, 1, 0)
            if name == "sample_chain":
                want = p
            else:
                same = same and torch.equal(p, want)
            if i >= a.warmup:
                pair[name] += ms
    spread = max(pair["sample_chain"]) - min(pair["sample_chain"])
    diff = statistics.median(pair["sample_chain_from"]) - statistics.median(pair["sample_chain"])
    verdict = abs(diff) <= spread
    res["from_T_vs_sample_chain"] = {"sample_chain_ms": pair["sample_chain"], "sample_chain_from_ms": pair["sample_chain_from"], "diff_ms": diff,
                                     "spread_ms": spread, "within_spread": verdict, "same_bits": same}
    print(f"alternating, same trajectory (bits equal: {same}): sample_chain median {statistics.median(pair['sample_chain']):.2f} ms "
          f"(min {min(pair['sample_chain']):.2f}, max {max(pair['sample_chain']):.2f}), sample_chain_from(n_steps = T) median "
          f"{statistics.median(pair['sample_chain_from']):.2f} ms (min {min(pair['sample_chain_from']):.2f}, max {max(pair['sample_chain_from']):.2f}); "
          f"difference {diff:+.2f} ms, run-to-run spread of sample_chain {spread:.2f} ms: {'within' if verdict else 'OUTSIDE'}")
    res["finite"] = finite
    print(json.dumps(res), flush=True)
    if not (finite and same and verdict):
        sys.exit(1)


if __name__ == "__main__":
    main()
