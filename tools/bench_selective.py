"""Milliseconds and device memory of selective noise sampling (diverse generation) at the shipped size:

    python tools/bench_selective.py [--shapes 128] [--K 100] [--keep 10] [--timesteps 100] [--reps 7] [--out FILE]

S shapes x K aligner noises = S K candidate rows, of which S keep are kept, for both modes ('shape': the keep most different of every
shape; 'global': the S keep most different of all, farthest-point rule) and the first-pick rule.  Per mode, device-event medians
(min .. max) over --reps runs after one warm-up:

* pass       the aligner and the scores over all rows and nothing else: dfx_part_search_global with P = 1 (its selection is one
             step) for 'global', dfx_part_search 'first' with P = K plus the draw statistics and scores for 'shape';
* selection  the selection alone on the resident candidates: dfx_select_diverse_global / dfx_select_diverse (each includes its score
             kernel over the S K rows, one thread per row); for the global one also small batches of up to 512 rows on both of its
             launch paths (one workgroup for the whole call, the automatic choice there; one launch per pick, forced by
             dfx_debug_diverse_global_path);
* whole      LatentSampler.sample_latents_selective (flow, search, selection, compose of the kept rows);
* chain      the reverse chain on the kept rows (modules.decode).

For comparison: the farthest-point loop of the rule restated in plain torch on the same device scores (one pick per iteration,
float64 distances over the common parts), with its picks compared to the kernel's; and device memory of each path from a fresh
sampler, two figures: the growth of the device's used bytes (torch.cuda.mem_get_info) at the end of the call, which holds the
weights, libdfx's workspace (grow-only, so at its peak then) and torch's cached blocks but can miss torch temporaries already
returned to the driver; and the peak of torch's allocated bytes during the call (torch.cuda.max_memory_allocated), which sees
those temporaries and not libdfx's own allocations.  Synthetic weights.  Numbers only; not part of bench.py.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import numpy as np
import torch

from difffacto_amd import _ffi, part_sampling as psm, synth
from difffacto_amd.latents import LatentSampler
from difffacto_amd.modules import decode
from generate import build

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=int, default=128)
ap.add_argument("--K", type=int, default=100)
ap.add_argument("--keep", type=int, default=10)
ap.add_argument("--timesteps", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
S, K, KEEP, J, Z, ND, N = a.shapes, a.K, a.keep, 4, 256, 32, 2048
R, P = S * K, S * a.keep
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def timed(f, reps=a.reps):
    """One warm-up, then device events around each of `reps` runs: (last result, median, min, max) in ms."""
    out = f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, float(np.median(ms)), min(ms), max(ms)


def row(name, t):
    say(f"{name:<58s} {t[1]:9.3f} ms  ({t[2]:.3f} .. {t[3]:.3f})")
    return t[0]


def used():
    free, total = torch.cuda.mem_get_info()
    return total - free


def torch_farthest(scores, valid, K, P):
    """The farthest-point rule in plain torch: one arg-max per pick, float64 distances over the parts valid in both rows, a pair
    without a common part skipped, ties to the lowest index (torch.argmax of the first maximum is not guaranteed on the device, so
    the smallest index among the maxima is taken explicitly).  Finite rows assumed (synthetic inputs)."""
    sc = scores.double()
    m = valid.double().repeat_interleave(K, 0)
    R = sc.shape[0]
    mind = torch.full((R,), float("inf"), dtype=torch.float64, device=sc.device)
    free = torch.ones(R, dtype=torch.bool, device=sc.device)
    idx = torch.empty(P, dtype=torch.int64, device=sc.device)
    ar = torch.arange(R, device=sc.device)
    last = torch.zeros((), dtype=torch.int64, device=sc.device)
    idx[0] = 0
    free[0] = False
    for p in range(1, P):
        w = m * m[last]
        n = w.sum(1)
        d = (((sc - sc[last]) ** 2) * w[:, None, :]).sum((1, 2)) / n
        mind = torch.where(n > 0, torch.minimum(mind, d), mind)
        v = torch.where(free, mind, torch.full_like(mind, -1.0))
        last = torch.where(v == v.max(), ar, R).min()
        idx[p] = last
        free[last] = False
    return idx


W = synth.make_latent_weights(0)
rng = np.random.Generator(np.random.PCG64(0))
cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
w_noise = cu(rng.standard_normal((S, Z, J)).astype(np.float32))
noise = cu(rng.standard_normal((R, ND)).astype(np.float32))
valid = cu(synth.make_latents(S, seed=0)[3])
code_a = np.repeat(np.arange(S, dtype=np.int32)[:, None], J, 1)
enc, diff = build("gen_chair", a.timesteps, "bf16", 0)
diff.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()})
diff = diff.cuda().eval()

say(f"selective noise sampling: {S} shapes x K = {K} = {R} candidate rows -> {P} kept rows, n_class {J}, N = {N}, T = {a.timesteps} (bf16 chain), "
    f"median (min .. max) of {a.reps} after one warm-up; shapes with an absent part: {int((valid.sum(1) < J).sum())}")
sampler = LatentSampler(W, noise_scale=100.0)
code = sampler.flow_reverse(w_noise)
stats = psm.draw_stats(R, J, seed=1)
mean, logvar = sampler.part_aligner(code.repeat_interleave(K, 0), valid.repeat_interleave(K, 0), noise)

say("-- global --")
row("pass: aligner + draw statistics + scores, all rows (P = 1)", timed(lambda: sampler.part_search_global(code, code_a, valid, noise, K, 1, seed=1)))
sel = {}
for rule in ("farthest", "first_pick"):
    sel[rule] = row(f"selection alone, {rule} (scores + {P} picks, one launch per pick)",
                    timed(lambda: psm.select_diverse_global(mean, logvar, valid, K, P, rule=rule, stats=stats)))
row("selection alone, 1 pick (scores + state set-up)", timed(lambda: psm.select_diverse_global(mean, logvar, valid, K, 1, stats=stats)))
say("   small batches (farthest): one workgroup for the whole call (the automatic choice up to 512 rows) against one launch per pick")
for s_small in (1, 2, 4, 5):
    r_small = s_small * K
    for path, pname in ((-1, "one workgroup"), (1, "one launch per pick")):
        _ffi.lib().dfx_debug_diverse_global_path(path)
        row(f"   {s_small} shapes = {r_small} rows -> {s_small * KEEP} picks, {pname}",
            timed(lambda: psm.select_diverse_global(mean[:r_small], logvar[:r_small], valid[:s_small], K, s_small * KEEP, stats=stats[:r_small])))
_ffi.lib().dfx_debug_diverse_global_path(-1)
g = row("whole sample_latents_selective('global')", timed(lambda: sampler.sample_latents_selective(w_noise, noise, valid, "global", K=K, keep=KEEP, seed=1, npoints=N)))
per_shape = torch.bincount(g["source_row"], minlength=S)
say(f"    rows per shape: min {int(per_shape.min())} max {int(per_shape.max())}; n_bad {int(g['n_bad'])}")
row(f"chain on the {P} kept rows", timed(lambda: decode(diff, [g["part_code"], g["params"]], g["seg_mask"], valid_id=g["valid_id"], seed=0), reps=3))
t = timed(lambda: torch_farthest(sel["farthest"]["scores"], valid, K, P), reps=3)
row("torch restatement of the farthest-point loop (same scores)", t)
say(f"    picks equal to the kernel's: {100 * float((t[0] == sel['farthest']['idx'].long()).float().mean()):.2f} %")

say("-- shape --")
def shape_pass():
    o = sampler.part_search(code, code_a, valid, noise, K, "first", P=K)
    st = psm.draw_stats(R, J, seed=1)
    return o, st
row("pass: aligner ('first', P = K) + draw statistics", timed(shape_pass))
row(f"selection alone (scores + {KEEP} picks in each of {S} workgroups)", timed(lambda: psm.select_diverse(mean, logvar, valid, K, KEEP, stats=stats)))
s_ = row("whole sample_latents_selective('shape')", timed(lambda: sampler.sample_latents_selective(w_noise, noise, valid, "shape", K=K, keep=KEEP, seed=1, npoints=N)))
row(f"chain on the {P} kept rows", timed(lambda: decode(diff, [s_["part_code"], s_["params"]], s_["seg_mask"], valid_id=s_["valid_id"], seed=0), reps=3))
sampler.close()
del sampler, mean, logvar, g, s_, sel, t

say("-- device memory over one call from a fresh sampler: growth of the device's used bytes at the end of the call (weights, libdfx's grow-only")
say("   workspace, which is at its largest then, and what torch's allocator holds) | peak of torch's allocated bytes during the call --")
def grown(name, f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base, base_t = used(), torch.cuda.memory_allocated()
    s = LatentSampler(W, noise_scale=100.0)
    out = f(s)
    torch.cuda.synchronize()
    say(f"{name:<58s} {(used() - base) / 2 ** 20:9.0f} MiB | {(torch.cuda.max_memory_allocated() - base_t) / 2 ** 20:7.0f} MiB")
    s.close()
    del out
grown("sample_latents_selective('global')", lambda s: s.sample_latents_selective(w_noise, noise, valid, "global", K=K, keep=KEEP, seed=1, npoints=N))
grown("sample_latents_selective('shape')", lambda s: s.sample_latents_selective(w_noise, noise, valid, "shape", K=K, keep=KEEP, seed=1, npoints=N))
def plain(s):
    c = s.flow_reverse(w_noise)
    m, l = s.part_aligner(c.repeat_interleave(K, 0), valid.repeat_interleave(K, 0), noise)
    d = psm.select_diverse(m, l, valid, K, 1, stats=psm.draw_stats(R, J, seed=1))
    return torch_farthest(d["scores"], valid, K, P)
grown("torch: all candidate codes, one aligner call, torch loop", plain)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
