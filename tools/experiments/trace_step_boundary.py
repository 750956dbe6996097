"""Cycles per slot of k_denoise_pipe<8> around a step boundary, from the slot-boundary clock stamps of a library built with -DDFX_TRACE
(include/dfx_debug.h: dfx_debug_trace; stamps of wavefronts 0 = group A and 4 = group B of workgroup 0, which share a SIMD):

    python tools/experiments/trace_step_boundary.py [T] [B]        (defaults: T = 20, B = 128 shapes of 2048 points, bf16, in-kernel noise)

A block of a wavefront is 38 slots — V0 M0 V1 M1 V2, M(F0), then V M for the FF records 1 .. 16 — and 89 stamps (csrc/denoiser_kernel.hip:
DFX_SLOT stamps 1 = arrival at a record's management barrier, 2 = release, 3 = a slot boundary without a barrier; ff_m stamps 4 at its
first instruction, ff_v stamps 8 behind its last).  Per slot, for either group: the ticks from the slot's start (stamp 2 or 3) to the next
slot's first stamp, the wait at the barrier in front of it (1 -> 2) and, for an M slot of the feed-forward, the record-management stretch
between the barrier and the first MFMA (2 -> 4).  Printed: the block with the step boundary (block 0 of a step > 0), a block without one
(block 1), medians over the steps 1 .. T-1; V0 of the boundary block holds post_eps, the posterior, the noise draw, proj_in and LayerNorms."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from difffacto_amd import _ffi, synth  # noqa: E402
from difffacto_amd.engine import DenoiserEngine, last_kernel_variant  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
N, CAP, PER_BLOCK = 2048, 16384, 89

# stamps of one block, by group
PATTERN = {0: [3, 1, 2, 3, 3, 3, 1, 2, 4] + [3, 8, 1, 2, 4] * 16,
           1: [1, 2, 3, 3, 3, 1, 2, 3, 4] + [1, 2, 8, 3, 4] * 16}


def slots(g, t):
    """t: the block's 89 clock values + the next block's first -> {slot: ticks}"""
    s = {}
    if g == 0:
        s["V0"], s["wait M0"], s["M0"], s["V1"], s["M1"], s["V2"] = t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5]
        s["wait M(F0)"], s["mgmt M(F0)"], s["M(F0)"] = t[7] - t[6], t[8] - t[7], t[9] - t[8]
        v, w, m, mm = [], [], [], []
        for r in range(16):
            b = 9 + 5 * r
            v.append(t[b + 2] - t[b]), w.append(t[b + 3] - t[b + 2]), mm.append(t[b + 4] - t[b + 3]), m.append(t[b + 5] - t[b + 4])
    else:
        s["wait V0"], s["V0"], s["M0"], s["V1"], s["M1"] = t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4]
        s["wait V2"], s["V2"], s["mgmt M(F0)"], s["M(F0)"] = t[6] - t[5], t[7] - t[6], t[8] - t[7], t[9] - t[8]
        v, w, m, mm = [], [], [], []
        for r in range(16):
            b = 9 + 5 * r
            w.append(t[b + 1] - t[b]), v.append(t[b + 3] - t[b + 1]), mm.append(t[b + 4] - t[b + 3]), m.append(t[b + 5] - t[b + 4])
    s["FF V (steady, median of records 1..14)"] = float(np.median(v[:14]))
    s["FF wait (steady)"] = float(np.median(w[:14]))
    s["FF mgmt (steady)"] = float(np.median(mm[:14]))
    s["FF M (steady)"] = float(np.median(m[:14]))
    s["FF record (steady: V + wait + mgmt + M)"] = float(np.median([a + b_ + c + d for a, b_, c, d in zip(v[:14], w[:14], mm[:14], m[:14])]))
    s["M(F15)"], s["M(F16)"] = m[14], m[15]
    s["block"] = t[89] - t[0]
    return s


def main():
    W = synth.make_denoiser_weights(0)
    eng = DenoiserEngine({k: torch.from_numpy(v) for k, v in W.items()}, num_timesteps=T, precision="bf16")
    pc, m, lv, va = synth.make_latents(B, seed=1)
    ctx = eng.prepare_shapes(*map(torch.from_numpy, (pc, m, np.exp(lv).astype(np.float32), va)))
    seg = torch.from_numpy(synth.make_seg_mask(va, N))
    _ffi.lib().dfx_debug_pipe_waves(8)
    eng.sample_chain(ctx, seg, seed=1)
    buf = torch.zeros(2 * CAP, dtype=torch.int64, device="cuda")
    _ffi.lib().dfx_debug_trace(ctypes.c_void_p(buf.data_ptr()), CAP)
    eng.sample_chain(ctx, seg, seed=1)
    torch.cuda.synchronize()
    _ffi.lib().dfx_debug_trace(None, 0)
    fn = getattr(_ffi.lib(), "dfx_debug_last_chain_kind", None)   # (a library from before the PLAIN instantiations has none)
    if fn is not None:
        fn.restype = ctypes.c_char_p
    kind = fn().decode() if fn is not None else "general (the only one)"
    print(f"# {last_kernel_variant()}, instantiation: {kind}; B = {B} x {N} points, T = {T}, depth {eng.depth}; ticks of the stamp clock")
    tr = buf.cpu().numpy().reshape(2, CAP)
    nblocks = T * eng.depth
    rows = {}
    for g in range(2):
        t = tr[g]
        t = t[t != 0]
        tag, clk = ((t >> 56) & 0xff).astype(int), (t & ((1 << 56) - 1)).astype(np.int64)
        assert len(t) == nblocks * PER_BLOCK + 1, (len(t), nblocks * PER_BLOCK + 1, "a library without -DDFX_TRACE leaves the buffer empty")
        for kind_, b in (("boundary", 0), ("plain", 1)):
            acc = []
            for step in range(1, T):
                k = (step * eng.depth + b) * PER_BLOCK
                assert tag[k:k + PER_BLOCK].tolist() == PATTERN[g], (g, step, b, tag[k:k + PER_BLOCK].tolist())
                acc.append(slots(g, clk[k:k + PER_BLOCK + 1]))
            rows[(g, kind_)] = {key: float(np.median([a[key] for a in acc])) for key in acc[0]}
        rows[(g, "total")] = float(clk[-1] - clk[0])
    for g in range(2):
        print(f"# group {'AB'[g]} (wavefront {4 * g}): whole chain {rows[(g, 'total')]:.0f} ticks = {rows[(g, 'total')] / T:.0f} per step")
        print(f"{'slot':<46}{'block 0 of a step (boundary)':>30}{'block 1 (no boundary)':>24}{'difference':>12}")
        for key in rows[(g, "boundary")]:
            a, b = rows[(g, "boundary")][key], rows[(g, "plain")][key]
            print(f"{key:<46}{a:>30.0f}{b:>24.0f}{a - b:>12.0f}")


if __name__ == "__main__":
    main()
