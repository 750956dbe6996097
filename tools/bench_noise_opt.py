"""Milliseconds per iteration of the aligner-noise optimization (part re-configuration editing), R rows at once:

    python tools/bench_noise_opt.py [--iters 200] [--rows 1,16,256]

* native: one dfx_noise_opt_run call (LatentSampler.optimize_noise), stop rule disabled so that every row runs all iterations;
* python: the reference-style loop (tools/shape_edit.py:80-129: Adam([z]) + ReduceLROnPlateau + a host read of the loss per iteration) over
  the same objective through training.AlignerTrainFn (dfx_aligner_train_forward + dfx_aligner_input_backward), rows batched in one call.

Synthetic weights and problems.  Numbers only; not part of bench.py.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from difffacto_amd import editing, synth, training
from difffacto_amd.latents import LatentSampler

ITERS = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 200
ROWS = [int(r) for r in (sys.argv[sys.argv.index("--rows") + 1] if "--rows" in sys.argv else "1,16,256").split(",")]

W = synth.make_latent_weights(0)
sampler = LatentSampler(W, noise_scale=100.0)
P = {k[len("part_aligner."):]: torch.from_numpy(v.copy()).cuda() for k, v in W.items() if k.startswith("part_aligner.")}


def problem(R, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    code = torch.from_numpy(rng.standard_normal((R, 256, 4)).astype(np.float32)).cuda()
    valid = torch.ones(R, 4)
    ref_mean = (rng.standard_normal((R, 3, 4)) * 0.3).astype(np.float32)
    ref_var = (rng.uniform(0.2, 0.6, size=(R, 3, 4)) ** 2).astype(np.float32)
    new_var = ref_var[:, :, 0] * np.array([1.0, 1.0, 1.2], np.float32)
    z0 = torch.from_numpy(rng.standard_normal((R, 32)).astype(np.float32)).cuda()
    prob = editing.noise_problem(valid, ref_mean, ref_var, [0, 1, 1, 1], 0, new_var=new_var, stop_atol=-1.0, stop_rtol=0.0)
    return code, valid.cuda(), z0, prob


def native(code, valid, z0, prob):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = sampler.optimize_noise(code, valid, z0, prob, ITERS)
    torch.cuda.synchronize()
    assert int(out["iters_done"].min()) == ITERS
    return (time.perf_counter() - t) * 1e3 / ITERS, float(editing.noise_losses(prob, out["mean"], out["logvar"], out["z"])["L"].mean())


def python_loop(code, valid, z0, prob):
    z = torch.nn.Parameter(z0.clone())
    opt = torch.optim.Adam([z], lr=1)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=10, min_lr=5e-2)
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in prob.items()}
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(ITERS):
        opt.zero_grad()
        mean, logvar = training.aligner_train_forward(P, code, valid, z, noise_scale=100.0)
        loss = editing.noise_losses(dev, mean, logvar, z)["L"].sum()      # rows stay independent under a sum; one learning rate for all (the reference's)
        loss.backward()
        opt.step()
        sched.step(loss)                                                   # reads the loss on the host, like the reference
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / ITERS, float(loss) / len(z0)


for R in ROWS:
    case = problem(R)
    native(*case)                                                          # warm-up: module load, allocator
    ms_n, L_n = native(*case)
    ms_p, L_p = python_loop(*case)
    print(f"R = {R:4d}  {ITERS} iterations: native {ms_n:.3f} ms/iteration (mean final L {L_n:.4f}), python loop {ms_p:.3f} ms/iteration (mean final L {L_p:.4f})")
