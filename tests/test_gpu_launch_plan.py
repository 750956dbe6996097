"""launch() takes the kernel its planner names: after single eps calls (T = 2), dfx_last_kernel_variant() against the host-only hook
dfx_debug_plan_variant with the same arguments (tests/test_launch_plan_cpu.py pins that hook's whole decision table on CPU; the results of
every variant are gated elsewhere)."""
import numpy as np
import pytest
import torch

from difffacto_amd import _ffi, synth
from _variants import forced

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1   # DFX_PREC_*

#        engine         code  B   N     the kernel, where the shape was chosen for one
CASES = [("bf16",       0,    1,  2048, "k_denoise_coop"),
         ("bf16",       0,    5,  2048, "k_denoise_coop2"),
         ("bf16",       0,    9,  2048, "k_denoise_pipe<4>"),
         ("bf16",       0,    17, 2048, "k_denoise_pipe<8>"),
         ("bf16",       0,    3,  32,   "k_denoise_coop"),
         ("bf16_nofold", 0,   3,  2048, "k_denoise<bf16>"),
         ("f32",        0,    3,  2048, None),
         ("f32",        0,    3,  96,   None),
         ("bf16",       16,   3,  2048, "k_denoise_coop2"),
         ("bf16",       16,   3,  96,   "k_denoise_coop")]


def test_launch_takes_the_planned_kernel():
    from difffacto_amd.engine import DenoiserEngine, last_kernel_variant
    L = _ffi.lib()
    tw = {k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()}
    engines = {"bf16": DenoiserEngine(tw, 2, precision="bf16"), "f32": DenoiserEngine(tw, 2, precision="f32")}
    L.dfx_debug_w1_fold(0)
    try:
        engines["bf16_nofold"] = DenoiserEngine(tw, 2, precision="bf16")
    finally:
        L.dfx_debug_w1_fold(-1)
    assert engines["bf16"].w1_fold()[0] and not engines["bf16_nofold"].w1_fold()[0]
    for key, code, B, N, expect in CASES:
        eng = engines[key]
        pc, mean, logvar, valid = synth.make_latents(B, seed=3)
        ctx = eng.prepare_shapes(*(torch.from_numpy(a) for a in (pc, mean, np.exp(logvar).astype(np.float32), valid)))
        x = torch.randn(B, 3, N, generator=torch.Generator().manual_seed(B * N))
        with forced(code):
            out = eng.eps(ctx, x, torch.from_numpy(synth.make_seg_mask(valid, N)), 1)
        took = last_kernel_variant()
        planned = L.dfx_debug_plan_variant(F32 if key == "f32" else BF16, int(key == "bf16"), 0, code, B, N, None).decode()
        assert took == planned and (expect is None or took == expect), (key, code, B, N, took, planned, expect)
        assert torch.isfinite(out).all()
