"""Every output bit of the bf16 denoiser kernels' masked softmax, for EVERY presence pattern of the 4 parts, against a fixture written by the
PARENT of the commit that added this file (tests/golden/chain_bits_masks/chain_bits_masks_parent.npz, written by tools/make_chain_bits_masks_golden.py
with that commit's library loaded, never by the code under test).  tests/test_gpu_chain_bits.py sees only the patterns that synth.make_latents
draws for one or two shapes; the softmax of the attention slots on register pairs (softmax4<true> / attn_softmax) must leave each half the same
IEEE operation in the same order under every key mask — masked keys (exp of -FLT_MAX - m), a single live key (exp(0) / 1) and all four included.

B = 15: shape i carries the presence pattern i + 1 (bit j = part j present).  T = 2 chains and one eps evaluation at t = 1, explicit noise, seeded
synthetic weights, on k_denoise_coop at N = 32, forced k_denoise_pipe<2> at N = 64, forced k_denoise_pipe<8> at N = 256 and the direct
k_denoise<bf16> at N = 64; the kernel of every launch is asserted."""
import os

import numpy as np
import pytest
import torch

import _variants

from difffacto_amd import synth

pytestmark = pytest.mark.gpu
T = 2
B = 15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_bits_masks", "chain_bits_masks_parent.npz")

#        name      forced code (tests/_variants.py; None: dfx_debug_force_direct)   N    kernel
CASES = [("coop",   1,    32,  "k_denoise_coop"),
         ("pipe2",  2,    64,  "k_denoise_pipe<2>"),
         ("pipe8",  8,    256, "k_denoise_pipe<8>"),
         ("direct", None, 64,  "k_denoise<bf16>")]


def presence_patterns():
    """(15, 4) float32: every non-empty subset of the 4 parts, shape i = pattern i + 1."""
    return np.array([[(m >> j) & 1 for j in range(4)] for m in range(1, 16)], dtype=np.float32)


def make_engine():
    from difffacto_amd.engine import DenoiserEngine
    W = {k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(seed=0).items()}
    return DenoiserEngine(W, num_timesteps=T, precision="bf16")


def run_case(e, case):
    """-> {key: float32 array} of the case's outputs, after asserting the kernel every launch took."""
    from difffacto_amd import _ffi
    from difffacto_amd.engine import last_kernel_variant
    name, code, N, kernel = case
    pc, mean, logvar, _ = synth.make_latents(B, seed=2000 + N)
    va = presence_patterns()
    cx = e.prepare_shapes(*map(torch.from_numpy, (pc, mean, np.exp(logvar).astype(np.float32), va)))
    sg = torch.from_numpy(synth.make_seg_mask(va, N))
    g = torch.Generator().manual_seed(11 * N + B)
    xT, sn = torch.randn(B, 3, N, generator=g), torch.randn(T, B, 3, N, generator=g)
    out = {}

    def launch(key, fn):
        if code is None:
            _ffi.lib().dfx_debug_force_direct(1)
        try:
            with _variants.forced(code or 0):
                r = fn()
        finally:
            if code is None:
                _ffi.lib().dfx_debug_force_direct(0)
        assert last_kernel_variant() == kernel, f"{name}/{key}: expected {kernel}, the launch took {last_kernel_variant()}"
        out[f"{name}.{key}"] = np.ascontiguousarray(r.cpu().numpy(), dtype=np.float32)

    launch("chain", lambda: e.sample_chain(cx, sg, x_T_noise=xT, step_noise=sn)[0])
    launch("eps", lambda: e.eps(cx, xT, sg, 1))
    return out


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_engine()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_patterns_cover_every_mask():
    va = presence_patterns()
    assert va.shape == (B, 4) and sorted(int(sum(int(v) << j for j, v in enumerate(r))) for r in va) == list(range(1, 16))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_parent(engine, golden, case):
    got = run_case(engine, case)
    assert set(got) == {f"{case[0]}.chain", f"{case[0]}.eps"}
    for k, a in got.items():
        want = golden[k]
        assert a.dtype == want.dtype == np.float32 and a.shape == want.shape, (k, a.dtype, a.shape, want.dtype, want.shape)
        assert np.isfinite(a).all(), k
        diff = a.view(np.uint32) != want.view(np.uint32)
        shapes = sorted(set(np.nonzero(diff)[0].tolist()))
        assert not diff.any(), (f"{k}: {int(diff.sum())} of {a.size} values differ from the parent's bits, max-abs {np.abs(a - want).max():.3e}, "
                                f"presence patterns {[s + 1 for s in shapes]}")


def test_fixture_is_complete(golden):
    """Nothing in the fixture that no case reads, no output of a case that the fixture lacks."""
    assert set(golden) == {f"{c[0]}.{key}" for c in CASES for key in ("chain", "eps")}
