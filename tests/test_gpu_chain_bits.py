"""Every output bit of every bf16 denoiser kernel against a fixture written by the PARENT of the commit that added this file
(tests/golden/chain_bits/chain_bits_parent.npz, written by tools/make_chain_bits_golden.py with that commit's library loaded, never by the code under
test).  A rewrite of the kernels' fp32 work outside the feed-forward loop (packing two IEEE operations into one instruction, another table
layout in LDS) must leave each half the same operation in the same order: this test is the judge of that, contraction included.

T = 3 chains and one eps evaluation at t = 1, explicit noise, seeded synthetic weights, each variant at its smallest shape:
  forced k_denoise_pipe<8> at B = 2, N = 256; forced pipe<4> at N = 128; forced pipe<2> at N = 64; k_denoise_coop at B = 1, N = 32;
  k_denoise_coop2 at the smallest batch the planner gives it by itself (N = 64, B = 129); the direct k_denoise<bf16>;
  one partial (FROM) chain: refine_chain, the forward noising in the prologue, on pipe<4>.
The fixture holds the outputs themselves; for the coop2 case (99 KiB per output) their SHA-256 and the first two shapes.  It has a directory of
its own: the fixtures directly under tests/golden/ are those of tests/golden/MANIFEST.sha256, which lists what make_golden.py regenerates."""
import hashlib
import os

import numpy as np
import pytest
import torch

import _variants

from difffacto_amd import synth

pytestmark = pytest.mark.gpu
T = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_bits", "chain_bits_parent.npz")

#        name       forced code (tests/_variants.py; None: dfx_debug_force_direct)   B    N    kernel        partial chain   digest only
CASES = [("pipe8",  8,    2,   256, "k_denoise_pipe<8>", False, False),
         ("pipe4",  4,    2,   128, "k_denoise_pipe<4>", False, False),
         ("pipe2",  2,    2,   64,  "k_denoise_pipe<2>", False, False),
         ("coop",   1,    1,   32,  "k_denoise_coop",    False, False),
         ("coop2",  0,    129, 64,  "k_denoise_coop2",   False, True),
         ("direct", None, 2,   64,  "k_denoise<bf16>",   False, False),
         ("from",   4,    2,   128, "k_denoise_pipe<4>", True,  False)]


def make_engine():
    from difffacto_amd.engine import DenoiserEngine
    W = {k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(seed=0).items()}
    return DenoiserEngine(W, num_timesteps=T, precision="bf16")


def run_case(e, case):
    """-> {key: float32 array} of the case's outputs, after asserting the kernel every launch took."""
    from difffacto_amd import _ffi
    from difffacto_amd.engine import last_kernel_variant
    name, code, B, N, kernel, partial, _ = case
    pc, mean, logvar, va = synth.make_latents(B, seed=1000 + N)
    cx = e.prepare_shapes(*map(torch.from_numpy, (pc, mean, np.exp(logvar).astype(np.float32), va)))
    sg = torch.from_numpy(synth.make_seg_mask(va, N))
    g = torch.Generator().manual_seed(7 * N + B)
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
        out[key] = np.ascontiguousarray(r.cpu().numpy(), dtype=np.float32)

    if partial:
        launch("chain", lambda: e.refine_chain(cx, sg, xT * 0.25, T, start_noise=sn[0], step_noise=sn)[0])
    else:
        launch("chain", lambda: e.sample_chain(cx, sg, x_T_noise=xT, step_noise=sn)[0])
        launch("eps", lambda: e.eps(cx, xT, sg, 1))
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def fixture_entries(case, out):
    """What the fixture keeps of a case's outputs (shared with tools/make_chain_bits_golden.py)."""
    ent = {}
    for key, a in out.items():
        if case[6]:
            ent[f"{case[0]}.{key}.sha256"] = digest(a)
            ent[f"{case[0]}.{key}.head"] = a[:2].copy()
        else:
            ent[f"{case[0]}.{key}"] = a
    return ent


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_engine()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_parent(engine, golden, case):
    got = fixture_entries(case, run_case(engine, case))
    assert got, case
    for k, a in got.items():
        want = golden[k]
        assert a.dtype == want.dtype and a.shape == want.shape, (k, a.dtype, a.shape, want.dtype, want.shape)
        if a.dtype == np.float32:
            assert np.isfinite(a).all(), k
            diff = a.view(np.uint32) != want.view(np.uint32)
            assert not diff.any(), f"{k}: {int(diff.sum())} of {a.size} values differ from the parent's bits, max-abs {np.abs(a - want).max():.3e}"
        else:
            assert np.array_equal(a, want), f"{k}: digest differs from the parent's"


def test_fixture_is_complete(golden):
    """Nothing in the fixture that no case reads, no output of a case that the fixture lacks (its keys are fixed by CASES alone)."""
    keys = set()
    for c in CASES:
        for key in (("chain",) if c[5] else ("chain", "eps")):
            keys |= {f"{c[0]}.{key}.sha256", f"{c[0]}.{key}.head"} if c[6] else {f"{c[0]}.{key}"}
    assert set(golden) == keys
