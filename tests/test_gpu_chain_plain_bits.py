"""The plain-generation (PLAIN) instantiations of the five bf16 chain kernels against their GENERAL instantiations, bit for bit, and the key
mask that dfx_shape_ctx_prepare writes into the bf16 attention records' sbias.

A dfx_sample_chain launch with in-kernel Philox noise and no snapshots takes the PLAIN instantiation of its kernel (csrc/denoiser_kernel.hip:
ChainKind, plain_launch), in which the mode selects of KParams are compile-time facts; dfx_debug_chain_general(1) makes the same launch take
the GENERAL one, which tests them at run time.  Every bit of `pred` must agree.  T = 4 throughout; B = 15, shape i carries the presence
pattern i + 1 of the 4 parts; k_denoise_pipe<8> at N = 256 and at N = 288 (a ragged last tile: seven of its eight wavefronts store nothing),
k_denoise_pipe<4> at N = 128, k_denoise_pipe<2>, k_denoise_coop and k_denoise_coop2 at N = 64, each forced by dfx_debug_pipe_waves; two
seeds that differ only in the high word, and a shape_offset beyond 2^32.  The kernel name and the instantiation of every launch are asserted
(dfx_last_kernel_variant, dfx_debug_last_chain_kind).  A launch that asks for snapshots is not plain: it takes GENERAL whatever the switch says.

The mask: the sbias rows of an absent part hold -FLT_MAX in a bf16 context (the A_s MFMAs start from sbias, so the softmax needs no select),
every other entry is what a context with all four parts present holds; an fp32 context carries no mask (the exact kernels select)."""
import contextlib

import numpy as np
import pytest
import torch

import _variants

from difffacto_amd import synth

pytestmark = pytest.mark.gpu
T = 4
B = 15
SEED_LO = 0x5DEECE66D & 0xFFFFFFFF
SEEDS = (SEED_LO, (0x9E37 << 32) | SEED_LO)   # the same low word
OFFSET = (1 << 32) + 77

#        name     dfx_debug_pipe_waves code   N    kernel
CASES = [("pipe8",      8, 256, "k_denoise_pipe<8>"),
         ("pipe8_rag",  8, 288, "k_denoise_pipe<8>"),
         ("pipe4",      4, 128, "k_denoise_pipe<4>"),
         ("pipe2",      2, 64,  "k_denoise_pipe<2>"),
         ("coop",       1, 64,  "k_denoise_coop"),
         ("coop2",      16, 64, "k_denoise_coop2")]


def presence_patterns():
    """(15, 4) float32: every non-empty subset of the 4 parts, shape i = pattern i + 1."""
    return np.array([[(m >> j) & 1 for j in range(4)] for m in range(1, 16)], dtype=np.float32)


def make_engine(precision="bf16"):
    from difffacto_amd.engine import DenoiserEngine
    W = {k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(seed=0).items()}
    return DenoiserEngine(W, num_timesteps=T, precision=precision)


def latents():
    pc, mean, logvar, _ = synth.make_latents(B, seed=4100)
    return pc, mean, np.exp(logvar).astype(np.float32)


@contextlib.contextmanager
def general(on):
    from difffacto_amd import _ffi
    _ffi.lib().dfx_debug_chain_general(int(on))
    try:
        yield
    finally:
        _ffi.lib().dfx_debug_chain_general(0)


def chain_kind():
    from difffacto_amd import _ffi
    return _ffi.lib().dfx_debug_last_chain_kind().decode()


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_engine()


@pytest.fixture(scope="module")
def ctx(engine):
    pc, mean, var = latents()
    return engine.prepare_shapes(*map(torch.from_numpy, (pc, mean, var, presence_patterns())))


def launch(engine, ctx, case, force_general, **kw):
    """-> (pred, traj) as numpy, after asserting the kernel and the instantiation the launch took."""
    from difffacto_amd.engine import last_kernel_variant
    name, code, N, kernel = case
    seg = torch.from_numpy(synth.make_seg_mask(presence_patterns(), N))
    want = "general" if force_general or kw.get("ret_interval") else "plain"
    with _variants.forced(code), general(force_general):
        pred, traj = engine.sample_chain(ctx, seg, **kw)
    assert last_kernel_variant() == kernel, f"{name}: expected {kernel}, the launch took {last_kernel_variant()}"
    assert chain_kind() == want, f"{name}: expected the {want} instantiation, the launch took {chain_kind()!r}"
    return pred.cpu().numpy(), None if traj is None else traj.cpu().numpy()


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (what, a.dtype, a.shape, b.dtype, b.shape)
    assert np.isfinite(a).all(), what
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {a.size} values differ, max-abs {np.abs(a - b).max():.3e}, "
                            f"presence patterns {sorted(set((np.nonzero(diff)[-3] + 1).tolist()))}")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plain_equals_general(engine, ctx, case):
    preds = []
    for kw in ({"seed": SEEDS[0]}, {"seed": SEEDS[1]}, {"seed": SEEDS[0], "shape_offset": OFFSET}):
        plain, _ = launch(engine, ctx, case, False, **kw)
        gen, _ = launch(engine, ctx, case, True, **kw)
        assert plain.shape == (B, case[2], 3)
        assert_same_bits(plain, gen, f"{case[0]} {kw}")
        preds.append(plain)
    # the three launches drew different noise: the seed's high word and the shape offset reach the Philox key / counter of PLAIN too
    assert not np.array_equal(preds[0], preds[1]) and not np.array_equal(preds[0], preds[2])


def test_snapshots_are_not_plain(engine, ctx):
    """ret_interval = 2: snapshots at t = 4, 2.  The launch takes GENERAL under either switch state (asserted in launch()); its pred is the
    plain launch's, and the forced-GENERAL launch gives the same pred and the same snapshots."""
    case = CASES[0]
    plain, none = launch(engine, ctx, case, False, seed=SEEDS[1])
    assert none is None
    pred0, traj0 = launch(engine, ctx, case, False, seed=SEEDS[1], ret_interval=2)
    pred1, traj1 = launch(engine, ctx, case, True, seed=SEEDS[1], ret_interval=2)
    assert traj0.shape == (2, B, case[2], 3)
    assert_same_bits(pred0, plain, "pred with snapshots vs plain")
    assert_same_bits(pred1, pred0, "pred with snapshots, switch on vs off")
    assert_same_bits(traj1, traj0, "snapshots, switch on vs off")


def test_explicit_noise_is_not_plain(engine, ctx):
    """A launch that brings its own x_T or step noise keeps the GENERAL instantiation."""
    name, code, N, kernel = CASES[3]
    seg = torch.from_numpy(synth.make_seg_mask(presence_patterns(), N))
    g = torch.Generator().manual_seed(5)
    xT, sn = torch.randn(B, 3, N, generator=g), torch.randn(T, B, 3, N, generator=g)
    for kw in ({"x_T_noise": xT, "seed": 3}, {"step_noise": sn, "seed": 3}, {"x_T_noise": xT, "step_noise": sn}):
        with _variants.forced(code):
            engine.sample_chain(ctx, seg, **kw)
        assert chain_kind() == "general", (kw.keys(), chain_kind())


# ---- the key mask in sbias -------------------------------------------------------------------------------------------------------------
def sbias_of(engine, ctx_buf):
    """(B, depth, 256) float32: the 1 KiB sbias piece of every attention record (csrc/denoiser_internal.h: shape_ctx_view, asms_bytes)."""
    bf16 = engine.precision == "bf16"
    tile = (2 if bf16 else 4) * 64 * 16
    rec = 8 * tile + 1024
    a256 = lambda x: (x + 255) & ~255
    off = a256(4 * 32 * B) + a256(4 * 4 * 128 * B)
    raw = ctx_buf.cpu().numpy()[off:off + rec * B * engine.depth].reshape(B, engine.depth, rec)
    return np.ascontiguousarray(raw[:, :, 8 * tile:]).view(np.float32)


def key_of_entry():
    """sbias entry i = 16 hf + r sits in the accumulator register r of half-wave hf: row rho(r, hf) = 4 head + key of A_s."""
    i = np.arange(32)
    hf, r = i >> 4, i & 15
    return ((r & 3) + 8 * (r >> 2) + 4 * hf) & 3


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_sbias_carries_the_key_mask(precision):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = make_engine(precision)
    pc, mean, var = latents()
    va = presence_patterns()
    got = sbias_of(e, e.prepare_shapes(*map(torch.from_numpy, (pc, mean, var, va))).buf)
    full = sbias_of(e, e.prepare_shapes(*map(torch.from_numpy, (pc, mean, var, np.ones_like(va)))).buf)
    assert got.shape == full.shape == (B, e.depth, 256)
    assert np.isfinite(full).all() and not (full[:, :, 32:] != 0).any() and np.abs(full[:, :, :32]).max() < 1e30
    absent = va[:, key_of_entry()] == 0                      # (B, 32)
    absent = np.broadcast_to(absent[:, None, :], (B, e.depth, 32))
    want = full.copy()
    if precision == "bf16":
        assert absent.any() and not absent.all()
        want[:, :, :32][absent] = -np.finfo(np.float32).max
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.nonzero(got.view(np.uint32) != want.view(np.uint32))
