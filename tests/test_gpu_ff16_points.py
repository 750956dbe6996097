"""The bf16 chain kernels run their feed-forward on two 16-point N-tiles per wavefront (csrc/denoiser_ff16.h): 16-lane row swaps take the
LayerNorm output and the residual stream from one point per lane to that form and back.  What the host test (test_ff16_layout_cpu.py) cannot
see is the hardware: that the swap instruction moves the rows it is read to move, and that no kernel crosses the two N-tiles.  Here, on the
smallest clouds that have a full and a ragged last tile (N = 64, 96; B = 2, T = 2, explicit noise), through every chain kernel:
  (i)   permuting the points inside each 32-point tile, with their part ids, x_T and step noise, permutes the cloud bit for bit;
  (ii)  scaling one point's x_T draw by a large factor leaves every other point's bits alone;
  (iii) eps at one t is within the existing bf16-vs-fp32 bound (test_gpu_denoiser.TOL_BF16_EPS) of the exact-fp32 engine.
And with three and with one valid part (B = 3, N = 32) the bf16 chain stays within that bound of the fp32 chain.

A forced variant that the planner does not grant falls back as include/dfx_debug.h documents — k_denoise_pipe<8> would pad 64 points more than
3x (direct kernel), k_denoise_coop2 needs N % 64 == 0 (k_denoise_coop) — and the test asserts that name instead: the direct kernel runs the same
feed-forward helpers."""
import numpy as np
import pytest
import torch

import _variants
from test_gpu_denoiser import TOL_BF16_EPS

from difffacto_amd import synth

pytestmark = pytest.mark.gpu
T, B = 2, 2


def _expected(nw, N):
    if nw == 8 and N == 64:
        return "k_denoise<bf16>"
    if nw == 16 and N % 64:
        return "k_denoise_coop"
    return _variants.NAMES["bf16"][nw]


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from difffacto_amd.engine import DenoiserEngine
    W = {k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(seed=0).items()}
    return {p: DenoiserEngine(W, num_timesteps=T, precision=p) for p in ("bf16", "f32")}


@pytest.fixture(scope="module")
def case(engines):
    """Per N: inputs, their in-tile permutation, and the fp32 eps — computed once, never written to."""
    cache = {}

    def get(N):
        if N not in cache:
            pc, mean, logvar, va = synth.make_latents(B, seed=N)
            lat = tuple(map(torch.from_numpy, (pc, mean, np.exp(logvar).astype(np.float32), va)))
            sg = torch.from_numpy(synth.make_seg_mask(va, N))
            g = torch.Generator().manual_seed(N)
            xT, sn = torch.randn(B, 3, N, generator=g), torch.randn(T, B, 3, N, generator=g)
            perm = torch.cat([32 * k + torch.randperm(32, generator=g) for k in range(N // 32)])
            assert not torch.equal(perm[:16].sort().values, torch.arange(16))   # points do move between the two 16-point halves of a tile
            ef = engines["f32"]
            eps32 = ef.eps(ef.prepare_shapes(*lat), xT, sg, 1).cpu()
            cache[N] = dict(lat=lat, sg=sg, xT=xT, sn=sn, perm=perm, eps32=eps32)
        return cache[N]
    return get


def _run(e, nw, N, fn):
    from difffacto_amd.engine import last_kernel_variant
    with _variants.forced(nw):
        out = fn()
    assert last_kernel_variant() == _expected(nw, N), (last_kernel_variant(), _expected(nw, N))
    return out


@pytest.mark.parametrize("N", [64, 96])
@pytest.mark.parametrize("nw", [8, 2, 1, 16])
def test_points_stay_apart_and_in_place(engines, case, nw, N):
    e, c = engines["bf16"], case(N)
    cx = e.prepare_shapes(*c["lat"])
    sg, xT, sn, perm = c["sg"], c["xT"], c["sn"], c["perm"]
    base = _run(e, nw, N, lambda: e.sample_chain(cx, sg, x_T_noise=xT, step_noise=sn)[0]).cpu()
    assert torch.isfinite(base).all()
    # (i) the same points in another order inside every 32-point tile
    moved = _run(e, nw, N, lambda: e.sample_chain(cx, sg[:, perm].contiguous(), x_T_noise=xT[:, :, perm].contiguous(),
                                                  step_noise=sn[:, :, :, perm].contiguous())[0]).cpu()
    assert torch.equal(moved, base[:, perm, :])
    # (ii) one point far away: nobody else notices
    for p in (5, N - 9):   # one in the first tile's first half, one in the second half of the last (ragged for N = 96) tile
        x2 = xT.clone()
        x2[1, :, p] *= 64.0
        out = _run(e, nw, N, lambda: e.sample_chain(cx, sg, x_T_noise=x2, step_noise=sn)[0]).cpu()
        same = (out == base).all(dim=2)
        assert not same[1, p] and same.sum().item() == B * N - 1, (p, (~same).nonzero().tolist())
    # (iii) one evaluation against exact fp32
    eps = _run(e, nw, N, lambda: e.eps(cx, xT, sg, 1)).cpu()
    err = (eps - c["eps32"]).abs().max().item()
    print(f"N={N} {_expected(nw, N)}: eps bf16 vs fp32 max-abs {err:.3e}")
    assert err < TOL_BF16_EPS


@pytest.mark.parametrize("nvalid", [3, 1])
@pytest.mark.parametrize("nw", [0, 2])
def test_part_presence_masks(engines, nw, nvalid):
    Bm, N = 3, 32
    pc, mean, logvar, _ = synth.make_latents(Bm, seed=20 + nvalid)
    va = np.zeros((Bm, 4), np.float32)
    va[:, :nvalid] = 1.0
    lat = tuple(map(torch.from_numpy, (pc, mean, np.exp(logvar).astype(np.float32), va)))
    sg = torch.from_numpy(synth.make_seg_mask(va, N))
    g = torch.Generator().manual_seed(nvalid)
    xT, sn = torch.randn(Bm, 3, N, generator=g), torch.randn(T, Bm, 3, N, generator=g)
    eb, ef = engines["bf16"], engines["f32"]
    want = ef.sample_chain(ef.prepare_shapes(*lat), sg, x_T_noise=xT, step_noise=sn)[0].cpu()
    with _variants.forced(nw):
        got = eb.sample_chain(eb.prepare_shapes(*lat), sg, x_T_noise=xT, step_noise=sn)[0].cpu()
    name = _variants.ran("bf16", nw)
    err = (got - want).abs().max().item()
    print(f"{nvalid} valid part(s), {name}: chain T={T} bf16 vs fp32 max-abs {err:.3e}")
    assert torch.isfinite(got).all() and err < TOL_BF16_EPS
