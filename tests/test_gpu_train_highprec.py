"""The training step's kernels against a float64 oracle and a rounding model (oracle/train.py), judged by rms, max and per-group
statistics (tests/_gradstats.py) against yardsticks computed in the same process — instead of a max-abs over the tensor against 3x a
number a kernel once printed (tests/test_gpu_train.py, whose tests stay as they are).

Per (case, dropout setting) the float64 truth, the fp32 torch-CPU oracle (yardstick of the fp32 kernels) and the bf16 rounding model
(yardstick of the bf16 paths; for the fused path with the attention's two products rounded where its folded form rounds them,
oracle/train.py: attn_fold) are computed once and shared by the three paths: fp32 (layer-by-layer kernels), layer-by-layer bf16
(dfx_debug_train_fused(0)) and fused bf16; the path taken is asserted from dfx_debug_last_train_path.  Dropout (0.2, seed) is replayed
into the oracles with the factors the kernels draw (test_gpu_train.replayed_drops).  x_t and variances_pt require a gradient in every
call, so d_x and d_variances (k_stem_dx) are judged elementwise everywhere, the padded case included.

  B, N      rows   what it reaches
  8, 32      256   smallest fused shape: one 32-point tile per shape (one live wavefront of four in every k_ff workgroup), 8 tiles across
                   8 slabs, param_split 1; valid = None and no flags
  3, 160     480   five tiles per shape: a full and a quarter-full workgroup; 15 slabs
  5, 480    2400   75 tiles over 64 slabs: per = 2, so slabs 38..63 get an empty range (train_ff_fused.h: t0 > ntiles) and contribute zeros
  3, 100     300   padded on the host to 128: d_x / d_variances of the real points, nothing from the padding
  3, 2048   6144   the only large case: 576 values per lane group (3 x 3 x 2048 / 32 >= 512), needed for the point-indexed group ratios;
                   matrix group ratios are judged here and at 5 x 480

One `TRAINHP ...` line per case, path and tensor family (the family's worst ratios, and the new absolute bound beside the old 1.7e-2 /
5e-4 of max-abs), one `TRAINHP-TENSOR` line per tensor for the large case, one `TRAINHP-POOL` line per pool of small tensors and path
(tests/_gradstats.py: pooling); profiles/train_highprec_parity.txt holds them.

Thresholds (tests/_gradstats.py: R32T, RBT, RMAXT, GT): the largest ratio measured on the MI355X over the cases of this file x 1.25, none cut.
                 measured worst   x 1.25   threshold    where (profiles/train_highprec_parity.txt)
  R32T               2.457         3.071    3.08         max-abs, d to_q.weight B3_N2048 p0.2 (its rms: 1.854, the worst rms too)
  RBT                1.184         1.480    1.48         eps B8_N32 p0.2, layer-by-layer (fused worst: 1.176, d time_embed.net.2.weight B3_N2048 p0.2)
  RMAXT              1.754         2.192    2.20         d ff2.weight B3_N100 p0, layer-by-layer (fused worst: 1.488, d to_q.weight B3_N160 p0.2)
  GT[chunk]          1.209         1.511    1.52         d ff2.weight B3_N2048 p0.2, fused
  GT[half]           1.046         1.308    1.31         d ff0.bias B3_N2048 p0.2, fused
  GT[colblock]       1.024         1.280    1.28         d ff0.weight B5_N480 p0, fused
  GT[head]           1.414         1.767    1.77         d to_q.weight B3_N2048 p0, fused
  GT[lane]           1.126         1.407    1.41         d_variances B3_N2048 p0.2, layer-by-layer
  GT[wave]           1.041         1.301    1.31         d_x B5_N480 p0.2, layer-by-layer
  GT[group]          1.100         1.375    1.38         d_variances B3_N2048 p0.2, layer-by-layer
  GT[shape]          1.123         1.404    1.41         eps B5_N480 p0, fused
  GT[coord]          1.112         1.390    1.39         eps B5_N480 p0, fused
  pools of small tensors (same thresholds): worst rms 1.340 / max 1.896 on the fp32 path (norm2.weight / to_out.bias), 1.070 / 1.209 on the bf16
  paths (ff2.bias fused / norm3.bias layer-by-layer), ff0.bias by chunk 1.027 / 1.014.
  Wall time of tests/test_gpu_train_highprec.py: 7 s, CPU oracles included (36 tests).
  No threshold had to be cut: under these values the CPU self-test rejects all six wrong variants (the narrowest, one halved row of one
  dW1: rms 1.56 x, max 7.3 x, chunk share 3.0 x) and also sees the seventh, reported-only one (gradient between blocks rounded to bf16: 2.3 - 2.5 x rms on
  d_variances).  Group ratios are judged on the bf16 paths only; on the fp32 path they are printed.

What had to be restated in the rounding model, instead of widening anything (oracle/train.py, oracle/torch_cpu.py):
  * Against the reference-layout model the layer-by-layer bf16 path measured 1.00 - 1.18 x on every tensor: its errors correlate 0.996 - 0.999
    with the model's, element by element.  The FUSED path measured up to 1.79 x rms / 3.7 x head share (d to_q.weight), 2.1 x rms / 3.8 x max
    (ff2.bias pool) and 0.46 x (time embedding) against it — x 1.25 that is RBT 2.6, RMAXT 4.8, under which a halved dW1 row passes on rms.
  * attn_fold: the attention's two products rounded as the fused kernels evaluate them (A_s xn2, M_s P per shape).  Explains the head shares and
    the context side (the fold moves error between heads and off the to_k / to_v / time-embedding gradients).
  * ff_fold: W1 diag(gamma3) and the plain normalised row as the rounded operands of FF net.0, the bias b1 + W1 beta3 exact, and with dropout the
    scale 1 / (1 - p) on the `a` half of the folded weight (the factors then only select).  Without it the fused kernels' errors were ANTI-correlated
    (-0.45 .. -0.7) with the model's W1-rounding component and 1.5 - 2.7 x the model on every gradient that sums over the points; with gamma3 = 1
    in the weights the same kernels matched the model at once (0.9 - 1.0 x, correlation 0.8 - 0.96) — the rounded operand is another matrix, so
    it is another draw of a coherent error, not a larger or smaller one on average.  With both folds stated: fused <= 1.18 x rms, correlation 0.97.
  * Tried and found NOT to matter (each < 5 % of the yardstick): the fused kernels' sigmoid-form GELU, the forward's fp16 polynomial GEGLU with its
    fp16 GEMM2, the DROP = true kernel variants with a probability that drops nothing (same bits of error as p = 0).
  No defect was found in the kernels.
"""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _gradstats as gs  # noqa: E402
from oracle import train as otrain  # noqa: E402

pytestmark = pytest.mark.gpu

#         name         B  N     seed mixed  flags  matrix / point group ratios judged
CASES = {"B8_N32": (8, 32, 31, False, False, False),
         "B3_N160": (3, 160, 32, True, True, False),
         "B5_N480": (5, 480, 33, True, True, True),
         "B3_N100": (3, 100, 34, True, True, False),
         "B3_N2048": (3, 2048, 35, True, True, True)}
DROPS = {"p0": None, "p0.2": (0.2, 20261019)}
PATHS = {"f32": ("f32", 1, "layer_f32"), "layer": ("bf16", 0, "layer_bf16"), "fused": ("bf16", 1, "fused_bf16")}   # precision, dfx_debug_train_fused, record
_POOLS = {p: gs.Pool() for p in PATHS}


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    """Not a gate: the wall time of this module (CPU oracles included) goes next to the measurements."""
    t0 = time.time()
    yield
    print(f"\nTRAINHP wall time of tests/test_gpu_train_highprec.py: {time.time() - t0:.0f} s", flush=True)


@functools.lru_cache(maxsize=None)
def _case(name):
    B, N, seed, mixed, flags, _ = CASES[name]
    return gs.make_train_case(B, N, seed, mixed=mixed, with_flags=flags)


def _drops(name, drop):
    """The kernels' factors for the oracles.  The kernels number a site's elements over the rows they run: N padded to a multiple of 32."""
    if drop is None:
        return None
    from test_gpu_train import replayed_drops
    B, N = CASES[name][:2]
    Np = (N + 31) // 32 * 32
    d = replayed_drops(drop[1], drop[0], B, Np)
    return {k: (v if k == "te" else np.ascontiguousarray(v[:, :N])) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _oracles(name, dkey):
    """float64 truth and the yardstick of every path — the fp32 oracle, the rounding model, the rounding model with the fused path's
    folded attention (oracle/train.py: attn_fold) — once per (case, p), shared by the three paths and left unchanged."""
    c, drops = _case(name), _drops(name, DROPS[dkey])
    truth = gs.flatten(otrain.loss_and_grads(**c, drops=drops, dtype=torch.float64))
    y32 = gs.flatten(otrain.loss_and_grads(**c, drops=drops))
    ybf = gs.flatten(otrain.loss_and_grads(**c, drops=drops, dtype=torch.float64, operand_round=otrain.round_bf16))
    yfold = gs.flatten(otrain.loss_and_grads(**c, drops=drops, dtype=torch.float64, operand_round=otrain.round_bf16, attn_fold=True, ff_fold=True))
    if drops is not None:    # the replayed factors did something in the oracle
        plain = otrain.loss_and_grads(**c, dtype=torch.float64)
        assert np.abs(plain["eps"] - truth["eps"]).max() > 1e-2
    return truth, {"f32": y32, "layer": ybf, "fused": yfold}


def _run_kernel(c, path, drop, want_x=True, want_var=True):
    """One forward + loss + backward on `path`; the path the library recorded is asserted.  -> dict in the layout of gs.flatten."""
    from difffacto_amd import _ffi, training
    prec, fused, record = PATHS[path]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = {k: cu(v).requires_grad_(True) for k, v in c["W"].items()}
    cc, cm = cu(c["ctx_code"]).requires_grad_(True), cu(c["ctx_mv"]).requires_grad_(True)
    x, var = cu(c["x_t"]).requires_grad_(want_x), cu(c["variances_pt"]).requires_grad_(want_var)
    _ffi.lib().dfx_debug_train_fused(fused)
    try:
        eps = training.denoiser_train_forward(P, x, cu(c["t"]), cc, cm, cu(c["anchors_pt"]), var, None if c["valid"] is None else cu(c["valid"]),
                                              cu(c["assignment"]), precision=prec, dropout=drop)
        took = _ffi.lib().dfx_debug_last_train_path().decode()
        loss = training.masked_mse(cu(c["noise"]), eps, None if c["flags"] is None else cu(c["flags"]))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _ffi.lib().dfx_debug_train_fused(1)
    assert took == record + ("_dropout" if drop else ""), f"path {path}: the library took {took}"
    out = {"eps": eps.detach().cpu().numpy(), "d_ctx_code": cc.grad.cpu().numpy(), "d_ctx_mv": cm.grad.cpu().numpy()}
    out.update({k: v.grad.cpu().numpy() for k, v in P.items()})
    out["d_x"] = x.grad.cpu().numpy() if want_x else None
    out["d_variances"] = var.grad.cpu().numpy() if want_var else None
    return out


@functools.lru_cache(maxsize=None)
def _result(name, dkey, path):
    """Failures of one (case, p, path), its lines printed and its small tensors added to the path's pool — once."""
    truth, yards = _oracles(name, dkey)
    got = _run_kernel(_case(name), path, DROPS[dkey])
    prec = PATHS[path][0]
    for k in ("d_x", "d_variances"):
        assert got[k].shape == truth[k].shape, (k, got[k].shape)     # the real points only: nothing from the padding
    fails, rows = gs.judge_outputs(prec, got, truth, yards[path], CASES[name][5], _POOLS[path])
    label = f"{name} {dkey}"
    for f, d in gs.worst_by_family(rows).items():
        print(gs.family_line(label, path, prec, f, d), flush=True)
    if name == "B3_N2048":
        for row in rows:
            print(gs.tensor_line(label, path, prec, row), flush=True)
    return tuple(f"{label} [{path}]: {f}" for f in fails)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dkey", list(DROPS))
@pytest.mark.parametrize("name", list(CASES))
def test_training_step_against_float64_and_its_yardstick(name, dkey, path):
    """eps, the 77 parameter gradients, d_ctx_code, d_x and d_variances, each tensor of >= 512 elements on its own: rms and max-abs of the
    error against float64 within R32T x the fp32 oracle's (fp32 path) or RBT / RMAXT x the rounding model's (bf16 paths), and on the two
    largest cases the group ratios of tests/_gradstats.py within GT.  All failures of the case are collected before asserting."""
    fails = _result(name, dkey, path)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("path", list(PATHS))
def test_small_tensors_pooled_over_blocks_and_cases(path):
    """The 128-vectors, proj_out, d_ctx_mv (and ff0.bias by chunk): errors divided by the yardstick's rms of the tensor, pooled over
    the five blocks and the ten (case, p) runs of this path (tests/_gradstats.py), then judged like one tensor."""
    for name in CASES:
        for dkey in DROPS:
            _result(name, dkey, path)
    fails, rows = _POOLS[path].judge(PATHS[path][0])
    for row in rows:
        print(gs.pool_line(path, row), flush=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("path", list(PATHS))
def test_requesting_one_or_neither_input_gradient_changes_nothing_else(path):
    """d_x and d_variances are optional outputs of dfx_denoiser_train_backward (k_stem_dx behind everything else): asking for only one,
    or for neither, leaves eps, every parameter gradient, d_ctx_* and the requested one bit-identical to the call that asks for both.
    The padded case with dropout."""
    c, drop = _case("B3_N100"), DROPS["p0.2"]
    both = _run_kernel(c, path, drop)
    for want_x, want_var in ((True, False), (False, True), (False, False)):
        r = _run_kernel(c, path, drop, want_x, want_var)
        assert (r["d_x"] is None) == (not want_x) and (r["d_variances"] is None) == (not want_var)
        for k, v in both.items():
            if r[k] is not None:
                assert np.array_equal(r[k], v), (path, want_x, want_var, k)
