"""PointNetV2's training step and the flows' prior loss on the HIP path (fp32) against a float64 oracle ON THE BRANCH THE KERNELS TOOK, judged
by rms and max-abs against the fp32 torch-CPU oracle's own error computed in the same process (tests/_encstats.py, which says why the branch
has to be the kernels' own and how it is checked for legitimacy; acceptance: tests/_gradstats.py, R32T = 3.08, unchanged).  The fixed-fraction
gates of tests/test_gpu_encoder_train.py stay as they are.

PointNetV2 (momentum 0.1; shape 0 lacks one part):
  B, N      rows   what it reaches
  2, 33       66   BatchNorm over two rows in the heads; ragged everything
  5, 160     800   the golden's size
  4, 333    1332   ragged row tiles; shape 1 holds a single part
  8, 1024   8192   exactly 8192 rows: first use of the epilogue statistics        } both settings of dfx_debug_bn_fused_stats, each held to
  9, 1000   9000   ragged last row tile                                             } the same gate, and differing in at least one bit
  5, 2048  10240   more workgroups than row tiles                                   }
  3, 70      210   momentum < 0: the running statistics stay the inputs bit for bit
Prior loss: B = 1, 6 (the kernels' branch must EQUAL the float64 branch: margins 375 x and 12.8 x the site error, _encstats.FLOW_SEED), 32,
37 (the former "known kink case", now strict), 64 / 65 (the 64-row slab count of carve_flow), 70; ragged validity, one shape with one part.

Measured on the MI355X (profiles/encoder_highprec_parity.txt): no unit of any case is off the float64 branch without being ambiguous (at most one
per site differs at all); the flows measure <= 1.72 x rms and <= 3.00 x max-abs on every tensor (pools <= 1.11 x), B = 37 and the kink-free
B = 1 / B = 6 included; PointNetV2 against the yardstick as tests/_encstats.py restates it ("What was found": the heads' products as a chain over
K, the heads' BatchNorm and bn4 written out in fp32, eight draws of the summation order) measures <= 1.58 x rms / 2.14 x max-abs in nine of its
ten runs, both statistics paths of the three >= 8192-row cases among them, and 2.56 x / 2.95 x at 2 x 33.
2 x 33 is the narrow one, and why is known: its heads hold BatchNorm channels with a batch variance of 0.0 .. 0.4 eps (two rows), one of which
(channel 203 of mlp_m.1, amplification ~300) met a 2.7-sigma draw of an input error that is of the yardstick's own size everywhere else
(tests/_encstats.py).  The yardstick's draws are torch-CPU products and follow the host's torch build: judged on another host, the same kernel
outputs measured 3.26 x on the max-abs of mlp_m.4.running_mean.  Nothing was widened for it.
Wall time of the module: 18 - 20 s, CPU oracles included (21 tests; the slowest are the three >= 8192-row cases at 5.9, 3.6 and 3.5 s: eight
fp32 draws of the yardstick and the float64 passes on every distinct branch; every other test about 1 s or less).

One `ENCHP ...` line per case and tensor family (worst ratios, and per site the units off the float64 branch: kernels' / fp32 oracle's),
one `ENCHP-POOL` line per pool of small tensors; profiles/encoder_highprec_parity.txt holds them with the module's wall time.
"""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _encstats as es  # noqa: E402
import _gradstats as gs  # noqa: E402

pytestmark = pytest.mark.gpu
_POOL = gs.Pool()
BIG = [c for c in es.PN_CASES if c[0] * c[1] >= 8192]
PN_RUNS = [(B, N, 1) for B, N in es.PN_CASES] + [(B, N, 0) for B, N in BIG]      # (B, N, dfx_debug_bn_fused_stats)


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    """Not a gate: the wall time of this module (CPU oracles included) goes next to the measurements."""
    t0 = time.time()
    yield
    print(f"\nENCHP wall time of tests/test_gpu_encoder_train_highprec.py: {time.time() - t0:.0f} s", flush=True)


@functools.lru_cache(maxsize=None)
def _pn(B, N, momentum=0.1):
    case = es.pn_case(B, N)
    return case, es.pn_oracles(case, momentum=momentum)


@functools.lru_cache(maxsize=None)
def _flow(B):
    case = es.flow_case(B)
    return case, es.flow_oracles(case)


@functools.lru_cache(maxsize=None)
def _pn_kernel(B, N, fused, momentum=0.1):
    """One forward, the branch export, the backward -> (result in the oracle's layout, branch in the oracle's layout)."""
    from difffacto_amd import _ffi, training
    case = _pn(B, N, momentum)[0]
    W = case["W"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = {n: cu(W[n]).requires_grad_(True) for n in training.PNV2_PARAMS}
    Bf = {n: cu(W[n]) for n in training.PNV2_BUFFERS}
    _ffi.lib().dfx_debug_bn_fused_stats(fused)
    try:
        m, v = training.pointnet_v2_train_forward(P, Bf, cu(case["x"]), cu(case["attn"]), momentum=momentum)
        exp = {k: t.cpu().numpy() for k, t in training.pointnet_v2_branch(m).items()}
        ((m * cu(case["dm"])).sum() + (v * cu(case["dv"])).sum()).backward()
        torch.cuda.synchronize()
    finally:
        _ffi.lib().dfx_debug_bn_fused_stats(1)
    got = dict(m=m.detach().cpu().numpy(), v=v.detach().cpu().numpy(), running={n: b.cpu().numpy() for n, b in Bf.items()},
               grads={n: p.grad.cpu().numpy() for n, p in P.items()})
    return got, es.pn_branch_of_export(exp, case["attn"])


@functools.lru_cache(maxsize=None)
def _pn_result(B, N, fused):
    case, orc = _pn(B, N)
    got, branch = _pn_kernel(B, N, fused)
    label = f"B{B}_N{N}" + ("" if (B, N) not in BIG else " epilogue-stats" if fused else " two-pass-stats")
    fails, lines = es.judge(label, orc, got, branch, es.pn_flatten, _POOL)
    print("\n".join(lines), flush=True)
    return tuple(fails)


@functools.lru_cache(maxsize=None)
def _flow_result(B):
    from difffacto_amd import training
    case, orc = _flow(B)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = {n: cu(case["W"][n]).requires_grad_(True) for n in training.flow_param_names(14)}
    z, lv = cu(case["part_code"]).requires_grad_(True), cu(case["logvar"]).requires_grad_(True)
    loss, log_p, ent = training.prior_loss(P, z, lv, cu(case["valid"]), prior_var=case["prior_var"], kl_weight=case["kl_weight"])
    branch = {k: t.cpu().numpy() for k, t in training.prior_loss_branch(loss).items()}
    loss.backward()
    torch.cuda.synchronize()
    got = dict(loss=float(loss.detach()), log_p=log_p.cpu().numpy(), entropy=ent.cpu().numpy(), d_part_code=z.grad.cpu().numpy(),
               d_logvar=lv.grad.cpu().numpy(), grads={n: p.grad.cpu().numpy() for n, p in P.items()})
    fails, lines = es.judge(f"flows_B{B}", orc, got, branch, functools.partial(es.flow_flatten, case=case), _POOL)
    fails += [f"flows_B{B}: {f}" for f in es.absent_rows_exactly_zero(got, case)]
    if B in es.FLOW_SEED:
        off = {s: int(es.differing(orc, branch, s).sum()) for s in es.FLOW_SITES}
        if any(off.values()):
            fails.append(f"flows_B{B}: the kernels' branch is not the float64 branch on a batch without ambiguous units: {off}")
    print("\n".join(lines), flush=True)
    return tuple(fails)


@pytest.mark.parametrize("B,N,fused", PN_RUNS)
def test_pointnet_v2_training_step_against_float64_on_the_kernels_branch(B, N, fused):
    """m, v, the twelve running statistics and the 36 parameter gradients (the eleven mathematically zero ones as a family of their own): every
    tensor of >= 512 elements within R32T x the fp32 oracle's rms and max-abs error; every unit off the float64 branch ambiguous."""
    fails = _pn_result(B, N, fused)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,N", BIG)
def test_the_two_statistics_paths_are_two_summation_orders(B, N):
    """From 8192 rows on the epilogue statistics are in use: the two settings give different bits (each is held to the gate above)."""
    a, b = _pn_kernel(B, N, 1)[0], _pn_kernel(B, N, 0)[0]
    assert any(not np.array_equal(a["running"][k], b["running"][k]) for k in a["running"]) or not np.array_equal(a["m"], b["m"])


def test_negative_momentum_leaves_the_running_statistics_untouched():
    """momentum < 0: outputs and gradients through the same gate; the twelve running statistics equal the inputs bit for bit."""
    B, N = es.PN_FROZEN_CASE
    case, orc = _pn(B, N, -1.0)
    got, branch = _pn_kernel(B, N, 1, -1.0)
    for k, a in got["running"].items():
        assert np.array_equal(a, case["W"][k]), k
    fails, lines = es.judge(f"B{B}_N{N} momentum<0", orc, got, branch, functools.partial(es.pn_flatten, running=False), _POOL)
    print("\n".join(lines), flush=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", es.FLOW_CASES)
def test_prior_loss_against_float64_on_the_kernels_branch(B):
    """Loss, log_p, entropy (pooled over the cases), d_part_code, d_logvar (rows of absent parts exactly 0) and the 168 weight gradients on their
    own, the 168 bias gradients pooled by layer kind; every ReLU unit off the float64 branch ambiguous, none at all at B = 1 and B = 6."""
    fails = _flow_result(B)
    assert not fails, "\n".join(fails)


def test_small_tensors_pooled_over_layers_and_cases():
    """conv1.weight, the trunk's BatchNorm parameters and running statistics, the small zero gradients, the flows' biases, log_p with the loss,
    entropy: errors divided by the yardstick's rms of the tensor, pooled over every run of this file, then judged like one tensor."""
    for run in PN_RUNS:
        _pn_result(*run)
    for B in es.FLOW_CASES:
        _flow_result(B)
    fails, lines = es.judge_pool(_POOL)
    print("\n".join(lines), flush=True)
    assert not fails, "\n".join(fails)
