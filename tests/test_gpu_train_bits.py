"""Every output bit of a denoiser training iteration (forward + masked_mse + backward) against a fixture written by the PARENT of the commit that
added this file (tests/golden/train_bits/parent.json, written by tools/make_train_bits_golden.py with that commit's library loaded, never by
the code under test).  That commit removed the split-attention training path and folded the run-time flags it needed out of the fused backward
kernel (k_ff_bwd) and k_head_bwd: the kernels that remain must compute what they computed, to the bit.

The fixture holds the SHA-256 of the raw bytes of loss, eps, every parameter gradient, d_ctx_code, d_ctx_mv, d_x and d_variances, per case of
tests/_train_bits_case.py: the fused path at its smallest shape, with a ragged last workgroup, with empty weight-gradient slabs and at an even
depth, each without and with dropout, and one case of each layer-by-layer path.  Each case runs twice and must also equal itself."""
import json

import pytest
import torch

import _train_bits_case as tb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(tb.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", tb.CASES, ids=[c[0] for c in tb.CASES])
def test_bits_equal_parent(golden, case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    got, again, want = tb.run_case(case), tb.run_case(case), golden[case[0]]
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    unstable = sorted(k for k in got if got[k] != again[k])
    assert not unstable, f"{case[0]}: two runs of the same iteration differ in {unstable}"
    moved = sorted(k for k in got if got[k] != want[k])
    assert not moved, f"{case[0]}: {len(moved)} of {len(got)} outputs differ from the parent's bits: {moved}"


def test_fixture_is_complete(golden):
    """Nothing in the fixture that no case reads; every case has the six non-parameter outputs and one digest per parameter."""
    from difffacto_amd import training
    assert set(golden) == {c[0] for c in tb.CASES}
    for c in tb.CASES:
        assert set(golden[c[0]]) == {"loss", "eps", "d_ctx_code", "d_ctx_mv", "d_x", "d_variances"} | {"g/" + n for n in training.param_names(c[1])}, c[0]
