"""The four training workspaces keep their sizes: every `*_workspace_bytes` function against tests/golden/train_workspace_bytes.json, written by
tools/make_train_workspace_golden.py with the library of the commit before the denoiser workspace was split into its common / layered / fused
groups (csrc/train_kernels.hip: carve(), carve_pn(), carve_flow(), carve_smt()).  The fused step's buffers are views into layered ones, and a view
whose need exceeded the buffer under it would make dfx_denoiser_train_workspace_bytes return 0: no legal shape may."""
import json

import pytest

import _train_workspace_case as t


@pytest.fixture(scope="module")
def lib():
    return t.load()


def test_sizes_are_the_recorded_ones(lib):
    with open(t.GOLDEN) as f:
        want = json.load(f)
    got = t.sizes(lib)
    assert sorted(got) == sorted(want) and {k: len(v) for k, v in got.items()} == {
        "dfx_denoiser_train_workspace_bytes": 10, "dfx_pointnet_v2_train_workspace_bytes": 4, "dfx_prior_loss_workspace_bytes": 5,
        "dfx_shared_mlp_train_workspace_bytes": 4}
    for fn in want:
        assert sorted(got[fn]) == sorted(want[fn]), fn
        for shape, nbytes in want[fn].items():
            assert nbytes > 0 and got[fn][shape] == nbytes, (fn, shape, got[fn][shape], nbytes)


def test_no_view_outgrows_its_buffer_on_a_legal_shape(lib):
    for depth in (1, 5, 8):
        for B in range(1, 10):
            for N in range(32, 513, 32):
                assert lib.dfx_denoiser_train_workspace_bytes(B, N, depth) > 0, (B, N, depth)


def test_illegal_arguments_still_give_zero(lib):
    assert lib.dfx_denoiser_train_workspace_bytes(0, 64, 5) == 0 and lib.dfx_denoiser_train_workspace_bytes(2, 16, 5) == 0
    assert lib.dfx_denoiser_train_workspace_bytes(2, 64, 0) == 0
    assert lib.dfx_pointnet_v2_train_workspace_bytes(1, 64, 4, 256) == 0 and lib.dfx_pointnet_v2_train_workspace_bytes(2, 64, 3, 256) == 0
    assert lib.dfx_prior_loss_workspace_bytes(0, 14, 256) == 0 and lib.dfx_prior_loss_workspace_bytes(4, 0, 256) == 0
    assert lib.dfx_shared_mlp_train_workspace_bytes(None, 2, 4, 4) == 0
