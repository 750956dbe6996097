"""Partial reverse chains, the parts that need no GPU: the three entry points are declared, bound and exported; the labelling of the
snapshots a partial chain returns (``engine.snapshot_times``) against tables written by hand; the ``hold`` mask conversion; which parts
``editing.vary_shape`` holds."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfx_sample_chain_from", "dfx_refine_chain", "dfx_sample_chain_ddim_from")


def test_symbols_are_declared_bound_and_exported():
    from difffacto_amd import _ffi
    header = open(os.path.join(ROOT, "include", "dfx.h")).read()
    L = _ffi.lib()
    assert L.dfx_version() >= 108 and L.dfx_abi_version() == 5 == _ffi.DFX_ABI_VERSION
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = _ffi.SIGNATURES[name]
        assert len(args) == n_args, (name, len(args), n_args)
        assert getattr(L, name).argtypes == args
    # null handle: an error code with a message, no launch
    rc = L.dfx_sample_chain_from(None, None, None, None, 1, None, 0, 0, None, 0, None, None, 1, 32, None)
    assert rc != 0 and b"null denoiser" in L.dfx_last_error()


def test_snapshot_times_tables():
    from difffacto_amd.engine import snapshot_times
    T = 12
    assert snapshot_times(T, 4) == [12, 8, 4]
    # sample_chain_from: the slots of the executed timesteps n_steps-1 .. 0; the t = T slot (the first state) only for the whole chain
    assert snapshot_times(T, 4, n_steps=12) == [12, 8, 4]
    assert snapshot_times(T, 4, n_steps=11) == [8, 4]
    assert snapshot_times(T, 4, n_steps=9) == [8, 4]
    assert snapshot_times(T, 4, n_steps=8) == [4]          # resumed from the slot labelled 8: that slot is the input, not an output
    assert snapshot_times(T, 4, n_steps=5) == [4]
    assert snapshot_times(T, 4, n_steps=4) == []
    assert snapshot_times(T, 4, n_steps=3) == []           # n_steps < ret_interval
    assert snapshot_times(T, 4, n_steps=1) == []
    # refine_chain: never the t = T slot
    assert snapshot_times(T, 4, n_steps=12, fused=True) == [8, 4]
    assert snapshot_times(T, 4, n_steps=9, fused=True) == [8, 4]
    # ret_interval that does not divide T: no t = T slot at all (slot 0 is t = 10)
    assert snapshot_times(T, 5) == [10, 5]
    assert snapshot_times(T, 5, n_steps=12) == [10, 5]
    assert snapshot_times(T, 5, n_steps=10) == [5]
    assert snapshot_times(T, 1, n_steps=3) == [2, 1]
    assert snapshot_times(10, 5, n_steps=10) == [10, 5] and snapshot_times(10, 5, n_steps=7) == [5] and snapshot_times(10, 5, n_steps=1) == []


def test_hold_mask_conversion():
    from difffacto_amd.engine import DenoiserEngine
    hm = DenoiserEngine.hold_mask
    assert hm(None, 3) is None
    m = hm(torch.tensor([[0, 1, 0, 0], [1, 1, 0, 1], [0, 0, 0, 0]]), 3)
    assert m.dtype == torch.int32 and m.tolist() == [2, 11, 0]
    assert hm(torch.tensor([[0., 1., 0., 0.], [1., 1., 0., 1.]]), 2).tolist() == [2, 11]       # 0/1 floats (a `present`-style mask)
    assert hm(torch.tensor([[True, False, True, False]]), 1).tolist() == [5]
    b = hm(torch.tensor([2, 11, 0], dtype=torch.int64), 3)
    assert b.dtype == torch.int32 and b.tolist() == [2, 11, 0]
    assert hm([4, 8], 2).tolist() == [4, 8]
    for bad in (torch.tensor([1, 2]), torch.tensor([1.0, 2.0, 3.0]), torch.zeros(2, 4), torch.zeros(3, 2, 2)):
        with pytest.raises(RuntimeError, match="hold"):
            hm(bad, 3)


def test_held_parts():
    from difffacto_amd import editing
    valid = torch.tensor([[1., 1., 1., 1.], [1., 0., 1., 1.], [0., 0., 1., 0.]])
    assert editing.held_parts(valid, None, 4).tolist() == [[0.] * 4] * 3
    assert editing.held_parts(valid, [1], 4).tolist() == [[1., 0., 1., 1.], [1., 0., 1., 1.], [0., 0., 1., 0.]]
    assert editing.held_parts(valid, (2, 0), 4).tolist() == [[0., 1., 0., 1.], [0., 0., 0., 1.], [0., 0., 0., 0.]]
    assert valid.tolist()[1] == [1., 0., 1., 1.]           # the caller's mask is not written to
    with pytest.raises(ValueError):
        editing.held_parts(valid, [4], 4)
