"""CPU checks of the editing modes (shape interpolation, part mixing, anchor drift): the dfx_compose_latents entry point is exported and
bound, rejects bad recipes before touching a GPU, the model mirror constructs with the editing switches, the host-side recipe builders
equal a restatement of the reference's index bookkeeping (anchor_gen.py:239-251, :361-370, :489-498), and the golden fixtures of
tests/golden/edit/ match their manifest."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDIT = os.path.join(ROOT, "tests", "golden", "edit")


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_compose_latents_is_exported_and_bound(L):
    from difffacto_amd import _ffi
    assert "dfx_compose_latents" in _ffi.SIGNATURES
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "dfx_compose_latents")
    assert L.dfx_version() >= 101 and L.dfx_abi_version() == 5


class _Stub:
    """A dfx_latents handle without device memory (dfx_debug_latents_stub): n_class 4, zdim 16, cimle with noise_dim 8."""

    def __init__(self, L, cimle=1):
        self.L, self.h = L, ctypes.c_void_p()
        assert L.dfx_debug_latents_stub(ctypes.byref(self.h), 4, 16, cimle, 8) == 0

    def close(self):
        self.L.dfx_latents_destroy(self.h)


FAKE = ctypes.c_void_p(0x1000)   # a non-null "device pointer": never dereferenced, the checks fail (or stop) first


def _call(L, h, R=6, S=3, code_a=None, code_b=None, alpha=None, noise=FAKE, Sn=6, noise_row=None, seg_mode=0, seg_src=None, Ss=0,
          seg_row=None, npoints=64, valid=FAKE, part_code=FAKE, noise_out=FAKE):
    J = 4
    code_a = np.zeros((R, J), np.int32) if code_a is None else np.ascontiguousarray(code_a, np.int32)
    hp = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.c_void_p)
    keep = [code_a, code_b, noise_row, seg_row]
    rc = L.dfx_compose_latents(h, FAKE, S, hp(code_a), hp(code_b), alpha, valid, noise, Sn, hp(noise_row), None, None, seg_mode, seg_src,
                               Ss, hp(seg_row), R, npoints, part_code, noise_out, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None)
    del keep
    return rc, (L.dfx_last_error() or b"").decode()


def test_compose_latents_rejects_bad_recipes_without_a_gpu(L):
    s = _Stub(L)
    try:
        h = s.h
        ok_rc, ok_msg = _call(L, h)
        assert ok_rc == -1 and "holds no weights" in ok_msg            # every check passed; the stub stops it before HIP
        assert _call(L, h, R=0)[0] == 0                                # empty request: a no-op
        bad = [
            (dict(code_a=np.full((6, 4), 3)), "code_a"),               # index == S
            (dict(code_a=np.full((6, 4), -1)), "code_a"),
            (dict(code_b=np.zeros((6, 4)), alpha=None), "together"),
            (dict(code_b=np.full((6, 4), -2), alpha=FAKE), "code_b"),
            (dict(code_b=np.full((6, 4), 3), alpha=FAKE), "code_b"),
            (dict(noise=None), "noise"),                               # cimle without noise
            (dict(noise_out=None), "noise"),
            (dict(Sn=5), "Sn >= R"),                                   # identity rows need Sn >= R
            (dict(noise_row=np.array([0, 1, 2, 3, 4, 5]), Sn=5), "noise_row"),
            (dict(npoints=63), "multiple of n_class"),
            (dict(seg_mode=3), "seg_mode"),
            (dict(seg_mode=-1), "seg_mode"),
            (dict(seg_mode=2), "seg_mode 2"),                          # no seg_src / seg_row
            (dict(seg_mode=2, seg_src=FAKE, Ss=2, seg_row=np.array([0, 0, 1, 1, 2, 2])), "seg_row"),
            (dict(seg_mode=0, seg_src=FAKE, Ss=1, seg_row=np.zeros(6)), "seg_mode 2 only"),
            (dict(valid=None), "null pointer"),
            (dict(part_code=None), "null pointer"),
            (dict(S=0), "code_src"),
        ]
        for kw, needle in bad:
            rc, msg = _call(L, h, **kw)
            assert rc == -1 and needle in msg, (kw, msg)
        assert _call(L, h, code_b=np.full((6, 4), -1), alpha=FAKE, noise_row=np.array([0, 0, 1, 1, 2, 2]), Sn=3)[1].endswith("no weights")
        assert _call(L, h, seg_mode=2, seg_src=FAKE, Ss=3, seg_row=np.array([0, 0, 1, 1, 2, 2]))[1].endswith("no weights")
    finally:
        s.close()
    s = _Stub(L, cimle=0)
    try:
        assert "without cimle" in _call(L, s.h)[1]
        assert _call(L, s.h, noise=None, noise_out=None)[1].endswith("no weights")
    finally:
        s.close()
    assert L.dfx_compose_latents(None, FAKE, 1, None, None, None, FAKE, None, 0, None, None, None, 0, None, 0, None, 1, 64, FAKE, None,
                                 FAKE, FAKE, None, None, None, None, None) == -1


def test_model_mirror_constructs_with_the_editing_switches():
    from difffacto_amd.networks import AnchorDiffAE
    from test_modules_cpu import model_cfg
    for flag in ("interpolate", "combine", "drift_anchors"):
        m = AnchorDiffAE(**model_cfg(**{flag: True}))
        assert getattr(m, flag) is True
    assert AnchorDiffAE(**model_cfg(interpolate_part_id=1)).interpolate_part_id == 1
    for flag in ("zero_anchors", "use_input", "save_weights", "pretrain_prior", "train_language", "forward_sample"):
        with pytest.raises(NotImplementedError):
            AnchorDiffAE(**model_cfg(**{flag: True}))
    cfg = model_cfg(interpolate=True)
    cfg["encoder"] = dict(cfg["encoder"], selective_noise_sampling=True)
    with pytest.raises(NotImplementedError):
        AnchorDiffAE(**cfg)


def _labelled_codes(B, Z, J):
    """code[b, c, j] = 1000 b + 10 j + c / Z: every source (shape, part) distinguishable after any gather."""
    b, c, j = np.meshgrid(np.arange(B), np.arange(Z), np.arange(J), indexing="ij")
    return torch.from_numpy((1000.0 * b + 10.0 * j + c / Z).astype(np.float32))


def _gather(codes, code_a):
    R, J = code_a.shape
    return torch.stack([codes[torch.from_numpy(code_a[:, j].astype(np.int64)), :, j] for j in range(J)], dim=-1)


@pytest.mark.parametrize("B,K,pid", [(2, 10, 2), (5, 10, 0), (3, 4, 3)])
def test_interpolation_recipe_matches_the_reference_bookkeeping(B, K, pid):
    from difffacto_amd import editing
    J, Z = 4, 6
    part_code = _labelled_codes(B, Z, J)
    gen = torch.Generator().manual_seed(B * 7 + K)
    perm = torch.randperm(B, generator=gen)
    dx = torch.linspace(0, 1, steps=K).reshape(1, -1, 1)
    # anchor_gen.py:244-247, literally
    interp = part_code[..., pid].unsqueeze(1) + (part_code[perm, :, pid].unsqueeze(1) - part_code[..., pid].unsqueeze(1)) * dx
    ref = part_code.unsqueeze(1).repeat_interleave(K, dim=1)
    ref[..., pid] = interp
    ref = ref.reshape(B * K, -1, J)
    code_a, code_b = editing.interpolation_recipe(B, K, J, pid, perm.numpy())
    alpha = editing.interpolation_alpha(B, K, J, pid, dx.reshape(-1))
    a, b = _gather(part_code, code_a), _gather(part_code, np.where(code_b < 0, code_a, code_b))
    got = torch.where(torch.from_numpy(code_b < 0)[:, None, :], a, a + (b - a) * alpha[:, None, :])
    assert torch.equal(got, ref)
    assert (code_b[:, [j for j in range(J) if j != pid]] == -1).all()
    rows = editing.repeat_rows(B, K)
    assert np.array_equal(rows, torch.arange(B).repeat_interleave(K).numpy())            # noise / valid / seg rows (:248-254)


@pytest.mark.parametrize("B,K", [(3, 2), (6, 1), (4, 10)])
def test_mixing_recipe_matches_the_reference_bookkeeping(B, K):
    from difffacto_amd import editing
    J, Z = 4, 5
    gen = torch.Generator().manual_seed(B + 31 * K)
    part_code = _labelled_codes(B, Z, J)
    valid = (torch.rand(B, J, generator=gen) > 0.3).float()
    perms = [torch.randperm(B, generator=gen) for _ in range(J)]
    ref_code, ref_valid = part_code.clone(), valid.clone()
    for i in range(J):                                                                     # anchor_gen.py:489-496, literally
        perm = perms[i]
        ref_code[..., i] = ref_code[perm][..., i]
        ref_valid[:, i] = ref_valid[perm][..., i] * ref_valid[:, i]
    ref_code, ref_valid = (t.repeat_interleave(K, dim=0) for t in (ref_code, ref_valid))   # :498
    code_a = editing.mixing_recipe([p.numpy() for p in perms], K)
    assert torch.equal(_gather(part_code, code_a), ref_code)
    got_valid = editing.mixing_valid(valid, perms)
    assert torch.equal(got_valid.repeat_interleave(K, dim=0), ref_valid)
    assert torch.equal(valid, valid.clone()) and got_valid.data_ptr() != valid.data_ptr()  # the caller's mask is not written
    # seg ids of rule 0 (:510-511) and rule 1 (:437-438)
    ids0 = torch.arange(J)[None] * ref_valid + torch.argmax(ref_valid, dim=1)[:, None] * (1 - ref_valid)
    assert torch.equal(editing.seg_ids(ref_valid, 64, 0), ids0.repeat_interleave(16, dim=1).to(torch.int32))
    ids1 = (torch.arange(J)[None] * ref_valid.long()).repeat_interleave(16, dim=1).to(torch.int32)
    assert torch.equal(editing.seg_ids(ref_valid, 64, 1), ids1)


@pytest.mark.parametrize("B,K", [(2, 3), (4, 10)])
def test_drift_factors_match_the_reference_bookkeeping(B, K):
    from difffacto_amd import editing
    J = 4
    gen = torch.Generator().manual_seed(K)
    mean, logvar = torch.randn(B * K, 3, J, generator=gen), torch.randn(B * K, 3, J, generator=gen)
    dx = torch.linspace(1, 5, steps=K).reshape(1, -1).expand(B, -1).reshape(B * K, 1)     # anchor_gen.py:362
    rm, rl = mean.clone(), logvar.clone()
    rm[:, 1, [0, 2]] = rm[:, 1, [0, 2]] * torch.sqrt(dx)                                    # :369-370
    rl[:, 1, [0, 2]] = rl[:, 1, [0, 2]] + torch.log(dx)
    s, l = editing.drift_factors(B, K, J, torch.linspace(1, 5, steps=K))
    assert torch.equal(mean * s, rm) and torch.equal(logvar + l, rl)


def test_edit_golden_manifest():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import manifest
    want = {}
    for line in open(os.path.join(EDIT, "MANIFEST.sha256")):
        if line.strip() and not line.startswith("#"):
            h, name = line.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(EDIT, f)) for f in sorted(os.listdir(EDIT)) if f.endswith(".npz")}
    assert want == have
    assert set(have) == {"interp_gen_B2.npz", "interp_enc_B2.npz", "mixing_B3_K2.npz", "specific_K2.npz", "drift_B2_K3.npz"}
    for f in have:
        assert os.path.getsize(os.path.join(EDIT, f)) < 512 * 1024
