"""GPU checks of the editing front end (dfx_compose_latents) and of the editing modes built on it:

* the identity recipe gives dfx_sample_latents' bits; the code lerp, the anchor edit and seg rules 1 / 2 give the bits of a torch
  restatement on the same device;
* AnchorDiffAE.interpolate_latent (both branches), combine_latent, combine_latent_specific and interpolate_params against goldens made by the
  reference's own methods (tests/golden/make_golden_edit.py), with the recorded draws and permutations replayed at the same sites.
  Tolerances as tests/test_gpu_forward.py: integer / pass-through keys bit-exact, fp32 engine 2e-4 x max(1, |ref|), bf16 3e-2;
* the seeding contract of the public helpers (difffacto_amd.editing), and the shipped size: 128 shapes x 10 steps through one chain launch.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from difffacto_amd import synth
from _replay import replay_draws

pytestmark = pytest.mark.gpu
EDIT = os.path.join(os.path.dirname(__file__), "golden", "edit")


@pytest.fixture(scope="module")
def sampler():
    from difffacto_amd.latents import LatentSampler
    return LatentSampler(synth.make_latent_weights(seed=0), noise_scale=100.0)


def _inputs(S, K, seed):
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(S, 256, 4, generator=g)
    valid = torch.ones(S, 4)
    valid[1 % S, 3] = 0
    valid[2 % S, 0] = 0
    noise = torch.randn(S * K, 32, generator=g)
    return code.cuda(), valid.cuda(), noise.cuda(), g


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a.float() - b.float()).abs().max()))


def test_identity_recipe_gives_sample_latents_bits(sampler):
    from difffacto_amd import editing
    S, K, N = 5, 3, 64
    code, valid, noise, _ = _inputs(S, K, 1)
    ref = sampler.sample_latents(None, noise, valid, K=K, npoints=N, part_code=code)
    rows = editing.repeat_rows(S, K)
    got = sampler.compose_latents(code, np.repeat(rows[:, None], 4, 1), valid.repeat_interleave(K, 0), noise_src=noise, npoints=N)
    for k in ("part_code", "valid_id", "noise", "mean", "logvar", "params", "seg_mask", "mean_per_point", "logvar_per_point"):
        _same(got[k], ref[k], k)


def test_lerp_is_torch_bits_and_copies_keep_negative_zero(sampler):
    from difffacto_amd import editing
    S, K, N, pid = 4, 6, 64, 2
    code, valid, noise, g = _inputs(S, 1, 2)
    code[0, :8, :] = -0.0
    partner = np.array([2, 0, 3, 1])
    code_a, code_b = editing.interpolation_recipe(S, K, 4, pid, partner)
    code_b[::5, 1] = 3                                                      # a second lerped part on some rows
    alpha = torch.rand(S * K, 4, generator=g).cuda()
    out = sampler.compose_latents(code, code_a, valid.repeat_interleave(K, 0), code_b=code_b, alpha=alpha, noise_src=noise,
                                  noise_row=editing.repeat_rows(S, K), npoints=N)
    ia, ib = torch.from_numpy(code_a).long().cuda(), torch.from_numpy(np.maximum(code_b, 0)).long().cuda()
    a = torch.stack([code[ia[:, j], :, j] for j in range(4)], -1)
    b = torch.stack([code[ib[:, j], :, j] for j in range(4)], -1)
    want = torch.where(torch.from_numpy(code_b >= 0).cuda()[:, None, :], a + (b - a) * alpha[:, None, :], a)
    _same(out["part_code"], want, "part_code")
    copied = out["part_code"][:K, :8, 0]                                    # shape 0, part 0: a copy of -0.0
    assert bool(torch.signbit(copied).all())
    _same(out["noise"], noise.repeat_interleave(K, 0), "noise")


def test_anchor_edit_and_seg_rules_are_torch_bits(sampler):
    from difffacto_amd import editing
    S, K, N = 3, 4, 64
    code, valid, noise, g = _inputs(S, 1, 3)
    rows = editing.repeat_rows(S, K)
    code_a = np.repeat(rows[:, None], 4, 1)
    v = valid.repeat_interleave(K, 0)
    kw = dict(noise_src=noise, noise_row=rows, npoints=N)
    plain = sampler.compose_latents(code, code_a, v, **kw)
    s, l = editing.drift_factors(S, K, 4, torch.linspace(1, 5, steps=K))
    s, l = s.cuda(), l.cuda()
    seg_src = torch.randint(0, 4, (S, N), generator=g, dtype=torch.int32).cuda()
    for mode in (0, 1, 2):
        seg_kw = {"seg_mode": mode} if mode < 2 else {"seg_mode": 2, "seg_src": seg_src, "seg_row": rows}
        out = sampler.compose_latents(code, code_a, v, mean_scale=s, logvar_shift=l, **kw, **seg_kw)
        _same(out["part_code"], plain["part_code"], "part_code")
        mean, logvar = plain["mean"] * s, plain["logvar"] + l                # anchor_gen.py:369-370
        _same(out["mean"], mean, "mean")
        _same(out["logvar"], logvar, "logvar")
        _same(out["params"][:, :3], mean, "params mean")
        torch.testing.assert_close(out["params"][:, 3:], torch.exp(logvar), rtol=2e-7, atol=0)
        seg = editing.seg_ids(v, N, mode) if mode < 2 else seg_src[torch.from_numpy(rows).long().cuda()]
        _same(out["seg_mask"], seg, f"seg_mask[{mode}]")
        idx = seg.long()[:, None, :].expand(-1, 3, -1)
        _same(out["mean_per_point"], torch.gather(mean, 2, idx), "mean_per_point")
        _same(out["logvar_per_point"], torch.gather(logvar, 2, idx) + 0.0, "logvar_per_point")
    with pytest.raises(ValueError):
        sampler.compose_latents(code, code_a, v, seg_mode=2, seg_src=seg_src + 4, seg_row=rows, **kw)


# ---------------------------------------------------------------------------------------------------- goldens of the reference
def _model(T, N, K, precision, ret_interval=5, **flags):
    from difffacto_amd.networks import AnchorDiffAE
    from test_modules_cpu import model_cfg
    m = AnchorDiffAE(**model_cfg(num_timesteps=T, npoints=N, cimle_sample_num=K, ret_interval=ret_interval, **flags), precision=precision)
    W = {"diffusion.model." + k: v for k, v in synth.make_denoiser_weights(0).items()}
    W.update({"encoder." + k: v for k, v in synth.make_latent_weights(0).items()})
    W.update({"encoder.encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.cuda().eval()


def _load(tag):
    g = np.load(os.path.join(EDIT, f"{tag}.npz"))
    draws = [g[f"draw_{i}"] for i in range(int(g["n_draws"]))]
    perms = [g[f"perm_{i}"] for i in range(int(g["n_perms"]))]
    expect = {k[4:]: g[k] for k in g.files if k.startswith("out/")}
    return g, draws, perms, expect


@contextlib.contextmanager
def _replay(model, draws, perms, chain_at, T):
    chain = draws[chain_at:chain_at + T + 1]
    orig = model.decode

    def decode(*a, **k):
        return orig(*a, x_T_noise=torch.from_numpy(chain[0]).cuda(), step_noise=torch.from_numpy(np.stack(chain[1:])).cuda(), **k)

    model.decode = decode
    pq = [torch.from_numpy(p.copy()) for p in perms]
    real = torch.randperm

    def randperm(n, *a, **k):
        p = pq.pop(0)
        assert p.numel() == n
        return p

    torch.randperm = randperm
    try:
        with replay_draws(draws[:chain_at] + draws[chain_at + T + 1:]) as queue:
            yield
        assert not queue and not pq, f"{len(queue)} draws / {len(pq)} permutations were not consumed"
    finally:
        torch.randperm = real


def _compare(pred, expect, tol):
    assert set(map(str, pred)) == set(expect), (sorted(map(str, pred)), sorted(expect))
    worst = 0.0
    for k, v in pred.items():
        ref = expect[str(k)]
        got = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if ref.dtype.kind in "iub":
            assert np.array_equal(got, ref), k
        else:
            err = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
            assert err <= tol, (k, err)
            worst = max(worst, err)
    return worst


MODES = [("interp_gen_B2", dict(interpolate=True, gen=True), "interpolate"),
         ("interp_enc_B2", dict(interpolate=True, gen=False), "interpolate"),
         ("mixing_B3_K2", dict(combine=True), "mixing"),
         ("drift_B2_K3", dict(drift_anchors=True), "interpolate_params")]


@pytest.mark.parametrize("prec,tol", [("f32", 2e-4), ("bf16", 3e-2)])
@pytest.mark.parametrize("tag,flags,name", MODES)
def test_editing_mode_matches_reference(tag, flags, name, prec, tol):
    g, draws, perms, expect = _load(tag)
    batch = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in/")}
    before = {k: v.clone() for k, v in batch.items()}
    T, K, N = int(g["T"]), int(g["K"]), batch["ref"].shape[1]
    model = _model(T, N, K, prec, ret_interval=int(g["ret_interval"]), **flags)
    with _replay(model, draws, perms, int(g["chain_at"]), T):
        out = model(batch, device="cuda", epoch=0)
    assert len(out) == 1 and out[0][1] == name == str(g["name"])
    worst = _compare(out[0][0], expect, tol)
    assert all(torch.equal(before[k], batch[k]) for k in batch), "the caller's batch was written to"
    print(f"{tag}[{prec}]: {len(expect)} keys, worst rel err {worst:.2e}")


@pytest.mark.parametrize("prec,tol", [("f32", 2e-4), ("bf16", 3e-2)])
def test_combine_latent_specific_matches_reference(prec, tol):
    g, draws, perms, expect = _load("specific_K2")
    inputs = [torch.from_numpy(g[f"inp/{i}"]) for i in range(4)]
    model = _model(int(g["T"]), 64, int(g["K"]), prec, ret_interval=int(g["ret_interval"]))
    with _replay(model, draws, perms, int(g["chain_at"]), int(g["T"])):
        pred = model.combine_latent_specific(inputs, "cuda")
    worst = _compare(pred, expect, tol)
    print(f"combine_latent_specific[{prec}]: worst rel err {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- public helpers
@pytest.fixture(scope="module")
def small_model():
    return _model(10, 64, 1, "bf16")


def test_helpers_seedless_calls_are_fresh_and_replay_under_manual_seed(small_model):
    from difffacto_amd import editing
    enc, diff = small_model.encoder, small_model.diffusion
    code = torch.randn(3, 256, 4, generator=torch.Generator().manual_seed(9)).cuda()
    calls = [lambda: editing.interpolate_part(enc, diff, code, 2, 4, npoints=64)["pred"],
             lambda: editing.mix_parts(enc, diff, code, np.array([[0, 1, 2, 0], [1, 2, 0, 1], [2, 0, 1, 2]]), K=2, npoints=64)["pred"],
             lambda: editing.drift_anchors(enc, diff, code, [1.0, 2.0, 3.0], npoints=64)["pred"]]
    for f in calls:
        torch.manual_seed(77)
        a, b = f(), f()
        assert not torch.equal(a, b)
        torch.manual_seed(77)
        a2, b2 = f(), f()
        assert torch.equal(a, a2) and torch.equal(b, b2)
        assert bool(torch.isfinite(a).all())
    r1 = editing.interpolate_part(enc, diff, code, 2, 4, npoints=64, generator=torch.Generator().manual_seed(5))
    r2 = editing.interpolate_part(enc, diff, code, 2, 4, npoints=64, generator=torch.Generator().manual_seed(5))
    assert torch.equal(r1["pred"], r2["pred"])
    # the first step of an interpolation is the unedited shape: its part codes are the source codes, bit for bit
    assert torch.equal(r1["part_code"][:, 0], code)
    a, b = code[:, :, 2], code[[1, 2, 0], :, 2]
    assert torch.equal(r1["part_code"][:, -1, :, 2], a + (b - a) * 1.0)


def test_full_size_interpolation_is_one_chain_launch(monkeypatch):
    from difffacto_amd import editing, engine
    model = _model(10, 2048, 1, "bf16")
    calls = []
    real = engine.DenoiserEngine.sample_chain

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(engine.DenoiserEngine, "sample_chain", counted)
    code = torch.randn(128, 256, 4, generator=torch.Generator().manual_seed(3)).cuda()
    out = editing.interpolate_part(model.encoder, model.diffusion, code, 2, 10, npoints=2048, seed=11)
    assert len(calls) == 1
    variant = engine.last_kernel_variant()
    assert variant.startswith("k_denoise"), variant
    assert out["pred"].shape == (128, 10, 2048, 3) and bool(torch.isfinite(out["pred"]).all())
    print("full-size interpolation: 1280 rows, kernel", variant)
