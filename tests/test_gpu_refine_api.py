"""The public surface of partial chains above the engine: editing.vary_shape, AnchorDiffAE.refine on a batch of data.PartCloudSet, and
examples/edit.py --vary.  N = 256, T = 10, each = 3, parts = [1]: shapes and keys, held parts bit-equal to the batch's clouds, variations
that differ, and the same bits as the engine-level call over the same rows with the same seed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from difffacto_amd import synth  # noqa: E402
import _batch_case as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, EACH, STEPS = 10, 256, 3, 6


@pytest.fixture(scope="module")
def model():
    from difffacto_amd.networks import AnchorDiffAE
    from test_modules_cpu import model_cfg
    m = AnchorDiffAE(**model_cfg(num_timesteps=T, npoints=N, cimle_sample_num=1, ret_interval=5, gen=False), precision="bf16")
    W = {"diffusion.model." + k: v for k, v in synth.make_denoiser_weights(0).items()}
    W.update({"encoder." + k: v for k, v in synth.make_latent_weights(0).items()})
    W.update({"encoder.encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def pcds():
    """Four labelled box clouds, the third without part 1."""
    from difffacto_amd import data
    rng = np.random.default_rng(7)
    counts = ([90, 60, 70, 80], [40, 200, 30, 30], [150, 0, 100, 50], [75, 75, 75, 75])
    ds = data.PartCloudSet.from_arrays([bc.box_cloud(rng, 4, c) for c in counts], 4)
    out = ds.batch([0, 1, 2, 3], seed=3, npoints=N)
    assert out["present"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 1]]
    return out


def _held_points(held, seg):
    return held.gather(1, seg.long()) != 0                                   # (B,N): the point's part is held


def test_vary_shape_against_the_engine_call():
    from difffacto_amd import editing
    from difffacto_amd.modules import AnchoredDiffusion
    from test_modules_cpu import DIFF_CFG
    B = 4
    d = AnchoredDiffusion(num_timesteps=T, precision="bf16", **DIFF_CFG)
    d.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()})
    d = d.cuda().eval()
    part_code, mean, logvar, valid = synth.make_latents(B, seed=12, all_valid=True)
    valid[2] = [1, 0, 1, 1]
    seg = torch.from_numpy(synth.make_seg_mask(valid, N)).cuda()
    params = torch.from_numpy(np.concatenate([mean, np.exp(logvar)], 1).astype(np.float32)).cuda()
    ctx = [torch.from_numpy(part_code).cuda(), params]
    cloud = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(1)).cuda() * 0.2
    v = torch.from_numpy(valid).cuda()
    out = editing.vary_shape(d, ctx, seg, cloud, STEPS, parts=[1], each=EACH, valid_id=v, seed=11, ret_interval=5)
    assert set(out) == {"pred", "seg_mask", "held", "traj"}
    assert out["pred"].shape == (B, EACH, N, 3) and out["seg_mask"].shape == (B, EACH, N) and out["held"].shape == (B, 4)
    assert out["traj"].shape == (1, B, EACH, N, 3)                           # t = 5, the one slot six steps execute
    assert out["held"].tolist() == [[1, 0, 1, 1]] * B
    assert torch.equal(out["seg_mask"], seg[:, None].expand(B, EACH, N))
    held = _held_points(out["held"], seg)
    assert held[2].all() and int(held[0].sum()) == 3 * N // 4
    for k in range(EACH):
        assert torch.equal(out["pred"][:, k][held], cloud[held]) and torch.equal(out["traj"][0, :, k][held], cloud[held])
    for b in (0, 1, 3):
        free = ~held[b]
        assert not torch.equal(out["pred"][b, 0][free], out["pred"][b, 1][free]) and not torch.equal(out["pred"][b, 1][free], out["pred"][b, 2][free])
        assert not torch.equal(out["pred"][b, 0][free], cloud[b][free])
    assert bool(torch.isfinite(out["pred"]).all())
    # the engine-level call over the same rows with the same seed
    eng = d.model.engine()
    rep = lambda t: t.repeat_interleave(EACH, 0)
    sc = eng.prepare_shapes(rep(ctx[0]), rep(params[:, :3]), rep(params[:, 3:]), rep(v))
    pred, traj = eng.refine_chain(sc, rep(seg), rep(cloud.transpose(1, 2)), STEPS, seed=11, hold=rep(out["held"]), ret_interval=5)
    assert torch.equal(pred.reshape(B, EACH, N, 3), out["pred"]) and torch.equal(traj.reshape(1, B, EACH, N, 3), out["traj"])
    # a batch split over two calls: the rows before a call are its shape_offset
    tail = editing.vary_shape(d, [ctx[0][3:], params[3:]], seg[3:], cloud[3:], STEPS, parts=[1], each=EACH, valid_id=v[3:], seed=11,
                              shape_offset=3 * EACH)
    assert torch.equal(tail["pred"], out["pred"][3:])
    # parts=None: nothing held, every point regenerated
    free = editing.vary_shape(d, ctx, seg, cloud, STEPS, each=1, valid_id=v, seed=11)
    assert free["held"].sum() == 0 and not bool((free["pred"][:, 0] == cloud).all(-1).any())
    with pytest.raises(ValueError):
        editing.vary_shape(d, ctx, seg, cloud[:, :128], STEPS)


def test_refine_on_a_part_cloud_batch(model, pcds):
    from difffacto_amd import editing
    B = 4
    torch.manual_seed(5)
    out = model.refine(pcds, STEPS, parts=[1], each=EACH, seed=11)
    assert {"pred", "seg_mask", "held", "input_ref", "present"} <= set(out)
    assert out["pred"].shape == (B, EACH, N, 3) and out["seg_mask"].shape == (B, EACH, N) and out["held"].shape == (B, 4)
    ref, seg = pcds["ref"].cuda(), pcds["ref_seg_mask"].cuda()
    assert out["held"].tolist() == [[1, 0, 1, 1]] * B and torch.equal(out["input_ref"], ref)
    held = _held_points(out["held"], seg)
    assert held[2].all() and 0 < int(held[0].sum()) < N
    for k in range(EACH):
        assert torch.equal(out["pred"][:, k][held], ref[held])               # held parts: the batch's own points, bit for bit
    for b in (0, 1, 3):
        free = ~held[b]
        assert not torch.equal(out["pred"][b, 0][free], out["pred"][b, 1][free]) and not torch.equal(out["pred"][b, 0][free], out["pred"][b, 2][free])
    assert bool(torch.isfinite(out["pred"]).all())
    # the same latents (the encoder's host draws replayed) through vary_shape and through the engine
    torch.manual_seed(5)
    with torch.no_grad():
        noise, _ = model.encoder.sample_noise(pcds, "cuda", 1)
        ctx = model.encoder(pcds, "cuda", noise=noise)[0]
    valid = pcds["present"].cuda().float()
    again = editing.vary_shape(model.diffusion, ctx, seg, ref, STEPS, parts=[1], each=EACH, valid_id=valid, seed=11)
    assert torch.equal(again["pred"], out["pred"])
    eng = model.diffusion.model.engine()
    rep = lambda t: t.repeat_interleave(EACH, 0)
    sc = eng.prepare_shapes(rep(ctx[0]), rep(ctx[1][:, :3]), rep(ctx[1][:, 3:]), rep(valid))
    pred, _ = eng.refine_chain(sc, rep(seg), rep(ref.transpose(1, 2)), STEPS, seed=11, hold=rep(out["held"]))
    assert torch.equal(pred.reshape(B, EACH, N, 3), out["pred"])
    # another seed: other variations, the same held points
    other = model.refine(pcds, STEPS, parts=[1], each=1, seed=12)
    assert torch.equal(other["pred"][:, 0][held], ref[held]) and not torch.equal(other["pred"][:, 0], out["pred"][:, 0])


def test_edit_example_vary(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "edit.py"), "--vary", "--shapes", "2", "--timesteps", "10", "--steps-back", "5",
                        "--parts", "1", "--each", "2", "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "vary: 4 rows in one launch, 5 of 10 steps back, parts [1]" in r.stdout and "unchanged: True" in r.stdout and "finite: True" in r.stdout
    pred, base = np.load(tmp_path / "vary.npy"), np.load(tmp_path / "vary_base.npy")
    seg = np.load(tmp_path / "vary_seg.npy")
    assert pred.shape == (2, 2, 2048, 3) and base.shape == (2, 2048, 3) and seg.shape == (2, 2, 2048)
    keep = seg != 1
    assert np.array_equal(pred[keep], np.broadcast_to(base[:, None], pred.shape)[keep]) and not np.array_equal(pred[~keep], np.broadcast_to(base[:, None], pred.shape)[~keep])
