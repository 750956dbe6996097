"""GPU checks of the training-batch assembly (difffacto_amd/data.py over batch_kernels.hip): the reference's recorded items through
PartCloudSet.batch with explicit draws, with the equalities and the error gate of test_batch_cpu.py; bit-reproducibility; batch
sizes 1 and 130 with repeated indices; the Philox draws (range, uniformity, independence of row and batch size, seeds); a loader
batch through training.stage1_losses."""
import numpy as np
import pytest
import torch

import _batch_case as bc

pytestmark = pytest.mark.gpu


def _np(out):
    return {k: v.detach().cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _case_batch(name, **extra):
    from difffacto_amd import data
    d, cfg, C = bc.load_case(name)
    ds = data.PartCloudSet.from_arrays([(d["points"], d["labels"])], C)
    cfg = dict(cfg, **extra)
    out = ds.batch([0], choice=d["choice"][None], drop_u=d["drop_u"][None], aug_u=d["aug_u"][None], npoints=len(d["choice"]), **cfg)
    return d, cfg, C, out


PARITY = {}


@pytest.mark.parametrize("name", bc.case_names())
def test_batch_matches_reference_fixture(name):
    d, cfg, C, out = _case_batch(name)
    assert out["attn_map"] is out["ref_attn_map"] and out["seg_mask"] is out["ref_seg_mask"]
    assert out["attn_map"].dtype == torch.int64 and out["seg_mask"].dtype == torch.int64 and out["ref"].dtype == torch.float32
    assert out["noise"].shape == (1, 1) and out["noise"].dtype == torch.float64 and out["token"] == ["0"] and out["id"].tolist() == [0]
    got = {k: v[0] for k, v in _np(out).items()}
    bc.check_exact(got, d, name)
    f64 = bc.item_numpy(d["points"], d["labels"], d["choice"], d["drop_u"], d["aug_u"], C, cfg)
    lines, missed = bc.gate_lines(name, bc.family_errors(d, f64), bc.family_errors(got, f64))
    for line in lines:
        print("BATCH_PARITY gpu   " + line)
    PARITY[name] = lines
    bc.write_parity("gpu", PARITY)          # profiles/batch_parity.txt, once every fixture has run
    assert not missed, "\n".join(lines)


def _toy_set(n_clouds=6, seed=0, sizes=(40, 300, 2700)):
    from difffacto_amd import data
    rng = np.random.default_rng(seed)
    clouds = []
    for k in range(n_clouds):
        m = sizes[k % len(sizes)]
        counts = np.bincount(rng.integers(0, 4, m - 4), minlength=4) + 1
        clouds.append(bc.box_cloud(rng, 4, counts))
    return data.PartCloudSet.from_arrays(clouds, 4), clouds


OPTS = dict(npoints=256, dropout_part=0.3, augment=True)


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v[rows_a], b[k][rows_b]), k


def test_two_runs_are_bit_identical_and_rows_do_not_depend_on_the_batch():
    ds, clouds = _toy_set()
    a, b = ds.batch([3, 5, 1, 3], seed=5, **OPTS), ds.batch([3, 5, 1, 3], seed=5, **OPTS)
    _same(a, b)
    _same(a, a, slice(0, 1), slice(3, 4))                       # the same cloud and sample_id twice in one batch
    one = ds.batch([5], seed=5, **OPTS)                         # B = 1
    _same(one, a, slice(0, 1), slice(1, 2))
    assert one["ref"].shape == (1, 256, 3) and one["scale"].shape == (1, 1, 3) and one["shift"].shape == (1, 1, 3)
    # explicit draws: the device result equals the host-side restatement's decisions
    got = _np(one)
    c = ds.draw(torch.tensor([5], device="cuda"), torch.tensor([5], device="cuda"), 5, 256)
    f64 = bc.item_numpy(*clouds[5], c[0][0].cpu().numpy(), c[1][0].cpu().numpy(), c[2][0].cpu().numpy(), 4,
                        dict(bc.DEFAULT_CFG, dropout_part=0.3, augment_shift=True, augment_scale=True))
    bc.check_exact({k: v[0] for k, v in got.items()}, f64, "B=1")


def test_batch_of_130_with_repeated_indices():
    ds, _ = _toy_set()
    idx = (np.arange(130) * 7) % 6
    sid = np.arange(130) % 50
    big = ds.batch(idx, sample_id=sid, seed=9, **OPTS)
    assert big["ref"].shape == (130, 256, 3) and big["attn_map"].shape == (130, 256, 4) and big["part_shift"].shape == (130, 3, 4)
    assert torch.isfinite(big["ref"]).all() and torch.isfinite(big["input"]).all()
    assert torch.equal(big["attn_map"].sum(-1), torch.ones(130, 256, dtype=torch.int64, device="cuda"))
    assert torch.equal(big["attn_map"].argmax(-1), big["seg_mask"])
    for r in (0, 64, 129):
        one = ds.batch([idx[r]], sample_id=[sid[r]], seed=9, **OPTS)
        _same(one, big, slice(0, 1), slice(r, r + 1))
    # rows 1 and 43: same cloud (7 * 42 % 6 == 0), other sample_id: other draws
    assert idx[1] == idx[43] and sid[1] != sid[43] and not torch.equal(big["ref"][1], big["ref"][43])


def test_draws():
    from difffacto_amd import data
    rng = np.random.default_rng(1)
    sizes = (40, 300, 2700)
    ds = data.PartCloudSet.from_arrays([bc.box_cloud(rng, 4, [m // 4] * 4) for m in sizes], 4)
    B, N = 64, 2048
    idx = torch.tensor(np.arange(B) % 3, device="cuda")
    sid = torch.arange(B, device="cuda")
    choice, drop_u, aug_u = ds.draw(idx, sid, 1234, N)
    assert choice.shape == (B, N) and choice.dtype == torch.int32 and drop_u.shape == (B, 4) and aug_u.shape == (B, 6)
    M = torch.tensor(sizes, device="cuda")[idx][:, None]
    assert bool((choice >= 0).all()) and bool((choice < M).all())
    for u in (drop_u, aug_u):
        assert bool((u >= 0).all()) and bool((u < 1).all()) and 0.4 < float(u.mean()) < 0.6 and u.unique().numel() > u.numel() // 2
    # chi-square of the 300-point cloud's counts: 21 rows x 2048 draws over 300 bins
    rows = choice[idx == 1].reshape(-1).cpu().numpy()
    counts = np.bincount(rows, minlength=300)
    expected = len(rows) / 300.0
    chi2, dof = float(((counts - expected) ** 2 / expected).sum()), 299
    print(f"BATCH_DRAW chi-square {chi2:.1f} (dof {dof}, bound {dof + 6 * np.sqrt(2 * dof):.1f})")
    assert chi2 < dof + 6 * np.sqrt(2 * dof)
    # an item's draws depend on (seed, sample_id) and the cloud only
    pair = ds.draw(torch.tensor([1, 2], device="cuda"), torch.tensor([3, 7], device="cuda"), 1234, N)
    for r, (s, i) in enumerate(((1, 3), (2, 7))):
        single = ds.draw(torch.tensor([s], device="cuda"), torch.tensor([i], device="cuda"), 1234, N)
        for a, b in zip(pair, single):
            assert torch.equal(a[r], b[0])
    a = ds.batch([1, 2], sample_id=[3, 7], seed=1234, npoints=N)
    for r, (s, i) in enumerate(((2, 7), (1, 3))):
        _same(ds.batch([s], sample_id=[i], seed=1234, npoints=N), a, slice(0, 1), slice(1 - r, 2 - r))
    other = ds.draw(idx, sid, 1235, N)
    assert not torch.equal(other[0], choice) and not torch.equal(other[1], drop_u) and not torch.equal(other[2], aug_u)
    again = ds.draw(idx, sid, 1234, N)
    assert all(torch.equal(x, y) for x, y in zip(again, (choice, drop_u, aug_u)))
    # more items than a grid's second dimension holds (65535)
    B = 70000
    idx, sid = torch.arange(B, device="cuda") % 3, torch.arange(B, device="cuda")
    big = ds.draw(idx, sid, 1234, 10)
    assert bool((big[0] >= 0).all()) and bool((big[0] < torch.tensor(sizes, device="cuda")[idx][:, None]).all())
    assert torch.equal(big[0][:64], choice[:, :10]) and torch.equal(big[1][:64], drop_u) and torch.equal(big[0][B - 1:], ds.draw(idx[B - 1:], sid[B - 1:], 1234, 10)[0])


def test_largest_item_and_lazy_check():
    """N = 8192 (128 KB of LDS) against the float64 restatement's decisions; a label outside [0,C) through the lazy check."""
    from difffacto_amd import data
    rng = np.random.default_rng(2)
    pts, seg = bc.box_cloud(rng, 8, [400, 5, 300, 0, 350, 12, 380, 7])
    ds = data.PartCloudSet.from_arrays([(pts, seg)], 8)
    choice = rng.integers(0, len(pts), 8192).astype(np.int32)
    drop_u, aug_u = rng.uniform(0, 1, 8).astype(np.float32), rng.uniform(0, 1, 6).astype(np.float32)
    out = ds.batch([0], choice=choice[None], drop_u=drop_u[None], aug_u=aug_u[None], npoints=8192, dropout_part=0.5)
    f64 = bc.item_numpy(pts, seg, choice, drop_u, aug_u, 8, dict(bc.DEFAULT_CFG, dropout_part=0.5))
    got = {k: v[0] for k, v in _np(out).items()}
    bc.check_exact(got, f64, "N=8192")
    errs = bc.family_errors(got, f64)
    amp = 1.0 / min(1.0, float(f64["part_scale"].min()))
    for k, (err, ulp) in errs.items():
        assert err <= 8 * max(ulp, errs["ref"][1]) * (amp if k == "input" else 1.0), (k, err)
    bad = data.PartCloudSet.from_arrays([(pts, np.where(np.arange(len(pts)) < 3, 8, seg))], 8)
    with pytest.raises(ValueError, match=r"3 sampled label\(s\) outside \[0,8\)"):
        bad.batch([0], choice=np.arange(64, dtype=np.int32)[None], drop_u=drop_u[None], aug_u=aug_u[None], npoints=64)
    lazy = bad.batch([0], choice=np.arange(64, dtype=np.int32)[None], drop_u=drop_u[None], aug_u=aug_u[None], npoints=64, check=False)
    with pytest.raises(ValueError, match="3 sampled"):
        lazy["check"].raise_if_bad()
    with pytest.raises(IndexError, match="1 item"):
        bad.batch(torch.tensor([4], device="cuda"), seed=1, npoints=64)          # a device index is checked by the kernel


def test_noise_rows_and_loader():
    from difffacto_amd import data
    ds, _ = _toy_set()
    ds.set_noise(torch.arange(6 * 32, dtype=torch.float32).reshape(6, 32))
    out = ds.batch([4, 0], seed=1, npoints=64)
    assert out["noise"].shape == (2, 32) and out["noise"][:, 0].tolist() == [128.0, 0.0] and out["token"] == ["4", "0"]
    assert out["class"].shape == (2, 1) and out["scale"].shape == (2, 1, 1)
    a, b = data.PartCloudLoader(ds, 4, seed=3, **OPTS), data.PartCloudLoader(ds, 4, seed=3, **OPTS)
    ea, eb = [list(a), list(a)], [list(b), list(b)]
    assert len(ea[0]) == 1 and ea[0][0]["ref"].shape == (4, 256, 3)
    for e in range(2):
        _same(ea[e][0], eb[e][0])
    assert not torch.equal(ea[0][0]["ref"], ea[1][0]["ref"])
    a.raise_if_bad()
    tail = list(data.PartCloudLoader(ds, 4, drop_last=False, shuffle=False, seed=3, npoints=64))
    assert [t["id"].tolist() for t in tail] == [[0, 1, 2, 3], [4, 5]]


def test_loader_and_host_arguments_do_not_make_the_host_wait():
    """With check=False nothing in the loader or in batch() may synchronise the host with the stream: torch's sync debug mode
    turns every such call (a blocking copy from pageable memory among them) into an error."""
    from difffacto_amd import data
    ds, _ = _toy_set()
    loader = data.PartCloudLoader(ds, 2, seed=3, **OPTS)
    host_args = dict(sample_id=np.asarray([3, 4]), choice=np.zeros((2, 256), np.int32), drop_u=np.zeros((2, 4), np.float32),
                     aug_u=torch.zeros(2, 6), check=False, **OPTS)
    first = list(loader)                                          # warm-up: code objects, the allocators' first blocks
    ds.batch([1, 2], **host_args)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                         # the mode is live: this is the copy the loader must not make
            torch.zeros(3).to("cuda")
        epochs = [list(loader), list(loader)]
        ds.batch([1, 2], **host_args)
        ds.batch(np.asarray([0, 5]), seed=4, check=False, **OPTS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    loader.raise_if_bad()
    assert loader._bad is None and all(len(e) == 3 and e[0]["token"] == [str(i) for i in e[0]["id"].tolist()] for e in epochs)
    replay = data.PartCloudLoader(ds, 2, seed=3, **OPTS)
    _same(first[2], list(replay)[2])


def test_loader_adds_up_the_deferred_check():
    from difffacto_amd import data
    rng = np.random.default_rng(3)
    clouds = [bc.box_cloud(rng, 4, [30, 30, 30, 30]) for _ in range(4)]
    clouds[2] = (clouds[2][0], np.full(120, 5, np.int32))
    loader = data.PartCloudLoader(data.PartCloudSet.from_arrays(clouds, 4), 2, seed=1, npoints=64)
    for _ in range(3):
        list(loader)
    assert loader._bad.shape == (2,)                              # one device counter, however many batches
    with pytest.raises(ValueError, match=r"192 sampled label\(s\)"):
        loader.raise_if_bad()
    loader.raise_if_bad()                                         # cleared


def test_loader_batch_trains_stage1():
    """A loader batch (B = 4, N = 256, toy set) through training.stage1_losses: finite losses, identical to the same tensors as a
    hand-built dict."""
    from difffacto_amd import data, training
    ds, _ = _toy_set(sizes=(300, 400))
    batch = next(iter(data.PartCloudLoader(ds, 4, seed=2, npoints=256, dropout_part=0.2)))
    enc, diff = bc.stage1_modules()
    hand = {"input": batch["input"].clone(), "ref": batch["ref"].clone(), "present": batch["present"].clone(),
            "dp_present": batch["dp_present"].clone(), "ref_seg_mask": batch["seg_mask"].clone(),
            "ref_attn_map": batch["attn_map"].to(torch.float32), "part_shift": batch["part_shift"].clone(),
            "part_scale": batch["part_scale"].clone(), "noise": torch.zeros(4, 1, dtype=torch.float64).cuda()}
    t = torch.tensor([3, 50, 77, 99], device="cuda")
    noise = torch.randn(4, 3, 256, generator=torch.Generator().manual_seed(0)).cuda()
    results = []
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    for pcds in (batch, hand):
        enc.load_state_dict(state)                               # the BatchNorm running statistics move with every forward
        torch.manual_seed(7)
        losses = training.stage1_losses(enc, diff, pcds, t=t, noise=noise)
        results.append({k: float(v.detach().sum()) for k, v in losses.items() if "loss" in k})
    assert set(results[0]) >= {"prior_loss", "mse_loss"} and all(np.isfinite(v) for v in results[0].values()), results
    assert results[0] == results[1], results
