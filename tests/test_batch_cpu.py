"""CPU checks of the training-batch assembly: the entry points are exported and bound and reject bad arguments before touching a GPU;
the kernel's per-item routine, compiled for the host (dfx_debug_batch_build_host), against the reference's recorded items
(tests/golden/batch/, make_golden_batch.py) and against a float64 restatement (tests/_batch_case.py); the Python layer's argument
checks, the ShapeNet txt reader and the save / load round trip; the fixtures' manifest.

Gate of the float families (ref, input, shift, scale, part_shift, part_scale), per fixture: E_ref = max |reference - float64
restatement|, E_nat the same for the native result, E_nat <= 2 E_ref + one float32 ulp of the family's largest magnitude.  The
native value is a float32 rounding of a better-accumulated quantity and should sit inside the reference's own error band; the
factor 2 is there because the per-part division amplifies ulp-level shift differences by 1 / part_scale and a maximum over a few
thousand values is noisy.  The table is printed (BATCH_PARITY lines) and, once every fixture has run, written to
profiles/batch_parity.txt (the `host` rows; test_gpu_batch.py writes the `gpu` rows)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import _batch_case as bc

NEW = ("dfx_batch_draw", "dfx_batch_build_f32", "dfx_debug_batch_build_host")
FAKE = ctypes.c_void_p(0x1000)   # a non-null "device pointer": never dereferenced, the checks fail first


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _err(L, rc):
    return rc, (L.dfx_last_error() or b"").decode()


def test_batch_symbols_are_exported_and_bound(L):
    from difffacto_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert L.dfx_version() >= 105 and L.dfx_abi_version() == 5 == _ffi.DFX_ABI_VERSION


def test_product_entry_points_reject_bad_arguments_without_a_gpu(L):
    def build(S=3, B=2, C=4, N=256, sm=1, pm=5, points=FAKE, n_bad=FAKE):
        return _err(L, L.dfx_batch_build_f32(points, FAKE, FAKE, S, FAKE, B, FAKE, FAKE, FAKE, C, N, sm, pm, 0, 0.0, 0, 0,
                                             *([FAKE] * 10), n_bad, None))
    for kw, msg in [(dict(points=None), "null input"), (dict(n_bad=None), "null output"), (dict(S=0), "positive"), (dict(B=0), "positive"),
                    (dict(C=9), "n_class = 9"), (dict(C=0), "n_class = 0"), (dict(N=9), "npoints = 9"), (dict(N=8193), "npoints = 8193"),
                    (dict(sm=5), "scale_mode = 5"), (dict(sm=-1), "scale_mode"), (dict(pm=7), "part_scale_mode = 7")]:
        rc, m = build(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)

    def draw(S=3, B=2, N=256, C=4, choice=FAKE):
        return _err(L, L.dfx_batch_draw(FAKE, S, FAKE, FAKE, B, N, C, 7, choice, FAKE, FAKE, None))
    for kw, msg in [(dict(choice=None), "null"), (dict(B=-1), "positive"), (dict(N=9), "npoints"), (dict(N=8193), "npoints"), (dict(C=9), "n_class")]:
        rc, m = draw(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)


def _toy(rng, counts, C=4):
    pts, seg = bc.box_cloud(rng, C, counts)
    return pts, seg


def test_host_twin_rejects_bad_arguments(L):
    rng = np.random.default_rng(0)
    pts, seg = _toy(rng, [20, 20, 20, 20])
    cfg = bc.DEFAULT_CFG

    def run(index=(0,), N=16, C=4, offsets=None, sm=1, pm=5):
        offsets = [0, len(pts)] if offsets is None else offsets
        B = len(index)
        rc, _ = bc.host_batch_raw(L, pts, seg, offsets, index, np.zeros((B, max(N, 1)), np.int32), np.zeros((B, C)), np.zeros((B, 6)), C, N, sm, pm, cfg)
        return _err(L, rc)
    assert run()[0] == 0
    for kw, msg in [(dict(index=(1,)), "index[0] = 1 outside [0,1)"), (dict(index=(0, -1)), "index[1] = -1"), (dict(N=9), "npoints = 9"),
                    (dict(N=8193), "npoints = 8193"), (dict(C=9), "n_class = 9"), (dict(offsets=[0, 0, len(pts)], index=(1, 0)), "cloud 0 is empty"),
                    (dict(sm=6), "scale_mode"), (dict(pm=9), "part_scale_mode")]:
        rc, m = run(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)


def test_host_twin_counts_bad_labels_and_choices(L):
    rng = np.random.default_rng(1)
    pts, seg = _toy(rng, [20, 20, 20, 20])
    seg = seg.copy()
    seg[3], seg[5] = 4, -1
    choice = np.arange(80, dtype=np.int32)[None]
    rc, o = bc.host_batch_raw(L, pts, seg, [0, len(pts)], [0], choice, np.zeros((1, 4)), np.zeros((1, 6)), 4, 80, 1, 5, bc.DEFAULT_CFG)
    assert rc == 0 and o["n_bad"].tolist() == [2, 0]
    assert o["attn_map"][0, 3].sum() == 0 and o["attn_map"][0, 5].sum() == 0 and o["attn_map"][0].sum() == 78
    choice[0, 7] = len(pts)      # past the cloud: read as 0 and reported, never dereferenced
    rc, o = bc.host_batch_raw(L, pts, seg, [0, len(pts)], [0], choice, np.zeros((1, 4)), np.zeros((1, 6)), 4, 80, 1, 5, bc.DEFAULT_CFG)
    assert rc == 0 and o["n_bad"].tolist() == [2, 1]


# ---- the reference's recorded items ----
PARITY = {}


@pytest.mark.parametrize("name", bc.case_names())
def test_host_twin_matches_reference_fixture(L, name):
    d, cfg, C = bc.load_case(name)
    got = bc.host_item(L, d["points"], d["labels"], d["choice"], d["drop_u"], d["aug_u"], C, cfg)
    bc.check_exact(got, d, name)
    f64 = bc.item_numpy(d["points"], d["labels"], d["choice"], d["drop_u"], d["aug_u"], C, cfg)
    bc.check_exact(f64, d, name + " (float64 restatement)")
    lines, missed = bc.gate_lines(name, bc.family_errors(d, f64), bc.family_errors(got, f64))
    for line in lines:
        print("BATCH_PARITY host  " + line)
    PARITY[name] = lines
    bc.write_parity("host", PARITY)
    assert not missed, "\n".join(lines)


def test_parity_table_holds_every_fixture_for_the_host_twin():
    rows = [l for l in open(bc.PARITY_FILE) if l.startswith("host ")]
    assert len(rows) == len(bc.case_names()) * len(bc.FAMILIES) and not any(l.rstrip().endswith("MISS") for l in rows)


def test_fixtures_hold_the_cases_they_are_named_after():
    names = bc.case_names()
    assert len(names) == 16
    seen = set()
    for name in names:
        d, cfg, C = bc.load_case(name)
        sampled = np.bincount(d["labels"][d["choice"]], minlength=C)
        final = np.bincount(d["seg_mask"], minlength=C)
        zero = int((d["input"] == 0).all(-1).sum())
        seen.add("M<N" if len(d["points"]) < len(d["choice"]) else "M>=N")
        seen |= {f"sampled {c}" for c in sampled.tolist() if c in (9, 10)}
        if zero:
            seen.add("zero rows")
        if ((sampled == 9) & (final == 10) & (d["present"] == 1)).any():
            seen.add("lifted to 10")
        if ((sampled > 0) & (sampled < 10) & (final == 0)).sum() >= 2:
            seen.add("chain")
        if (sampled == 0).sum() == 1:
            seen.add("absent")
        if (sampled > 0).sum() == 1:
            seen.add("one part")
        if cfg["dropout_part"] > 0:
            seen.add("dropout")
        seen.add(f"aug {int(cfg['augment_shift'])}{int(cfg['augment_scale'])}")
        seen.add(f"{cfg['scale_mode']}+{cfg['part_scale_mode']}+clip{int(cfg['clip'])}")
        seen.add(f"N {len(d['choice'])}")
    want = {"M<N", "M>=N", "sampled 9", "sampled 10", "zero rows", "lifted to 10", "chain", "absent", "one part", "dropout", "aug 00",
            "aug 11", "aug 10", "aug 01", "shape_unit+shape_canonical+clip0", "shape_bbox+shape_canonical_bbox+clip1",
            "shape_unit+shape_canonical+clip1", "N 250", "N 256", "N 2048"}
    assert want <= seen, want - seen


# ---- no reference fixture: against the float64 restatement only ----
def _against_f64(L, pts, seg, choice, C, cfg, what, drop_u=None, aug_u=None):
    """Equal decisions; floats within 8 float32 ulp of the largest magnitude (the family's or ref's), divided by the smallest part
    scale for the per-part rows: a float32 rounding each of the shift, the scale, the difference and the quotient on both levels."""
    drop_u = np.linspace(0.05, 0.95, C).astype(np.float32) if drop_u is None else drop_u
    aug_u = np.asarray([0.1, 0.5, 0.9, 0.2, 0.6, 0.8], np.float32) if aug_u is None else aug_u
    got = bc.host_item(L, pts, seg, choice, drop_u, aug_u, C, cfg)
    f64 = bc.item_numpy(pts, seg, choice, drop_u, aug_u, C, cfg)
    bc.check_exact(got, f64, what)
    amp = 1.0 / min(1.0, float(f64["part_scale"].min()))
    errs = bc.family_errors(got, f64)
    for k, (err, ulp) in errs.items():
        bound = 8 * max(ulp, errs["ref"][1]) * (amp if k == "input" else 1.0)   # every family inherits the rounding of ref
        print(f"BATCH_F64 {what} {k}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, k, err, bound)
    return got, f64


def test_flat_part_follows_the_written_rule(L):
    """Part 1 lies in the plane y = 0.25: std(0) has an exact zero, so present = 0, the scale of that axis is 1 and the shift is
    the mean; numpy's float32 std of such a part is almost never exactly zero."""
    rng = np.random.default_rng(2)
    pts, seg = _toy(rng, [60, 60, 60, 60])
    pts = pts.copy()
    pts[seg == 1, 1] = 0.25
    choice = rng.integers(0, len(pts), 250).astype(np.int32)
    got, f64 = _against_f64(L, pts, seg, choice, 4, bc.DEFAULT_CFG, "flat")
    assert got["present"].tolist() == [1, 0, 1, 1] and got["part_scale"][1, 1] == 1.0
    assert got["part_scale"][0, 1] != 1.0 and got["part_scale"][2, 1] != 1.0
    ref_y = got["ref"][got["seg_mask"] == 1, 1]
    assert np.all(ref_y == ref_y[0]) and got["part_shift"][1, 1] == ref_y[0]
    assert np.all(got["input"][got["seg_mask"] == 1, 1] == 0)


@pytest.mark.parametrize("scale_mode,part_scale_mode,clip", [
    ("shape_half", "shape_half", False), ("shape_34", "shape_unit", False), ("shape_bbox", "shape_bbox", False), (None, None, False),
    ("none", "shape_canonical_bbox", False), ("shape_unit", "shape_34", True), ("shape_half", "shape_canonical", True)])
def test_remaining_scale_modes(L, scale_mode, part_scale_mode, clip):
    rng = np.random.default_rng(3)
    pts, seg = _toy(rng, [80, 5, 70, 90])
    choice = rng.integers(0, len(pts), 256).astype(np.int32)
    cfg = dict(bc.DEFAULT_CFG, scale_mode=scale_mode, part_scale_mode=part_scale_mode, clip=clip, dropout_part=0.5, augment_shift=True,
               augment_scale=True)
    got, _ = _against_f64(L, pts, seg, choice, 4, cfg, f"{scale_mode}+{part_scale_mode}")
    assert got["scale"].shape == (1, 3)


def test_smallest_item_and_class_counts(L):
    rng = np.random.default_rng(4)
    pts, seg = _toy(rng, [30, 30, 30, 30])
    # N = 10: all ten samples from part 2, and nine from part 2 with one from part 0 (relabelled)
    p2, p0 = np.flatnonzero(seg == 2), np.flatnonzero(seg == 0)
    got, _ = _against_f64(L, pts, seg, p2[:10].astype(np.int32), 4, bc.DEFAULT_CFG, "N=10 one part")
    assert got["present"].tolist() == [0, 0, 1, 0]
    got, _ = _against_f64(L, pts, seg, np.concatenate([p0[:1], p2[:9]]).astype(np.int32), 4, bc.DEFAULT_CFG, "N=10 nine and one")
    assert got["present"].tolist() == [0, 0, 1, 0] and np.all(got["seg_mask"] == 2)
    # C = 1 and C = 8
    pts1, seg1 = _toy(rng, [50], C=1)
    got, _ = _against_f64(L, pts1, seg1, rng.integers(0, 50, 64).astype(np.int32), 1, bc.DEFAULT_CFG, "C=1")
    assert got["attn_map"].shape == (64, 1) and got["attn_map"].all() and got["part_shift"].shape == (3, 1)
    pts8, seg8 = _toy(rng, [40, 3, 40, 0, 40, 12, 40, 7], C=8)
    got, _ = _against_f64(L, pts8, seg8, rng.integers(0, len(pts8), 300).astype(np.int32), 8, dict(bc.DEFAULT_CFG, dropout_part=0.5), "C=8")
    assert got["attn_map"].shape == (300, 8) and got["present"][3] == 0 and got["present"][0] == 1


def test_items_do_not_depend_on_their_row(L):
    """A batch of three items over two clouds through the host twin: each row equals the single-item call."""
    rng = np.random.default_rng(5)
    a, b = _toy(rng, [40, 40, 4, 40]), _toy(rng, [25, 0, 25, 25])
    pts, seg = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    offsets = [0, len(a[0]), len(pts)]
    index = [1, 0, 1]
    choice = np.stack([rng.integers(0, len((a, b)[s][0]), 128) for s in index]).astype(np.int32)
    drop_u, aug_u = rng.uniform(0, 1, (3, 4)).astype(np.float32), rng.uniform(0, 1, (3, 6)).astype(np.float32)
    cfg = dict(bc.DEFAULT_CFG, dropout_part=0.3, augment_shift=True, augment_scale=True)
    rc, o = bc.host_batch_raw(L, pts, seg, offsets, index, choice, drop_u, aug_u, 4, 128, 1, 5, cfg)
    assert rc == 0 and not o["n_bad"].any()
    for r, s in enumerate(index):
        one = bc.host_item(L, (a, b)[s][0], (a, b)[s][1], choice[r], drop_u[r], aug_u[r], 4, cfg)
        for k, v in one.items():
            assert np.array_equal(o[k][r], v), (r, k)


# ---- the Python layer (no GPU: a set on the CPU device holds the data; batch() itself needs the GPU) ----
def _cpu_set(rng, labels_ok=True):
    from difffacto_amd import data
    clouds = [_toy(rng, [20, 20, 20, 20]) for _ in range(3)]
    if not labels_ok:
        clouds[1][1][:5] = 4
    return data.PartCloudSet.from_arrays(clouds, 4, device="cpu"), clouds


def test_python_layer_argument_checks():
    from difffacto_amd import data
    rng = np.random.default_rng(6)
    ds, _ = _cpu_set(rng)
    assert len(ds) == 3 and ds.offsets.tolist() == [0, 80, 160, 240] and ds.labels.dtype.is_floating_point is False
    with pytest.raises(IndexError, match=r"outside \[0,3\)"):
        ds.batch([0, 3])
    with pytest.raises(IndexError):
        ds.batch([-1])
    with pytest.raises(ValueError, match="npoints = 9"):
        ds.batch([0], npoints=9)
    with pytest.raises(ValueError, match="npoints = 8193"):
        ds.batch([0], npoints=8193)
    with pytest.raises(NotImplementedError, match="global_unit"):
        ds.batch([0], scale_mode="global_unit")
    with pytest.raises(NotImplementedError, match="global_unit"):
        ds.batch([0], part_scale_mode="global_unit")
    with pytest.raises(ValueError, match="scale_mode"):
        ds.batch([0], scale_mode="shape_canonical")
    with pytest.raises(ValueError, match="n_class = 9"):
        data.PartCloudSet.from_arrays([_toy(rng, [20] * 4)], 9, device="cpu")
    with pytest.raises(ValueError, match="cloud 1 is empty"):
        data.PartCloudSet.from_arrays([_toy(rng, [20] * 4), (np.zeros((0, 3)), np.zeros(0))], 4, device="cpu")
    with pytest.raises(ValueError, match=r"\(3, D\)"):
        ds.set_noise(np.zeros((2, 8)))
    with pytest.raises(TypeError, match="index"):
        data.PartCloudLoader(ds, 2, index=[0])
    with pytest.raises(ValueError, match="batch_size"):
        data.PartCloudLoader(ds, 4)


def test_bad_label_count_raises_value_error_naming_the_count(L):
    """The count the native routine reports goes through the layer's deferred check: ValueError naming it."""
    import torch
    from difffacto_amd import data
    rng = np.random.default_rng(7)
    ds, clouds = _cpu_set(rng, labels_ok=False)
    pts, seg = clouds[1]
    choice = np.arange(64, dtype=np.int32)[None]
    rc, o = bc.host_batch_raw(L, pts, seg, [0, len(pts)], [0], choice, np.zeros((1, 4)), np.zeros((1, 6)), 4, 64, 1, 5, bc.DEFAULT_CFG)
    assert rc == 0 and o["n_bad"].tolist() == [5, 0]
    with pytest.raises(ValueError, match=r"5 sampled label\(s\) outside \[0,4\)"):
        data.BatchCheck(torch.from_numpy(o["n_bad"]), 4).raise_if_bad()
    with pytest.raises(IndexError, match="2 item"):
        data.BatchCheck(torch.tensor([0, 2], dtype=torch.int32), 4).raise_if_bad()
    data.BatchCheck(torch.zeros(2, dtype=torch.int32), 4).raise_if_bad()


def test_loader_order_and_sample_ids_are_replayable():
    from difffacto_amd import data
    rng = np.random.default_rng(8)
    ds, _ = _cpu_set(rng)
    a, b = data.PartCloudLoader(ds, 2, seed=11), data.PartCloudLoader(ds, 2, seed=11)
    assert len(a) == 1 and len(data.PartCloudLoader(ds, 2, drop_last=False)) == 2
    assert np.array_equal(a.order(0), b.order(0)) and sorted(a.order(3).tolist()) == [0, 1, 2]
    assert any(not np.array_equal(a.order(0), a.order(e)) for e in range(1, 6))
    assert data.PartCloudLoader(ds, 2, shuffle=False).order(5).tolist() == [0, 1, 2]


def test_from_shapenet_dir_and_save_load(tmp_path):
    from difffacto_amd import data
    rng = np.random.default_rng(9)
    root = tmp_path / "shapenet"
    folder = root / data.SHAPENET_SYNSETS["Chair"]
    folder.mkdir(parents=True)
    (root / "train_test_split").mkdir()
    clouds = {}
    for token, m in (("bbb", 12), ("aaa", 7), ("ccc", 9)):
        xyz, lab = rng.uniform(-1, 1, (m, 3)), rng.integers(12, 16, m)
        rows = np.concatenate([xyz, rng.uniform(-1, 1, (m, 3)), lab[:, None].astype(np.float64)], 1)
        np.savetxt(folder / f"{token}.txt", rows, fmt="%.6f")
        clouds[token] = (np.loadtxt(folder / f"{token}.txt").astype(np.float32)[:, :3], lab - 12)
    for split, tokens in (("train", ["bbb", "aaa"]), ("val", ["ccc"]), ("test", [])):
        with open(root / "train_test_split" / f"shuffled_{split}_file_list.json", "w") as f:
            json.dump([f"shape_data/{data.SHAPENET_SYNSETS['Chair']}/{t}" for t in tokens], f)
    ds = data.PartCloudSet.from_shapenet_dir(str(root), "Chair", "train", device="cpu")
    assert ds.tokens == ["aaa", "bbb"] and ds.n_class == 4 and ds.class_id == 4 and ds.offsets.tolist() == [0, 7, 19]
    assert np.array_equal(ds.points.numpy(), np.concatenate([clouds["aaa"][0], clouds["bbb"][0]]))
    assert np.array_equal(ds.labels.numpy(), np.concatenate([clouds["aaa"][1], clouds["bbb"][1]]))
    assert data.PartCloudSet.from_shapenet_dir(str(root), "Chair", "trainval", device="cpu").tokens == ["aaa", "bbb", "ccc"]
    assert data.PartCloudSet.from_shapenet_dir(str(root), "Chair", "val", device="cpu").tokens == ["ccc"]
    with pytest.raises(ValueError, match="no file"):
        data.PartCloudSet.from_shapenet_dir(str(root), "Chair", "test", device="cpu")
    path = str(tmp_path / "set.npz")
    ds.save(path)
    back = data.PartCloudSet.load(path, device="cpu")
    assert back.tokens == ds.tokens and back.n_class == 4 and back.class_id == 4
    for x, y in zip(back.host, ds.host):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_batch_golden_manifest():
    sys.path.insert(0, os.path.join(bc.ROOT, "tests", "golden"))
    import manifest
    want = {}
    for line in open(os.path.join(bc.BATCH, "MANIFEST.sha256")):
        if line.strip() and not line.startswith("#"):
            h, name = line.split()
            want[name] = h
    files = sorted(os.listdir(bc.BATCH))
    assert all(f.endswith(".npz") or f == "MANIFEST.sha256" for f in files), files
    have = {f: manifest.content_hash(os.path.join(bc.BATCH, f)) for f in files if f.endswith(".npz")}
    assert want == have
    assert sum(os.path.getsize(os.path.join(bc.BATCH, f)) for f in files) < 400 * 1024
