#!/usr/bin/env python
"""Golden vectors of the reference's training item (dev container only; the reference's own ``_ShapeNetSegParts.__getitem__`` on CPU).

    python tests/golden/make_golden_batch.py

Written to tests/golden/batch/ with their own MANIFEST.sha256 (manifest.content_hash).

The data set object is made with ``object.__new__`` (no files are read), its attributes are set and ``cache`` is pre-filled with an
in-memory cloud, so ``__getitem__`` runs unmodified.  During the call ``np.random.choice`` / ``np.random.rand`` / ``torch.rand``
return planted arrays, which are recorded: ``choice`` (N) int32, ``drop_u`` (C) float32-representable, ``aug_u`` (6) float32
([0:3] the scale draw, [3:6] the shift draw).  Each case file holds the cloud (points, labels), the draws, the configuration and
the item's arrays (part_shift / part_scale as the item returns them: (3,C)).

The generator asserts the conditions under which the reference's discrete decisions are stable, so that the reference alone
decides each case: every part that is normalised has a std of at least 1e-3 on every axis (no flat part), unclipped part scales
are at least 1 % away from 1e-2 and 1 where clip is on, drop_u is at least 1e-3 away from dropout_part; and that each case holds
what it is named after.
"""
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "batch")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import manifest  # noqa: E402
import ref_import  # noqa: E402
import _batch_case as bc  # noqa: E402

SEED = 20261018
C = 4
# the four boxes of a chair-like shape: (centre, half extent)
BASE = [((0.0, 0.0, 0.0), (0.4, 0.05, 0.4)), ((0.0, 0.45, -0.35), (0.4, 0.4, 0.05)), ((0.0, -0.4, 0.0), (0.35, 0.35, 0.35)),
        ((0.5, 0.2, 0.0), (0.05, 0.15, 0.3))]
A = dict(bc.DEFAULT_CFG)
B = dict(A, scale_mode="shape_bbox", part_scale_mode="shape_canonical_bbox", clip=True)
CLIP = dict(A, clip=True)


def blob(label, m, n, centre=None, half=None):
    """m points of part `label` in the cloud, n of the item's samples drawn from them (with replacement)."""
    c, h = BASE[label] if centre is None else (centre, half)
    return dict(label=label, m=m, n=n, centre=np.asarray(c, np.float64), half=np.asarray(h, np.float64))


def build(rng, blobs):
    pts, seg, choice, first = [], [], [], 0
    for b in blobs:
        pts.append(b["centre"] + b["half"] * rng.uniform(-1, 1, (b["m"], 3)))
        seg.append(np.full(b["m"], b["label"], np.int64))
        pick = rng.integers(0, b["m"], b["n"])
        if b["n"] >= b["m"]:
            pick[:b["m"]] = np.arange(b["m"])        # every point at least once
        choice.append(first + pick)
        first += b["m"]
    order = rng.permutation(first)                    # the cloud's own order is mixed, and so is the order of the samples
    inv = np.argsort(order)
    pts, seg = np.concatenate(pts).astype(np.float32)[order], np.concatenate(seg)[order]
    choice = inv[np.concatenate(choice)]
    return pts, seg, choice[rng.permutation(len(choice))].astype(np.int32)


def cases(rng):
    u = lambda n: rng.uniform(0, 1, n).astype(np.float32)
    even = [blob(k, 100, 64) for k in range(4)]
    yield "small_cloud", A, [blob(0, 10, 70), blob(1, 10, 60), blob(2, 10, 60), blob(3, 10, 60)], None, None
    yield "large_cloud", A, even, None, None
    yield "nine_and_ten", A, [blob(0, 150, 137), blob(1, 30, 9), blob(2, 30, 10), blob(3, 100, 100)], None, None
    yield "into_earlier", A, [blob(0, 120, 120), blob(1, 100, 100), blob(2, 3, 3, (0.1, 0.0, 0.1), (0.01, 0.01, 0.01)), blob(3, 40, 33)], None, None
    yield "into_later_lift", A, [blob(0, 1, 1, (0.0, -0.6, 0.0), (0.0, 0.0, 0.0)), blob(1, 150, 146), blob(2, 9, 9), blob(3, 100, 100)], None, None
    yield "chain", A, [blob(0, 2, 2, (0.8, 0.8, 0.8), (0.01, 0.01, 0.01)), blob(1, 3, 3, (0.8, 0.8, 0.75), (0.01, 0.01, 0.01)),
                       blob(2, 160, 151), blob(3, 100, 100)], None, None
    yield "absent_part", A, [blob(0, 90, 96), blob(1, 80, 77), blob(2, 80, 77)], None, None
    yield "one_part", A, [blob(1, 60, 250)], None, None
    yield "dropout", dict(A, dropout_part=0.5), even, np.asarray([0.1, 0.9, 0.3, 0.7], np.float32), None
    yield "augment_both", dict(A, augment_shift=True, augment_scale=True), even, None, u(6)
    yield "augment_shift", dict(A, augment_shift=True), even, None, u(6)
    yield "augment_scale", dict(A, augment_scale=True), even, None, u(6)
    thin = blob(0, 100, 64, (0.0, 0.0, 0.0), (0.4, 0.004, 0.4))
    yield "bbox_clip", B, [thin, blob(1, 100, 64), blob(2, 100, 64), blob(3, 100, 64)], None, None
    yield "bbox_clip_small", dict(B, dropout_part=0.5), [blob(0, 10, 70, (0.0, 0.0, 0.0), (0.4, 0.004, 0.4)), blob(1, 10, 60), blob(2, 10, 60), blob(3, 10, 60)], np.asarray([0.25, 0.75, 0.6, 0.1], np.float32), None
    long_part = blob(2, 100, 64, (0.0, -0.4, 0.0), (2.0, 0.05, 0.05))
    yield "unit_clip", CLIP, [blob(0, 100, 64, (0.0, 0.0, 0.0), (0.4, 0.003, 0.4)), blob(1, 100, 64), long_part, blob(3, 100, 64)], None, None
    yield "n2048", dict(A, dropout_part=0.5, augment_shift=True, augment_scale=True), even_n(2048), np.asarray([0.75, 0.25, 0.6, 0.4], np.float32), u(6)


def even_n(n):
    return [blob(k, 100, n // 4) for k in range(4)]


def reference_item(ds_cls, torch, pts, seg, choice, drop_u, aug_u, cfg, n_class):
    ds = object.__new__(ds_cls)
    ds.cache = {0: (pts, np.array([4]).astype(np.int32), seg.astype(np.int64), "fixture")}
    ds.noises, ds.num_class, ds.npoints = {}, n_class, len(choice)
    ds.scale_mode, ds.part_scale_mode, ds.clip = cfg["scale_mode"], cfg["part_scale_mode"], cfg["clip"]
    ds.dropout_part, ds.augment_shift, ds.augment_scale = cfg["dropout_part"], cfg["augment_shift"], cfg["augment_scale"]
    planted = ([aug_u[0:3]] if cfg["augment_scale"] else []) + ([aug_u[3:6]] if cfg["augment_shift"] else [])
    calls = {"choice": 0, "rand": 0}

    def fake_choice(m, n, replace=True):
        assert m == len(pts) and n == len(choice) and replace
        calls["choice"] += 1
        return choice.astype(np.int64)

    def fake_rand(n):
        assert n == n_class
        calls["rand"] += 1
        return drop_u.astype(np.float64)

    def fake_torch_rand(*shape):
        assert shape == (1, 3)
        return torch.from_numpy(planted.pop(0).astype(np.float32).reshape(1, 3).copy())

    with mock.patch.object(np.random, "choice", fake_choice), mock.patch.object(np.random, "rand", fake_rand), \
            mock.patch.object(torch, "rand", fake_torch_rand):
        item = ds[0]
    assert calls == {"choice": 1, "rand": 1} and not planted
    assert item["attn_map"] is item["ref_attn_map"] and item["seg_mask"] is item["ref_seg_mask"]
    return {"ref": item["ref"].numpy(), "input": item["input"].numpy(), "seg_mask": np.asarray(item["seg_mask"], np.int64),
            "attn_map": item["attn_map"].numpy(), "present": item["present"].numpy(), "dp_present": item["dp_present"].numpy(),
            "part_shift": np.ascontiguousarray(item["part_shift"].numpy()), "part_scale": np.ascontiguousarray(item["part_scale"].numpy()),
            "shift": item["shift"].numpy(), "scale": item["scale"].numpy()}


def main():
    ref_import.import_reference()
    import torch
    from difffacto.datasets.shapenet_seg import _ShapeNetSegParts
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(SEED)
    for name, cfg, blobs, drop_u, aug_u in cases(rng):
        pts, seg, choice = build(rng, blobs)
        drop_u = rng.uniform(0, 1, C).astype(np.float32) if drop_u is None else drop_u
        aug_u = np.zeros(6, np.float32) if aug_u is None else aug_u
        got = reference_item(_ShapeNetSegParts, torch, pts, seg, choice, drop_u, aug_u, cfg, C)
        assert all(v.dtype in (np.float32, np.int64) for v in got.values()), {k: v.dtype for k, v in got.items()}

        # the conditions under which the reference's discrete decisions are stable
        info = {}
        f64 = bc.item_numpy(pts, seg, choice, drop_u, aug_u, C, cfg, info=info)
        for k in bc.EXACT:
            assert np.array_equal(got[k].astype(np.float64), f64[k].astype(np.float64)), (name, k)
        for i, std in info.get("part_std", {}).items():
            assert std.min() >= 1e-3, (name, i, std)
        if cfg["clip"]:
            raw = bc.item_numpy(pts, seg, choice, drop_u, aug_u, C, dict(cfg, clip=False))["part_scale"][:, sorted(info["part_std"])]
            assert np.all(np.abs(raw / 1e-2 - 1) >= 0.01) and np.all(np.abs(raw - 1) >= 0.01), (name, raw)
            sides = (bool((raw < 1e-2).any()), bool((raw > 1e-2).any()), bool((raw < 1).any()), bool((raw > 1).any()))
            print(f"  {name}: unclipped part scales below/above 1e-2: {sides[0]}/{sides[1]}, below/above 1: {sides[2]}/{sides[3]}")
            assert sides[0] and sides[1] and sides[2] and (sides[3] or cfg["scale_mode"] == "shape_bbox"), (name, sides)
        assert np.all(np.abs(drop_u.astype(np.float64) - cfg["dropout_part"]) >= 1e-3)

        # what the case is named after
        n, M = len(choice), len(pts)
        sampled = np.bincount(seg[choice], minlength=C)
        final = np.bincount(got["seg_mask"], minlength=C)
        zero_rows = int((got["input"] == 0).all(-1).sum())
        assert len(np.unique(choice)) < n, name                                         # duplicated points
        if name == "small_cloud":
            assert M < n
        if name == "large_cloud":
            assert M > n
        if name == "nine_and_ten":
            assert sampled[1] == 9 and sampled[2] == 10 and got["present"][1] == 0 and got["present"][2] == 1 and final[1] == 0
        if name == "into_earlier":
            assert sampled[2] == 3 and final[0] == sampled[0] + 3 and zero_rows == 3 and got["present"][2] == 0
        if name == "into_later_lift":
            assert sampled[0] == 1 and sampled[2] == 9 and final[2] == 10 and got["present"][2] == 1 and zero_rows == 0
        if name == "chain":
            assert sampled[0] == 2 and sampled[1] == 3 and final[0] == 0 and final[1] == 0 and final.sum() == n
            assert sorted(got["present"].tolist()) == [0, 0, 1, 1]
        if name == "absent_part":
            assert sampled[3] == 0 and got["present"].tolist() == [1, 1, 1, 0]
        if name == "one_part":
            assert got["present"].tolist() == [0, 1, 0, 0]
        if cfg["dropout_part"] > 0:
            dropped = drop_u < cfg["dropout_part"]
            assert dropped.any() and (~dropped).any() and np.array_equal(got["dp_present"], np.where(dropped, 0, got["present"]))
            assert (got["present"][dropped] == 1).any()
        assert got["scale"].shape == ((1, 3) if cfg["augment_shift"] or cfg["augment_scale"] else (1, 1)), got["scale"].shape

        np.savez_compressed(os.path.join(OUT, name + ".npz"), points=pts, labels=seg.astype(np.int32), choice=choice, drop_u=drop_u,
                            aug_u=aug_u, n_class=np.int64(C), scale_mode=np.asarray(cfg["scale_mode"]),
                            part_scale_mode=np.asarray(cfg["part_scale_mode"]), clip=np.asarray(cfg["clip"]),
                            dropout_part=np.float64(cfg["dropout_part"]), augment_shift=np.asarray(cfg["augment_shift"]),
                            augment_scale=np.asarray(cfg["augment_scale"]), **got)
        print(f"{name}: M {M} N {n} sampled {sampled.tolist()} final {final.tolist()} present {got['present'].tolist()} zero rows {zero_rows}")

    with open(os.path.join(OUT, "MANIFEST.sha256"), "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    total = 0
    for fn in sorted(os.listdir(OUT)):
        total += os.path.getsize(os.path.join(OUT, fn))
        print(fn, os.path.getsize(os.path.join(OUT, fn)))
    print("total", total)


if __name__ == "__main__":
    main()
