"""Shared pieces of the batch-assembly tests (test_batch_cpu.py, test_gpu_batch.py), of tests/golden/make_golden_batch.py and of
tools/bench_batch.py: the recorded reference items of tests/golden/batch/, a numpy restatement of one training item
(``item_numpy``: pure float64 by default, with no intermediate rounding and the written zero-std rule; with ``dtype=np.float32``
the per-item loop a numpy loader would run, which the bench tool times on one core), the host twin's ctypes call and the error
gates the two test files share."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = os.path.join(ROOT, "tests", "golden", "batch")
PARITY_FILE = os.path.join(ROOT, "profiles", "batch_parity.txt")
PARITY_HEAD = ("# E_ref = max |reference - float64 restatement|, E_nat = max |native - float64 restatement| per fixture and float family;",
               "# gate: E_nat <= 2 E_ref + one float32 ulp of the family's largest magnitude.  Written by the tests themselves:",
               "# the `host` rows by tests/test_batch_cpu.py (the host twin), the `gpu` rows by tests/test_gpu_batch.py (an MI355X).")
FAMILIES = ("ref", "input", "shift", "scale", "part_shift", "part_scale")
EXACT = ("seg_mask", "attn_map", "present", "dp_present")
MODES = {None: 0, "none": 0, "shape_unit": 1, "shape_half": 2, "shape_34": 3, "shape_bbox": 4, "shape_canonical": 5,
         "shape_canonical_bbox": 6}
DEFAULT_CFG = dict(scale_mode="shape_unit", part_scale_mode="shape_canonical", clip=False, dropout_part=0.0, augment_shift=False,
                   augment_scale=False)


def case_names():
    return sorted(f[:-4] for f in os.listdir(BATCH) if f.endswith(".npz"))


def load_case(name):
    with np.load(os.path.join(BATCH, name + ".npz")) as z:
        d = {k: z[k] for k in z.files}
    cfg = dict(scale_mode=str(d.pop("scale_mode")), part_scale_mode=str(d.pop("part_scale_mode")), clip=bool(d.pop("clip")),
               dropout_part=float(d.pop("dropout_part")), augment_shift=bool(d.pop("augment_shift")),
               augment_scale=bool(d.pop("augment_scale")))
    return d, cfg, int(d.pop("n_class"))


# ---- the numpy restatement ----
def _pc_norm(pc, mode, clip, dt):
    one = dt(1.0)
    if mode in ("shape_unit", "shape_half", "shape_34"):
        shift = pc.mean(0)
        scale = np.full(3, pc.reshape(-1).std() / dt({"shape_unit": 1.0, "shape_half": 0.5, "shape_34": 0.75}[mode]), dt)
    elif mode == "shape_bbox":
        shift = (pc.min(0) + pc.max(0)) / dt(2)
        scale = np.full(3, (pc.max(0) - pc.min(0)).max() / dt(2), dt)
    elif mode in ("shape_canonical", "shape_canonical_bbox"):
        if mode == "shape_canonical":
            shift, scale = pc.mean(0), np.where(pc.max(0) == pc.min(0), dt(0), pc.std(0))   # the std of equal values is zero
        else:
            shift, scale = (pc.min(0) + pc.max(0)) / dt(2), (pc.max(0) - pc.min(0)) / dt(2)
        if clip:
            scale = np.clip(scale, dt(1e-2), one)
        scale = np.where(scale == 0, one, scale)
    elif mode in (None, "none"):
        shift, scale = np.zeros(3, dt), np.ones(3, dt)
    else:
        raise ValueError(mode)
    return ((pc - shift) / scale).astype(dt), shift.astype(dt), scale.astype(dt)


def item_numpy(points, labels, choice, drop_u, aug_u, n_class, cfg, dtype=np.float64, info=None):
    """One item from the planted draws.  Arrays as the collated item holds them: part_shift / part_scale (3,C), shift (1,3),
    scale (1,1) or, with an augmentation, (1,3).  ``info`` (a dict) receives the per-axis std of every part that had 10 points."""
    dt = dtype
    C = n_class
    choice = np.asarray(choice, np.int64)
    pts = np.asarray(points, np.float32)[choice].astype(dt)
    seg = np.asarray(labels, np.int64)[choice].copy()
    ref, shift, scale = _pc_norm(pts, cfg["scale_mode"], False, dt)
    out = np.zeros_like(ref)
    shifts, scales, present = np.zeros((C, 3), dt), np.ones((C, 3), dt), np.zeros(C, np.float32)
    for i in range(C):
        idx = seg == i
        if idx.sum() >= 10:
            part = ref[idx]
            std = part.astype(np.float64).std(0) if dt is np.float64 else part.std(0)
            flat = bool(np.any(part.max(0) == part.min(0)))    # the written rule: an axis std of exactly zero = all values equal
            present[i] = 0.0 if flat else 1.0
            if info is not None:
                info.setdefault("part_std", {})[i] = std
            out[idx], shifts[i], scales[i] = _pc_norm(part, cfg["part_scale_mode"], cfg["clip"], dt)
        elif idx.any():
            part, rest, rest_seg = ref[idx], ref[~idx], seg[~idx]
            d = part[:, None] - rest[None]
            dist = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            seg[idx] = rest_seg[dist.argmin(1)]
    dp_present = present.copy()
    dp_present[np.asarray(drop_u, np.float64) < cfg["dropout_part"]] = 0.0
    scale = scale[:1]
    if cfg["augment_shift"] or cfg["augment_scale"]:
        u = np.asarray(aug_u, np.float32).astype(dt)
        rs = u[0:3] / dt(2) + dt(np.float32(0.7)) if cfg["augment_scale"] else np.ones(3, dt)
        rt = u[3:6] - dt(0.5) if cfg["augment_shift"] else np.zeros(3, dt)
        ref = (ref + rt) * rs
        shift = shift + scale * rt
        scale = rs * scale
    return {"ref": ref, "input": out, "seg_mask": seg, "attn_map": (seg[:, None] == np.arange(C)[None]).astype(np.int64),
            "present": present, "dp_present": dp_present, "part_shift": shifts.T.copy(), "part_scale": scales.T.copy(),
            "shift": shift.reshape(1, 3), "scale": scale.reshape(1, -1)}


# ---- the host twin ----
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_batch_raw(L, points, labels, offsets, index, choice, drop_u, aug_u, n_class, npoints, scale_code, part_code, cfg):
    """dfx_debug_batch_build_host on a ragged host set -> (rc, dict of batched arrays incl. n_bad)."""
    points = np.ascontiguousarray(points, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    index = np.ascontiguousarray(index, np.int64)
    B, N, C = len(index), int(npoints), int(n_class)
    Bs, Ns, Cs = max(B, 1), max(N, 1), max(C, 1)
    choice = np.ascontiguousarray(choice, np.int32)
    drop_u, aug_u = np.ascontiguousarray(drop_u, np.float32), np.ascontiguousarray(aug_u, np.float32)
    o = {"ref": np.zeros((Bs, Ns, 3), np.float32), "input": np.zeros((Bs, Ns, 3), np.float32), "seg_mask": np.zeros((Bs, Ns), np.int64),
         "attn_map": np.zeros((Bs, Ns, Cs), np.int64), "present": np.zeros((Bs, Cs), np.float32), "dp_present": np.zeros((Bs, Cs), np.float32),
         "part_shift": np.zeros((Bs, 3, Cs), np.float32), "part_scale": np.zeros((Bs, 3, Cs), np.float32),
         "shift": np.zeros((Bs, 1, 3), np.float32), "scale": np.zeros((Bs, 1, 3), np.float32), "n_bad": np.zeros(2, np.int32)}
    rc = L.dfx_debug_batch_build_host(_p(points), _p(labels), _p(offsets), len(offsets) - 1, _p(index), B, _p(choice), _p(drop_u), _p(aug_u),
                                      C, N, scale_code, part_code, int(cfg["clip"]), float(cfg["dropout_part"]),
                                      int(cfg["augment_shift"]), int(cfg["augment_scale"]), *[_p(o[k]) for k in (
                                          "ref", "input", "seg_mask", "attn_map", "present", "dp_present", "part_shift", "part_scale",
                                          "shift", "scale", "n_bad")])
    if not (cfg["augment_shift"] or cfg["augment_scale"]):
        o["scale"] = o["scale"][:, :, :1]
    return rc, o


def host_item(L, points, labels, choice, drop_u, aug_u, n_class, cfg):
    """One item of one cloud through the host twin -> the item's arrays (no batch axis)."""
    rc, o = host_batch_raw(L, points, labels, [0, len(points)], [0], np.asarray(choice)[None], np.asarray(drop_u)[None],
                           np.asarray(aug_u)[None], n_class, len(choice), MODES[cfg["scale_mode"]], MODES[cfg["part_scale_mode"]], cfg)
    assert rc == 0, (L.dfx_last_error() or b"").decode()
    assert not o["n_bad"].any(), o["n_bad"]
    return {k: v[0] for k, v in o.items() if k != "n_bad"}


# ---- gates ----
def check_exact(got, want, what):
    """seg, attn_map, present, dp_present and the set of all-zero input rows are EQUAL."""
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]).astype(np.float64), np.asarray(want[k]).astype(np.float64)), (what, k)
    zg, zw = (np.asarray(got["input"]) == 0).all(-1), (np.asarray(want["input"]) == 0).all(-1)
    assert np.array_equal(zg, zw), (what, "all-zero input rows", int(zg.sum()), int(zw.sum()))


def family_errors(got, f64):
    """max |got - float64 restatement| per float family, and one float32 ulp of the family's largest magnitude."""
    out = {}
    for k in FAMILIES:
        g, w = np.asarray(got[k], np.float64), np.asarray(f64[k], np.float64)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        out[k] = (float(np.abs(g - w).max()), float(np.spacing(np.float32(np.abs(w).max()))))
    return out


def gate_lines(name, e_ref, e_nat):
    """(lines of the parity table, list of families that miss E_nat <= 2 E_ref + ulp)."""
    lines, missed = [], []
    for k in FAMILIES:
        bound = 2.0 * e_ref[k][0] + e_ref[k][1]
        ok = e_nat[k][0] <= bound
        lines.append(f"{name:<22}{k:<11}E_ref {e_ref[k][0]:.3e}  E_nat {e_nat[k][0]:.3e}  ulp {e_ref[k][1]:.3e}  bound {bound:.3e}  {'ok' if ok else 'MISS'}")
        if not ok:
            missed.append(k)
    return lines, missed


def write_parity(who, table):
    """Replace the rows of `who` ("host" / "gpu") in profiles/batch_parity.txt by `table` ({fixture: lines of gate_lines}); the
    other rows stay.  Only a complete table (every fixture) is written, so a run of a few selected cases leaves the file alone."""
    if sorted(table) != case_names():
        return False
    keep = []
    if os.path.exists(PARITY_FILE):
        keep = [l.rstrip("\n") for l in open(PARITY_FILE) if not l.startswith("#") and l.strip() and not l.startswith(f"{who:<5}")]
    rows = sorted(keep + [f"{who:<5}{line}" for name in sorted(table) for line in table[name]], key=lambda l: (l[:5] != "host ", l[:27]))
    misses = sum(l.rstrip().endswith("MISS") for l in rows)
    with open(PARITY_FILE, "w") as f:
        f.write("\n".join(list(PARITY_HEAD) + rows + [f"# {len(rows)} rows, {misses} miss(es)"]) + "\n")
    return True


def stage1_modules():
    """The stage-1 model of configs/train_chair_stage1.py as examples/train_stage1.py builds it (no dropout, T = 100, fp32 products)."""
    from difffacto_amd.encoders import PartEncoderForTransformerDecoder
    from difffacto_amd.modules import AnchoredDiffusion
    enc = PartEncoderForTransformerDecoder(encoder=dict(type="PointNetV2", zdim=256, per_part_mlp=True), n_class=4, part_aligner=None,
                                           include_z=False, include_part_code=True, include_params=True, use_gt_params=True, kl_weight=5e-4,
                                           use_flow=True, latent_flow_depth=14, latent_flow_hidden_dim=256, gen=True, prior_var=1.0)
    net = dict(type='TransformerNet', in_channels=3, out_channels=3, n_heads=8, d_head=16, depth=5, dropout=0.0, context_dim=256 + 6,
               n_class=4, class_cond=True, use_linear=True, cat_params_to_x=True, use_checkpoint=False, single_attn=True, cat_class_to_x=True)
    diff = AnchoredDiffusion(net=net, num_timesteps=100, beta_1=1e-4, beta_T=.02, k=1.0, res=False, mode='linear', use_beta=False,
                             rescale_timesteps=False, model_mean_type="epsilon", learn_variance=True, loss_type='mse', include_anchors=False,
                             precision="f32")
    return enc.cuda().train(), diff.cuda().train()


# ---- synthetic clouds (tests without a reference fixture, the toy set, the bench tool) ----
def box_cloud(rng, n_class, counts, spread=1.0):
    """Labelled boxes: part k = counts[k] points uniform in a box of its own size and place."""
    pts, seg = [], []
    for k in range(n_class):
        if counts[k] == 0:
            continue
        centre = spread * rng.uniform(-1, 1, 3)
        half = rng.uniform(0.05, 0.4, 3)
        pts.append(centre + half * rng.uniform(-1, 1, (counts[k], 3)))
        seg.append(np.full(counts[k], k, np.int32))
    order = rng.permutation(sum(len(p) for p in pts))
    return np.concatenate(pts).astype(np.float32)[order], np.concatenate(seg)[order]
