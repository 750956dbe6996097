"""CPU checks behind tests/test_gpu_latent_configs.py: the configurations of tests/_latent_cfg.py beyond the shipped one.

* synth.make_latent_weights keeps its bits for the default arguments;
* the fp32 numpy oracle (oracle/latents.py, now with `heads` and `cimle=False`), its float64 restatement (oracle/latents_highprec.py)
  and the torch restatement `_aligner_torch` agree with the reference's goldens (tests/golden/latentcfg/) and with each other, forward
  and gradients, at the existing gates (1e-4 x max(1, |ref|) for outputs, 5e-4 of max-abs for gradients); the gaps are printed;
* the entry points' argument checks reject what they should and accept every named configuration, before any HIP call;
* the acceptance functions of the GPU file, at its recorded factors F and FG, reject six deliberately wrong variants of the restatement.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import _latent_cfg as lc
from difffacto_amd import synth
from oracle import latents as ol
from oracle import latents_highprec as oh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "latentcfg")
GOLDEN_TAGS = ("tiny", "wide", "one", "plain")
OUT_TOL, G_RTOL, G_ATOL = 1e-4, 5e-4, 1e-7


# ---------------------------------------------------------------------------------------------------- synth
def _latent_param_shapes_before(n_class=4, flow_depth=14, flow_hidden=256, depth=5, heads=8, d_head=32, noise_dim=32):
    """synth.latent_param_shapes as it was before it took `zdim` (the module constant 256 throughout)."""
    s, Z = [], 256
    half = Z - Z // 2
    for i in range(n_class):
        for l in range(flow_depth):
            p = f"flow.{i}.chain.{l}.net_s_t."
            s += [(p + "0.weight", (flow_hidden, half)), (p + "0.bias", (flow_hidden,)), (p + "2.weight", (flow_hidden, flow_hidden)),
                  (p + "2.bias", (flow_hidden,)), (p + "4.weight", ((Z - half) * 2, flow_hidden)), (p + "4.bias", ((Z - half) * 2,))]
    inner, P = heads * d_head, "part_aligner."
    s += [(P + "class_emb.weight", (n_class, inner)), (P + "pre_norm.weight", (inner,)), (P + "pre_norm.bias", (inner,)),
          (P + "post_norm.weight", (inner,)), (P + "post_norm.bias", (inner,)), (P + "proj_in.weight", (inner, Z + noise_dim)), (P + "proj_in.bias", (inner,))]
    for i in range(depth):
        p = f"{P}transformer_blocks.{i}."
        s += [(p + "ff.net.0.proj.weight", (8 * inner, inner)), (p + "ff.net.0.proj.bias", (8 * inner,)), (p + "ff.net.2.weight", (inner, 4 * inner)),
              (p + "ff.net.2.bias", (inner,)), (p + "attn2.to_q.weight", (inner, inner)), (p + "attn2.to_k.weight", (inner, inner)),
              (p + "attn2.to_v.weight", (inner, inner)), (p + "attn2.to_out.0.weight", (inner, inner)), (p + "attn2.to_out.0.bias", (inner,)),
              (p + "norm2.weight", (inner,)), (p + "norm2.bias", (inner,)), (p + "norm3.weight", (inner,)), (p + "norm3.bias", (inner,))]
    return s + [(P + "proj_out.weight", (6, inner)), (P + "proj_out.bias", (6,))]


@pytest.mark.parametrize("seed", [0, 3])
def test_default_latent_weights_keep_their_bits(seed, monkeypatch):
    new, named = synth.make_latent_weights(seed), lc.weights("shipped", seed)
    assert synth.latent_param_shapes() == _latent_param_shapes_before()
    monkeypatch.setattr(synth, "latent_param_shapes", _latent_param_shapes_before)
    old = synth.make_latent_weights(seed)
    assert list(old) == list(new) and all(old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]) for k in old)
    assert list(named) == list(new) and all(np.array_equal(v, new[k]) for k, v in named.items())


def test_every_named_configuration_has_weights_of_its_sizes():
    for tag, cfg in lc.CONFIGS.items():
        W = lc.weights(tag)
        inner, Z = cfg["heads"] * cfg["d_head"], cfg["zdim"]
        assert W["part_aligner.proj_in.weight"].shape == (inner, Z + cfg["noise_dim"]) and W["part_aligner.class_emb.weight"].shape == (cfg["n_class"], inner)
        assert ol.flow_depth(W) == cfg["flow_depth"] and ol.aligner_depth(W) == cfg["depth"]
        if cfg["flow_depth"]:
            assert W["flow.0.chain.0.net_s_t.0.weight"].shape == (cfg["flow_hidden"], Z // 2)
            assert f"flow.{cfg['n_class'] - 1}.chain.{cfg['flow_depth'] - 1}.net_s_t.4.bias" in W
        else:
            assert not any(k.startswith("flow.") for k in W)
    assert lc.CONFIGS["plain"]["depth"] == lc.MAX_DEPTH


# ---------------------------------------------------------------------------------------------------- the restatements and the goldens
def _close(got, ref, what):
    err, scale = float(np.abs(np.asarray(got, np.float64) - ref).max()), max(1.0, float(np.abs(ref).max()))
    assert err <= OUT_TOL * scale, (what, err, scale)
    return err


def _grad_close(got, ref, what):
    err, scale = float(np.abs(np.asarray(got, np.float64) - ref).max()), float(np.abs(ref).max())
    assert err <= G_ATOL + G_RTOL * scale, (what, err, scale)
    return err / scale if scale else 0.0


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
def test_restatements_agree_with_the_reference_and_each_other(tag):
    cfg, g, Wn = lc.CONFIGS[tag], np.load(os.path.join(GOLD, f"{tag}.npz")), lc.weights(tag)
    W64 = oh.widen(Wn)
    K, npoints, J = int(g["K"]), int(g["npoints"]), cfg["n_class"]
    kw = dict(noise_scale=lc.NOISE_SCALE, heads=cfg["heads"], cimle=cfg["cimle"])
    for pattern in lc.VALID_PATTERNS:
        pre = pattern + "/"
        x = {k: (g[pre + "in/" + k] if pre + "in/" + k in g.files else None) for k in ("w_noise", "noise", "valid", "code", "d_mean", "d_logvar")}
        again = lc.inputs(tag, 5, K, 500 + lc.VALID_PATTERNS.index(pattern), pattern)
        assert all(np.array_equal(x[k], again[k]) for k in x if x[k] is not None), "the fixture's inputs are the helper's"
        o32 = ol.sample_latents(Wn, x["w_noise"], x["noise"], x["valid"], np.zeros(J), K, npoints, **kw)
        o64 = oh.sample_latents(W64, x["w_noise"], x["noise"], x["valid"], np.zeros(J), K, npoints, **kw)
        assert np.array_equal(o32["seg_mask"], g[pre + "sl/seg_mask"]) and np.array_equal(o32["valid_id"], g[pre + "sl/valid_id"])
        assert np.array_equal(o64["seg_mask"], o32["seg_mask"]) and np.array_equal(o64["valid_id"], o32["valid_id"])
        gaps = {}
        for k in ("part_code", "mean", "logvar", "mean_per_point", "logvar_per_point"):
            ref = g[pre + "sl/" + k].astype(np.float64)
            gaps[k] = (_close(o32[k], ref, (tag, pattern, k, "fp32")), _close(o64[k], ref, (tag, pattern, k, "f64")))
            assert o32[k].dtype == np.float32 and o64[k].dtype == np.float64
        _close(o32["ctx"][1], g[pre + "sl/ctx1"].astype(np.float64), "ctx1")
        _close(o64["params"], g[pre + "sl/ctx1"].astype(np.float64), "params")
        # the aligner on a given code, forward and autograd
        code, valid = np.repeat(x["code"], K, axis=0), np.repeat(x["valid"], K, axis=0)
        m32, l32 = ol.part_aligner_forward(Wn, code, valid, x["noise"], **kw)
        m64, l64 = oh.part_aligner_forward(W64, code, valid, x["noise"], **kw)
        rm, rl = g[pre + "al/mean"].astype(np.float64), g[pre + "al/logvar"].astype(np.float64)
        gaps["al"] = (max(_close(m32, rm, "mean fp32"), _close(l32, rl, "logvar fp32")), max(_close(m64, rm, "mean f64"), _close(l64, rl, "logvar f64")))
        if cfg["cimle"]:
            import torch
            t64 = lc.autograd(Wn, tag, code, valid, x["noise"], x["d_mean"], x["d_logvar"], torch.float64)
            t32 = lc.autograd(Wn, tag, code, valid, x["noise"], x["d_mean"], x["d_logvar"], torch.float32)
            assert np.abs(t64["mean"] - m64).max() < 1e-12 * max(1, np.abs(m64).max()) and np.abs(t64["logvar"] - l64).max() < 1e-12 * max(1, np.abs(l64).max())
            _close(t32["mean"], rm, "torch fp32 mean"), _close(t32["logvar"], rl, "torch fp32 logvar")
            for k in ("d_part_code", "d_noise"):
                ref = g[pre + "al/" + k].astype(np.float64)
                gaps[k] = (_grad_close(t32[k], ref, (tag, pattern, k, "fp32")), _grad_close(t64[k], ref, (tag, pattern, k, "f64")))
            names = [k[len(pre + "al/grad/"):] for k in g.files if k.startswith(pre + "al/grad/")]
            assert bool(names) == (tag in ("tiny", "one") and pattern == "shape_all_absent")
            for n in names:
                _grad_close(t64["grads"][n], g[pre + "al/grad/" + n].astype(np.float64), (tag, n))
                _grad_close(t32["grads"][n], g[pre + "al/grad/" + n].astype(np.float64), (tag, n))
            assert not names or not any(n.startswith("pre_norm") for n in names)
        else:   # torch restatement of the cimle=False branch: forward only (the training path requires cimle)
            import torch
            with torch.no_grad():
                W = {k: torch.from_numpy(v).double() for k, v in Wn.items()}
                tm, tl = lc._aligner_torch(W, torch.from_numpy(code).double(), torch.from_numpy(valid).double(), None, heads=cfg["heads"], cimle=False)
            assert np.abs(tm.numpy() - m64).max() < 1e-12 * max(1, np.abs(m64).max()) and np.abs(tl.numpy() - l64).max() < 1e-12 * max(1, np.abs(l64).max())
        print(f"LATCFG-CPU {tag} {pattern}: |restatement - reference golden| (fp32, float64): " + ", ".join(f"{k} ({a:.1e}, {b:.1e})" for k, (a, b) in gaps.items()))


def test_the_fp32_oracle_defaults_are_the_shipped_configuration():
    W, x = lc.weights("shipped"), lc.inputs("shipped", 2, 1, 9)
    a = ol.part_aligner_forward(W, x["code"], x["valid"], x["noise"])
    b = ol.part_aligner_forward(W, x["code"], x["valid"], x["noise"], noise_scale=100.0, heads=8, cimle=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(AssertionError):
        ol.sample_latents(lc.weights("plain"), x["w_noise"], None, x["valid"], np.zeros(4), 2, 8, cimle=False)      # K must be 1


def test_latentcfg_fixture_manifest():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import manifest
    want = {}
    for ln in open(os.path.join(GOLD, "MANIFEST.sha256")):
        if ln.strip() and not ln.startswith("#"):
            h, name = ln.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(GOLD, f)) for f in sorted(os.listdir(GOLD)) if f.endswith(".npz")}
    assert want == have and set(have) == {t + ".npz" for t in GOLDEN_TAGS}
    assert all(os.path.getsize(os.path.join(GOLD, f)) < 1 << 20 for f in have)


# ---------------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _lw(cfg, **over):
    """dfx_latent_weights with the sizes of `cfg`, never-dereferenced top-level pointers and NULL block / flow weights: dfx_latents_create gets
    through every size check and stops at "null weight pointer", before its first HIP call."""
    from difffacto_amd import _ffi
    c = dict(cfg, **over)
    w = _ffi.LatentWeights()
    w.n_class, w.zdim, w.flow_depth, w.flow_hidden = c["n_class"], c["zdim"], c["flow_depth"], c["flow_hidden"]
    w.depth, w.n_heads, w.d_head, w.cimle, w.noise_dim, w.noise_scale, w.prior_var = c["depth"], c["heads"], c["d_head"], int(c["cimle"]), c["noise_dim"], 100.0, 1.0
    for f in ("proj_in_w", "proj_in_b", "class_emb", "pre_norm_w", "pre_norm_b", "post_norm_w", "post_norm_b", "proj_out_w", "proj_out_b"):
        setattr(w, f, 0x1000)
    keep = None
    if c["flow_depth"] > 0:
        keep = (_ffi.c_fp * (c["n_class"] * c["flow_depth"] * 6))()
        w.flow = ctypes.cast(keep, ctypes.POINTER(_ffi.c_fp))
    return w, keep


def _msg(lib):
    return lib.dfx_last_error().decode()


REJECTED = [("n_class", 0, "n_class"), ("n_class", 9, "n_class"), ("zdim", 40, "zdim"), ("d_head", 24, "d_head"), ("heads", 3, "inner dim 96"),
            ("heads", 34, "inner dim 1088"), ("noise_dim", 12, "noise_dim"), ("flow_hidden", 12, "flow"), ("depth", 0, "depth"),
            ("depth", lc.MAX_DEPTH + 1, "depth")]


def test_create_rejects_bad_sizes_and_accepts_every_named_configuration(lib):
    from difffacto_amd import _ffi
    assert lc.MAX_DEPTH == _ffi.DFX_MAX_DEPTH
    shipped = lc.CONFIGS["shipped"]
    for field, value, word in REJECTED:
        w, keep = _lw(shipped, **{field: value})
        h = ctypes.c_void_p()
        rc = lib.dfx_latents_create(ctypes.byref(h), ctypes.byref(w), None)
        assert rc != 0 and not h.value and word in _msg(lib) and "null weight pointer" not in _msg(lib), (field, value, _msg(lib))
    for tag, cfg in lc.CONFIGS.items():
        w, keep = _lw(cfg)
        h = ctypes.c_void_p()
        rc = lib.dfx_latents_create(ctypes.byref(h), ctypes.byref(w), None)
        assert rc != 0 and not h.value and _msg(lib).endswith("latents_create: null weight pointer"), (tag, _msg(lib))   # past every size check


def test_training_entry_points_reject_bad_sizes_and_accept_the_cimle_configurations(lib):
    p = 0x1000                       # never dereferenced: every call returns from its argument checks

    def calls(w, nbytes):
        return {"dfx_aligner_train_forward": lib.dfx_aligner_train_forward(w, p, nbytes, p, p, p, p, p, 2, None),
                "dfx_aligner_train_backward": lib.dfx_aligner_train_backward(w, p, nbytes, p, p, p, w, p, 2, None),
                "dfx_aligner_input_backward": lib.dfx_aligner_input_backward(w, p, nbytes, p, p, p, p, p, 2, None)}

    shipped = lc.CONFIGS["shipped"]
    for field, value, word in REJECTED:
        if field in ("zdim", "noise_dim", "flow_hidden"):      # sizes the exact-fp32 training kernels do not constrain
            continue
        w, _ = _lw(shipped, **{field: value})
        for name in ("dfx_aligner_train_forward", "dfx_aligner_train_backward", "dfx_aligner_input_backward"):
            rc = calls(w, 1 << 30)[name]
            assert rc != 0 and any(s in _msg(lib) for s in ("n_class", "d_head", "inner dim")) and "workspace" not in _msg(lib), (name, field, value, _msg(lib))
    for tag, cfg in lc.CONFIGS.items():
        w, _ = _lw(cfg)
        for name in ("dfx_aligner_train_forward", "dfx_aligner_train_backward", "dfx_aligner_input_backward"):
            rc = calls(w, 16)[name]
            want = "workspace too small" if cfg["cimle"] else "cIMLE"                                         # cimle = 0: rejected by all three
            assert rc != 0 and want in _msg(lib), (tag, name, _msg(lib))
        nb = lib.dfx_aligner_train_workspace_bytes(2, cfg["n_class"], cfg["zdim"], cfg["noise_dim"], cfg["heads"], cfg["d_head"], cfg["depth"])
        assert nb > 0


# ---------------------------------------------------------------------------------------------------- the acceptance functions reject wrong variants
def _forward_variant_ratio(tag, mutate, pattern="one_absent", B=5, K=2):
    """Worst ratio, over the float outputs of sample_latents, of |mutated float64 restatement - truth| to |fp32 oracle - truth|."""
    cfg, Wn = lc.CONFIGS[tag], lc.weights(tag)
    K = K if cfg["cimle"] else 1
    x, J = lc.inputs(tag, B, K, 40, pattern), cfg["n_class"]
    kw = dict(noise_scale=lc.NOISE_SCALE, heads=cfg["heads"], cimle=cfg["cimle"])
    args = (x["w_noise"], x["noise"], x["valid"], np.zeros(J), K, 2 * J)
    truth, o32 = oh.sample_latents(oh.widen(Wn), *args, **kw), ol.sample_latents(Wn, *args, **kw)
    bad = oh.sample_latents(oh.widen(Wn), *args, **kw, mutate=mutate)
    return max(lc.ratio(lc.err_stats(bad[k], truth[k]), lc.err_stats(o32[k], truth[k])) for k in ("part_code", "mean", "logvar", "mean_per_point", "logvar_per_point"))


def _grad_variant_ratio(tag, pattern, B=5):
    import torch
    Wn, x = lc.weights(tag), lc.inputs(tag, B, 1, 41, pattern)
    a = (Wn, tag, x["code"], x["valid"], x["noise"], x["d_mean"], x["d_logvar"])
    truth, yard = lc.autograd(*a, torch.float64, params=False), lc.autograd(*a, torch.float32, params=False)
    bad = lc.autograd(*a, torch.float64, mutate="absent_keys_grad", params=False)
    assert np.array_equal(bad["mean"], truth["mean"]), "the variant differs in the gradient only"
    return {k: lc.shape_ratio(bad[k], yard[k], truth[k]) for k in ("d_part_code", "d_noise")}, \
        {k: np.abs(bad[k] - truth[k]).max() / np.abs(truth[k]).max() for k in ("d_part_code", "d_noise")}


def test_the_recorded_factors_reject_every_wrong_variant():
    """(a) gradient through the keys of an all-absent shape, (b) class embedding row j % 4, (c) the last 8 input channels of proj_in dropped,
    (d) heads split at width 32, (e) pre_norm skipped, (f) flow swap parity inverted: each is rejected at F / FG on a named configuration.  On
    `shipped` (b), (d) and (e) are the restatement itself, so no test at that configuration can see them."""
    assert lc.F is not None and lc.FG is not None
    where = {"class_mod4": "wide", "drop_in8": "tiny", "head32": "tiny", "no_pre_norm": "plain", "swap_parity": "tiny"}
    for mutate, tag in where.items():
        r = _forward_variant_ratio(tag, mutate)
        print(f"variant {mutate} on {tag}: error {r:.3g} x the fp32 oracle's (F = {lc.F})")
        assert r > lc.F, (mutate, tag, r)
    print(f"variant head32 on wide (16 heads of 64 at one block): {_forward_variant_ratio('wide', 'head32'):.3g} x (tiny is where it is caught)")
    shape_r, of_max = _grad_variant_ratio("tiny", "shape_all_absent")
    b = 5 // 2
    print(f"variant absent_keys_grad on tiny: shape {b} at {shape_r['d_part_code'][b]:.3g} (d_part_code) / {shape_r['d_noise'][b]:.3g} (d_noise) x the fp32 autograd's "
          f"worst shape (FG = {lc.FG}); {of_max['d_part_code']:.2e} / {of_max['d_noise']:.2e} of the tensor's max-abs")
    assert shape_r["d_part_code"][b] > lc.FG and shape_r["d_noise"][b] > lc.FG
    assert all(np.all(np.delete(v, b) == 0) for v in shape_r.values()), "shapes with a present part keep their gradient"
    # what a test at the shipped configuration can and cannot see
    accepted = {m for m in where if not _forward_variant_ratio("shipped", m, B=2) > lc.F}
    sr, om = _grad_variant_ratio("shipped", "shape_all_absent", B=3)
    print(f"shipped: variants accepted {sorted(accepted)}; absent_keys_grad: shape ratio {sr['d_part_code'][1]:.3g} / {sr['d_noise'][1]:.3g}, "
          f"{om['d_part_code']:.2e} / {om['d_noise']:.2e} of max-abs (the 5e-4 gate of the tensor's max-abs passes d_noise)")
    assert accepted == {"class_mod4", "head32", "no_pre_norm"}
    assert sr["d_part_code"][1] > lc.FG and om["d_noise"] < 5e-4
