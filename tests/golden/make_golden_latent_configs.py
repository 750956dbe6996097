#!/usr/bin/env python
"""Golden vectors of the reference's latent front end at configurations other than the shipped one (dev container only; conventions and
helpers of make_golden.py / make_golden_forward.py).

    python tests/golden/make_golden_latent_configs.py

Written to tests/golden/latentcfg/ with their own MANIFEST.sha256.  The reference's PartEncoderForTransformerDecoder is built from
configs/gen_chair.py with the encoder section's sizes replaced by those of tests/_latent_cfg.py:CONFIGS (tiny, wide, one, plain), and
loaded with the project's synthetic weights (synth.make_latent_weights(0, ...): not stored).  One file per configuration,
<tag>.npz, B = 5, keys prefixed by the validity pattern ("all/", "one_absent/", "one_present/", "shape_all_absent/"):

in/*                     w_noise (5,Z,J), noise (5 K,ND; cimle only), valid (5,J), code (5,Z,J), d_mean / d_logvar (5 K,3,J)
sl/*                     PartEncoder.sample_latents(fixed_id = 0, K = 2; K = 1 for plain) on w_noise: part_code, mean, logvar, valid_id,
                         seg_mask, mean_per_point, logvar_per_point, ctx1 (npoints = 3 J)
al/mean, al/logvar       PartAlignerTransformer.forward(code repeated K times, valid repeated, noise)
al/d_part_code, d_noise  torch autograd of sum(mean d_mean) + sum(logvar d_logvar) (cimle configurations)
al/grad/<name>           the parameter gradients of the same backward, for tiny and one and there under "shape_all_absent/" only, which
                         keeps each file under 1 MiB (those of wide are tens of MB); all others are checked against float64 autograd
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "latentcfg")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_forward  # noqa: E402,F401  (sets up sys.path for ref_import / difffacto_amd)
import manifest  # noqa: E402
import ref_import  # noqa: E402
import _latent_cfg as lc  # noqa: E402

F32 = np.float32
B = 5
TAGS = ("tiny", "wide", "one", "plain")
PARAM_GRADS = ("tiny", "one")


def build_encoder(tag):
    cfg = lc.CONFIGS[tag]
    ref_import.import_reference()
    from difffacto.config.config import get_cfg, init_cfg
    from difffacto.utils.registry import ENCODERS, build_from_cfg
    init_cfg(os.path.join(ref_import.REF_ROOT, "configs", "gen_chair.py"))
    e = get_cfg().model["encoder"]
    e["encoder"]["zdim"] = cfg["zdim"]
    e["n_class"] = cfg["n_class"]
    e["use_flow"] = cfg["flow_depth"] > 0
    e["latent_flow_depth"], e["latent_flow_hidden_dim"] = cfg["flow_depth"], cfg["flow_hidden"]
    a = e["part_aligner"]
    a["in_channels"], a["n_class"], a["d_head"], a["n_heads"], a["depth"] = cfg["zdim"], cfg["n_class"], cfg["d_head"], cfg["heads"], cfg["depth"]
    a["cimle"] = cfg["cimle"]
    if cfg["cimle"]:
        a["noise_dim"] = cfg["noise_dim"]
    with contextlib.redirect_stdout(io.StringIO()):
        enc = build_from_cfg(e, ENCODERS)
    W = lc.weights(tag, 0)
    sd = enc.state_dict()
    assert {k for k in sd if k.startswith(("flow.", "part_aligner."))} == set(W), sorted(set(W) ^ {k for k in sd if k.startswith(("flow.", "part_aligner."))})[:6]
    for k, v in W.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v.copy())
    enc.load_state_dict(sd, strict=True)
    return enc.eval()


def gen(tag):
    cfg, enc = lc.CONFIGS[tag], build_encoder(tag)
    J, K = cfg["n_class"], 2 if cfg["cimle"] else 1
    npoints = 3 * J
    arrays = {"K": np.array(K), "npoints": np.array(npoints), "weight_seed": np.array(0)}
    t = lambda a: None if a is None else torch.from_numpy(a.copy())
    for i, pattern in enumerate(lc.VALID_PATTERNS):
        x = lc.inputs(tag, B, K, 500 + i, pattern)
        pre = pattern + "/"
        arrays.update({pre + "in/" + k: v for k, v in x.items() if v is not None})
        queue = [x["w_noise"]] + ([x["noise"]] if cfg["cimle"] else [])
        real = torch.randn

        def fake_randn(*shape, **kw):   # part_encoders.py:1054, :1065 (in this order)
            a = queue.pop(0)
            assert tuple(shape) == a.shape, (shape, a.shape)
            return torch.from_numpy(a.copy())

        try:
            torch.randn = fake_randn
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                ctx, mpp, lpp, seg, vid, lat = enc.sample_latents(B, npoints, "cpu", fixed_id=torch.zeros(J), valid_id=t(x["valid"]), epoch=0, K=K)
        finally:
            torch.randn = real
        assert not queue
        arrays.update({pre + "sl/part_code": lat[0], pre + "sl/mean": lat[1], pre + "sl/logvar": lat[2], pre + "sl/valid_id": vid,
                       pre + "sl/seg_mask": seg.to(torch.int32), pre + "sl/mean_per_point": mpp, pre + "sl/logvar_per_point": lpp, pre + "sl/ctx1": ctx[1]})
        code = t(np.repeat(x["code"], K, axis=0)).requires_grad_(cfg["cimle"])
        noise = t(x["noise"])
        if noise is not None:
            noise.requires_grad_(True)
        enc.part_aligner.zero_grad()
        with torch.set_grad_enabled(cfg["cimle"]):
            m, l = enc.part_aligner(code, t(np.repeat(x["valid"], K, axis=0)), noise=noise)
        arrays.update({pre + "al/mean": m.detach(), pre + "al/logvar": l.detach()})
        if cfg["cimle"]:
            ((m * t(x["d_mean"])).sum() + (l * t(x["d_logvar"])).sum()).backward()
            arrays.update({pre + "al/d_part_code": code.grad, pre + "al/d_noise": noise.grad})
            if tag in PARAM_GRADS and pattern == "shape_all_absent":
                arrays.update({pre + "al/grad/" + k: p.grad for k, p in enc.part_aligner.named_parameters() if p.grad is not None})
    arrays = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    arrays = {k: (v.astype(F32) if v.dtype == np.float64 else v) for k, v in arrays.items()}
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {tag}: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    for tag in TAGS:
        gen(tag)
    path = os.path.join(OUT, "MANIFEST.sha256")
    with open(path, "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
