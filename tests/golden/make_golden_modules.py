#!/usr/bin/env python
"""Generate tests/golden/reference_modules.npz from the REFERENCE's own config loader and registry on CPU (dev container only).

    python tests/golden/make_golden_modules.py && python tests/golden/manifest.py

What tests/test_modules_cpu.py checks the drop-in modules against, recorded once so that the tests need nothing outside the
repository: for every shipped config (configs/gen_{chair,airplane,car,lamp}.py, configs/train_chair_stage{1,2}.py) its
`cfg.model` as plain data and the state_dict layout (key order, shape, dtype) and parameter count of the model the reference's
`build_from_cfg(cfg.model, MODELS)` builds; the same for gen_chair's diffusion at num_timesteps = 10 and its encoder (with the
attributes encoders.attach() reads from it); and the keyword arguments the reference's AnchorDiffAE.decode passes to the
diffusion's p_sample_loop_progressive (anchor_gen.py:149-158).  The document is JSON, stored as uint8 bytes under the key `json`
(the manifest hashes array contents).
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CONFIGS = ["gen_chair.py", "gen_airplane.py", "gen_car.py", "gen_lamp.py", "train_chair_stage1.py", "train_chair_stage2.py"]


def plain(c):
    if hasattr(c, "items"):
        return {k: plain(v) for k, v in c.items()}
    if isinstance(c, (list, tuple)):
        return [plain(v) for v in c]
    return c


def layout(sd):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]


class _Stop(Exception):
    pass


def decode_kwargs():
    """Names of the keyword arguments the reference's decode hands to p_sample_loop_progressive (recorded by a spy diffusion)."""
    import ref_import
    with contextlib.redirect_stdout(io.StringIO()):
        model, _ = ref_import.build_reference_model("gen_chair.py", 10)
    seen = {}

    def spy(*a, **k):
        seen["args"], seen["kwargs"] = len(a), sorted(k)
        raise _Stop

    model.diffusion.p_sample_loop_progressive = spy
    B, N = 1, 32
    ctx = [torch.zeros(B, 256, 4), torch.ones(B, 6, 4)]
    seg = torch.zeros(B, N, dtype=torch.int32)
    try:
        model.decode(torch.zeros(B, 3, N), ctx=ctx, variance=torch.ones(B, 3, N), anchor_assignments=seg, valid_id=torch.ones(B, 4),
                     device="cpu")
    except _Stop:
        pass
    return seen


def encoder_attrs(enc):
    """The attributes of a built reference PartEncoderForTransformerDecoder that encoders.attach() reads."""
    al, blk = enc.part_aligner, enc.part_aligner.transformer_blocks[0]
    names = ("zdim", "n_class", "include_z", "include_part_code", "include_params", "use_gt_params", "encode_ref", "log_scale_var", "gen",
             "fit_loss_type", "fit_loss_weight", "use_flow", "prior_var", "selective_noise_sampling", "selective_noise_sampling_global",
             "per_part_encoder")
    al_names = ("inner_dim", "use_linear", "n_class", "class_cond", "mask_out_unreferenced_code", "cimle", "noise_dim", "noise_scale",
                "cimle_start_epoch", "add_class_cond", "cond_noise_type")
    return {"encoder": {k: getattr(enc, k) for k in names},
            "part_aligner": {**{k: getattr(al, k) for k in al_names}, "depth": len(al.transformer_blocks), "heads": blk.attn2.heads,
                             "single_attn": blk.single_attn, "proj_out_features": al.proj_out.out_features},
            "flow": {"count": len(enc.flow), "depth": len(enc.flow[0].chain), "hidden": enc.flow[0].chain[0].net_s_t[0].out_features}}


def main():
    import ref_import
    doc = {"configs": {}}
    for name in CONFIGS:
        with contextlib.redirect_stdout(io.StringIO()):
            model, cfg = ref_import.build_reference_model(name)
        doc["configs"][name] = {"model_cfg": plain(cfg.model), "state_dict": layout(model.state_dict()),
                                "n_params": int(sum(p.numel() for p in model.parameters()))}
    with contextlib.redirect_stdout(io.StringIO()):
        model, cfg = ref_import.build_reference_model("gen_chair.py", 10)
    doc["gen_chair_T10_diffusion_state_dict"] = layout(model.diffusion.state_dict())
    doc["gen_chair_encoder_state_dict"] = layout(model.encoder.state_dict())
    doc["gen_chair_encoder_attrs"] = encoder_attrs(model.encoder)
    doc["decode_call"] = decode_kwargs()
    text = json.dumps(doc, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "reference_modules.npz"), json=np.frombuffer(text.encode(), dtype=np.uint8))
    print("wrote reference_modules.npz:", len(text), "bytes of JSON")


if __name__ == "__main__":
    main()
