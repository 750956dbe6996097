#!/usr/bin/env python
"""End-to-end generation with libdfx through the reference's module API (what `tools/run_net.py --task val` does for
configs/gen_*.py, anchor_gen.py:1034-1084): latent sampler -> fused reverse chain -> optional generation metrics.

    python examples/generate.py --config gen_chair --shapes 32 --K 2 --timesteps 100 [--checkpoint pretrained/chair.pth]
                                [--ddim 25] [--metrics [--jsd]] [--out clouds.npy]
                                [--selective {shape,global} [--keep 10] [--rule first_pick]]

--selective: diverse generation (the reference's selective noise sampling): 100 aligner noises per shape unless --K says otherwise,
of which --keep per shape survive: the most different ones of every shape, or of the whole batch ('global').

Without a checkpoint the networks are random-init (synthetic weights): the clouds are noise-shaped, the timings are real.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difffacto_amd import synth  # noqa: E402
from difffacto_amd.encoders import PartEncoderForTransformerDecoder, generate  # noqa: E402
from difffacto_amd.modules import AnchoredDiffusion  # noqa: E402

# the model sections of configs/gen_{chair,airplane,car,lamp}.py that matter for generation
NOISE_SCALE = {"gen_chair": 100, "gen_airplane": 50, "gen_car": 50, "gen_lamp": 10}
NPOINTS = {"gen_chair": 2048, "gen_airplane": 2048, "gen_car": 8192, "gen_lamp": 2048}


def build(config, timesteps, precision, ddim):
    enc = PartEncoderForTransformerDecoder(
        encoder=dict(type="PointNetV2", zdim=256, point_dim=3, per_part_mlp=True),
        part_aligner=dict(type="PartAlignerTransformer", in_channels=256, out_channels=6, n_class=4, d_head=32, depth=5, n_heads=8,
                          dropout=0., use_checkpoint=False, use_linear=True, class_cond=True, single_attn=True, add_class_cond=True,
                          cimle=True, noise_scale=NOISE_SCALE[config], cond_noise_type=0),
        n_class=4, kl_weight=0, fit_loss_type=4, fit_loss_weight=1.0, use_flow=True, latent_flow_depth=14, latent_flow_hidden_dim=256,
        include_z=False, include_part_code=True, include_params=True, use_gt_params=False, gen=True, prior_var=1.0)
    net = dict(type="TransformerNet", in_channels=3, out_channels=3, n_heads=8, d_head=16, depth=5, dropout=0.2, context_dim=256 + 6,
               use_linear=True, single_attn=True, class_cond=True, n_class=4, cat_params_to_x=True, cat_class_to_x=True)
    extra = dict(ddim_sampling=True, ddim_nsteps=ddim, ddim_discretize="quad", ddim_eta=1.0) if ddim else {}
    diff = AnchoredDiffusion(net=net, num_timesteps=timesteps, beta_1=1e-4, beta_T=0.02, k=1.0, res=False, mode="linear", use_beta=False,
                             rescale_timesteps=False, model_mean_type="epsilon", model_var_type="fixed_small", learn_variance=True,
                             learn_anchor=True, include_anchors=False, precision=precision, **extra)
    return enc, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gen_chair", choices=sorted(NOISE_SCALE))
    ap.add_argument("--shapes", type=int, default=32, help="shapes drawn from the flow prior")
    ap.add_argument("--K", type=int, default=None, help="aligner noises per shape (default 2; 100 with --selective; the reference's val pass uses 10)")
    ap.add_argument("--selective", default=None, choices=["shape", "global"], help="keep the most different configurations: per shape, or of the whole batch")
    ap.add_argument("--keep", type=int, default=10, help="with --selective: rows kept per shape")
    ap.add_argument("--rule", default="farthest", choices=["farthest", "first_pick"],
                    help="with --selective global: farthest-point selection, or the distance to the first pick only (what the reference executes)")
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--ddim", type=int, default=0, help="DDIM with this many steps ('quad' list) instead of DDPM")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--checkpoint", default=None, help="reference checkpoint (Runner.save format: {'model': state_dict})")
    ap.add_argument("--metrics", action="store_true", help="MMD / COV / 1-NNA of the first half of the clouds against the second")
    ap.add_argument("--jsd", action="store_true", help="with --metrics: occupancy-grid JSD of the two halves, whole shapes and per part")
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.jsd and not a.metrics:
        ap.error("--jsd adds to the generation metrics: pass --metrics as well")

    enc, diff = build(a.config, a.timesteps, a.precision, a.ddim)
    if a.checkpoint:
        sd = torch.load(a.checkpoint, map_location="cpu")
        sd = sd.get("model", sd)
        sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
        enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=True)
        diff.model.load_state_dict({k[len("diffusion.model."):]: v for k, v in sd.items() if k.startswith("diffusion.model.")}, strict=True)
    else:
        W = synth.make_latent_weights(0)
        W.update({"encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
        diff.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()})
    enc, diff = enc.cuda().eval(), diff.cuda().eval()
    torch.manual_seed(a.seed)
    valid = torch.from_numpy(synth.make_latents(a.shapes, seed=a.seed)[3]).cuda()
    N = NPOINTS[a.config]
    generate(enc, diff, 2, N, valid_id=valid[:2], K=1, seed=a.seed)   # warm-up (library load, handles)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K = a.K if a.K is not None else (100 if a.selective else 2)
    out = generate(enc, diff, a.shapes, N, valid_id=valid, fixed_id=[0, 0, 0, 0], K=K, seed=a.seed, selective=a.selective,
                   selective_keep=a.keep, selective_rule=a.rule)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pred = out["pred"]
    n = pred.shape[0]
    steps = len(diff.steps)
    print(f"{a.config}: {n} clouds x {N} points, {steps} {'DDIM' if a.ddim else 'DDPM'} steps ({a.precision}) in {dt * 1e3:.1f} ms = {n / dt:.1f} shapes/s; "
          f"finite: {bool(torch.isfinite(pred).all())}")
    if a.selective:
        per_shape = torch.bincount(out["source_row"], minlength=a.shapes)
        print(f"selective {a.selective} ({a.rule}): {K} candidates per shape, {n} rows kept; rows per shape min {int(per_shape.min())} max {int(per_shape.max())}")
    if a.out:
        np.save(a.out, pred.cpu().numpy())
    if a.metrics:
        from difffacto_amd.evaluation import compute_all_metrics
        lo, hi = pred.amin((1, 2), keepdim=True), pred.amax((1, 2), keepdim=True)
        unit = (pred - lo) / (hi - lo)                      # EMD expects clouds inside the unit cube
        m = n // 2
        t0 = time.perf_counter()
        res = compute_all_metrics(unit[:m].contiguous(), unit[m:2 * m].contiguous(), batch_size=32)
        if a.jsd:   # the evaluation's [-1, 1] normalisation, scaled into the unit cube (exact in fp32)
            from difffacto_amd.evaluation import _normalize_shapes, part_jsd
            half, seg = _normalize_shapes(pred) * 0.5, out["pred_seg_mask"]
            res.update(part_jsd(half[:m].contiguous(), seg[:m], half[m:2 * m].contiguous(), seg[m:2 * m], n_class=4))
        torch.cuda.synchronize()
        print(f"metrics of clouds[:{m}] vs clouds[{m}:{2 * m}] ({time.perf_counter() - t0:.1f} s): " + ", ".join(f"{k} {float(v):.4g}" for k, v in sorted(res.items())))


if __name__ == "__main__":
    main()
