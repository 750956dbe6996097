#!/usr/bin/env python
"""Part-level shape editing with libdfx (the paper's editing applications): interpolate one part between shapes, mix parts across
shapes, drift part anchors — each one dfx_compose_latents call + one persistent chain launch (difffacto_amd.editing).

    python examples/edit.py --shapes 4 --steps 5 --timesteps 100 [--checkpoint pretrained/chair.pth] [--out-dir edits]

Without a checkpoint the networks are random-init (synthetic weights): the clouds are noise-shaped, the calls and shapes are real.
Writes interpolate.npy (shapes, steps, N, 3), mix.npy (shapes, 1, N, 3), drift.npy (shapes, steps, N, 3) and their seg ids.

    python examples/edit.py --reconfigure --shapes 4 --starts 3 --part 0

re-configures instead: part --part of every shape is made 1.2 / 1.5 times larger along z (two candidate edits) and the other parts re-arrange
themselves, by gradient descent on the aligner noise from --starts random starts per edit; all shapes x edits x starts rows are ONE
dfx_noise_opt_run call and one chain launch (editing.reconfigure_part).  Writes reconfigure.npy (shapes, edits, N, 3): the best start per edit.

    python examples/edit.py --resample-part 1 --each 5 [--free-size --params 3 [--selective]] [--candidates 100]

samples new styles instead (the reference's tools/run_sample_one_part.py): --each new styles of part --resample-part per shape; among --candidates
aligner noises per style the one that keeps the other parts where they were, or with --free-size the first / the --params most diverse ones
(--selective); one dfx_part_search call for all shapes, one chain launch (editing.sample_part).  Writes resample.npy (shapes, each, params, N, 3).

    python examples/edit.py --vary --steps-back 40 --parts 1 --each 4

makes variations of EXISTING clouds instead (here: the shapes' own generated clouds): each cloud is noised --steps-back steps back and denoised again,
--each times with different noise; only the points of --parts are regenerated (all parts without --parts), the other parts' points come back bit
for bit.  One dfx_refine_chain launch for all shapes x each rows (editing.vary_shape).  Writes vary.npy (shapes, each, N, 3) and vary_base.npy.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from difffacto_amd import editing, modules, synth  # noqa: E402
from generate import NPOINTS, build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gen_chair", choices=sorted(NPOINTS))
    ap.add_argument("--shapes", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="interpolation steps / drift factors per shape")
    ap.add_argument("--part", type=int, default=2, help="the part to interpolate")
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--checkpoint", default=None, help="reference checkpoint (Runner.save format: {'model': state_dict})")
    ap.add_argument("--out-dir", default="edits")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reconfigure", action="store_true", help="edit the size of --part and let the other parts re-arrange (noise optimization)")
    ap.add_argument("--starts", type=int, default=3, help="--reconfigure: random noise starts per candidate edit")
    ap.add_argument("--max-iter", type=int, default=300, help="--reconfigure: iterations of the noise optimization")
    ap.add_argument("--resample-part", type=int, default=None, help="sample new styles of this part, the other parts kept")
    ap.add_argument("--each", type=int, default=5, help="--resample-part: new styles per shape")
    ap.add_argument("--free-size", action="store_true", help="--resample-part: do not fit the other parts to where they were")
    ap.add_argument("--params", type=int, default=1, help="--resample-part --free-size: configurations per new style")
    ap.add_argument("--selective", action="store_true", help="--resample-part --free-size: the most diverse configurations instead of the first")
    ap.add_argument("--candidates", type=int, default=100, help="--resample-part: aligner noises searched per new style")
    ap.add_argument("--vary", action="store_true", help="variations of the shapes' generated clouds: noise --steps-back steps, denoise again")
    ap.add_argument("--steps-back", type=int, default=40, help="--vary: strength, 1 .. --timesteps")
    ap.add_argument("--parts", type=int, nargs="*", default=None, help="--vary: regenerate these parts only, hold the others (default: all)")
    a = ap.parse_args()

    enc, diff = build(a.config, a.timesteps, a.precision, 0)
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
    N, B = NPOINTS[a.config], a.shapes
    g = torch.Generator().manual_seed(a.seed)
    codes = enc.sampler().flow_reverse(torch.randn(B, enc.zdim, enc.n_class, generator=g).cuda())   # part codes from the flow prior
    os.makedirs(a.out_dir, exist_ok=True)
    if a.vary:
        valid = torch.ones(B, enc.n_class, device="cuda")
        ctx, _mean_pp, _logvar_pp, seg, valid, _lat = enc.compose_latents(codes, np.repeat(np.arange(B, dtype=np.int32)[:, None], enc.n_class, 1),
                                                                          valid, N, noise_src=editing._noise(enc, B, "cuda", g))
        base = modules.decode(diff, ctx, seg, valid_id=valid, seed=a.seed)["pred"]                     # the clouds to vary (B,N,3)
        out = editing.vary_shape(diff, ctx, seg, base, a.steps_back, parts=a.parts, each=a.each, valid_id=valid, seed=a.seed + 1)
        pred = out["pred"]
        held = (out["held"][:, None, :].expand(B, a.each, -1).gather(2, out["seg_mask"].long()) != 0)   # (B,each,N): points of held parts
        same = torch.equal(pred[held], base[:, None].expand_as(pred)[held])
        np.save(os.path.join(a.out_dir, "vary.npy"), pred.cpu().numpy())
        np.save(os.path.join(a.out_dir, "vary_base.npy"), base.cpu().numpy())
        np.save(os.path.join(a.out_dir, "vary_seg.npy"), out["seg_mask"].cpu().numpy())
        moved = float((pred - base[:, None]).abs().amax()) if pred.numel() else 0.0
        print(f"vary: {B * a.each} rows in one launch, {a.steps_back} of {a.timesteps} steps back, parts {a.parts if a.parts is not None else 'all'}; "
              f"held points {int(held.sum())} of {held.numel()} unchanged: {same}; largest move {moved:.3f}; clouds {tuple(pred.shape)}, "
              f"finite: {bool(torch.isfinite(pred).all())} -> {a.out_dir}/vary.npy")
        return
    if a.resample_part is not None:
        # the shapes' own configuration: the aligner's parameters under one noise draw per shape
        valid = torch.ones(B, enc.n_class)
        mean, logvar = enc.sampler().part_aligner(codes, valid, torch.randn(B, enc.part_aligner.noise_dim, generator=g))
        out = editing.sample_part(enc, diff, codes, valid, mean, logvar, a.resample_part, a.each, fix_size=not a.free_size,
                                  param_sample_num=a.params, selective=a.selective, K=a.candidates, npoints=N, seed=a.seed, generator=g)
        pred = out["pred"]
        np.save(os.path.join(a.out_dir, "resample.npy"), pred.cpu().numpy())
        np.save(os.path.join(a.out_dir, "resample_seg.npy"), out["seg_mask"].reshape(*pred.shape[:3], N).cpu().numpy())
        print(f"resample part {a.resample_part}: {B * a.each * a.candidates} candidate rows in one search call, picked noises {out['idx'].reshape(B, -1)[0].tolist()} "
              f"(shape 0), non-finite candidates {int(out['n_bad'])}, clouds {tuple(pred.shape)}, finite: {bool(torch.isfinite(pred).all())} "
              f"-> {a.out_dir}/resample.npy")
        return
    if a.reconfigure:
        # the shapes' own configuration: the aligner's parameters under one noise draw per shape
        valid = torch.ones(B, enc.n_class)
        mean, logvar = enc.sampler().part_aligner(codes, valid, torch.randn(B, enc.part_aligner.noise_dim, generator=g))
        factors = torch.tensor([1.2, 1.5])
        E, T = len(factors), a.starts
        shape_row = np.repeat(np.arange(B), E * T)
        var = torch.exp(logvar).cpu()
        new_var = var[torch.as_tensor(shape_row), :, a.part].clone()
        new_var[:, 2] *= factors.repeat_interleave(T).repeat(B)
        out = editing.reconfigure_part(enc, diff, codes, mean.cpu(), var, a.part, new_var=new_var, shape_row=shape_row, max_iter=a.max_iter,
                                       npoints=N, generator=g)
        L = out["losses"]["L"].reshape(B, E, T)
        best = L.argmin(2)                                                                            # the best start of every (shape, edit)
        pick = (torch.arange(B * E, device=best.device) * T + best.reshape(-1))
        pred = out["pred"][pick].reshape(B, E, N, 3)
        np.save(os.path.join(a.out_dir, "reconfigure.npy"), pred.cpu().numpy())
        np.save(os.path.join(a.out_dir, "reconfigure_seg.npy"), out["seg_mask"][pick].reshape(B, E, N).cpu().numpy())
        print(f"reconfigure: {B * E * T} rows in one optimizer call, iterations {int(out['iters_done'].min())}..{int(out['iters_done'].max())}, "
              f"best loss per (shape, edit) {[[round(float(x), 4) for x in row] for row in L.min(2)[0].cpu()]} -> {a.out_dir}/reconfigure.npy {tuple(pred.shape)}")
        return
    runs = {
        "interpolate": lambda: editing.interpolate_part(enc, diff, codes, a.part, a.steps, npoints=N, generator=g),
        "mix": lambda: editing.mix_parts(enc, diff, codes, np.stack([np.roll(np.arange(B), -j) for j in range(enc.n_class)], 1),
                                         npoints=N, generator=g),
        "drift": lambda: editing.drift_anchors(enc, diff, codes, np.linspace(1, 5, a.steps), npoints=N, generator=g),
    }
    for name, run in runs.items():
        out = run()
        pred = out["pred"]
        np.save(os.path.join(a.out_dir, f"{name}.npy"), pred.cpu().numpy())
        np.save(os.path.join(a.out_dir, f"{name}_seg.npy"), out["seg_mask"].cpu().numpy())
        print(f"{name}: clouds {tuple(pred.shape)}, finite: {bool(torch.isfinite(pred).all())} -> {a.out_dir}/{name}.npy")


if __name__ == "__main__":
    main()
