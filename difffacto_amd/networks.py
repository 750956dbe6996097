"""Host-side mirror of the reference's top-level model ``MODELS['AnchorDiffAE']`` (python/difffacto/models/networks/anchor_gen.py:29-1136)
for the configurations it ships: same constructor arguments, sub-module names (``encoder.*`` / ``diffusion.*`` state_dict keys, so
``pretrained/*.pth`` loads), methods and — the contract ``Runner.val`` writes to disk (runner/runner.py:353-377) — the same output
dicts from ``forward``:

* eval + ``gen``            -> ``[(dict, "gen_fixed0000")]``  (anchor_gen.py:1034-1084: encoder pass, sample_latents, decode, K-fold
                               ``"{k}_sample {i}"`` / ``"sample prior {i}"`` keys under cIMLE)
* eval, not ``gen`` (cIMLE) -> ``[(dict, "sample")]``         (:1085-1134: sample_noise, encode, decode — the reconstruction mode)
* eval + ``interpolate`` / ``combine`` / ``drift_anchors`` -> ``[(dict, "interpolate" / "mixing" / "interpolate_params")]`` (:1027-1032:
                               the editing modes, ``interpolate_latent`` / ``combine_latent`` / ``interpolate_params``; ``combine_latent_specific``
                               is the mixing runner's entry, runner/mixing_runner.py:89)
* train()                   -> loss dict                      (:1002-1021: prior_loss / fit_loss / mse_loss; stage 1 natively, see
                               ``training.stage1_losses``)

Everything heavy runs in libdfx through the encoder / diffusion mirrors; this file is the reference's bookkeeping (dict keys,
K-fold regrouping, which random draw happens where).  Random draws happen at the reference's sites in the reference's order
(reparameterisation -> latents -> aligner noise -> chain -> priors); the chain's noise is libdfx's Philox stream keyed by a seed
that is drawn from torch's generator at the point where the reference draws x_T (``engine.resolve_seed``).
Options outside the shipped ``configs/gen_*.py`` / ``train_*.py`` raise ``NotImplementedError``.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import modules as _modules
from .encoders import PartEncoderForTransformerDecoder
from .modules import AnchoredDiffusion


def _unsupported(what):
    raise NotImplementedError(f"libdfx implements the shipped gen_* / train_* AnchorDiffAE configuration only: {what}")


class Uniform:
    """``SAMPLERS['Uniform']`` (samplers/sampler.py:25-47): timesteps drawn with ``np.random.choice`` on the host, unit weights."""

    def __init__(self, num_timesteps):
        self.num_timesteps = int(num_timesteps)
        self.weight = np.ones([self.num_timesteps])

    def weights(self):
        return self.weight

    def sample(self, batch_size, device):
        w = self.weights()
        p = w / np.sum(w)
        idx = np.random.choice(len(p), size=(batch_size,), p=p)
        return torch.from_numpy(idx).long().to(device), torch.from_numpy(1 / (len(p) * p[idx])).float().to(device)


def _fold(v, h):
    """einops ``rearrange(v, "(b h) ... -> b h ...", h=h)`` (anchor_gen.py:1062)."""
    return v.reshape(v.shape[0] // h, h, *v.shape[1:])


class AnchorDiffAE(nn.Module):
    def __init__(self, encoder, diffusion, sampler, num_anchors, num_timesteps, npoints=2048, zero_anchors=False, gen=False,
                 sample_noise_num=20, cimle=False, cimle_sample_num=10, diffusion_loss_weight=1.0, use_input=False, learn_var=False,
                 detach_variance=True, detach_anchor=True, global_shift=False, global_scale=False, vertical_only=True, ret_traj=False,
                 ret_interval=20, forward_sample=False, interpolate=False, interpolate_part_id=2, fix_part_ids=None, combine=False,
                 drift_anchors=False, save_pred_xstart=False, save_dir=None, save_weights=False, noise_reg_loss=True,
                 reg_loss_weight=1.0, pretrain_prior=False, train_language=False, language_encoder=None, clip_weight=1.0,
                 triplet_weight=1.0, triplet_thresh=0.1, precision="bf16"):
        super().__init__()
        for name, val in (("zero_anchors", zero_anchors), ("use_input", use_input), ("save_weights", save_weights),
                          ("pretrain_prior", pretrain_prior), ("train_language", train_language), ("forward_sample", forward_sample)):
            if val:
                _unsupported(f"{name}=True")
        if isinstance(encoder, nn.Module):
            self.encoder = encoder
        else:
            cfg = dict(encoder)
            if cfg.pop("type", "PartEncoderForTransformerDecoder") != "PartEncoderForTransformerDecoder":
                _unsupported("encoder type other than PartEncoderForTransformerDecoder")
            self.encoder = PartEncoderForTransformerDecoder(**cfg)
        if isinstance(diffusion, nn.Module):
            self.diffusion = diffusion
        else:
            cfg = dict(diffusion)
            if cfg.pop("type", "AnchoredDiffusion") != "AnchoredDiffusion":
                _unsupported("diffusion type other than AnchoredDiffusion")
            self.diffusion = AnchoredDiffusion(num_timesteps=num_timesteps, precision=precision, **cfg)   # anchor_gen.py:87
        if isinstance(sampler, dict):
            if sampler.get("type", "Uniform") != "Uniform":
                _unsupported("sampler type other than Uniform")
            sampler = Uniform(num_timesteps)
        self.sampler = sampler
        self.diffusion_loss_weight, self.sample_noise_num, self.cimle, self.cimle_sample_num = \
            diffusion_loss_weight, sample_noise_num, cimle, cimle_sample_num
        self.fix_part_ids, self.gen = fix_part_ids, gen
        self.interpolate, self.interpolate_part_id, self.combine, self.drift_anchors = interpolate, interpolate_part_id, combine, drift_anchors
        self.num_timesteps, self.num_anchors, self.npoints = int(num_timesteps), num_anchors, npoints
        # detach_anchor=False raises in the training forward (stage1_losses); detach_variance detaches a tensor the reference no longer reads
        # (anchor_gen.py:1013-1014 vs :1002), and learn_var / global_shift / global_scale / vertical_only are stored and never read by the
        # reference (:95-102): accepted and without effect, like there.
        self.detach_anchor, self.detach_variance = detach_anchor, detach_variance
        self.noise_reg_loss, self.reg_loss_weight = noise_reg_loss, reg_loss_weight           # edit_latent / optimize_latent (:891, :911)
        self.fixed_id = [0] * num_anchors
        self.points_per_anchor = npoints // num_anchors
        self.ret_traj, self.ret_interval, self.save_pred_xstart = ret_traj, ret_interval, save_pred_xstart

    # ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, anchors, ctx=None, noise=None, variance=None, anchor_assignments=None, valid_id=None, device="cuda", seed=None,
               generator=None, x_T_noise=None, step_noise=None):
        """anchor_gen.py:145-169.  ``anchors`` / ``variance`` (B,3,N) are the gathers of ctx[1] by ``anchor_assignments`` on every
        call path of the reference (:1044-1045, :1093-1099) — the kernel indexes ctx[1] itself.  ``noise``: an explicit x_T point
        cloud (B,3,N) as in the reference (:153, anchored_diffusion.py:560-561); then, or with ``save_pred_xstart``, the chain is
        walked one launch per step, else it is ONE persistent launch.  ``x_T_noise`` (B,3,N standard normal) / ``step_noise``
        (T,B,3,N) / ``seed`` / ``generator`` are libdfx extras (parity replays, reproducible runs)."""
        return _modules.decode(self.diffusion, ctx, anchor_assignments, valid_id=valid_id, ret_traj=self.ret_traj,
                               ret_interval=self.ret_interval, seed=seed, generator=generator, x_T_noise=x_T_noise,
                               step_noise=step_noise, save_pred_xstart=self.save_pred_xstart, x_T=noise)

    @torch.no_grad()
    def sample_one_part(self, code, valid_id, mean, logvar, seg_mask, part_id, sample_num_each, fix_size, param_sample_num,
                        selective_param_sample, K=100):
        """anchor_gen.py:307-337 (tools/run_sample_one_part.py): new styles for one part of every shape, decoded.  Returns the
        reference's 7-tuple (pred (bs,E,P,np,3), seg_mask (bs,E,P,np), valid_id (bs,E,P,J), codes (bs,E,P,zdim,J), noise_latents
        (bs*E*P,noise_dim), means, logvars (bs,E,P,3,J)); P = 1 under ``fix_size`` whatever ``param_sample_num`` says.  K and the
        repaired fix_size=False branches: ``PartEncoderForTransformerDecoder.sample_with_fixed_latents``."""
        bs, n = code.shape[0], seg_mask.shape[1]
        ctx, mean_pp, logvar_pp, seg, valid, (codes, noises, means, logvars) = self.encoder.sample_with_fixed_latents(
            code, valid_id, mean, logvar, seg_mask, part_id, sample_num_each, fix_size, param_sample_num, selective_param_sample, K=K)
        E, P = int(sample_num_each), codes.shape[0] // (bs * int(sample_num_each))
        pred = self.decode(mean_pp, ctx=ctx, variance=torch.exp(logvar_pp), anchor_assignments=seg.to(torch.int32), valid_id=valid)["pred"]
        J, Z = self.num_anchors, self.encoder.zdim
        return (pred.reshape(bs, E, P, n, 3), seg.reshape(bs, E, P, n), valid.reshape(bs, E, P, J), codes.reshape(bs, E, P, Z, J), noises,
                means.reshape(bs, E, P, 3, J), logvars.reshape(bs, E, P, 3, J))

    def sample(self, sample_num, fixed_id, valid_id, device, epoch, K=10, **selective):
        """anchor_gen.py:798-801 (K is ignored there as well: cimle_sample_num rows per shape).  With ``selective='shape' | 'global'``
        (and ``selective_keep``, ``selective_rule``, ``seed``, ``return_selection``: the keywords of the encoder's ``sample_latents``):
        its selective noise sampling, 100 candidates per shape of which ``selective_keep`` per shape are kept."""
        K = None if selective.get("selective") is not None else self.cimle_sample_num
        return self.encoder.sample_latents(sample_num, self.npoints, device, fixed_id=torch.as_tensor(fixed_id).to(device),
                                           valid_id=valid_id, epoch=epoch, K=K, part_code=None, **selective)

    @torch.no_grad()
    def cache_noise(self, pcds, device, eval_whole=False):
        """anchor_gen.py:807-815 (cIMLE noise caching of stage 2): the best of ``sample_noise_num`` aligner noises per shape."""
        if eval_whole:
            # (the reference's own eval_whole branch cannot run: it unpacks FIVE values from the encoder's six-tuple, anchor_gen.py:819 vs
            # part_encoders.py:1254 — ValueError before any arithmetic; no shipped config sets eval_whole: nothing to mirror)
            _unsupported("cache_noise(eval_whole=True) (the reference's branch raises ValueError at anchor_gen.py:819)")
        noise, idx = self.encoder.sample_noise(pcds, device, self.sample_noise_num)
        return noise[torch.arange(noise.shape[0], device=noise.device), idx]

    # ------------------------------------------------------------------------------------------------------------------
    # Part re-configuration (tools/shape_edit.py, tools/optimize_noise.py): ONE evaluation of the objective, differentiable in the aligner
    # noise ``z`` through training.AlignerTrainFn (dfx_aligner_train_forward / dfx_aligner_input_backward), so the reference's own loop
    # (``Adam([z])`` + ``ReduceLROnPlateau``) runs on top unmodified.  Freeze the model (``requires_grad_(False)``): PointNetV2 in eval() has
    # no backward, and with frozen weights the aligner's backward is the data-gradient chain alone.  Many problems at once, without the host
    # round trips: ``editing.reconfigure_part`` / ``editing.invert_noise``.
    def edit_latent(self, z, input, seg_flag, valid_id, ref_means, ref_vars, fix_ids, edit_part_id, edit_part_mean, edit_part_var, fit_weight=1):
        """anchor_gen.py:872-893: {'fit_loss' (B,), 'edit_loss' (1,) or (), 'reg_loss' (B,) with ``noise_reg_loss``}.  The part codes are
        computed without a graph (they do not depend on ``z``)."""
        fit_loss_dict = dict()
        with torch.no_grad():
            part_code_means, _ = self.encoder.get_part_code(input, seg_flag)
        part_code = part_code_means.transpose(1, 2)
        mean, logvar = self.encoder.get_params_from_part_code(part_code, valid_id, noise=z)
        fit_loss = (torch.cat([mean, logvar], dim=1) - torch.cat([ref_means, torch.log(ref_vars)], dim=1)) ** 2
        fit_loss = fit_loss * (valid_id * fix_ids).unsqueeze(1)
        fit_loss = fit_loss.sum(dim=(-1, -2)) / (valid_id * fix_ids).sum(dim=-1)
        if edit_part_mean is not None:
            edit_l_mean = torch.nn.functional.mse_loss(mean[..., edit_part_id], edit_part_mean)
        else:
            edit_l_mean = torch.zeros(1, device=mean.device)
        if edit_part_var is not None:
            edit_l_var = torch.nn.functional.mse_loss(logvar[..., edit_part_id], torch.log(edit_part_var))
        else:
            edit_l_var = torch.zeros(1, device=mean.device)
        fit_loss_dict["fit_loss"] = fit_weight * fit_loss
        fit_loss_dict["edit_loss"] = edit_l_var + edit_l_mean
        if self.noise_reg_loss:
            fit_loss_dict["reg_loss"] = self.reg_loss_weight * (z ** 2).sum(1)
        return fit_loss_dict

    def optimize_latent(self, pcds, z, device="cuda"):
        """anchor_gen.py:895-913: the encoder's loss dict (prior terms, 'fit_loss' (B,)) at aligner noise ``z`` (B,1,noise_dim) or
        (B,noise_dim), plus 'reg_loss'.  Goes through ``self.encoder(...)`` like the reference, reparameterisation draw included."""
        _ctx, _mean_pp, _logvar_pp, _flag_pp, fit_los_dict, _ = self.encoder(pcds, device, noise=z if z.dim() == 3 else z.unsqueeze(1))
        if self.noise_reg_loss:
            fit_los_dict["reg_loss"] = self.reg_loss_weight * (z ** 2).sum(1)
        return fit_los_dict

    @torch.no_grad()
    def cimle_forward(self, pcds, device="cuda", noise=None):
        """anchor_gen.py:837-870: decode every shape under K given aligner noises ``noise`` (B,K,noise_dim) (default: 10 candidates of
        ``sample_noise``).  Keys: "{k}_sample {i}" for every key of decode's dict, "sample prior {i}", "pred", "input", "input_ref",
        "seg_mask", "pred_seg_mask", "ref_seg_mask", "shift", "scale"; everything on the CPU."""
        inp = pcds["input"].to(device)
        ref = pcds["ref"].to(device)
        input_seg_mask = pcds["seg_mask"].to(device)
        seg_mask = pcds["ref_seg_mask"].to(device)
        valid_id = pcds["present"].to(device)
        B, N, C = ref.shape
        if noise is None:
            noise, _ = self.encoder.sample_noise(pcds, device, 10)
        noise = noise.detach()
        if noise.dim() == 2:
            noise = noise.unsqueeze(1)
        K = noise.shape[1]
        ctx, mean_pp, logvar_pp, _flag, _losses, _lat = self.encoder(pcds, device, noise=noise)
        var_pp = torch.exp(logvar_pp)
        priors = torch.randn_like(var_pp).transpose(1, 2) * torch.sqrt(var_pp.transpose(1, 2)) + mean_pp.transpose(1, 2)
        seg_mask, valid_id = (t.repeat_interleave(K, dim=0) for t in (seg_mask, valid_id))
        _pred = self.decode(mean_pp, ctx=ctx, device=device, variance=var_pp, anchor_assignments=seg_mask.to(torch.int32), valid_id=valid_id)
        pred = {}
        for i in range(K):
            for k, v in _pred.items():
                pred[f"{k}_sample {i}"] = _fold(v, K)[:, i]
        for i in range(K):
            pred[f"sample prior {i}"] = priors.reshape(B, K, N, C)[:, i]
        pred["pred"] = _fold(_pred["pred"], K)[:, 0]
        pred.update({"input": inp, "input_ref": ref, "seg_mask": input_seg_mask, "pred_seg_mask": seg_mask, "ref_seg_mask": pcds["ref_seg_mask"],
                     "shift": pcds["shift"], "scale": pcds["scale"]})
        return {k: v.detach().cpu() for k, v in pred.items()}

    # ------------------------------------------------------------------------------------------------------------------
    def forward(self, pcds, device="cuda", epoch=0, **kwargs):
        """anchor_gen.py:970-1136.  The gen branch takes ``selective='shape' | 'global'`` (+ ``selective_keep``, ``selective_rule``, ``seed``):
        the encoder's selective noise sampling.  'shape': the reference's dict with ``selective_keep`` samples per shape in place of
        ``cimle_sample_num`` ("pred_sample i" = kept row i of every shape).  'global': the B * selective_keep rows in pick order, one
        entry per row ("pred", "sample prior", "pred_seg_mask", "anchors", "present" = the row's own mask); the batch's own entries
        ("input", "shift", ...) stay per shape.  Both add "source_row" (the shape behind every kept row) and "selected"."""
        inp = pcds["input"].to(device)
        ref = pcds["ref"].to(device)
        input_seg_mask = pcds["seg_mask"].to(device)
        seg_mask = pcds["ref_seg_mask"].to(device)
        valid_id = pcds.get("present", None)
        dp_valid_id = pcds.get("dp_present", None)
        valid_id = None if valid_id is None else valid_id.to(device)
        B, N, C = ref.shape
        if self.npoints < N:
            _unsupported("npoints smaller than the reference cloud (anchor_gen.py:997-1001)")
        if self.training:
            from . import training as _training
            t, _ = self.sampler.sample(B, device)
            return _training.stage1_losses(self.encoder, self.diffusion, pcds, device=device, epoch=epoch, t=t,
                                           diffusion_loss_weight=self.diffusion_loss_weight, detach_anchor=self.detach_anchor)
        with torch.no_grad():
            # the reference runs the encoder on every val batch, gen branch included (:995): its reparameterisation draw comes first
            ctx, mean_pp, logvar_pp, _flag, _losses, _latents = self.encoder(pcds, device, epoch=epoch)
            if self.interpolate:                                                               # :1027-1032, in this order
                return [(self.interpolate_latent(device, pcds), "interpolate")]
            if self.combine:
                return [(self.combine_latent(pcds, device), "mixing")]
            if self.drift_anchors:
                return [(self.interpolate_params(device, pcds), "interpolate_params")]
            h = self.cimle_sample_num
            if self.gen:
                fixed_id = [0] * self.num_anchors
                for i in (self.fix_part_ids or ()):
                    fixed_id[i] = 1
                selective, kept = kwargs.get("selective"), None
                if selective is not None:
                    keys = ("selective", "selective_keep", "selective_rule", "seed")
                    ctx, mean_pp, logvar_pp, _seg, _valid, _lat, kept = self.sample(B, fixed_id, valid_id, device, epoch, return_selection=True,
                                                                                    **{k: kwargs[k] for k in keys if k in kwargs})
                    h = int(kwargs.get("selective_keep", 10))                                  # rows per shape instead of cimle_sample_num
                else:
                    ctx, mean_pp, logvar_pp, _seg, _valid, _lat = self.sample(B, fixed_id, valid_id, device, epoch, K=10)
                var_pp = torch.exp(logvar_pp)
                _pred = self.decode(mean_pp, ctx=ctx, device=device, variance=var_pp, anchor_assignments=_seg.to(torch.int32), valid_id=_valid)
                priors = torch.randn_like(var_pp.transpose(1, 2)) * torch.sqrt(var_pp.transpose(1, 2)) + mean_pp.transpose(1, 2)
                present = valid_id
                if self.cimle and selective != "global":
                    pred = {}
                    for i in range(h):
                        for k, v in _pred.items():
                            pred[f"{k}_sample {i}"] = _fold(v, h)[:, i]
                    for i in range(h):
                        pred[f"sample prior {i}"] = priors.reshape(B, h, self.npoints, C)[:, i]
                    pred["pred"] = _fold(_pred["pred"], h)[:, 0]
                    pred["pred_seg_mask"] = _fold(_seg, h)[:, 0]
                    pred["anchors"] = _fold(mean_pp, h)[:, 0].transpose(1, 2)
                else:
                    # one entry per row.  selective='global': the B * selective_keep rows come in pick order and a shape owns any number of
                    # them, so nothing is folded by shape: 'present' is every row's own mask and 'source_row' names its shape
                    pred = _pred
                    pred["sample prior"] = priors
                    pred["pred_seg_mask"] = _seg
                    pred["anchors"] = mean_pp.transpose(1, 2)
                    if selective == "global":
                        present = _valid
                if kept is not None:
                    pred["source_row"], pred["selected"] = kept["source_row"], kept["idx"]
                pred.update({"input": inp, "input_ref": ref, "ref_seg_mask": pcds["ref_seg_mask"], "seg_mask": input_seg_mask,
                             "present": present, "shift": pcds["shift"], "scale": pcds["scale"]})
                pred = {k: v.detach().cpu() for k, v in pred.items()}
                return [(pred, "gen_fixed" + "".join(str(i) for i in fixed_id))]
            # ---- reconstruction ("sample") mode :1085-1134 ----
            if self.cimle:
                noise, _ = self.encoder.sample_noise(pcds, device, h)
                ctx, mean_pp, logvar_pp, _, _, latents = self.encoder(pcds, device, noise=noise)
                part_code, mean, logvar, noise = latents
                seg_mask, valid_id = (t.repeat_interleave(h, dim=0) for t in (seg_mask, valid_id))
            var_pp = torch.exp(logvar_pp)
            Np = mean_pp.shape[-1]
            if self.npoints > Np:                                                               # :1091-1093
                mean_pp, var_pp = (t.repeat_interleave(self.npoints // Np, dim=-1) for t in (mean_pp, var_pp))
                seg_mask = seg_mask.repeat_interleave(self.npoints // Np, dim=-1)
            _pred = self.decode(mean_pp, ctx=ctx, device=device, variance=var_pp, anchor_assignments=seg_mask.to(torch.int32), valid_id=valid_id)
            if self.cimle:
                pred = {}
                for i in range(h):
                    for k, v in _pred.items():
                        pred[f"{k}_sample {i}"] = _fold(v, h)[:, i]
                for i in range(h):
                    priors = torch.randn_like(var_pp).transpose(1, 2) * torch.sqrt(var_pp.transpose(1, 2)) + mean_pp.transpose(1, 2)
                    pred[f"sample prior {i}"] = priors.reshape(B, h, self.npoints, C)[:, i]
                    pred[f"noise latent {i}"] = noise.reshape(B, h, -1)[:, i]
                    pred[f"sample {i} mean"] = mean.reshape(B, h, 3, self.num_anchors)[:, i]
                    pred[f"sample {i} logvar"] = logvar.reshape(B, h, 3, self.num_anchors)[:, i]
                pred["pred"] = _fold(_pred["pred"], h)[:, 0]
                pred["pred_seg_mask"] = _fold(seg_mask, h)[:, 0]
                pred["anchors"] = _fold(mean_pp, h)[:, 0].transpose(1, 2)
                pred["part_latents"] = _fold(part_code, h)[:, 0]
                pred["valid_id"] = _fold(valid_id, h)[:, 0]
            else:
                pred = _pred
                pred["pred_seg_mask"] = seg_mask
                pred["anchors"] = mean_pp.transpose(1, 2)
                pred["sample prior"] = torch.randn_like(var_pp.transpose(1, 2)) * torch.sqrt(var_pp.transpose(1, 2)) + mean_pp.transpose(1, 2)
            pred.update({"input": inp, "input_ref": ref, "ref_seg_mask": pcds["ref_seg_mask"], "seg_mask": input_seg_mask,
                         "token": pcds["token"], "present": valid_id, "shift": pcds["shift"], "scale": pcds["scale"]})
            pred = {k: v.detach().cpu() if isinstance(v, torch.Tensor) else v for k, v in pred.items()}
            return [(pred, "sample")]

    @torch.no_grad()
    def refine(self, pcds, n_steps, parts=None, each=1, device="cuda", seed=None):
        """``each`` variations of every shape of a batch at strength ``n_steps``: the clouds ``pcds["ref"]`` are noised to step n_steps-1 and
        denoised again under the batch's own latents, taken as the reconstruction branch of ``forward`` takes them (the encoder on the
        batch, one aligner noise per shape with cIMLE), in ONE launch (``editing.vary_shape``).  ``parts``: the parts to regenerate, the
        points of the other parts come back untouched; None: the whole cloud.  ``pcds``: a val batch or ``data.PartCloudSet.batch``'s.
        Returns ``vary_shape``'s dict ('pred' (B,each,N,3), 'seg_mask', 'held') + 'input_ref', 'present'."""
        from . import editing
        ref = pcds["ref"].to(device)
        seg_mask = pcds["ref_seg_mask"].to(device)
        valid_id = pcds.get("present", None)
        valid_id = None if valid_id is None else valid_id.to(device)
        if self.cimle:
            noise, _ = self.encoder.sample_noise(pcds, device, 1)
            ctx, _mean_pp, _logvar_pp, _, _, _latents = self.encoder(pcds, device, noise=noise)
        else:
            ctx, _mean_pp, _logvar_pp, _flag, _losses, _latents = self.encoder(pcds, device, epoch=0)
        out = editing.vary_shape(self.diffusion, ctx, seg_mask, ref, n_steps, parts=parts, each=each, valid_id=valid_id, seed=seed)
        out.update({"input_ref": ref, "present": valid_id})
        return out

    # ------------------------------------------------------------------------------------------------------------------
    # Editing modes (anchor_gen.py:206-532).  Each is ONE dfx_compose_latents call (the latent rows of every edit: code lerp /
    # part swap, aligner, anchor edit, seg ids, per-point gathers) and ONE persistent chain launch over all B*K rows (the
    # reference decodes in chunks of 50 rows; the chunking changes nothing but the launch count).  Random draws happen at the
    # reference's sites in its order, torch.randperm included.  The caller's batch is never written to: the reference's
    # in-place writes into pcds["present"] (:231, :494, which reach the caller only when the batch already lives on `device`)
    # are made on a copy, and its permutation of pcds["part_shift"] (:495; the aligner never reads it) is left out — the
    # returned values are the same.
    def _edit_batch(self, pcds, device):
        if not self.cimle:
            # the reference crashes here without cIMLE (noise = None, then None.repeat_interleave: :250, :366)
            _unsupported("the interpolate / drift_anchors editing modes without cimle (the reference's own methods fail there)")
        ref = pcds["ref"].to(device)
        inp = pcds["input"].to(device)
        ref_seg_mask = pcds["ref_seg_mask"].to(device)
        seg_flag = pcds["attn_map"].to(device)
        valid_id = pcds["present"].to(device).to(torch.float32).clone()
        return ref, inp, ref_seg_mask, seg_flag, valid_id

    def _part_code(self, inp, seg_flag):
        m, lv = self.encoder.get_part_code(inp, seg_flag)
        return self.encoder._reparameterize(m, lv) if self.encoder.gen else m.transpose(1, 2)

    def _decode_rows(self, ctx, seg, valid, device):
        return self.decode(None, ctx=ctx, device=device, variance=None, anchor_assignments=seg, valid_id=valid)

    @torch.no_grad()
    def interpolate_latent(self, device, pcds):
        """anchor_gen.py:206-305: part ``interpolate_part_id`` of every shape lerped towards that of a random partner
        (``torch.randperm``) in K = 10 steps, ``dx = linspace(0, 1)`` (both hard-coded in the reference, mirrored).  ``gen``:
        fresh part codes from the flows, the interpolated part marked present, seg ids by rule 0; else the encoded codes
        (reparameterised) and the batch's ``ref_seg_mask`` (seg rule 2).  The ``priors`` draw (:265) is made and dropped like
        the reference's.  Keys: "interpolate sample {i}" (on the CPU, like the reference's chunked outputs), "pred",
        "pred_seg_mask", "ref_seg_mask", "input_ref", "permuted_ref", "permuted_ref_seg_mask", "shift", "scale".  The
        per-point log-variances carry ``log_scale_var`` (0 in every shipped config; the reference leaves it out here, :255) —
        they only feed the dropped priors."""
        from . import editing
        ref, inp, ref_seg_mask, seg_flag, valid_id = self._edit_batch(pcds, device)
        B, J, pid = inp.shape[0], self.num_anchors, self.interpolate_part_id
        noise, _ = self.encoder.sample_noise(pcds, device, 1)
        noise = noise.squeeze(1)
        seg_kw = {}
        if self.gen:
            w = torch.randn(B, self.encoder.zdim, J).to(device)                              # :224 (scaled by sqrt(prior_var) in-kernel)
            if self.encoder.use_flow:
                part_code = self.encoder.sampler().flow_reverse(w)
            else:
                part_code = w * math.sqrt(self.encoder.prior_var)
            valid_id[..., pid] = 1.                                                          # :231
        else:
            part_code = self._part_code(inp, seg_flag)
            Nr = ref_seg_mask.shape[1]
            pred_seg_mask = ref_seg_mask.reshape(-1, Nr, 1).expand(-1, -1, self.npoints // Nr).reshape(-1, self.npoints)   # :237
        K = 10
        dx = torch.linspace(0, 1, steps=K)
        perm = torch.randperm(B)
        rows = editing.repeat_rows(B, K)
        code_a, code_b = editing.interpolation_recipe(B, K, J, pid, perm.numpy())
        if not self.gen:
            seg_kw = {"seg_mode": 2, "seg_src": pred_seg_mask, "seg_row": rows}
        ctx, mean_pp, logvar_pp, seg, valid, _lat = self.encoder.compose_latents(
            part_code, code_a, valid_id.repeat_interleave(K, dim=0), self.npoints, code_b=code_b,
            alpha=editing.interpolation_alpha(B, K, J, pid, dx).to(device), noise_src=noise, noise_row=rows, **seg_kw)
        if self.gen:
            pred_seg_mask = seg.reshape(B, K, -1)[:, 0].to(torch.float32)                   # :232-233 (float ids, like the reference)
        torch.randn_like(logvar_pp)                                                          # :265 priors, never returned
        _pred = self._decode_rows(ctx, seg, valid, device)
        pred = _pred["pred"].cpu().reshape(B, K, self.npoints, 3)
        out = {f"interpolate sample {i}": pred[:, i] for i in range(K)}
        out.update({"pred_seg_mask": pred_seg_mask[:B], "ref_seg_mask": ref_seg_mask, "pred": out["interpolate sample 0"], "input_ref": ref,
                    "permuted_ref": ref[perm.to(ref.device)], "permuted_ref_seg_mask": ref_seg_mask[perm.to(ref.device)],
                    "shift": pcds["shift"], "scale": pcds["scale"]})
        return out

    @torch.no_grad()
    def interpolate_params(self, device, pcds):
        """anchor_gen.py:338-410 (``drift_anchors=True``): every shape K = ``cimle_sample_num`` times with the y anchors of parts 0
        and 2 scaled by sqrt(dx) and their log-variances shifted by log(dx), dx = linspace(1, 5, K) (the reference's constants,
        mirrored); seg ids from the batch (rule 2, so ``ref`` must have ``npoints`` points).  The priors keep the reference's
        formula, noise times the VARIANCE (not the standard deviation, :385).  Keys: "interpolate sample {i}",
        "interpolate sample prior {i}", "pred", "pred_seg_mask", "ref_seg_mask", "seg_mask", "input_ref", "shift", "scale"."""
        from . import editing
        ref, inp, ref_seg_mask, seg_flag, valid_id = self._edit_batch(pcds, device)
        B, J = inp.shape[0], self.num_anchors
        if ref_seg_mask.shape[1] != self.npoints:
            _unsupported("interpolate_params with a reference cloud of other than npoints points (the reference's reshape fails, :395)")
        noise, _ = self.encoder.sample_noise(pcds, device, 1)
        noise = noise.squeeze(1)
        part_code = self._part_code(inp, seg_flag)
        K = self.cimle_sample_num
        scale, shift = editing.drift_factors(B, K, J, torch.linspace(1, 5, steps=K))
        rows = editing.repeat_rows(B, K)
        ctx, mean_pp, logvar_pp, seg, valid, _lat = self.encoder.compose_latents(
            part_code, np.repeat(rows[:, None], J, 1), valid_id.repeat_interleave(K, dim=0), self.npoints, noise_src=noise, noise_row=rows,
            mean_scale=scale.to(device), logvar_shift=shift.to(device), seg_mode=2, seg_src=ref_seg_mask, seg_row=rows)
        var_pp = torch.exp(logvar_pp)
        priors = torch.randn(B * K, self.npoints, 3).to(device) * var_pp.transpose(1, 2) + mean_pp.transpose(1, 2)   # :385
        _pred = self._decode_rows(ctx, seg, valid, device)
        pred = _pred["pred"].reshape(B, K, self.npoints, 3)
        priors = priors.reshape(B, K, self.npoints, 3)
        out = {f"interpolate sample {i}": pred[:, i] for i in range(K)}
        out.update({f"interpolate sample prior {i}": priors[:, i] for i in range(K)})
        out.update({"pred_seg_mask": ref_seg_mask, "ref_seg_mask": ref_seg_mask, "seg_mask": ref_seg_mask, "pred": out["interpolate sample 0"],
                    "input_ref": ref, "shift": pcds["shift"], "scale": pcds["scale"]})
        return out

    @torch.no_grad()
    def combine_latent(self, pcds, device):
        """anchor_gen.py:457-532 (``combine=True``): part i of every shape taken from shape ``perm_i[b]`` (one ``torch.randperm``
        per part), present when both shapes have it (:494), K = ``cimle_sample_num`` aligner noises per shape from
        ``sample_noise``, seg ids by rule 0.  Keys: "{k}_sample_{i}" for every key of decode's dict, "pred", "pred_seg_mask",
        "input_ref", "ref_seg_mask", "input_ref{i}", "ref_seg_mask{i}", "shift", "scale"."""
        from . import editing
        ref = pcds["ref"].to(device)
        inp = pcds["input"].to(device)
        seg_flag = pcds["attn_map"].to(device)
        valid_id = pcds["present"].to(device).to(torch.float32).clone()
        B, J = inp.shape[0], self.num_anchors
        part_code = self._part_code(inp, seg_flag)
        if self.cimle:
            K = self.cimle_sample_num
            noise, _ = self.encoder.sample_noise(pcds, device, K)
            noise = noise.reshape(B * K, -1)
        else:
            K, noise = 1, None
        perms = [torch.randperm(B) for _ in range(J)]                                         # :489-496
        valid = editing.mixing_valid(valid_id, [p.to(device) for p in perms])
        ctx, mean_pp, logvar_pp, seg, valid, _lat = self.encoder.compose_latents(
            part_code, editing.mixing_recipe([p.numpy() for p in perms], K), valid.repeat_interleave(K, dim=0), self.npoints, noise_src=noise)
        _pred = self._decode_rows(ctx, seg, valid, device)
        pred = {}
        for k, v in _pred.items():
            v = _fold(v, K)
            for i in range(K):
                pred[f"{k}_sample_{i}"] = v[:, i]
        pred["pred"] = pred["pred_sample_0"]
        pred["pred_seg_mask"] = seg.reshape(B, K, -1)[:, 0]
        pred["input_ref"] = ref
        pred["ref_seg_mask"] = pcds["ref_seg_mask"]
        for i in range(J):
            pred[f"input_ref{i}"] = ref[perms[i].to(ref.device)]
            pred[f"ref_seg_mask{i}"] = pcds["ref_seg_mask"][perms[i]]
        pred["shift"], pred["scale"] = pcds["shift"], pcds["scale"]
        return pred

    @torch.no_grad()
    def combine_latent_specific(self, inputs, device):
        """anchor_gen.py:412-455, the mixing runner's entry (runner/mixing_runner.py:89): ``inputs`` = one (n_i, 3) point set per
        part, an all-zero set = the part is absent.  The present sets are encoded as ONE shape (PointNetV2 means, no
        reparameterisation), K = ``cimle_sample_num`` aligner noises, seg ids by rule 1 (arange * valid: absent parts map to
        part 0).  Keys: "{k}_sample_{i}", "pred", "input", "pred_seg_mask", "seg_mask", "shift", "scale"."""
        assert len(inputs) == self.num_anchors
        J = self.num_anchors
        present = [bool(torch.any(inp != 0)) for inp in inputs]
        valid_id = torch.tensor([1 if p else 0 for p in present]).to(device).unsqueeze(0)
        eye = torch.eye(J)
        seg_flag = torch.cat([eye[i].reshape(1, J).repeat_interleave(inp.shape[0], dim=0) for i, inp in enumerate(inputs) if present[i]],
                             dim=0).unsqueeze(0).to(device)
        inp = torch.cat([x for x, p in zip(inputs, present) if p], dim=0).unsqueeze(0).to(device)
        m, _lv = self.encoder.get_part_code(inp, seg_flag)
        part_code = m.transpose(1, 2)
        if self.cimle:
            K = self.cimle_sample_num
            noise = torch.randn(K, self.encoder.part_aligner.noise_dim).to(device)            # :426
        else:
            K, noise = 1, None
        ctx, mean_pp, logvar_pp, seg, valid, _lat = self.encoder.compose_latents(
            part_code, np.zeros((K, J), np.int32), valid_id.repeat_interleave(K, dim=0).to(torch.float32), self.npoints, noise_src=noise,
            seg_mode=1)
        _pred = self._decode_rows(ctx, seg, valid, device)
        pred = {}
        for k, v in _pred.items():
            v = _fold(v, K)
            for i in range(K):
                pred[f"{k}_sample_{i}"] = v[:, i]
        pred["pred"] = pred["pred_sample_0"]
        pred["input"] = inp
        pred["pred_seg_mask"] = seg
        pred["seg_mask"] = torch.argmax(seg_flag, dim=2)
        pred["shift"] = torch.zeros(1, 1, 3, device=device)
        pred["scale"] = torch.ones(1, 1, 1, device=device)
        return pred
