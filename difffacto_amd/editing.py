"""Part-level shape editing on explicit part codes: interpolation, part mixing and anchor drift (the paper's editing
applications; the reference's AnchorDiffAE.interpolate_latent / combine_latent / interpolate_params, anchor_gen.py:206-532).

    out = interpolate_part(encoder, diffusion, codes, part_id=2, steps=10)          # (B, steps, npoints, 3) clouds
    out = mix_parts(encoder, diffusion, codes, donors)                              # part j of shape b taken from donors[b, j]
    out = drift_anchors(encoder, diffusion, codes, scale=[1, 2, 3])                 # y anchors of parts 0 / 2 scaled

``codes`` (S, zdim, n_class) are part codes (e.g. the flows' output, or PointNetV2 means of real shapes).  Each helper is one
``dfx_compose_latents`` call (code lerp / swap, aligner, anchor edit, seg ids, per-point gathers) and one ``modules.decode``
(one persistent chain launch over all rows).  ``seed`` / ``generator`` mean what they mean in ``encoders.generate``: the
aligner noise and the chain noise are drawn from ``generator`` (torch's global generator when None), the chain's Philox key
is ``seed`` when given.

Part re-configuration (the reference's tools/shape_edit.py and tools/optimize_noise.py: gradient descent on the aligner's cIMLE
noise) is ``reconfigure_part`` / ``invert_noise``: every row (a shape x a candidate edit x a random start) is an independent
problem, all of them optimized by ONE ``dfx_noise_opt_run`` call, then one ``dfx_compose_latents`` and one chain launch.

    out = reconfigure_part(encoder, diffusion, codes, ref_mean, ref_var, edit_part=0, new_var=v, fix_parts=[0, 1, 1, 1])
    out = invert_noise(encoder, codes, ref_mean, ref_var)                           # the noise that reproduces a configuration

Part-level sampling (the reference's tools/run_sample_one_part.py: AnchorDiffAE.sample_one_part, anchor_gen.py:307-337) is
``sample_part``: new styles for one part of every shape, a search over K aligner noises per style for configurations in which the
other parts stay where they were (or for the first / the most diverse configurations), ONE ``dfx_part_search`` call for all shapes,
one ``dfx_compose_latents`` for the picked rows and one chain launch.

    out = sample_part(encoder, diffusion, codes, valid_id, ref_mean, ref_logvar, part_id=1, how_many_each=50)

The recipe builders below are host-side index bookkeeping (no GPU): rows are ``r = b * K + k`` like the reference's
``repeat_interleave(K, dim=0)``.
"""
import numpy as np
import torch

from .modules import decode


# ---------------------------------------------------------------------------------------------------- recipe builders
def repeat_rows(B, K):
    """Source row of every output row for ``repeat_interleave(K, dim=0)``: (B*K,) int32, r -> r // K."""
    return np.repeat(np.arange(B, dtype=np.int32), K)


def interpolation_recipe(B, K, n_class, part_id, partner):
    """anchor_gen.py:244-247: rows r = b*K + k keep every part of shape b except ``part_id``, which is lerped from shape b towards
    shape ``partner[b]`` with weight dx[k].  -> code_a (B*K, n_class), code_b (B*K, n_class) (-1 = copy code_a)."""
    partner = np.asarray(partner, dtype=np.int64).reshape(B)
    rows = repeat_rows(B, K)
    code_a = np.repeat(rows[:, None], n_class, axis=1).astype(np.int32)
    code_b = np.full((B * K, n_class), -1, np.int32)
    code_b[:, part_id] = partner[rows]
    return code_a, code_b


def interpolation_alpha(B, K, n_class, part_id, dx):
    """(B*K, n_class) lerp weights: dx[k] in column ``part_id`` (the other columns are copies and never read)."""
    dx = torch.as_tensor(dx, dtype=torch.float32).reshape(K)
    alpha = torch.zeros(B * K, n_class, dtype=torch.float32)
    alpha[:, part_id] = dx.repeat(B)
    return alpha


def mixing_recipe(perms, K):
    """anchor_gen.py:489-498: part i of shape b comes from shape ``perms[i][b]``, then every shape is repeated K times.
    -> code_a (B*K, n_class)."""
    perms = np.stack([np.asarray(p, dtype=np.int64) for p in perms], axis=1)        # (B, n_class)
    return np.repeat(perms, K, axis=0).astype(np.int32)


def mixing_valid(valid_id, perms):
    """anchor_gen.py:494: valid[:, i] = valid[perm_i, i] * valid[:, i] (a part is present when the donor has it AND the receiving
    shape has it).  valid_id (B, n_class) -> (B, n_class), a new tensor."""
    out = valid_id.clone()
    for i, p in enumerate(perms):
        p = torch.as_tensor(p, dtype=torch.long, device=valid_id.device)
        out[:, i] = valid_id[p, i] * valid_id[:, i]
    return out


def drift_factors(B, K, n_class, dx, parts=(0, 2), axis=1):
    """anchor_gen.py:369-370: mean[:, axis, parts] *= sqrt(dx), logvar[:, axis, parts] += log(dx), dx[r] = dx[r % K].  Returns the
    (B*K, 3, n_class) factors (1 / 0 elsewhere: exact no-ops) built with torch's sqrt / log."""
    dx = torch.as_tensor(dx, dtype=torch.float32).reshape(1, K).expand(B, -1).reshape(B * K, 1)
    scale = torch.ones(B * K, 3, n_class, dtype=torch.float32)
    shift = torch.zeros(B * K, 3, n_class, dtype=torch.float32)
    parts = list(parts)
    scale[:, axis, parts] = torch.sqrt(dx).expand(-1, len(parts))
    shift[:, axis, parts] = torch.log(dx).expand(-1, len(parts))
    return scale, shift


def seg_ids(valid, npoints, mode=0):
    """Host restatement of the kernel's segment rules 0 / 1 (part_encoders.py:1105-1108; anchor_gen.py:437): (R, npoints) int32."""
    J = valid.shape[1]
    ar = torch.arange(J, device=valid.device)[None]
    ids = ar * valid if mode == 1 else ar * valid + torch.argmax(valid, dim=1, keepdim=True) * (1 - valid)
    return ids.repeat_interleave(npoints // J, dim=1).to(torch.int32)


# ---------------------------------------------------------------------------------------------------- public helpers
def _setup(encoder, codes, valid_id):
    device = next(encoder.parameters()).device
    codes = codes.to(device=device, dtype=torch.float32)
    S, J = codes.shape[0], encoder.n_class
    valid_id = torch.ones(S, J, device=device) if valid_id is None else valid_id.to(device=device, dtype=torch.float32)
    return device, codes, valid_id


def _noise(encoder, n, device, generator):
    al = encoder.part_aligner
    if not al.cimle:
        return None
    return torch.randn(n, al.noise_dim, generator=generator).to(device)


def _run(encoder, diffusion, codes, code_a, valid, npoints, seed, generator, **recipe):
    ctx, mean_pp, logvar_pp, seg, valid, lat = encoder.compose_latents(codes, code_a, valid, npoints, **recipe)
    pred = decode(diffusion, ctx, seg, valid_id=valid, seed=seed, generator=generator)["pred"]
    return pred, seg, mean_pp, valid, lat


@torch.no_grad()
def interpolate_part(encoder, diffusion, codes, part_id, steps, partner=None, valid_id=None, npoints=2048, noise=None, seed=None,
                     generator=None):
    """Lerp part ``part_id`` of every shape b towards shape ``partner[b]`` (default: the next shape, cyclically) in ``steps``
    equal steps from 0 to 1, the other parts fixed; one aligner noise per shape, shared by its steps (``noise`` (B, noise_dim)
    or drawn).  Returns {'pred': (B, steps, npoints, 3), 'seg_mask': (B, steps, npoints), 'anchors': (B, steps, npoints, 3),
    'part_code': (B, steps, zdim, n_class)}."""
    device, codes, valid_id = _setup(encoder, codes, valid_id)
    B, J, K = codes.shape[0], encoder.n_class, int(steps)
    partner = np.roll(np.arange(B), -1) if partner is None else np.asarray(torch.as_tensor(partner).cpu())
    code_a, code_b = interpolation_recipe(B, K, J, part_id, partner)
    alpha = interpolation_alpha(B, K, J, part_id, torch.linspace(0, 1, steps=K)).to(device)
    valid = valid_id.clone()
    valid[:, part_id] = 1.                                                  # the interpolated part exists (anchor_gen.py:231)
    if noise is None:
        noise = _noise(encoder, B, device, generator)
    rows = repeat_rows(B, K)
    pred, seg, mean_pp, valid, lat = _run(encoder, diffusion, codes, code_a, valid.repeat_interleave(K, 0), npoints, seed, generator,
                                          code_b=code_b, alpha=alpha, noise_src=noise, noise_row=None if noise is None else rows)
    return {"pred": pred.reshape(B, K, npoints, 3), "seg_mask": seg.reshape(B, K, npoints),
            "anchors": mean_pp.transpose(1, 2).reshape(B, K, npoints, 3), "part_code": lat[0].reshape(B, K, *codes.shape[1:])}


@torch.no_grad()
def mix_parts(encoder, diffusion, codes, donors, valid_id=None, K=1, npoints=2048, noise=None, seed=None, generator=None):
    """Part j of output shape b comes from shape ``donors[b, j]`` (donors (B, n_class) ints into ``codes``) and is present when
    its donor has it (``AnchorDiffAE.combine_latent`` keeps the reference's stricter rule, ``mixing_valid``).  ``K``
    aligner-noise samples per shape (``noise``
    (B*K, noise_dim) or drawn).  Returns {'pred': (B, K, npoints, 3), 'seg_mask', 'anchors', 'present' (B, n_class)}."""
    device, codes, valid_id = _setup(encoder, codes, valid_id)
    donors = np.asarray(torch.as_tensor(donors).cpu(), dtype=np.int64)
    B, J = donors.shape
    perms = [donors[:, j] for j in range(J)]
    valid = torch.stack([valid_id[torch.as_tensor(donors[:, j], device=device), j] for j in range(J)], 1)
    if noise is None:
        noise = _noise(encoder, B * K, device, generator)
    pred, seg, mean_pp, valid_rows, lat = _run(encoder, diffusion, codes, mixing_recipe(perms, K), valid.repeat_interleave(K, 0),
                                               npoints, seed, generator, noise_src=noise)
    return {"pred": pred.reshape(B, K, npoints, 3), "seg_mask": seg.reshape(B, K, npoints),
            "anchors": mean_pp.transpose(1, 2).reshape(B, K, npoints, 3), "present": valid}


@torch.no_grad()
def drift_anchors(encoder, diffusion, codes, scale, parts=(0, 2), axis=1, valid_id=None, seg_mask=None, npoints=2048, noise=None,
                  seed=None, generator=None):
    """For every factor dx in ``scale`` (K values): the aligner's anchors of ``parts`` on ``axis`` scaled by sqrt(dx) and their
    log-variances shifted by log(dx) (the reference's interpolate_params uses y, parts 0 and 2, dx = linspace(1, 5, K)).  One
    aligner noise per shape (``noise`` (B, noise_dim) or drawn).  ``seg_mask`` (B, npoints) ids: the segmentation to decode with
    (default: npoints // n_class points per present part).  Returns {'pred': (B, K, npoints, 3), 'seg_mask', 'anchors'}."""
    device, codes, valid_id = _setup(encoder, codes, valid_id)
    B, J = codes.shape[0], encoder.n_class
    dx = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
    K = dx.numel()
    s, l = drift_factors(B, K, J, dx, parts, axis)
    if noise is None:
        noise = _noise(encoder, B, device, generator)
    rows = repeat_rows(B, K)
    seg_kw = {} if seg_mask is None else {"seg_mode": 2, "seg_src": seg_mask, "seg_row": rows}
    pred, seg, mean_pp, valid, lat = _run(encoder, diffusion, codes, np.repeat(rows[:, None], J, 1), valid_id.repeat_interleave(K, 0),
                                          npoints, seed, generator, noise_src=noise, noise_row=None if noise is None else rows,
                                          mean_scale=s.to(device), logvar_shift=l.to(device), **seg_kw)
    return {"pred": pred.reshape(B, K, npoints, 3), "seg_mask": seg.reshape(B, K, npoints),
            "anchors": mean_pp.transpose(1, 2).reshape(B, K, npoints, 3)}


# ---------------------------------------------------------------------------------------------------- variations of a given cloud
def held_parts(valid_id, parts, n_class):
    """(B, n_class) 0/1: the parts a variation keeps -- every present part that is not in ``parts`` (``parts=None``: nothing is held, the
    whole cloud is regenerated)."""
    if parts is None:
        return torch.zeros_like(valid_id)
    parts = sorted({int(p) for p in parts})
    if any(not 0 <= p < n_class for p in parts):
        raise ValueError(f"vary_shape: parts {parts} outside [0, {n_class})")
    held = (valid_id != 0).to(valid_id.dtype)
    held[:, parts] = 0
    return held


@torch.no_grad()
def vary_shape(diffusion, ctx, seg, cloud, n_steps, parts=None, each=1, valid_id=None, seed=None, generator=None, ret_interval=None,
               shape_offset=0):
    """``each`` variations of every labelled cloud at strength ``n_steps`` (the usual diffusion recipe: noise to step n_steps-1, denoise
    n_steps steps), ONE ``dfx_refine_chain`` launch over the B*each rows r = b*each + k.  ``ctx`` = [part_code (B,zdim,J), params (B,6,J)] and
    ``seg`` (B,N) are the shapes' context and part ids, ``cloud`` (B,N,3) their points (a data-set shape, a scan, an earlier output).
    ``parts``: the parts to regenerate -- the points of every other present part come back bit for bit (the kernel writes them from
    ``cloud``); None regenerates everything.  Row r draws the Philox noise of global row ``shape_offset + r``, so the variations of a
    shape differ, and a batch split over calls (``shape_offset`` = rows before it) gives the unsplit clouds.
    Returns {'pred': (B, each, N, 3), 'seg_mask': (B, each, N), 'held': (B, J) 0/1} (+ 'traj': (n_keep, B, each, N, 3) with ``ret_interval``)."""
    part_code, params = ctx[0], ctx[1]
    B, J, K = part_code.shape[0], part_code.shape[-1], int(each)
    device = part_code.device
    seg = seg.to(device=device, dtype=torch.int32)
    cloud = cloud.to(device=device, dtype=torch.float32)
    N = seg.shape[1]
    if tuple(cloud.shape) != (B, N, 3):
        raise ValueError(f"vary_shape: cloud (B,N,3) = ({B},{N},3) expected, got {tuple(cloud.shape)}")
    valid_id = torch.ones(B, J, device=device) if valid_id is None else valid_id.to(device=device, dtype=torch.float32)
    held = held_parts(valid_id, parts, J)
    rep = lambda t: t.repeat_interleave(K, 0)
    pred, traj = diffusion.refine_chain([rep(part_code), rep(params)], rep(seg), rep(cloud.transpose(1, 2)), n_steps, valid_id=rep(valid_id),
                                        seed=seed, generator=generator, ret_interval=ret_interval, shape_offset=shape_offset,
                                        hold=rep(held) if parts is not None else None)
    out = {"pred": pred.reshape(B, K, N, 3), "seg_mask": rep(seg).reshape(B, K, N), "held": held}
    if traj is not None:
        out["traj"] = traj.reshape(traj.shape[0], B, K, N, 3)
    return out


# ---------------------------------------------------------------------------------------------------- part-level sampling
def part_sampling_recipe(S, E, P, n_class, part_id):
    """Rows r = (s*E + e)*P + p of the final ``dfx_compose_latents`` call over the source rows [the S shapes | the S*E new styles]:
    every part from shape s except ``part_id``, which is new style s*E + e.  -> code_a (S*E*P, n_class), shape_row (S*E*P,)."""
    group = np.repeat(np.arange(S * E, dtype=np.int32), P)
    shape_row = (group // E).astype(np.int32)
    code_a = np.repeat(shape_row[:, None], n_class, axis=1)
    code_a[:, part_id] = S + group
    return code_a, shape_row


def sample_part_latents(encoder, codes, valid_id, ref_mean, ref_logvar, part_id, how_many_each, fix_size=True, param_sample_num=1,
                        selective=False, K=100, seg_mask=None, npoints=2048, noise=None, seed=None, generator=None, row_budget=0):
    """``sample_part`` up to the chain: the draws, the new styles, the candidate search and the composed rows.  Returns
    (``encoder.compose_latents``' 6-tuple, search dict with idx (S,E,P), scores, n_bad, P)."""
    from .encoders import _unsupported
    al = encoder.part_aligner
    if al is None or not al.cimle:
        _unsupported("part-level sampling without a cIMLE part aligner (there are no candidate noises to search)")
    device, codes, valid_id = _setup(encoder, codes, valid_id)
    S, J, E, K = codes.shape[0], encoder.n_class, int(how_many_each), int(K)
    if not 0 <= int(part_id) < J:
        raise ValueError(f"sample_part: part_id {part_id} outside [0, {J})")
    if fix_size:                                                          # part_encoders.py:661-663
        param_sample_num, selective = 1, False
    P = int(param_sample_num)
    if not 1 <= P <= K:
        raise ValueError(f"sample_part: param_sample_num {P} outside [1, K = {K}]")
    if noise is None:                                                     # the reference's order: w (:655), then per shape (:669)
        w = torch.randn(S * E, encoder.zdim, generator=generator)
        z = torch.cat([torch.randn(E * K, al.noise_dim, generator=generator) for _ in range(S)])
    else:
        w, z = noise
    w, z = w.to(device=device, dtype=torch.float32), z.to(device=device, dtype=torch.float32)
    sampler = encoder.sampler()
    new_code = sampler.flow_reverse_part(part_id, w, scale_prior=False) if encoder.use_flow else w.contiguous()      # :656-659
    G = S * E
    group_shape = repeat_rows(S, E)
    valid_g = valid_id.repeat_interleave(E, 0)
    kw = {}
    if fix_size:
        mode = "fit"
        f32 = lambda t: torch.as_tensor(t).to(device=device, dtype=torch.float32).reshape(S, 3, J).repeat_interleave(E, 0)
        weight = valid_g.clone()
        weight[:, part_id] = 0.0                                          # :680
        kw = {"target_mean": f32(ref_mean), "target_logvar": f32(ref_logvar), "weight": weight}
    elif selective:
        mode = "diverse"
        kw = {"seed": int(seed) if seed is not None else int(torch.randint(0, 2 ** 62, (), generator=generator))}
    else:
        mode = "first"
    found = sampler.part_search(codes, np.repeat(group_shape[:, None], J, 1), valid_g, z, K, mode, P=P, new_code=new_code,
                                new_part=int(part_id), row_budget=row_budget, return_scores=True, **kw)
    # the S*E*P final rows: the new styles as extra source rows, the picked noises as noise_src, the shapes' own segmentation
    extra = codes.new_zeros(G, encoder.zdim, J)
    extra[:, :, part_id] = new_code
    code_a, shape_row = part_sampling_recipe(S, E, P, J, int(part_id))
    seg_kw = {} if seg_mask is None else {"seg_mode": 2, "seg_src": seg_mask, "seg_row": shape_row}
    lat = encoder.compose_latents(torch.cat([codes, extra]), code_a, valid_g.repeat_interleave(P, 0), npoints, noise_src=found["noise"],
                                  **seg_kw)
    found["idx"] = found["idx"].reshape(S, E, P)
    return lat, found, P


@torch.no_grad()
def sample_part(encoder, diffusion, codes, valid_id, ref_mean, ref_logvar, part_id, how_many_each, fix_size=True, param_sample_num=1,
                selective=False, K=100, seg_mask=None, npoints=2048, noise=None, seed=None, generator=None, row_budget=0):
    """Keep every shape of ``codes`` (S,zdim,J), draw ``how_many_each`` = E new styles for part ``part_id`` and let the aligner find
    configurations for them among K noises per style (AnchorDiffAE.sample_one_part, anchor_gen.py:307-337;
    PartEncoder.sample_with_fixed_latents, part_encoders.py:623-710):

    * ``fix_size=True`` (P = 1): the noise whose parameters of the OTHER present parts are closest to the shape's own ``ref_mean`` /
      ``ref_logvar`` (S,3,J): the untouched parts stay where they were (:677-682);
    * ``fix_size=False``: P = ``param_sample_num`` configurations per style: the first P noises, or with ``selective`` the P most
      diverse ones by the greedy rule of ``subsample_params`` (:545-589; its 512 unit draws per candidate come from Philox keyed by
      ``seed``, or by a key drawn from ``generator``).

    Deviations from the reference's letter: K is a parameter (hard-coded 100 at :664); the two ``fix_size=False`` branches raise in
    the reference (a boolean mask / a Python list where ``gather_operation`` needs indices, :685-690) and follow their evident intent
    here, the selective one with each shape's own validity mask (the reference passes column 0 of the batch's).

    The host draws come in the reference's order (w (S*E,zdim), then (E*K,noise_dim) per shape), so one ``torch.manual_seed``
    reproduces its latents; ``noise`` = (w, z (S*E*K,noise_dim)) supplies them instead.  ``seg_mask`` (S,npoints) ids: the shapes' own
    segmentation (default: npoints // J points per present part).  ``row_budget``: candidate rows the aligner sees at once (0 = the
    library's default).  Returns the keys of ``LatentSampler.sample_latents`` over the S*E*P rows r = (s*E + e)*P + p, and 'pred'
    (S,E,P,npoints,3), 'idx' (S,E,P) the picked noise of every row, 'scores' ((S*E,K) fit sums / (S*E*K,6,J) diverse scores / None),
    'n_bad' (candidates with a non-finite score)."""
    lat, found, P = sample_part_latents(encoder, codes, valid_id, ref_mean, ref_logvar, part_id, how_many_each, fix_size, param_sample_num,
                                        selective, K, seg_mask, npoints, noise, seed, generator, row_budget)
    ctx, mean_pp, logvar_pp, seg, valid, (part_code, mean, logvar, z) = lat
    pred = decode(diffusion, ctx, seg, valid_id=valid, seed=seed, generator=generator)["pred"]
    S, E = found["idx"].shape[:2]
    return {"part_code": part_code, "valid_id": valid, "noise": z, "mean": mean, "logvar": logvar, "params": ctx[1], "seg_mask": seg,
            "mean_per_point": mean_pp, "logvar_per_point": logvar_pp, "pred": pred.reshape(S, E, P, npoints, 3), "idx": found["idx"],
            "scores": found["scores"], "n_bad": found["n_bad"]}


# ---------------------------------------------------------------------------------------------------- aligner-noise optimization
# constants of tools/shape_edit.py:83-85,126 (Adam defaults, ReduceLROnPlateau(factor 0.5, patience 10, min_lr 5e-2), torch.allclose) and of
# edit_latent's call there (fit_weight 0.05); reg_weight = AnchorDiffAE's reg_loss_weight default
NOISE_OPT_DEFAULTS = {"fit_weight": 0.05, "reg_weight": 1.0, "lr0": 1.0, "beta1": 0.9, "beta2": 0.999, "adam_eps": 1e-8, "factor": 0.5,
                      "threshold": 1e-4, "min_lr": 5e-2, "lr_eps": 1e-8, "stop_atol": 1e-8, "stop_rtol": 1e-5, "patience": 10}


def noise_problem(valid, ref_mean, ref_var, fix_parts, edit_part, new_mean=None, new_var=None, fit_weight=0.05, reg_weight=1.0, **constants):
    """Targets and masks of ``LatentSampler.optimize_noise`` for R rows, the terms of ``AnchorDiffAE.edit_latent`` (anchor_gen.py:877-892) per row:

        fit  = sum(f * ((mean - ref_mean)^2 + (logvar - log ref_var)^2)) / sum(f),   f = valid * fix_parts          (:877-879)
        edit = mse(mean[..., edit_part], new_mean) + mse(logvar[..., edit_part], log new_var)   (each absent when None)   (:880-888)

    valid (R,J) 0/1; ref_mean / ref_var (R,3,J); fix_parts (J,) or (R,J) 0/1 (the reference's ``fix_ids``); edit_part an int, (R,) ints or None
    (no edit term: ``optimize_latent``'s objective with fix_parts all ones); new_mean / new_var (3,) or (R,3).  Host tensors (fp32).
    ValueError for an edited part that is absent and for a row without any fixed present part (the reference divides by zero there).  Where
    f = 0 the fit target is set to 0 (the reference multiplies log(ref_var) of an absent part by 0: NaN when that variance is 0)."""
    f32 = lambda a: torch.as_tensor(a).detach().cpu().to(torch.float32)
    valid, ref_mean, ref_var = f32(valid), f32(ref_mean), f32(ref_var)
    R, J = valid.shape
    if tuple(ref_mean.shape) != (R, 3, J) or tuple(ref_var.shape) != (R, 3, J):
        raise ValueError(f"noise_problem: ref_mean / ref_var (R,3,J) = ({R},3,{J}) expected")
    fix = valid * f32(fix_parts).reshape(-1, J).expand(R, J)
    if bool((fix.sum(1) == 0).any()):
        raise ValueError("noise_problem: a row has no fixed part that is present (the fit term would divide by zero)")
    keep = fix[:, None, :].expand(R, 3, J) != 0
    unknown = set(constants) - set(NOISE_OPT_DEFAULTS)
    if unknown:
        raise TypeError(f"noise_problem: unknown constants {sorted(unknown)}")
    p = {"fit_mean": torch.where(keep, ref_mean, torch.zeros(())), "fit_logvar": torch.where(keep, torch.log(torch.where(keep, ref_var, torch.ones(()))), torch.zeros(())),
         "fix": fix, "fit_weight": float(fit_weight), "reg_weight": float(reg_weight), **constants}
    if edit_part is None:
        if new_mean is not None or new_var is not None:
            raise ValueError("noise_problem: an edit target without edit_part")
        return p
    ep = torch.as_tensor(edit_part).reshape(-1).expand(R).long()
    if bool(((ep < 0) | (ep >= J)).any()) or bool((valid[torch.arange(R), ep] == 0).any()):
        raise ValueError("noise_problem: the edited part is absent (or its id is out of range)")
    sel = torch.zeros(R, J)
    sel[torch.arange(R), ep] = 1.0
    for name, tgt, key, selkey in (("new_mean", new_mean, "edit_mean", "edit_mean_sel"), ("new_var", new_var, "edit_logvar", "edit_var_sel")):
        if tgt is None:
            continue
        t = f32(tgt).reshape(-1, 3).expand(R, 3)
        full = torch.zeros(R, 3, J)
        full[torch.arange(R), :, ep] = torch.log(t) if name == "new_var" else t
        p[key], p[selkey] = full, sel.clone()
    return p


def noise_losses(problem, mean, logvar, z):
    """The per-row loss terms of ``noise_problem`` at (mean, logvar, z) in torch (any device / dtype; the formulas k_edit_loss implements):
    dict L, fit, edit, reg, each (R,)."""
    g = lambda k: None if problem.get(k) is None else torch.as_tensor(problem[k]).to(mean)
    f = g("fix")[:, None, :]
    fit = (f * ((mean - g("fit_mean")) ** 2 + (logvar - g("fit_logvar")) ** 2)).sum((1, 2)) / g("fix").sum(1)
    edit = torch.zeros_like(fit)
    if g("edit_mean_sel") is not None:
        edit = edit + (g("edit_mean_sel")[:, None, :] * (mean - g("edit_mean")) ** 2).sum((1, 2)) / 3
    if g("edit_var_sel") is not None:
        edit = edit + (g("edit_var_sel")[:, None, :] * (logvar - g("edit_logvar")) ** 2).sum((1, 2)) / 3
    reg = (z.to(mean) ** 2).sum(1)
    c = {**NOISE_OPT_DEFAULTS, **{k: v for k, v in problem.items() if k in NOISE_OPT_DEFAULTS}}
    return {"L": c["fit_weight"] * fit + edit + c["reg_weight"] * reg, "fit": fit, "edit": edit, "reg": reg}


def noise_opt_replay(losses, grads, z0, **constants):
    """Float64 restatement of ONE row of k_noise_step (noise_opt.hip): ``torch.optim.Adam`` defaults driven by the gradient sequence
    ``grads`` (K, noise_dim), then ``ReduceLROnPlateau(mode min, threshold mode rel, cooldown 0)`` and the ``torch.allclose`` stop rule driven
    by the loss sequence ``losses`` (K,).  The oracle of the kernel's trace (fed with the traced losses and gradients) and, on the CPU, checked
    against torch's own optimizer and scheduler.  Returns dict: z (n+1, noise_dim) (z[k] = before step k; z[n] = the result), lr (n,) the rate
    of step k, reduced_at (iterations whose scheduler step lowered the rate), stopped_at (iteration or None), n = iterations run."""
    c = {**NOISE_OPT_DEFAULTS, **constants}
    losses, grads = np.asarray(losses, np.float64), np.asarray(grads, np.float64)
    z = np.asarray(z0, np.float64).reshape(-1).copy()
    m, v = np.zeros_like(z), np.zeros_like(z)
    lr, best, prev, bad = float(c["lr0"]), float("inf"), 0.0, 0
    zs, lrs, reduced, stopped = [z.copy()], [], [], None
    for k in range(len(losses)):
        g, L = grads[k], float(losses[k])
        m = m + (1 - c["beta1"]) * (g - m)
        v = v * c["beta2"] + (1 - c["beta2"]) * g * g
        bc1, bc2 = 1 - c["beta1"] ** (k + 1), 1 - c["beta2"] ** (k + 1)
        z = z - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + c["adam_eps"]))
        lrs.append(lr)
        zs.append(z.copy())
        if L < best * (1.0 - c["threshold"]):
            best, bad = L, 0
        else:
            bad += 1
        if bad > c["patience"]:
            new = max(lr * c["factor"], c["min_lr"])
            if lr - new > c["lr_eps"]:
                lr = new
                reduced.append(k)
            bad = 0
        if abs(L - prev) <= c["stop_atol"] + c["stop_rtol"] * abs(prev):
            stopped = k
            break
        prev = L
    return {"z": np.stack(zs), "lr": np.asarray(lrs), "reduced_at": reduced, "stopped_at": stopped, "n": len(lrs)}


def _optimize_rows(encoder, diffusion, codes, problem_of, valid_id, shape_row, z0, max_iter, npoints, seed, generator, trace):
    device, codes, valid_id = _setup(encoder, codes, valid_id)
    S, J = codes.shape[0], encoder.n_class
    rows = np.arange(S, dtype=np.int32) if shape_row is None else np.asarray(torch.as_tensor(shape_row).cpu(), dtype=np.int32).reshape(-1)
    if rows.size == 0 or rows.min() < 0 or rows.max() >= S:
        raise ValueError(f"shape_row: indices into the {S} source shapes expected")
    idx = torch.as_tensor(rows, dtype=torch.long, device=device)
    valid = valid_id[idx].contiguous()
    problem = problem_of(idx.cpu(), valid.cpu())
    if z0 is None:
        z0 = _noise(encoder, len(rows), device, generator)
    opt = encoder.sampler().optimize_noise(codes[idx], valid, z0, problem, max_iter, trace=trace)
    out = {"z": opt["z"], "mean": opt["mean"], "logvar": opt["logvar"], "iters_done": opt["iters_done"], "trace": opt["trace"],
           "losses": noise_losses(problem, opt["mean"], opt["logvar"], opt["z"]), "problem": problem}
    if diffusion is not None:
        pred, seg, mean_pp, _valid, _lat = _run(encoder, diffusion, codes, np.repeat(rows[:, None], J, 1), valid, npoints, seed, generator,
                                                noise_src=opt["z"])
        out.update({"pred": pred, "seg_mask": seg, "anchors": mean_pp.transpose(1, 2)})
    return out


@torch.no_grad()
def reconfigure_part(encoder, diffusion, codes, ref_mean, ref_var, edit_part, new_mean=None, new_var=None, fix_parts=None, valid_id=None,
                     shape_row=None, z0=None, max_iter=300, fit_weight=0.05, reg_weight=1.0, npoints=2048, seed=None, generator=None,
                     trace=False, **constants):
    """Edit one part's position (``new_mean``) and / or size (``new_var``) and let the other parts re-arrange themselves: the reference's
    tools/shape_edit.py, for R rows at once.  Row r edits shape ``shape_row[r]`` of ``codes`` (S,zdim,J) (default: one row per shape), so rows
    can be several shapes x several candidate edits x several random starts; ``ref_mean`` / ``ref_var`` (S,3,J) are the shapes' own part
    parameters, ``fix_parts`` (J,) / (R,J) 0/1 the parts held to them (default: every part but the edited one), ``edit_part`` an int or (R,),
    ``new_mean`` / ``new_var`` (3,) or (R,3), ``z0`` (R,noise_dim) the start (drawn when None).  Rows do not see each other (the reference's
    batch mean would couple them).  ONE optimizer call, one ``dfx_compose_latents`` with the optimized noise rows, ONE chain launch.
    Returns dict: z (R,noise_dim), mean / logvar (R,3,J) at z, iters_done (R,), losses {L, fit, edit, reg} (R,) at z, trace, problem, and
    pred (R,npoints,3), seg_mask (R,npoints), anchors (R,npoints,3) (omitted with ``diffusion=None``)."""
    J = encoder.n_class

    def problem_of(idx, valid):
        ep = torch.as_tensor(edit_part).reshape(-1).expand(len(idx)).long()
        fix = fix_parts
        if fix is None:
            fix = torch.ones(len(idx), J)
            fix[torch.arange(len(idx)), ep] = 0.0
        return noise_problem(valid, torch.as_tensor(ref_mean).cpu()[idx], torch.as_tensor(ref_var).cpu()[idx], fix, ep, new_mean, new_var,
                             fit_weight=fit_weight, reg_weight=reg_weight, **constants)

    return _optimize_rows(encoder, diffusion, codes, problem_of, valid_id, shape_row, z0, max_iter, npoints, seed, generator, trace)


@torch.no_grad()
def invert_noise(encoder, codes, ref_mean, ref_var, diffusion=None, valid_id=None, shape_row=None, z0=None, max_iter=300, fit_weight=1.0,
                 reg_weight=1.0, npoints=2048, seed=None, generator=None, trace=False, **constants):
    """The aligner noise under which a shape's part codes give its own configuration ``ref_mean`` / ``ref_var`` (S,3,J): the reference's
    tools/optimize_noise.py (``optimize_latent``'s fit + reg objective over the present parts), rows as in ``reconfigure_part`` (several random
    starts per shape through ``shape_row``).  Returns ``reconfigure_part``'s dict (clouds only with a ``diffusion``)."""
    def problem_of(idx, valid):
        return noise_problem(valid, torch.as_tensor(ref_mean).cpu()[idx], torch.as_tensor(ref_var).cpu()[idx], torch.ones(valid.shape[1]), None,
                             fit_weight=fit_weight, reg_weight=reg_weight, **constants)

    return _optimize_rows(encoder, diffusion, codes, problem_of, valid_id, shape_row, z0, max_iter, npoints, seed, generator, trace)
