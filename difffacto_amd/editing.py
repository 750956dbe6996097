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
