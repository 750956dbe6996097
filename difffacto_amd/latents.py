"""Host-side driver of libdfx's latent sampler: owns the opaque ``dfx_latents`` handle.

    ls = LatentSampler(params, n_class=4, zdim=256, n_heads=8, d_head=32, noise_scale=100.0)
    out = ls.sample_latents(w_noise, aligner_noise, valid_id, fixed_id, K=10, npoints=2048)

``params`` maps the reference ``state_dict`` names relative to ``encoder.`` (``flow.{i}.chain.{l}.net_s_t.{0,2,4}.*``,
``part_aligner.*``; python/difffacto/models/encoders/flow.py:9-19, part_encoders.py:52-86) to fp32 tensors.
PyTorch is used for device memory and the stream only; the random draws are inputs.
"""
import ctypes

import numpy as np
import torch

from . import _ffi

_BLOCK_FIELDS = {
    "norm2_w": "norm2.weight", "norm2_b": "norm2.bias", "to_q": "attn2.to_q.weight", "to_k": "attn2.to_k.weight",
    "to_v": "attn2.to_v.weight", "to_out_w": "attn2.to_out.0.weight", "to_out_b": "attn2.to_out.0.bias",
    "norm3_w": "norm3.weight", "norm3_b": "norm3.bias", "ff_proj_w": "ff.net.0.proj.weight",
    "ff_proj_b": "ff.net.0.proj.bias", "ff_out_w": "ff.net.2.weight", "ff_out_b": "ff.net.2.bias",
}
_TOP_FIELDS = {
    "proj_in_w": "proj_in.weight", "proj_in_b": "proj_in.bias", "class_emb": "class_emb.weight",
    "pre_norm_w": "pre_norm.weight", "pre_norm_b": "pre_norm.bias", "post_norm_w": "post_norm.weight",
    "post_norm_b": "post_norm.bias", "proj_out_w": "proj_out.weight", "proj_out_b": "proj_out.bias",
}
_FLOW_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")


class LatentSampler:
    def __init__(self, params, n_class=4, zdim=256, n_heads=8, d_head=32, cimle=True, noise_dim=32,
                 noise_scale=10.0, prior_var=1.0, log_scale_var=0.0, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("LatentSampler needs a HIP device (there is no CPU path)")
        self.device = torch.device(device if device is not None else "cuda")
        self.n_class, self.zdim, self.noise_dim, self.cimle = int(n_class), int(zdim), int(noise_dim), bool(cimle)
        inner = n_heads * d_head
        flow_depth = 0
        while f"flow.0.chain.{flow_depth}.net_s_t.0.weight" in params:
            flow_depth += 1
        depth = 0
        while f"part_aligner.transformer_blocks.{depth}.norm2.weight" in params:
            depth += 1
        if not 1 <= depth <= _ffi.DFX_MAX_DEPTH:
            raise RuntimeError(f"unsupported aligner depth {depth}")
        keep = []

        def dev(key, shape=None):
            t = params[key]
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t))
            t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
            keep.append((key, t))
            return t.data_ptr()

        w = _ffi.LatentWeights()
        w.n_class, w.zdim, w.flow_depth = self.n_class, self.zdim, flow_depth
        half = zdim // 2
        flow_ptrs = None
        hidden = 0
        if flow_depth:
            hidden = int(params["flow.0.chain.0.net_s_t.0.weight"].shape[0])
            shapes = ((hidden, half), (hidden,), (hidden, hidden), (hidden,), (2 * half, hidden), (2 * half,))
            flow_ptrs = (_ffi.c_fp * (self.n_class * flow_depth * 6))()
            for p in range(self.n_class):
                for l in range(flow_depth):
                    for k, (suffix, shp) in enumerate(zip(_FLOW_KEYS, shapes)):
                        flow_ptrs[(p * flow_depth + l) * 6 + k] = dev(f"flow.{p}.chain.{l}.net_s_t.{suffix}", shp)
            w.flow = ctypes.cast(flow_ptrs, ctypes.POINTER(_ffi.c_fp))
        w.flow_hidden = hidden
        w.depth, w.n_heads, w.d_head = depth, int(n_heads), int(d_head)
        w.cimle, w.noise_dim = int(self.cimle), self.noise_dim
        w.noise_scale, w.prior_var, w.log_scale_var = float(noise_scale), float(prior_var), float(log_scale_var)
        in_ch = zdim + (noise_dim if cimle else 0)
        top_shapes = {"proj_in_w": (inner, in_ch), "class_emb": (self.n_class, inner), "proj_out_w": (6, inner)}
        for field, key in _TOP_FIELDS.items():
            setattr(w, field, dev("part_aligner." + key, top_shapes.get(field)))
        blk_shapes = {"to_q": (inner, inner), "to_k": (inner, inner), "to_v": (inner, inner), "to_out_w": (inner, inner),
                      "ff_proj_w": (8 * inner, inner), "ff_out_w": (inner, 4 * inner)}
        for b in range(depth):
            for field, key in _BLOCK_FIELDS.items():
                setattr(w.blocks[b], field, dev(f"part_aligner.transformer_blocks.{b}.{key}", blk_shapes.get(field)))
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_latents_create(ctypes.byref(handle), ctypes.byref(w), _ffi.current_stream())
        _ffi.check(rc, "dfx_latents_create")
        # create() synchronised the stream and packed its own copies.  The aligner's plain fp32 tensors stay, for the entry point that takes
        # dfx_latent_weights directly (optimize_noise: the exact-fp32 training kernels); the flows are not needed there
        w.flow, w.flow_depth = None, 0
        self._w, self._keep = w, [t for key, t in keep if key.startswith("part_aligner.")]
        del keep, flow_ptrs
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().dfx_latents_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _f(self, t):
        return None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def flow_reverse(self, w):
        """w (S,zdim,n_class) standard normal -> part_code (S,zdim,n_class) (part_encoders.py:1054-1060)."""
        w = self._f(w)
        S = w.shape[0]
        assert tuple(w.shape) == (S, self.zdim, self.n_class)
        out = torch.empty_like(w)
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_flow_reverse(self._h, _ffi.ptr(w), _ffi.ptr(out), S, _ffi.current_stream())
        _ffi.check(rc, "dfx_flow_reverse")
        return out

    def part_aligner(self, part_code, valid_id, noise=None):
        """PartAlignerTransformer.forward (part_encoders.py:88-109) -> mean (B,3,J), logvar (B,3,J)."""
        part_code, valid_id, noise = self._f(part_code), self._f(valid_id), self._f(noise)
        B = part_code.shape[0]
        assert tuple(part_code.shape) == (B, self.zdim, self.n_class) and tuple(valid_id.shape) == (B, self.n_class)
        if noise is not None:
            assert tuple(noise.shape) == (B, self.noise_dim)
        mean = torch.empty(B, 3, self.n_class, dtype=torch.float32, device=self.device)
        logvar = torch.empty_like(mean)
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_part_aligner(self._h, _ffi.ptr(part_code), _ffi.ptr(valid_id), _ffi.ptr(noise),
                                             _ffi.ptr(mean), _ffi.ptr(logvar), B, _ffi.current_stream())
        _ffi.check(rc, "dfx_part_aligner")
        return mean, logvar

    def sample_latents(self, w_noise, aligner_noise, valid_id, fixed_id=None, K=1, npoints=2048, part_code=None):
        """Everything of sample_latents after the random draws (part_encoders.py:1052-1110); dict of tensors with
        R = S*K rows: part_code, valid_id, noise, mean, logvar, params (= ctx[1]), seg_mask, mean_per_point,
        logvar_per_point."""
        w_noise, part_code, aligner_noise, valid_id = map(self._f, (w_noise, part_code, aligner_noise, valid_id))
        S = valid_id.shape[0]
        J, Z, R = self.n_class, self.zdim, S * int(K)
        for t in (w_noise, part_code):
            assert t is None or tuple(t.shape) == (S, Z, J)
        if aligner_noise is not None:
            assert tuple(aligner_noise.shape) == (R, self.noise_dim)
        fid = (ctypes.c_int32 * J)(*([0] * J if fixed_id is None else [int(v) for v in fixed_id]))
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=self.device)
        out = {"part_code": e(R, Z, J), "valid_id": e(R, J), "noise": e(R, self.noise_dim) if self.cimle else None,
               "mean": e(R, 3, J), "logvar": e(R, 3, J), "params": e(R, 6, J), "seg_mask": e(R, npoints, dtype=torch.int32),
               "mean_per_point": e(R, 3, npoints), "logvar_per_point": e(R, 3, npoints)}
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_sample_latents(
                self._h, _ffi.ptr(w_noise), _ffi.ptr(part_code), _ffi.ptr(aligner_noise), _ffi.ptr(valid_id), fid, S,
                int(K), int(npoints), _ffi.ptr(out["part_code"]), _ffi.ptr(out["valid_id"]), _ffi.ptr(out["noise"]),
                _ffi.ptr(out["mean"]), _ffi.ptr(out["logvar"]), _ffi.ptr(out["params"]), _ffi.ptr(out["seg_mask"]),
                _ffi.ptr(out["mean_per_point"]), _ffi.ptr(out["logvar_per_point"]), _ffi.current_stream())
        _ffi.check(rc, "dfx_sample_latents")
        return out

    def compose_latents(self, code_src, code_a, valid, code_b=None, alpha=None, noise_src=None, noise_row=None, mean_scale=None,
                        logvar_shift=None, seg_mode=0, seg_src=None, seg_row=None, npoints=2048):
        """The editing front end (``dfx_compose_latents``): ``sample_latents``' dict from an explicit recipe over S source codes.

        code_src (S,zdim,J); code_a / code_b (R,J) source rows per output row and part (host ints; code_b -1 or None = copy code_a)
        with alpha (R,J) the lerp weights; valid (R,J) the final key mask; noise_src (Sn,noise_dim) + noise_row (R,) (None =
        identity); mean_scale / logvar_shift (R,3,J) anchor edits after the aligner; seg_mode 0 / 1 / 2 (seg_src (Ss,npoints)
        ids + seg_row (R,) for mode 2).  Returns the keys of ``sample_latents``; ``valid_id`` is ``valid``."""
        host = lambda a: None if a is None else np.ascontiguousarray(
            (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.int32))
        code_a, code_b, noise_row, seg_row = map(host, (code_a, code_b, noise_row, seg_row))
        code_src, valid, alpha, noise_src, mean_scale, logvar_shift = map(
            self._f, (code_src, valid, alpha, noise_src, mean_scale, logvar_shift))
        J, Z = self.n_class, self.zdim
        S, R = code_src.shape[0], code_a.shape[0]
        assert tuple(code_src.shape) == (S, Z, J) and code_a.shape == (R, J) and tuple(valid.shape) == (R, J)
        for t, shape in ((code_b, (R, J)), (noise_row, (R,)), (seg_row, (R,))):
            assert t is None or t.shape == shape
        for t in (alpha, mean_scale, logvar_shift):
            assert t is None or t.numel() == R * J * (1 if t is alpha else 3)
        Sn = 0 if noise_src is None else noise_src.shape[0]
        if noise_src is not None:
            assert tuple(noise_src.shape) == (Sn, self.noise_dim)
        Ss = 0
        if seg_src is not None:
            seg_src = seg_src.detach().to(device=self.device, dtype=torch.int32).contiguous()
            Ss = seg_src.shape[0]
            assert tuple(seg_src.shape) == (Ss, npoints)
            if bool(((seg_src < 0) | (seg_src >= J)).any()):
                raise ValueError(f"compose_latents: segment ids outside [0, {J})")
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=self.device)
        out = {"part_code": e(R, Z, J), "valid_id": valid, "noise": e(R, self.noise_dim) if self.cimle else None,
               "mean": e(R, 3, J), "logvar": e(R, 3, J), "params": e(R, 6, J), "seg_mask": e(R, npoints, dtype=torch.int32),
               "mean_per_point": e(R, 3, npoints), "logvar_per_point": e(R, 3, npoints)}
        hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_compose_latents(
                self._h, _ffi.ptr(code_src), S, hp(code_a), hp(code_b), _ffi.ptr(alpha), _ffi.ptr(valid), _ffi.ptr(noise_src), Sn,
                hp(noise_row), _ffi.ptr(mean_scale), _ffi.ptr(logvar_shift), int(seg_mode), _ffi.ptr(seg_src), Ss, hp(seg_row), R,
                int(npoints), _ffi.ptr(out["part_code"]), _ffi.ptr(out["noise"]), _ffi.ptr(out["mean"]), _ffi.ptr(out["logvar"]),
                _ffi.ptr(out["params"]), _ffi.ptr(out["seg_mask"]), _ffi.ptr(out["mean_per_point"]),
                _ffi.ptr(out["logvar_per_point"]), _ffi.current_stream())
        _ffi.check(rc, "dfx_compose_latents")
        return out

    def flow_reverse_part(self, part, w, scale_prior=True):
        """flow[part](w, reverse=True) (part_encoders.py:655-659): w (R,zdim) standard normal -> (R,zdim) codes of that part.
        ``scale_prior``: scale w by sqrt(prior_var) first, as ``flow_reverse`` does (the reference's :655 does not)."""
        w = self._f(w)
        R = w.shape[0]
        assert tuple(w.shape) == (R, self.zdim)
        out = torch.empty_like(w)
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_flow_reverse_part(self._h, int(part), _ffi.ptr(w), int(bool(scale_prior)), _ffi.ptr(out), R,
                                                  _ffi.current_stream())
        _ffi.check(rc, "dfx_flow_reverse_part")
        return out

    def part_search(self, code_src, code_a, valid, noise, K, mode, P=1, new_code=None, new_part=-1, target_mean=None,
                    target_logvar=None, weight=None, stats=None, seed=0, row0=0, n_draws=512, row_budget=0, return_scores=False):
        """``dfx_part_search``: for G groups of K aligner noises each, the aligner over chunks of whole groups of at most ``row_budget``
        candidate rows (0 = the library's default), the selection ``mode`` ('fit' / 'first' / 'diverse') and the P picks per group.

        code_src (S,zdim,J) + code_a (G,J) host ints: the source row of every part of a group; new_code (G,zdim) replaces part
        ``new_part``; valid (G,J); noise (G K,noise_dim); fit: target_mean / target_logvar (G,3,J), weight (G,J); diverse: stats
        (G K,4,3,J) or None (Philox from ``seed``, global rows from ``row0``).  Returns dict: idx (G,P) int32, noise (G P,noise_dim),
        mean / logvar (G P,3,J), scores ((G K,6,J) diverse, (G,K) fit; None unless ``return_scores``), n_bad (1,) int32."""
        from . import part_sampling
        mode = part_sampling.MODES[mode] if isinstance(mode, str) else int(mode)
        code_a = np.ascontiguousarray((code_a.detach().cpu().numpy() if isinstance(code_a, torch.Tensor) else np.asarray(code_a)).astype(np.int32))
        code_src, valid, noise, new_code, target_mean, target_logvar, weight, stats = map(
            self._f, (code_src, valid, noise, new_code, target_mean, target_logvar, weight, stats))
        J, Z, ND = self.n_class, self.zdim, self.noise_dim
        S, G, K, P = code_src.shape[0], code_a.shape[0], int(K), int(P)
        assert tuple(code_src.shape) == (S, Z, J) and code_a.shape == (G, J) and tuple(valid.shape) == (G, J)
        assert tuple(noise.shape) == (G * K, ND)
        assert new_code is None or tuple(new_code.shape) == (G, Z)
        for t, shape in ((target_mean, (G, 3, J)), (target_logvar, (G, 3, J)), (weight, (G, J)), (stats, (G * K, 4, 3, J))):
            assert t is None or tuple(t.shape) == shape
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=self.device)
        scores = None
        if return_scores and mode != part_sampling.MODES["first"]:
            scores = e(G * K, 6, J) if mode == part_sampling.MODES["diverse"] else e(G, K)
        out = {"idx": e(G, P, dtype=torch.int32), "noise": e(G * P, ND), "mean": e(G * P, 3, J), "logvar": e(G * P, 3, J), "scores": scores,
               "n_bad": e(1, dtype=torch.int32)}
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_part_search(
                self._h, _ffi.ptr(code_src), S, code_a.ctypes.data_as(ctypes.c_void_p), _ffi.ptr(new_code), int(new_part), _ffi.ptr(valid),
                _ffi.ptr(noise), G, K, mode, P, _ffi.ptr(target_mean), _ffi.ptr(target_logvar), _ffi.ptr(weight), _ffi.ptr(stats), int(seed),
                int(row0), int(n_draws), int(row_budget), _ffi.ptr(out["idx"]), _ffi.ptr(out["noise"]), _ffi.ptr(out["mean"]),
                _ffi.ptr(out["logvar"]), _ffi.ptr(scores), _ffi.ptr(out["n_bad"]), _ffi.current_stream())
        _ffi.check(rc, "dfx_part_search")
        return out

    def part_search_global(self, code_src, code_a, valid, noise, K, P, rule="farthest", stats=None, seed=0, row0=0, n_draws=512, row_budget=0,
                           return_scores=False):
        """``dfx_part_search_global``: ``part_search``'s chunked aligner pass over G groups of K noises, then ONE diverse selection over all
        G K rows (``part_sampling.select_diverse_global``: 'farthest' or 'first_pick').  Arguments as ``part_search`` (no new part).
        Returns dict: idx (P,) int32 global rows, noise (P,noise_dim), mean / logvar (P,3,J), scores ((G K,6,J) or None), n_bad."""
        from . import part_sampling
        rule = part_sampling.rule_id(rule)
        code_a = np.ascontiguousarray((code_a.detach().cpu().numpy() if isinstance(code_a, torch.Tensor) else np.asarray(code_a)).astype(np.int32))
        code_src, valid, noise, stats = map(self._f, (code_src, valid, noise, stats))
        J, Z, ND = self.n_class, self.zdim, self.noise_dim
        S, G, K, P = code_src.shape[0], code_a.shape[0], int(K), int(P)
        assert tuple(code_src.shape) == (S, Z, J) and code_a.shape == (G, J) and tuple(valid.shape) == (G, J)
        assert tuple(noise.shape) == (G * K, ND) and (stats is None or tuple(stats.shape) == (G * K, 4, 3, J))
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=self.device)
        scores = e(G * K, 6, J) if return_scores else None
        out = {"idx": e(max(P, 0), dtype=torch.int32), "noise": e(max(P, 0), ND), "mean": e(max(P, 0), 3, J), "logvar": e(max(P, 0), 3, J),
               "scores": scores, "n_bad": e(1, dtype=torch.int32)}
        with torch.cuda.device(self.device):
            rc = _ffi.lib().dfx_part_search_global(
                self._h, _ffi.ptr(code_src), S, code_a.ctypes.data_as(ctypes.c_void_p), _ffi.ptr(valid), _ffi.ptr(noise), G, K, P, rule,
                _ffi.ptr(stats), int(seed), int(row0), int(n_draws), int(row_budget), _ffi.ptr(out["idx"]), _ffi.ptr(out["noise"]),
                _ffi.ptr(out["mean"]), _ffi.ptr(out["logvar"]), _ffi.ptr(scores), _ffi.ptr(out["n_bad"]), _ffi.current_stream())
        _ffi.check(rc, "dfx_part_search_global")
        return out

    def sample_latents_selective(self, w_noise, aligner_noise, valid_id, mode, K=100, keep=10, rule="farthest", fixed_id=None, npoints=2048,
                                 part_code=None, stats=None, seed=0, row0=0, n_draws=512, row_budget=0):
        """``sample_latents`` with the reference's selective noise sampling (part_encoders.py:1052-1110 with selective_noise_sampling /
        selective_noise_sampling_global): K aligner noises per shape, of which ``keep`` per shape survive.

        mode 'shape': the ``keep`` most different configurations of every shape (``part_search`` 'diverse'); rows shape-major.
        mode 'global': the S keep most different of all S K candidates, whatever shape they belong to (``part_search_global`` with
        ``rule``); rows in pick order.  w_noise (S,zdim,J) or part_code (S,zdim,J); aligner_noise (S K,noise_dim); valid_id (S,J);
        fixed_id as ``sample_latents`` (:1071-1081: a fixed part takes shape 0's code and is valid, and with any fixed part every
        shape uses shape 0's K noises).  The candidates' codes are never materialised; the kept rows go through one
        ``dfx_compose_latents`` call.  Returns ``sample_latents``' dict over S keep rows plus idx ((S,keep) candidates in [0,K) for
        'shape', (S keep,) global rows for 'global'), source_row (S keep,) int64 (the shape behind every row) and n_bad.
        Deviation: ``noise`` holds the SELECTED rows (the reference returns all S K)."""
        if mode not in ("shape", "global"):
            raise ValueError(f"sample_latents_selective: mode {mode!r} not in ('shape', 'global')")
        if (w_noise is None) == (part_code is None):
            raise ValueError("sample_latents_selective: give exactly one of w_noise / part_code")
        valid_id, aligner_noise = self._f(valid_id), self._f(aligner_noise)
        S, J, K, keep = valid_id.shape[0], self.n_class, int(K), int(keep)
        code = self.flow_reverse(w_noise) if part_code is None else self._f(part_code)
        assert tuple(code.shape) == (S, self.zdim, J) and tuple(aligner_noise.shape) == (S * K, self.noise_dim)
        fid = np.zeros(J, np.int32) if fixed_id is None else np.asarray([int(v) != 0 for v in fixed_id], np.int32)
        code_a = np.where(fid[None, :] != 0, 0, np.arange(S, dtype=np.int32)[:, None]).astype(np.int32)            # :1074
        valid = valid_id
        if fid.any():
            f = torch.as_tensor(fid, dtype=torch.float32, device=self.device)
            valid = valid_id * (1 - f) + f * (valid_id[:1] + f).clamp(0, 1)                                           # :1072-1075
            aligner_noise = aligner_noise[:K].repeat(S, 1)                                                            # :1076-1081
        kw = dict(stats=stats, seed=seed, row0=row0, n_draws=n_draws, row_budget=row_budget)
        if mode == "shape":
            found = self.part_search(code, code_a, valid, aligner_noise, K, "diverse", P=keep, **kw)
            source = torch.arange(S, device=self.device).repeat_interleave(keep)
        else:
            found = self.part_search_global(code, code_a, valid, aligner_noise, K, S * keep, rule=rule, **kw)
            source = found["idx"].long() // K
        src_host = source.cpu().numpy()
        out = self.compose_latents(code, code_a[src_host], valid[source].contiguous(), noise_src=found["noise"], npoints=npoints)
        out.update(idx=found["idx"], source_row=source, n_bad=found["n_bad"])
        return out

    def optimize_noise(self, part_code, valid, z0, problem, max_iter, trace=False):
        """``dfx_noise_opt_run``: R independent gradient descents on the aligner noise (tools/shape_edit.py:80-129 per row), enqueued
        without host round trips.  part_code (R,zdim,J), valid (R,J), z0 (R,noise_dim); ``problem``: dict with the (R,3,J) targets
        ``fit_mean`` / ``fit_logvar``, the (R,J) mask ``fix`` (= valid * fix_ids), optionally ``edit_mean`` + ``edit_mean_sel`` and
        ``edit_logvar`` + ``edit_var_sel``, and the scalars of ``editing.NOISE_OPT_DEFAULTS`` (``editing.noise_problem`` builds it).
        Returns dict: z, mean, logvar (at the returned z), iters_done (R,) int32, trace (max_iter,R,5 + 2 noise_dim) or None."""
        from . import editing
        if not self.cimle:
            raise RuntimeError("optimize_noise needs the cIMLE aligner")
        part_code, valid, z = self._f(part_code), self._f(valid), self._f(z0).clone()
        R, J, ND = part_code.shape[0], self.n_class, self.noise_dim
        assert tuple(part_code.shape) == (R, self.zdim, J) and tuple(valid.shape) == (R, J) and tuple(z.shape) == (R, ND)
        p, keep = _ffi.NoiseOptProblem(), []
        for name, shape in (("fit_mean", (R, 3, J)), ("fit_logvar", (R, 3, J)), ("fix", (R, J)), ("edit_mean", (R, 3, J)), ("edit_mean_sel", (R, J)),
                            ("edit_logvar", (R, 3, J)), ("edit_var_sel", (R, J))):
            t = self._f(problem.get(name))
            if t is not None:
                assert tuple(t.shape) == shape, (name, tuple(t.shape), shape)
                keep.append(t)
                setattr(p, name, t.data_ptr())
        for name, default in editing.NOISE_OPT_DEFAULTS.items():
            setattr(p, name, type(default)(problem.get(name, default)))
        lib = _ffi.lib()
        nbytes = lib.dfx_noise_opt_workspace_bytes(ctypes.byref(self._w), R)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        mean = torch.empty(R, 3, J, dtype=torch.float32, device=self.device)
        logvar = torch.empty_like(mean)
        iters = torch.empty(R, dtype=torch.int32, device=self.device)
        tr = torch.empty(int(max_iter), R, 5 + 2 * ND, dtype=torch.float32, device=self.device) if trace else None
        with torch.cuda.device(self.device):
            rc = lib.dfx_noise_opt_run(ctypes.byref(self._w), (ws.data_ptr() + 255) & ~255, nbytes, ctypes.byref(p), _ffi.ptr(part_code), _ffi.ptr(valid),
                                       _ffi.ptr(z), _ffi.ptr(mean), _ffi.ptr(logvar), _ffi.ptr(iters), _ffi.ptr(tr), R, int(max_iter),
                                       _ffi.current_stream())
        _ffi.check(rc, "dfx_noise_opt_run")
        return {"z": z, "mean": mean, "logvar": logvar, "iters_done": iters, "trace": tr}
