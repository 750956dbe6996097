#!/usr/bin/env python
"""Golden vectors of the reference's editing modes (dev container only; same conventions as make_golden_forward.py, whose helpers
this imports).

    python tests/golden/make_golden_edit.py

Written to tests/golden/edit/ with their own MANIFEST.sha256 (manifest.content_hash).  configs/gen_chair.py with num_timesteps = 10,
npoints = 64, ret_traj on with ret_interval = 5; the reference's own AnchorDiffAE methods run on CPU:

interp_gen_B2.npz        forward with interpolate = True, gen = True (anchor_gen.py:1027 -> interpolate_latent :206-305, flows branch)
interp_enc_B2.npz        the same with gen = False (encoded part codes, the batch's seg ids)
mixing_B3_K2.npz         forward with combine = True (combine_latent :457-532), cimle_sample_num = 2, one absent part
specific_K2.npz          combine_latent_specific (:412-455) on four per-part point sets, one of them all zero
drift_B2_K3.npz          forward with drift_anchors = True (interpolate_params :338-410), cimle_sample_num = 3

Every torch.randn / randn_like is served from a numpy PCG64 stream and recorded in call order ("draw_{i}"), every torch.randperm
likewise ("perm_{i}"); "chain_at" is the index of the first draw of the reference's decode (x_T, then one per step).
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "edit")
sys.path.insert(0, HERE)

import make_golden_forward as mgf  # noqa: E402  (sets up sys.path for ref_import / difffacto_amd)
from make_golden_forward import DrawRecorder, load_all_weights, make_batch  # noqa: E402
import manifest  # noqa: E402

import ref_import  # noqa: E402

F32 = np.float32
T, N, RET = 10, 64, 5


class EditRecorder(DrawRecorder):
    """DrawRecorder that also serves torch.randperm from the same numpy stream and records the permutations."""

    def __init__(self, seed):
        super().__init__(seed)
        self.perms = []

    def __enter__(self):
        super().__enter__()
        self._randperm = torch.randperm

        def randperm(n, *a, **k):
            p = self.rng.permutation(int(n)).astype(np.int64)
            self.perms.append(p)
            return torch.from_numpy(p.copy())

        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.randperm = self._randperm
        super().__exit__(*exc)

    def as_dict(self):
        d = super().as_dict()
        d.update({f"perm_{i}": p for i, p in enumerate(self.perms)})
        return d


def _model(**flags):
    with contextlib.redirect_stdout(io.StringIO()):
        model, cfg = ref_import.build_reference_model("gen_chair.py", num_timesteps=T)
    load_all_weights(model)
    model.eval()
    model.npoints, model.ret_traj, model.ret_interval = N, True, RET
    for k, v in flags.items():
        setattr(model, k, v)
    return model


def _watch_chain(model, rec):
    """Index of the first draw of the reference's decode (the first call; interpolate_latent's chunks are one chunk here)."""
    at = []
    orig = model.decode

    def decode(*a, **k):
        if not at:
            at.append(len(rec.draws))
        return orig(*a, **k)

    model.decode = decode
    return at


def _save(tag, pred, rec, chain_at, extra):
    out = mgf.np_out(pred)
    meta = dict(T=np.array(T), ret_interval=np.array(RET), n_draws=np.array(len(rec.draws)), n_perms=np.array(len(rec.perms)),
                chain_at=np.array(chain_at))
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **extra, **rec.as_dict(), **out, **meta)
    size = os.path.getsize(os.path.join(OUT, f"{tag}.npz"))
    print(f"wrote {tag}: {len(pred)} keys, {len(rec.draws)} draws, {len(rec.perms)} perms, chain at {chain_at}, {size / 1024:.0f} KiB")


def gen_mode(tag, flags, B, seed, absent=((1, 3),), K=1):
    model = _model(cimle_sample_num=K, **flags)
    batch = make_batch(B, N, seed, absent=absent)
    with EditRecorder(seed + 1) as rec, torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), \
            contextlib.redirect_stderr(io.StringIO()):
        at = _watch_chain(model, rec)
        out = model(mgf.to_torch(batch), device="cpu", epoch=0)
    assert len(out) == 1
    pred, name = out[0]
    _save(tag, pred, rec, at[0], {**{f"in/{k}": v for k, v in batch.items()}, "name": np.array(name), "K": np.array(K)})


def gen_specific(tag, K=2, seed=171, n=(20, 16, 0, 12)):
    model = _model(cimle_sample_num=K)
    rng = np.random.Generator(np.random.PCG64(seed))
    inputs = [(rng.standard_normal((m if m else 8, 3)) * 0.3 * (1 if m else 0)).astype(F32) for m in n]
    with EditRecorder(seed + 1) as rec, torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        at = _watch_chain(model, rec)
        pred = model.combine_latent_specific([torch.from_numpy(a.copy()) for a in inputs], "cpu")
    _save(tag, pred, rec, at[0], {**{f"inp/{i}": a for i, a in enumerate(inputs)}, "K": np.array(K)})


def main():
    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    gen_mode("interp_gen_B2", dict(interpolate=True, gen=True), B=2, seed=201)
    gen_mode("interp_enc_B2", dict(interpolate=True, gen=False), B=2, seed=211)
    gen_mode("mixing_B3_K2", dict(combine=True), B=3, seed=221, absent=((1, 3),), K=2)
    gen_specific("specific_K2")
    gen_mode("drift_B2_K3", dict(drift_anchors=True), B=2, seed=231, K=3)
    path = os.path.join(OUT, "MANIFEST.sha256")
    with open(path, "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
