#!/usr/bin/env python
"""Golden vectors of the reference's part re-configuration editing (dev container only; conventions and helpers of
make_golden_edit.py / make_golden_forward.py).

    python tests/golden/make_golden_noiseopt.py

Written to tests/golden/noiseopt/ with their own MANIFEST.sha256.  configs/gen_chair.py with the project's synthetic weights; the
reference's own AnchorDiffAE.edit_latent / optimize_latent (anchor_gen.py:872-913) and parse_losses (utils/misc.py:120-132) run on
the CPU inside DrawRecorder (which serves the draws and turns the hard-coded ``.cuda()`` of :883/:887 into the identity):

edit_point_B1.npz      one evaluation of edit_latent, B = 1, ``edit_part_var`` only: inputs ("in/*", "z", "ref_means", "ref_vars",
                       "fix_ids", "edit_id", "edit_part_var", "fit_weight"), the loss dict ("loss/*"), parse_losses' total ("total") and
                       its gradient in z from torch autograd ("z_grad")
edit_point_B3.npz      the same with B = 3, one absent part, ``edit_part_mean`` only
optimize_point_B2.npz  optimize_latent on a batch of 2 (one absent part): "z" (2,1,32), the recorded reparameterisation draw
                       ("draw_0"), "loss/*", "total", "z_grad"
edit_traj.npz          the reference's own loop (tools/shape_edit.py:80-129: Adam([z], lr 1), ReduceLROnPlateau(factor 0.5, patience 10,
                       min_lr 5e-2), torch.allclose stop, max_iter 300) on two problems "p0/" (``edit_part_var``, all parts present) and
                       "p1/" (``edit_part_mean``, one absent part), each run three times: "f32/" as is, "f64/" with the whole model and
                       all inputs cast to float64, "pert/" in float64 with z.grad multiplied before every optimizer.step() by
                       1 + eps * n, n a recorded standard-normal draw ("pert/n", eps = "eps" = 5e-4).  Per run, for the n iterations
                       it took: "z" (n,32) BEFORE the step, "z_end" (32) after the last, "L", "fit" (weighted, as in the loss dict),
                       "edit", "reg", "lr" (the rate the step of that iteration used) and, for f64, "grad" (n,32) = z.grad.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "noiseopt")
sys.path.insert(0, HERE)

import make_golden_forward as mgf  # noqa: E402  (sets up sys.path for ref_import / difffacto_amd)
from make_golden_forward import DrawRecorder, load_all_weights, make_batch  # noqa: E402
import manifest  # noqa: E402

import ref_import  # noqa: E402

F32 = np.float32
N = 64
EPS = 5e-4
MAX_ITER = 300


def _model():
    with contextlib.redirect_stdout(io.StringIO()):
        model, cfg = ref_import.build_reference_model("gen_chair.py", num_timesteps=10)
    load_all_weights(model)
    model.eval()
    return model


def _parse(losses):
    from difffacto.utils.misc import parse_losses
    return parse_losses(losses)


def _edit_inputs(batch, z0, fix_ids, edit_id, new_mean, new_var, dtype):
    t = lambda a: torch.from_numpy(np.asarray(a).copy()).to(dtype)
    seg_flag = torch.from_numpy(np.eye(4, dtype=F32)[batch["seg_mask"]]).to(dtype)          # F.one_hot(seg_mask, 4) (shape_edit.py:101)
    return dict(input=t(batch["input"]), seg_flag=seg_flag, valid_id=t(batch["present"]), ref_means=t(batch["part_shift"]),
                ref_vars=t(batch["part_scale"]) ** 2, fix_ids=torch.tensor(fix_ids), edit_id=edit_id,
                edit_part_mean=None if new_mean is None else t(new_mean), edit_part_var=None if new_var is None else t(new_var)), \
        torch.nn.Parameter(t(z0))


def _edit_losses(model, a, z, fit_weight):
    return model.edit_latent(z, a["input"], a["seg_flag"], a["valid_id"], a["ref_means"], a["ref_vars"], a["fix_ids"], a["edit_id"],
                             a["edit_part_mean"], a["edit_part_var"], fit_weight=fit_weight)


def _save(tag, **arrays):
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {tag}: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


def _target(batch, edit_id, kind):
    """shape_edit.py:95-97: the edited part's own variance with axis 2 times 1.2; or its mean moved by (0.15, 0, -0.1)."""
    if kind == "var":
        v = (batch["part_scale"] ** 2)[..., edit_id].copy()
        v[:, 2] *= 1.2
        return None, v.astype(F32)
    m = batch["part_shift"][..., edit_id].copy() + np.array([0.15, 0.0, -0.1], F32)
    return m.astype(F32), None


def gen_edit_point(model, tag, B, seed, absent, edit_id, fix_ids, kind, fit_weight=0.05):
    batch = make_batch(B, N, seed, absent=absent)
    z0 = np.random.Generator(np.random.PCG64(seed + 1)).standard_normal((B, 32)).astype(F32)
    new_mean, new_var = _target(batch, edit_id, kind)
    with DrawRecorder(seed + 2) as rec:
        a, z = _edit_inputs(batch, z0, fix_ids, edit_id, new_mean, new_var, torch.float32)
        losses = _edit_losses(model, a, z, fit_weight)
        total, _ = _parse(losses)
        total.backward()
    assert not rec.draws
    extra = {} if new_mean is None else {"edit_part_mean": new_mean}
    if new_var is not None:
        extra["edit_part_var"] = new_var
    _save(tag, **{f"in/{k}": v for k, v in batch.items()}, z=z0, ref_means=batch["part_shift"], ref_vars=(batch["part_scale"] ** 2).astype(F32),
          fix_ids=np.asarray(fix_ids, np.int64), edit_id=np.array(edit_id), fit_weight=np.array(fit_weight), **extra,
          **{f"loss/{k}": v.detach().numpy().astype(F32) for k, v in losses.items()}, total=total.detach().numpy().astype(F32),
          z_grad=z.grad.numpy().astype(F32), noise_reg_loss=np.array(bool(model.noise_reg_loss)), reg_loss_weight=np.array(float(model.reg_loss_weight)))


def gen_optimize_point(model, tag, B=2, seed=331):
    batch = make_batch(B, N, seed, absent=((1, 2),))
    z0 = np.random.Generator(np.random.PCG64(seed + 1)).standard_normal((B, 1, 32)).astype(F32)
    z = torch.nn.Parameter(torch.from_numpy(z0.copy()))
    with DrawRecorder(seed + 2) as rec, contextlib.redirect_stdout(io.StringIO()):
        losses = model.optimize_latent(mgf.to_torch(batch), z, device="cpu")
        total, _ = _parse(losses)
        total.backward()
    _save(tag, **{f"in/{k}": v for k, v in batch.items()}, z=z0, **rec.as_dict(), n_draws=np.array(len(rec.draws)),
          **{f"loss/{k}": v.detach().numpy().astype(F32) for k, v in losses.items() if isinstance(v, torch.Tensor)},
          total=total.detach().numpy().astype(F32), z_grad=z.grad.numpy().astype(F32))


def run_loop(model, batch, z0, fix_ids, edit_id, new_mean, new_var, dtype, fit_weight=0.05, pert=None):
    """tools/shape_edit.py:80-129 around edit_latent; ``pert`` (MAX_ITER,32): z.grad *= 1 + EPS * pert[it] before optimizer.step()."""
    a, z = _edit_inputs(batch, z0, fix_ids, edit_id, new_mean, new_var, dtype)
    prev = torch.zeros(1, dtype=dtype)
    optimizer = torch.optim.Adam([z], lr=1)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, factor=0.5, patience=10, min_lr=5e-2)
    rec = {k: [] for k in ("z", "L", "fit", "edit", "reg", "lr", "grad")}
    for it in range(MAX_ITER):
        optimizer.zero_grad()
        losses = _edit_losses(model, a, z, fit_weight)
        all_loss, parsed = _parse(losses)
        all_loss.backward()
        rec["z"].append(z.detach().numpy().reshape(-1).copy())
        rec["grad"].append(z.grad.numpy().reshape(-1).copy())
        for k, name in (("fit", "fit_loss"), ("edit", "edit_loss"), ("reg", "reg_loss")):
            rec[k].append(float(parsed[name].detach()))
        rec["L"].append(all_loss.detach().numpy().reshape(()).copy())
        rec["lr"].append(optimizer.param_groups[0]["lr"])
        if pert is not None:
            z.grad.mul_(1 + EPS * torch.from_numpy(pert[it]).to(dtype).reshape(z.shape))
        optimizer.step()
        scheduler.step(all_loss)
        if torch.allclose(all_loss, prev):
            break
        prev = all_loss
    out = {k: np.asarray(v) for k, v in rec.items()}
    out["z_end"] = z.detach().numpy().reshape(-1).copy()
    return out


def gen_traj(model, tag):
    problems = [dict(seed=201, absent=(), zseed=7, edit_id=0, fix_ids=[0, 1, 1, 1], kind="var"),
                dict(seed=341, absent=((0, 3),), zseed=8, edit_id=1, fix_ids=[1, 0, 1, 1], kind="mean")]
    arrays = {"eps": np.array(EPS), "max_iter": np.array(MAX_ITER), "n_problems": np.array(len(problems)),
              "reg_loss_weight": np.array(float(model.reg_loss_weight)), "fit_weight": np.array(0.05)}
    model64 = _model().double()
    for i, p in enumerate(problems):
        batch = make_batch(1, N, p["seed"], absent=p["absent"])
        z0 = np.random.Generator(np.random.PCG64(p["zseed"])).standard_normal((1, 32)).astype(F32)
        new_mean, new_var = _target(batch, p["edit_id"], p["kind"])
        pert = np.random.Generator(np.random.PCG64(1000 + i)).standard_normal((MAX_ITER, 32)).astype(F32)
        with DrawRecorder(0) as rec:
            runs = {"f32": run_loop(model, batch, z0, p["fix_ids"], p["edit_id"], new_mean, new_var, torch.float32),
                    "f64": run_loop(model64, batch, z0, p["fix_ids"], p["edit_id"], new_mean, new_var, torch.float64),
                    "pert": run_loop(model64, batch, z0, p["fix_ids"], p["edit_id"], new_mean, new_var, torch.float64, pert=pert)}
        assert not rec.draws
        pre = f"p{i}/"
        arrays.update({pre + f"in/{k}": v for k, v in batch.items()})
        arrays.update({pre + "z0": z0, pre + "edit_id": np.array(p["edit_id"]), pre + "fix_ids": np.asarray(p["fix_ids"], np.int64)})
        if new_mean is not None:
            arrays[pre + "edit_part_mean"] = new_mean
        if new_var is not None:
            arrays[pre + "edit_part_var"] = new_var
        for name, r in runs.items():
            n = len(r["L"])
            dt = F32 if name == "f32" else np.float64
            for k in ("z", "z_end", "L", "fit", "edit", "reg"):
                arrays[f"{pre}{name}/{k}"] = r[k].astype(dt)
            arrays[f"{pre}{name}/lr"] = r["lr"].astype(np.float64)
            if name == "f64":
                arrays[f"{pre}{name}/grad"] = r["grad"].astype(np.float64)
            if name == "pert":
                arrays[f"{pre}{name}/n"] = pert[:n]
            print(f"  p{i} {name}: {n} iterations, L {float(r['L'][0]):.4f} -> {float(r['L'][-1]):.5f}, lr {sorted(set(r['lr'].tolist()), reverse=True)}")
        z64, zp, z32 = runs["f64"]["z"], runs["pert"]["z"], runs["f32"]["z"]
        for k in (40, 60):
            print(f"  p{i}: within {k} iterations: max|z32 - z64| = {np.abs(z32[:k] - z64[:k]).max():.2e}, P_{k} = {np.abs(zp[:k] - z64[:k]).max():.2e}, "
                  f"lr equal f32/f64: {np.array_equal(runs['f32']['lr'][:k], runs['f64']['lr'][:k])}, pert: {np.array_equal(runs['pert']['lr'][:k], runs['f64']['lr'][:k])}")
    _save(tag, **arrays)


def main():
    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    model = _model()
    gen_edit_point(model, "edit_point_B1", 1, 301, (), 0, [0, 1, 1, 1], "var")
    gen_edit_point(model, "edit_point_B3", 3, 311, ((1, 3),), 0, [0, 1, 1, 1], "mean")
    gen_optimize_point(model, "optimize_point_B2")
    gen_traj(model, "edit_traj")
    path = os.path.join(OUT, "MANIFEST.sha256")
    with open(path, "w") as f:
        f.write("# sha256 over array contents (name | dtype | shape | bytes, keys sorted), see tests/golden/manifest.py\n")
        for fn in sorted(os.listdir(OUT)):
            if fn.endswith(".npz"):
                f.write(f"{manifest.content_hash(os.path.join(OUT, fn))}  {fn}\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
