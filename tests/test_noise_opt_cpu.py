"""CPU checks of the part re-configuration feature: the ABI additions (dfx_aligner_input_backward, dfx_noise_opt_workspace_bytes,
dfx_noise_opt_run) and their argument errors (which come before any HIP call), editing.noise_problem / noise_losses against a numpy restatement of
the reference's edit_latent (anchor_gen.py:877-892), editing.noise_opt_replay against torch's own Adam + ReduceLROnPlateau on the reference's
recorded sequences (tests/golden/noiseopt/edit_traj.npz), and the fixture manifest."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "noiseopt")
NEW = ("dfx_aligner_input_backward", "dfx_noise_opt_workspace_bytes", "dfx_noise_opt_run")


@pytest.fixture(scope="module")
def lib():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from difffacto_amd import _ffi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert "dfx_noise_opt_problem" in header
    assert lib.dfx_version() >= 103 and lib.dfx_abi_version() == 5 == _ffi.DFX_ABI_VERSION


def _weights(cimle=1):
    from difffacto_amd import _ffi
    w = _ffi.LatentWeights()
    w.n_class, w.zdim, w.depth, w.n_heads, w.d_head, w.cimle, w.noise_dim, w.noise_scale = 4, 256, 5, 8, 32, cimle, 32 if cimle else 0, 100.0
    return w


def _fails(lib, rc, *words):
    msg = lib.dfx_last_error().decode()
    assert rc != 0 and msg, (rc, msg)
    assert any(w in msg for w in words), msg


def test_input_backward_argument_errors_come_before_any_hip_call(lib):
    w, p = _weights(), 0x1000                         # never dereferenced: every call below returns from its argument checks
    nbytes = lib.dfx_aligner_train_workspace_bytes(2, 4, 256, 32, 8, 32, 5)
    assert nbytes > 0
    f = lib.dfx_aligner_input_backward
    _fails(lib, f(None, p, nbytes, p, p, p, p, p, 2, None), "null weights")
    _fails(lib, f(_weights(cimle=0), p, nbytes, p, p, p, p, p, 2, None), "cIMLE")
    _fails(lib, f(w, p, nbytes, p, p, p, p, p, 0, None), "null argument")
    _fails(lib, f(w, p, nbytes, p, p, p, p, p, -3, None), "null argument")
    _fails(lib, f(w, None, nbytes, p, p, p, p, p, 2, None), "null argument")
    _fails(lib, f(w, p, nbytes, None, p, p, p, p, 2, None), "null argument")
    _fails(lib, f(w, p, nbytes, p, None, None, p, p, 2, None), "null argument")
    _fails(lib, f(w, p, nbytes, p, p, p, None, None, 2, None), "neither")
    _fails(lib, f(w, p, nbytes - 1, p, p, p, p, None, 2, None), "workspace too small")
    bad = _weights()
    bad.d_head = 24
    _fails(lib, f(bad, p, nbytes, p, p, p, p, p, 2, None), "d_head")


def test_noise_opt_argument_errors_come_before_any_hip_call(lib):
    from difffacto_amd import _ffi, editing
    w, p = _weights(), 0x1000
    assert lib.dfx_noise_opt_workspace_bytes(None, 4) == 0 and lib.dfx_noise_opt_workspace_bytes(ctypes.byref(w), 0) == 0
    assert lib.dfx_noise_opt_workspace_bytes(ctypes.byref(_weights(cimle=0)), 4) == 0
    nbytes = lib.dfx_noise_opt_workspace_bytes(ctypes.byref(w), 4)
    assert nbytes > lib.dfx_aligner_train_workspace_bytes(4, 4, 256, 32, 8, 32, 5) > 0

    def prob(**over):
        q = _ffi.NoiseOptProblem()
        for k in ("fit_mean", "fit_logvar", "fix", "edit_mean", "edit_mean_sel"):
            setattr(q, k, p)
        for k, v in {**editing.NOISE_OPT_DEFAULTS, **over}.items():
            setattr(q, k, v)
        return q

    f = lib.dfx_noise_opt_run
    ok = prob()
    _fails(lib, f(None, p, nbytes, ok, p, p, p, p, p, p, None, 4, 10, None), "null weights")
    _fails(lib, f(_weights(cimle=0), p, nbytes, ok, p, p, p, p, p, p, None, 4, 10, None), "cIMLE")
    _fails(lib, f(w, p, nbytes, ok, p, p, p, p, p, p, None, 0, 10, None), "R = 0")
    _fails(lib, f(w, p, nbytes, ok, p, p, p, p, p, p, None, -1, 10, None), "R = -1")
    _fails(lib, f(w, p, nbytes, ok, p, p, p, p, p, p, None, 4, -1, None), "max_iter")
    _fails(lib, f(w, p, nbytes, None, p, p, p, p, p, p, None, 4, 10, None), "null argument")
    for i in (1, 4, 5, 6, 7, 8, 9):                   # workspace, part_code, valid, z, mean, logvar, iters_done
        args = [w, p, nbytes, ok, p, p, p, p, p, p, None, 4, 10, None]
        args[i] = None
        _fails(lib, f(*args), "null argument")
    q = prob()
    q.fix = None
    _fails(lib, f(w, p, nbytes, q, p, p, p, p, p, p, None, 4, 10, None), "null fit target")
    q = prob()
    q.edit_mean = None                                # a selector without its target
    _fails(lib, f(w, p, nbytes, q, p, p, p, p, p, p, None, 4, 10, None), "come together")
    _fails(lib, f(w, p, nbytes, prob(factor=1.5), p, p, p, p, p, p, None, 4, 10, None), "out of range")
    _fails(lib, f(w, p, nbytes, prob(lr0=0.0), p, p, p, p, p, p, None, 4, 10, None), "out of range")
    _fails(lib, f(w, p, nbytes - 1, ok, p, p, p, p, p, p, None, 4, 10, None), "workspace too small")
    _fails(lib, f(w, p, lib.dfx_noise_opt_workspace_bytes(ctypes.byref(w), 3), ok, p, p, p, p, p, p, None, 4, 10, None), "workspace too small")


# ---------------------------------------------------------------------------------------------------- the objective
def _edit_latent_numpy(mean, logvar, z, valid, ref_mean, ref_var, fix_ids, edit_id, new_mean, new_var, fit_weight, reg_weight):
    """anchor_gen.py:877-892 for one shape (B = 1), then parse_losses: float64 numpy."""
    d = np.concatenate([mean, logvar], 0) - np.concatenate([ref_mean, np.log(ref_var)], 0)          # (6, J)
    f = valid * fix_ids
    fit = (d ** 2 * f[None]).sum() / f.sum()
    edit = 0.0
    if new_mean is not None:
        edit += ((mean[:, edit_id] - new_mean) ** 2).mean()
    if new_var is not None:
        edit += ((logvar[:, edit_id] - np.log(new_var)) ** 2).mean()
    reg = (z ** 2).sum()
    return fit_weight * fit + edit + reg_weight * reg, fit, edit, reg


def test_noise_problem_is_the_reference_objective_row_by_row():
    from difffacto_amd import editing
    rng = np.random.Generator(np.random.PCG64(3))
    R, J = 6, 4
    valid = np.ones((R, J))
    valid[1, 3] = valid[4, 0] = 0
    ref_mean, ref_var = rng.standard_normal((R, 3, J)) * 0.3, rng.uniform(0.04, 0.4, size=(R, 3, J))
    ref_var[1, :, 3] = 0.0                             # an absent part with zero variance: log = -inf must not reach the loss
    fix = np.array([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 0], [1, 0, 1, 1], [1, 1, 1, 0]], np.float64)
    ep = np.array([0, 1, 2, 3, 1, 3])
    new_mean, new_var = rng.standard_normal((R, 3)) * 0.3, rng.uniform(0.04, 0.4, size=(R, 3))
    mean, logvar, z = rng.standard_normal((R, 3, J)), rng.standard_normal((R, 3, J)), rng.standard_normal((R, 32))
    for kw in (dict(new_mean=new_mean), dict(new_var=new_var), dict(new_mean=new_mean, new_var=new_var)):
        prob = editing.noise_problem(valid, ref_mean, ref_var, fix, ep, fit_weight=0.05, reg_weight=0.7, **kw)
        assert all(v.dtype == torch.float32 for v in prob.values() if isinstance(v, torch.Tensor))
        assert ("edit_mean" in prob) == ("new_mean" in kw) and ("edit_logvar" in prob) == ("new_var" in kw)
        got = editing.noise_losses(prob, torch.from_numpy(mean), torch.from_numpy(logvar), torch.from_numpy(z))
        for r in range(R):
            rv = np.where(valid[r] * fix[r] != 0, ref_var[r], 1.0)
            want = _edit_latent_numpy(mean[r], logvar[r], z[r], valid[r], ref_mean[r], rv, fix[r], ep[r], kw.get("new_mean", [None] * R)[r],
                                      kw.get("new_var", [None] * R)[r], 0.05, 0.7)
            for k, w in zip(("L", "fit", "edit", "reg"), want):
                assert abs(float(got[k][r]) - w) <= 2e-6 * max(1.0, abs(w)), (r, k, float(got[k][r]), w)
    # scalar / broadcast forms, the inversion objective, and the errors
    p1 = editing.noise_problem(valid[:1], ref_mean[:1], ref_var[:1], [0, 1, 1, 1], 0, new_var=new_var[0])
    assert torch.equal(p1["edit_var_sel"], torch.tensor([[1.0, 0, 0, 0]])) and torch.equal(p1["fix"], torch.tensor([[0.0, 1, 1, 1]]))
    assert torch.allclose(p1["edit_logvar"][0, :, 0], torch.log(torch.from_numpy(new_var[0]).float())) and not p1["edit_logvar"][0, :, 1:].any()
    inv = editing.noise_problem(valid, ref_mean, ref_var, np.ones(J), None, fit_weight=1.0)
    assert "edit_mean" not in inv and "edit_logvar" not in inv and torch.equal(inv["fix"], torch.from_numpy(valid).float())
    assert bool(torch.isfinite(inv["fit_logvar"]).all())
    with pytest.raises(ValueError, match="absent"):
        editing.noise_problem(valid, ref_mean, ref_var, np.ones(J), 3, new_var=new_var)             # row 1 lacks part 3
    with pytest.raises(ValueError, match="divide by zero"):
        editing.noise_problem(valid, ref_mean, ref_var, [1, 0, 0, 0], 1, new_var=new_var)           # row 4 has no part 0
    with pytest.raises(ValueError):
        editing.noise_problem(valid, ref_mean, ref_var, np.ones(J), None, new_var=new_var)
    with pytest.raises(TypeError):
        editing.noise_problem(valid, ref_mean, ref_var, np.ones(J), 0, new_var=new_var, momentum=0.9)


# ---------------------------------------------------------------------------------------------------- the optimizer rules
def _torch_loop(L, G, z0, max_iter):
    """torch.optim.Adam + ReduceLROnPlateau + torch.allclose driven by recorded gradients / losses (tools/shape_edit.py:80-129), float64."""
    z = torch.nn.Parameter(torch.from_numpy(np.asarray(z0, np.float64).reshape(1, -1).copy()))
    opt = torch.optim.Adam([z], lr=1)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=10, min_lr=5e-2)
    prev = torch.zeros(1, dtype=torch.float64)
    zs, lrs, reduced, stopped = [z.detach().numpy().ravel().copy()], [], [], None
    for k in range(max_iter):
        z.grad = torch.from_numpy(G[k].reshape(1, -1).copy())
        lr = opt.param_groups[0]["lr"]
        lrs.append(lr)
        opt.step()
        sched.step(float(L[k]))
        if opt.param_groups[0]["lr"] != lr:
            reduced.append(k)
        zs.append(z.detach().numpy().ravel().copy())
        loss = torch.tensor(float(L[k]), dtype=torch.float64)
        if torch.allclose(loss, prev):
            stopped = k
            break
        prev = loss
    return np.stack(zs), np.asarray(lrs), reduced, stopped


@pytest.mark.parametrize("p", [0, 1])
def test_replay_is_torch_adam_plus_plateau_plus_allclose(p):
    from difffacto_amd import editing
    g = np.load(os.path.join(GOLD, "edit_traj.npz"))
    pre = f"p{p}/f64/"
    L, G, z0 = g[pre + "L"], g[pre + "grad"], g[f"p{p}/z0"]
    n = len(L)
    zs, lrs, reduced, stopped = _torch_loop(L, G, z0, n)
    rep = editing.noise_opt_replay(L, G, z0)
    assert rep["n"] == len(lrs) == n and rep["stopped_at"] == stopped == n - 1
    assert np.array_equal(rep["lr"], lrs) and rep["reduced_at"] == reduced and len(reduced) >= 2
    assert np.abs(rep["z"] - zs).max() <= 1e-12
    # ... which is the trajectory the reference's loop recorded (z before every step, the rate of every step, the end point)
    assert np.abs(rep["z"][:n] - g[pre + "z"]).max() <= 1e-12 and np.abs(rep["z"][n] - g[pre + "z_end"]).max() <= 1e-12
    assert np.array_equal(rep["lr"], g[pre + "lr"])
    # a sequence cut short does not stop; a constant loss stops at once; the rate never falls below min_lr
    assert editing.noise_opt_replay(L[:30], G[:30], z0)["stopped_at"] is None
    flat = editing.noise_opt_replay(np.full(200, 2.0), np.tile(G[:1], (200, 1)), z0)
    assert flat["stopped_at"] == 1 and flat["n"] == 2
    slow = editing.noise_opt_replay(2.0 + 1.0 / np.arange(1, 201), np.tile(G[:1], (200, 1)), z0, stop_rtol=0.0, stop_atol=0.0, threshold=0.5)
    assert slow["stopped_at"] is None and slow["lr"].min() == 5e-2 and slow["lr"][0] == 1.0
    zt, lt, rt, st = _torch_loop(np.full(200, 2.0) + 1.0 / np.arange(1, 201), np.tile(G[:1], (200, 1)), z0, 200)
    dflt = editing.noise_opt_replay(2.0 + 1.0 / np.arange(1, 201), np.tile(G[:1], (200, 1)), z0)
    assert dflt["stopped_at"] == st and np.array_equal(dflt["lr"], lt) and dflt["reduced_at"] == rt and np.abs(dflt["z"] - zt).max() <= 1e-12


def test_the_fixture_problems_meet_the_conditions_of_the_gpu_gates():
    """What tests/test_gpu_noise_opt.py relies on: within 40 iterations the fp32, fp64 and perturbed reference runs share one learning-rate
    sequence and the perturbation has moved z by far more than rounding has; the loss falls."""
    g = np.load(os.path.join(GOLD, "edit_traj.npz"))
    assert int(g["n_problems"]) == 2 and float(g["eps"]) == 5e-4
    for p in range(2):
        pre = f"p{p}/"
        z32, z64, zp = g[pre + "f32/z"], g[pre + "f64/z"], g[pre + "pert/z"]
        assert min(len(z32), len(z64), len(zp)) >= 60
        assert np.array_equal(g[pre + "f32/lr"][:40], g[pre + "f64/lr"][:40]) and np.array_equal(g[pre + "pert/lr"][:40], g[pre + "f64/lr"][:40])
        P40, r40 = np.abs(zp[:40] - z64[:40]).max(), np.abs(z32[:40] - z64[:40]).max()
        assert 1e-4 < P40 < 1e-2 and r40 < 1e-5 < P40
        for run in ("f32", "f64", "pert"):
            assert g[pre + run + "/L"][-1] < 0.05 * g[pre + run + "/L"][0]
    assert g["p1/in/present"].min() == 0 and "p1/edit_part_mean" in g.files and "p0/edit_part_var" in g.files


def test_noiseopt_fixture_manifest():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import manifest
    want = {}
    for line in open(os.path.join(GOLD, "MANIFEST.sha256")):
        if line.strip() and not line.startswith("#"):
            h, name = line.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(GOLD, f)) for f in sorted(os.listdir(GOLD)) if f.endswith(".npz")}
    assert want == have and set(have) == {"edit_point_B1.npz", "edit_point_B3.npz", "optimize_point_B2.npz", "edit_traj.npz"}
