"""CPU side of tests/test_gpu_shared_mlp_train_shapes.py: the width rule, the kernel each case is predicted to reach, the float64 truth
checked against a plain numpy restatement (no autograd), the float32 yardstick's headroom under the gates, and a model of the
K = 4 (mod 8) defect that the gates must reject."""
import numpy as np
import pytest
import torch

import _smt_case as sc


def test_width_rule_table():
    """train_widths_ok over 4 .. 1032 step 4: an output width passes iff it is a multiple of 8 and <= 1024, wherever it stands in the stack."""
    from difffacto_amd.pointnet2_ops.pointnet2_modules import train_widths_ok
    for w in range(4, 1033, 4):
        want = w % 8 == 0 and w <= 1024
        assert train_widths_ok([3, w]) is want, w
        assert train_widths_ok([3, 64, w]) is want, w
        assert train_widths_ok([3, w, 64]) is want, w
        assert train_widths_ok([w, 64]), w               # the input width is free (padded by libdfx)
    assert train_widths_ok([6, 64, 64, 128]) and train_widths_ok([259, 256, 512, 1024]) and train_widths_ok([1, 8])
    assert not train_widths_ok([6, 12, 20]) and not train_widths_ok([6, 36, 68]) and not train_widths_ok([10, 12])
    assert not train_widths_ok([6, 0]) and not train_widths_ok([6, 7]) and not train_widths_ok([6, 1032])
    assert not train_widths_ok([6]) and not train_widths_ok([0, 8])
    assert train_widths_ok([6, 8, 8, 8, 8]) and not train_widths_ok([6, 8, 8, 8, 8, 8])      # DFX_MLP_MAX_LAYERS = 4


def test_every_case_reaches_its_kernels_and_the_table_reaches_every_kernel():
    seen = set()
    for name, c in sc.CASES.items():
        got = sc.kernel_set(c["spec"], c["dims"])
        assert got == c["kernels"], (name, sorted(got), sorted(c["kernels"]))
        seen |= got
        from difffacto_amd.pointnet2_ops.pointnet2_modules import train_widths_ok
        assert train_widths_ok(c["spec"]), name
    assert seen == sc.ALL_KERNELS, sorted(sc.ALL_KERNELS - seen)


def _by_product(name):
    c = sc.CASES[name]
    return {(d, l): (k, info, mnk) for d, l, mnk, k, info in sc.predict(c["spec"], c["dims"])}


def test_cases_reach_the_loop_shapes_they_are_listed_for():
    """The details behind the kernel names: trip counts and tails of k_lin, U of the wide kernels, the striding loop, the ragged last tile."""
    a = _by_product("A")
    assert [(a["fwd", l][1]["trips"], a["fwd", l][1]["tail"]) for l in range(4)] == [(0, 1), (0, 1), (0, 3), (1, 1)]
    assert (a["bwd", 3][1]["trips"], a["bwd", 3][1]["tail"]) == (3, 1) and a["fwd", 0][2][0] == 70
    a2 = _by_product("A2")
    assert [(a2["fwd", l][1]["trips"], a2["fwd", l][1]["tail"]) for l in (1, 2)] == [(2, 0), (3, 0)]
    assert (a2["bwd", 2][1]["trips"], a2["bwd", 2][1]["tail"]) == (2, 1)
    b = _by_product("B")
    assert sorted(v[1]["tiles"] for v in b.values()) == [129, 258, 258, 387] and all(v[2][0] == 4100 for v in b.values())
    c = _by_product("C")
    split = {k: (v[2][1], v[2][2], v[1]["trips"], v[1]["tail"]) for k, v in c.items() if v[0] == sc.K_SPLIT}
    assert split == {("fwd", 1): (32, 160, 5, 0), ("fwd", 3): (16, 136, 4, 1), ("bwd", 2): (32, 136, 4, 1), ("bwd", 0): (8, 160, 5, 0)}
    d1 = _by_product("D1")
    assert {k: v[1]["U"] for k, v in d1.items() if v[0] == sc.K_LDS4} == {("fwd", 0): 1, ("fwd", 2): 5, ("bwd", 1): 5}
    assert all(v[1]["last_rows"] == 31 and v[1]["row_tiles"] == 33 for v in d1.values() if v[0] == sc.K_LDS4)
    d2 = _by_product("D2")
    assert {k: (v[0], v[1]["U"]) for k, v in d2.items() if v[0] != sc.K_LIN} == {("fwd", 0): (sc.K_LDS4, 6), ("fwd", 2): (sc.K_LDS2, 35), ("bwd", 1): (sc.K_LDS2, 35)}
    d3 = _by_product("D3")["fwd", 1]
    assert d3[0] == sc.K_LDS4 and d3[1] == dict(U=34, rows=32, row_tiles=33, last_rows=31)       # 32 row blocks walk 33 tiles: rt += gridDim.y
    d4 = _by_product("D4")["fwd", 1]
    assert d4[0] == sc.K_LDS2 and d4[1]["U"] == 68
    e1 = _by_product("E1")
    assert (e1["fwd", 0][0], e1["fwd", 0][1]["U"]) == (sc.K_WIDE, 3) and (e1["bwd", 1][0], e1["bwd", 1][1]["U"]) == (sc.K_WIDE, 16)
    e2 = _by_product("E2")["fwd", 1]
    assert e2[0] == sc.K_WIDE and e2[1]["U"] == 69
    for g in ("G1", "G2"):
        B, M, ns = sc.CASES[g]["dims"]
        assert B * M > 65535 and sc.CASES[g]["pool"]
    assert sc.CASES["G2"]["dims"][0] > 1
    # the thresholds themselves
    assert sc.lin_kernel(4096, 512, 8)[0] == sc.K_LIN and sc.lin_kernel(8191, 512, 8)[0] == sc.K_WIDE and sc.lin_kernel(8192, 512, 8)[0] == sc.K_LDS4
    assert sc.lin_kernel(8192, 512, 272)[0] == sc.K_LDS4 and sc.lin_kernel(8192, 512, 280)[0] == sc.K_LDS2 and sc.lin_kernel(8192, 512, 552)[0] == sc.K_WIDE
    assert sc.lin_kernel(4100, 64, 128)[0] == sc.K_LIN and sc.lin_kernel(4100, 32, 128)[0] == sc.K_SPLIT and sc.lin_kernel(4100, 32, 120)[0] == sc.K_LIN


# ---- a plain numpy restatement of the stack and its backward (BatchNorm on batch statistics, ReLU, max over ns): no torch, no autograd ----
def numpy_stack(case, product=None, eps=1e-5, momentum=0.1):
    """float64 forward + backward of a pooled train-mode BatchNorm case.  product(l, X, W) replaces the forward product of layer l (the defect model)."""
    assert case["bn"] and case["train"] and case["pool"]
    sd = {k: v.double().numpy() for k, v in sc.make_stack(case["spec"], True, case["seed"]).state_dict().items()}
    x, gout = (a.astype(np.float64) for a in sc.make_inputs(case["spec"], case["dims"], True, case["seed"]))
    B, C, M, ns = x.shape
    R, L = B * M * ns, len(case["spec"]) - 1
    h = x.transpose(0, 2, 3, 1).reshape(R, C)                    # rows (b, m, s)
    res, saved = {}, []
    for l in range(L):
        W = sd[f"{3 * l}.weight"][:, :, 0, 0]
        g, be = sd[f"{3 * l + 1}.weight"], sd[f"{3 * l + 1}.bias"]
        z = product(l, h, W) if product else h @ W.T
        mean = z.sum(0) / R
        var = ((z - mean) ** 2).sum(0) / R
        rstd = 1.0 / np.sqrt(var + eps)
        xhat = (z - mean) * rstd
        y = np.maximum(xhat * g + be, 0.0)
        res[f"r.{3 * l + 1}.running_mean"] = (1 - momentum) * sd[f"{3 * l + 1}.running_mean"] + momentum * mean
        res[f"r.{3 * l + 1}.running_var"] = (1 - momentum) * sd[f"{3 * l + 1}.running_var"] + momentum * var * R / (R - 1)
        saved.append((h, W, g, rstd, xhat, y))
        h = y
    Cl = h.shape[1]
    grp = h.reshape(B, M, ns, Cl)
    at = grp.argmax(axis=2)                                       # first maximum
    res["out"] = grp.max(axis=2).transpose(0, 2, 1)               # (B, Cl, M)
    dy = np.zeros_like(grp)
    np.put_along_axis(dy, at[:, :, None, :], gout.transpose(0, 2, 1)[:, :, None, :], axis=2)
    dy = dy.reshape(R, Cl)
    for l in reversed(range(L)):
        xin, W, g, rstd, xhat, y = saved[l]
        gm = dy * (y > 0)
        dbeta, dgamma = gm.sum(0), (gm * xhat).sum(0)
        dz = g * rstd * (gm - dbeta / R - xhat * dgamma / R)
        res[f"g.{3 * l}.weight"] = (dz.T @ xin)[:, :, None, None]
        res[f"g.{3 * l + 1}.weight"], res[f"g.{3 * l + 1}.bias"] = dgamma, dbeta
        dy = dz @ W
    res["d_x"] = dy.reshape(B, M, ns, C).transpose(0, 3, 1, 2)
    return res


@pytest.mark.parametrize("name", ["A", "B"])
def test_truth_is_reproduced_by_a_numpy_restatement(name):
    ref, mine = sc.truth(name), numpy_stack(sc.CASES[name])
    assert set(ref) == set(mine)
    for k, r in ref.items():
        assert r.dtype == np.float64 and mine[k].shape == r.shape, k
        assert np.abs(mine[k] - r).max() <= 1e-12 * max(1.0, np.abs(r).max()), (k, float(np.abs(mine[k] - r).max()))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_float32_yardstick_has_headroom_under_the_gates(name):
    """The same stack in float32 on the CPU sits at least 10x inside the gates on every case: neither the gates nor the ReLU / arg-max
    flips of these inputs can fail a correct fp32 kernel."""
    y = sc.yardstick(name)
    print(sc.line(name, y, y))
    for k, gate in sc.GATES.items():
        assert y[k] * sc.HEADROOM <= gate, (name, k, y[k], y["at"].get(k))


def test_the_gates_reject_the_k_mod_8_defect():
    """What the fp32 kernels computed for K = 12 before the width rule: lane half 1 of the second K block multiplies in the first four
    values of the NEXT row of X and of W (past the last row: whatever follows, here zeros).  On the float64 truth of a [6, 12, 20] stack."""
    case = sc._case([6, 12, 20], (2, 7, 5), seed=31)
    good = numpy_stack(case)

    def defective(l, X, W):
        z = X @ W.T
        if X.shape[1] % 8 == 4:
            Xn = np.vstack([X[1:, :4], np.zeros((1, 4))])
            Wn = np.vstack([W[1:, :4], np.zeros((1, 4))])
            z = z + Xn @ Wn.T
        return z

    bad = numpy_stack(case, product=defective)
    assert sc.passes(sc.errors(good, good))
    e = sc.errors(bad, good)
    print(f"K = 12 defect model: out {e['out']:.2e} stat {e['stat']:.2e} grad {e['grad']:.2e} (gates {sc.OUT_TOL:.0e} / {sc.GRAD_TOL:.0e})")
    assert not sc.passes(e)
    assert e["out"] > 100 * sc.OUT_TOL and e["grad"] > 100 * sc.GRAD_TOL      # by orders of magnitude, not marginally
