"""The float64 gradient oracle, the bf16 rounding model (oracle/train.py) and the gradient statistics (tests/_gradstats.py) that the GPU
gate tests/test_gpu_train_highprec.py stands on.  CPU only.

  * the float64 oracle is pinned to the reference: it agrees with the reference-produced golden train_grads_B3_N64_T10 (77 tensors,
    d_ctx_*) at the bounds the fp32 oracle is held to (tests/test_oracle_golden.py);
  * the identity hook reproduces the float64 oracle bit for bit, and the fused path's folds (attn_fold, ff_fold) equal the reference layout in real arithmetic;
  * central finite differences in float64, independent of autograd, on sampled elements of d_x, d_variances, d_ctx_mv and of the ff0 /
    ff2 / to_q / norm3 / proj_in gradients;
  * self-test of the acceptance function under the COMMITTED thresholds: the rounding model run in fp32 (a stand-in for a correct bf16
    kernel) is accepted, each of six deliberately wrong variants of it (oracle/train.py: ``mutate=``) is rejected — conditions on the
    thresholds, not measurements; a seventh (the gradient between two blocks rounded to bf16, a lost lo half of the pair) is reported.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _gradstats as gs  # noqa: E402
from _train_case import check_against_golden, load_case  # noqa: E402
from oracle import torch_cpu, train  # noqa: E402

B, N, P_DROP = 5, 480, 0.2      # the self-test's case: the smaller of the two on which the GPU gate judges the matrix group ratios


def _numpy_drops(B, N, p, seed):
    rng = np.random.default_rng(seed)
    fac = lambda *s: ((rng.uniform(size=s) >= p) / (1.0 - p)).astype(np.float32)
    d = {"te": fac(B, 1024)}
    for i in range(5):
        d[("attn", i)], d[("ff", i)] = fac(B, N, 128), fac(B, N, 512)
    return d


@pytest.fixture(scope="module")
def selftest():
    """Per dropout setting: the case, float64 truth, the rounding model (yardstick) and the stand-in kernel (the model in fp32)."""
    out = {}
    for key, drops in (("p0", None), ("p0.2", _numpy_drops(B, N, P_DROP, 5))):
        c = gs.make_train_case(B, N, seed=21)
        run = lambda c=c, drops=drops, **kw: gs.flatten(train.loss_and_grads(**c, drops=drops, **kw))
        out[key] = dict(c=c, drops=drops, run=run, truth=run(dtype=torch.float64), yard=run(dtype=torch.float64, operand_round=train.round_bf16),
                        stand=run(operand_round=train.round_bf16))
    return out


def test_float64_oracle_is_pinned_to_the_reference_golden():
    g, c = load_case("B3_N64_T10")
    r = train.loss_and_grads(**c, dtype=torch.float64)
    assert r["eps"].dtype == np.float64 and all(v.dtype == np.float64 for v in r["grads"].values())
    assert abs(r["loss"] - float(g["loss"])) < 2e-6
    assert np.abs(r["eps"] - g["eps"]).max() < 5e-6
    n, worst = check_against_golden(g, r["grads"], rtol=1e-4, atol=1e-8)
    assert n == 77
    for k in ("d_ctx_code", "d_ctx_mv"):
        assert np.abs(r[k] - g[k]).max() <= 1e-4 * np.abs(g[k]).max() + 1e-9
    print(f"float64 oracle vs the reference's fp32 autograd: worst max-abs error / max-abs over 77 tensors = {worst:.2e}")


def test_identity_hook_changes_no_bit_and_the_fold_is_exact_in_real_arithmetic():
    g, c = load_case("B3_N64_T10")
    for dtype in (torch.float64, torch.float32):
        a = gs.flatten(train.loss_and_grads(**c, dtype=dtype))
        b = gs.flatten(train.loss_and_grads(**c, dtype=dtype, operand_round=train.identity))
        for k in a:
            assert np.array_equal(a[k], b[k]), (dtype, k)
    f = gs.flatten(train.loss_and_grads(**c, dtype=torch.float64, operand_round=train.identity, attn_fold=True))
    truth = gs.flatten(train.loss_and_grads(**c, dtype=torch.float64))
    for k in truth:
        assert np.abs(f[k] - truth[k]).max() <= 1e-12 * max(np.abs(truth[k]).max(), 1e-300), k


def test_float64_gradients_against_central_finite_differences():
    """Independent of autograd: (L(x + h) - L(x - h)) / 2h in float64 on 20 sampled elements per tensor.
    Step and bound.  The error of a central difference is  h^2 |L'''| / 6  (truncation)  +  eps_L |L| / h  (rounding of the two losses).
    L is a mean over B x 3 x N squared residuals evaluated with ~1e4 float64 operations per point: eps_L <= 1e-15 relative is generous, so
    with |L| ~ 1 the rounding term is 1e-15 / h.  Along one coordinate the loss curves on the scale of that coordinate (LayerNorm, the
    softmax and 1/variance-like dependence): |L'''| <= c^2 |L'| / s^2 with s the element's scale (|x|, at least 1e-2: the smallest
    variances) and c a stiffness factor; c <= 30 covers a softmax logit or a LayerNorm input moved by its own size.  With h = 1e-5 s the
    truncation term is 1e-10 c^2 / 6 <= 1.5e-8 of |L'| and the rounding term 1e-10 / s <= 1e-8 absolute.  Bound: 1e-7 |g| + 4e-8 —
    the two terms with a factor 4 to 6; an autograd mistake (a missing term, a wrong site) is O(1) of |g|."""
    g, c = load_case("B3_N64_T10")
    r = gs.flatten(train.loss_and_grads(**c, dtype=torch.float64))
    r.update({"x_t": r["d_x"], "variances_pt": r["d_variances"], "ctx_mv": r["d_ctx_mv"]})
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)

    def loss(cc):
        with torch.no_grad():
            W = {k: tt(v) for k, v in cc["W"].items()}
            eps = torch_cpu.transformer_net_forward(W, tt(cc["x_t"]), torch.from_numpy(cc["t"].astype(np.int64)), [tt(cc["ctx_code"]), tt(cc["ctx_mv"])],
                                                    tt(cc["anchors_pt"]), tt(cc["variances_pt"]), torch.from_numpy(cc["valid"]),
                                                    torch.from_numpy(cc["assignment"]), dtype=torch.float64)
            return float(train.masked_mse(tt(cc["noise"]), eps, tt(cc["flags"])))

    rng = np.random.default_rng(3)
    c64 = dict(c, W={k: v.astype(np.float64) for k, v in c["W"].items()}, x_t=c["x_t"].astype(np.float64),
               variances_pt=c["variances_pt"].astype(np.float64), ctx_mv=c["ctx_mv"].astype(np.float64))
    blk = "transformer_blocks.3."
    worst = 0.0
    for name in ("x_t", "variances_pt", "ctx_mv", blk + "ff.net.0.proj.weight", blk + "ff.net.2.weight", blk + "attn2.to_q.weight", blk + "norm3.weight",
                 "proj_in.weight"):
        holder = c64["W"] if name in c64["W"] else c64
        base = holder[name]
        live = np.flatnonzero(np.abs(r[name]).ravel() > 0) if name in ("x_t", "variances_pt") else np.arange(base.size)   # (masked points have no gradient: FD would only confirm 0 = 0)
        for i in rng.choice(live, 20, replace=False):
            idx = np.unravel_index(i, base.shape)
            h = 1e-5 * max(abs(base[idx]), 1e-2)
            vals = []
            for s in (+1, -1):
                a = base.copy()
                a[idx] += s * h
                holder[name] = a
                vals.append(loss(c64))
            holder[name] = base
            fd, ag = (vals[0] - vals[1]) / (2 * h), r[name][idx]
            worst = max(worst, abs(fd - ag) / (1e-7 * abs(ag) + 4e-8))
            assert abs(fd - ag) <= 1e-7 * abs(ag) + 4e-8, (name, idx, fd, ag)
    print(f"finite differences: worst |fd - autograd| / bound = {worst:.3f}")


def _judge(s, got, pool=None, only=None):
    return gs.judge_outputs("bf16", got, s["truth"], s["yard"], True, pool, only)


def test_stand_in_kernel_is_accepted_under_the_committed_thresholds(selftest):
    """The rounding model in fp32 — bf16-rounded operands, fp32 accumulation and fp32 everything else — judged as the GPU gate judges a
    bf16 kernel: every tensor, every group ratio, the pools (both dropout settings fill them)."""
    pool = gs.Pool()
    for key, s in selftest.items():
        fails, rows = _judge(s, s["stand"], pool)
        worst = {k: max(r[4].get(k, 0.0) for r in rows) for k in ("rms", "max", *gs.GT)}
        print(f"stand-in {key}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
        assert not fails, "\n".join(fails)
    fails, rows = pool.judge("bf16")
    assert not fails, "\n".join(fails)
    assert gs.R32T >= 1.0 and gs.RBT >= 1.0 and gs.RMAXT >= 1.0 and min(gs.GT.values()) >= 1.0


@pytest.mark.parametrize("key", ["p0", "p0.2"])
def test_folded_stand_in_is_accepted_against_the_folded_model(selftest, key):
    """The fused path's yardstick (attn_fold + ff_fold, oracle/train.py) and its fp32 stand-in, as above; the folds equal the reference
    layout in real arithmetic, dropout scale on the folded W1 included; the shift between the two models is printed."""
    s = selftest[key]
    exact = s["run"](dtype=torch.float64, operand_round=train.identity, attn_fold=True, ff_fold=True)
    for k, v in s["truth"].items():
        assert np.abs(exact[k] - v).max() <= 1e-12 * max(np.abs(v).max(), 1e-300), k
    yfold = s["run"](dtype=torch.float64, operand_round=train.round_bf16, attn_fold=True, ff_fold=True)
    stand = s["run"](operand_round=train.round_bf16, attn_fold=True, ff_fold=True)
    fails, rows = gs.judge_outputs("bf16", stand, s["truth"], yfold, True)
    assert not fails, "\n".join(fails)
    fails, rows = _judge(s, yfold)
    for f, d in gs.worst_by_family(rows).items():
        print(f"folded model / reference-layout model {key}, {f}: " + " ".join(f"{k}={v[0]:.3f}" for k, v in d.items() if isinstance(v, tuple)))


#            mutation        dropout  the tensors at least one of whose failures must be among the reasons
MUTATIONS = [("truncate", "p0.2", None),
             ("fold_bias_term", "p0", ("ff.net.0.proj.weight",)),
             ("chunk_scale", "p0.2", (f"transformer_blocks.{train.MUT_BLOCK}.ff.net.0.proj.weight", f"transformer_blocks.{train.MUT_BLOCK}.ff.net.0.proj.bias")),
             ("halve_unit", "p0", (f"transformer_blocks.{train.MUT_BLOCK}.ff.net.0.proj.weight",)),
             ("stale_mask_tile", "p0.2", None),
             ("stem_dx_term", "p0", ("d_x", "d_variances"))]


@pytest.mark.parametrize("mutation,key,where", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_wrong_variant_of_the_stand_in_is_rejected(selftest, mutation, key, where):
    """Conditions on the committed thresholds (tests/_gradstats.py)."""
    s = selftest[key]
    fails, rows = _judge(s, s["run"](operand_round=train.round_bf16, mutate=mutation))
    print(f"{mutation}: {len(fails)} failures, e.g. {fails[:3]}")
    assert fails, f"{mutation} passes the acceptance function: a threshold is too wide"
    if where is not None:
        assert any(any(w in f.split(":")[0] for w in where) for f in fails), (mutation, fails[:5])
    if mutation in ("chunk_scale", "halve_unit"):   # the mutated tensor's own failures are what rejects it: nothing else changed
        assert all(where[0].rsplit(".", 1)[0] in f for f in fails), fails


def test_lost_lo_half_of_the_gradient_pair_is_reported(selftest):
    """Reported only: the gradient between two blocks rounded to bf16 (the pair's lo half lost).  Not required to fail."""
    for key, s in selftest.items():
        fails, rows = _judge(s, s["run"](operand_round=train.round_bf16, mutate="lost_lo"))
        worst = max(rows, key=lambda r: r[4]["rms"])
        print(f"lost_lo {key}: the gate {'SEES' if fails else 'does NOT see'} it ({len(fails)} failures; worst rms ratio {worst[4]['rms']:.3f} on {worst[0]})")
