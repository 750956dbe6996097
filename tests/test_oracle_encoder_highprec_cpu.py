"""CPU self-test of the encoder-side float64 gate (tests/_encstats.py): the acceptance function and the legitimacy rule have teeth at exactly
the thresholds tests/test_gpu_encoder_train_highprec.py uses.

Stand-in kernels: fp32 restatements of PointNetV2's training step and of the prior loss with another summation order than the torch-CPU
oracle's — the points of every shape (the shapes of the flows' batch) permuted, every product with K >= 128 summed as two halves, BatchNorm
statistics as (count, mean, M2) pieces of 257 rows merged by Chan's formula, BatchNorm's backward written out with column sums over the same
pieces — and their own branch recorded.  They must pass; eight deliberately wrong variants must each be rejected; and the cases of the GPU
file must meet the conditions the method rests on (the fp32 oracle's own flips are all ambiguous, ambiguous units are < 0.1 % of a site).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _encstats as es  # noqa: E402
import _gradstats as gs  # noqa: E402

PIECE = 257


# ---- the stand-in kernels ----------------------------------------------------------------------------------------------------------------
def _lin(x, W, b):
    K = W.shape[1]
    if K < 128:
        return x @ W.t() + b
    h = K // 2
    return (x[:, :h] @ W[:, :h].t() + x[:, h:] @ W[:, h:].t()) + b


def _piece_sum(a):
    return torch.stack([p.sum(0) for p in a.split(PIECE)]).sum(0)


def _chan_stats(z):
    """(mean, biased variance) of the columns of z from (count, mean, M2) pieces merged left to right."""
    cnt, mean, m2 = 0, None, None
    for p in z.split(PIECE):
        c, mt = p.shape[0], p.mean(0)
        q = ((p - mt) ** 2).sum(0)
        if cnt == 0:
            mean, m2 = mt, q
        else:
            d, tot = mt - mean, cnt + c
            mean, m2 = mean + d * (c / tot), m2 + q + d * d * (cnt * c / tot)
        cnt += c
    return mean, m2 / cnt


class _BN(torch.autograd.Function):
    """y = xhat g + b with the batch-statistics backward written out; no_xhat_term: a channel whose dz lacks xhat mean(dy xhat) (a wrong variant)."""

    @staticmethod
    def forward(ctx, z, g, b, mu, rstd, no_xhat_term):
        xhat = (z - mu) * rstd
        ctx.save_for_backward(xhat, rstd, g)
        ctx.no_xhat_term = no_xhat_term
        return xhat * g + b

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd, g = ctx.saved_tensors
        R = dy.shape[0]
        dbeta, dgamma = _piece_sum(dy), _piece_sum(dy * xhat)
        coef = dgamma / R
        if ctx.no_xhat_term is not None:
            coef = coef.clone()
            coef[ctx.no_xhat_term] = 0
        return g * rstd * (dy - dbeta / R - xhat * coef), dgamma, dbeta, None, None, None


def standin_pn(case, momentum=0.1, wrong=None, eps=1e-5):
    """-> (result in the layout of oracle.pointnet_v2_train.outputs_and_grads, its own branch in the layout of es.pn_branch_of_record)."""
    W = {k: torch.from_numpy(a.copy()) for k, a in case["W"].items()}
    for k, t in W.items():
        if "running" not in k:
            t.requires_grad_(True)
    x, attn = case["x"], case["attn"]
    B, N, A = attn.shape
    rng = np.random.Generator(np.random.PCG64(7))
    perm = np.stack([rng.permutation(N) for _ in range(B)])
    rows = (np.arange(B)[:, None] * N + perm).ravel()
    h = torch.from_numpy(x.reshape(B * N, 3)[rows])
    at = torch.from_numpy(attn.reshape(B * N, A)[rows]).view(B, N, A)
    running, branch = {}, {}

    def bn_relu(z, p, site, relu=True):
        mu, var = _chan_stats(z.detach())
        R = z.shape[0]
        if momentum >= 0:
            unbias = 1.0 if wrong == "running_var_biased" else R / (R - 1)
            running[p + "running_mean"] = ((1 - momentum) * W[p + "running_mean"] + momentum * mu).numpy()
            running[p + "running_var"] = ((1 - momentum) * W[p + "running_var"] + momentum * var * unbias).numpy()
        else:
            running[p + "running_mean"], running[p + "running_var"] = W[p + "running_mean"].numpy().copy(), W[p + "running_var"].numpy().copy()
        y = _BN.apply(z, W[p + "weight"], W[p + "bias"], mu, 1.0 / torch.sqrt(var + eps), 5 if (wrong == "bn2_no_xhat_term" and p == "bn2.") else None)
        if not relu:
            return y
        branch[site] = (y.detach() > 0).numpy().astype(np.uint8)
        return torch.relu(y)

    for i in (1, 2, 3, 4):
        h = bn_relu(_lin(h, W[f"conv{i}.weight"][:, :, 0], W[f"conv{i}.bias"]), f"bn{i}.", f"bn{i}", relu=i < 4)
    for s in es.PN_SITES[:3]:                                  # back to the callers' point order
        m = np.empty_like(branch[s])
        m[rows] = branch[s]
        branch[s] = m
    w = h.view(B, N, 1, 512) * at.view(B, N, A, 1) * A          # (B, N, A, 512)
    mx, idx = w.max(1)                                          # (B, A, 512)
    hit = at.permute(0, 2, 1).unsqueeze(-1).expand(B, A, N, 512).gather(2, idx.unsqueeze(2)).squeeze(2) != 0
    branch["pool"] = np.where(hit.numpy(), np.take_along_axis(perm[:, None, :], idx.numpy().reshape(B, 1, -1), 2).reshape(B, A, 512), -1).astype(np.int32)
    pooled = mx
    if wrong == "pool_runner_up":                               # one unit's gradient goes to the second-best member point (the value stays the maximum's)
        member = torch.where(at.permute(0, 2, 1).unsqueeze(-1) != 0, w.detach().permute(0, 2, 1, 3), torch.tensor(float("-inf")))   # (B, A, N, 512)
        b_, a_, c_ = 1, 0, 17
        assert bool(hit[b_, a_, c_])
        idx = idx.clone()
        idx[b_, a_, c_] = member[b_, a_, :, c_].topk(2).indices[1]
        picked = w.gather(1, idx.unsqueeze(1)).squeeze(1)
        pooled = picked + (mx - picked).detach()
    outs = []
    for name in ("mlp_m", "mlp_v"):
        t = pooled
        for conv, bnl, C in ((0, 1, 256), (3, 4, 128)):
            Wc, bc = W[f"{name}.{conv}.weight"][:, :, 0], W[f"{name}.{conv}.bias"]
            z = torch.cat([_lin(t[:, a], Wc[a * C:(a + 1) * C], bc[a * C:(a + 1) * C]) for a in range(A)], 1)
            t = bn_relu(z, f"{name}.{bnl}.", f"{name}.{bnl}").view(B, A, C)
        Wc, bc = W[name + ".6.weight"][:, :, 0], W[name + ".6.bias"]
        Z = Wc.shape[0] // A
        outs.append(torch.stack([_lin(t[:, a], Wc[a * Z:(a + 1) * Z], bc[a * Z:(a + 1) * Z]) for a in range(A)], 1))
    m, v = outs
    ((m * torch.from_numpy(case["dm"])).sum() + (v * torch.from_numpy(case["dv"])).sum()).backward()
    grads = {k: t.grad.numpy().copy() for k, t in W.items() if t.requires_grad}
    if wrong == "conv3_row_halved":
        grads["conv3.weight"][7] *= 0.5
    return dict(m=m.detach().numpy(), v=v.detach().numpy(), running=running, grads=grads), branch


def standin_flow(case, wrong=None, depth=14):
    """-> (result in the layout of oracle.prior_loss.loss_and_grads, its own branch)."""
    import math
    W = {k: torch.from_numpy(a.copy()).requires_grad_(True) for k, a in case["W"].items() if k.startswith("flow.")}
    z = torch.from_numpy(case["part_code"].copy()).requires_grad_(True)
    lv = torch.from_numpy(case["logvar"].copy()).requires_grad_(True)
    B, C, M = z.shape
    p = np.random.Generator(np.random.PCG64(9)).permutation(B)
    valid = torch.from_numpy(case["valid"][p])
    zp, lvp = z[p], lv[p]
    pre = {s: np.zeros((depth, M * B, 256), dtype=np.float32) for s in es.FLOW_SITES}
    cols = []
    for i in range(M):
        x = zp[:, :, i]
        logdet = torch.zeros(B)
        for l in range(depth):
            pf = f"flow.{i}.chain.{l}.net_s_t."
            if l % 2 == 0:
                x = torch.cat([x[:, 128:], x[:, :128]], 1)
            h1 = _lin(x[:, :128], W[pf + "0.weight"], W[pf + "0.bias"])
            h2 = _lin(torch.relu(h1), W[pf + "2.weight"], W[pf + "2.bias"])
            st = _lin(torch.relu(h2), W[pf + "4.weight"], W[pf + "4.bias"])
            pre["h1"][l, i * B + p], pre["h2"][l, i * B + p] = h1.detach().numpy(), h2.detach().numpy()
            scale = torch.sigmoid(st[:, :128] + 2.0)
            y1 = x[:, 128:] * scale + st[:, 128:]
            ld = torch.log(scale).sum(1)
            logdet = logdet + (ld.detach() if (wrong == "logdet_dropped" and (i, l) == (2, 5)) else ld)
            x = torch.cat([y1, x[:, :128]], 1) if l % 2 == 0 else torch.cat([x[:, :128], y1], 1)
        log_pw = (-math.log(case["prior_var"]) - 0.5 * math.log(2 * math.pi) * C - x.pow(2) / (2.0 * case["prior_var"])).sum(1)
        cols.append(torch.where(valid[:, i] == 1, log_pw + logdet, torch.zeros(B)))
    log_p = torch.stack(cols, 1)
    ent = 0.5 * lvp.sum(2) + 0.5 * C * (1.0 + math.log(2 * math.pi))
    loss = case["kl_weight"] * (((-log_p - ent) * valid).sum(1) / valid.sum(1)).mean()
    loss.backward()
    unperm = lambda a: a.detach().numpy()[np.argsort(p)]
    r = dict(loss=float(loss.detach()), log_p=unperm(log_p), entropy=unperm(ent), d_part_code=z.grad.numpy().copy(), d_logvar=lv.grad.numpy().copy(),
             grads={k: t.grad.numpy() for k, t in W.items()})
    if wrong == "d_logvar_scaled":
        r["d_logvar"] *= np.float32(1.001)
    if wrong == "absent_row_nonzero":
        b, i = np.argwhere(case["valid"] == 0)[0]
        r["d_part_code"][b, :, i] = 1e-12
    return r, {s: (a > 0).astype(np.uint8) for s, a in pre.items()}


# ---- shared oracles ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pn(B, N):
    case = es.pn_case(B, N)
    return case, es.pn_oracles(case)


@functools.lru_cache(maxsize=None)
def _flow(B):
    case = es.flow_case(B)
    return case, es.flow_oracles(case)


_POOL = gs.Pool()
PN_PASS = [(2, 33), (5, 160), (4, 333), (8, 1024)]
FLOW_PASS = [6, 37]


def _judge_pn(B, N, wrong=None, pool=None, flip=None):
    case, orc = _pn(B, N)
    got, branch = standin_pn(case, wrong=wrong)
    if flip is not None:
        branch = flip(orc, branch)
    return es.judge(f"B{B}_N{N}", orc, got, branch, es.pn_flatten, gs.Pool() if pool is None else pool, who="stand-in")


def _judge_flow(B, wrong=None, pool=None):
    case, orc = _flow(B)
    got, branch = standin_flow(case, wrong=wrong)
    fails, lines = es.judge(f"flows_B{B}", orc, got, branch, functools.partial(es.flow_flatten, case=case), gs.Pool() if pool is None else pool, who="stand-in")
    return fails + es.absent_rows_exactly_zero(got, case), lines


# ---- the stand-ins pass --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pn_pass(B, N):
    return _judge_pn(B, N, pool=_POOL)


@functools.lru_cache(maxsize=None)
def _flow_pass(B):
    return _judge_flow(B, pool=_POOL)


@pytest.mark.parametrize("B,N", PN_PASS)
def test_standin_encoder_passes(B, N):
    fails, lines = _pn_pass(B, N)
    print("\n".join(lines))
    assert not fails, "\n".join(fails)
    assert len(lines) >= 8


@pytest.mark.parametrize("B", FLOW_PASS)
def test_standin_prior_loss_passes(B):
    fails, lines = _flow_pass(B)
    print("\n".join(lines))
    assert not fails, "\n".join(fails)


def test_standin_small_tensors_pooled_over_the_cases_pass():
    for B, N in PN_PASS:
        _pn_pass(B, N)
    for B in FLOW_PASS:
        _flow_pass(B)
    pool = _POOL
    for p in [p for p in pool.k if sum(len(a) for a in pool.k[p]) < gs.MIN_GROUP]:    # log_p + loss and entropy: 130-odd values from these two flow batches; the GPU file's seven fill them
        assert p in ("entropy", "loss_terms"), p
        del pool.k[p], pool.y[p]
    fails, lines = es.judge_pool(pool, who="stand-in")
    print("\n".join(lines))
    assert not fails, "\n".join(fails)
    assert {"conv1.weight", "trunk_bn.weight", "trunk_bn.bias", "running", "zero", "net_s_t.0.bias"} <= set(pool.k)


def test_standin_takes_another_branch_somewhere_and_differs_in_bits():
    """Otherwise the stand-in would not exercise what the gate is for."""
    case, orc = _pn(8, 1024)
    got, branch = standin_pn(case)
    assert not np.array_equal(got["grads"]["conv2.weight"], orc["r32"]["grads"]["conv2.weight"])
    case, orc = _flow(37)
    got, branch = standin_flow(case)
    assert not np.array_equal(got["grads"]["flow.0.chain.0.net_s_t.0.weight"], orc["r32"]["grads"]["flow.0.chain.0.net_s_t.0.weight"])


# ---- the wrong variants are rejected ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong,where", [("bn2_no_xhat_term", "g/"), ("running_var_biased", "running_var"), ("pool_runner_up", "g/"),
                                         ("conv3_row_halved", "g/conv3.weight")])
@pytest.mark.parametrize("B,N", [(5, 160), (8, 1024)])
def test_wrong_encoder_variant_is_rejected(B, N, wrong, where):
    fails, _ = _judge_pn(B, N, wrong=wrong)
    assert any(where in f for f in fails), (wrong, fails)


@pytest.mark.parametrize("wrong,where", [("logdet_dropped", "g/flow.2.chain.5"), ("d_logvar_scaled", "d_logvar"), ("absent_row_nonzero", "absent part")])
@pytest.mark.parametrize("B", FLOW_PASS)
def test_wrong_prior_loss_variant_is_rejected(B, wrong, where):
    fails, _ = _judge_flow(B, wrong=wrong)
    assert any(where in f for f in fails), (wrong, fails)


@pytest.mark.parametrize("site", ["bn2", "mlp_v.4", "pool"])
def test_a_flipped_unit_with_a_clear_margin_is_rejected_by_name(site):
    """A mask bit (a pool selection) flipped on the unit whose float64 margin is closest to 100 x the site's fp32 error from above: the numbers the
    implementation returns are untouched, the legitimacy rule alone must refuse the branch and name the unit."""
    named = []

    def flip(orc, branch):
        m = np.abs(orc["margin"][site]).astype(np.float64)
        m[m < 100 * orc["site_err"][site]] = np.inf
        if site == "pool":
            m[branch["pool"] < 0] = np.inf
        at = np.unravel_index(np.argmin(m), m.shape)
        assert np.isfinite(m[at])
        out = dict(branch)
        out[site] = branch[site].copy()
        if site == "pool":
            out[site][at] = (branch[site][at] + 1) % 160
        else:
            out[site][at] ^= 1
        named.append(f"unit {site}{tuple(int(i) for i in at)}")
        return out

    fails, _ = _judge_pn(5, 160, flip=flip)
    assert any(named[0] in f and "not ambiguous" in f for f in fails), (named, fails)


# ---- the conditions the method rests on, for every case of the GPU file ----------------------------------------------------------------------
def _conditions(orc, label):
    fails, counts = es.legitimacy(orc, orc["b32"], "fp32 oracle")
    assert not fails, (label, fails)
    for site in orc["margin"]:
        amb = es.ambiguous(orc, site)
        assert amb.mean() < 1e-3, (label, site, int(amb.sum()), amb.size)
    return counts


@pytest.mark.parametrize("B,N", es.PN_CASES + [es.PN_FROZEN_CASE])
def test_case_conditions_encoder(B, N):
    print(f"B{B}_N{N}: the fp32 oracle's units off the float64 branch, all ambiguous:", _conditions(_pn(B, N)[1], (B, N)))


@pytest.mark.parametrize("B", es.FLOW_CASES)
def test_case_conditions_prior_loss(B):
    case, orc = _flow(B)
    print(f"flows B{B}: the fp32 oracle's units off the float64 branch, all ambiguous:", _conditions(orc, B))
    if B >= 2:
        assert case["valid"][B - 1].sum() == 1 and (case["valid"].sum(1) < 4).any()
    if B in es.FLOW_SEED:
        assert es.clear_margin(orc) > 2 * gs.R32T, es.clear_margin(orc)     # nothing within twice the ambiguity band: the branch is unique
