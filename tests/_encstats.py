"""Test helper: the encoder side of the stage-1 step (PointNetV2 in train mode, the flows' prior loss) judged against a float64 truth ON THE
BRANCH THE IMPLEMENTATION TOOK, with tests/_gradstats.py's statistics, pools and acceptance function unchanged (R32T = 3.08 for fp32 kernels).

Both functions are piecewise smooth (ReLU units, a max over points).  No seed gives a batch whose units all stay clear of 0 at the sizes the
kernels care about, so two correct fp32 implementations routinely land on different pieces and their gradients then differ by whole units'
shares.  Hence, per case and per implementation X (the HIP kernels, the CPU stand-in of the self-test, the fp32 torch-CPU oracle):
  truth of X      the float64 oracle with branch = X's own branch (oracle/pointnet_v2_train.py, oracle/prior_loss.py: forced in the derivative
                  only).  The kernels' branch is exported by the library exactly as the backward derives it (training.pointnet_v2_branch /
                  prior_loss_branch); the fp32 oracle's is its own record.
  yardstick       the fp32 torch-CPU oracle's error against ITS truth.  Each side is measured on its own branch: a flip costs neither.
                  For PointNetV2 the oracle's heads and bn4 are restated (oracle/pointnet_v2_train.py: head_products="chain", head_bn="written"),
                  and the yardstick's rms and max-abs are the root mean square of those of YARD_DRAWS = 8 draws of that oracle's error: the
                  oracle as it stands and seven runs of the same function with every product summed in another order (pn_yardstick_draw), each
                  against float64 on its own branch.  See "What was found" below.
  legitimacy      a unit whose state differs from the float64 run's own state must be ambiguous: the float64 |pre-activation| (for the pool: the
                  float64 gap between the maximum and the runner-up) at most R32T x the fp32 oracle's max-abs error at that site.  Any other
                  differing unit is a failure that names it.  Pool state "none" (-1): the maximum is the 0 of a non-member point, zero
                  gradient whichever point is named.  Flow rows of absent parts carry no gradient and are not compared.
  judged          rms and max-abs of the error <= R32T x the yardstick's, for every tensor of >= 512 elements on its own; smaller ones pooled
                  by kind (gs.Pool: normalised by the yardstick's rms, over layers and cases, judged by the test file after its last case).
                  The mathematically zero gradients (a bias in front of a batch-statistics BatchNorm, and bn4.bias in front of the heads')
                  are judged the same way as a family of their own: the truth is ~1e-17 and the yardstick is the oracle's cancellation noise.
                  The prior loss itself is one number per case: it joins log_p's vector in log_p's unit (loss / kl_weight is an average of
                  log_p + entropy terms), so that kind is judged over all cases' valid parts and losses together.

What was found (nothing was widened; no defect in the kernels):
  * Against the oracle as it stood, the flows passed at once (<= 1.72 x rms, <= 3.00 x max-abs, B = 37 included) and so did every trunk tensor, but the heads'
    tensors measured 2.6 - 2.8 x rms throughout and 3.2 - 7.7 x on max-abs in every case (running statistics of the heads, head weights, biases),
    on the MI355X and, on the CPU, for a stand-in that merely sums K in two halves.  The cleanest probe is d mlp_v.4.bias — one K = 256 product
    and a sum over the B rows — at 2.64 - 2.74 x rms in every case.  Cause: torch's fp32 products sum K as one chain of multiply-adds from a few
    dozen rows on (bit-identical to a written-out chain for K <= 256 from 9 .. 64 rows on), but with FEWER rows — the heads: B = 2 .. 9 — they take
    interleaved partial sums whose rounding error measures 2.7 - 3.4 x smaller (K = 128 .. 512).  The kernels' fp32 matrix pipe is a chain at every
    row count.  Restated: head_products="chain".  With it the heads measure <= 2.07 x rms and the trunk's BatchNorm pools 1.13 x (1.59 x before).
  * The mathematically zero gradients of the heads (and conv4.bias behind them) still measured up to 5.3 x (stand-in) / 7.5 x (kernels) on max-abs:
    they are nothing but the rounding left over when sum(dz) of a BatchNorm cancels, and its size follows the arrangement of the backward, not
    its quality.  Restated: head_bn="written" — fp32 reductions in the order of a four-row-group workgroup and dz = g rstd (dy - sum(dy) / R -
    xhat sum(dy xhat) / R) as the kernels (and the stand-in) write it.
  * bn4's BatchNorm is written out in the yardstick like the heads': d conv4.bias is a zero gradient too, and where the kernels' was largest (2 x 33, channel
    187: 1.4e-3 against draws of +-3e-4) it is delta(mean) rstd^2 g d_gamma — the half-ulp the fp32 mean carries, with the mean taken as sum x fl(1 / R).
  * One draw of the yardstick is not a yardstick where the heads normalise over B = 2 .. 9 rows.  A channel whose batch variance is near eps multiplies the
    rounding that reaches it by up to 1 / sqrt(eps) = 316 and then carries a block's error alone.  At 2 x 33 channel 203 of mlp_m.1 (batch variance 0.15 eps)
    carries 97.6 % of the error of part 3 of mlp_m.4's running mean; what reaches it is the error of hz[0] - hz[1], to which the pooled input contributes
    -4.4e-6 in the kernels and +0.3e-6 in torch, while over all 1024 channels that contribution measures 1.98e-6 rms (kernels) and 1.97e-6 (torch), both equal
    to what independent errors of the measured size (pooled: 2.39e-6 and 2.34e-6 rms) give: the two are equally good and drew differently at the one channel that
    is amplified.  Hence the draws.  Reordering rows or relabelling hidden channels alone does not redraw torch's error (correlation 0.9999+ between such runs:
    the first layer's K = 3 products dominate what is inherited); relabelling the three coordinates as well does.
  * With all this every case of the GPU file is within the gate; 2 x 33 is the narrow one (2.95 x on one max-abs) and depends on the host's torch; that file's docstring.
"""
import re

import numpy as np
import torch

import _gradstats as gs

PN_CASES = [(2, 33), (5, 160), (4, 333), (8, 1024), (9, 1000), (5, 2048)]     # (B, N); >= 8192 rows: both statistics paths
PN_FROZEN_CASE = (3, 70)                                                       # momentum < 0: running statistics untouched
FLOW_CASES = [1, 6, 32, 37, 64, 65, 70]
# B = 1 and B = 6: the seeds, of 1 .. 15 tried on the CPU, whose smallest float64 |pre-activation| is furthest from 0 in units of the fp32 oracle's
# max-abs error at the site (clear_margin): 375 x and 12.8 x.  The other seeds give 5.7 .. 338 x at B = 1 and 0.3 .. 6.9 x at B = 6.
FLOW_SEED = {1: 10, 6: 11}
# Input draws of the PointNetV2 cases (default 0): the first of 0, 1, 2 under which fewer than 0.1 % of every site's units are ambiguous.  The heads'
# sites hold only 512 B .. 1024 B units, so three or four units near 0 are already too many at B = 5 and B = 3; 0 and 1 gave 0.16 / 0.12 % and 0.13 / 0.13 %.
PN_DRAW = {(5, 2048): 2, (3, 70): 2}
ZERO_GRAD = {f"conv{i}.bias" for i in (1, 2, 3, 4)} | {f"{h}.{i}.bias" for h in ("mlp_m", "mlp_v") for i in (0, 3)} | {"bn4.bias"}
# Draws of the PointNetV2 yardstick.  Where ONE ill-conditioned channel carries a tensor's error, error^2 is one chi-square draw for the kernels and the
# mean of YARD_DRAWS such draws for the yardstick: two equally good implementations exceed R32T^2 = 9.49 with probability P(F(1, 8) > 9.49) = 1.5 % at 8
# draws (20 % at one draw, 2.7 % at five); from there on more draws buy little and each costs an fp32 pass per case.
YARD_DRAWS = 8
PN_SITES = ("bn1", "bn2", "bn3", "mlp_m.1", "mlp_m.4", "mlp_v.1", "mlp_v.4")
FLOW_SITES = ("h1", "h2")


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def pn_case(B, N, wseed=2):
    """Shape 0 lacks part 2; at (4, 333) shape 1 holds the single part 3."""
    from difffacto_amd import synth
    rng = np.random.Generator(np.random.PCG64(B * 1000 + N + 100000 * PN_DRAW.get((B, N), 0)))
    x = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    seg = rng.integers(0, 4, size=(B, N))
    seg[0][seg[0] == 2] = 1
    if (B, N) == (4, 333):
        seg[1][:] = 3
    return dict(W=synth.make_pointnet_v2_weights(wseed), x=x, attn=np.eye(4, dtype=np.float32)[seg],
                dm=rng.standard_normal((B, 4, 256)).astype(np.float32), dv=rng.standard_normal((B, 4, 256)).astype(np.float32))


def flow_case(B, wseed=1):
    """Ragged validity from synth.make_latents; from B = 2 on the last shape has one valid part."""
    from difffacto_amd import synth
    rng = np.random.Generator(np.random.PCG64(FLOW_SEED.get(B, 3) * 100 + B))
    valid = synth.make_latents(B, seed=5)[3].copy()
    if B >= 2:
        valid[B - 1] = (0, 1, 0, 0)
    return dict(W=synth.make_latent_weights(wseed), part_code=rng.standard_normal((B, 256, 4)).astype(np.float32),
                logvar=(-2.0 + 0.5 * rng.standard_normal((B, 4, 256))).astype(np.float32), valid=valid.astype(np.float32), prior_var=1.0, kl_weight=5e-4)


# ---- branches --------------------------------------------------------------------------------------------------------------------------
def pn_branch_of_record(rec):
    b = {s: (rec["pre"][s] > 0).astype(np.uint8) for s in PN_SITES}
    b["pool"] = rec["sel"].astype(np.int32)
    return b


def pn_branch_of_export(exp, attn):
    """training.pointnet_v2_branch's tensors (as numpy) -> the oracle's branch: arg -> -1 where the named point is no member of the part."""
    b = {s: np.asarray(exp[s]).astype(np.uint8) for s in PN_SITES}
    arg = np.asarray(exp["arg"]).astype(np.int64)                                   # (B, 4, 512)
    B, A, _ = arg.shape
    hit = attn[np.arange(B)[:, None, None], arg, np.arange(A)[None, :, None]] != 0
    b["pool"] = np.where(hit, arg, -1).astype(np.int32)
    return b


def flow_branch_of_record(rec):
    return {s: (rec[s] > 0).astype(np.uint8) for s in FLOW_SITES}


def same_branch(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ---- oracles, once per case --------------------------------------------------------------------------------------------------------------
def pn_yardstick_draw(case, momentum, d):
    """Draw d >= 1 of the PointNetV2 yardstick: the same fp32 oracle summing every product in another order over K — the heads' chains take their
    terms in a drawn order (chain_order), and the trunk's channels are relabelled (the three coordinates, and the outputs of conv1 .. conv4
    together with their BatchNorm and the next layer's input columns: the same function, torch's products meet their terms in another order).  Results, running
    statistics, gradients and the record are mapped back to the original labels."""
    from oracle import pointnet_v2_train as pt
    rng = np.random.Generator(np.random.PCG64(4000 + d))
    perm = [np.roll(np.arange(3), d) if d % 3 else np.arange(3)[::-1].copy()] + [rng.permutation(c) for c in (128, 128, 256, 512)]   # [0]: the coordinates
    W = dict(case["W"])
    for i in (1, 2, 3, 4):
        w = case["W"][f"conv{i}.weight"][perm[i]]
        W[f"conv{i}.weight"] = np.ascontiguousarray(w[:, perm[i - 1]])
        for k in (f"conv{i}.bias", f"bn{i}.weight", f"bn{i}.bias", f"bn{i}.running_mean", f"bn{i}.running_var"):
            W[k] = np.ascontiguousarray(case["W"][k][perm[i]])
    for h in ("mlp_m", "mlp_v"):
        W[h + ".0.weight"] = np.ascontiguousarray(case["W"][h + ".0.weight"][:, perm[4]])
    r = pt.outputs_and_grads(W, np.ascontiguousarray(case["x"][:, :, perm[0]]), case["attn"], case["dm"], case["dv"], record="light", momentum=momentum, head_products="chain",
                             head_bn="written", chain_order=d)

    def back(a, i, j=None):          # a = original[perm[i]] (and [:, perm[j]]) -> original
        o = np.empty_like(a)
        if j is None:
            o[perm[i]] = a
        else:
            o[np.ix_(perm[i], perm[j])] = a
        return o

    for i in (1, 2, 3, 4):
        r["grads"][f"conv{i}.weight"] = back(r["grads"][f"conv{i}.weight"], i, i - 1)
        for k in (f"conv{i}.bias", f"bn{i}.weight", f"bn{i}.bias"):
            r["grads"][k] = back(r["grads"][k], i)
        for k in (f"bn{i}.running_mean", f"bn{i}.running_var"):
            r["running"][k] = back(r["running"][k], i)
        if i < 4:
            r["record"]["pre"][f"bn{i}"] = np.ascontiguousarray(back(r["record"]["pre"][f"bn{i}"].T, i).T)
    for h in ("mlp_m", "mlp_v"):
        g = r["grads"][h + ".0.weight"]
        o = np.empty_like(g)
        o[:, perm[4]] = g
        r["grads"][h + ".0.weight"] = o
    r["record"]["sel"] = np.ascontiguousarray(back(r["record"]["sel"].transpose(2, 0, 1), 4).transpose(1, 2, 0))
    return r


def pn_oracles(case, momentum=0.1):
    from oracle import pointnet_v2_train as pt
    args = (case["W"], case["x"], case["attn"], case["dm"], case["dv"])
    r64 = pt.outputs_and_grads(*args, dtype=torch.float64, record=True, momentum=momentum)
    r32 = pt.outputs_and_grads(*args, record=True, momentum=momentum, head_products="chain", head_bn="written")
    b64, b32 = pn_branch_of_record(r64["record"]), pn_branch_of_record(r32["record"])
    site_err = {s: float(np.abs(r32["record"]["pre"][s] - r64["record"]["pre"][s]).max()) for s in PN_SITES}
    site_err["pool"] = float(np.abs(r32["record"]["pool_in"] - r64["record"]["pool_in"]).max())
    margin = {s: r64["record"]["pre"][s] for s in PN_SITES}
    margin["pool"] = r64["record"]["gap"]
    cache = {}

    def truth(branch):
        """float64 on `branch`, once per distinct branch (the yardstick's draws share the trunk's and mostly the heads')."""
        if same_branch(branch, b64):
            return r64
        key = hash(tuple(np.ascontiguousarray(branch[k]).tobytes() for k in sorted(branch)))
        if key not in cache:
            cache[key] = pt.outputs_and_grads(*args, dtype=torch.float64, branch=branch, momentum=momentum)
        return cache[key]

    del r32["record"]["pool_in"], r64["record"]["pool_in"]
    orc = dict(kind="pn", r64=r64, r32=r32, b64=b64, b32=b32, t32=truth(b32), site_err=site_err, margin=margin, truth=truth, valid_rows=None)
    orc["yards"] = [(r32, orc["t32"])]
    for d in range(1, YARD_DRAWS):
        r = pn_yardstick_draw(case, momentum, d)
        orc["yards"].append((r, truth(pn_branch_of_record(r["record"]))))
    return orc


def flow_oracles(case):
    from oracle import prior_loss as pl
    args = (case["W"], case["part_code"], case["logvar"], case["valid"])
    kw = dict(prior_var=case["prior_var"], kl_weight=case["kl_weight"])
    r64 = pl.loss_and_grads(*args, dtype=torch.float64, record=True, **kw)
    r32 = pl.loss_and_grads(*args, record=True, **kw)
    b64, b32 = flow_branch_of_record(r64["record"]), flow_branch_of_record(r32["record"])
    site_err = {s: float(np.abs(r32["record"][s] - r64["record"][s]).max()) for s in FLOW_SITES}
    margin = {s: r64["record"][s] for s in FLOW_SITES}
    truth = lambda branch: r64 if same_branch(branch, b64) else pl.loss_and_grads(*args, dtype=torch.float64, branch=branch, **kw)
    rows = np.ascontiguousarray(case["valid"].T).ravel() != 0                      # part-major rows of present parts
    t32 = truth(b32)
    return dict(kind="flow", r64=r64, r32=r32, b64=b64, b32=b32, t32=t32, site_err=site_err, margin=margin, truth=truth, valid_rows=rows, yards=[(r32, t32)])


# ---- legitimacy ------------------------------------------------------------------------------------------------------------------------
def differing(orc, branch, site):
    """Boolean array: the units of `site` whose state in `branch` is not the float64 run's own."""
    if site == "pool":
        return branch["pool"] != orc["b64"]["pool"]
    d = (branch[site] != 0) != (orc["b64"][site] != 0)
    if orc["valid_rows"] is not None:
        d = d & orc["valid_rows"][None, :, None]
    return d


def ambiguous(orc, site):
    """Boolean array: the units of `site` whose float64 margin is at most R32T x the fp32 oracle's max-abs error there."""
    m = np.abs(orc["margin"][site]) <= gs.R32T * orc["site_err"][site]
    if orc["valid_rows"] is not None:
        m = m & orc["valid_rows"][None, :, None]
    return m


def legitimacy(orc, branch, who):
    """(failures, {site: differing units}) of a branch against the float64 run's own."""
    fails, counts = [], {}
    for site in orc["margin"]:
        d = differing(orc, branch, site)
        counts[site] = int(d.sum())
        bad = d & ~ambiguous(orc, site)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            fails.append(f"{who}: unit {site}{at} is not on the float64 branch and is not ambiguous: margin {abs(float(orc['margin'][site][at])):.3e} > "
                         f"{gs.R32T} x site error {orc['site_err'][site]:.3e} ({int(bad.sum())} such units at this site)")
    return fails, counts


def clear_margin(orc, sites=None):
    """The smallest float64 margin over the compared units, in units of the site's fp32 error (> R32T: no unit is ambiguous)."""
    out = np.inf
    for site in sites or orc["margin"]:
        m = np.abs(orc["margin"][site])
        if orc["valid_rows"] is not None:
            m = m[:, orc["valid_rows"], :]
        out = min(out, float(m.min()) / orc["site_err"][site])
    return out


# ---- flattening and families -------------------------------------------------------------------------------------------------------------
def pn_flatten(r, running=True):
    out = {"m": r["m"], "v": r["v"]}
    if running:
        out.update({"run/" + k: a for k, a in r["running"].items()})
    out.update({"g/" + k: a for k, a in r["grads"].items()})
    return out


def flow_flatten(r, case):
    """log_p of the present parts and the loss in log_p's unit as one vector; entropy of the present parts; the gradients."""
    present = case["valid"] != 0
    out = {"loss_terms": np.concatenate([np.asarray(r["log_p"], dtype=np.float64)[present], [float(r["loss"]) / case["kl_weight"]]]),
           "entropy": np.asarray(r["entropy"], dtype=np.float64)[present], "d_part_code": r["d_part_code"], "d_logvar": r["d_logvar"]}
    out.update({"g/" + k: a for k, a in r["grads"].items()})
    return out


_FLOW = re.compile(r"^g/flow\.\d+\.chain\.\d+\.(net_s_t\.\d\.(?:weight|bias))$")


def family(name):
    if name in ("m", "v"):
        return "out"
    if name.startswith("run/"):
        return "running"
    f = _FLOW.match(name)
    if f:
        return f.group(1)
    if not name.startswith("g/"):
        return name
    p = name[2:]
    if p in ZERO_GRAD:
        return "zero"
    if p.startswith("conv"):
        return "conv1.weight" if p == "conv1.weight" else "trunk.weight"
    if p.startswith("bn4"):
        return "bn4.weight"
    if p.startswith("bn"):
        return "trunk_bn." + p.split(".")[1]
    layer, kind = p.split(".")[1:]
    return "head." + kind if layer in "036" else "head_bn." + kind


def judge(label, orc, got, branch, flatten, pool, who="kernel"):
    """got: an implementation's result in the oracle's layout, branch: its own branch.  Returns (failures, printed lines); small tensors go to `pool`."""
    fails, counts = legitimacy(orc, branch, who)
    _, counts32 = legitimacy(orc, orc["b32"], "fp32 oracle")
    flips = " ".join(f"{s}={counts[s]}/{counts32[s]}" for s in counts)
    truth, mine = flatten(orc["truth"](branch)), flatten(got)
    yards = [(flatten(y), flatten(yt)) for y, yt in orc["yards"]]
    fam = {}
    for name, t in truth.items():
        t = np.asarray(t, dtype=np.float64)
        ek = np.asarray(mine[name], dtype=np.float64) - t
        eys = [np.asarray(y[name], dtype=np.float64) - np.asarray(yt[name], dtype=np.float64) for y, yt in yards]
        assert ek.shape == t.shape == eys[0].shape, (name, ek.shape, t.shape, eys[0].shape)
        f = family(name)
        if t.size < gs.MIN_GROUP:
            pool.add(f, ek, eys[0])
            continue
        k, ys = gs.stats(ek), [gs.stats(e) for e in eys]
        y = dict(ys[0], rms=float(np.sqrt(np.mean([d["rms"] ** 2 for d in ys]))), max=float(np.sqrt(np.mean([d["max"] ** 2 for d in ys]))))
        r = gs.ratios(k, y)
        fails += [f"{name}: {m}" for m in gs.accept("f32", k, y)]
        d = fam.setdefault(f, dict(n=0, rms=(-1.0, ""), max=(-1.0, "")))
        d["n"] += 1
        for key in ("rms", "max"):
            if r[key] > d[key][0]:
                d[key] = (r[key], name)
    lines = [f"ENCHP {label} [{who}] {f} x{d['n']}: ratio rms {d['rms'][0]:.3f} ({d['rms'][1]}) max {d['max'][0]:.3f} ({d['max'][1]}) | "
             f"flips {who}/fp32-oracle {flips}" for f, d in sorted(fam.items())]
    return [f"{label}: {m}" for m in fails], lines


def judge_pool(pool, who="kernel"):
    fails, rows = pool.judge("f32")
    return fails, [f"ENCHP-POOL [{who}] {p} n={k['n']}: ratio rms {r['rms']:.3f} max {r['max']:.3f}" for p, k, y, r in rows]


def absent_rows_exactly_zero(r, case):
    """d_part_code (B,256,4) and d_logvar (B,4,256): the rows of absent parts."""
    absent = case["valid"] == 0
    fails = []
    if np.any(np.asarray(r["d_part_code"]).transpose(0, 2, 1)[absent] != 0):
        fails.append("d_part_code is not exactly 0 in a row of an absent part")
    if np.any(np.asarray(r["d_logvar"])[absent] != 0):
        fails.append("d_logvar is not exactly 0 in a row of an absent part")
    return fails
