"""Test helper: error statistics of a denoiser output (B, 3, N) against the float64 oracle, and the acceptance function that
judges a kernel's statistics against a yardstick computed in the same test (oracle/highprec.py) — never a stored number.

Statistics: max-abs and rms over the tensor, and for each grouping the rms of every group relative to the overall rms.  An
error that sits in one lane, one wavefront slot, one tile, one shape or one output coordinate is the LAST thing a max-abs
over the tensor sees and the FIRST thing its group's rms sees.  No mean-of-error (bias) statistic: the weight rounding is
shared by all points, so the rounding model's own mean error is 30 to 50 standard errors from zero.
"""
import numpy as np

# point index n, shape b, output coordinate c -> group id
GROUPINGS = {
    "lane": lambda b, c, n: n % 32,            # lane of the 32-point tile of one wavefront
    "lane16": lambda b, c, n: n % 16,          # point within half a 32-point tile
    "wave": lambda b, c, n: (n // 32) % 8,     # wavefront slot in the 256-point workgroup
    "tile": lambda b, c, n: n // 256,          # workgroup tile
    "shape": lambda b, c, n: b,
    "coord": lambda b, c, n: c,
}
MIN_GROUP = 512     # a group ratio is asserted only where every group of the grouping holds this many error values

# ---- thresholds of the GPU gate (tests/test_gpu_denoiser_highprec.py) -------------------------------------------------------------
# Each one is the largest ratio measured on the MI355X over all cases of that file x 1.25 (profiles/highprec_parity.txt), cut to the
# cap where the product exceeds it.  The caps are enforced by tests/test_oracle_highprec_cpu.py: RB < 1.5 and G[lane], G[lane16],
# G[wave] <= 1.25, so that every deliberately wrong variant of the rounding model fails; R32 <= 8.
#                measured worst  x 1.25   threshold
#   R32             6.69          8.36     8.0  (cap)    eps B3_N100 t=0, k_denoise_pipe_f32<8> and k_denoise<f32> (bit-identical)
#   RB              1.134         1.418    1.42          eps_t B4_N2048, shape 3 (t = 500) on its own, k_denoise_pipe<8>
#   RMAX            1.223         1.529    1.53          eps B4_N2048 t=6, outlier weights, fold moved to channel 109
#   G[lane]         1.170         1.463    1.25 (cap)    same case
#   G[lane16]       1.087         1.359    1.25 (cap)    same case
#   G[wave]         1.060         1.325    1.25 (cap)    same case
#   G[tile]         1.090         1.363    1.37          eps B1_N8192 t=5
#   G[shape]        1.312         1.640    1.64          eps B12_N2048 t=500 (the rounding model's own worst shape there: 1.30)
#   G[coord]        1.320         1.650    1.65          eps B1_N8192 t=500, outlier weights
# A worst-group ratio is >= 1 by construction, so 1.25 x measured always exceeds the 1.25 cap of the lane and wavefront groupings: there
# the cap is the threshold (kernel and yardstick are deterministic on fixed seeds; the measured values leave 7 to 18 %).  R32: the fp32
# kernels' error is rms 7.6e-7 in every case, 3 to 6.7 times the numpy oracle's, because the MFMA chain accumulates the to_out and FF
# products straight into the fp32 residual stream (h is the C operand), so each of the 64 / 256 accumulation steps rounds at the size
# of h instead of the size of the product; the numpy oracle restated with that accumulation order (oracle/highprec.py:
# fp32_residual_order_forward, checked in tests/test_oracle_highprec_cpu.py) gives rms 5.5e-7 .. 8.4e-7 on the B3_N100 case (one rounding
# per two / per one term).  Arithmetic of the fused design, not a defect; the cap leaves 19 %.
R32 = 8.0           # fp32 kernels: rms and max-abs <= R32 x the fp32 numpy oracle's
RB = 1.42           # bf16 kernels: rms <= RB x the rounding model's
RMAX = 1.53         # bf16 kernels: max-abs <= RMAX x the rounding model's (an extreme-value statistic: its own factor)
G = {"lane": 1.25, "lane16": 1.25, "wave": 1.25, "tile": 1.37, "shape": 1.64, "coord": 1.65}


def stats(err, groupings=tuple(GROUPINGS)):
    """err (B, 3, N) -> dict(max, rms, n, groups={name: dict(worst=ratio, at=group id, min_count=values in the smallest group)})."""
    err = np.asarray(err, dtype=np.float64)
    assert err.ndim == 3 and err.shape[1] == 3, err.shape
    B, _, N = err.shape
    sq = err * err
    rms = float(np.sqrt(sq.mean()))
    out = dict(max=float(np.abs(err).max()), rms=rms, n=err.size, groups={})
    b, c, n = np.meshgrid(np.arange(B), np.arange(3), np.arange(N), indexing="ij")
    for name in groupings:
        gid = GROUPINGS[name](b, c, n).ravel()
        cnt = np.bincount(gid)
        ms = np.bincount(gid, weights=sq.ravel()) / np.maximum(cnt, 1)
        ratio = np.sqrt(ms) / rms if rms > 0 else np.zeros_like(ms)
        ratio[cnt == 0] = 0.0
        at = int(np.argmax(ratio))
        out["groups"][name] = dict(worst=float(ratio[at]), at=at, min_count=int(cnt[cnt > 0].min()))
    return out


def ratios(kernel, yardstick):
    """The figures `accept` judges: rms and max-abs of the kernel relative to the yardstick, and the kernel's worst group ratios of the
    groupings whose groups are all large enough."""
    r = dict(rms=kernel["rms"] / yardstick["rms"], max=kernel["max"] / yardstick["max"])
    for name, g in kernel["groups"].items():
        if g["min_count"] >= MIN_GROUP:
            r[name] = g["worst"]
    return r


def accept(prec, kernel, yardstick, groupings=(), floor=None):
    """Failures (empty list = accepted) of a kernel's `stats` against the yardstick's `stats` of the same case: the fp32 numpy
    oracle's error for prec = "f32", the bf16 rounding model's error for prec = "bf16".  `groupings`: the group ratios to assert
    (bf16 only); one whose smallest group holds fewer than MIN_GROUP values is an error of the test, not skipped.

    `floor` (bf16 only; the DDIM x_{t-1} and nothing else): the fp32 numpy oracle's `stats` on the same output.  The DDIM update
    cancels its two eps terms at small t, the rounding model's error falls to 1e-10 there and what a bf16 kernel still shows is the
    fp32 rounding of the update, which runs in fp32 in both precisions; the rms and max bounds are then the sum of both yardsticks'."""
    fails = []
    if prec == "f32":
        assert floor is None
        for k in ("rms", "max"):
            if not kernel[k] <= R32 * yardstick[k]:
                fails.append(f"{k} {kernel[k]:.3e} > {R32} x {yardstick[k]:.3e}")
        return fails
    assert prec == "bf16", prec
    for k, factor in (("rms", RB), ("max", RMAX)):
        if floor is None:
            if not kernel[k] <= factor * yardstick[k]:
                fails.append(f"{k} {kernel[k]:.3e} > {factor} x {yardstick[k]:.3e}")
        elif not kernel[k] <= factor * yardstick[k] + R32 * floor[k]:
            fails.append(f"{k} {kernel[k]:.3e} > {factor} x {yardstick[k]:.3e} + {R32} x {floor[k]:.3e}")
    for name in groupings:
        g = kernel["groups"][name]
        assert g["min_count"] >= MIN_GROUP, f"grouping {name}: a group of {g['min_count']} values is too small to judge"
        if not g["worst"] <= G[name]:
            fails.append(f"{name} group {g['at']}: rms {g['worst']:.3f} x overall > {G[name]}")
    return fails


def line(label, variant, kernel, yardstick):
    """One printed line per case: variant, max, rms, ratios, worst group and which one."""
    r = ratios(kernel, yardstick)
    gs = {k: v for k, v in r.items() if k not in ("rms", "max")}
    worst = max(gs, key=lambda k: gs[k] / G[k]) if gs else None
    tail = f" worst-group {worst}[{kernel['groups'][worst]['at']}] {gs[worst]:.3f}" if worst else " worst-group -"
    allg = " ".join(f"{k}={v:.3f}" for k, v in gs.items())
    return (f"HIGHPREC {label} [{variant}] max {kernel['max']:.3e} rms {kernel['rms']:.3e} | yardstick max {yardstick['max']:.3e} rms "
            f"{yardstick['rms']:.3e} | ratio rms {r['rms']:.3f} max {r['max']:.3f} |{tail} | {allg}")


# ---- seeded inputs shared by the CPU self-test and the GPU gate -----------------------------------------------------------------------
def make_case(B, N, seed, mixed=True):
    """Seeded denoiser inputs: latents with mixed validity (shape 0 has a single valid part, shape 1 lacks one, when `mixed`), part
    labels drawn per point among the shape's valid parts — so that every lane, wavefront slot and 256-point tile holds every part and
    the group statistics do not follow the part layout — and x = anchors + sqrt(variance) z."""
    from difffacto_amd import synth
    from oracle import diffusion as odf
    part_code, mean, logvar, valid = synth.make_latents(B, seed=seed)
    if mixed:
        valid[0] = [0, 0, 1, 0]
        if B > 1:
            valid[1] = [1, 0, 1, 1]
    var = np.exp(logvar).astype(np.float32)
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 4, size=(B, N)).astype(np.int32)
    seg = np.where(valid[np.arange(B)[:, None], seg] > 0, seg, np.argmax(valid, axis=1)[:, None]).astype(np.int32)
    anchors, variance = odf.gather_params(seg, mean, var)
    x = (np.sqrt(variance) * rng.standard_normal((B, 3, N)).astype(np.float32) + anchors).astype(np.float32)
    return dict(B=B, N=N, part_code=part_code, mean=mean, var=var, valid=valid, seg=seg, anchors=anchors, variance=variance, x=x,
                ctx=[part_code, np.concatenate([mean, var], 1)])


def eps_of(module, W, case, t, x=None, **kw):
    """eps (B,3,N) of `module` (oracle.denoiser or oracle.highprec, or a forward function with their signature) on a case; t an int or a per-shape (B,) array."""
    t = np.full((case["B"],), t, dtype=np.int64) if np.ndim(t) == 0 else np.asarray(t, dtype=np.int64)
    fwd = module if callable(module) else module.transformer_net_forward
    return fwd(W, case["x"] if x is None else x, t, case["ctx"], case["anchors"].transpose(0, 2, 1),
                                          case["variance"].transpose(0, 2, 1), case["valid"], case["seg"], **kw)
