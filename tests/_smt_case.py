"""Cases, float64 truth and kernel prediction for the PointNet++ training shared MLP (dfx_shared_mlp_train_*), shared by
tests/test_shared_mlp_train_cpu.py and tests/test_gpu_shared_mlp_train_shapes.py.

Truth: the project's own ``build_shared_mlp`` stack on the CPU in float64 (weights from the ``_randomize`` recipe of
test_gpu_sa_modules.py, inputs standard normal from PCG64, backward through autograd, ``amax(dim=3)`` when pooled).
Yardstick: the same stack in float32 on the CPU against that truth.  Gates (those of test_gpu_sa_modules.py's train-mode tests):
outputs and running statistics within OUT_TOL x max(1, |ref|), every gradient tensor within GRAD_TOL of its max-abs.

Which kernel a product takes is restated here from ``lin()`` (train_kernels.hip) and ``dfx::lin::launch`` (mfma_linear.h):

  lin(M, N, K):        M <= 4096 -> k_lin (one wavefront per 32 x 32 tile); else launch()
  launch(M, N, K):     wide   = N % 128 == 0 and M >= 512 and (N / 128) ceil(M / 128) >= 256 and ldy % 4 == 0 (ldy = N here)
                       wide and K % 8 == 0 and K <= 544 and M >= 8192 and ldx % 4 == 0 (ldx = K here)
                           -> k_lin_wide_lds, NT = 2 (64-channel blocks) when K > 272 else NT = 4; grid rows =
                              min(ceil(M / 256), max(1, 256 per_cu / cols)), per_cu = clamp((160 KiB - 1 KiB) / lds bytes, 1, 2)
                       wide otherwise -> k_lin_wide
                       else k_lin, split-K (k_lin<, 4>) when K >= 128 and ceil(N / 32) ceil(M / 32) <= 256
  forward product of layer l:   (M, N, K) = (R, ch[l + 1], ch[l]; layer 0: ch[0] rounded up to a multiple of 8)
  backward dX of layer l:       (R, c_in (padded for layer 0), c_out)
"""
import functools

import numpy as np
import torch

OUT_TOL, GRAD_TOL = 2e-4, 5e-4      # test_gpu_sa_modules.py: _check_train
HEADROOM = 10.0                      # the float32 yardstick must sit this far inside the gates on every case

K_LIN, K_SPLIT, K_WIDE, K_LDS4, K_LDS2 = "k_lin", "k_lin<,4>", "k_lin_wide", "k_lin_wide_lds<4>", "k_lin_wide_lds<2>"
ALL_KERNELS = frozenset((K_LIN, K_SPLIT, K_WIDE, K_LDS4, K_LDS2))


def _case(spec, dims, pool=True, bn=True, train=True, seed=0, kernels=(), note=""):
    return dict(spec=list(spec), dims=tuple(dims), pool=pool, bn=bn, train=train, seed=seed, kernels=frozenset(kernels), note=note)


# name -> case.  `kernels`: the exact set of fp32 product kernels the forward and the backward reach (asserted against predict()).
CASES = {
    "A": _case([3, 8, 24, 40, 104], (2, 7, 5), seed=11, kernels=[K_LIN],
               note="R = 70: k_lin at K = 8 / 24 (tail only), 40 (trip + tail), 104 (three trips + tail); ragged rows and N tiles"),
    "A_eval": _case([3, 8, 24, 40, 104], (2, 7, 5), train=False, seed=11, kernels=[K_LIN], note="case A in eval() under autograd: running statistics (k_bn_apply)"),
    "A2": _case([16, 64, 96, 72], (2, 7, 5), bn=False, seed=12, kernels=[K_LIN],
                note="K = 64 (prefetch pair loop), 96 (pair + leftover), 72 (pair + tail); conv bias + k_smt_relu"),
    "B": _case([6, 64, 96], (1, 41, 100), seed=13, kernels=[K_LIN], note="R = 4100 > 4096: launch() -> unsplit k_lin, 387 / 258 tiles"),
    "C": _case([3, 160, 32, 136, 16], (1, 4100, 1), pool=False, seed=14, kernels=[K_LIN, K_SPLIT],
               note="split-K: forward N = 32 / K = 160, N = 16 / K = 136; backward N = 32 / K = 136, N = 8 / K = 160"),
    "D1": _case([8, 512, 40, 512], (1, 3, 2741), seed=15, kernels=[K_LIN, K_LDS4], note="R = 8223 (last tile 31 rows); NT = 4 at U = 1 and U = 5"),
    "D2": _case([48, 512, 280, 512], (1, 3, 2741), seed=16, kernels=[K_LIN, K_LDS4, K_LDS2], note="NT = 4 at U = 6; NT = 2 at K = 280 (U = 35, tail 3)"),
    "D3": _case([8, 272, 1024], (1, 3, 2741), seed=17, kernels=[K_LIN, K_LDS4], note="NT = 4 at its LDS limit K = 272: 32 row blocks for 33 tiles (striding loop)"),
    "D4": _case([8, 544, 512], (1, 3, 2741), seed=18, kernels=[K_LIN, K_LDS2], note="NT = 2 at its limit K = 544"),
    "E1": _case([24, 1024, 128], (1, 4100, 1), pool=False, seed=19, kernels=[K_LIN, K_SPLIT, K_WIDE],
                note="k_lin_wide at 4096 < R < 8192: K = 24 (odd U) forward, K = 128 (even U) backward; the K = 1024 dX of layer 0 (N = 24) is split-K"),
    "E2": _case([8, 552, 512], (1, 3, 2741), seed=20, kernels=[K_LIN, K_WIDE], note="k_lin_wide through K > 544 at R >= 8192, U = 69"),
    "G1": _case([3, 8], (1, 65600, 1), seed=21, kernels=[K_LIN], note="65 600 pooled groups (> 65 535)"),
    "G2": _case([3, 8], (2, 32800, 2), seed=22, kernels=[K_LIN], note="65 600 pooled groups with B = 2: g / M, g % M"),
}


# ---- which kernel runs: lin() of train_kernels.hip and dfx::lin::launch of mfma_linear.h, restated (module docstring) ----
def lin_kernel(M, N, K):
    """(kernel name, details) of the fp32 product Y (M, N) = X (M, K) W^T as dfx_shared_mlp_train_* issues it (ldx = K, ldy = N, one group)."""
    assert K % 8 == 0, K
    cdiv = lambda a, b: -(-a // b)
    if M <= 4096:
        return K_LIN, dict(tiles=cdiv(N, 32) * cdiv(M, 32), trips=K // 32, tail=K % 32 // 8)
    if N % 128 == 0 and M >= 512 and (N // 128) * cdiv(M, 128) >= 256 and N % 4 == 0:
        if K <= 544 and M >= 8192 and K % 4 == 0:
            narrow = K > 272
            lds = K // 8 * (2048 if narrow else 4096)
            cols = N // (64 if narrow else 128)
            per_cu = max(1, min(2, (160 * 1024 - 1024) // lds))
            rows = min(cdiv(M, 256), max(1, 256 * per_cu // cols))
            return (K_LDS2 if narrow else K_LDS4), dict(U=K // 8, rows=rows, row_tiles=cdiv(M, 256), last_rows=M % 32)
        return K_WIDE, dict(U=K // 8)
    tiles = cdiv(N, 32) * cdiv(M, 32)
    if K >= 128 and tiles <= 256:
        return K_SPLIT, dict(tiles=tiles, trips=K // 32, tail=K % 32 // 8)
    return K_LIN, dict(tiles=tiles, trips=K // 32, tail=K % 32 // 8)


def products(spec, dims):
    """[(direction, layer, M, N, K)] of the products of one forward + backward (d_x requested)."""
    B, M, ns = dims
    R = B * M * ns
    cp0 = (spec[0] + 7) // 8 * 8
    out = []
    for l in range(len(spec) - 1):
        out.append(("fwd", l, R, spec[l + 1], cp0 if l == 0 else spec[l]))
    for l in reversed(range(len(spec) - 1)):
        out.append(("bwd", l, R, cp0 if l == 0 else spec[l], spec[l + 1]))
    return out


def predict(spec, dims):
    """[(direction, layer, (M, N, K), kernel, details)]."""
    return [(d, l, (M, N, K)) + lin_kernel(M, N, K) for d, l, M, N, K in products(spec, dims)]


def kernel_set(spec, dims):
    return frozenset(p[3] for p in predict(spec, dims))


# ---- the stack, its weights and inputs ----
def randomize(mod, seed):
    """The `_randomize` recipe of test_gpu_sa_modules.py (weights U(+-1) / sqrt(fan_in); biases, BN shifts, running means U(+-0.2); BN scales U(.8, 1.2);
    running variances U(.5, 1.5)), on the CPU, mode untouched."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = mod.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            a = rng.uniform(0.5, 1.5, size=tuple(v.shape))
        elif k.endswith("running_mean") or k.endswith("bias"):
            a = rng.uniform(-0.2, 0.2, size=tuple(v.shape))
        elif v.dim() == 1:
            a = rng.uniform(0.8, 1.2, size=tuple(v.shape))
        else:
            a = rng.uniform(-1, 1, size=tuple(v.shape)) / np.sqrt(v.shape[1])
        sd[k] = torch.from_numpy(a.astype(np.float32))
    mod.load_state_dict(sd)
    return mod


def make_stack(spec, bn, seed, train=True):
    """float32 ``build_shared_mlp(spec, bn)`` on the CPU with the case's weights."""
    from difffacto_amd.pointnet2_ops.pointnet2_modules import build_shared_mlp
    return randomize(build_shared_mlp(list(spec), bn=bn), seed).train(train)


def make_inputs(spec, dims, pool, seed):
    """x (B, ch[0], M, ns) and the output gradient, standard normal float32 from PCG64."""
    B, M, ns = dims
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    x = rng.standard_normal((B, spec[0], M, ns)).astype(np.float32)
    gout = rng.standard_normal((B, spec[-1], M) if pool else (B, spec[-1], M, ns)).astype(np.float32)
    return x, gout


def collect(stack, out, x):
    """numpy dict of one forward + backward: out, d_x, g.<parameter>, r.<running statistic>."""
    res = {"out": out.detach().cpu().numpy(), "d_x": x.grad.detach().cpu().numpy()}
    for k, p in stack.named_parameters():
        res["g." + k] = p.grad.detach().cpu().numpy()
    for k, b in stack.named_buffers():
        if "running" in k:
            res["r." + k] = b.detach().cpu().numpy()
    return res


def run_torch(case, dtype):
    """The stack's own torch layers on the CPU in `dtype` (float64: the truth; float32: the yardstick)."""
    stack = make_stack(case["spec"], case["bn"], case["seed"], case["train"]).to(dtype)
    x, gout = make_inputs(case["spec"], case["dims"], case["pool"], case["seed"])
    x = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = stack(x)
    out = y.amax(dim=3) if case["pool"] else y
    out.backward(torch.from_numpy(gout).to(dtype))
    return collect(stack, out, x)


@functools.lru_cache(maxsize=None)
def truth(name):
    return run_torch(CASES[name], torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """errors() of the float32 CPU stack against the truth."""
    return errors(run_torch(CASES[name], torch.float32), truth(name))


def errors(got, ref):
    """{"out", "stat", "grad"}: the worst gated figure of each kind — outputs / running statistics as max |got - ref| / max(1, max |ref|), gradients
    (d_x and every parameter's) as max |got - ref| / max |ref| — and "at", the tensor behind each."""
    worst = {"out": 0.0, "stat": 0.0, "grad": 0.0}
    at = {}
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    for k, r in ref.items():
        g = np.asarray(got[k], np.float64)
        r = np.asarray(r, np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.isfinite(g).all(), k
        d = float(np.abs(g - r).max()) if r.size else 0.0
        if k == "out" or k.startswith("r."):
            kind, e = ("out" if k == "out" else "stat"), d / max(1.0, float(np.abs(r).max()))
        else:
            kind, e = "grad", d / max(float(np.abs(r).max()), 1e-30)
        if e >= worst[kind]:
            worst[kind], at[kind] = e, k
    worst["at"] = at
    return worst


GATES = {"out": OUT_TOL, "stat": OUT_TOL, "grad": GRAD_TOL}


def passes(err):
    """The gates on errors()' figures (a stack without BatchNorm has no running statistics: its "stat" is 0)."""
    return all(err[k] <= GATES[k] for k in GATES)


def ratio(err, yard):
    """The worst of err / yardstick over the three kinds (kinds the yardstick reproduces exactly are skipped)."""
    return max([err[k] / yard[k] for k in GATES if yard[k] > 0.0] or [0.0])


def line(name, err, yard):
    """One line per case for profiles/shared_mlp_train_shapes.txt: spec, R, kernels, error, ratio."""
    c = CASES[name]
    B, M, ns = c["dims"]
    ks = " ".join(sorted(kernel_set(c["spec"], c["dims"])))
    opts = ("pool" if c["pool"] else "rows") + ("" if c["bn"] else " nobn") + ("" if c["train"] else " eval")
    return (f"SMT {name:6s} {str(c['spec']):24s} (B, M, ns) = {str(c['dims']):16s} {opts:10s} R = {B * M * ns:6d}  [{ks}]  "
            f"out {err['out']:.2e} stat {err['stat']:.2e} grad {err['grad']:.2e}  yardstick {yard['out']:.1e} {yard['stat']:.1e} {yard['grad']:.1e}  "
            f"ratio {ratio(err, yard):.2f}")
