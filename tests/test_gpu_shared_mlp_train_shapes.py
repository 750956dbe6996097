"""dfx_shared_mlp_train_* across the row-count / width dispatch of the fp32 MFMA product kernels (mfma_linear.h: k_lin, split-K k_lin<,4>,
k_lin_wide, k_lin_wide_lds NT = 4 / NT = 2), and the gates in front of it (the K % 8 width rule, PointNetV2's zdim, the PointNet2 head).

Every case of tests/_smt_case.py runs ``shared_mlp_train(stack, x, pool)`` forward and backward on the GPU and is compared with the same
``build_shared_mlp`` stack in float64 on the CPU: output, d_x, every parameter gradient, the running statistics.  Gates: those of
test_gpu_sa_modules.py's train-mode tests (2e-4 x max(1, |ref|) on outputs and running statistics, 5e-4 of max-abs on every gradient tensor).
The float32 CPU stack against the same truth is the yardstick: each case prints one ``SMT`` line with its errors and the ratio to it
(recorded in profiles/shared_mlp_train_shapes.txt, not gated).  The kernel set each case is predicted to reach (``_smt_case.predict``: the
conditions of ``lin()`` and ``dfx::lin::launch`` restated) is asserted, so that a change of the dispatch thresholds fails here instead
of silently moving a case back onto k_lin.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _smt_case as sc

pytestmark = pytest.mark.gpu


def _raiser(msg):
    def f(*a, **k):
        raise AssertionError(msg)
    return f


def _no_torch_layers(monkeypatch, layers):
    for layer in layers:
        if not isinstance(layer, (torch.nn.ReLU, torch.nn.Dropout)):
            monkeypatch.setattr(layer, "forward", _raiser("torch layer used where the native path serves"))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_shared_mlp_train_against_float64_across_the_dispatch(name):
    from difffacto_amd.pointnet2_ops import pointnet2_modules as pm
    c = sc.CASES[name]
    assert sc.kernel_set(c["spec"], c["dims"]) == c["kernels"], name           # the case still reaches what it is listed for
    stack = sc.make_stack(c["spec"], c["bn"], c["seed"], c["train"]).cuda()
    assert pm._train_native_ok(stack)
    x, gout = sc.make_inputs(c["spec"], c["dims"], c["pool"], c["seed"])
    x = torch.from_numpy(x).cuda().requires_grad_(True)
    out = pm.shared_mlp_train(stack, x, pool=c["pool"])
    out.backward(torch.from_numpy(gout).cuda())
    torch.cuda.synchronize()
    err, yard = sc.errors(sc.collect(stack, out, x), sc.truth(name)), sc.yardstick(name)
    print(sc.line(name, err, yard))
    for k, gate in sc.GATES.items():
        assert err[k] <= gate, (name, k, err[k], err["at"].get(k))
    for k, b in stack.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == (1 if c["train"] else 0), k


# ---- widths the kernels do not serve: modules stay on their torch layers, a direct call is an error that touches nothing ----
def _mlp_truth(seq, x_gpu, pool):
    """The module's stack in float64 on the CPU on the tensor the GPU module fed its MLP: (out, d_out, d_in, parameter gradients)."""
    ref = copy.deepcopy(seq).cpu().double()
    xin = x_gpu.detach().cpu().double().requires_grad_(True)
    y = ref(xin)
    out = y.amax(dim=3) if pool else y
    gout = torch.from_numpy(np.random.Generator(np.random.PCG64(77)).standard_normal(tuple(out.shape)))
    out.backward(gout)
    return out.detach(), gout, xin.grad, {k: p.grad for k, p in ref.named_parameters()}


def _close(got, ref, tol, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert float((got - ref).abs().max()) <= tol, (what, float((got - ref).abs().max()), tol)


def _check_module(seq, out, gout, truth, leaves, mlp_in):
    t_out, _, t_din, t_grads = truth
    _close(out, t_out, sc.OUT_TOL * max(1.0, float(t_out.abs().max())), "out")
    out.backward(gout.to(out))
    for k, p in seq.named_parameters():
        _close(p.grad, t_grads[k], sc.GRAD_TOL * float(t_grads[k].abs().max()), k)
    # the gradients of the module's inputs: the truth's d (MLP input) pulled back through the same grouping / interpolation kernels
    want = torch.autograd.grad(mlp_in, leaves, t_din.to(mlp_in), allow_unused=True)
    for leaf, w in zip(leaves, want):
        _close(leaf.grad, w, sc.GRAD_TOL * float(w.abs().max()), "input gradient")


def test_sa_module_with_a_width_off_the_rule_runs_its_torch_layers(monkeypatch):
    from difffacto_amd.pointnet2_ops import pointnet2_modules as pm
    mod = pm.PointnetSAModule(npoint=16, radius=0.5, nsample=8, mlp=[3, 12, 20])
    sc.randomize(mod, 41).cuda().train()
    assert not pm._train_native_ok(mod.mlps[0])
    monkeypatch.setattr(pm, "shared_mlp_train", _raiser("native training op called with widths [6, 12, 20]"))
    rng = np.random.Generator(np.random.PCG64(42))
    xyz = torch.from_numpy(rng.uniform(-1, 1, size=(2, 64, 3)).astype(np.float32)).cuda()
    feats = torch.from_numpy(rng.standard_normal((2, 3, 64)).astype(np.float32)).cuda().requires_grad_(True)
    before = copy.deepcopy(mod.mlps[0])
    new_xyz, out = mod(xyz, feats)
    assert tuple(out.shape) == (2, 20, 16)
    grouped = mod.groupers[0](xyz, new_xyz, feats)
    truth = _mlp_truth(before, grouped, pool=True)
    _check_module(mod.mlps[0], out, truth[1], truth, [feats], grouped)


def test_fp_module_with_a_width_off_the_rule_runs_its_torch_layers(monkeypatch):
    from difffacto_amd.pointnet2_ops import pointnet2_modules as pm
    from difffacto_amd.pointnet2_ops import pointnet2_utils as pu
    mod = pm.PointnetFPModule(mlp=[10, 12])
    sc.randomize(mod, 43).cuda().train()
    assert not pm._train_native_ok(mod.mlp)
    monkeypatch.setattr(pm, "shared_mlp_train", _raiser("native training op called with widths [10, 12]"))
    rng = np.random.Generator(np.random.PCG64(44))
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    unknown, known = f32(rng.uniform(-1, 1, size=(2, 37, 3))), f32(rng.uniform(-1, 1, size=(2, 11, 3)))
    uf, kf = f32(rng.standard_normal((2, 4, 37))).requires_grad_(True), f32(rng.standard_normal((2, 6, 11))).requires_grad_(True)
    before = copy.deepcopy(mod.mlp)
    out = mod(unknown, known, uf, kf)
    assert tuple(out.shape) == (2, 12, 37)
    dist, idx = pu.three_nn(unknown, known)
    inv = 1.0 / (dist + 1e-8)
    stacked = torch.cat([pu.three_interpolate(kf, idx, inv / inv.sum(dim=2, keepdim=True)), uf], dim=1).unsqueeze(-1)
    truth = _mlp_truth(before, stacked, pool=False)
    _check_module(mod.mlp, out.unsqueeze(-1), truth[1], truth, [uf, kf], stacked)


def _smt_desc(stack):
    """dfx_shared_mlp_train over a BatchNorm build_shared_mlp stack on the GPU, as _SharedMLPTrainFn fills it."""
    from difffacto_amd import _ffi
    convs = [m for m in stack if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in stack if isinstance(m, torch.nn.BatchNorm2d)]
    d = _ffi.SharedMlpTrain()
    d.layers, d.relu_mask, d.bn_eps = len(convs), (1 << len(convs)) - 1, float(bns[0].eps)
    d.ch[0] = convs[0].in_channels
    keep = []
    for l, (conv, bn) in enumerate(zip(convs, bns)):
        w = conv.weight.detach().reshape(conv.out_channels, conv.in_channels).contiguous()
        keep.append(w)
        d.ch[l + 1] = conv.out_channels
        d.conv_w[l], d.bn_w[l], d.bn_b[l] = w.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr()
        d.bn_mean[l], d.bn_var[l] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
    return d, keep


def test_direct_call_with_a_width_off_the_rule_is_an_invalid_argument_and_writes_nothing():
    from difffacto_amd import _ffi
    from difffacto_amd.pointnet2_ops import pointnet2_modules as pm
    stack = sc.make_stack([6, 12, 20], True, 45).cuda()
    x = torch.from_numpy(sc.make_inputs([6, 12, 20], (2, 7, 5), True, 45)[0]).cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"dfx_shared_mlp_train_forward failed \(code -1\).*layer 0: 12 output channels \(multiple of 8"):
        pm.shared_mlp_train(stack, x, pool=True)
    # the C entry point itself: the code, and neither the output nor the running statistics touched
    lib = _ffi.lib()
    desc, keep = _smt_desc(stack)
    B, M, ns = 2, 7, 5
    nbytes = lib.dfx_shared_mlp_train_workspace_bytes(ctypes.byref(desc), B, M, ns)
    assert nbytes > 0
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 20, M), 12345.0, device="cuda")
    stats = [b.clone() for b in stack.buffers()]
    rc = lib.dfx_shared_mlp_train_forward(ctypes.byref(desc), ctypes.c_void_p((ws.data_ptr() + 255) & ~255), nbytes, _ffi.ptr(x.detach()), _ffi.ptr(out), B, M, ns,
                                          1, 1, 0.1, _ffi.current_stream())
    torch.cuda.synchronize()
    assert rc == -1                                                            # DFX_ERR_INVALID_ARG (include/dfx.h)
    assert b"multiple of 8" in lib.dfx_last_error()
    assert bool((out == 12345.0).all()) and not bool(ws.any())
    assert all(torch.equal(a, b) for a, b in zip(stats, stack.buffers()))
    desc.ch[1], desc.ch[2] = 16, 20                                            # the rule holds for every layer, and the message names the layer
    rc = lib.dfx_shared_mlp_train_forward(ctypes.byref(desc), ctypes.c_void_p((ws.data_ptr() + 255) & ~255), nbytes, _ffi.ptr(x.detach()), _ffi.ptr(out), B, M, ns,
                                          1, 1, 0.1, _ffi.current_stream())
    assert rc == -1 and b"layer 1: 20 output channels" in lib.dfx_last_error()
    assert bool((out == 12345.0).all())


# ---- PointNetV2 training: zdim is the K of the last head layer's input-gradient products ----
# (a bias in front of a train-mode BatchNorm has a mathematically zero gradient: rounding noise, compared in absolute terms as in test_gpu_encoder_train.py)
ZERO_GRAD = {f"conv{i}.bias" for i in (1, 2, 3, 4)} | {f"{h}.{i}.bias" for h in ("mlp_m", "mlp_v") for i in (0, 3)}


def test_pointnet_v2_train_rejects_zdim_off_the_rule():
    from difffacto_amd import _ffi, synth, training
    from difffacto_amd.encoders import PointNetV2
    enc = PointNetV2(zdim=12, num_anchors=4, per_part_mlp=True).cuda().train()
    x = torch.rand(2, 33, 3, device="cuda") * 2 - 1
    attn = torch.eye(4, device="cuda")[torch.randint(0, 4, (2, 33), device="cuda")]
    with pytest.raises(NotImplementedError, match=r"zdim % 8 == 0; got B=2, num_anchors=4, zdim=12"):
        enc(x, attn)
    W = synth.make_pointnet_v2_weights(3, zdim=12)
    t = {n: torch.from_numpy(W[n]).cuda() for n in training.PNV2_PARAMS + training.PNV2_BUFFERS}
    lib = _ffi.lib()
    B, N = 2, 33
    nbytes = lib.dfx_pointnet_v2_train_workspace_bytes(B, N, 4, 12)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    m, v = torch.full((B, 4, 12), 12345.0, device="cuda"), torch.full((B, 4, 12), 12345.0, device="cuda")
    w = training._pnv2_struct(t, 4, 12, True, 1e-5)
    rc = lib.dfx_pointnet_v2_train_forward(ctypes.byref(w), ctypes.c_void_p((ws.data_ptr() + 255) & ~255), nbytes, _ffi.ptr(x), _ffi.ptr(attn), _ffi.ptr(m), _ffi.ptr(v),
                                           0.1, B, N, training.PRECISIONS["f32"], _ffi.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"zdim % 8 == 0" in lib.dfx_last_error()
    assert bool((m == 12345.0).all()) and bool((v == 12345.0).all())
    assert all(torch.equal(t[n].cpu(), torch.from_numpy(W[n])) for n in training.PNV2_BUFFERS)


# The gradients no two-row BatchNorm stands behind or in front of: d mlp_*.6.bias = sum_b d out, and d mlp_*.4.bias = sum_b mask dX — the two-row sums of the
# K = zdim product dX = d out W6 itself (a wrong product moves them by its own size; nothing amplifies their rounding).
PN_DIRECT = {f"{h}.{i}.bias" for h in ("mlp_m", "mlp_v") for i in (4, 6)}
PN_AMPLIFIED = 1e-2     # pnv2_judge


def pnv2_zdim8_case():
    """tests/_encstats.py's (2, 33) case with zdim = 8 heads (the trunk and the heads' first two layers are the same draws as at zdim = 256)."""
    import _encstats as es
    from difffacto_amd import synth
    case = es.pn_case(2, 33)
    rng = np.random.Generator(np.random.PCG64(2033 + 8))
    case["W"] = synth.make_pointnet_v2_weights(2, zdim=8)
    case["dm"], case["dv"] = rng.standard_normal((2, 4, 8)).astype(np.float32), rng.standard_normal((2, 4, 8)).astype(np.float32)
    return case


def pnv2_judge(got, truth, o32):
    """Figures and failures of one implementation's result against the float64 truth on its own branch; o32: the fp32 oracle's result (figures only).
    The heads normalise over TWO rows here.  A channel whose batch variance is near eps multiplies the rounding of z[0] - z[1] by up to 1 / sqrt(eps) = 316,
    forward (xhat) and backward (rstd) alike (tests/_encstats.py, "What was found"); that rounding is at most K u |z| = 512 x 2^-24 x O(1) = 3e-5 for the
    heads' K = 512 products, so two correct fp32 evaluations may stand 316 x 3e-5 = PN_AMPLIFIED = 1e-2 apart, and the fixed gates of
    tests/test_gpu_encoder_train.py (set at B >= 4) do not hold at B = 2 for the fp32 torch oracle itself (CPU: outputs 6.9e-5, gradients 1.6e-3).
    Gates: outputs and running statistics PN_AMPLIFIED x max(1, |ref|), gradients PN_AMPLIFIED of max-abs; PN_DIRECT gradients, which nothing amplifies,
    test_gpu_encoder_train.py's 1e-3 of max-abs.  The mathematically zero gradients (a bias in front of a batch-statistics BatchNorm) are what is left when
    sum_b dz_b cancels; dz reaches 1e3 here (rstd of a two-row channel), so that file's absolute 5e-3, set where d weight is O(10), becomes its 1e-3 on the scale
    of the same layer's d weight — the same product with the inputs replaced by ones.  A product that mishandles K = 8 is off by O(1) in all of them."""
    fails, lines = [], []
    for k in ("m", "v"):
        e = float(np.abs(got[k] - truth[k]).max())
        lines.append(f"{k} {e:.2e}")
        if not e <= PN_AMPLIFIED * max(1.0, float(np.abs(truth[k]).max())):
            fails.append((k, e))
    er = {k: float(np.abs(got["running"][k] - a).max()) / max(1.0, float(np.abs(a).max())) for k, a in truth["running"].items()}
    lines.append(f"running {max(er.values()):.2e}")
    fails += [(k, e) for k, e in er.items() if not e <= PN_AMPLIFIED]
    worst, zero = {"direct": (0.0, 0.0, ""), "amplified": (0.0, 0.0, "")}, 0.0
    for k, g in truth["grads"].items():
        a = got["grads"][k]
        assert a.shape == g.shape and np.isfinite(a).all(), k
        if k in ZERO_GRAD:      # sum_b dz_b = the layer's d weight with its inputs replaced by ones: terms of d weight's size that cancel to 0
            zscale = float(np.abs(truth["grads"][k[:-4] + "weight"]).max())
            zero = max(zero, float(np.abs(a).max()) / zscale)
            if not float(np.abs(a).max()) <= 1e-3 * zscale:
                fails.append((k, float(np.abs(a).max()), zscale))
            continue
        scale = max(float(np.abs(g).max()), 1e-30)
        e, y = float(np.abs(a - g).max()) / scale, float(np.abs(o32["grads"][k] - g).max()) / scale
        kind = "direct" if k in PN_DIRECT else "amplified"
        if not e <= (1e-3 if kind == "direct" else PN_AMPLIFIED):
            fails.append((k, e))
        if e >= worst[kind][0]:
            worst[kind] = (e, y, k)
    lines += [f"{kind} gradients {e:.2e} of max-abs (fp32 oracle {y:.2e}; {k})" for kind, (e, y, k) in worst.items()]
    lines.append(f"zero gradients {zero:.2e} of their layer's d weight")
    return fails, "PNV2 zdim = 8, (B, N) = (2, 33): " + ", ".join(lines)


def test_pointnet_v2_train_at_zdim_8_vs_oracle():
    """The smallest zdim the rule leaves (K = 8 of the heads' last input-gradient products: k_lin's tail only) against the existing oracle
    (oracle/pointnet_v2_train.py): float64 on the branch the kernels took (exported by the library, checked for legitimacy as in
    test_gpu_encoder_train_highprec.py), the fp32 oracle's own error printed beside the kernels'.  Gates: pnv2_judge."""
    import _encstats as es
    from difffacto_amd import training
    from oracle import pointnet_v2_train as pt
    case = pnv2_zdim8_case()
    args = (case["W"], case["x"], case["attn"], case["dm"], case["dv"])
    r64 = pt.outputs_and_grads(*args, dtype=torch.float64, record=True)
    r32 = pt.outputs_and_grads(*args, record=True)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = {n: cu(case["W"][n]).requires_grad_(True) for n in training.PNV2_PARAMS}
    Bf = {n: cu(case["W"][n]) for n in training.PNV2_BUFFERS}
    m, v = training.pointnet_v2_train_forward(P, Bf, cu(case["x"]), cu(case["attn"]), zdim=8)
    exp = {k: t.cpu().numpy() for k, t in training.pointnet_v2_branch(m).items()}
    ((m * cu(case["dm"])).sum() + (v * cu(case["dv"])).sum()).backward()
    torch.cuda.synchronize()
    got = dict(m=m.detach().cpu().numpy(), v=v.detach().cpu().numpy(), running={n: b.cpu().numpy() for n, b in Bf.items()},
               grads={n: p.grad.cpu().numpy() for n, p in P.items()})
    branch, b64 = es.pn_branch_of_export(exp, case["attn"]), es.pn_branch_of_record(r64["record"])
    site_err = {s: float(np.abs(r32["record"]["pre"][s] - r64["record"]["pre"][s]).max()) for s in es.PN_SITES}
    site_err["pool"] = float(np.abs(r32["record"]["pool_in"] - r64["record"]["pool_in"]).max())
    margin = dict({s: r64["record"]["pre"][s] for s in es.PN_SITES}, pool=r64["record"]["gap"])
    flips, counts = es.legitimacy(dict(b64=b64, margin=margin, site_err=site_err, valid_rows=None), branch, "kernel")
    truth = r64 if es.same_branch(branch, b64) else pt.outputs_and_grads(*args, dtype=torch.float64, branch=branch)
    fails, line = pnv2_judge(got, truth, r32)
    print(line + f"; units off the float64 branch {counts}")
    assert not flips, flips
    assert not fails, fails


# ---- the Linear / BatchNorm1d head of PointNet2SSG / PointNet2MSG ----
def _encoder(zdim, num_anchors, seed=51):
    from difffacto_amd.encoders import PointNet2SSG
    enc = PointNet2SSG(zdim=zdim, num_anchors=num_anchors)
    sc.randomize(enc.fc_layer, seed)
    return enc.cuda()


def _feat(B=4):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(52)).standard_normal((B, 1024)).astype(np.float32)).cuda()


@pytest.mark.parametrize("zdim,num_anchors", [(10, 2), (512, 4)])
def test_head_outside_the_kernels_reach_is_the_fc_layer(zdim, num_anchors, monkeypatch):
    """zdim * num_anchors = 20 (off the width rule) and 2048 (> 1024): constructor arguments the reference accepts -> the module's own layers."""
    from difffacto_amd.pointnet2_ops import pointnet2_modules as pm
    monkeypatch.setattr(pm, "mlp_train", _raiser("native training op called for a head it does not serve"))
    enc, feat = _encoder(zdim, num_anchors), _feat()
    twin = copy.deepcopy(enc)
    for mode in (False, True):                      # eval() under autograd, then train() (Dropout on torch's generator: the same seed, the same mask)
        enc.train(mode), twin.train(mode)
        torch.manual_seed(5)
        got = enc._head(feat)
        torch.manual_seed(5)
        want = twin.fc_layer(feat)
        assert tuple(got.shape) == (4, zdim * num_anchors) and torch.equal(got, want)
        for (k, a), (_, b) in zip(enc.fc_layer.named_buffers(), twin.fc_layer.named_buffers()):
            assert torch.equal(a, b), k


def test_head_at_the_shipped_width_stays_native(monkeypatch):
    enc, feat = _encoder(256, 4), _feat()
    ref = copy.deepcopy(enc.fc_layer).cpu().double().eval()
    _no_torch_layers(monkeypatch, enc.fc_layer)
    enc.eval()
    got = enc._head(feat)                           # eval() under autograd: the training kernels on the running statistics
    want = ref(feat.cpu().double())
    assert tuple(got.shape) == (4, 1024)
    _close(got, want, sc.OUT_TOL * max(1.0, float(want.detach().abs().max())), "head")
    enc.train()
    assert tuple(enc._head(feat).shape) == (4, 1024) and all(int(b) == 1 for k, b in enc.fc_layer.named_buffers() if k.endswith("num_batches_tracked"))


def test_head_with_one_row_in_train_mode_raises_like_batchnorm1d():
    enc = _encoder(256, 4).train()
    before = {k: b.clone() for k, b in enc.fc_layer.named_buffers()}
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        enc._head(_feat(1))
    for k, b in enc.fc_layer.named_buffers():
        if "running" in k:          # (nn.BatchNorm1d counts the batch in num_batches_tracked before it refuses it: so does the head)
            assert torch.equal(b, before[k]), k
    assert tuple(enc.eval()._head(_feat(1)).shape) == (1, 1024)      # eval(): one row is fine, as in torch
