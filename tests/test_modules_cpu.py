"""CPU: the drop-in modules keep the reference's constructor arguments and state_dict layout; compared key-for-key with what the
reference built from its shipped configs (recorded in tests/golden/reference_modules.npz), and registry installation checked."""
import os
import sys

import pytest
import torch

from difffacto_amd import synth
from difffacto_amd.modules import TransformerNet, AnchoredDiffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NET_CFG = dict(type='TransformerNet', in_channels=3, out_channels=3, n_heads=8, d_head=16, depth=5, dropout=0.2,
               context_dim=256 + 6, n_class=4, class_cond=True, use_linear=True, cat_params_to_x=True,
               use_checkpoint=False, single_attn=True, cat_class_to_x=True)          # configs/gen_chair.py:54-70
DIFF_CFG = dict(net=NET_CFG, beta_1=1e-4, beta_T=.02, k=1.0, res=False, mode='linear', use_beta=False,
                rescale_timesteps=False, model_mean_type="epsilon", learn_variance=True, loss_type='mse',
                include_anchors=False, classifier_weight=1., guidance=False, ddim_sampling=False, ddim_nsteps=25,
                ddim_discretize='quad', ddim_eta=1.)                                  # configs/gen_chair.py:52-86


def test_state_dict_matches_synth_layout():
    d = AnchoredDiffusion(num_timesteps=100, **DIFF_CFG)
    sd = d.model.state_dict()
    shapes = dict(synth.denoiser_param_shapes(5))
    assert set(sd) == set(shapes)
    for k, v in sd.items():
        assert tuple(v.shape) == shapes[k], k
    W = synth.make_denoiser_weights(0)
    d.model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    assert list(d.state_dict())[0].startswith("model.")


def test_unsupported_options_fail_loudly():
    bad = dict(NET_CFG)
    bad.pop("type")
    bad["single_attn"] = False
    with pytest.raises(NotImplementedError):
        TransformerNet(**bad)
    with pytest.raises(NotImplementedError):
        AnchoredDiffusion(num_timesteps=10, **{**DIFF_CFG, "model_mean_type": "start_x"})
    d = AnchoredDiffusion(num_timesteps=1000, **{**DIFF_CFG, "ddim_sampling": True, "ddim_nsteps": 25, "ddim_discretize": "quad"})
    assert d.steps[:4] == [0, 1, 5, 12] and len(d.steps) == 25 and d.steps[-1] == 800   # anchored_diffusion.py:120-122


def test_cpu_forward_is_rejected():
    args = dict(NET_CFG)
    args.pop("type")
    net = TransformerNet(**args)
    with pytest.raises(RuntimeError, match="CPU not supported|HIP device"):
        net(torch.zeros(1, 3, 32), torch.zeros(1, dtype=torch.long), [torch.zeros(1, 256, 4), torch.ones(1, 6, 4)],
            valid_id=torch.ones(1, 4), anchor_assignment=torch.zeros(1, 32, dtype=torch.int32))


def _reference_facts():
    """tests/golden/reference_modules.npz (tests/golden/make_golden_modules.py): what the reference's own config loader and registry
    built from the shipped configs — cfg.model, state_dict layouts, parameter counts, the attributes encoders.attach() reads and the
    keyword arguments its decode passes to p_sample_loop_progressive."""
    import json
    import numpy as np
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_modules.npz")) as z:
        return json.loads(z["json"].tobytes())


def _checkpoint(layout, seed=0):
    """A checkpoint with the recorded layout (keys in order, shapes, dtypes) and seeded values."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape, dtype in layout:
        dt = getattr(torch, dtype)
        out[k] = torch.randn(shape, generator=g).to(dt) if dt.is_floating_point else torch.randint(0, 100, shape, generator=g).to(dt)
    return out


@pytest.fixture
def reference_registry():
    """The reference's registry protocol (utils/registry.py:1-46: Registry._modules / get; build_from_cfg copies the dict, pops 'type'
    and calls the registered class with the rest) as the module `difffacto.utils.registry`, its entries standing for the reference's
    classes, so that difffacto_amd.install() has a registry to register into.  sys.modules is restored afterwards."""
    import types

    class Registry:
        def __init__(self, names):
            self._modules = {n: type(n, (), {"__module__": "difffacto.models"}) for n in names}

        def get(self, name):
            assert name in self._modules, f"{name} is not registered."
            return self._modules[name]

    def build_from_cfg(cfg, registry, **kwargs):
        args = dict(cfg, **kwargs)
        return registry.get(args.pop("type"))(**args)

    reg = types.ModuleType("difffacto.utils.registry")
    reg.build_from_cfg = build_from_cfg
    reg.NETS, reg.DIFFUSIONS, reg.MODELS = Registry(["TransformerNet"]), Registry(["AnchoredDiffusion"]), Registry(["AnchorDiffAE"])
    reg.ENCODERS = Registry(["PartEncoderForTransformerDecoder", "PointNetV2", "PartAlignerTransformer", "PointNet2SSG", "PointNet2MSG"])
    reg.SAMPLERS = Registry(["Uniform"])
    pkg, utils = types.ModuleType("difffacto"), types.ModuleType("difffacto.utils")
    pkg.utils, utils.registry = utils, reg
    names = ("difffacto", "difffacto.utils", "difffacto.utils.registry", "pointnet2_ops", "pointnet2_ops.pointnet2_utils",
             "pointnet2_ops.pointnet2_modules")
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules.update({"difffacto": pkg, "difffacto.utils": utils, "difffacto.utils.registry": reg})
    try:
        yield reg
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_keys_and_registry_against_reference(reference_registry):
    facts = _reference_facts()
    ref_sd = {k: tuple(shape) for k, shape, _ in facts["gen_chair_T10_diffusion_state_dict"]}
    mine = AnchoredDiffusion(num_timesteps=10, **DIFF_CFG).state_dict()
    assert set(ref_sd) == set(mine)
    for k in ref_sd:
        assert ref_sd[k] == tuple(mine[k].shape), k
    # registry installation: the reference's build_from_cfg now yields the libdfx-backed classes
    import difffacto_amd
    from difffacto.utils.registry import DIFFUSIONS, build_from_cfg
    assert difffacto_amd.install() is True
    built = build_from_cfg(dict(facts["configs"]["gen_chair.py"]["model_cfg"]["diffusion"], num_timesteps=10), DIFFUSIONS)
    assert isinstance(built, AnchoredDiffusion) and isinstance(built.model, TransformerNet)
    import pointnet2_ops
    assert pointnet2_ops.pointnet2_utils.gather_operation.__self__.__module__.startswith("difffacto_amd")


ENC_CFG = dict(
    encoder=dict(type='PointNetV2', zdim=256, point_dim=3, per_part_mlp=True),
    part_aligner=dict(type="PartAlignerTransformer", in_channels=256, out_channels=6, n_class=4, d_head=32, depth=5,
                      n_heads=8, dropout=0., use_checkpoint=False, use_linear=True, class_cond=True, single_attn=True,
                      add_class_cond=True, cimle=True, noise_scale=100, cond_noise_type=0),
    n_class=4, kl_weight=0, fit_loss_type=4, fit_loss_weight=1.0, use_flow=True, latent_flow_depth=14,
    latent_flow_hidden_dim=256, include_z=False, include_part_code=True, include_params=True, use_gt_params=False,
    kl_weight_annealing=False, gen=True, prior_var=1.0)   # configs/gen_chair.py:6-47


TOP_CFG = dict(sampler=dict(type='Uniform'), num_anchors=4, num_timesteps=100, npoints=2048, gen=True, cimle=True, cimle_sample_num=1, ret_traj=True,
               ret_interval=10, forward_sample=False, drift_anchors=False, interpolate=False, save_weights=False)   # configs/gen_chair.py:88-104


def model_cfg(**overrides):
    """`cfg.model` of the unmodified configs/gen_chair.py without its 'type' key (test_install_full_... checks that against the reference's own
    config loader), with the knobs the golden fixtures were generated under (num_timesteps, npoints, cimle_sample_num, ret_interval, ...) replaced:
    what the -m gpu composition tests construct networks.AnchorDiffAE from."""
    net = overrides.pop("net", {})
    diffusion = dict(type="AnchoredDiffusion", **{**DIFF_CFG, "net": dict(DIFF_CFG["net"], **net)})
    return {**TOP_CFG, "encoder": dict(type="PartEncoderForTransformerDecoder", **ENC_CFG), "diffusion": diffusion, **overrides}


def _plain(c):
    return {k: _plain(v) for k, v in c.items()} if hasattr(c, "items") else c


def test_encoder_mirror_state_dict_keys_and_unsupported_options():
    from difffacto_amd.encoders import PartEncoderForTransformerDecoder, PartAlignerTransformer
    enc = PartEncoderForTransformerDecoder(**ENC_CFG)
    W = synth.make_latent_weights(0)
    W.update({"encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
    sd = {k: v for k, v in enc.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert set(sd) == set(W)
    for k, v in sd.items():
        assert tuple(v.shape) == W[k].shape, k
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    with pytest.raises(NotImplementedError):
        PartAlignerTransformer(256, 8, 32, 6, depth=5, use_linear=True, single_attn=True, add_class_cond=True, cimle=True,
                               cond_noise_type=2)
    with pytest.raises(NotImplementedError):
        PartEncoderForTransformerDecoder(**{**ENC_CFG, "selective_noise_sampling": True})


def test_encoder_mirror_matches_reference_state_dict():
    import types
    facts = _reference_facts()
    layout = facts["gen_chair_encoder_state_dict"]
    ref = {k: tuple(shape) for k, shape, _ in layout}
    from difffacto_amd.encoders import PartEncoderForTransformerDecoder
    enc = PartEncoderForTransformerDecoder(**ENC_CFG)
    assert ref == {k: tuple(v.shape) for k, v in enc.state_dict().items()}       # incl. encoder.* (PointNetV2): strict loading
    enc.load_state_dict(_checkpoint(layout), strict=True)
    # attach() on an object carrying the recorded attributes of the reference's built encoder (construction only: the first
    # sample_latents call needs the GPU)
    from difffacto_amd.encoders import attach
    a = facts["gen_chair_encoder_attrs"]
    al = a["part_aligner"]
    ns = types.SimpleNamespace
    block = ns(attn2=ns(heads=al["heads"]), single_attn=al["single_attn"])
    part_aligner = ns(transformer_blocks=[block] * al["depth"], proj_out=ns(out_features=al["proj_out_features"]),
                      **{k: v for k, v in al.items() if k not in ("heads", "single_attn", "depth", "proj_out_features")})
    flow = [ns(chain=[ns(net_s_t=[ns(out_features=a["flow"]["hidden"])])] * a["flow"]["depth"])] * a["flow"]["count"]
    built = type("BuiltEncoder", (), {})()          # (attach keeps a weak reference to it)
    built.__dict__.update(part_aligner=part_aligner, flow=flow, **a["encoder"])
    mirror = attach(built)
    assert {k for k in mirror.state_dict() if not k.startswith("encoder.")} == {k for k in ref if not k.startswith("encoder.")}
    assert mirror.part_aligner.noise_scale == 100
    assert built.sample_latents.__name__ == "sample_latents"


def test_point_padding_helpers_of_the_engine():
    """Host logic behind 'any N like the reference': the kernels take N % 32 == 0, the engine pads with zeros / the shape's first
    label and cuts the padding off (points are independent).  The helpers are plain tensor code: checked here without a GPU."""
    import torch
    from difffacto_amd.engine import DenoiserEngine as E
    assert [E._pad(n) for n in (0, 1, 31, 32, 33, 100, 2048, 2080)] == [0, 31, 1, 0, 31, 28, 0, 0]
    x = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    xp = E._pad_last(x, 3)
    assert xp.shape == (2, 3, 8) and torch.equal(xp[..., :5], x) and float(xp[..., 5:].abs().sum()) == 0.0
    assert E._pad_last(None, 3) is None
    seg = torch.tensor([[2, 1, 0, 3, 3], [1, 1, 1, 0, 2]], dtype=torch.int32)
    sp = E._pad_seg(seg, 3)
    assert sp.shape == (2, 8) and sp.is_contiguous() and torch.equal(sp[:, :5], seg)
    assert sp[0, 5:].tolist() == [2, 2, 2] and sp[1, 5:].tolist() == [1, 1, 1]      # a label that is present in that shape


def test_pointnet_v2_rejects_cpu_tensors_in_every_mode():
    """No torch-layer fallback behind the native part encoder: CPU tensors raise the reference op's
    'CPU not supported' in eval / no_grad, eval / grad and train() alike."""
    import torch
    from difffacto_amd.encoders import PointNetV2
    enc = PointNetV2(zdim=256, num_anchors=4, per_part_mlp=True)
    x, attn = torch.zeros(2, 64, 3), torch.ones(2, 64, 4)
    for train in (False, True):
        enc.train(train)
        for grad in (False, True):
            with torch.set_grad_enabled(grad), pytest.raises(RuntimeError, match="CPU not supported"):
                enc(x, attn)


def test_parameter_generation_is_per_parameter_set():
    """an optimiser step on one parameter set must not invalidate the packed-weight caches of another (they key on
    training.generation_of(their own parameters), which Adam.step bumps per stepped tensor)."""
    import torch
    from difffacto_amd import training
    a, b = [torch.zeros(3), torch.zeros(2, 2)], [torch.zeros(5)]
    ga, gb, ga0 = training.generation_of(a), training.generation_of(b), training.generation_of(a[:1])
    training._bump_generation(a)
    g1 = training.generation_of(a)
    training._bump_generation(a)
    # every step of a's optimiser moves a's generation (and that of each of its tensors), never b's
    assert training.generation_of(a) > g1 > ga and training.generation_of(b) == gb and training.generation_of(a[:1]) > ga0


def test_generation_counter_follows_storage_aliases():
    """packed-weight caches key on training.generation_of(their parameters); an update through an ALIAS of a parameter
    (second Parameter / view on the same storage) must move it too, an update of unrelated tensors must not."""
    import torch
    from difffacto_amd import training
    p, q = torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(8))
    alias = torch.nn.Parameter(p.data)          # same storage, different tensor object
    view = p.data[2:6]
    g0p, g0q = training.generation_of([p]), training.generation_of([q])
    training._bump_generation([alias])
    assert training.generation_of([p]) > g0p and training.generation_of([q]) == g0q
    g1p = training.generation_of([p])
    training._bump_generation([view])
    assert training.generation_of([p]) > g1p and training.generation_of([q]) == g0q
    training._bump_generation([q])
    assert training.generation_of([q]) > g0q


def test_bench_evidence_helpers_read_the_newest_committed_profiles():
    """bench.py's roofline.traffic names the profile file and round it came from (newest committed rNN_traffic.json),
    and the power-limited ceiling is parsed from the newest committed micro-benchmark run instead of a hard-coded constant."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    traffic, src = b.measured_traffic(1000, 128, 2048)
    # round 5: fixed + per_step * T from PMC passes at two chain lengths (profiles/r05_write_size_scaling.txt: the writes do not grow with T at all;
    # rounds 1-4 multiplied ONE T = 20 launch by T / 20 and reported 4.2 GB) -> ~0.19 GB per T = 1000 launch
    assert traffic is not None and 1e8 < traffic < 1e9 and src["file"].startswith("profiles/r") and src["file"].endswith("_traffic.json")
    assert int(src["round"][1:]) >= 5 and "not measured in this run" in src["note"] and src["bytes_per_launch_fixed"] > 5e7
    assert abs(b.measured_traffic(40, 128, 2048)[0] - (src["bytes_per_launch_fixed"] + 40 * src["bytes_per_step"])) < 1.0
    assert b.measured_traffic(1000, 7, 2048) == (None, None)          # no profile for that batch: no number
    c = b.power_limited_ceiling()
    assert c["source"].startswith("profiles/r") and 1500 < c["bare_mfma_tflops"] < 2500 and 1000 < c["kernel_mix_tflops"] < c["refill_per_mfma_tflops"] < c["bare_mfma_tflops"]
    assert abs(b.flops_per_step(2048) - 4.733899e9) < 1e4


def test_reference_decode_protocol_through_install_on_oracle_backend(reference_registry, monkeypatch):
    """The drop-in protocol WITHOUT a GPU: the reference's AnchorDiffAE.decode (anchor_gen.py:145-169) is one call of the registered
    diffusion's p_sample_loop_progressive, iterated down to t = 0, with the keyword arguments recorded from the reference in
    tests/golden/reference_modules.npz (shape positional; anchors=, ctx=, variance=, noise=None, anchor_assignment=, valid_id=, device=,
    progress=).  The diffusion comes from the registry after difffacto_amd.install(), its libdfx handle replaced by the numpy-oracle
    stand-in (tests/_oracle_backend.py, test-only).  Checks: those arguments are accepted and the chain runs T steps to a finite cloud;
    seed-less sampling is FRESH per decode() call — ONE key per loop, a new one per call — and replays under torch.manual_seed.
    (The forward dict of the reference's gen branch against its golden: test_anchor_diff_ae_mirror_bookkeeping_on_oracle_backends.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _oracle_backend import OracleEngine
    import difffacto_amd
    from difffacto_amd import modules
    facts = _reference_facts()
    call = facts["decode_call"]
    T, B, N = 10, 2, 32
    assert difffacto_amd.install() is True
    from difffacto.utils.registry import DIFFUSIONS, build_from_cfg
    diffusion = build_from_cfg(dict(facts["configs"]["gen_chair.py"]["model_cfg"]["diffusion"], num_timesteps=T), DIFFUSIONS)
    assert isinstance(diffusion, modules.AnchoredDiffusion)
    diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()})
    diffusion.eval()
    engines = {}
    monkeypatch.setattr(modules.TransformerNet, "engine", lambda net: engines.setdefault(id(net), OracleEngine(
        {k: v.detach() for k, v in net.named_parameters()}, net._dfx_T, *net._dfx_betas)))

    pc, mean, logvar, valid = synth.make_latents(B, seed=5)
    t_ = torch.from_numpy
    ctx = [t_(pc), torch.cat([t_(mean), torch.exp(t_(logvar))], 1)]
    seg = t_(synth.make_seg_mask(valid, N))
    idx = seg.long()[:, None, :].expand(-1, 3, -1)
    anchors, variance = torch.gather(ctx[1][:, :3], 2, idx), torch.gather(ctx[1][:, 3:], 2, idx)
    kw = dict(anchors=anchors, ctx=ctx, variance=variance, noise=None, anchor_assignment=seg.to(torch.int32), valid_id=t_(valid),
              device="cpu", progress=False)
    assert call["args"] == 1 and sorted(kw) == call["kwargs"]

    def decode():   # what the reference's decode does with the diffusion (anchor_gen.py:149-158)
        steps, final = [], None
        for t, sample in diffusion.p_sample_loop_progressive([B, 3, N], **kw):
            steps.append(t)
            if t == 0:
                final = sample["sample"].transpose(2, 1)
        assert steps == list(range(T, -1, -1)) and final.shape == (B, N, 3) and bool(torch.isfinite(final).all())
        return final

    OracleEngine.seeds_seen = []
    try:
        torch.manual_seed(11)
        with torch.no_grad():
            a, b = decode(), decode()
        seeds = list(OracleEngine.seeds_seen)
        assert len(seeds) == 2 * T and len(set(seeds[:T])) == 1 and len(set(seeds[T:])) == 1 and seeds[0] != seeds[T]   # one key per loop
        assert not torch.equal(a, b)
        torch.manual_seed(11)
        with torch.no_grad():
            a2 = decode()
        assert torch.equal(a, a2)
    finally:
        OracleEngine.seeds_seen = []


@pytest.mark.parametrize("tag,chain_at", [("gen_B2_K2_T10", 3), ("sample_B2_K2_T10", 4)])
def test_anchor_diff_ae_mirror_bookkeeping_on_oracle_backends(tag, chain_at, monkeypatch):
    """networks.AnchorDiffAE.forward (the mirror's dict bookkeeping, draw order, K-fold regrouping) with every libdfx handle replaced by
    the numpy oracle (test-only stand-ins): equals the golden of the reference's AnchorDiffAE.forward.  The GPU twin of this test
    (tests/test_gpu_forward.py) runs the same comparison through the real kernels."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from _oracle_backend import OracleEngine, OracleLatentSampler
    from _replay import load_forward_fixture, replay_draws
    from difffacto_amd import encoders, modules, training
    from difffacto_amd.networks import AnchorDiffAE
    from oracle import pointnet_v2 as opv
    from oracle import prior_loss as opl
    batch, draws, expect, meta = load_forward_fixture(os.path.join(ROOT, "tests", "golden", f"forward_{tag}.npz"))
    T, K, N = int(meta["T"]), int(meta["K"]), batch["ref"].shape[1]
    m = AnchorDiffAE(encoder=dict(type="PartEncoderForTransformerDecoder", **ENC_CFG), diffusion=dict(type="AnchoredDiffusion", **DIFF_CFG),
                     sampler=dict(type="Uniform"), num_anchors=4, num_timesteps=T, npoints=N, gen=tag.startswith("gen"), cimle=True,
                     cimle_sample_num=K, ret_traj=True, ret_interval=int(meta["ret_interval"]))
    W = {"diffusion.model." + k: v for k, v in synth.make_denoiser_weights(0).items()}
    W.update({"encoder." + k: v for k, v in synth.make_latent_weights(0).items()})
    W.update({"encoder.encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    m.eval()
    engines = {}
    monkeypatch.setattr(modules.TransformerNet, "engine", lambda net: engines.setdefault(id(net), OracleEngine(
        {k: v.detach() for k, v in net.named_parameters()}, net._dfx_T, *net._dfx_betas)))
    monkeypatch.setattr(encoders, "LatentSampler", OracleLatentSampler)
    Wpn = synth.make_pointnet_v2_weights(0)
    monkeypatch.setattr(encoders.PointNetV2, "forward", lambda self, x, a: tuple(map(torch.from_numpy, opv.forward(Wpn, x.numpy(), a.numpy()))))

    def prior(params, part_code, logvar, valid, depth=14, hidden=256, prior_var=1.0, kl_weight=5e-4, stream=None):
        return opl.prior_loss({k: v.detach() for k, v in params.items()}, part_code, logvar, valid, depth=depth, prior_var=prior_var, kl_weight=kl_weight)
    monkeypatch.setattr(training, "prior_loss", prior)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    chain = draws[chain_at:chain_at + T + 1]
    orig = m.decode
    m.decode = lambda *a, **k: orig(*a, x_T_noise=torch.from_numpy(chain[0]), step_noise=torch.from_numpy(np.stack(chain[1:])), **k)
    with replay_draws(draws[:chain_at] + draws[chain_at + T + 1:]) as queue:
        out = m(batch, device="cpu", epoch=0)
    assert not queue
    pred, name = out[0]
    assert name == str(meta["name"]) and set(map(str, pred)) == set(expect), (sorted(map(str, pred)), sorted(expect))
    for k, v in pred.items():
        ref, got = expect[str(k)], v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if ref.dtype.kind in "iub":
            assert np.array_equal(got, ref), k
        else:
            assert float(np.abs(got - ref).max()) <= 2e-5 * max(1.0, float(np.abs(ref).max())), k


@pytest.mark.parametrize("cfg_name", ["gen_chair.py", "gen_airplane.py", "gen_car.py", "gen_lamp.py", "train_chair_stage1.py", "train_chair_stage2.py"])
def test_install_full_builds_the_mirror_from_the_unmodified_configs(cfg_name, reference_registry):
    """INTEGRATION.md §2's "take the whole model" binding: after `install(full=True)` the registry's
    `build_from_cfg(cfg.model, MODELS)` (utils/registry.py:24-46) on the `cfg.model` of an unmodified shipped config (as the reference's
    own `init_cfg` loads it, tests/golden/reference_modules.npz) yields `networks.AnchorDiffAE` whose `state_dict` has the reference
    model's keys, shapes and dtypes, and a checkpoint of that layout loads `strict=True` — also through the shape-checking, `strict=False`
    protocol of `Runner.load` (runner.py:505-520), with nothing dropped and nothing left unloaded."""
    import copy
    import difffacto_amd
    from difffacto_amd import networks, encoders, modules
    facts = _reference_facts()["configs"][cfg_name]
    model_cfg_ref = facts["model_cfg"]
    ref_sd = _checkpoint(facts["state_dict"])
    from difffacto.utils.registry import MODELS, ENCODERS, build_from_cfg
    import contextlib
    import io
    assert difffacto_amd.install(full=True) is True
    with contextlib.redirect_stdout(io.StringIO()):
        mine = build_from_cfg(copy.deepcopy(model_cfg_ref), MODELS)
    assert type(mine) is networks.AnchorDiffAE
    if cfg_name == "gen_chair.py":       # the dict the -m gpu composition tests build the mirror from IS this config's cfg.model
        assert _plain(model_cfg_ref) == {"type": "AnchorDiffAE", **model_cfg()}
    if cfg_name == "train_chair_stage2.py":   # stage 2 = gen_chair's model up to these keys (the stage2_step golden was made on gen_chair's)
        got, base = copy.deepcopy(model_cfg_ref), {"type": "AnchorDiffAE", **model_cfg()}
        assert got.pop("save_dir") and got.pop("ret_interval") == 1 and "cimle_sample_num" not in got
        assert got["encoder"]["part_aligner"].pop("noise_scale") == 50
        base.pop("ret_interval"), base.pop("cimle_sample_num"), base["encoder"]["part_aligner"].pop("noise_scale")
        assert got == base
    assert type(mine.encoder) is encoders.PartEncoderForTransformerDecoder and type(mine.encoder.encoder) is encoders.PointNetV2
    assert ENCODERS.get("PointNet2SSG") is encoders.PointNet2SSG and ENCODERS.get("PointNet2MSG") is encoders.PointNet2MSG   # (registered, unused by the configs)
    assert type(mine.diffusion) is modules.AnchoredDiffusion and type(mine.diffusion.model) is modules.TransformerNet
    my_sd = mine.state_dict()
    assert list(my_sd) == list(ref_sd) or set(my_sd) == set(ref_sd)
    assert len(ref_sd) == (473 if cfg_name == "train_chair_stage1.py" else 547)   # stage 1 has no part aligner (train_chair_stage1.py)
    for k, v in ref_sd.items():
        assert tuple(my_sd[k].shape) == tuple(v.shape) and my_sd[k].dtype == v.dtype, k
    assert sum(p.numel() for p in mine.parameters()) == facts["n_params"]
    mine.load_state_dict(ref_sd, strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(v, ref_sd[k]), k
    # Runner.load's protocol on a checkpoint written by DataParallel-wrapped training ("module." prefix stripped by the caller, runner.py:503)
    with contextlib.redirect_stdout(io.StringIO()):
        again = build_from_cfg(copy.deepcopy(model_cfg_ref), MODELS)
    ckpt = {"module." + k: v.clone() for k, v in ref_sd.items()}
    state = {k.replace("module.", ""): v for k, v in ckpt.items()}
    target = again.state_dict()
    dropped = [k for k in state if k not in target]
    reshaped = [k for k in state if k in target and state[k].shape != target[k].shape]
    missing = [k for k in target if k not in state]
    assert not dropped and not reshaped and not missing
    res = again.load_state_dict(state, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, ref_sd[k]) for k, v in again.state_dict().items())
