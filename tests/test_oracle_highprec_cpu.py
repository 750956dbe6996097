"""The float64 oracle and the bf16 rounding model (oracle/highprec.py) and the error statistics (tests/_errstats.py) that the GPU gate
tests/test_gpu_denoiser_highprec.py stands on.  CPU only.

  * the float64 oracle is pinned to the reference: the goldens that the reference's own fp32 model produced lie within
    4 x |fp32 numpy oracle - float64 oracle| of it (max-abs and rms, same inputs; the 4 covers torch-vs-numpy summation order);
  * the yardsticks keep their order of magnitude (a later edit that turns the model into a no-op or into fp32 fails here);
  * self-test of the statistics: the unmutated rounding model in the kernel's place passes the GPU gate's acceptance function, each
    of the four deliberately wrong variants (oracle/highprec.py: ``mutate=``) fails it — a condition on the gate's thresholds;
  * the groups the GPU gate asserts on hold at least 512 error values.
"""
import os

import numpy as np
import pytest

import _errstats as es
from difffacto_amd import synth
from oracle import denoiser as dn
from oracle import diffusion as df
from oracle import highprec as hp

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PIN = 4.0       # |f64 - golden| <= PIN x |fp32 numpy oracle - f64|
ALL_GROUPS = tuple(es.GROUPINGS)


@pytest.fixture(scope="module")
def W():
    return synth.make_denoiser_weights(seed=0)


def _ctx(g):
    return [g["part_code"], np.concatenate([g["mean"], np.exp(g["logvar"])], axis=1).astype(np.float32)]


def _per_point(g):
    return df.gather_params(g["seg"], g["mean"], np.exp(g["logvar"]).astype(np.float32))


def _pin(what, truth, golden, f32):
    """The golden (the reference's fp32 output) is as close to the float64 oracle as fp32 arithmetic allows."""
    truth, golden, f32 = (np.asarray(a, dtype=np.float64) for a in (truth, golden, f32))
    assert truth.shape == golden.shape == f32.shape, what
    dg, d32 = truth - golden, truth - f32
    mx, my = np.abs(dg).max(), np.abs(d32).max()
    rx, ry = np.sqrt((dg * dg).mean()), np.sqrt((d32 * d32).mean())
    print(f"pin {what}: |f64 - golden| max {mx:.2e} rms {rx:.2e}; |f64 - fp32 oracle| max {my:.2e} rms {ry:.2e}; ratio max {mx / my:.2f} rms {rx / ry:.2f}")
    assert my > 0 and mx <= PIN * my, (what, mx, my)
    assert rx <= PIN * ry, (what, rx, ry)


@pytest.mark.parametrize("tag", ["B2_N128_mixed", "B2_N128_allvalid", "B1_N2048"])
def test_f64_eps_pinned_to_reference_golden(W, tag):
    g = np.load(os.path.join(GOLDEN, f"denoiser_eps_{tag}.npz"))
    anchors, variance = _per_point(g)
    B = g["x"].shape[0]
    net = hp.Net(W)
    for t in g["ts"]:
        args = (g["x"], np.full((B,), t), _ctx(g), anchors.transpose(0, 2, 1), variance.transpose(0, 2, 1), g["valid"], g["seg"])
        _pin(f"eps {tag} t={int(t)}", hp.transformer_net_forward(net, *args), g[f"eps_t{int(t)}"], dn.transformer_net_forward(W, *args))


def _chain_pin(W, g, tb, what):
    anchors, variance = _per_point(g)
    args = (anchors, _ctx(g), variance, g["seg"], g["valid"], g["x_T_noise"], g["step_noise"])
    t64 = np.stack([o["sample"] for _, o in hp.p_sample_loop_progressive(tb, W, *args)])
    t32 = np.stack([o["sample"] for _, o in df.p_sample_loop_progressive(tb, W, *args)])
    _pin(what + " trajectory", t64[1:], g["traj"][1:], t32[1:])
    ri = int(g["ret_interval"])
    d64 = hp.decode(tb, W, *args, ret_traj=True, ret_interval=ri)
    d32 = df.decode(tb, W, *args, ret_traj=True, ret_interval=ri)
    assert sorted("decode_" + str(k) for k in d64) == sorted(k for k in g.files if k.startswith("decode_"))
    _pin(what + " decode pred", d64["pred"], g["decode_pred"], d32["pred"])


@pytest.mark.parametrize("tag", ["B2_N128_mixed", "B3_N64_allvalid"])
def test_f64_ddpm_chain_pinned_to_reference_golden(W, tag):
    _chain_pin(W, np.load(os.path.join(GOLDEN, f"chain_T10_{tag}.npz")), df.Tables(10), f"chain_T10_{tag}")


DDIM_CASES = {"quad8_eta1": dict(ddim_nsteps=8, ddim_discretize="quad", ddim_eta=1.0),
              "uniform5_eta0": dict(ddim_nsteps=5, ddim_discretize="uniform", ddim_eta=0.0)}


@pytest.mark.parametrize("name", sorted(DDIM_CASES))
def test_f64_ddim_chain_pinned_to_reference_golden(W, name):
    g = np.load(os.path.join(GOLDEN, f"ddim_T40_{name}_B2_N64.npz"))
    tb = df.Tables(40, ddim_sampling=True, **DDIM_CASES[name])
    assert tb.steps == g["steps"].tolist()
    _chain_pin(W, g, tb, f"ddim_T40_{name}")


def test_f64_training_forward_pinned_to_reference_golden(W):
    """q_sample, the per-shape-t denoiser and the masked MSE.  The loss is ONE number: its fp32 yardstick is the fp32 oracle's error
    on it or one fp32 ulp of it, whichever is larger (a single value can round luckily)."""
    g = np.load(os.path.join(GOLDEN, "train_fwd_B3_N64_T10.npz"))
    tb = df.Tables(10)
    anchors, variance = _per_point(g)
    for name, fl in (("flags", g["flags"]), ("noflags", None)):
        args = (g["x_start"], g["t"], anchors, variance, _ctx(g), g["seg"], g["valid"], fl, g["noise"])
        r64, r32 = hp.training_losses(tb, W, *args), df.training_losses(tb, W, *args)
        _pin("train_fwd x_t", r64["x_t"], g["x_t"], r32["x_t"])
        ref = float(g["mse_loss_" + name])
        yard = max(abs(float(r32["mse_loss"]) - r64["mse_loss"]), float(np.spacing(np.float32(ref))))
        print(f"pin train_fwd mse_loss_{name}: f64 {r64['mse_loss']:.9f} golden {ref:.9f} fp32 oracle {float(r32['mse_loss']):.9f}")
        assert abs(r64["mse_loss"] - ref) <= PIN * yard, (name, r64["mse_loss"], ref, yard)
        assert hp.masked_mse(g["noise"], r64["eps"], fl) == r64["mse_loss"]


# ------------------------------------------------------------------------------------------------ yardsticks and the statistics
SEEDS = (11, 12)      # 11: the case of the GPU gate's B = 4 x N = 2048 eps test; 12: a second draw of latents, labels and x


FOLDS = (None, 127)   # the rounding model of the plain W1 pack, and of the folded pack every benchmark kernel runs (the GPU gate's yardstick)


@pytest.fixture(scope="module")
def table_case(W):
    """B = 4, N = 2048, mixed validity: the truth, the fp32 oracle's error, the rounding model's error for the plain and the folded W1
    pack (`models[fold]`; `model` = the plain one) and the float64 ranking of block 2's hidden units, per (seed, t), computed once."""
    cache = {}

    def get(seed, t):
        if (seed, t) not in cache:
            c = es.make_case(4, 2048, seed)
            truth = es.eps_of(hp, W, c, t)
            models = {f: es.stats(es.eps_of(hp, W, c, t, operand_round="bf16", w1_fold=f) - truth) for f in FOLDS}
            order = hp.ff_unit_ranking(W, c["x"], np.full((4,), t), c["ctx"], c["anchors"].transpose(0, 2, 1),
                                       c["variance"].transpose(0, 2, 1), c["valid"], c["seg"])
            cache[seed, t] = dict(case=c, truth=truth, f32=es.stats(es.eps_of(dn, W, c, t) - truth), models=models, model=models[None],
                                  unit=int(order[hp.MUT_RANK]), order=order)
        return cache[seed, t]
    return get


def test_threshold_conditions():
    """What the GPU gate's thresholds must respect wherever the measurements put them: below the weakest mutation on the overall rms
    (1.95: truncation) and on the lane groupings (1.40: a halved unit), and a small multiple for fp32."""
    assert es.RB < 1.5 and es.R32 <= 8.0
    assert all(es.G[k] <= 1.25 for k in ("lane", "lane16", "wave"))
    assert set(es.G) == set(es.GROUPINGS) and es.MIN_GROUP >= 512


@pytest.mark.parametrize("seed", SEEDS)
def test_yardsticks_keep_their_order_of_magnitude(table_case, seed):
    c = table_case(seed, 500)
    print(f"yardsticks seed {seed} t=500: fp32 oracle max {c['f32']['max']:.2e} rms {c['f32']['rms']:.2e}; "
          f"rounding model max {c['model']['max']:.2e} rms {c['model']['rms']:.2e}")
    assert 3e-8 <= c["f32"]["rms"] <= 1e-6, c["f32"]
    assert 2e-4 <= c["model"]["rms"] <= 2e-3, c["model"]
    assert np.abs(c["truth"]).max() > 1.0          # eps is O(1): the brackets are absolute


def test_w1_fold_site_of_the_model(W, table_case):
    """The folded W1 pack is the same function in real arithmetic, so its rounding model stays a rounding model: same order of magnitude
    as the plain one (the weight differences round a little coarser), for channel 127 and for a moved channel."""
    c = table_case(11, 500)
    for k in (127, 5):
        s = es.stats(es.eps_of(hp, W, c["case"], 500, operand_round="bf16", w1_fold=k) - c["truth"])
        print(es.line(f"self-test seed 11 t=500 w1_fold={k}", "rounding model, folded", s, c["model"]))
        assert 2e-4 <= s["rms"] <= 2e-3 and 0.8 <= s["rms"] / c["model"]["rms"] <= 1.6, s
        assert es.accept("bf16", s, s, ALL_GROUPS) == []
    with pytest.raises(ValueError):
        hp.Net(W, w1_fold=127)


def test_fp32_kernels_accumulation_order_costs_a_small_multiple_of_the_blas_order(W):
    """Why R32 is not about 1: the fp32 kernels accumulate the to_out and FF net.2 products straight into the fp32 residual stream
    (hp.fp32_residual_order_forward).  On the GPU gate's B3_N100 case — where the kernels measured rms 7.5e-7 .. 7.9e-7 = up to 6.7 x the
    numpy oracle — that order alone costs 3 to 8 times the BLAS-ordered oracle's rms error (5.0 x with one rounding per MFMA, 7.1 x with one per product)."""
    c = es.make_case(3, 100, 14)
    for t in (0, 500):
        truth = es.eps_of(hp, W, c, t)
        base = es.stats(es.eps_of(dn, W, c, t) - truth)
        for step in (2, 1):
            s = es.stats(es.eps_of(hp.fp32_residual_order_forward, W, c, t, terms_per_step=step) - truth)
            print(f"fp32 residual-order oracle B3_N100 t={t}, {step} product(s) per rounding: rms {s['rms']:.3e} max {s['max']:.3e} = "
                  f"{s['rms'] / base['rms']:.2f} x / {s['max'] / base['max']:.2f} x the numpy oracle's ({base['rms']:.3e} / {base['max']:.3e})")
            assert 3.0 <= s["rms"] / base["rms"] <= es.R32 and 4e-7 <= s["rms"] <= 1.2e-6, (t, step, s["rms"], base["rms"])
            if step == 2:         # one rounding per MFMA: inside the gate; one per product (3.3e-6 max-abs) is past it on max-abs
                assert es.accept("f32", s, base) == []


def test_rounding_helper():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 0.0])
    assert hp.round_bf16(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 0.0]       # ties to even
    assert hp.round_bf16(x, truncate=True).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, -1.0, 0.0]
    r = hp.round_bf16(np.random.default_rng(0).standard_normal(4096))
    assert r.dtype == np.float64 and np.array_equal(r.astype(np.float32).view(np.uint32) & 0xFFFF, np.zeros(4096, np.uint32))
    with pytest.raises(ValueError):
        hp.Net({}, operand_round="fp16")
    with pytest.raises(ValueError):
        hp.Net({}, mutate="truncate")


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_unmutated_model_passes_the_gate_and_its_groups_are_quiet(table_case, seed, fold):
    for t in (500, 5):
        c = table_case(seed, t)
        m = c["models"][fold]
        print(es.line(f"self-test seed {seed} t={t} w1_fold={fold}", "rounding model", m, m))
        assert es.accept("bf16", m, m, ALL_GROUPS) == []
        for name in ALL_GROUPS:           # the model's own sampling spread stays below each grouping's threshold
            g = m["groups"][name]
            assert g["min_count"] >= es.MIN_GROUP and g["worst"] < es.G[name], (name, g)
        assert es.accept("f32", c["f32"], c["f32"]) == []


RMS_BLIND = {("truncate", 12, 5, 127)}     # (mutation, seed, t, fold) that fails the gate on max-abs only: see the docstring below
SHARP = {"truncate": "rms ", "t_plus_one": "rms ", "drop_unit": "lane group 5", "halve_unit": "lane group 5"}


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("t", [500, 5])
@pytest.mark.parametrize("mutation", ["truncate", "drop_unit", "halve_unit", "t_plus_one"])
def test_each_mutation_fails_the_gate(W, table_case, seed, mutation, t, fold):
    """The mutated model in the kernel's place, judged as a bf16 kernel is: against the unmutated model of the SAME pack — the plain
    one, and the folded one (w1_fold = 127) that the GPU gate builds for every benchmark kernel — on two seeds and at both ends of the
    t list.  All four pass a 6e-3 max-abs gate at some t.  Each must fail, and by the statistic built to see it: the overall rms for
    truncation and the time table, lane 5's group for the unit.

    What the unit mutations prove is a statement about weight.  The unit is rank hp.MUT_RANK = 64 of block 2's 512 hidden units by
    the energy it carries in the float64 forward of the same inputs (hp.ff_unit_ranking: independent of the mutated run, of the fold
    and of the rounding).  Halved in one lane it gives a lane ratio of 1.59 .. 3.4 over these 8 cases (threshold 1.25), dropped
    2.5 .. 4.7; ranks 32 and 128 give 1.47 .. 3.3 halved.  The folded yardstick is 0.98 to 1.28 times the plain one and costs that much
    sensitivity: the same unit's lane ratio falls from 1.90 to 1.63 (seed 12, t = 500), truncation's rms ratio from 1.96 to 1.48 there
    (RB = 1.42).  Lighter units are seen less: around rank 320 a halved unit shows 1.05 .. 1.3 against the folded yardstick and passes
    — its whole contribution is below the rounding noise of the other 511 units in that lane.

    One case is caught by the maximum alone (RMS_BLIND): truncation against the folded yardstick at seed 12, t = 5 has an rms ratio of
    1.409, just under RB = 1.42 (measured worst kernel 1.134 x 1.25), and fails on max-abs (1.59 > RMAX = 1.53).  Truncation roughly
    doubles the activation rounding noise but leaves the weight rounding, and the folded pack's coarser weights are a larger share of
    the yardstick; the other seven truncation cases exceed RB (1.48 .. 2.03)."""
    c = table_case(seed, t)
    yard = c["models"][fold]
    m = (mutation, c["unit"]) if mutation.endswith("_unit") else mutation
    s = es.stats(es.eps_of(hp, W, c["case"], t, operand_round="bf16", w1_fold=fold, mutate=m) - c["truth"])
    print(es.line(f"self-test seed {seed} t={t} w1_fold={fold} mutate={m}", "mutated model", s, yard))
    fails = es.accept("bf16", s, yard, ALL_GROUPS)
    print("   ->", fails)
    assert fails, (mutation, es.ratios(s, yard))
    if (mutation, seed, t, fold) in RMS_BLIND:
        assert [f[:4] for f in fails] == ["max "] and es.ratios(s, yard)["rms"] > 1.35, fails
    else:
        assert any(f.startswith(SHARP[mutation]) for f in fails), (mutation, fails)     # not by the maximum alone
    if mutation != "t_plus_one":          # fp32: any of these shows at once
        assert es.accept("f32", s, c["f32"])


def test_mutated_unit_is_the_callers_choice(W, table_case):
    c = table_case(11, 500)
    assert sorted(c["order"].tolist()) == list(range(512))
    for bad in ("drop_unit", ("truncate", 3), ("drop_unit",)):
        with pytest.raises((ValueError, IndexError)):
            hp.Net(W, operand_round="bf16", mutate=bad)


def test_t_plus_one_is_a_mutation_of_the_exact_model_too(W, table_case):
    c = table_case(11, 5)
    s = es.stats(es.eps_of(hp, W, c["case"], 5, mutate="t_plus_one") - c["truth"])
    assert s["max"] < 6e-3 and es.accept("f32", s, c["f32"])      # invisible to a 6e-3 max-abs gate, plain to the fp32 yardstick


@pytest.mark.parametrize("B,N,groups", [(4, 2048, ALL_GROUPS), (1, 8192, ("lane", "lane16", "wave", "tile", "coord")),
                                        (12, 2048, ALL_GROUPS)])
def test_groups_of_the_gpu_cases_are_large_enough(B, N, groups):
    s = es.stats(np.ones((B, 3, N)), groups)
    for name in groups:
        assert s["groups"][name]["min_count"] >= 512, (name, s["groups"][name])
        assert abs(s["groups"][name]["worst"] - 1.0) < 1e-12
    small = es.stats(np.ones((3, 3, 100)))
    assert set(es.ratios(small, small)) == {"rms", "max", "tile"}             # N = 100: one tile of 900 values, every other group too small
    with pytest.raises(AssertionError, match="too small"):
        es.accept("bf16", small, small, ("lane",))
