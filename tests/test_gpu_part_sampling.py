"""GPU checks of part-level sampling (csrc/part_sampling.hip, dfx_part_search / dfx_flow_reverse_part in latents_kernels.hip,
editing.sample_part and the mirrors of the reference's sample_with_fixed_latents / sample_one_part).

* the device selections against the host twin on the same inputs (bit-equal picks and fit sums; scores within one float32 ulp of the
  float64 closed form) at the boundary shapes of tests/_part_sampling_case.py;
* the draw statistics against the dumped normals (min / max exact, mean / std within one float32 ulp of float64), bit-equal under a
  split over row0, sane pooled moments;
* the single-part flow against column `part` of dfx_flow_reverse, bit-equal under dfx_debug_lin_split_k(1);
* the search against the composition "materialise the candidate codes, dfx_part_aligner, host-twin selection" (12 groups x 100
  candidates = 1200 aligner rows, the largest case here): equal picks, parameters bit-equal under dfx_debug_lin_split_k(1), one group
  per chunk against everything at once;
* the reference's fixtures end to end (tests/golden/partsample/): picks equal, latents within 5e-4 x max(1, |ref|), the decoded clouds
  with replayed chain draws within the fp32 chain gate of the edit goldens (2e-4).

A pick is compared exactly only where its float64 gap exceeds 4 x the largest measured |native - float64| error of its case (relative
to the winner); at most one group in ten may be left out, on the fixtures none.  The measured errors, gaps and exclusion counts go to
profiles/part_sampling_parity.txt once every case has run."""
import os

import numpy as np
import pytest
import torch

import _part_sampling_case as ps
from _replay import replay_draws
from difffacto_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, "profiles", "part_sampling_parity.txt")
PARITY = {}
PARITY_KEYS = {"selections", "draw_stats", "search", "fix_S4_E3", "one_part_S2_E2_T10"}
LATENT_TOL, CHAIN_TOL = 5e-4, 2e-4


def _record(key, lines):
    PARITY.setdefault(key, []).extend(lines)
    for line in lines:
        print("PART_SAMPLING_PARITY " + line)
    if set(PARITY) == PARITY_KEYS:
        head = ["# part-level sampling on the GPU against the host twin, the float64 restatement and the reference's fixtures",
                "# (tests/test_gpu_part_sampling.py; errors relative to the winner of the decision, gaps likewise)"]
        try:
            with open(PARITY_FILE, "w") as f:
                f.write("\n".join(head + [l for k in sorted(PARITY) for l in PARITY[k]]) + "\n")
        except OSError:
            pass


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def sampler():
    from difffacto_amd.latents import LatentSampler
    return LatentSampler(synth.make_latent_weights(seed=0), noise_scale=100.0)


@pytest.fixture()
def one_grouping(L):
    L.dfx_debug_lin_split_k(1)
    yield
    L.dfx_debug_lin_split_k(-1)


# ---------------------------------------------------------------------------------------------------- selections
def test_device_selections_equal_the_host_twin(L):
    from difffacto_amd import part_sampling as psm
    lines = []
    for G, K, J, P in ps.BOUNDARY_SHAPES:
        c = ps.make_case(G, K, J, seed=2000 + 7 * K + J)
        if K >= 63:                                       # non-finite candidates on the device path too
            c["mean"][K // 2, 0, 0] = np.nan
            c["logvar"][(G - 1) * K + 1, 2, J - 1] = np.inf
        d = psm.select_diverse(cu(c["mean"]), cu(c["logvar"]), cu(c["valid"]), K, P, stats=cu(c["stats"]))
        sc = host(d["scores"])
        want = ps.scores_f64(c["mean"], c["logvar"], c["valid"], c["stats"], K)
        fin = np.isfinite(want)
        # a candidate with a non-finite parameter is non-finite in both (numpy's max spreads a NaN over the candidate's box, fmax does not)
        assert np.isfinite(sc)[fin].all() and np.array_equal(np.isfinite(sc).all((1, 2)), fin.all((1, 2)))
        ulps = float((np.abs(sc.astype(np.float64)[fin] - want[fin]) / ps.ulp32(want[fin])).max())
        assert ulps <= 1.0, (G, K, J, ulps)
        idx, _, n_bad = ps.host_diverse(L, sc, c["valid"], K, P)
        assert np.array_equal(host(d["idx"]), idx) and int(d["n_bad"]) == n_bad
        w = ps.fit_weight(c["valid"], J - 1)
        f = psm.select_fit(cu(c["mean"]), cu(c["logvar"]), cu(c["tm"]), cu(c["tl"]), cu(w), K)
        fidx, fit, fbad = ps.host_fit(L, c["mean"], c["logvar"], c["tm"], c["tl"], w, K)
        assert np.array_equal(host(f["idx"]), fidx) and int(f["n_bad"]) == fbad
        assert np.array_equal(host(f["fit"]), fit, equal_nan=True)
        lines.append(f"selections G {G:2d} K {K:3d} J {J} P {P:3d}: scores {ulps:.3f} ulp of float64, picks and fit sums equal the host twin's, "
                     f"n_bad {n_bad} / {fbad}")
    _record("selections", lines)


# ---------------------------------------------------------------------------------------------------- draws
def test_draw_statistics(L):
    from difffacto_amd import part_sampling as psm
    lines = []
    pooled = []
    for rows, J, n, row0 in ((6, 4, 512, 0), (3, 5, 64, 7), (2, 8, 4, (1 << 33) + 5), (300, 1, 8, 0)):
        st = host(psm.draw_stats(rows, J, seed=11, row0=row0, n_draws=n))
        u = host(psm.draw_normals(rows, J, seed=11, row0=row0, n_draws=n))
        assert u.shape == (rows, n, 3, J) and np.isfinite(u).all()
        want = ps.stats_of(u)
        assert np.array_equal(st[:, 2], u.min(1)) and np.array_equal(st[:, 3], u.max(1))
        ulps = float((np.abs(st[:, :2].astype(np.float64) - want[:, :2]) / ps.ulp32(want[:, :2])).max())
        assert ulps <= 1.0, (rows, J, n, ulps)
        cut = rows // 2
        parts = [psm.draw_stats(cut, J, seed=11, row0=row0, n_draws=n), psm.draw_stats(rows - cut, J, seed=11, row0=row0 + cut, n_draws=n)]
        assert np.array_equal(host(torch.cat(parts)), st)
        assert not np.array_equal(host(psm.draw_stats(rows, J, seed=12, row0=row0, n_draws=n)), st)
        lines.append(f"draw_stats rows {rows} J {J} n {n} row0 {row0}: min / max exact, mean / std {ulps:.3f} ulp of float64, split over row0 bit-equal")
        pooled.append(u.reshape(-1).astype(np.float64))
    p = np.concatenate(pooled)
    m, v, k4 = p.mean(), p.var(), ((p - p.mean()) ** 4).mean() / p.var() ** 2
    se = 1.0 / np.sqrt(p.size)
    lines.append(f"draw_stats pooled {p.size} normals: mean {m:+.4f} (5 sigma = {5 * se:.4f}), variance {v:.4f}, kurtosis {k4:.3f}, |max| {np.abs(p).max():.2f}")
    assert abs(m) < 5 * se and abs(v - 1) < 5 * np.sqrt(2.0) * se and abs(k4 - 3) < 5 * np.sqrt(24.0) * se and 3 < np.abs(p).max() < 7
    c = np.corrcoef(p[:-1], p[1:])[0, 1]
    assert abs(c) < 5 * se
    # NULL stats = the same numbers drawn inside the selection
    c = ps.make_case(3, 20, 4, seed=4)
    a = psm.select_diverse(cu(c["mean"]), cu(c["logvar"]), cu(c["valid"]), 20, 6, stats=None, seed=9, row0=40, n_draws=512)
    b = psm.select_diverse(cu(c["mean"]), cu(c["logvar"]), cu(c["valid"]), 20, 6, stats=psm.draw_stats(60, 4, seed=9, row0=40))
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["idx"], b["idx"])
    _record("draw_stats", lines)


# ---------------------------------------------------------------------------------------------------- single-part flow
@pytest.mark.parametrize("S", [5, 33])
def test_single_part_flow_is_a_column_of_the_full_one(sampler, one_grouping, S):
    w = torch.randn(S, 256, 4, generator=torch.Generator().manual_seed(S)).cuda()
    full = sampler.flow_reverse(w)
    for part in range(4):
        col = w[:, :, part].contiguous()
        assert torch.equal(sampler.flow_reverse_part(part, col), full[:, :, part])
        assert torch.equal(sampler.flow_reverse_part(part, col, scale_prior=False), full[:, :, part])      # prior_var = 1
    assert not torch.equal(sampler.flow_reverse_part(0, w[:, :, 1].contiguous()), full[:, :, 1])


# ---------------------------------------------------------------------------------------------------- search
def _search_case(seed=21, S=4, E=3, K=100, J=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    G = S * E
    codes = rng.standard_normal((S, 256, J)).astype(np.float32)
    new = rng.standard_normal((G, 256)).astype(np.float32)
    valid = np.ones((S, J), np.float32)
    valid[1, 2] = valid[3, 0] = 0
    noise = rng.standard_normal((G * K, 32)).astype(np.float32)
    tm = (0.3 * rng.standard_normal((S, 3, J))).astype(np.float32)
    tl = (-4 + 0.5 * rng.standard_normal((S, 3, J))).astype(np.float32)
    rep = lambda a: np.repeat(a, E, axis=0)
    part = 1
    full = rep(codes).copy()
    full[:, :, part] = new
    return dict(codes=codes, new=new, valid=rep(valid), noise=noise, tm=rep(tm), tl=rep(tl), w=ps.fit_weight(rep(valid), part), part=part,
                code_a=np.repeat(np.repeat(np.arange(S, dtype=np.int32), E)[:, None], J, 1), full=full, G=G, K=K, J=J)


def _search(sampler, c, mode, P, budget, stats=None):
    kw = dict(target_mean=cu(c["tm"]), target_logvar=cu(c["tl"]), weight=cu(c["w"])) if mode == "fit" else {}
    if mode == "diverse":
        kw = dict(stats=stats)
    return sampler.part_search(cu(c["codes"]), c["code_a"], cu(c["valid"]), cu(c["noise"]), c["K"], mode, P=P, new_code=cu(c["new"]),
                               new_part=c["part"], row_budget=budget, return_scores=True, **kw)


def _composition(sampler, c):
    """Materialise the (G K, zdim, J) candidate codes and run one dfx_part_aligner call over them."""
    K = c["K"]
    mean, logvar = sampler.part_aligner(cu(np.repeat(c["full"], K, axis=0)), cu(np.repeat(c["valid"], K, axis=0)), cu(c["noise"]))
    return host(mean), host(logvar)


def test_search_equals_the_composition_bit_for_bit_with_one_k_grouping(L, sampler, one_grouping):
    c = _search_case()
    G, K, J = c["G"], c["K"], c["J"]
    stats = ps.make_case(G, K, J, seed=3, n_draws=512)["stats"]
    mean, logvar = _composition(sampler, c)
    rows = lambda idx: (np.arange(G)[:, None] * K + idx).reshape(-1)
    want = {"fit": ps.host_fit(L, mean, logvar, c["tm"], c["tl"], c["w"], K)[0][:, None],
            "first": np.tile(np.arange(5, dtype=np.int32), (G, 1)),
            "diverse": ps.host_diverse(L, ps.host_scores(L, mean, logvar, c["valid"], stats, K), c["valid"], K, 5)[0]}
    for mode, P in (("fit", 1), ("first", 5), ("diverse", 5)):
        outs = [_search(sampler, c, mode, P, budget, cu(stats)) for budget in (K, 5 * K, G * K)]       # chunks of 1, of 5 + 5 + 2 and of all 12 groups
        for o in outs:
            idx = host(o["idx"])
            assert np.array_equal(idx, want[mode]), mode
            r = rows(idx)
            assert np.array_equal(host(o["mean"]), mean[r]) and np.array_equal(host(o["logvar"]), logvar[r]) and np.array_equal(host(o["noise"]), c["noise"][r])
            assert int(o["n_bad"]) == 0
        for o in outs[1:]:
            assert mode == "first" or torch.equal(o["scores"], outs[0]["scores"])
    # NULL stats: the search draws each chunk's statistics itself, the numbers of dfx_part_draw_stats at the global rows
    from difffacto_amd import part_sampling as psm
    kw = dict(new_code=cu(c["new"]), new_part=c["part"], return_scores=True)
    own = sampler.part_search(cu(c["codes"]), c["code_a"], cu(c["valid"]), cu(c["noise"]), K, "diverse", P=5, seed=9, row0=70, row_budget=5 * K, **kw)
    given = sampler.part_search(cu(c["codes"]), c["code_a"], cu(c["valid"]), cu(c["noise"]), K, "diverse", P=5,
                                stats=psm.draw_stats(G * K, J, seed=9, row0=70), **kw)
    assert torch.equal(own["scores"], given["scores"]) and torch.equal(own["idx"], given["idx"]) and torch.equal(own["mean"], given["mean"])
    # a group of the recipe without a new code: the source shapes themselves
    plain = sampler.part_search(cu(c["codes"]), c["code_a"], cu(c["valid"]), cu(c["noise"]), K, "first", P=2, row_budget=3 * K)
    m0, l0 = sampler.part_aligner(cu(np.repeat(np.repeat(c["codes"], 3, axis=0), 2, axis=0)), cu(np.repeat(c["valid"], 2, axis=0)),
                                  cu(c["noise"].reshape(G, K, -1)[:, :2].reshape(G * 2, -1)))
    assert torch.equal(plain["mean"], m0) and torch.equal(plain["logvar"], l0)


def test_search_picks_do_not_depend_on_the_chunking_under_the_automatic_grouping(L, sampler):
    c = _search_case(seed=22)
    G, K = c["G"], c["K"]
    mean, logvar = _composition(sampler, c)
    _, fit64, gap = ps.fit_f64(mean, logvar, c["tm"], c["tl"], c["w"], K)
    lines, errs = [], []
    outs = [_search(sampler, c, "fit", 1, budget) for budget in (K, G * K)]
    for o in outs:
        errs.append(float((np.abs(host(o["scores"]).astype(np.float64) - fit64) / fit64.min(1, keepdims=True)).max()))
    err = max(errs)
    keep = gap > 4 * err
    assert (~keep).sum() <= G // 10, (gap, err)
    a, b = host(outs[0]["idx"])[:, 0], host(outs[1]["idx"])[:, 0]
    assert np.array_equal(a[keep], b[keep]) and np.array_equal(a[keep], ps.fit_f64(mean, logvar, c["tm"], c["tl"], c["w"], K)[0][keep])
    # the regrouped K sums move the last bits only: inside the front end's gate against its oracle (test_gpu_latents.py: 1e-4 x max(1, |ref|))
    ref = host(outs[1]["mean"])
    dm = float(np.abs(host(outs[0]["mean"]) - ref).max()) / max(1.0, float(np.abs(ref).max()))
    lines.append(f"search fit G {G} K {K}: chunk of one group vs everything: relative fit error to float64 {err:.3g}, smallest gap {gap.min():.3g}, "
                 f"groups left out {int((~keep).sum())}, picks equal, max relative mean difference {dm:.3g}")
    assert dm <= 1e-4
    _record("search", lines)


# ---------------------------------------------------------------------------------------------------- the reference's fixtures
def _model(T, N, precision):
    from test_gpu_edit import _model as edit_model
    return edit_model(T, N, 1, precision)


def _close(got, ref, tol, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))
    assert err <= tol, (what, err)
    return err


def _picks(noise_rows, draws, S, E, K):
    z = np.stack(draws[1:1 + S]).reshape(S * E, K, -1)
    return np.array([int(np.flatnonzero((z[g] == noise_rows[g]).all(1))[0]) for g in range(S * E)])


def test_fixed_size_fixture_end_to_end():
    d = ps.load("fix_S4_E3")
    E, K, part = int(d["E"]), int(d["K"]), int(d["part"])
    S, N = d["in/seg_mask"].shape
    draws = [d[f"draw_{i}"] for i in range(int(d["n_draws"]))]
    enc = _model(10, N, "f32").encoder
    t = lambda k: torch.from_numpy(d[k].copy()).cuda()
    with replay_draws(draws) as queue:
        ctx, mpp, lpp, seg, valid, (codes, noise, means, logvars) = enc.sample_with_fixed_latents(
            t("in/codes"), t("in/valid"), t("in/mean"), t("in/logvar"), t("in/seg_mask"), part, E, True, 7, True, K=K)
    assert not queue
    # fix_size overrides param_sample_num = 7 and selective: S*E rows, the reference's dtypes and row order (s*E + e)
    assert seg.dtype == torch.int64 and np.array_equal(host(seg), d["out/seg"]) and np.array_equal(host(valid), d["out/valid"])
    picks = _picks(host(noise), draws, S, E, K)
    rep = lambda a: np.repeat(a, E, axis=0)
    m, l = d["cand/mean"].reshape(-1, 3, 4), d["cand/logvar"].reshape(-1, 3, 4)
    _, fit64, gap = ps.fit_f64(m, l, rep(d["in/mean"]), rep(d["in/logvar"]), ps.fit_weight(rep(d["in/valid"]), part), K)
    # the native candidates' error: the picked rows' parameters against the reference's, relative to the winner's fit
    errs = {k: _close(got, d["out/" + k], LATENT_TOL, k) for k, got in (("codes", codes), ("noise", noise), ("means", means), ("logvars", logvars),
                                                                       ("mean_per_point", mpp), ("logvar_per_point", lpp))}
    assert np.array_equal(picks, d["picks"].reshape(-1)), (picks, d["picks"])
    assert np.array_equal(host(noise), d["out/noise"])
    _close(ctx[0], d["out/codes"], LATENT_TOL, "ctx0")
    _close(ctx[1], np.concatenate([d["out/means"], np.exp(d["out/logvars"])], axis=1), LATENT_TOL, "ctx1")
    _record("fix_S4_E3", [f"fix_S4_E3: picks equal the reference's in all {S * E} groups (smallest float64 gap {gap.min():.3g}, fixture's own "
                          f"{float(d['min_gap']):.3g} at float32 deviation {float(d['max_dev']):.3g}), groups left out 0; "
                          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (gate {LATENT_TOL})"])


def test_sample_one_part_fixture_end_to_end():
    from test_gpu_edit import _replay
    d = ps.load("one_part_S2_E2_T10")
    E, K, part, T = int(d["E"]), int(d["K"]), int(d["part"]), int(d["T"])
    S, N = d["in/seg_mask"].shape
    draws = [d[f"draw_{i}"] for i in range(int(d["n_draws"]))]
    model = _model(T, N, "f32")
    t = lambda k: torch.from_numpy(d[k].copy()).cuda()
    with _replay(model, draws, [], int(d["chain_at"]), T):
        out = model.sample_one_part(t("in/codes"), t("in/valid"), t("in/mean"), t("in/logvar"), t("in/seg_mask"), part, E, True, 1, False, K=K)
    names = ("pred", "seg", "valid", "codes", "noise", "means", "logvars")
    assert len(out) == 7
    for name, got in zip(names, out):
        assert tuple(got.shape) == d["out/" + name].shape, name
    assert out[1].dtype == torch.int64 and np.array_equal(host(out[1]), d["out/seg"]) and np.array_equal(host(out[2]), d["out/valid"])
    assert np.array_equal(_picks(host(out[4]), draws, S, E, K), d["picks"].reshape(-1))
    errs = {name: _close(got, d["out/" + name], LATENT_TOL, name) for name, got in zip(names[3:], out[3:])}
    errs["pred"] = _close(out[0], d["out/pred"], CHAIN_TOL, "pred")
    _record("one_part_S2_E2_T10", [f"one_part_S2_E2_T10: picks equal in all {S * E} groups (fixture gap {float(d['min_gap']):.3g}), groups left out 0; "
                                   + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (gates {LATENT_TOL} latents, {CHAIN_TOL} pred)"])


# ---------------------------------------------------------------------------------------------------- the public helper
def test_sample_part_modes_shapes_and_replay(one_grouping):
    from difffacto_amd import editing
    model = _model(10, 64, "bf16")
    enc, diff = model.encoder, model.diffusion
    g = torch.Generator().manual_seed(3)
    S, E, K, N = 3, 2, 16, 64
    codes = torch.randn(S, 256, 4, generator=g).cuda()
    valid = torch.ones(S, 4).cuda()
    valid[1, 3] = 0
    rm, rl = 0.3 * torch.randn(S, 3, 4, generator=g), -4 + 0.5 * torch.randn(S, 3, 4, generator=g)
    seg = torch.randint(0, 3, (S, N), generator=g).cuda()
    for kw, P in ((dict(fix_size=True, param_sample_num=4, selective=True), 1), (dict(fix_size=False, param_sample_num=3), 3),
                  (dict(fix_size=False, param_sample_num=3, selective=True), 3)):
        torch.manual_seed(5)
        a = editing.sample_part(enc, diff, codes, valid, rm, rl, 1, E, K=K, seg_mask=seg, npoints=N, seed=7, **kw)
        torch.manual_seed(5)
        b = editing.sample_part(enc, diff, codes, valid, rm, rl, 1, E, K=K, seg_mask=seg, npoints=N, seed=7, row_budget=K, **kw)
        assert a["pred"].shape == (S, E, P, N, 3) and a["idx"].shape == (S, E, P) and bool(torch.isfinite(a["pred"]).all())
        assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["pred"], b["pred"]) and int(a["n_bad"]) == 0
        R = S * E * P
        assert a["part_code"].shape == (R, 256, 4) and a["mean"].shape == (R, 3, 4) and a["noise"].shape == (R, 32)
        # the untouched parts are the shapes' own codes, bit for bit; the resampled part is shared by a style's P rows
        pc = a["part_code"].reshape(S, E * P, 256, 4)
        assert torch.equal(pc[:, :, :, [0, 2, 3]], codes[:, None, :, [0, 2, 3]].expand(-1, E * P, -1, -1))
        assert torch.equal(a["seg_mask"].reshape(S, E * P, N), seg[:, None].expand(-1, E * P, -1).to(torch.int32))
        if not kw["fix_size"] and not kw.get("selective"):
            assert torch.equal(a["idx"], torch.arange(P, dtype=torch.int32).cuda().expand(S, E, P))
        if P > 1:
            assert all(len(set(r)) == P for r in a["idx"].reshape(-1, P).tolist())
