"""CPU checks of part-level sampling's candidate selection: the entry points are exported and bound and reject bad arguments before
touching a GPU; the kernels' own score / selection routines, compiled for the host (dfx_debug_part_scores_host,
dfx_debug_select_diverse_host, dfx_debug_select_fit_host), against the float64 restatements of tests/_part_sampling_case.py and
against the reference's recorded picks (tests/golden/partsample/, make_golden_partsample.py).

Gates.  Scores: within one float32 ulp of the float64 closed form (they are float64 arithmetic rounded once; exp / log of the two
libraries differ in the last float64 bits, which can move a rounding).  Picks on the twin's own float32 scores: equal to the float64
greedy / arg-min on those scores, no margin (the distances are float64 sums of the same terms in the same order).  Picks against the
reference: equal wherever the decision's float64 gap exceeds 4 x the largest relative |native - float64| distance error of the case; on
the fixtures that must hold for every group (the generator refuses near-ties).  The last test shows that these gates reject five
deliberately wrong variants of the restatement."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _part_sampling_case as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfx_flow_reverse_part", "dfx_part_draw_stats", "dfx_select_diverse", "dfx_select_fit", "dfx_part_search",
       "dfx_debug_part_draw_normals", "dfx_debug_part_scores_host", "dfx_debug_select_diverse_host", "dfx_debug_select_fit_host")
FAKE = ctypes.c_void_p(0x1000)   # a non-null "device pointer": never dereferenced, the checks fail first
FIXTURES = ("diverse_G6_K100_P8", "fix_S4_E3", "one_part_S2_E2_T10")


@pytest.fixture(scope="module")
def L():
    from difffacto_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _err(L, rc):
    return rc, (L.dfx_last_error() or b"").decode()


def test_symbols_are_exported_and_bound(L):
    from difffacto_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert L.dfx_version() >= 106 and L.dfx_abi_version() == 5 == _ffi.DFX_ABI_VERSION


def test_fixture_manifest():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import manifest
    want = {}
    for ln in open(os.path.join(ps.GOLDEN, "MANIFEST.sha256")):
        if ln.strip() and not ln.startswith("#"):
            h, name = ln.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(ps.GOLDEN, f)) for f in sorted(os.listdir(ps.GOLDEN)) if f.endswith(".npz")}
    assert want == have and set(have) == {t + ".npz" for t in FIXTURES}
    assert all(os.path.getsize(os.path.join(ps.GOLDEN, f)) < 1 << 20 for f in have)
    for t in FIXTURES:
        d = ps.load(t)
        assert d["min_gap"] >= 20 * d["max_dev"] > 0, t


def test_selection_entry_points_reject_bad_arguments_without_a_gpu(L):
    def diverse(G=2, K=8, J=4, P=2, mean=FAKE, stats=FAKE, scores=FAKE):
        return _err(L, L.dfx_select_diverse(mean, FAKE, FAKE, stats, G, K, J, P, FAKE, scores, FAKE, None))
    for kw, msg in [(dict(G=0), "positive"), (dict(K=0), "positive"), (dict(K=4097), "K = 4097"), (dict(J=9), "n_class = 9"), (dict(J=0), "n_class = 0"),
                    (dict(P=0), "P = 0"), (dict(P=9), "P = 9"), (dict(mean=None), "null"), (dict(scores=None), "null"),
                    (dict(stats=None), "null")]:
        rc, m = diverse(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)

    def fit(G=2, K=8, J=4, w=FAKE, idx=FAKE):
        return _err(L, L.dfx_select_fit(FAKE, FAKE, FAKE, FAKE, w, G, K, J, idx, None, FAKE, None))
    for kw, msg in [(dict(G=-1), "positive"), (dict(K=5000), "K = 5000"), (dict(J=9), "n_class"), (dict(w=None), "null"), (dict(idx=None), "null")]:
        rc, m = fit(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)

    def stats(row0=0, rows=4, J=4, n=512, out=FAKE):
        return _err(L, L.dfx_part_draw_stats(3, row0, rows, J, n, out, None))
    for kw, msg in [(dict(row0=-2), "row0"), (dict(rows=0), "rows = 0"), (dict(J=9), "n_class"), (dict(n=510), "n_draws = 510"), (dict(n=2), "n_draws = 2"),
                    (dict(out=None), "null")]:
        rc, m = stats(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)
    assert L.dfx_debug_part_draw_normals(3, 0, 2, 4, 7, FAKE, None) == -1


def test_search_and_flow_entry_points_check_everything_before_the_first_hip_call(L):
    """Against a handle that holds sizes and no device memory: a call that passes every check stops at "holds no weights"."""
    h = ctypes.c_void_p()
    assert L.dfx_debug_latents_stub(ctypes.byref(h), 4, 256, 1, 32) == 0
    G, K, J = 3, 10, 4
    good_a = np.zeros((G, J), np.int32)

    def search(handle=h, S=2, code_a=good_a, new_code=FAKE, new_part=1, G=G, K=K, mode=0, P=1, tm=FAKE, w=FAKE, stats=None, n_draws=512,
               budget=0, idx=FAKE):
        a = np.ascontiguousarray(code_a, np.int32)
        return _err(L, L.dfx_part_search(handle, FAKE, S, a.ctypes.data_as(ctypes.c_void_p), new_code, new_part, FAKE, FAKE, G, K, mode, P, tm,
                                         FAKE, w, stats, 5, 0, n_draws, budget, idx, FAKE, FAKE, FAKE, None, FAKE, None))
    bad_a = good_a.copy()
    bad_a[2, 1] = 2
    for kw, msg in [(dict(handle=None), "null handle"), (dict(K=0), "positive"), (dict(K=4097), "K = 4097"), (dict(mode=3), "mode 3"),
                    (dict(mode=-1), "mode -1"), (dict(P=2), "picks one"), (dict(mode=1, P=11), "P = 11"), (dict(mode=2, P=0), "P = 0"),
                    (dict(code_a=bad_a), "code_a[9] = 2 outside [0,2)"), (dict(new_part=4), "new_part 4"), (dict(new_part=-1), "together"),
                    (dict(new_code=None), "together"), (dict(tm=None), "targets"), (dict(w=None), "targets"), (dict(budget=9), "row_budget 9"),
                    (dict(mode=2, n_draws=3), "n_draws = 3"), (dict(idx=None), "null pointer"), (dict(S=0), "code_src")]:
        rc, m = search(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)
    for kw in (dict(), dict(mode=1, P=10, tm=None, w=None), dict(mode=2, P=3, tm=None, w=None), dict(mode=2, P=3, stats=FAKE, n_draws=0),
               dict(new_code=None, new_part=-1), dict(budget=10)):
        rc, m = search(**kw)
        assert rc == -1 and "holds no weights" in m, (kw, rc, m)
    for part, msg in ((4, "part 4 outside [0,4)"), (-1, "part -1"), (2, "holds no weights")):
        rc, m = _err(L, L.dfx_flow_reverse_part(h, part, FAKE, 1, FAKE, 5, None))
        assert rc == -1 and msg in m, (part, rc, m)
    assert L.dfx_flow_reverse_part(h, 0, None, 1, None, 0, None) == 0           # no rows: a no-op
    L.dfx_latents_destroy(h)
    h2 = ctypes.c_void_p()
    assert L.dfx_debug_latents_stub(ctypes.byref(h2), 4, 256, 0, 0) == 0
    rc, m = search(handle=h2)
    assert rc == -1 and "without cimle" in m
    L.dfx_latents_destroy(h2)


def test_python_layer_without_a_gpu():
    import types
    from difffacto_amd import editing
    code_a, shape_row = editing.part_sampling_recipe(S=2, E=3, P=2, n_class=4, part_id=1)
    assert code_a.shape == (12, 4) and shape_row.tolist() == [0] * 6 + [1] * 6
    assert code_a[:, [0, 2, 3]].tolist() == [[s] * 3 for s in shape_row] and code_a[:, 1].tolist() == [2 + g for g in range(6) for _ in range(2)]
    for aligner in (None, types.SimpleNamespace(cimle=False)):
        with pytest.raises(NotImplementedError, match="cIMLE"):
            editing.sample_part_latents(types.SimpleNamespace(part_aligner=aligner), None, None, None, None, 0, 2)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def _score_ulps(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float((np.abs(got.astype(np.float64) - want)[fin] / ps.ulp32(want[fin])).max())


@pytest.mark.parametrize("G,K,J,P", ps.BOUNDARY_SHAPES)
def test_scores_and_picks_follow_the_float64_restatement(L, G, K, J, P):
    c = ps.make_case(G, K, J, seed=1000 + 7 * K + J)
    sc = ps.host_scores(L, c["mean"], c["logvar"], c["valid"], c["stats"], K)
    ulps = _score_ulps(sc, ps.scores_f64(c["mean"], c["logvar"], c["valid"], c["stats"], K))
    print(f"G {G} K {K} J {J}: scores within {ulps:.3g} float32 ulp of the float64 closed form")
    assert ulps <= 1.0
    idx, dist, n_bad = ps.host_diverse(L, sc, c["valid"], K, P)
    idx64, dist64, _ = ps.diverse_f64(sc, c["valid"], K, P)
    assert n_bad == 0 and np.array_equal(idx, idx64)
    assert np.allclose(dist, dist64, rtol=1e-12, atol=0)
    assert all(len(set(row)) == P for row in idx.tolist())
    w = ps.fit_weight(c["valid"], part=J - 1)
    fidx, fit, n_bad = ps.host_fit(L, c["mean"], c["logvar"], c["tm"], c["tl"], w, K)
    fidx64, fit64, _ = ps.fit_f64(c["mean"], c["logvar"], c["tm"], c["tl"], w, K)
    assert n_bad == 0 and np.array_equal(fidx, fidx64)
    assert np.array_equal(fit, fit64.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the reference's recorded picks
def test_diverse_picks_and_parameters_equal_the_reference(L):
    d = ps.load("diverse_G6_K100_P8")
    K, P = int(d["K"]), int(d["P"])
    G, J = d["valid"].shape
    sc = ps.host_scores(L, d["mean"], d["logvar"], d["valid"], d["stats"].astype(np.float32), K)
    sc64 = ps.scores_f64(d["mean"], d["logvar"], d["valid"], d["stats"], K)
    idx, dist, n_bad = ps.host_diverse(L, sc, d["valid"], K, P)
    idx64, dist64, gap = ps.diverse_f64(sc64, d["valid"], K, P)
    err = float(np.abs(dist[:, 1:] - dist64[:, 1:]).max() / dist64[:, 1:].min())
    left_out = [g for g in range(G) if not gap[g, 1:].min() > 4 * err]
    print(f"diverse fixture: score error {_score_ulps(sc, sc64):.3g} ulp (float32 stats), relative distance error {err:.3g}, smallest gap "
          f"{gap[:, 1:].min():.3g}, groups left out {left_out}")
    assert not left_out and n_bad == 0
    assert np.array_equal(idx64, d["ids"]), "float64 closed form"
    assert np.array_equal(idx, d["ids"])
    rows = (np.arange(G)[:, None] * K + idx).reshape(-1)
    assert np.array_equal(d["mean"][rows], d["sel_mean"]) and np.array_equal(d["logvar"][rows], d["sel_logvar"])


@pytest.mark.parametrize("name", ["fix_S4_E3", "one_part_S2_E2_T10"])
def test_fit_picks_equal_the_reference(L, name):
    d = ps.load(name)
    K, E, part = int(d["K"]), int(d["E"]), int(d["part"])
    S, J = d["in/valid"].shape
    # the reference's returned (noise, mean, logvar) identify its picks: the rows of the recorded candidates it gathered
    noise = np.stack([d[f"draw_{1 + s}"] for s in range(S)]).reshape(S * E, K, -1)
    ref_pick = np.array([int(np.flatnonzero((noise[g] == d["out/noise"].reshape(S * E, -1)[g]).all(1))[0]) for g in range(S * E)])
    assert np.array_equal(ref_pick, d["picks"].reshape(-1))
    rep = lambda a: np.repeat(a, E, axis=0)
    w = ps.fit_weight(rep(d["in/valid"]), part)
    m, l = d["cand/mean"].reshape(S * E * K, 3, J), d["cand/logvar"].reshape(S * E * K, 3, J)
    idx, fit, n_bad = ps.host_fit(L, m, l, rep(d["in/mean"]), rep(d["in/logvar"]), w, K)
    _, fit64, gap = ps.fit_f64(m, l, rep(d["in/mean"]), rep(d["in/logvar"]), w, K)
    err = float((np.abs(fit.astype(np.float64) - fit64) / fit64.min(1, keepdims=True)).max())
    print(f"{name}: relative fit error {err:.3g}, smallest gap {gap.min():.3g}")
    assert gap.min() > 4 * err and n_bad == 0
    assert np.array_equal(idx, ref_pick)
    rows = np.arange(S * E) * K + idx
    assert np.array_equal(m[rows], d["out/means"].reshape(S * E, 3, J)) and np.array_equal(l[rows], d["out/logvars"].reshape(S * E, 3, J))


# ---------------------------------------------------------------------------------------------------- ties, degenerate masks, non-finite values
def _tie_case():
    c = ps.make_case(2, 10, 4, seed=77)
    sc = np.zeros((2 * 10, 6, 4), np.float32)
    rng = np.random.Generator(np.random.PCG64(78))
    sc[:] = 0.1 * rng.standard_normal(sc.shape)
    for g in range(2):
        sc[g * 10 + 3] = sc[g * 10 + 7] = 5.0 + g            # identical, and far from every other candidate
    return c, sc


def test_of_two_identical_candidates_the_lower_index_wins(L):
    c, sc = _tie_case()
    idx, dist, _ = ps.host_diverse(L, sc, c["valid"], 10, 10)
    assert idx[:, 0].tolist() == [0, 0] and idx[:, 1].tolist() == [3, 3]
    assert idx[:, -1].tolist() == [7, 7] and dist[:, -1].tolist() == [0.0, 0.0]      # its twin is selected: distance 0, picked last
    m, l = c["mean"].copy(), c["logvar"].copy()
    for g in range(2):
        m[g * 10 + 3] = m[g * 10 + 7] = c["tm"][g]
        l[g * 10 + 3] = l[g * 10 + 7] = c["tl"][g]
    fidx, fit, _ = ps.host_fit(L, m, l, c["tm"], c["tl"], ps.fit_weight(c["valid"], 0), 10)
    assert fidx.tolist() == [3, 3] and fit[:, 3].tolist() == [0.0, 0.0] == fit[:, 7].tolist()


def test_only_the_resampled_part_valid_gives_zero_scores_and_index_zero(L):
    c = ps.make_case(2, 9, 4, seed=5)
    valid = np.zeros((2, 4), np.float32)
    valid[:, 2] = 1
    fidx, fit, n_bad = ps.host_fit(L, c["mean"], c["logvar"], c["tm"], c["tl"], ps.fit_weight(valid, 2), 9)
    assert fidx.tolist() == [0, 0] and not fit.any() and n_bad == 0


def test_a_group_without_a_valid_part_takes_the_first_candidates(L):
    c = ps.make_case(2, 9, 4, seed=6)
    c["valid"][1] = 0
    sc = ps.host_scores(L, c["mean"], c["logvar"], c["valid"], c["stats"], 9)
    idx, dist, n_bad = ps.host_diverse(L, sc, c["valid"], 9, 4)
    assert idx[1].tolist() == [0, 1, 2, 3] and not dist[1].any() and n_bad == 0
    assert np.array_equal(idx[:1], ps.diverse_f64(sc[:9], c["valid"][:1], 9, 4)[0])


def test_non_finite_candidates_are_skipped_and_counted(L):
    G, K, J, P = 2, 12, 4, 5
    c = ps.make_case(G, K, J, seed=9)
    c["valid"][:] = [[1, 1, 1, 1], [1, 0, 1, 1]]
    m, l = c["mean"].copy(), c["logvar"].copy()
    m[0 * K + 0, 1, 2] = np.nan            # group 0: its candidate 0 (the reference's start) and candidate 5
    l[0 * K + 5, 0, 0] = np.inf
    l[1 * K + 4, 2, 3] = -np.inf           # group 1: candidate 4; candidate 6 only on its absent part: finite as far as it is read
    m[1 * K + 6, 0, 1] = np.nan
    sc = ps.host_scores(L, m, l, c["valid"], c["stats"], K)
    idx, _, n_bad = ps.host_diverse(L, sc, c["valid"], K, P)
    assert n_bad == 3 and idx[0, 0] == 1 and idx[1, 0] == 0
    assert not {0, 5} & set(idx[0].tolist()) and 4 not in idx[1].tolist()
    idx64, _, _ = ps.diverse_f64(sc, c["valid"], K, P)
    assert np.array_equal(idx, idx64)
    full, _, n_bad = ps.host_diverse(L, sc, c["valid"], K, K)      # P = K: the non-finite ones come last, lowest index first
    assert n_bad == 3 and full[0, -2:].tolist() == [0, 5] and full[1, -1] == 4
    assert sorted(full[0].tolist()) == list(range(K)) == sorted(full[1].tolist())
    # fit: the target pulls towards the bad candidates; they lose to every finite one
    w = ps.fit_weight(c["valid"], 3)
    tm, tl = c["tm"].copy(), c["tl"].copy()
    fidx, fit, n_bad = ps.host_fit(L, m, l, tm, tl, w, K)
    fidx64, _, _ = ps.fit_f64(m, l, tm, tl, w, K)
    assert n_bad == 2 and np.array_equal(fidx, fidx64) and fidx[0] not in (0, 5)       # group 1's candidate 4 is bad on the zeroed part only
    assert np.isfinite(fit[1]).all() and not np.isfinite(fit[0, [0, 5]]).any()
    allbad = np.full_like(m, np.nan)
    fidx, _, n_bad = ps.host_fit(L, allbad, l, tm, tl, w, K)
    assert fidx.tolist() == [0, 0] and n_bad == G * K
    idx, _, n_bad = ps.host_diverse(L, ps.host_scores(L, allbad, l, c["valid"], c["stats"], K), c["valid"], K, 3)
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and n_bad == G * K


# ---------------------------------------------------------------------------------------------------- the gates reject wrong variants
def test_the_gates_reject_every_wrong_variant(L):
    d = ps.load("diverse_G6_K100_P8")
    K, P = int(d["K"]), int(d["P"])
    st32 = d["stats"].astype(np.float32)
    sc = ps.host_scores(L, d["mean"], d["logvar"], d["valid"], st32, K)
    assert _score_ulps(sc, ps.scores_f64(d["mean"], d["logvar"], d["valid"], st32, K)) <= 1
    # a box over the absent parts too: the groups with an absent part leave the one-ulp gate (and only they)
    bad = ps.scores_f64(d["mean"], d["logvar"], d["valid"], st32, K, variant="box_all").reshape(6, K, 6, 4)
    ulps = [_score_ulps(sc.reshape(6, K, 6, 4)[g], bad[g]) for g in range(6)]
    print("box_all: ulps per group", [f"{u:.3g}" for u in ulps])
    assert ulps[0] <= 1 and ulps[5] <= 1 and all(u > 100 for u in ulps[1:5])
    # biased std: 2 log std moves by log(511 / 512)
    rng = np.random.Generator(np.random.PCG64(3))
    u = rng.standard_normal((K, 512, 3, 4)).astype(np.float32)
    st, st_biased = ps.stats_of(u).astype(np.float32), ps.stats_of(u, biased=True).astype(np.float32)
    own = ps.host_scores(L, d["mean"][:K], d["logvar"][:K], d["valid"][:1], st, K)
    assert _score_ulps(own, ps.scores_f64(d["mean"][:K], d["logvar"][:K], d["valid"][:1], st, K)) <= 1
    assert _score_ulps(own, ps.scores_f64(d["mean"][:K], d["logvar"][:K], d["valid"][:1], st_biased, K)) > 100
    # a distance without / sum(valid): the picks are the same, the recorded distances are not
    idx, dist, _ = ps.host_diverse(L, sc, d["valid"], K, P)
    idx_nd, dist_nd, _ = ps.diverse_f64(sc, d["valid"], K, P, variant="no_div")
    assert np.array_equal(idx, idx_nd) and not np.allclose(dist, dist_nd, rtol=1e-12, atol=0)
    # the resampled part kept in the fit weight: other picks than the reference's
    f = ps.load("fix_S4_E3")
    E, part = int(f["E"]), int(f["part"])
    rep = lambda a: np.repeat(a, E, axis=0)
    m, l = f["cand/mean"].reshape(-1, 3, 4), f["cand/logvar"].reshape(-1, 3, 4)
    kept, _, _ = ps.fit_f64(m, l, rep(f["in/mean"]), rep(f["in/logvar"]), ps.fit_weight(rep(f["in/valid"]), part, variant="part_kept"), K)
    assert not np.array_equal(kept, f["picks"].reshape(-1))
    # ties to the highest index
    c, tsc = _tie_case()
    high, _, _ = ps.diverse_f64(tsc, c["valid"], 10, 10, variant="tie_high")
    low, _, _ = ps.host_diverse(L, tsc, c["valid"], 10, 10)
    assert high[:, 1].tolist() == [7, 7] and not np.array_equal(high, low)
