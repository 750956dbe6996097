"""CPU checks of selective noise sampling (diverse generation): the new entry points are exported and bound and reject bad arguments
before touching a GPU; the global selection's own routine, compiled for the host (dfx_debug_select_diverse_global_host), against the
float64 restatement of tests/_selective_case.py, on hand-made cases, and against the reference's recorded picks
(tests/golden/selective/, make_golden_selective.py).

Gates.  Picks on the twin's float32 scores: equal to the float64 restatement's on those scores for both rules, pick distances to 1e-12
relative (float64 sums of the same terms; numpy adds them in another order), on inputs whose every finite decision gap is at least
1e-10 (a property of the inputs, asserted).  Picks against the reference: equal; the generator refuses a fixture whose smallest gap
is below 20 x the reference's own float32 deviation.  The last test shows that the comparison rejects four wrong variants."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

import _part_sampling_case as ps
import _selective_case as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfx_select_diverse_global_workspace_bytes", "dfx_select_diverse_global", "dfx_part_search_global",
       "dfx_debug_select_diverse_global_host")
FAKE = ctypes.c_void_p(0x1000)   # a non-null, 16-byte aligned "device pointer": never dereferenced, the checks fail first
FIXTURES = ("global_first_pick_all", "global_first_pick_absent2", "sample_latents_shape_S3", "sample_latents_shape_S3_fixed")


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
    assert L.dfx_version() >= 107 and L.dfx_abi_version() == 5 == _ffi.DFX_ABI_VERSION


def test_fixture_manifest():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import manifest
    want = {}
    for ln in open(os.path.join(sel.GOLDEN, "MANIFEST.sha256")):
        if ln.strip() and not ln.startswith("#"):
            h, name = ln.split()
            want[name] = h
    have = {f: manifest.content_hash(os.path.join(sel.GOLDEN, f)) for f in sorted(os.listdir(sel.GOLDEN)) if f.endswith(".npz")}
    assert want == have and set(have) == {t + ".npz" for t in FIXTURES}
    assert all(os.path.getsize(os.path.join(sel.GOLDEN, f)) < 1 << 20 for f in have)
    for t in FIXTURES:
        d = sel.load(t)
        assert d["min_gap"] >= 20 * d["max_dev"] > 0, t


# ---------------------------------------------------------------------------------------------------- argument checks
def test_global_selection_rejects_bad_arguments_without_a_gpu(L):
    need = L.dfx_select_diverse_global_workspace_bytes
    assert need(0) == 0 and need(1) >= 9 + 6 * 8 * 4 and need(12800) >= 12800 * (9 + 6 * 8 * 4) and need(12800) % 16 == 0

    def call(G=2, K=8, J=4, P=2, rule=0, mean=FAKE, idx=FAKE, scores=FAKE, ws=FAKE, nbytes=None):
        nbytes = need(max(G, 0) * max(K, 0)) if nbytes is None else nbytes
        return _err(L, L.dfx_select_diverse_global(mean, FAKE, FAKE, FAKE, G, K, J, P, rule, idx, scores, FAKE, ws, nbytes, None))
    for kw, msg in [(dict(G=0), "positive"), (dict(K=4097), "K = 4097"), (dict(J=9), "n_class = 9"), (dict(P=0), "P = 0"), (dict(P=17), "P = 17"),
                    (dict(G=65, K=4096), "candidate rows above 262144"), (dict(rule=2), "rule 2"), (dict(rule=-1), "rule -1"),
                    (dict(mean=None), "null"), (dict(idx=None), "null"), (dict(ws=None), "null"), (dict(nbytes=need(16) - 1), "workspace of"),
                    (dict(scores=None, nbytes=0), "workspace of"), (dict(ws=ctypes.c_void_p(0x1008)), "16-byte aligned")]:
        rc, m = call(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)
    # the host twin checks the same shape rules
    z, v, i, d, nb = np.zeros((16, 6, 4), np.float32), np.ones((2, 4), np.float32), np.zeros(20, np.int32), np.zeros(20), np.zeros(1, np.int32)
    for P, rule, msg in ((0, 0, "P = 0"), (17, 0, "P = 17"), (2, 5, "rule 5")):
        rc, m = _err(L, L.dfx_debug_select_diverse_global_host(ps._p(z), ps._p(v), 2, 8, 4, P, rule, ps._p(i), ps._p(d), ps._p(nb)))
        assert rc == -1 and msg in m, (P, rule, m)


def test_global_search_checks_everything_before_the_first_hip_call(L):
    """Against a handle that holds sizes and no device memory: a call that passes every check stops at "holds no weights"."""
    h = ctypes.c_void_p()
    assert L.dfx_debug_latents_stub(ctypes.byref(h), 4, 256, 1, 32) == 0
    G, K, J = 3, 10, 4
    good_a = np.zeros((G, J), np.int32)

    def search(handle=h, S=2, code_a=good_a, G=G, K=K, P=6, rule=0, stats=None, n_draws=512, row0=0, budget=0, idx=FAKE, noise=FAKE):
        a = np.ascontiguousarray(code_a, np.int32)
        return _err(L, L.dfx_part_search_global(handle, FAKE, S, a.ctypes.data_as(ctypes.c_void_p), FAKE, noise, G, K, P, rule, stats, 5, row0,
                                                n_draws, budget, idx, FAKE, FAKE, FAKE, None, FAKE, None))
    bad_a = good_a.copy()
    bad_a[2, 1] = 2
    for kw, msg in [(dict(handle=None), "null handle"), (dict(K=0), "positive"), (dict(K=4097), "K = 4097"), (dict(P=0), "P = 0"),
                    (dict(P=31), "P = 31 outside [1,G K = 30]"), (dict(rule=2), "rule 2"), (dict(code_a=bad_a), "code_a[9] = 2 outside [0,2)"),
                    (dict(budget=9), "row_budget 9"), (dict(n_draws=3), "n_draws = 3"), (dict(row0=-1), "row0 = -1"), (dict(idx=None), "null pointer"),
                    (dict(noise=None), "null pointer"), (dict(S=0), "code_src")]:
        rc, m = search(**kw)
        assert rc == -1 and msg in m, (kw, rc, m)
    for kw in (dict(), dict(P=30, rule=1), dict(stats=FAKE, n_draws=0), dict(budget=10), dict(P=1)):
        rc, m = search(**kw)
        assert rc == -1 and "holds no weights" in m, (kw, rc, m)
    L.dfx_latents_destroy(h)
    h2 = ctypes.c_void_p()
    assert L.dfx_debug_latents_stub(ctypes.byref(h2), 4, 256, 0, 0) == 0
    rc, m = search(handle=h2)
    assert rc == -1 and "without cimle" in m
    L.dfx_latents_destroy(h2)


def test_python_wiring_without_a_gpu():
    from difffacto_amd import part_sampling
    from difffacto_amd.encoders import PartEncoderForTransformerDecoder as Enc
    from test_modules_cpu import ENC_CFG
    enc = Enc(**ENC_CFG)
    with pytest.raises(ValueError, match="bogus"):
        enc.sample_latents(2, 64, "cpu", selective="bogus")
    for flag in ("selective_noise_sampling", "selective_noise_sampling_global"):
        with pytest.raises(NotImplementedError, match="selective='global'"):
            Enc(**{**ENC_CFG, flag: True})
    for aligner in (None, types.SimpleNamespace(cimle=False)):
        with pytest.raises(NotImplementedError, match="cIMLE"):
            Enc.sample_latents.__wrapped__(types.SimpleNamespace(part_aligner=aligner), 2, 64, "cpu", selective="shape")
    assert part_sampling.rule_id("farthest") == 0 and part_sampling.rule_id("first_pick") == 1
    with pytest.raises(ValueError, match="nearest"):
        part_sampling.rule_id("nearest")


# ---------------------------------------------------------------------------------------------------- float64 restatement
@pytest.fixture(scope="module")
def cases(L):
    """(G, K, J, P, seed) -> (twin scores, valid): computed once, shared, never modified."""
    out = {}
    for G, K, J, P in sel.SHAPES:
        for seed in sel.SEEDS:
            c = ps.make_case(G, K, J, seed)
            out[G, K, J, P, seed] = (ps.host_scores(L, c["mean"], c["logvar"], c["valid"], c["stats"], K), c["valid"])
    return out


@pytest.mark.parametrize("G,K,J,P", sel.SHAPES)
def test_picks_follow_the_float64_restatement(L, cases, G, K, J, P):
    for seed in sel.SEEDS:
        sc, valid = cases[G, K, J, P, seed]
        for rule in sel.RULES:
            idx64, dist64, gap = sel.diverse_global_f64(sc, valid, K, P, rule)
            fin = gap[np.isfinite(gap)]
            print(f"G {G} K {K} J {J} P {P} seed {seed} {rule}: smallest finite gap {fin.min() if len(fin) else float('inf'):.3g}")
            assert (fin >= 1e-10).all()
            idx, dist, n_bad = sel.host_diverse_global(L, sc, valid, K, P, rule)
            assert n_bad == 0 and np.array_equal(idx, idx64), (seed, rule)
            assert sel.same_dist(dist, dist64), (seed, rule)
            assert len(set(idx.tolist())) == P and dist[0] == 0


# ---------------------------------------------------------------------------------------------------- hand-made cases
@pytest.mark.parametrize("rule", list(sel.RULES))
def test_of_two_identical_rows_the_lower_index_wins_and_neither_is_picked_twice(L, rule):
    sc, valid, K = sel.twins_case()
    idx, dist, n_bad = sel.host_diverse_global(L, sc, valid, K, 12, rule)
    assert idx[:2].tolist() == [0, 3] and sorted(idx.tolist()) == list(range(12)) and n_bad == 0
    if rule == "farthest":                                   # its twin is selected: distance 0, picked last
        assert idx[-1] == 9 and dist[-1] == 0.0
    else:                                                    # equally far from pick 0: right after it, the lower index first
        assert idx[2] == 9 and dist[2] == dist[1]
    assert np.array_equal(idx, sel.diverse_global_f64(sc, valid, K, 12, rule)[0])


@pytest.mark.parametrize("rule", list(sel.RULES))
def test_a_row_without_a_common_part_is_picked_right_after_pick_zero(L, rule):
    sc, valid, K = sel.disjoint_case()
    idx, dist, n_bad = sel.host_diverse_global(L, sc, valid, K, 12, rule)
    idx64, dist64, _ = sel.diverse_global_f64(sc, valid, K, 12, rule)
    assert idx[:2].tolist() == [0, 4] and dist[0] == 0 and np.isposinf(dist[1]) and n_bad == 0
    # farthest: the middle group's other rows now have a pick to be compared with; first pick: they never do and all come next
    assert np.isinf(dist).sum() == (1 if rule == "farthest" else 4)
    assert np.array_equal(idx, idx64) and sel.same_dist(dist, dist64) and sorted(idx.tolist()) == list(range(12))


@pytest.mark.parametrize("rule", list(sel.RULES))
def test_non_finite_rows_come_last_in_index_order_and_are_counted(L, rule):
    sc, valid, K = sel.bad_rows_case()
    for P in (5, 12):                                        # P = R: every row, once
        idx, dist, n_bad = sel.host_diverse_global(L, sc, valid, K, P, rule)
        assert n_bad == 5 and np.array_equal(idx, sel.diverse_global_f64(sc, valid, K, P, rule)[0])
        assert not {2, 8, 9, 10, 11} & set(idx[:min(P, 7)].tolist()) and 1 in idx[:7].tolist() + [1] * (P < 7)
    assert idx[7:].tolist() == [2, 8, 9, 10, 11] and not dist[7:].any() and sorted(idx.tolist()) == list(range(12))
    allbad = np.full_like(sc, np.nan)
    idx, dist, n_bad = sel.host_diverse_global(L, allbad, valid, K, 3, rule)
    assert idx.tolist() == [0, 1, 2] and n_bad == 12 and not dist.any()


# ---------------------------------------------------------------------------------------------------- the reference's recorded picks
@pytest.mark.parametrize("name", ["global_first_pick_all", "global_first_pick_absent2"])
def test_first_pick_rule_returns_the_reference_ids(L, name):
    d = sel.load(name)
    K, P = int(d["K"]), int(d["P"])
    sc = ps.host_scores(L, d["mean"], d["logvar"], d["valid"], d["stats"].astype(np.float32), K)
    idx, dist, n_bad = sel.host_diverse_global(L, sc, d["valid"], K, P, "first_pick")
    print(f"{name}: fixture gap {float(d['min_gap']):.3g}, float32 deviation {float(d['max_dev']):.3g}")
    assert n_bad == 0 and np.array_equal(idx, d["ids"])
    assert np.array_equal(d["mean"][idx], d["sel_mean"]) and np.array_equal(d["logvar"][idx], d["sel_logvar"])
    # what the reference picks is the distance-to-row-0 order, not farthest-point selection
    order = np.argsort(-sel.dist_to(sc.astype(np.float64), sel.row_masks(d["valid"], K), 0), kind="stable")
    assert np.array_equal(idx[1:], order[order != 0][:P - 1])
    far, _, _ = sel.host_diverse_global(L, sc, d["valid"], K, P, "farthest")
    assert far[0] == 0 and far[1] == idx[1] and not np.array_equal(far, idx)


@pytest.mark.parametrize("name", ["sample_latents_shape_S3", "sample_latents_shape_S3_fixed"])
def test_per_shape_picks_equal_the_reference(L, name):
    d = sel.load(name)
    K, keep = int(d["K"]), int(d["keep"])
    valid, fixed = d["in/valid"], d["in/fixed_id"].astype(np.float32)
    merged = valid * (1 - fixed) + fixed * np.clip(valid[:1] + fixed, 0, 1)
    sc = ps.host_scores(L, d["cand/mean"], d["cand/logvar"], merged, d["stats"].astype(np.float32), K)
    idx, _, n_bad = ps.host_diverse(L, sc, merged, K, keep)
    assert n_bad == 0 and np.array_equal(idx, d["ids"])
    rows = (np.arange(valid.shape[0])[:, None] * K + idx).reshape(-1)
    assert np.array_equal(d["cand/mean"][rows], d["out/means"]) and np.array_equal(d["cand/logvar"][rows], d["out/logvars"])
    assert np.array_equal(d["out/valid"], np.repeat(merged, keep, 0))


# ---------------------------------------------------------------------------------------------------- the gates reject wrong variants
def test_the_comparison_rejects_every_wrong_variant(L, cases):
    def agrees(key, rule, variant=None, as_rule=None):
        sc, valid = cases[key]
        G, K, J, P, _ = key
        idx, dist, _ = sel.host_diverse_global(L, sc, valid, K, P, rule)
        idx64, dist64, _ = sel.diverse_global_f64(sc, valid, K, P, as_rule or rule, variant)
        return np.array_equal(idx, idx64) and sel.same_dist(dist, dist64)
    mixed, shared = (7, 37, 5, 40, 1), (1, 257, 8, 9, 1)          # groups with different masks / one group
    assert agrees(mixed, "farthest") and agrees(shared, "farthest")
    assert not agrees(mixed, "farthest", "own_mask") and agrees(shared, "farthest", "own_mask")      # wrong only where masks differ
    assert not agrees(mixed, "farthest", "no_div") and not agrees(shared, "farthest", "no_div")
    assert not agrees(mixed, "farthest", as_rule="first_pick") and not agrees(shared, "farthest", as_rule="first_pick")
    sc, valid, K = sel.twins_case()
    low, _, _ = sel.host_diverse_global(L, sc, valid, K, 12, "first_pick")
    high, _, _ = sel.diverse_global_f64(sc, valid, K, 12, "first_pick", "tie_high")
    assert low[1:3].tolist() == [3, 9] and high[1:3].tolist() == [9, 3]
