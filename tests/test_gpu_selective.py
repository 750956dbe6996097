"""GPU checks of selective noise sampling (diverse generation): dfx_select_diverse_global (csrc/part_sampling.hip),
dfx_part_search_global (latents_kernels.hip), LatentSampler.sample_latents_selective and the ``selective`` keyword of
PartEncoderForTransformerDecoder.sample_latents / encoders.generate.

* the device selection against the host twin on the device's own scores: equal picks at every shape of tests/_selective_case.py, at
  the last size one workgroup runs (R = 512) and the first that takes one launch per pick, with the launches forced at every size
  as well, for both rules, with and without the scores output, and on the
  hand-made cases (identical rows, masks without a common part, non-finite rows, P = R);
* the global search against the composition "dfx_part_aligner on all rows, dfx_select_diverse_global, indexing": bit for bit under
  dfx_debug_lin_split_k(1), the same bits for every row budget;
* the reference's fixtures end to end (tests/golden/selective/): picks equal, tensors within test_gpu_part_sampling.LATENT_TOL;
* generate(selective='global'): row count, consistency with the source rows, reproducibility, and selective=None unchanged;
  AnchorDiffAE.sample and the gen branch of AnchorDiffAE.forward pass the keyword through."""
import numpy as np
import pytest
import torch

import _part_sampling_case as ps
import _selective_case as sel
from _replay import replay_draws
from test_gpu_part_sampling import LATENT_TOL, _close, cu, host
from difffacto_amd import synth

pytestmark = pytest.mark.gpu


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


def _select_without_scores(mean, logvar, valid, stats, K, P, rule):
    """dfx_select_diverse_global with scores = NULL: they live in the workspace."""
    from difffacto_amd import _ffi
    G, J = valid.shape
    idx = torch.empty(P, dtype=torch.int32, device="cuda")
    n_bad = torch.empty(1, dtype=torch.int32, device="cuda")
    nbytes = _ffi.lib().dfx_select_diverse_global_workspace_bytes(G * K)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    rc = _ffi.lib().dfx_select_diverse_global(_ffi.ptr(mean), _ffi.ptr(logvar), _ffi.ptr(valid), _ffi.ptr(stats), G, K, J, P, sel.RULES[rule],
                                              _ffi.ptr(idx), None, _ffi.ptr(n_bad), (ws.data_ptr() + 15) & ~15, nbytes, _ffi.current_stream())
    _ffi.check(rc, "dfx_select_diverse_global")
    return idx, n_bad


def _device_equals_twin(L, c, K, P):
    """Both rules, with and without the scores output, on the automatic choice between the selection's two launch paths (one workgroup
    for the whole call up to 512 rows, one launch per pick above) and with one launch per pick forced."""
    from difffacto_amd import part_sampling as psm
    dev = [cu(c[k]) for k in ("mean", "logvar", "valid", "stats")]
    out = {}
    try:
        for path in (1, -1):
            L.dfx_debug_diverse_global_path(path)
            for rule in sel.RULES:
                d = psm.select_diverse_global(dev[0], dev[1], dev[2], K, P, rule=rule, stats=dev[3])
                sc = host(d["scores"])
                idx, dist, n_bad = sel.host_diverse_global(L, sc, c["valid"], K, P, rule)
                assert np.array_equal(host(d["idx"]), idx) and int(d["n_bad"]) == n_bad, (path, rule, host(d["idx"]), idx)
                idx_ws, n_bad_ws = _select_without_scores(*dev, K, P, rule)
                assert np.array_equal(host(idx_ws), idx) and int(n_bad_ws) == n_bad, (path, rule)
                out[rule] = (idx, dist, n_bad, sc)
    finally:
        L.dfx_debug_diverse_global_path(-1)
    return out


# three more shapes than the CPU test: 512 and 513 rows, on either side of the automatic choice between the two launch paths, and
# 70 000 rows, more than the 256 x 256 threads of one launch (two rows per thread)
@pytest.mark.parametrize("G,K,J,P", sel.SHAPES + [(1, 512, 4, 7), (1, 513, 4, 7), (20, 3500, 1, 5)])
def test_device_selection_equals_the_host_twin(L, G, K, J, P):
    c = ps.make_case(G, K, J, seed=1, n_draws=8 if G * K > 4000 else 64)
    got = _device_equals_twin(L, c, K, P)
    want = ps.host_scores(L, c["mean"], c["logvar"], c["valid"], c["stats"], K)      # the host's exp / log can differ in the last bit
    assert float((np.abs(got["farthest"][3].astype(np.float64) - want) / ps.ulp32(want.astype(np.float64))).max()) <= 1.0
    assert got["farthest"][2] == 0 and len(set(got["farthest"][0].tolist())) == P


def test_device_selection_on_the_hand_made_cases(L):
    # two identical rows, one mask: the lower index first, neither twice
    c = ps.make_case(2, 6, 4, seed=5)
    c["valid"][:] = 1
    for k in ("mean", "logvar", "stats"):
        c[k][9] = c[k][3]
    got = _device_equals_twin(L, c, 6, 12)
    for rule, (idx, dist, n_bad, sc) in got.items():
        assert np.array_equal(sc[3], sc[9]) and sorted(idx.tolist()) == list(range(12)) and n_bad == 0
        assert idx.tolist().index(3) < idx.tolist().index(9)
    assert got["farthest"][0][-1] == 9 and got["farthest"][1][-1] == 0.0
    # masks {0,1}, {2,3}, {0,1}: the first row without a common part with pick 0 comes right after it
    c = ps.make_case(3, 4, 4, seed=6)
    c["valid"][:] = [[1, 1, 0, 0], [0, 0, 1, 1], [1, 1, 0, 0]]
    for rule, (idx, dist, n_bad, _) in _device_equals_twin(L, c, 4, 12).items():
        assert idx[:2].tolist() == [0, 4] and np.isposinf(dist[1]) and n_bad == 0 and sorted(idx.tolist()) == list(range(12))
    # a NaN on a valid part, a NaN on an absent part only, a group without a valid part; P = R
    c = ps.make_case(3, 4, 4, seed=7)
    c["valid"][:] = [[1, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]]
    c["mean"][2, 1, 2] = np.nan
    c["mean"][1, 0, 1] = np.nan
    for rule, (idx, dist, n_bad, _) in _device_equals_twin(L, c, 4, 12).items():
        assert n_bad == 5 and idx[7:].tolist() == [2, 8, 9, 10, 11] and sorted(idx[:7].tolist()) == [0, 1, 3, 4, 5, 6, 7]


# ---------------------------------------------------------------------------------------------------- search
def test_global_search_equals_the_composition_bit_for_bit_with_one_k_grouping(L, sampler, one_grouping):
    from difffacto_amd import part_sampling as psm
    S, K, J, P = 4, 100, 4, 40
    rng = np.random.Generator(np.random.PCG64(31))
    codes = rng.standard_normal((S, 256, J)).astype(np.float32)
    valid = np.ones((S, J), np.float32)
    valid[1, 2] = valid[3, 0] = 0
    noise = rng.standard_normal((S * K, 32)).astype(np.float32)
    stats = ps.make_case(S, K, J, seed=3, n_draws=512)["stats"]
    code_a = np.repeat(np.arange(S, dtype=np.int32)[:, None], J, 1)
    mean, logvar = sampler.part_aligner(cu(np.repeat(codes, K, axis=0)), cu(np.repeat(valid, K, axis=0)), cu(noise))
    for rule in sel.RULES:
        want = psm.select_diverse_global(mean, logvar, cu(valid), K, P, rule=rule, stats=cu(stats))
        idx = host(want["idx"]).astype(np.int64)
        twin, _, _ = sel.host_diverse_global(L, host(want["scores"]), valid, K, P, rule)
        assert np.array_equal(idx, twin) and len(set((idx // K).tolist())) > 1
        outs = [sampler.part_search_global(cu(codes), code_a, cu(valid), cu(noise), K, P, rule=rule, stats=cu(stats), row_budget=budget,
                                           return_scores=True) for budget in (K, 3 * K, 0)]          # chunks of 1, of 3 + 1 and of all 4 shapes
        for o in outs:
            assert np.array_equal(host(o["idx"]), idx) and int(o["n_bad"]) == 0
            assert torch.equal(o["scores"], want["scores"])
            assert np.array_equal(host(o["mean"]), host(mean)[idx]) and np.array_equal(host(o["logvar"]), host(logvar)[idx])
            assert np.array_equal(host(o["noise"]), noise[idx])
        no_scores = sampler.part_search_global(cu(codes), code_a, cu(valid), cu(noise), K, P, rule=rule, stats=cu(stats), row_budget=2 * K)
        assert no_scores["scores"] is None and torch.equal(no_scores["idx"], outs[0]["idx"]) and torch.equal(no_scores["mean"], outs[0]["mean"])
    # NULL stats: the search draws each chunk's statistics itself, the numbers of dfx_part_draw_stats at the global rows
    own = sampler.part_search_global(cu(codes), code_a, cu(valid), cu(noise), K, P, seed=9, row0=70, row_budget=3 * K, return_scores=True)
    given = sampler.part_search_global(cu(codes), code_a, cu(valid), cu(noise), K, P, stats=psm.draw_stats(S * K, J, seed=9, row0=70),
                                       return_scores=True)
    assert torch.equal(own["scores"], given["scores"]) and torch.equal(own["idx"], given["idx"]) and torch.equal(own["mean"], given["mean"])


# ---------------------------------------------------------------------------------------------------- the reference's fixtures
def _encoder(N):
    from test_gpu_edit import _model
    return _model(10, N, 1, "f32").encoder


@pytest.mark.parametrize("name", ["sample_latents_shape_S3", "sample_latents_shape_S3_fixed"])
def test_per_shape_fixture_end_to_end(name):
    d = sel.load(name)
    K, keep, N = int(d["K"]), int(d["keep"]), int(d["N"])
    S = d["in/valid"].shape[0]
    enc = _encoder(N)
    fixed = torch.from_numpy(d["in/fixed_id"].astype(np.float32)).cuda()
    with replay_draws([d["draw_0"], d["draw_1"]]) as queue:
        ctx, mpp, lpp, seg, valid, (codes, means, logvars, noise), kept = enc.sample_latents(
            S, N, "cuda", fixed_id=fixed, valid_id=cu(d["in/valid"]), epoch=0, selective="shape", selective_stats=cu(d["stats"].astype(np.float32)),
            return_selection=True)
    assert not queue
    picks = host(kept["idx"])
    assert picks.shape == (S, keep) and np.array_equal(picks, d["ids"]), (picks, d["ids"])
    assert np.array_equal(host(kept["source_row"]), np.repeat(np.arange(S), keep)) and int(kept["n_bad"]) == 0
    # the returned noise holds the selected rows (with a fixed part: of shape 0's noises)
    z = d["draw_1"].reshape(S, K, -1)
    z = np.stack([z[0 if d["in/fixed_id"].any() else s][picks[s]] for s in range(S)]).reshape(S * keep, -1)
    assert np.array_equal(host(noise), z)
    assert seg.dtype == torch.int32 and np.array_equal(host(seg), d["out/seg"]) and np.array_equal(host(valid), d["out/valid"])
    for k, got in (("codes", codes), ("means", means), ("logvars", logvars), ("mean_per_point", mpp), ("logvar_per_point", lpp), ("ctx0", ctx[0]),
                   ("ctx1", ctx[1])):
        print(f"{name} {k}: {_close(got, d['out/' + k], LATENT_TOL, k):.2e} (gate {LATENT_TOL})")


@pytest.mark.parametrize("name", ["global_first_pick_all", "global_first_pick_absent2"])
def test_global_fixture_end_to_end(sampler, name):
    d = sel.load(name)
    K, P = int(d["K"]), int(d["P"])
    S = d["valid"].shape[0]
    out = sampler.sample_latents_selective(None, cu(d["noise"]), cu(d["valid"]), "global", K=K, keep=P // S, rule="first_pick", npoints=64,
                                           part_code=cu(d["codes"]), stats=cu(d["stats"].astype(np.float32)))
    idx = host(out["idx"])
    assert np.array_equal(idx, d["ids"]), (idx, d["ids"])
    assert np.array_equal(host(out["source_row"]), d["ids"] // K) and int(out["n_bad"]) == 0
    assert np.array_equal(host(out["noise"]), d["noise"][d["ids"]]) and np.array_equal(host(out["valid_id"]), d["valid"][d["ids"] // K])
    _close(out["mean"], d["sel_mean"], LATENT_TOL, "mean")
    _close(out["logvar"], d["sel_logvar"], LATENT_TOL, "logvar")
    _close(out["part_code"], d["codes"][d["ids"] // K], 0.0, "part_code")
    far = sampler.sample_latents_selective(None, cu(d["noise"]), cu(d["valid"]), "global", K=K, keep=P // S, npoints=64, part_code=cu(d["codes"]),
                                           stats=cu(d["stats"].astype(np.float32)))
    assert not np.array_equal(host(far["idx"]), idx) and len(set(host(far["idx"]).tolist())) == P


# ---------------------------------------------------------------------------------------------------- generate
def test_generate_with_global_selection():
    from test_gpu_edit import _model
    from difffacto_amd import encoders
    S, N, keep = 3, 64, 10
    m = _model(10, N, 1, "f32")
    valid = torch.ones(S, 4, device="cuda")
    valid[1, 2] = 0

    def run(**kw):
        torch.manual_seed(5)
        return encoders.generate(m.encoder, m.diffusion, S, N, valid_id=valid, seed=17, **kw)
    a = run(selective="global", K=100, selective_keep=keep)
    src = host(a["source_row"])
    assert a["pred"].shape == (S * keep, N, 3) and src.shape == (S * keep,) and set(src.tolist()) <= set(range(S))
    assert np.array_equal(src, host(a["selected"]) // 100) and len(set(host(a["selected"]).tolist())) == S * keep
    v = host(valid)[src]
    assert np.array_equal(host(a["present"]), v)
    ids = np.arange(4)[None] * v + np.argmax(v, 1)[:, None] * (1 - v)
    assert np.array_equal(host(a["pred_seg_mask"]), np.repeat(ids.astype(np.int32), N // 4, axis=1))
    anchors = host(a["anchors"]).reshape(S * keep, 4, N // 4, 3)                       # one anchor per part: constant over its points
    assert np.array_equal(anchors, np.repeat(anchors[:, :, :1], N // 4, axis=2)) and np.isfinite(host(a["pred"])).all()
    absent = anchors[src == 1]
    assert np.array_equal(absent[:, 2], absent[:, 0])                                  # the absent part's points go to the first valid part
    b = run(selective="global", K=100, selective_keep=keep)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    shape = run(selective="shape", selective_keep=4)                                   # K defaults to 100
    assert shape["pred"].shape == (S * 4, N, 3) and np.array_equal(host(shape["source_row"]), np.repeat(np.arange(S), 4))
    assert tuple(shape["selected"].shape) == (S, 4) and int(shape["selected"].max()) >= 10
    # selective=None: the call as it was, 10 rows per shape, the same bits as the explicit front end + chain
    plain, plain10 = run(), run(K=10)
    assert plain["pred"].shape == (S * 10, N, 3) and "source_row" not in plain and all(torch.equal(plain[k], plain10[k]) for k in plain if torch.is_tensor(plain[k]))
    torch.manual_seed(5)
    ctx, mpp, lpp, seg, val, _ = m.encoder.sample_latents(S, N, "cuda", valid_id=valid, K=10)
    want = encoders.decode(m.diffusion, ctx, seg, valid_id=val, seed=17)
    assert torch.equal(plain["pred"], want["pred"]) and torch.equal(plain["anchors"], mpp.transpose(1, 2))
    with pytest.raises(ValueError, match="bogus"):
        run(selective="bogus")


def test_network_mirror_passes_the_keyword_through():
    """AnchorDiffAE.sample and the gen branch of AnchorDiffAE.forward.  'shape': selective_keep samples per shape instead of
    cimle_sample_num, folded by shape.  'global': rows in pick order, nothing folded; with different masks in the batch every row's
    present, segmentation and anchors are those of its source shape."""
    import os
    from _replay import load_forward_fixture
    from test_gpu_forward import GOLDEN, _model
    batch, _, _, meta = load_forward_fixture(os.path.join(GOLDEN, "forward_gen_B2_K2_T10.npz"))
    B, N, _ = batch["ref"].shape
    model = _model(int(meta["T"]), N, int(meta["K"]), gen=True, precision="f32", ret_interval=int(meta["ret_interval"]))
    batch["present"] = torch.tensor([[1., 1., 1., 1.], [1., 0., 1., 1.]])
    valid, keep = batch["present"].cuda(), 3
    torch.manual_seed(3)
    out = model.sample(B, [0, 0, 0, 0], valid, "cuda", 0, selective="shape", selective_keep=keep, seed=4, return_selection=True)
    ctx, mpp, lpp, seg, val, (codes, means, logvars, noise), kept = out
    assert tuple(ctx[0].shape) == (B * keep, 256, 4) == tuple(codes.shape) and tuple(noise.shape) == (B * keep, 32) and tuple(mpp.shape) == (B * keep, 3, N)
    assert torch.equal(val, valid.repeat_interleave(keep, 0)) and tuple(kept["idx"].shape) == (B, keep)
    assert len(model.sample(B, [0, 0, 0, 0], valid, "cuda", 0)) == 6

    def seg_of(v):
        ids = np.arange(4)[None] * v + np.argmax(v, 1)[:, None] * (1 - v)
        return np.repeat(ids.astype(np.int32), N // 4, axis=1)
    torch.manual_seed(3)
    (pred, name), = model(batch, device="cuda", epoch=0, selective="shape", selective_keep=keep, seed=4)
    assert name.startswith("gen_fixed") and {f"pred_sample {i}" for i in range(keep)} <= set(pred) and f"pred_sample {keep}" not in pred
    assert tuple(pred["pred"].shape) == (B, N, 3) and bool(torch.isfinite(pred[f"pred_sample {keep - 1}"]).all())
    assert torch.equal(pred["present"], batch["present"]) and pred["source_row"].tolist() == [0] * keep + [1] * keep
    assert np.array_equal(host(pred["pred_seg_mask"]), seg_of(host(batch["present"])))
    torch.manual_seed(3)
    (pred, name), = model(batch, device="cuda", epoch=0, selective="global", selective_keep=keep, seed=4)
    src = host(pred["source_row"])
    assert src.shape == (B * keep,) and np.array_equal(src, host(pred["selected"]) // 100) and "pred_sample 0" not in pred
    assert tuple(pred["pred"].shape) == (B * keep, N, 3) == tuple(pred["sample prior"].shape) and bool(torch.isfinite(pred["pred"]).all())
    assert tuple(pred["input"].shape)[0] == B                                          # the batch's own entries stay per shape
    v = host(batch["present"])[src]
    assert np.array_equal(host(pred["present"]), v) and np.array_equal(host(pred["pred_seg_mask"]), seg_of(v))
    anchors = host(pred["anchors"]).reshape(B * keep, 4, N // 4, 3)
    assert np.array_equal(anchors, np.repeat(anchors[:, :, :1], N // 4, axis=2))
    absent = anchors[src == 1]
    assert len(absent) and np.array_equal(absent[:, 1], absent[:, 0]) and not np.array_equal(anchors[src == 0][:, 1], anchors[src == 0][:, 0])
    with pytest.raises(ValueError, match="bogus"):
        model(batch, device="cuda", epoch=0, selective="bogus")
