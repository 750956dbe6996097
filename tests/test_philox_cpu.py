"""The independent statement of the in-kernel random streams (oracle/philox.py), checked without a GPU:

1. ``philox4x32`` against Random123's published known-answer vectors (kat_vectors: three inputs, 10 and 7 rounds);
2. the counter layouts: under one key no two streams of the same round count can meet over their admissible ranges;
3. the statistics of each stream of the statement on large fixed samples.  tests/test_gpu_random_streams.py shows the kernels draw the
   same words, so these figures are the kernels' as well.

Gates are in standard errors: every figure is a z-score (printed, ``PHILOX_STAT`` lines) of a statistic whose null distribution is normal
to a good approximation at these sample sizes, gated at 4.5 (two-sided p = 7e-6; a few hundred figures are tested).  The seeds are fixed, and
a seed is admissible only if the statement itself stays under the gate here: a failure after a change to oracle/philox.py is a finding
about the change.  The Kolmogorov-Smirnov distance is gated at the same tail probability of its own distribution,
sqrt(n) D < sqrt(ln(2 / 6.8e-6) / 2) = 2.51.
"""
import math

import numpy as np
import pytest
import torch

from oracle import philox as ph

GATE = 4.5
KS_GATE = 2.51
U64 = np.uint64


def _report(name, z, gate=GATE):
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    print(f"PHILOX_STAT {name}: n={z.size} max|z|={np.abs(z).max():.2f}  [" + " ".join(f"{v:+.2f}" for v in z.reshape(-1)[:16]) + "]")
    assert np.all(np.abs(z) < gate), (name, z)


# ------------------------------------------------------------------------------------------------ 1. known-answer vectors
PI = ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
ZERO = ((0, 0, 0, 0), (0, 0))
ONES = ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)
KAT = [(10, ZERO, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       (10, ONES, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       (10, PI, (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
       (7, ZERO, (0x5F6FB709, 0x0D893F64, 0x4F121F81, 0x4F730A48)),
       (7, ONES, (0x5207DDC2, 0x45165E59, 0x4D8EE751, 0x8C52F662)),
       (7, PI, (0x4DFCCABA, 0x190A87F0, 0xC47362BA, 0xB6B5242A))]


@pytest.mark.parametrize("rounds,inp,want", KAT, ids=[f"r{r}-{n}" for r in (10, 7) for n in ("zero", "ones", "pi")])
def test_known_answer_vectors(rounds, inp, want):
    got = tuple(int(w) for w in ph.philox4x32(*inp, rounds))
    assert got == want, [hex(w) for w in got]


def test_known_answer_vectors_vectorised():
    """The same six answers from one broadcast call per round count (the array path the streams use)."""
    for rounds in (10, 7):
        rows = [k for k in KAT if k[0] == rounds]
        ctr = [np.array([r[1][0][i] for r in rows], dtype=U64) for i in range(4)]
        key = [np.array([r[1][1][i] for r in rows], dtype=U64) for i in range(2)]
        got = np.stack(ph.philox4x32(ctr, key, rounds), axis=-1)
        assert np.array_equal(got, np.array([r[2] for r in rows], dtype=U64))


def test_round_counts_of_the_streams():
    assert (ph.CHAIN_ROUNDS, ph.BOX_ROUNDS) == (10, 10) and (ph.DROPOUT_ROUNDS, ph.BATCH_ROUNDS, ph.PART_ROUNDS) == (7, 7, 7)


# ------------------------------------------------------------------------------------------------ 2. counter spaces
# Admissible ranges.  Sites: 2 i and 2 i + 1 of block i < DFX_MAX_DEPTH, and the time embedding's 1000.  A dropout site's tensor lives in the
# training workspace: below 2^48 elements (1 PiB of floats, a thousand times the largest device; the layouts first meet at element
# 0xBA7C0 * 2^35 = 2^54.5).  Global point ids and box pairs: below 2^56.  Batch: N <= 8192 values per item (BATCH_MAX_N), C <= 8; part
# sampling: J <= MAX_J = 8 parts, three axes, n_draws <= 2^16; any 64-bit sample_id / row / seed.
MAX_DEPTH, MAX_J, MAX_C, BATCH_MAX_N, MAX_DRAWS, MAX_DROP_ELEMS, MAX_ELEMS = 8, 8, 8, 8192, 1 << 16, 1 << 48, 1 << 56
SITES = list(range(2 * MAX_DEPTH)) + [ph.SITE_TIME_EMBED]
IDS64 = [0, 1, 7, 0xD20F0, 0xBA7C0, 1000, (1 << 32) - 1, 1 << 32, (0xD20F0 << 32) | 5, (0xBA7C1 << 32) | 0x9A570003, (1 << 64) - 1]


def _tuples(words):
    w = np.broadcast_arrays(*[np.asarray(x, dtype=U64) for x in words])
    return {tuple(int(v) for v in row) for row in np.stack([a.reshape(-1) for a in w], axis=-1)}


def _grid(*axes):
    return [g.reshape(-1) for g in np.meshgrid(*[np.array(a, dtype=object) for a in axes], indexing="ij")]


def test_the_abi_constants_the_ranges_come_from():
    from difffacto_amd import _ffi
    assert _ffi.DFX_MAX_DEPTH == MAX_DEPTH


def test_seven_round_counter_spaces_are_disjoint():
    """Dropout (g8 lo, g8 hi, site, 0xD20F0), batch (g, purpose, id lo, id hi), part (g, 0x9A570000 | c * 8 + j, row lo, row hi): word 1 tells
    them apart.  Shown twice: as ranges of word 1 over the admissible ids, and as sets of whole tuples over a grid that includes the ids
    built to meet the other layouts' constants in words 2 and 3."""
    groups = [0, 1, 5, (1 << 32) - 1, 1 << 32, MAX_DROP_ELEMS // 8 - 1]
    g, site = _grid(groups, SITES)
    drop = _tuples(ph.dropout_counter(g, site))
    g, purpose, sid = _grid([0, 1, 5, BATCH_MAX_N // 4 - 1], [ph.DRAW_CHOICE, ph.DRAW_DROP, ph.DRAW_AUG], IDS64)
    batch = _tuples(ph.batch_counter(g, purpose, sid))
    g, c, j, row = _grid([0, 1, 5, MAX_DRAWS // 4 - 1], range(3), range(MAX_J), IDS64)
    part = _tuples(ph.part_counter(g, c, j, row))
    assert len(drop) == len(groups) * len(SITES) and len(batch) == 4 * 3 * len(IDS64) and len(part) == 4 * 3 * MAX_J * len(IDS64)
    assert not (drop & batch) and not (drop & part) and not (batch & part)
    w1_drop_max = max(t[1] for t in drop)
    w1_batch, w1_part = {t[1] for t in batch}, {t[1] for t in part}
    assert w1_drop_max == (MAX_DROP_ELEMS // 8 - 1) >> 32 < min(w1_batch | w1_part)           # dropout: the high half of a group index
    assert w1_batch == {0xBA7C0, 0xBA7C1, 0xBA7C2} and len(w1_part) == 3 * MAX_J        # (axis, part) -> word 1 is one to one
    assert w1_part == {0x9A570000 | v for v in range(3 * MAX_J)} and not (w1_batch & w1_part)
    assert {t[3] for t in drop} == {0xD20F0} and len({t[2] for t in drop}) == len(SITES)  # and the sites differ in word 2


def test_ten_round_counter_spaces_are_disjoint():
    """Chain noise (gid lo, gid hi, t, stream) against the box units (p, 0xB0C50000 | c * 2 + side, pair lo, pair hi): word 1 again — a global
    point id below 2^56 has a high half below 2^24.  The grid holds the tuples that met before the box layout carried its tag: chain
    (gid = p, t = pair, stream 0) against box (p, class 0, side 0, pair)."""
    gid, t, stream = _grid([0, 5, 511, 512, (1 << 32) - 1, 1 << 32, (0xB0C5 << 32) | 7, MAX_ELEMS - 1], [0, 1, 3, 999, 1000], [0, 1])
    chain = _tuples(ph.chain_counter(gid, t, stream))
    p, c, side, pair = _grid([0, 5, ph.BOX_PTS - 1], range(MAX_C), range(2), [0, 1, 3, 999, 1000, 1 << 32, (1 << 33) + 3, (1 << 56) - 1])
    box = _tuples(ph.box_counter(p, c, side, pair))
    assert len(chain) == 8 * 5 * 2 and len(box) == 3 * MAX_C * 2 * 8
    assert not (chain & box)
    assert max(t[1] for t in chain) == (MAX_ELEMS - 1) >> 32 < min(t[1] for t in box)
    assert {t[1] for t in box} == {0xB0C50000 | v for v in range(2 * MAX_C)}
    assert (5, 0, 3, 0) in chain and (5, 0xB0C50000, 3, 0) in box


# ------------------------------------------------------------------------------------------------ 3. statistics of the statement
N24 = 1 << 24
DROP_PAIRS = [(seed, site) for seed in (777, 1 << 32, (1 << 64) - 1, 0xDEADBEEF00000005, 20240607) for site in (0, 9, 1000)]


def _binom_z(k, n, q):
    return (np.asarray(k, dtype=np.float64) - n * q) / math.sqrt(n * q * (1 - q))


def test_dropout_frequency_p02_fifteen_seed_site_pairs():
    thr = ph.dropout_threshold(0.2)
    assert thr == 13107
    z = [_binom_z(int((ph.dropout_draws(seed, site, N24) < thr).sum()), N24, thr / 65536.0) for seed, site in DROP_PAIRS]
    _report("dropout p=0.2 drop frequency, 15 (seed, site) pairs, 2^24 draws each", z)


@pytest.mark.parametrize("p", [0.2, 0.5, 2.0 ** -16, 1 - 2.0 ** -16], ids=["p0.2", "p0.5", "p2^-16", "p1-2^-16"])
def test_dropout_frequency_per_lane_position(p):
    """Each of the eight 16-bit positions of a call on its own (2^21 draws per position).  At the two extreme p a position expects 32
    drops (keeps): the count is Poisson, whose 4.5 sigma tail is heavier than the normal's by a factor the gate still covers (P(X >= 58) < 2e-5)."""
    thr = ph.dropout_threshold(p)
    assert thr == {0.2: 13107, 0.5: 32768, 2.0 ** -16: 1, 1 - 2.0 ** -16: 65535}[p]
    d = ph.dropout_draws(4242, 3, N24).reshape(-1, 8)
    _report(f"dropout p={p:.6g} drop frequency per lane position", _binom_z((d < thr).sum(0), d.shape[0], thr / 65536.0))
    f = ph.dropout_factors(4242, 3, p, 4096)
    assert f.dtype == np.float32 and set(np.unique(f)) <= {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}


def test_dropout_threshold_rounding_and_cap():
    assert [ph.dropout_threshold(p) for p in (1e-5, 2.0 ** -17, 0.99999, 0.999999, 0.5)] == [1, 1, 65535, 65535, 32768]


def test_dropout_draws_chi_square_256_bins():
    d = ph.dropout_draws(99, 1, N24)
    assert int(d.max()) < 65536
    z = []
    for what, v in (("high byte", d >> U64(8)), ("low byte", d & U64(0xFF))):
        cnt = np.bincount(v.astype(np.int64), minlength=256)
        chi2 = float(((cnt - N24 / 256.0) ** 2).sum() / (N24 / 256.0))
        z.append((chi2 - 255.0) / math.sqrt(2 * 255.0))
    _report("dropout 16-bit draws chi^2 over 256 bins (high byte, low byte)", z)


def _corr_z(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()) * math.sqrt(a.size))


def test_dropout_factors_uncorrelated_between_sites_and_seeds():
    thr = ph.dropout_threshold(0.2)
    keep = lambda seed, site: (ph.dropout_draws(seed, site, 1 << 22) >= thr)
    z = [_corr_z(keep(31, 2 * i), keep(31, 2 * i + 1)) for i in (0, 3, 7)]
    z += [_corr_z(keep(s, 4), keep(s + 1, 4)) for s in (31, (1 << 32) - 1, 1 << 63)]
    z += [_corr_z(keep(31, 4)[:-1], keep(31, 4)[1:])]                                     # neighbouring elements of one site
    _report("dropout keep-flag correlation: sites (2i, 2i+1) x3, seeds (s, s+1) x3, lag 1", z)


def _chain_sample(seed=20240521, n_gid=1 << 21, ts=(0, 1, 2), stream=0, gid0=0):
    gid = (np.arange(n_gid, dtype=U64) + U64(gid0))[:, None]
    return ph.chain_normals(seed, gid, np.array(ts, dtype=U64)[None, :], stream)            # (n_gid, len(ts), 3)


@pytest.fixture(scope="module")
def chain_z():
    return _chain_sample()


def test_chain_normals_moments(chain_z):
    z = chain_z.reshape(-1)
    n = z.size
    assert n >= N24
    m = z.mean()
    c = z - m
    v, m3, m4 = (c ** 2).mean(), (c ** 3).mean(), (c ** 4).mean()
    _report("chain normals mean, variance, skew, kurtosis (2^21 gid x 3 t x 3 coordinates)",
            [m * math.sqrt(n), (v - 1) / math.sqrt(2.0 / n), m3 / v ** 1.5 / math.sqrt(6.0 / n), (m4 / v ** 2 - 3) / math.sqrt(24.0 / n)])


def test_chain_normals_kolmogorov_smirnov(chain_z):
    for c in range(3):
        z = np.sort(chain_z[:, :, c].reshape(-1))
        n = z.size
        cdf = torch.special.ndtr(torch.from_numpy(z)).numpy()
        i = np.arange(n, dtype=np.float64)
        D = max(float(((i + 1) / n - cdf).max()), float((cdf - i / n).max()))
        print(f"PHILOX_STAT chain normals coordinate {c}: KS D = {D:.3e}, sqrt(n) D = {math.sqrt(n) * D:.2f} (n = {n})")
        assert math.sqrt(n) * D < KS_GATE, (c, D)


def test_chain_normals_correlations(chain_z):
    z = chain_z
    zz = [_corr_z(z[..., a], z[..., b]) for a, b in ((0, 1), (0, 2), (1, 2))]             # (0, 1) share a radius: uncorrelated all the same
    zz += [_corr_z(z[:-1, :, c], z[1:, :, c]) for c in range(3)]                           # neighbouring gid
    zz += [_corr_z(z[:, 0, c], z[:, 1, c]) for c in range(3)]                              # t and t + 1
    s1 = _chain_sample(n_gid=1 << 20, stream=1)
    zz += [_corr_z(z[:1 << 20, :, c], s1[..., c]) for c in range(3)]                       # stream 0 against stream 1
    zz += [_corr_z(z[..., a] ** 2, z[..., b] ** 2) for a, b in ((0, 2), (1, 2))]           # squares across the two radii
    _report("chain normals correlations: coordinates x3, gid lag 1 x3, t lag 1 x3, stream 0/1 x3, squares x2", zz)


def test_chain_normals_high_words_of_gid_and_seed_matter():
    """Another high half of the seed or of gid, another t, another stream: each gives other words — and uncorrelated normals."""
    base = ph.chain_normals(5, np.arange(1 << 16, dtype=U64), 3, 0)
    others = {"seed hi": ph.chain_normals(5 + (1 << 32), np.arange(1 << 16, dtype=U64), 3, 0),
              "gid hi": ph.chain_normals(5, np.arange(1 << 16, dtype=U64) + U64(1 << 32), 3, 0),
              "t": ph.chain_normals(5, np.arange(1 << 16, dtype=U64), 4, 0),
              "stream": ph.chain_normals(5, np.arange(1 << 16, dtype=U64), 3, 1)}
    _report("chain normals against (seed + 2^32, gid + 2^32, t + 1, stream 1)", [_corr_z(base, o) for o in others.values()])
    assert all(not np.any(base == o) for o in others.values())


def test_part_normals_moments_and_pair_layout():
    z = ph.part_normals(11, 1 << 33, 128, 8, 512)                                          # (128, 512, 3, 8): 2^20 * 1.5 draws
    assert z.shape == (128, 512, 3, 8)
    f = z.reshape(-1)
    n = f.size
    v = f.var()
    _report("part normals mean, variance, kurtosis, even/odd draw correlation",
            [f.mean() * math.sqrt(n), (v - 1) / math.sqrt(2.0 / n), (((f - f.mean()) ** 4).mean() / v ** 2 - 3) / math.sqrt(24.0 / n),
             _corr_z(z[:, 0::2], z[:, 1::2])])
    # draws 2k and 2k+1 share a radius: n0^2 + n1^2 = -2 ln u1 with u1 from word 2k's top 24 bits
    w = ph.part_words(11, 1 << 33, 2, 8, 8)
    r2 = (z[:2, :8][:, 0::2] ** 2 + z[:2, :8][:, 1::2] ** 2)
    assert np.allclose(r2, -2 * np.log(ph.unit24_open(w[:, 0::2])), rtol=1e-12)


@pytest.mark.parametrize("M", [1, 3, 2048, (1 << 20) + 7])
def test_choice_uniformity(M):
    """choice = (w M) >> 32 over 2^24 words (2048 items of 8192 values); expected counts from the exact number of words that map to each bin."""
    ids = np.arange(2048, dtype=np.int64) + (1 << 40)
    offsets = np.array([0, M], dtype=np.int64)
    choice, drop_u, aug_u = ph.batch_draw(offsets, np.zeros(2048, dtype=np.int64), ids, 8192, 8, seed=(7 << 32) | 1)
    assert choice.shape == (2048, 8192) and choice.dtype == np.int32 and choice.min() >= 0 and choice.max() < M
    if M == 1:
        assert not choice.any()
        return
    k = np.arange(M + 1, dtype=object)
    edges = np.array([-((-(int(v) << 32)) // M) for v in k], dtype=np.float64)              # ceil(k 2^32 / M): first word of bin k
    expect = np.diff(edges) / 2.0 ** 32 * choice.size
    cnt = np.bincount(choice.reshape(-1), minlength=M)
    chi2 = float(((cnt - expect) ** 2 / expect).sum())
    _report(f"batch choice chi^2, M = {M}", [(chi2 - (M - 1)) / math.sqrt(2.0 * (M - 1))])
    if M == 2048:   # the unit draws of the same items
        for name, u in (("drop_u", drop_u), ("aug_u", aug_u)):
            assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
            _report(f"batch {name} mean (uniform: variance 1/12)", [(float(u.mean(dtype=np.float64)) - 0.5) * math.sqrt(12.0 * u.size)])


def test_box_units_uniformity():
    u = ph.box_units(3, 1 << 33, 64, 8)                                                      # (64, 8, 2, 512, 3)
    assert u.shape == (64, 8, 2, 512, 3) and u.dtype == np.float32
    cnt = np.bincount((u.reshape(-1).astype(np.float64) * 256).astype(np.int64), minlength=256)
    n = u.size
    chi2 = float(((cnt - n / 256.0) ** 2).sum() / (n / 256.0))
    _report("box units chi^2 over 256 bins, coordinate correlations x3",
            [(chi2 - 255) / math.sqrt(510.0)] + [_corr_z(u[..., a], u[..., b]) for a, b in ((0, 1), (0, 2), (1, 2))])


def test_ranges_of_every_conversion():
    """Unit draws lie in [0, 1) and a normal within sqrt(2 * 25 * ln 2) = 5.887 of zero: at the extreme words, and on the samples."""
    ext = np.array([0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF], dtype=U64)
    assert ph.unit24(ext).tolist() == [0.0, 0.0, 2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24]
    assert ph.unit24_open(ext).tolist() == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, 1 - 2.0 ** -25, 1 - 2.0 ** -25]
    bound = math.sqrt(2 * 25 * math.log(2))
    assert abs(math.sqrt(-2 * math.log(2.0 ** -25)) - bound) < 1e-12
    z = _chain_sample(seed=1, n_gid=1 << 20, ts=(9,))
    pz = ph.part_normals(1, 0, 64, 8, 512)
    print(f"PHILOX_STAT ranges: max |z| chain {np.abs(z).max():.3f}, part {np.abs(pz).max():.3f}, bound {bound:.3f}")
    assert np.abs(z).max() <= bound and np.abs(pz).max() <= bound and np.isfinite(z).all() and np.isfinite(pz).all()
    u = ph.box_units(1, 0, 4, 2)
    assert u.min() >= 0 and u.max() < 1
