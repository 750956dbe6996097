"""Independent numpy statement of every in-kernel random stream (ORACLE — test only, no GPU).

Written from Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3" (SC'11) and from the contracts the headers
state (include/dfx.h, include/dfx_debug.h, the comment blocks of dfx_dropout.h, batch_kernels.hip, part_sampling.hip, part_metrics.hip
and denoiser_kernel.hip; DESIGN.md "Random streams" is the table).  tests/test_philox_cpu.py holds ``philox4x32`` to Random123's
known-answer vectors and this statement's streams to their statistics; tests/test_gpu_random_streams.py holds the kernels to this
statement, word for word where the stream is integer or a plain float conversion, and in units of z where it is a normal.

Philox4x32-R (SC'11, section 3.3 and table 2): a counter of four and a key of two 32-bit words; one round is

    (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),      M0 = 0xD2511F53, M1 = 0xCD9E8D57

and the key is bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.

Every stream's key is its 64-bit seed, low word first.  A 64-bit id takes two counter words, low word first.  The layouts:

    stream          rounds  counter word 0        word 1                         word 2          word 3
    chain noise     10      gid lo                gid hi                         t               stream (0 = step noise, 1 = start draw)
    box units       10      point p < 512         0xB0C50000 | class * 2 + side  pair lo         pair hi
    dropout          7      g8 lo                 g8 hi                          site            0xD20F0
    batch draws      7      group of four g       0xBA7C0 / 0xBA7C1 / 0xBA7C2    sample_id lo    sample_id hi
    part normals     7      group of four g       0x9A570000 | axis * 8 + part   row lo          row hi
"""
import numpy as np

U64 = np.uint64
MASK32 = U64(0xFFFFFFFF)
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
WEYL0, WEYL1 = 0x9E3779B9, 0xBB67AE85

CHAIN_ROUNDS = BOX_ROUNDS = 10
DROPOUT_ROUNDS = BATCH_ROUNDS = PART_ROUNDS = 7          # "Philox4x32-7": the smallest variant SC'11 reports as Crush-resistant

STREAM_STEP, STREAM_START = 0, 1                         # chain noise, counter word 3
DROPOUT_TAG = 0xD20F0                                    # dropout, counter word 3
DRAW_CHOICE, DRAW_DROP, DRAW_AUG = 0xBA7C0, 0xBA7C1, 0xBA7C2   # batch draws, counter word 1
DRAW_PART = 0x9A570000                                   # part normals, counter word 1 (| axis * 8 + part)
DRAW_BOX = 0xB0C50000                                    # box units, counter word 1 (| class * 2 + side)
BOX_PTS = 512                                            # points drawn per box
SITE_TIME_EMBED = 1000                                   # dropout sites: 2 i / 2 i + 1 of block i, and this one


def _u64(a):
    """Integers (Python ints up to 2^64 - 1, negative int64 as their two's complement) -> uint64 array."""
    a = np.asarray(a)
    if a.dtype == object:
        a = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in a.reshape(-1)], dtype=U64).reshape(a.shape)
    return a.astype(U64)


def split64(v):
    """(low word, high word) of a 64-bit value."""
    v = _u64(v)
    return v & MASK32, v >> U64(32)


def philox4x32(counter4, key2, rounds):
    """Philox4x32-``rounds``.  ``counter4``: four broadcastable integer arrays (each word < 2^32), ``key2``: two.  Returns four uint64 arrays
    holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) for c in counter4])
    k0, k1 = (_u64(k) for k in key2)
    for _ in range(int(rounds)):
        p0, p1 = M0 * c0, M1 * c2                        # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + U64(WEYL0)) & MASK32, (k1 + U64(WEYL1)) & MASK32
    return c0, c1, c2, c3


# ---- counter layouts (tests/test_philox_cpu.py: the spaces under one key are disjoint) ----
def chain_counter(gid, t, stream):
    lo, hi = split64(gid)
    return lo, hi, _u64(t), _u64(stream)


def box_counter(p, c, side, pair):
    lo, hi = split64(pair)
    return _u64(p), U64(DRAW_BOX) | (_u64(c) * U64(2) + _u64(side)), lo, hi


def dropout_counter(g8, site):
    lo, hi = split64(g8)
    return lo, hi, _u64(site) & MASK32, U64(DROPOUT_TAG)


def batch_counter(g, purpose, sample_id):
    lo, hi = split64(sample_id)
    return _u64(g), _u64(purpose), lo, hi


def part_counter(g, c, j, row):
    lo, hi = split64(row)
    return _u64(g), U64(DRAW_PART) | (_u64(c) * U64(8) + _u64(j)), lo, hi


# ---- conversions ----
def unit24(w):
    """[0, 1) from the top 24 bits of a word: exact in float32."""
    return ((w >> U64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def unit24_open(w):
    """(0, 1) from the top 24 bits of a word, float64: the Box-Muller radius never sees 0."""
    return ((w >> U64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


# ---- chain noise ----
def chain_gid(shape_offset, B, N):
    """(B, N') global point ids of a launch: (shape_offset + b) N' + n with N' = N rounded up to a multiple of 32 — the engine pads a cloud to
    whole wavefronts before the launch, and the padded count is the one the kernels see."""
    Np = -(-int(N) // 32) * 32
    b = np.array([int(shape_offset) + i for i in range(int(B))], dtype=object)[:, None]
    return _u64(b * Np + np.arange(Np, dtype=object)[None, :])


def chain_words(seed, gid, t, stream):
    return philox4x32(chain_counter(gid, t, stream), split64(seed), CHAIN_ROUNDS)


def chain_normals(seed, gid, t, stream):
    """(..., 3) float64: Box-Muller on the 24-bit uniforms u_i = ((w_i >> 8) + 0.5) 2^-24 of the four words,
    (r(u0) cos 2 pi u1, r(u0) sin 2 pi u1, r(u2) cos 2 pi u3), r(u) = sqrt(-2 ln u)."""
    u0, u1, u2, u3 = (unit24_open(w) for w in chain_words(seed, gid, t, stream))
    ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    return np.stack([ra * np.cos(2 * np.pi * u1), ra * np.sin(2 * np.pi * u1), rb * np.cos(2 * np.pi * u3)], axis=-1)


# ---- dropout ----
def dropout_threshold(p):
    """round(p 2^16) of the float32 p (half up), capped at 2^16 - 1: a 16-bit draw below it drops the element."""
    return min(int(np.floor(float(np.float32(p)) * 65536.0 + 0.5)), 65535)


def dropout_draws(seed, site, n, first=0):
    """The 16-bit draws of elements first .. first + n - 1 of a site: element i is in group g8 = i >> 3; e = i & 7 reads word e >> 1,
    half e & 1, low half first."""
    first, n = int(first), int(n)
    g8 = np.arange(first >> 3, (first + n + 7) >> 3, dtype=U64)
    words = np.stack(philox4x32(dropout_counter(g8, site), split64(seed), DROPOUT_ROUNDS), axis=-1)            # (groups, 4)
    halves = np.stack([words & U64(0xFFFF), words >> U64(16)], axis=-1)                                     # (groups, word, half)
    return halves.reshape(-1)[first & 7:(first & 7) + n]


def dropout_factors(seed, site, p, n):
    """(n,) float32: 0 where the draw is below the threshold, else 1 / (1 - p) in float32 arithmetic."""
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(dropout_draws(seed, site, n) < U64(dropout_threshold(p)), np.float32(0.0), keep).astype(np.float32)


# ---- batch assembly ----
def batch_words(seed, purpose, sample_id, n):
    """(B, n) words: value i of an item is word i & 3 of group i >> 2."""
    sid = _u64(sample_id).reshape(-1, 1)
    g = np.arange((int(n) + 3) // 4, dtype=U64)[None, :]
    words = np.stack(philox4x32(batch_counter(g, purpose, sid), split64(seed), BATCH_ROUNDS), axis=-1)   # (B, groups, 4)
    return words.reshape(sid.shape[0], -1)[:, :int(n)]


def batch_draw(offsets, index, sample_id, N, C, seed):
    """(choice int32 (B,N), drop_u float32 (B,C), aug_u float32 (B,6)).  choice = (w M) >> 32 with M the point count of cloud index[b]
    (an index outside the set or an empty cloud: M = 0, every choice 0); the unit floats are (w >> 8) 2^-24."""
    offsets, index = np.asarray(offsets, dtype=np.int64), np.asarray(index, dtype=np.int64).reshape(-1)
    S = offsets.size - 1
    ok = (index >= 0) & (index < S)
    s = np.where(ok, index, 0)
    M = np.where(ok, np.maximum(offsets[s + 1] - offsets[s], 0), 0)
    assert M.max(initial=0) < 2 ** 32
    choice = ((batch_words(seed, DRAW_CHOICE, sample_id, N) * _u64(M)[:, None]) >> U64(32)).astype(np.int32)
    return choice, unit24(batch_words(seed, DRAW_DROP, sample_id, C)), unit24(batch_words(seed, DRAW_AUG, sample_id, 6))


# ---- part-sampling normals ----
def part_words(seed, row0, rows, J, n_draws):
    """(rows, n_draws, 3, J) words: draw d of (row, axis c, part j) is word d & 3 of group d >> 2."""
    row = np.array([int(row0) + r for r in range(int(rows))], dtype=object).reshape(-1, 1, 1, 1)
    g = np.arange(int(n_draws) // 4, dtype=U64).reshape(1, -1, 1, 1)
    c, j = np.arange(3, dtype=U64).reshape(1, 1, 3, 1), np.arange(int(J), dtype=U64).reshape(1, 1, 1, -1)
    w = np.stack(philox4x32(part_counter(g, c, j, _u64(row)), split64(seed), PART_ROUNDS), axis=2)   # (rows, groups, 4, 3, J)
    return w.reshape(int(rows), int(n_draws), 3, int(J))


def part_normals(seed, row0, rows, J, n_draws):
    """(rows, n_draws, 3, J) float64: words (2 k, 2 k + 1) of a group give draws (2 k, 2 k + 1) = r (cos, sin)(2 pi u2),
    r = sqrt(-2 ln u1), u1 = ((a >> 8) + 0.5) 2^-24 in (0, 1), u2 = (b >> 8) 2^-24 in [0, 1)."""
    w = part_words(seed, row0, rows, J, n_draws)
    a, b = w[:, 0::2], w[:, 1::2]
    r, ang = np.sqrt(-2.0 * np.log(unit24_open(a))), 2 * np.pi * (b >> U64(8)).astype(np.float64) * 2.0 ** -24
    out = np.empty(w.shape, dtype=np.float64)
    out[:, 0::2], out[:, 1::2] = r * np.cos(ang), r * np.sin(ang)
    return out


# ---- box-Chamfer unit draws ----
def box_words(seed, pair0, P, C):
    """(P, C, 2, 512, 4): all four words of (pair pair0 + i, class, side, point)."""
    pair = np.array([int(pair0) + i for i in range(int(P))], dtype=object).reshape(-1, 1, 1, 1)
    c, side = np.arange(int(C), dtype=U64).reshape(1, -1, 1, 1), np.arange(2, dtype=U64).reshape(1, 1, 2, 1)
    p = np.arange(BOX_PTS, dtype=U64).reshape(1, 1, 1, -1)
    return np.stack(philox4x32(box_counter(p, c, side, _u64(pair)), split64(seed), BOX_ROUNDS), axis=-1)


def box_units(seed, pair0, P, C):
    """(P, C, 2, 512, 3) float32 in [0, 1): words 0, 1, 2; word 3 is discarded."""
    return unit24(box_words(seed, pair0, P, C)[..., :3])
