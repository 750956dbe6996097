#!/usr/bin/env python
"""Dev-container-only: pins of FPS and the auction EMD to the reference's own CUDA kernels, run on the CPU.

    python tests/golden/make_golden_refkernels.py          # writes tests/golden/refk_*.npz and rewrites MANIFEST.sha256

oracle/refkernels.py cuts the kernel text of sampling_gpu.cu:59-173 and emd_cuda.cu:10-226,284-300 out of a checkout of the
reference (digest-checked), compiles it against the CUDA-on-CPU shim oracle/cuda_on_cpu.h — twice: without contraction and with
`-ffp-contract=fast -mfma` — and this script stores inputs and outputs.  Deterministic: a second run writes the same manifest.
The fixtures are chosen so that the two things the reference leaves open cannot decide them:

  contraction   lattice clouds (coordinates k/16, k/8, planted k/64): every product and sum of the distance is exact, the two
                builds must agree bit for bit (asserted).  Random clouds are kept only if both builds give the same indices /
                assignment; otherwise the next seed is tried (at most 16), the count of rejected seeds is stored.
  GetMax race   (emd_cuda.cu:181-194: every bidder inside 1e-6 of a target's best increment writes max_idx, unordered).
                Lattice clouds tie constantly; their fixtures are the ASCENDING fibre schedule = "last writer = largest bidder"
                (`race_rule`), and the DESCENDING assignment is stored next to it to show how much of the result the race is.
                Random clouds are kept only if both schedules (and both builds) agree: they pin Bid's chunking and merge,
                eviction and the last iteration without leaning on any race rule.

FPS runs on the DESCENDING schedule: the kernel reads dists_i[0] after the last barrier of a step (:170) and thread 0 overwrites
it in the next step's scan (:112) before any further barrier — a hazard of the reference.  Only thread 0 writes that slot, so the
schedule that runs thread 0 last between barriers is the hazard-free one.

FPS clouds: k/16 in [-1/2, 1/2] (heavy duplication, exact ties) with every seventh point planted on k/64, |k| <= 2, which puts
|p|^2 at 0 .. 12/4096 around the kernel's origin-skip threshold 1e-3 = 4.096/4096 (:100-101): 3/4096 and 4/4096 = 1/1024 are
skipped, 5/4096 is not; (1,1,1)/64, (2,0,0)/64 and (2,1,0)/64 are planted by hand wherever N allows.  ([-1/64, 1/64] alone
reaches 3/4096 only, so the range is one step wider.)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import refk_fixtures as fxs  # noqa: E402
from oracle import refkernels as rk  # noqa: E402

F32, I32 = np.float32, np.int32
MAX_SEEDS = 16

# ---------------------------------------------------------------------------------------------------------------- FPS
# tag: (B, N, M, seed)   N: 1, 5, 33 block sizes 1, 4, 32; 512/513/700 bs 512 on a 256-thread HIP kernel; 1024.., 2048.., 4096..
# the launch-table boundaries; 3000 the 512x8 shape; 8192/8193 the LDS-coordinates flip; 16384/16385 resident / streaming.
FPS_LATTICE = {
    "N1": (1, 1, 1, 9001), "N5": (1, 5, 5, 9005), "N33": (2, 33, 33, 9033),
    "N512": (2, 512, 128, 9512), "N513": (2, 513, 128, 9513), "N700": (2, 700, 64, 9700),
    "N1024": (2, 1024, 128, 91024), "N1025": (2, 1025, 128, 91025),
    "N2048": (2, 2048, 256, 92048), "N2049": (1, 2049, 128, 92049), "N3000": (1, 3000, 128, 93000),
    "N4096": (1, 4096, 128, 94096), "N4097": (1, 4097, 128, 94097),
    "N8192": (1, 8192, 64, 98192), "N8193": (1, 8193, 64, 98193),
    "N16384": (1, 16384, 64, 916384), "N16385": (1, 16385, 64, 916385),
}
FPS_DUP = ("dup600", 1, 600, 200, 9600, 50)       # 50 distinct locations: the maximum falls to 0, every later step is a pure tie
FPS_RANDOM = ("rand1500", 2, 1500, 200, 9150)     # first seed; the next ones follow
# The skip compares the float |p|^2 with the DOUBLE 1e-3 (:101), which no float equals: the largest skipped value is 0x3a83126e and
# the float 1e-3f = 0x3a83126f is already kept.  Points with exactly these two magnitudes, far from a small cluster, npoint = N: a kept
# point is picked sooner or later, a skipped one never.
FPS_THRESH = ("thresh40", 1, 40, 40, 9040)
SKIP_LAST, KEEP_FIRST = 0x3a83126e, 0x3a83126f


def fps_lattice_num(B, N, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    num = rng.integers(-8, 9, (B, N, 3)) * 4
    slots = np.arange(0, N, 7)
    num[:, slots] = rng.integers(-2, 3, (B, len(slots), 3))
    for s, p in zip(slots[1:4], ((1, 1, 1), (2, 0, 0), (2, 1, 0))):   # 3/4096, 4/4096 (skipped), 5/4096 (kept)
        num[:, s] = p
    return num.astype(np.int8)


def point_with_mag(bits):
    """(x, y): float32 with x*x + y*y == the float with these bits whichever way the sum is contracted (y a power of two or 0, so
    y*y is exact; x*x rounded first or fused into the addition give the same float)."""
    t = np.array(bits, np.uint32).view(F32)[()]
    for y in [0.0] + [2.0 ** -e for e in range(6, 12)]:
        lo = hi = F32(np.sqrt(float(t) - y * y))
        cands = [lo]
        for _ in range(8):
            lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(1))
            cands += [lo, hi]
        for c in cands:
            xx = float(c) * float(c)   # exact in float64
            if F32(float(F32(xx)) + y * y) == t and F32(xx + y * y) == t:
                return c, F32(y)
    raise RuntimeError(f"no point with |p|^2 = {bits:#x}")


def fps_threshold_cloud(N, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    cells = rng.permutation(5 ** 3)[:N]   # distinct lattice points k/16, k = 4..8, per coordinate: a cluster around (3/8, 3/8, 3/8)
    xyz = (np.stack([cells // 25, cells // 5 % 5, cells % 5], 1) + 4).astype(F32) / F32(16)
    (xk, yk), (xs, ys) = point_with_mag(KEEP_FIRST), point_with_mag(SKIP_LAST)
    special = [(xk, yk, 0), (0, -xk, yk), (xs, ys, 0), (-ys, 0, xs), (2 / 64, 0, 0), (2 / 64, 1 / 64, 0), (1 / 64, 1 / 64, 1 / 64), (0, 0, 0)]
    xyz[3:3 + 4 * len(special):4] = np.array(special, F32)
    return xyz[None]


def fps_tie_steps(xyz, idx, check):
    """Number of selection steps at which more than one candidate held the maximum distance (float32, uncontracted; exact on the
    lattice).  With check: the stored pick is one of the maxima at every step (it cannot say which — that is the fixture's job)."""
    ties = 0
    for b in range(xyz.shape[0]):
        x = xyz[b]
        keep = ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).astype(np.float64) > 1e-3
        d = np.full(len(x), 1e10, F32)
        for j in range(1, idx.shape[1]):
            t = x - x[idx[b, j - 1]]
            d = np.minimum(d, (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
            if not keep.any():
                assert idx[b, j] == 0
                continue
            top = d[keep].max()
            ties += int((d[keep] == top).sum() > 1)
            if check:
                assert keep[idx[b, j]] and d[idx[b, j]] == top, (b, j)
    return ties


def _fps_both_builds(xyz, M):
    out = {k: rk.fps(xyz, M, order=rk.DESCENDING, build_name=k) for k in rk.BUILDS}
    return out["nofma"], np.array_equal(out["nofma"], out["fma"])


def make_fps(tag):
    if tag in FPS_LATTICE or tag == FPS_DUP[0]:
        if tag in FPS_LATTICE:
            B, N, M, seed = FPS_LATTICE[tag]
            num = fps_lattice_num(B, N, seed)
        else:
            _, B, N, M, seed, nloc = FPS_DUP
            rng = np.random.Generator(np.random.PCG64(seed))
            locs = rng.integers(-8, 9, (nloc, 3)) * 4
            num = locs[rng.integers(0, nloc, (B, N))].astype(np.int8)
        xyz = num.astype(F32) / F32(64)
        idx, same = _fps_both_builds(xyz, M)
        assert same, f"{tag}: the contraction builds disagree on a lattice cloud"
        return dict(xyz_num=num, den=np.array(64), npoint=np.array(M), idx=idx.astype(I32), kind=np.array("lattice"),
                    seed=np.array(seed), rejected=np.array(0), tie_steps=np.array(fps_tie_steps(xyz, idx, True)))
    from oracle import pointnet2 as opn
    if tag == FPS_THRESH[0]:
        _, B, N, M, seed = FPS_THRESH
        xyz = fps_threshold_cloud(N, seed)
        idx, same = _fps_both_builds(xyz, M)
        assert same, f"{tag}: the contraction builds disagree"
        mag = (xyz.astype(np.float64) ** 2).sum(-1)[0]
        picked = np.isin(np.arange(N), idx[0])
        assert picked[mag > 1e-3].all() and not picked[(mag <= 1e-3) & (np.arange(N) > 0)].any()   # kept <=> picked
        assert set(np.nonzero(~picked)[0]) == {11, 15, 19, 27, 31}
        return dict(xyz=xyz, npoint=np.array(M), idx=idx.astype(I32), kind=np.array("threshold"), seed=np.array(seed),
                    rejected=np.array(0), tie_steps=np.array(fps_tie_steps(xyz, idx, True)))
    _, B, N, M, seed0 = FPS_RANDOM
    assert tag == FPS_RANDOM[0]
    for r in range(MAX_SEEDS):
        rng = np.random.Generator(np.random.PCG64(seed0 + r))
        xyz = rng.uniform(-1, 1, (B, N, 3)).astype(F32)
        xyz[:, 5::97] *= F32(0.03)        # a few points around the skip threshold
        idx, same = _fps_both_builds(xyz, M)
        if same and np.array_equal(idx, opn.furthest_point_sampling(xyz, M)):
            return dict(xyz=xyz, npoint=np.array(M), idx=idx.astype(I32), kind=np.array("random"), seed=np.array(seed0 + r),
                        rejected=np.array(r), tie_steps=np.array(fps_tie_steps(xyz, idx, False)))
        print(f"  fps {tag}: seed {seed0 + r} rejected (builds agree: {same})")
    raise RuntimeError("no random FPS cloud on which both contraction builds and the oracle agree")


# ---------------------------------------------------------------------------------------------------------------- EMD
# lattice, tag: (den, B, n, iters, eps, seed)
EMD_LATTICE = {
    "lat16_n1024_B1_it1": (16, 1, 1024, 1, 0.002, 7101), "lat16_n1024_B2_it2": (16, 2, 1024, 2, 0.002, 7102),
    "lat16_n1024_B1_it30": (16, 1, 1024, 30, 0.002, 7103), "lat16_n1024_B2_it200": (16, 2, 1024, 200, 0.002, 7104),
    "lat8_n1024_B2_it30": (8, 2, 1024, 30, 0.002, 7105), "lat8_n1024_B1_it200": (8, 1, 1024, 200, 0.002, 7106),
    "lat16_n2048_B1_it30": (16, 1, 2048, 30, 0.002, 7107), "lat8_n2048_B2_it2": (8, 2, 2048, 2, 0.002, 7108),
    "lat8_n2048_B1_it200": (8, 1, 2048, 200, 0.002, 7109), "lat16_n2048_B2_it1": (16, 2, 2048, 1, 0.002, 7110),
    # the last iteration has 1..8 bidders (the HIP kernel's separate tail path); eps raised so that a few hundred iterations get there
    "lat8_n1024_B1_tail": (8, 1, 1024, 207, 0.05, 7001),
    # n > 2048: Bid walks the targets in batches of 2048 (:125-158), each of a bidder's threads its chunk of EVERY batch, and merges the
    # threads in order — among equal values the winner is then not the first in k order.  It shows from the first iteration with two
    # or more threads per bidder (fewer than 512 (n / 1024) unassigned; asserted below).  3072 also has a short last batch, with a
    # chunk length of its own; its tail case runs the last 30 iterations with 8 .. 4 bidders (hundreds of threads each).
    "lat8_n4096_B1_it10": (8, 1, 4096, 10, 0.002, 7111), "lat16_n3072_B1_it30": (16, 1, 3072, 30, 0.002, 7112),
    "lat16_n3072_B1_tail": (16, 1, 3072, 123, 0.1, 7113),
}
# random, tag: (B, n, iters, eps, first seed, tail)
EMD_RANDOM = {
    "rand_n1024_B1_it100": (1, 1024, 100, 0.002, 7201, False), "rand_n1024_B2_it60": (2, 1024, 60, 0.002, 7221, False),
    "rand_n1024_B1_it30": (1, 1024, 30, 0.005, 7241, False), "rand_n2048_B1_it60": (1, 2048, 60, 0.002, 7261, False),
    "rand_n1024_B1_tail": (1, 1024, 261, 0.02, 7281, True),
}
EMD_BWD = ("lat16_n1024_B2", "lat16_n1024_B2_it2")   # backward: the clouds and assignment of that forward fixture


def emd_lattice_num(den, B, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, den + 1, (B, n, 3)).astype(np.uint8), rng.integers(0, den + 1, (B, n, 3)).astype(np.uint8)


def emd_random_clouds(B, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(0, 1, (B, n, 3)).astype(F32), rng.uniform(0, 1, (B, n, 3)).astype(F32)


def _emd_meta(kind, eps, iters, asg, asg_desc, dist, hist, ties, seed, rejected):
    return dict(eps=np.array(eps, F32), iters=np.array(iters), assignment=asg.astype(I32), assignment_desc=asg_desc.astype(I32),
                dist=dist.astype(F32), kind=np.array(kind), race_rule=np.array(fxs.RACE_RULE), seed=np.array(seed),
                rejected=np.array(rejected), tie_iters=np.array(int(ties[0])), tied_targets=np.array(int(ties[1])),
                race_moved=np.array(int((asg != asg_desc).sum())), last_bidders=np.array(int(hist[-1])))


def make_emd(tag):
    if tag in EMD_LATTICE:
        den, B, n, iters, eps, seed = EMD_LATTICE[tag]
        an, bn = emd_lattice_num(den, B, n, seed)
        a, b = an.astype(F32) / F32(den), bn.astype(F32) / F32(den)
        dist, asg, hist, ties = rk.emd_forward(a, b, eps, iters, order=rk.ASCENDING, build_name="nofma", trace=True)
        dist_f, asg_f = rk.emd_forward(a, b, eps, iters, order=rk.ASCENDING, build_name="fma")
        assert np.array_equal(asg, asg_f) and np.array_equal(dist, dist_f), f"{tag}: the contraction builds disagree on a lattice cloud"
        _, asg_desc = rk.emd_forward(a, b, eps, iters, order=rk.DESCENDING, build_name="nofma")
        if tag.endswith("_tail"):
            assert 1 <= hist[-1] <= 8, (tag, int(hist[-1]))
        if n > 2048:
            assert B == 1 and sum(1 for u in hist if u and 1024 // -(-int(u) // (n // 1024)) >= 2) >= 5, (tag, hist.tolist())
        return dict(a_num=an, b_num=bn, den=np.array(den), **_emd_meta("lattice", eps, iters, asg, asg_desc, dist, hist, ties, seed, 0))
    B, n, iters, eps, seed0, tail = EMD_RANDOM[tag]
    for r in range(MAX_SEEDS):
        a, b = emd_random_clouds(B, n, seed0 + r)
        dist, asg, hist, ties = rk.emd_forward(a, b, eps, iters, order=rk.ASCENDING, build_name="nofma", trace=True)
        why = None
        if tail and not 1 <= hist[-1] <= 8:
            why = f"last iteration has {int(hist[-1])} bidders"
        for order, build in ((rk.DESCENDING, "nofma"), (rk.ASCENDING, "fma"), (rk.DESCENDING, "fma")):
            if why is None and not np.array_equal(rk.emd_forward(a, b, eps, iters, order=order, build_name=build)[1], asg):
                why = f"assignment differs on the {'descending' if order else 'ascending'} schedule of the {build} build"
        if why is None:
            return dict(a=a, b=b, **_emd_meta("random", eps, iters, asg, asg, dist, hist, ties, seed0 + r, r))
        print(f"  emd {tag}: seed {seed0 + r} rejected: {why}")
    raise RuntimeError(f"{tag}: no seed on which both schedules and both contraction builds agree")


def make_emdbwd():
    fwd = make_emd(EMD_BWD[1])
    den = int(fwd["den"])
    a, b = fwd["a_num"].astype(F32) / F32(den), fwd["b_num"].astype(F32) / F32(den)
    rng = np.random.Generator(np.random.PCG64(7301))
    gnum = rng.integers(-12, 13, fwd["assignment"].shape).astype(np.int8)   # k/8 in [-1.5, 1.5]: 2 g (x1 - x2) is exact
    g = gnum.astype(F32) / F32(8)
    out = {k: rk.emd_backward(a, b, g, fwd["assignment"], order=o, build_name=k) for k in rk.BUILDS for o in (rk.ASCENDING,)}
    assert np.array_equal(out["nofma"], out["fma"])
    assert np.array_equal(out["nofma"], rk.emd_backward(a, b, g, fwd["assignment"], order=rk.DESCENDING))
    return dict(a_num=fwd["a_num"], b_num=fwd["b_num"], den=fwd["den"], eps=fwd["eps"], iters=fwd["iters"],
                assignment=fwd["assignment"], grad_dist_num=gnum, grad_den=np.array(8), grad_xyz1=out["nofma"].astype(F32))


def all_cases():
    """[(file name, maker)] of every fixture this script writes."""
    out = [(f"refk_fps_{t}.npz", (lambda t=t: make_fps(t))) for t in list(FPS_LATTICE) + [FPS_DUP[0], FPS_THRESH[0], FPS_RANDOM[0]]]
    out += [(f"refk_emd_{t}.npz", (lambda t=t: make_emd(t))) for t in list(EMD_LATTICE) + list(EMD_RANDOM)]
    out.append((f"refk_emdbwd_{EMD_BWD[0]}.npz", make_emdbwd))
    return out


def regeneration_subset():
    """What tests/test_refkernels_cpu.py rebuilds (about half a minute): every FPS fixture, every EMD fixture of <= 30 iterations."""
    small = [t for t, c in EMD_LATTICE.items() if c[3] <= 30] + [t for t, c in EMD_RANDOM.items() if c[2] <= 30]
    return [(n, m) for n, m in all_cases() if n.startswith("refk_fps_") or n[len("refk_emd_"):-4] in small]


def main():
    import manifest
    rk.build(force=True)
    for name, maker in all_cases():
        fx = maker()
        np.savez_compressed(os.path.join(HERE, name), **fx)
        if name.startswith("refk_fps_"):
            print(f"{name}: xyz {fx['idx'].shape[0]}x{(fx['xyz_num'] if 'xyz_num' in fx else fx['xyz']).shape[1]} npoint {int(fx['npoint'])} "
                  f"seed {int(fx['seed'])} rejected {int(fx['rejected'])} tie steps {int(fx['tie_steps'])} of "
                  f"{fx['idx'].shape[0] * (int(fx['npoint']) - 1)}")
        elif name.startswith("refk_emd_"):
            print(f"{name}: seed {int(fx['seed'])} rejected {int(fx['rejected'])} eps {float(fx['eps']):g} iters {int(fx['iters'])} "
                  f"tie iterations {int(fx['tie_iters'])} tied targets {int(fx['tied_targets'])} moved by the race "
                  f"{int(fx['race_moved'])} of {fx['assignment'].size} last-iteration bidders {int(fx['last_bidders'])}")
        else:
            print(f"{name}: grad_xyz1 {fx['grad_xyz1'].shape}")
    manifest.write()


if __name__ == "__main__":
    main()
