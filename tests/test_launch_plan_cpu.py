"""The denoiser launcher's kernel choice (csrc/denoiser_plan.h: plan_launch) through its host-only hook dfx_debug_plan_variant, against
tests/golden/launch_plan.npz: the decisions (variant name, workgroups) of the launcher this planner replaced, recorded from that
launcher's own lines compiled as a host program (-ffp-contract=off) over engine settings x forcing codes x batch shapes.  Equality on
every row: re-measuring a cost constant or adding a variant means regenerating the fixture on purpose."""
import ctypes
import os

import numpy as np
import pytest

from _variants import NAMES

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan.npz")
F32, BF16 = 0, 1   # DFX_PREC_*


@pytest.fixture(scope="module")
def plan():
    from difffacto_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.dfx_debug_plan_variant.restype = ctypes.c_char_p
    lib.dfx_debug_plan_variant.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_longlong)]

    def call(prec, w1_fold, force_direct, code, B, N):
        grid = ctypes.c_longlong(-1)
        name = lib.dfx_debug_plan_variant(int(prec), int(w1_fold), int(force_direct), int(code), int(B), int(N), ctypes.byref(grid))
        return name.decode(), grid.value
    return call


def test_every_recorded_decision(plan):
    g = np.load(FIXTURE)
    names = [str(n) for n in g["names"]]
    cols = [g[k] for k in ("prec", "w1_fold", "force_direct", "code", "B", "N", "variant_index", "grid")]
    assert len(names) == 10 and len(set(names)) == 10 and 2000 < len(cols[0]) < 3000
    seen, wrong = set(), []
    for prec, fold, fd, code, B, N, vi, grid in zip(*cols):
        got = plan(prec, fold, fd, code, B, N)
        seen.add(got[0])
        if got != (names[vi], int(grid)):
            wrong.append(((prec, fold, fd, code, B, N), got, (names[vi], int(grid))))
    assert not wrong, (len(wrong), wrong[:10])
    assert seen == set(names)
    assert set(names) == set(NAMES["bf16"].values()) | set(NAMES["f32"].values()) | {"k_denoise<bf16>"}


def test_forced_codes_agree_with_the_test_helper(plan):
    for prec, key in ((BF16, "bf16"), (F32, "f32")):
        for code, name in NAMES[key].items():
            assert plan(prec, 1, 0, code, 3, 2048)[0] == name, (key, code)


def test_unknown_code_is_automatic(plan):
    for prec in (BF16, F32):
        for B, N in ((1, 2048), (3, 96), (5, 2048), (9, 2048), (64, 2048), (64, 32)):
            for code in (7, 3, -1, 64, 160, 161, 162, 1 << 20):
                assert plan(prec, 1, 0, code, B, N) == plan(prec, 1, 0, 0, B, N), (prec, B, N, code)


def test_grid_pointer_is_optional(plan):
    from difffacto_amd import _ffi
    assert _ffi.lib().dfx_debug_plan_variant(BF16, 1, 0, 0, 1, 2048, None) == b"k_denoise_coop"
