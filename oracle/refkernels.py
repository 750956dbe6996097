"""The reference's own FPS and auction-EMD CUDA kernels, run on the CPU (ORACLE — test infrastructure, dev container only).

Both kernels synchronise only through ``__syncthreads()``; ``oracle/cuda_on_cpu.h`` runs such a kernel as plain C++, one block
at a time, each CUDA thread a fibre that yields at every barrier.  This module is the recipe:

  1. cut the spans (``SPANS``: file, first line, last line — the kernels and the seven lines of the block-size rule) out of a checkout of the reference into ``oracle/_ref/``,
     refusing to go on unless each span's SHA-256 equals the digest committed here — only digests and line numbers are part of
     this repository, never the text;
  2. compile ``oracle/refkernels_driver.cpp`` (our launch code around the spans) with g++ into ``oracle/_ref/`` twice:
     ``librefkernels_nofma.so`` with ``-ffp-contract=off`` and ``librefkernels_fma.so`` with ``-ffp-contract=fast -mfma`` — the
     two ways a compiler may evaluate the kernels' three-term sums of squares;
  3. wrap the entry points with ctypes (``fps``, ``emd_forward``, ``emd_backward``; ``order=`` selects the fibre schedule).

Only tests/golden/make_golden_refkernels.py and the regeneration test of tests/test_refkernels_cpu.py use it.  GPU tests, smoke()
and the benchmark read the fixtures it produced and never this module.  ``selftest_lib()`` builds the shim's own toy kernels
(``cuda_on_cpu_selftest.cpp``) and needs no reference.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, "_ref")
REF_ROOT = os.environ.get("DFX_REFERENCE_ROOT", "/root/reference")

ASCENDING, DESCENDING = 0, 1

# (file under the reference root, first line, last line, output name, sha256 of exactly those lines)
SPANS = (
    ("pointnet2_ops_lib/pointnet2_ops/_ext-src/include/cuda_utils.h", 13, 19, "ref_cuda_utils_13_19.inc",
     "c230a4d20ed5dd6fed2397d9287d698a0d11fe8fb35b71934608323df5094681"),
    ("pointnet2_ops_lib/pointnet2_ops/_ext-src/src/sampling_gpu.cu", 59, 173, "ref_sampling_gpu_59_173.inc",
     "0aefe583b1548ea099f458b7039f27484278d1a84c09a88887ce87aee703da0b"),
    ("python/difffacto/metrics/emd/emd_cuda.cu", 10, 226, "ref_emd_cuda_10_226.inc",
     "5cf22b5f20f250fccd04d398bc056124d20661a5d0659500982110c6589dd5d4"),
    ("python/difffacto/metrics/emd/emd_cuda.cu", 284, 300, "ref_emd_cuda_284_300.inc",
     "d0dc0a3ea04e6a2513007cbf4010aa0f4db0ae55da18d5b974625636be50fec5"),
)

CXX = os.environ.get("CXX", "g++")
BASE_FLAGS = ["-O1", "-std=c++17", "-fPIC", "-shared", "-w"]
BUILDS = {"nofma": ["-ffp-contract=off"], "fma": ["-ffp-contract=fast", "-mfma"]}

_F, _I = np.float32, np.int32
_libs = {}


def available():
    return all(os.path.isfile(os.path.join(REF_ROOT, s[0])) for s in SPANS)


def span_text(path, first, last):
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    return b"\n".join(lines[first - 1:last]) + b"\n"


def extract():
    """Write the spans to oracle/_ref/; RuntimeError when a digest does not match (another revision of the reference)."""
    os.makedirs(OUT, exist_ok=True)
    for rel, first, last, name, want in SPANS:
        text = span_text(os.path.join(REF_ROOT, rel), first, last)
        got = hashlib.sha256(text).hexdigest()
        if got != want:
            raise RuntimeError(f"{rel}:{first}-{last}: sha256 {got}, the recipe expects {want}")
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(text)


def _compile(src, out, flags, include_ref):
    cmd = [CXX] + BASE_FLAGS + flags + ["-I", _HERE] + (["-I", OUT] if include_ref else []) + ["-o", out, src]
    subprocess.check_call(cmd)


def build(force=False):
    """Extract + compile both contraction builds.  Returns {"nofma": path, "fma": path}."""
    src = os.path.join(_HERE, "refkernels_driver.cpp")
    deps = [src, os.path.join(_HERE, "cuda_on_cpu.h"), os.path.abspath(__file__)]
    paths = {k: os.path.join(OUT, f"librefkernels_{k}.so") for k in BUILDS}
    newest = max(os.path.getmtime(d) for d in deps)
    if force or not all(os.path.exists(p) and os.path.getmtime(p) >= newest for p in paths.values()):
        extract()
        for k, flags in BUILDS.items():
            _compile(src, paths[k], flags, True)
    return paths


def lib(build_name="nofma"):
    if build_name not in _libs:
        L = ctypes.CDLL(build()[build_name])
        L.ref_fps.restype = ctypes.c_int
        L.ref_emd_forward.restype = ctypes.c_int
        L.ref_emd_backward.restype = ctypes.c_int
        _libs[build_name] = L
    return _libs[build_name]


def selftest_lib():
    """The shim's toy kernels (no reference needed), built into oracle/_ref/ as well."""
    if "selftest" not in _libs:
        os.makedirs(OUT, exist_ok=True)
        src, out = os.path.join(_HERE, "cuda_on_cpu_selftest.cpp"), os.path.join(OUT, "libcuda_on_cpu_selftest.so")
        newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(_HERE, "cuda_on_cpu.h")))
        if not os.path.exists(out) or os.path.getmtime(out) < newest:
            _compile(src, out, ["-ffp-contract=off"], False)
        _libs["selftest"] = ctypes.CDLL(out)
    return _libs["selftest"]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def fps(xyz, npoint, order=DESCENDING, build_name="nofma"):
    """furthest_point_sampling (sampling.cpp:63-86 + the kernel wrapper): (B, npoint) int32.  The default schedule is DESCENDING:
    the kernel reads ``dists_i[0]`` after the last barrier of a step (:170) while thread 0 overwrites it in the next step's scan
    (:112) before any further barrier; only thread 0 writes that slot, so running thread 0 last between barriers is the
    hazard-free schedule."""
    xyz = np.ascontiguousarray(xyz, _F)
    B, N, _ = xyz.shape
    tmp = np.full((B, N), 1e10, _F)
    out = np.zeros((B, npoint), _I)
    L = lib(build_name)
    L.ref_schedule(order)
    if L.ref_fps(B, N, int(npoint), _p(xyz), _p(tmp), _p(out)) != 1:
        raise ValueError("the reference has no kernel instance for this size")
    return out


def emd_forward(xyz1, xyz2, eps, iters, order=ASCENDING, build_name="nofma", trace=False):
    """emdFunction.forward: (dist (B, n), assignment (B, n)); with trace=True also the first pair's unassigned count per iteration
    and (iterations with a target whose GetMax race is live, number of such (iteration, target) pairs)."""
    xyz1, xyz2 = np.ascontiguousarray(xyz1, _F), np.ascontiguousarray(xyz2, _F)
    B, n, _ = xyz1.shape
    assert xyz2.shape == xyz1.shape
    dist, asg, hist, ties = np.zeros((B, n), _F), np.zeros((B, n), _I), np.zeros(max(iters, 1), _I), np.zeros(2, _I)
    L = lib(build_name)
    L.ref_schedule(order)
    rc = L.ref_emd_forward(B, n, _p(xyz1), _p(xyz2), ctypes.c_float(eps), int(iters), _p(dist), _p(asg),
                           _p(hist) if trace else None, _p(ties) if trace else None)
    if rc != 1:
        raise ValueError("the reference refuses this input (n must be a multiple of 1024, B <= 512)")
    return (dist, asg, hist[:iters], ties) if trace else (dist, asg)


def emd_backward(xyz1, xyz2, grad_dist, assignment, order=ASCENDING, build_name="nofma"):
    xyz1, xyz2, grad_dist = (np.ascontiguousarray(a, _F) for a in (xyz1, xyz2, grad_dist))
    assignment = np.ascontiguousarray(assignment, _I)
    B, n, _ = xyz1.shape
    g = np.zeros_like(xyz1)
    L = lib(build_name)
    L.ref_schedule(order)
    if L.ref_emd_backward(B, n, _p(xyz1), _p(xyz2), _p(grad_dist), _p(assignment), _p(g)) != 1:
        raise ValueError("the reference refuses this input")
    return g


if __name__ == "__main__":
    for _rel, _first, _last, _name, _ in SPANS:   # print the digests of the checkout at hand
        print(hashlib.sha256(span_text(os.path.join(REF_ROOT, _rel), _first, _last)).hexdigest(), f"{_rel}:{_first}-{_last}")
