"""The shapes of tests/test_train_workspace_cpu.py and the calls of the four training `*_workspace_bytes` functions (no GPU: they carve at
a null base).  tools/make_train_workspace_golden.py runs sizes() on the library of the PARENT of the commit under test."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_workspace_bytes.json")

DENOISER = [(1, 32, 1), (1, 32, 5), (8, 32, 5), (1, 256, 5), (3, 160, 5), (5, 480, 5), (2, 224, 2), (128, 2048, 5), (1, 8192, 5), (4, 4096, 8)]   # B, N, depth
POINTNET = [(2, 33), (4, 333), (8, 1024), (128, 2048)]   # B, N (4 anchors, zdim 256)
PRIOR = [1, 37, 64, 65, 128]                             # B (flow depth 14, hidden 256)


def mlp_cases():
    from test_gpu_dirty_memory import MLP_CASES
    return [(list(spec), B, M, ns) for spec, B, M, ns, _pool, _train in MLP_CASES]


def load(path=None):
    from difffacto_amd import _ffi, build
    lib = ctypes.CDLL(path or build.build(verbose=False))
    for name in ("dfx_denoiser_train_workspace_bytes", "dfx_pointnet_v2_train_workspace_bytes", "dfx_prior_loss_workspace_bytes",
                 "dfx_shared_mlp_train_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _ffi.SIGNATURES[name]
    return lib


def mlp_bytes(lib, spec, B, M, ns):
    from difffacto_amd import _ffi
    t = _ffi.SharedMlpTrain()
    t.layers = len(spec) - 1
    for i, ch in enumerate(spec):
        t.ch[i] = ch
    return int(lib.dfx_shared_mlp_train_workspace_bytes(ctypes.byref(t), B, M, ns))


def sizes(lib):
    """{function: {"shape as text": bytes}}"""
    return {"dfx_denoiser_train_workspace_bytes": {f"{B},{N},{d}": int(lib.dfx_denoiser_train_workspace_bytes(B, N, d)) for B, N, d in DENOISER},
            "dfx_pointnet_v2_train_workspace_bytes": {f"{B},{N}": int(lib.dfx_pointnet_v2_train_workspace_bytes(B, N, 4, 256)) for B, N in POINTNET},
            "dfx_prior_loss_workspace_bytes": {f"{B}": int(lib.dfx_prior_loss_workspace_bytes(B, 14, 256)) for B in PRIOR},
            "dfx_shared_mlp_train_workspace_bytes": {f"case {i}: {spec},{B},{M},{ns}": mlp_bytes(lib, spec, B, M, ns)   # (cases 0 and 3 differ in the mode only)
                                                     for i, (spec, B, M, ns) in enumerate(mlp_cases())}}
