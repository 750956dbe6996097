"""The allocation harness of tests/_dirty.py, on the CPU: its fill patterns, its pass-throughs, that it restores
torch.empty after an exception, that it can fail (three defective stand-in "kernels" written in torch), and that every
function of the package that allocates with torch.empty is named by the GPU file's coverage tables."""
import ast
import glob
import importlib
import os

import pytest
import torch

import _dirty
from _dirty import allocations, first_difference, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = (torch.float32, torch.float64, torch.bfloat16, torch.float16)
SIGNED = (torch.int8, torch.int16, torch.int32, torch.int64)


# ---- fill patterns ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS + SIGNED + (torch.uint8,))
def test_fill_patterns_per_dtype(dtype):
    with allocations("zero", "cpu") as h:
        z = torch.empty(3, 5, dtype=dtype)
        zl = torch.empty_like(z)
        assert h.served == 2
        assert (z == 0).all() and (zl == 0).all()
    with allocations("ff", "cpu") as h:
        f = torch.empty(3, 5, dtype=dtype)
        fl = torch.empty_like(f, dtype=dtype)
        fs = torch.empty((), dtype=dtype)
        assert h.served == 3
        for t in (f, fl, fs):
            assert t.dtype == dtype and t.is_contiguous()
            assert (t.reshape(-1).view(torch.uint8) == 255).all()
            if dtype in FLOATS:
                assert torch.isnan(t).all()
            elif dtype in SIGNED:
                assert (t == -1).all()
            else:
                assert (t == 255).all()
        assert f.shape == (3, 5) and fl.shape == (3, 5) and fs.shape == ()


def test_ff_keeps_the_strides_of_empty_like_and_the_guard_size_rule():
    src = torch.zeros(4, 6).t()
    with allocations("ff", "cpu"):
        t = torch.empty_like(src)
        assert t.shape == src.shape and t.stride() == src.stride()
        assert torch.isnan(t).all()
    assert _dirty.guard_bytes(1) == 1 << 20
    assert _dirty.guard_bytes((1 << 20) + 1) == (1 << 20) + 256
    assert _dirty.guard_bytes(5 << 20) == 5 << 20
    assert _dirty.guard_bytes(1 << 30) == 64 << 20


def test_other_devices_pinned_requests_and_empty_tensors_pass_through():
    with allocations("ff", "cpu") as h:
        m = torch.empty(4, device="meta")
        e = torch.empty(0, 7)
        el = torch.empty_like(e)
        assert m.device.type == "meta"
        assert h.served == 0 and h.passed_through == 3
        torch.empty(1)          # a harness that served nothing raises on exit
    real = torch.empty
    with allocations("zero", "cpu") as h:
        seen = {}

        def probe(*a, **k):
            seen.update(k)
            return real(*a, **{x: y for x, y in k.items() if x != "pin_memory"})
        h._orig = (probe, h._orig[1])
        t = h._serve(probe(8, pin_memory=True), dict(pin_memory=True))      # a pinned request is not counted or filled
        assert h.served == 0 and seen["pin_memory"] is True and t.shape == (8,)
        torch.empty(1)
    z = torch.zeros
    with allocations("ff", "cpu"):
        assert torch.zeros is z                                            # torch.zeros is never patched
        torch.empty(1)


def test_a_harness_that_served_nothing_fails():
    with pytest.raises(AssertionError, match="served no allocation"):
        with allocations("zero", "cpu"):
            pass
    with pytest.raises(AssertionError, match="served no allocation"):
        with allocations("ff", "cpu"):
            torch.empty(3, device="meta")


def test_originals_are_restored_after_an_exception():
    e, el = torch.empty, torch.empty_like
    for mode in ("zero", "record", "ff"):
        with pytest.raises(KeyError):
            with allocations(mode, "cpu"):
                assert torch.empty is not e and torch.empty_like is not el
                torch.empty(2)
                raise KeyError("boom")
        assert torch.empty is e and torch.empty_like is el
    with pytest.raises(ValueError):
        with allocations("nonsense", "cpu"):
            pass
    assert torch.empty is e and torch.empty_like is el


# ---- stale -----------------------------------------------------------------------------------------------------
def test_stale_hands_back_the_recorded_buffers_in_order_unmodified():
    with allocations("record", "cpu") as rec:
        a = torch.empty(2, 3)
        b = torch.empty(4, dtype=torch.int32)
        a.fill_(7.0)
        b.copy_(torch.arange(4, dtype=torch.int32))
    with allocations("stale", "cpu", recording=rec.recording) as h:
        a2 = torch.empty(2, 3)
        b2 = torch.empty(4, dtype=torch.int32)
        assert a2.data_ptr() == a.data_ptr() and b2.data_ptr() == b.data_ptr()
        assert (a2 == 7.0).all() and b2.tolist() == [0, 1, 2, 3]
        assert h.served == 2


@pytest.mark.parametrize("second", [lambda: torch.empty(2, 4), lambda: torch.empty(2, 3, dtype=torch.float64),
                                    lambda: torch.empty_like(torch.zeros(3, 2).t())], ids=["shape", "dtype", "strides"])
def test_stale_raises_on_a_mismatch_with_the_recording(second):
    with allocations("record", "cpu") as rec:
        torch.empty(2, 3)
    with pytest.raises(_dirty.StaleMismatch, match="allocation #0"):
        with allocations("stale", "cpu", recording=rec.recording):
            second()
    assert torch.empty.__module__ == "torch" or torch.empty.__name__ == "empty"


def test_stale_raises_on_another_number_of_allocations():
    with allocations("record", "cpu") as rec:
        torch.empty(2, 3)
        torch.empty(5)
    with pytest.raises(_dirty.StaleMismatch, match="1 allocations served, 2 recorded"):
        with allocations("stale", "cpu", recording=rec.recording):
            torch.empty(2, 3)
    with allocations("record", "cpu") as rec:
        torch.empty(2, 3)
    with pytest.raises(_dirty.StaleMismatch, match="holds only 1"):
        with allocations("stale", "cpu", recording=rec.recording):
            torch.empty(2, 3)
            torch.empty(5)
    with pytest.raises(ValueError):
        with allocations("stale", "cpu"):
            pass


# ---- guards ----------------------------------------------------------------------------------------------------
def _writes_one_element_before_its_buffer(n):
    out = torch.empty(n, dtype=torch.float32)
    i = -1                                                     # an index read from an unwritten cell
    out.as_strided((1,), (1,), out.storage_offset() + i).fill_(3.0)
    out.fill_(1.0)
    return out


def test_guard_violation_is_reported_with_ordinal_and_frame():
    with pytest.raises(_dirty.GuardViolation) as ei:
        with allocations("ff", "cpu"):
            torch.empty(16)
            _writes_one_element_before_its_buffer(8)
    msg = str(ei.value)
    assert "allocation #1" in msg and "_writes_one_element_before_its_buffer" in msg and "test_dirty_cpu.py" in msg
    assert "4 guard byte(s) changed" in msg and "before the buffer, first at byte offset -4" in msg
    assert "allocation #0" not in msg


def test_guard_violation_behind_the_buffer_is_reported_too():
    with pytest.raises(_dirty.GuardViolation, match="after the buffer, first at byte offset 12"):
        with allocations("ff", "cpu"):
            out = torch.empty(3, dtype=torch.float32)
            out.as_strided((1,), (1,), out.storage_offset() + 3).fill_(0.0)


# ---- the harness must be able to fail ------------------------------------------------------------------------------
def k_correct(x):
    ws = torch.empty(x.shape[0] + 3)
    ws[:x.shape[0]] = x * 2
    out = torch.empty_like(x)
    out.copy_(ws[:x.shape[0]] + 1)
    return out


def k_reads_workspace_before_writing(x):
    ws = torch.empty(x.shape[0] + 1)
    ws[:x.shape[0]] = x * 2
    out = torch.empty_like(x)
    out.copy_(ws[:x.shape[0]] + ws[x.shape[0]])                # ws[n] is read here ...
    ws[x.shape[0]] = x.sum()                                   # ... and written only afterwards
    return out


def k_accumulates_into_uncleared_output(x):
    out = torch.empty_like(x)
    out += x                                                   # "contributes" to zeros it assumes
    return out


def k_multiplies_unwritten_cell_by_zero(x):
    ws = torch.empty(x.shape[0] + 1)
    ws[:x.shape[0]] = x
    mask = torch.cat([torch.ones_like(x), torch.zeros(1)])
    out = torch.empty_like(x)
    out.copy_(x + (ws * mask)[1:])                             # 0 * ws[n]: harmless unless ws[n] is NaN or Inf
    return out


def _three_modes(kernel):
    """Which modes tell the kernel's results apart from the zero baseline: the protocol of the GPU file, on the CPU."""
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(6, generator=gen)
    y = 4 * torch.randn(6, generator=gen)
    with allocations("zero", "cpu"):
        z1 = snapshot([kernel(x)])
    with allocations("zero", "cpu"):
        z2 = snapshot([kernel(x)])
    assert first_difference(z1, z2) is None
    with allocations("record", "cpu") as rec:
        kernel(y)
    with allocations("stale", "cpu", recording=rec.recording) as h:
        s = snapshot([kernel(x)])
        assert h.served > 0
    with allocations("ff", "cpu") as h:
        f = snapshot([kernel(x)])
        assert h.served > 0
    return {m for m, r in (("stale", s), ("ff", f)) if first_difference(z1, r) is not None}


def test_a_correct_kernel_passes_all_three_modes():
    assert _three_modes(k_correct) == set()


def test_a_read_before_write_is_caught_by_stale_and_by_ff():
    assert _three_modes(k_reads_workspace_before_writing) == {"stale", "ff"}


def test_an_uncleared_accumulator_is_caught_by_stale_and_by_ff():
    assert _three_modes(k_accumulates_into_uncleared_output) == {"stale", "ff"}


def test_an_unwritten_cell_times_zero_is_caught_by_ff_only():
    assert _three_modes(k_multiplies_unwritten_cell_by_zero) == {"ff"}


def test_first_difference_sees_bits_not_values():
    a = {"x": torch.tensor([0.0, float("nan")])}
    assert first_difference(a, snapshot(a)) is None                     # NaN == NaN bitwise
    assert "1 of 2 cells" in first_difference(a, {"x": torch.tensor([-0.0, float("nan")])})
    assert first_difference(a, {"y": a["x"]}) is not None
    assert first_difference(a, {"x": a["x"].double()}) is not None


# ---- completeness ----------------------------------------------------------------------------------------------
def _allocating_functions():
    """{"module.Class.function": "file:line"} for every function of difffacto_amd/ that calls torch.empty,
    torch.empty_like or <tensor>.new_empty (the outermost enclosing def; a lambda counts for its def)."""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "difffacto_amd", "**", "*.py"), recursive=True)):
        rel = os.path.relpath(path, ROOT)
        mod = os.path.splitext(os.path.relpath(path, os.path.join(ROOT, "difffacto_amd")))[0].replace(os.sep, ".")
        tree = ast.parse(open(path).read(), path)

        def walk(node, scope):
            for child in ast.iter_child_nodes(node):
                s = scope
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                    s = scope + [child.name]
                if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
                    f = child.func
                    is_torch = isinstance(f.value, ast.Name) and f.value.id == "torch" and f.attr in ("empty", "empty_like")
                    if is_torch or f.attr == "new_empty":
                        found.setdefault(".".join([mod] + (scope or ["<module>"])), f"{rel}:{child.lineno}")
                walk(child, s)
        walk(tree, [])
    return found


def test_the_walk_finds_the_sites_the_issue_names():
    found = _allocating_functions()
    for name in ("training.DenoiserTrainFn.forward", "pointnet2_ops.pointnet2_modules._SharedMLPTrainFn.forward",
                 "engine.DenoiserEngine.prepare_shapes", "metrics.emdFunction.forward",
                 "latents.LatentSampler.sample_latents", "part_sampling.select_diverse_global"):
        assert name in found, (name, sorted(found))           # sample_latents allocates through a lambda
    assert len(found) > 40
    assert not any("new_empty" in open(p).read() for p in glob.glob(os.path.join(ROOT, "difffacto_amd", "**", "*.py"), recursive=True)), \
        "the package now uses Tensor.new_empty: tests/_dirty.py has to patch it"


def test_every_allocating_function_is_covered_or_exempt():
    gpu = importlib.import_module("test_gpu_dirty_memory")
    found = _allocating_functions()
    unknown = [f"{where}: {name}" for name, where in found.items() if name not in gpu.COVERED and name not in gpu.EXEMPT]
    assert not unknown, "allocation sites that no dirty-memory case covers:\n  " + "\n  ".join(unknown)
    gone = [n for n in list(gpu.COVERED) + list(gpu.EXEMPT) if n not in found]
    assert not gone, f"coverage tables name functions that no longer allocate: {gone}"
    both = set(gpu.COVERED) & set(gpu.EXEMPT)
    assert not both, both
    tests = {n for n in dir(gpu) if n.startswith("test_")}
    for name, test_id in gpu.COVERED.items():
        assert test_id.split("[")[0] in tests, (name, test_id)
    for name, reason in gpu.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name
