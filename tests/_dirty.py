"""Allocation harness for the "outputs and workspaces are fully written by the call" contract of include/dfx.h.

`allocations(mode)` patches `torch.empty` and `torch.empty_like` (the package has no `new_empty` site) so that every
buffer a wrapper hands to the library comes back with chosen contents instead of whatever the caching allocator held:

  "zero"    zero-filled: the baseline.
  "record"  zero-filled and kept alive in `harness.recording`; the run behind "stale".
  "stale"   the buffers of a recording, handed back in the same order, unmodified: every cell holds the finished
            result of the same call at the same shapes on other inputs, so indices are in range, masks are 0/1 and
            floats are finite.  A shape, dtype, stride or order that differs from the recording raises.  A cell
            that no run ever writes still holds the recording's zero: only "ff" reaches such a cell.
  "ff"      every byte 0xFF (NaN in every float type, -1 in signed integers, 255 in uint8), the tensor being the middle
            of one larger allocation whose leading and trailing guard bands are filled the same way and are checked on
            exit.  An element index of -1 scaled by any stride that fits inside the buffer lands inside the guard.

Allocations on other devices, pinned allocations and zero-element allocations pass through.  `torch.zeros` is never
patched.  A harness that served no allocation raises on exit: it would have tested nothing.  Plain Python: importing
this module needs no GPU.
"""
import contextlib
import os
import sys

import torch

MODES = ("zero", "record", "stale", "ff")
GUARD_MIN = 1 << 20
GUARD_MAX = 64 << 20
_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))


class StaleMismatch(RuntimeError):
    """An allocation under "stale" does not match the recording."""


class GuardViolation(AssertionError):
    """A guard byte of an "ff" allocation was changed."""


def guard_bytes(nbytes):
    g = min(max(GUARD_MIN, int(nbytes)), GUARD_MAX)
    return (g + 255) // 256 * 256


def _caller():
    """file:line (function) of the nearest frame outside this file and outside torch."""
    f = sys._getframe(1)
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE and not fn.startswith(_TORCH_DIR) and "contextlib" not in fn:
            return f"{f.f_code.co_filename}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return "<unknown>"


class Harness:
    def __init__(self, mode, device_type, recording):
        self.mode, self.device_type = mode, device_type
        self.served = 0
        self.passed_through = 0
        self.recording = [] if mode == "record" else recording
        self._ff = []          # (ordinal, frame, whole uint8 buffer, guard, payload bytes)
        self._orig = None

    # -- one allocation --------------------------------------------------------------------------------------------
    def _serve(self, t, kwargs):
        if t.device.type != self.device_type or kwargs.get("pin_memory") or t.numel() == 0 or kwargs.get("out") is not None:
            self.passed_through += 1
            return t
        ordinal = self.served
        self.served += 1
        if self.mode == "zero":
            return t.zero_()
        if self.mode == "record":
            self.recording.append(t.zero_().detach())     # an alias that autograd never marks as an output
            return t
        if self.mode == "stale":
            if ordinal >= len(self.recording):
                raise StaleMismatch(f"allocation #{ordinal} at {_caller()}: the recording holds only {len(self.recording)}")
            r = self.recording[ordinal]
            if r.shape != t.shape or r.dtype != t.dtype or r.stride() != t.stride() or r.device != t.device:
                raise StaleMismatch(f"allocation #{ordinal} at {_caller()}: asked {tuple(t.shape)} {t.dtype} strides {t.stride()} on "
                                    f"{t.device}, recorded {tuple(r.shape)} {r.dtype} strides {r.stride()} on {r.device}")
            return r.detach().requires_grad_(t.requires_grad)
        # "ff"
        empty = self._orig[0]
        numel, item = t.numel(), t.element_size()
        span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
        if span != numel or t.layout != torch.strided:
            raise NotImplementedError(f"allocation #{ordinal} at {_caller()}: not dense ({tuple(t.shape)}, strides {t.stride()})")
        nbytes = numel * item
        g = guard_bytes(nbytes)
        payload = (nbytes + 255) // 256 * 256
        buf = empty(g + payload + g, dtype=torch.uint8, device=t.device).fill_(255)
        mid = buf[g:g + nbytes].view(t.dtype).as_strided(t.shape, t.stride())
        self._ff.append((ordinal, _caller(), buf, g, nbytes))
        return mid.requires_grad_(t.requires_grad)

    def check_guards(self):
        bad = []
        for ordinal, frame, buf, g, nbytes in self._ff:
            lead, trail = buf[:g], buf[g + nbytes:]
            n = int((lead != 255).sum()) + int((trail != 255).sum())
            if n:
                where = []
                for name, band, base in (("before", lead, -g), ("after", trail, nbytes)):
                    idx = (band != 255).nonzero()
                    if idx.numel():
                        where.append(f"{name} the buffer, first at byte offset {base + int(idx[0])}")
                bad.append(f"allocation #{ordinal} ({nbytes} bytes) asked for at {frame}: {n} guard byte(s) changed, " + "; ".join(where))
        if bad:
            raise GuardViolation("\n".join(bad))


@contextlib.contextmanager
def allocations(mode, device_type="cuda", recording=None):
    """Patch torch.empty / torch.empty_like for the duration; yields the Harness (see the module docstring)."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} not in {MODES}")
    if (mode == "stale") != (recording is not None):
        raise ValueError('"stale" needs recording=<harness.recording of a "record" run>, the other modes take none')
    h = Harness(mode, device_type, recording)
    orig_empty, orig_empty_like = torch.empty, torch.empty_like
    h._orig = (orig_empty, orig_empty_like)

    def empty(*args, **kwargs):
        return h._serve(orig_empty(*args, **kwargs), kwargs)

    def empty_like(*args, **kwargs):
        return h._serve(orig_empty_like(*args, **kwargs), kwargs)

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield h
    finally:
        torch.empty, torch.empty_like = orig_empty, orig_empty_like
    if mode == "stale" and h.served != len(recording):
        raise StaleMismatch(f"{h.served} allocations served, {len(recording)} recorded")
    if mode == "ff":
        h.check_guards()
    if h.served == 0:
        raise AssertionError(f'allocations("{mode}") served no allocation on {device_type}: nothing was tested')


# ---- comparing results -------------------------------------------------------------------------------------------
def snapshot(results):
    """Clone a {name: tensor | number | None} mapping (or a list of tensors) before the harness releases its buffers."""
    if not isinstance(results, dict):
        results = {str(i): r for i, r in enumerate(results)}
    out = {}
    for k, v in results.items():
        if v is None:
            continue
        if not torch.is_tensor(v):
            v = torch.as_tensor(v)
        out[k] = v.detach().clone()
    return out


def _bits(t):
    t = t.contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def first_difference(a, b):
    """None if the two snapshots are bit-identical, else a one-line description of the first differing tensor."""
    if a.keys() != b.keys():
        return f"result sets differ: {sorted(set(a) ^ set(b))}"
    for k in a:
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"{k}: {tuple(x.shape)} {x.dtype} vs {tuple(y.shape)} {y.dtype}"
        if not torch.equal(_bits(x), _bits(y)):
            ne = (x.reshape(-1) != y.reshape(-1)) | (x.reshape(-1) != x.reshape(-1)) | (y.reshape(-1) != y.reshape(-1))
            ne = ne.nonzero().reshape(-1)
            i = int(ne[0]) if ne.numel() else 0
            return (f"{k}: {int(ne.numel())} of {x.numel()} cells differ, first at flat index {i}: "
                    f"{x.reshape(-1)[i].item()!r} vs {y.reshape(-1)[i].item()!r}")
    return None
