"""Guard bands and poisoned memory around the tensors a kernel is handed (plain helper module: no conftest involved).

Every other test of the suite looks only at the values INSIDE the tensors it asked for.  This module controls what lies
around them and what was in them before the call, so that three kinds of kernel error become visible:

  * a store past the end (or before the start) of an output or workspace  -> a guard byte changes, `check()` names the block;
  * a load past the end of an operand                                     -> it returns NaN (floats) or -1 (integers; as a
    row index that is "one row before the array", inside the leading guard band), and the NaN reaches the result;
  * reliance on what `torch.empty` happens to hold                        -> it holds NaN / -1, not an old result or zeros.

POISON is the byte 0xFF everywhere: float32 / bfloat16 / float64 read it as NaN, int32 / int64 as -1.

The harness never makes a kernel touch memory it would not touch otherwise: it only decides what those bytes contain.
Nothing here needs a GPU; arenas work on CPU tensors the same way (tests/test_guarded_harness.py).
"""
import os
import sys

import pytest
import torch

POISON = 0xFF
ALIGN = 512                       # default payload alignment (what torch's caching allocator hands out)
MIN_GUARD = 4096                  # bytes per side, or one row at the leading dimension if that is more
KEEP_BYTES = 3 << 30              # poisoned_allocations: beyond this, the oldest blocks are checked and released early

_PKG_DIR = os.sep + "difformer_amd" + os.sep
_HERE = os.path.abspath(__file__)


def _round_up(x, m):
    return -(-x // m) * m


def _itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _call_site():
    """file:line of the innermost frame inside difformer_amd (the allocation's owner), else of the first frame outside
    this module."""
    f = sys._getframe(1)
    outside = None
    while f is not None:
        name = f.f_code.co_filename
        if _PKG_DIR in name:
            return f"difformer_amd/{name.rsplit(_PKG_DIR, 1)[1]}:{f.f_lineno}"
        if outside is None and os.path.abspath(name) != _HERE:
            outside = f"{os.path.basename(name)}:{f.f_lineno}"
        f = f.f_back
    return outside or "?"


class _Block:
    """One request: a flat uint8 buffer [guard | payload | guard]."""
    __slots__ = ("buf", "start", "nbytes", "site", "shape", "dtype")

    def __init__(self, buf, start, nbytes, site, shape, dtype):
        self.buf, self.start, self.nbytes, self.site, self.shape, self.dtype = buf, start, nbytes, site, shape, dtype

    def sides(self):
        return (("leading", self.buf[: self.start]), ("trailing", self.buf[self.start + self.nbytes:]))

    def describe(self, side, guard):
        bad = (guard != POISON).nonzero()
        first = int(bad[0]) if bad.numel() else -1
        # offsets relative to the payload: negative = before its first byte, >= 0 = bytes past its last
        off = first - guard.numel() if side == "leading" else first
        return (f"{side} guard of the block allocated at {self.site} (shape {tuple(self.shape)}, {self.dtype}, "
                f"{self.nbytes} payload bytes) was overwritten: first changed byte at payload "
                f"{'start' if side == 'leading' else 'end'} {off:+d}, {int(bad.numel())} bytes changed")


class GuardedArena:
    """Hands out tensors that sit between two bands of POISON bytes, one flat uint8 buffer per request, and checks the
    bands afterwards.  The tensors are NOT autograd views of the buffer (`_base` is None): they are ordinary tensors whose
    storage happens to be larger than they are and whose storage offset is not 0, so host code that looks at `_base` of
    ITS OWN views (autograd_ops._adjacent_columns) sees what it sees on a plain allocation."""

    def __init__(self):
        self.blocks = []
        self.held = 0

    def alloc(self, shape, dtype, device="cpu", ld=None, offset_bytes=0, zero=False, site=None):
        """-> tensor of `shape` / `dtype` on `device`, poisoned (or zero with zero=True) inside, guarded outside.
        ld: leading dimension in elements of a 2-d+ tensor whose rows are `prod(shape[1:])` wide: the payload is
        [rows, ld] and the result its [:, :width] part -- the tail of every row stays poisoned.
        offset_bytes: the payload starts that many bytes past a 512-byte boundary (the minimum alignment an entry point
        documents for the operand: 16 for float rows, 4 for the rows of dif_linear_packed_f32, ...)."""
        shape = tuple(int(s) for s in shape)
        item = _itemsize(dtype)
        if offset_bytes % item:
            raise ValueError(f"offset_bytes={offset_bytes} is no multiple of the {item}-byte element")
        numel = 1
        for s in shape:
            numel *= s
        width = numel // shape[0] if shape and shape[0] else 0
        if ld is not None:
            if len(shape) < 2 or ld < width:
                raise ValueError(f"ld={ld} needs a tensor of rows at least {width} wide")
            nbytes, row_bytes = shape[0] * ld * item, ld * item
        else:
            nbytes, row_bytes = numel * item, (width if len(shape) > 1 else 0) * item
        guard = _round_up(max(MIN_GUARD, row_bytes), ALIGN)
        total = guard + ALIGN + offset_bytes + nbytes + guard
        buf = torch.full((total,), POISON, dtype=torch.uint8, device=device)       # ONE fill per block
        start = guard + (-(buf.data_ptr() + guard)) % ALIGN + offset_bytes
        assert start >= guard and total - start - nbytes >= guard
        t = torch.empty(0, dtype=dtype, device=buf.device)
        if ld is not None:
            t.set_(buf.untyped_storage(), start // item, shape, (ld,) + _dense_strides(shape[1:]))
        else:
            t.set_(buf.untyped_storage(), start // item, shape, _dense_strides(shape))
        if zero and nbytes:
            buf[start: start + nbytes].zero_()
        self.blocks.append(_Block(buf, start, nbytes, site or _call_site(), shape, dtype))
        self.held += total
        return t

    def check(self, release=None):
        """Synchronise, assert that every guard byte is still POISON (one read-back per device for all blocks) and
        forget the checked blocks.  release: only the oldest `release` blocks."""
        blocks = self.blocks if release is None else self.blocks[:release]
        self.blocks = [] if release is None else self.blocks[release:]
        if torch.cuda.is_available() and any(b.buf.is_cuda for b in blocks):
            torch.cuda.synchronize()
        by_dev = {}
        for b in blocks:
            by_dev.setdefault(b.buf.device, []).append(b)
        errors = []
        for group in by_dev.values():
            mins = torch.stack([g.min() for b in group for _, g in b.sides()]).tolist()
            for i, b in enumerate(group):
                for j, (side, g) in enumerate(b.sides()):
                    if mins[2 * i + j] != POISON:
                        errors.append(b.describe(side, g))
        self.held -= sum(b.buf.numel() for b in blocks)
        assert not errors, "guard band hit:\n  " + "\n  ".join(errors)


def _dense_strides(shape):
    strides, s = [], 1
    for d in reversed(shape):
        strides.append(s)
        s *= max(int(d), 1)
    return tuple(reversed(strides))


def guarded_inputs(arena, device, min_align=False, **cpu_tensors):
    """Copies test operands into blocks of `arena` on `device` and returns the device tensors in argument order.
    An operand is a CPU tensor, None (stays None), or a tuple (tensor, ld) for a row-strided operand (payload [rows, ld],
    the [:, :width] part returned).  min_align: False = 512-byte aligned payloads; True = 16 bytes past such a boundary
    (the alignment the header promises for rows and workspaces); an int = that many bytes."""
    off = 0 if min_align is False else (16 if min_align is True else int(min_align))
    out = []
    for name, t in cpu_tensors.items():
        if t is None:
            out.append(None)
            continue
        t, ld = t if isinstance(t, tuple) else (t, None)
        item = t.element_size()
        d = arena.alloc(t.shape, t.dtype, device, ld=ld, offset_bytes=_round_up(off, item) if off else 0,
                        site=f"guarded_inputs({name})")
        d.copy_(t)
        out.append(d)
    return out


class TorchProxy:
    """Stands in for the name `torch` inside the package's modules: every attribute is the real module's, except
    `empty`, `empty_like` and `zeros` for a non-CPU device (cpu_too: for every device), which come out of `arena` --
    `empty` / `empty_like` poisoned inside and out, `zeros` zero inside and guarded outside.  While the current stream is
    being captured into a hipGraph the real functions run: a graph must not record the fills."""

    def __init__(self, arena, cpu_too=False):
        self.__dict__["_arena"] = arena
        self.__dict__["_cpu_too"] = cpu_too

    def __getattr__(self, name):
        return getattr(torch, name)

    def _wanted(self, device, kw):
        if set(kw) - {"dtype", "device", "requires_grad"} or kw.get("requires_grad"):
            return None                                  # pin_memory, out=, layout, memory_format, names: not ours
        device = torch.device(device) if device is not None else torch.empty(0).device
        if device.type == "cpu":
            return device if self._cpu_too else None
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return None
        return device

    def _from_arena(self, real, size, kw, zero):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            shape = tuple(size[0])
        else:
            shape = size
        device = self._wanted(kw.get("device"), kw) if all(isinstance(s, int) for s in shape) else None
        if device is None:
            return real(*size, **kw)
        return self._arena.alloc(shape, kw.get("dtype") or torch.get_default_dtype(), device, zero=zero)

    def empty(self, *size, **kw):
        return self._from_arena(torch.empty, size, kw, False)

    def zeros(self, *size, **kw):
        return self._from_arena(torch.zeros, size, kw, True)

    def empty_like(self, t, **kw):
        device = self._wanted(kw.get("device", t.device), kw) if t.is_contiguous() and t.layout == torch.strided else None
        if device is None:
            return torch.empty_like(t, **kw)
        return self._arena.alloc(t.shape, kw.get("dtype") or t.dtype, device)


PROXIED_MODULES = ("backend_hip", "ops", "tiny", "autograd_ops", "difformer_v2", "graph_utils", "dist")


class _ReleasingArena(GuardedArena):
    """The fixture's arena: it keeps every block until teardown, unless that would hold more than KEEP_BYTES -- then the
    oldest half is checked (after a synchronise) and released."""

    def alloc(self, *a, **kw):
        if self.held > KEEP_BYTES and len(self.blocks) > 1:
            self.check(release=len(self.blocks) // 2)
        return super().alloc(*a, **kw)


def install(monkeypatch, cpu_too=False):
    """Puts a TorchProxy over a new arena into the package's modules for the life of `monkeypatch` -> the arena."""
    import importlib
    arena = _ReleasingArena()
    proxy = TorchProxy(arena, cpu_too=cpu_too)
    for name in PROXIED_MODULES:
        monkeypatch.setattr(importlib.import_module("difformer_amd." + name), "torch", proxy)
    return arena


@pytest.fixture
def poisoned_allocations(monkeypatch):
    """Every torch.empty / empty_like / zeros the package makes on the GPU during the test comes poisoned and guarded;
    at teardown every guard band is checked.  Import the fixture into the test module (or wrap it in an autouse one)."""
    arena = install(monkeypatch)
    yield arena
    arena.check()
