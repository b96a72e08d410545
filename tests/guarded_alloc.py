"""Guard bands and poisoned payloads for the buffers the Python layer hands to the HIP library.

The C ABI's contract (include/disn_amd.h, "Conventions") is that the caller owns every buffer, sized exactly by the
shapes and the *_workspace_bytes() queries.  torch's caching allocator rounds every block up, so a kernel that
overruns by a few hundred bytes, or reads a slot nobody cleared, is never seen.  ``guarded(variant)`` makes both
visible without a fault:

    with guarded("A") as g:
        x = g.put(host_array)              # guarded + frozen input
        y = ops.something(x)               # the wrapper's torch.empty is substituted
        g.check()                          # guards intact, frozen inputs unchanged

Every substituted allocation is a view into a larger uint8 buffer ``[guard | payload | pad to 16 | guard]``; an
incorrect access lands in a guard (owned memory), so a finding is a failed assertion.  Run a scenario under variant A
and under variant B: the two differ in guard and poison bytes, so a result that depends on memory the kernel was not
given, or on the prior contents of a buffer it was given, changes bits between the runs.

Plain module (not a conftest); imported by test_guarded_alloc_host.py and test_gpu_memory_contract.py.
"""
from __future__ import annotations

import contextlib
import os
import sys
from typing import List, Optional

import numpy as np
import torch

GUARD_BYTES = 4096            # each side; a multiple of 256
ALIGN = 256                   # the payload starts on a multiple of this
VARIANTS = {"A": (0xA5, 0xFF),   # guard byte, payload poison: float32 NaN, int -1
            "B": (0x5A, 0x7F)}   # float32 ~3.4e38, int 0x7f7f7f7f
_HERE = os.path.abspath(__file__)
_ACTIVE: Optional["Guarded"] = None


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ("buf", "start", "nbytes", "shape", "dtype", "site")

    def __init__(self, buf, start, nbytes, shape, dtype, site):
        self.buf, self.start, self.nbytes, self.shape, self.dtype, self.site = buf, start, nbytes, shape, dtype, site

    def describe(self) -> str:
        return "%s %s allocated at %s" % (tuple(self.shape), str(self.dtype).replace("torch.", ""), self.site)


def _call_site() -> str:
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d" % (os.path.relpath(f.f_code.co_filename, os.path.dirname(os.path.dirname(_HERE))), f.f_lineno)


def _shape_of(args, kwargs):
    """the size of torch.empty / zeros / full in every form torch takes: a tuple or list, a torch.Size, varargs, a bare
    int, or size=...; None when it is none of these"""
    if "size" in kwargs:
        args = (kwargs["size"],)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    try:
        shape = tuple(int(v) for v in args)
    except (TypeError, ValueError):
        return None
    return shape if all(isinstance(v, (int, np.integer)) for v in args) else None


class _Recorder:
    """stands in for the CDLL behind disn_amd._lib.lib(): forwards everything, notes the disn_* functions called"""

    def __init__(self, real, names: List[str]):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_names", names)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("disn_"):
            return fn
        names = self._names

        class _Call:
            def __call__(_self, *a):
                names.append(name)
                return fn(*a)

            def __getattr__(_self, k):
                return getattr(fn, k)

        return _Call()

    def __setattr__(self, name, value):
        setattr(self._real, name, value)


class Guarded:
    PASS_KW = {"dtype", "device", "size"}        # any other keyword (out=, pin_memory=, ...): not substituted

    def __init__(self, variant: str, cpu: bool = False):
        if variant not in VARIANTS:
            raise ValueError("variant must be one of %s" % sorted(VARIANTS))
        self.variant = variant
        self.guard_byte, self.poison_byte = VARIANTS[variant]
        self.cpu = cpu
        self.records: List[_Record] = []
        self.frozen_inputs = []
        self.called: List[str] = []
        self._orig = {}

    # -- allocation -----------------------------------------------------------------------------------------------
    def _wanted(self, device) -> bool:
        if device is None:
            kind = "cpu"
        else:
            kind = torch.device(device).type
        return kind == "cuda" or (self.cpu and kind == "cpu")

    def alloc(self, shape, dtype, device, poison: bool = True) -> torch.Tensor:
        """a contiguous tensor of exactly numel * itemsize bytes between two guards"""
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        pad = (-n) % 16
        empty = self._orig.get("empty", torch.empty)
        buf = empty(ALIGN + GUARD_BYTES + n + pad + GUARD_BYTES, dtype=torch.uint8, device=device)
        start = (-(buf.data_ptr() + GUARD_BYTES)) % ALIGN + GUARD_BYTES
        buf.fill_(self.guard_byte)
        payload = buf[start:start + n]
        if poison:
            payload.fill_(self.poison_byte)
        t = payload.view(dtype).view(shape)
        assert t.is_contiguous() and t.data_ptr() % ALIGN == 0 and t.numel() * t.element_size() == n
        self.records.append(_Record(buf, start, n, shape, dtype, _call_site()))
        return t

    def put(self, array, freeze: bool = True) -> torch.Tensor:
        """a host array as a guarded device (or, in the host self-test, CPU) tensor; frozen unless asked otherwise"""
        a = np.ascontiguousarray(array)
        src = torch.from_numpy(a.copy())
        t = self.alloc(src.shape, src.dtype, "cpu" if self.cpu else "cuda", poison=False)
        t.copy_(src)
        if freeze:
            self.frozen(t)
        return t

    def poison(self, t: torch.Tensor) -> torch.Tensor:
        """fill an output or scratch tensor the caller allocated some other way with the variant's poison"""
        self._bytes_view(t).fill_(self.poison_byte)
        return t

    @staticmethod
    def _bytes_view(t: torch.Tensor) -> torch.Tensor:
        assert t.is_contiguous()
        return t.detach().view(-1).view(torch.uint8)

    def _substitute(self, name):
        orig = self._orig[name]

        def empty_like(*args, **kwargs):
            if len(args) != 1 or set(kwargs) - {"dtype", "device"} or not isinstance(args[0], torch.Tensor):
                return orig(*args, **kwargs)
            x = args[0]
            device = kwargs.get("device", x.device)
            if not self._wanted(device) or x.numel() == 0:
                return orig(*args, **kwargs)
            return self.alloc(x.shape, kwargs.get("dtype", x.dtype), device, poison=True)

        def sized(*args0, **kwargs0):
            args, kwargs, fill = args0, dict(kwargs0), None
            if name == "full":               # torch.full(size, fill_value, ...): the size is never varargs
                if "fill_value" in kwargs:
                    fill = kwargs.pop("fill_value")
                elif len(args) == 2:
                    args, fill = args[:1], args[1]
                else:
                    return orig(*args0, **kwargs0)
            shape = _shape_of(args, kwargs)
            if shape is None or set(kwargs) - self.PASS_KW or not self._wanted(kwargs.get("device")) \
                    or int(np.prod(shape, dtype=np.int64)) == 0:
                return orig(*args0, **kwargs0)
            dtype = kwargs.get("dtype")
            if dtype is None:
                if name == "full":
                    dtype = torch.bool if isinstance(fill, bool) else torch.int64 if isinstance(fill, int) \
                        else torch.get_default_dtype()
                else:
                    dtype = torch.get_default_dtype()
            t = self.alloc(shape, dtype, kwargs.get("device"), poison=(name == "empty"))
            if name == "zeros":
                t.zero_()
            elif name == "full":
                t.fill_(fill)
            return t

        return empty_like if name == "empty_like" else sized

    # -- inputs ---------------------------------------------------------------------------------------------------
    def frozen(self, *tensors):
        """snapshot tensors the header declares const; check() asserts they are bit-identical afterwards"""
        for i, t in enumerate(tensors):
            self.frozen_inputs.append((t, self._bytes(t).clone(), "%s #%d of frozen() at %s" % (
                tuple(t.shape), i, _call_site())))
        return tensors[0] if len(tensors) == 1 else tensors

    @staticmethod
    def _bytes(t: torch.Tensor) -> torch.Tensor:
        return t.detach().contiguous().view(-1).view(torch.uint8)

    # -- the check ------------------------------------------------------------------------------------------------
    def check(self) -> None:
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        problems = []
        if self.records:
            # one reduction per guard on its own device, ONE copy to the host per device for all of them
            per_device = {}
            for k, r in enumerate(self.records):
                per_device.setdefault(r.buf.device, []).append(k)
            counts = [None] * len(self.records)
            for ks in per_device.values():
                flat = torch.stack([c for k in ks for c in ((self.records[k].buf[:self.records[k].start] != self.guard_byte).sum(),
                                                            (self.records[k].buf[self.records[k].start + self.records[k].nbytes:]
                                                             != self.guard_byte).sum())]).cpu().tolist()
                for j, k in enumerate(ks):
                    counts[k] = (flat[2 * j], flat[2 * j + 1])
            for r, (front, back) in zip(self.records, counts):
                for side, n_bad in (("before", front), ("after", back)):
                    if not n_bad:
                        continue
                    region = r.buf[:r.start] if side == "before" else r.buf[r.start + r.nbytes:]
                    first = int((region != self.guard_byte).nonzero()[0, 0])
                    off = first - r.start if side == "before" else first
                    problems.append("guard %s the payload of %s damaged: %d byte(s), first at offset %d %s" % (
                        side, r.describe(), n_bad, off,
                        "(bytes relative to the payload's start)" if side == "before" else "(bytes past the payload's end)"))
        for t, snap, what in self.frozen_inputs:
            now = self._bytes(t)
            if not torch.equal(now, snap):
                diff = (now != snap).nonzero()
                problems.append("const input %s was written: %d byte(s), first at byte %d" % (
                    what, diff.shape[0], int(diff[0, 0])))
        if problems:
            raise GuardError("variant %s: %d memory-contract violation(s)\n  " % (self.variant, len(problems))
                             + "\n  ".join(problems))

    # -- which entries ran ----------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def recording(self):
        """swap disn_amd._lib._LIB for a forwarding proxy; yields the list of disn_* names called, in order"""
        from disn_amd import _lib
        real = _lib.lib()
        if isinstance(real, _Recorder):
            raise RuntimeError("recording() is already active")
        names: List[str] = []
        self.called = names                      # a scenario may look at the tail of the list: which entries a case ran
        _lib._LIB = _Recorder(real, names)
        try:
            yield names
        finally:
            _lib._LIB = real

    # -- context --------------------------------------------------------------------------------------------------
    def __enter__(self):
        global _ACTIVE
        if _ACTIVE is not None:
            raise RuntimeError("guarded() does not nest")
        _ACTIVE = self
        for name in ("empty", "zeros", "full", "empty_like"):
            self._orig[name] = getattr(torch, name)
        for name in list(self._orig):
            setattr(torch, name, self._substitute(name))
        return self

    def __exit__(self, *exc):
        global _ACTIVE
        for name, fn in self._orig.items():
            setattr(torch, name, fn)
        self._orig = {}
        _ACTIVE = None
        self.records = []
        self.frozen_inputs = []
        return False


def guarded(variant: str, cpu: bool = False) -> Guarded:
    """context manager; ``cpu=True`` substitutes CPU allocations too (the host self-test)"""
    return Guarded(variant, cpu=cpu)
