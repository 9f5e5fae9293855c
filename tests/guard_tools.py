"""Guard bands around the arrays an entry may write (tests/test_output_bounds_gpu.py), and the header's prototypes.

An array is carved from the middle of a larger uint8 buffer filled with PATTERN (neither 0x00 nor 0xFF: padding values are 0,
0.0 and -1, whose bytes an overrun of padding would leave unseen). Each guard is at least as long as the array and at least
MIN_GUARD bytes, on both sides, so an excess as large as the array itself still lands in a guard. The array starts ONE ELEMENT
PAST a 16-byte boundary: at its element's alignment and no better, which is all include/rag_hip.h promises for an output array
(no kernel stores to a caller's array through a type wider than the element; the arrays that are READ through float4 are inputs,
and the entries check those). check() compares every guard byte with PATTERN and names the array and the first changed offset.

Nothing here imports torch or the package at import time: the header parser is also used by the CPU tests."""
import os
import re

import numpy as np

PATTERN = 0xA5
MIN_GUARD = 64 * 1024
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rag_hip.h")


def guard_bytes(nbytes):
    return (max(nbytes, MIN_GUARD) + 15) // 16 * 16


def _size(shape):
    shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(shape)
    n = 1
    for s in shape:
        n *= int(s)
    return shape, n


class Guards:
    """The guarded allocations of one test: dev(...) / host(...) hand out arrays, check() looks at every guard."""

    def __init__(self):
        self.made = []                   # (what, buffer, start, nbytes, on_device)

    # ---- device ------------------------------------------------------------------------------------------------------------------
    def dev(self, shape, dtype, fill=None, what=None):
        """a torch CUDA tensor of `shape` and `dtype` between two guards; `fill` None leaves PATTERN in it (torch.empty)"""
        import torch
        shape, n = _size(shape)
        elem = torch.empty((), dtype=dtype).element_size()
        nbytes, g = n * elem, guard_bytes(n * elem)
        start = g + elem                                              # the buffer is 512-byte aligned, g a multiple of 16
        buf = REAL["torch.full"]((start + nbytes + g,), PATTERN, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        t = buf[start:start + nbytes].view(dtype).reshape(shape)
        assert nbytes == 0 or (t.data_ptr() == buf.data_ptr() + start and t.data_ptr() % 16 == elem % 16 and t.is_contiguous())
        if fill is not None:
            t.fill_(fill)
        self.made.append((what or f"device array #{len(self.made)} {tuple(shape)} {dtype}", buf, start, nbytes, True))
        return t

    # ---- host --------------------------------------------------------------------------------------------------------------------
    def host(self, shape, dtype=None, fill=None, what=None):
        """a numpy array of `shape` and `dtype` between two guards; `fill` None leaves PATTERN in it (np.empty)"""
        shape, n = _size(shape)
        dtype = np.dtype(np.float64 if dtype is None else dtype)
        elem = dtype.itemsize
        nbytes, g = n * elem, guard_bytes(n * elem)
        buf = np.full(g + 16 + elem + nbytes + g, PATTERN, np.uint8)
        start = g + (-(buf.ctypes.data + g)) % 16 + elem
        a = buf[start:start + nbytes].view(dtype).reshape(shape)
        assert nbytes == 0 or (a.ctypes.data == buf.ctypes.data + start and a.ctypes.data % 16 == elem % 16 and a.flags.c_contiguous)
        if fill is not None:
            a[...] = fill
        self.made.append((what or f"host array #{len(self.made)} {tuple(shape)} {dtype}", buf, start, nbytes, False))
        return a

    # ---- the check -----------------------------------------------------------------------------------------------------------------
    def check(self):
        """every guard byte is PATTERN; else: which array, and the first changed byte relative to its start (before) or end (behind)"""
        on_device = [m for m in self.made if m[4]]
        if on_device:
            import torch
            torch.cuda.synchronize()
        for what, buf, start, nbytes, dev in self.made:
            for side, lo, hi in (("before its start", 0, start), ("behind its end", start + nbytes, buf.shape[0])):
                part = buf[lo:hi]
                bad = (part != PATTERN)
                if bool(bad.any()):
                    first = int(bad.nonzero()[0, 0]) if dev else int(np.flatnonzero(bad)[0])
                    n_bad = int(bad.sum())
                    where = first - (start - lo) if lo == 0 else first
                    raise AssertionError(f"{what} ({nbytes} bytes): {n_bad} guard bytes changed {side}, the first at byte offset "
                                         f"{where:+d} from the array's {'start' if lo == 0 else 'end'}")
        return len(self.made)


REAL = {}                                # the allocators as they were before any patch (filled by patch_torch)


def patch_torch(monkeypatch, guards):
    """torch.empty / torch.full / torch.zeros hand out guarded tensors for device="cuda" for the rest of the test"""
    import torch
    for name in ("empty", "full", "zeros"):
        REAL.setdefault("torch." + name, getattr(torch, name))

    def on_cuda(kw):
        d = kw.get("device")
        return d is not None and torch.device(d).type == "cuda"

    def plain(kw):
        return set(kw) <= {"dtype", "device"}

    def shape_of(args):
        return args[0] if len(args) == 1 and not isinstance(args[0], (int, np.integer)) else args

    def empty(*size, **kw):
        if on_cuda(kw) and plain(kw):
            return guards.dev(shape_of(size), kw.get("dtype", torch.float32))
        return REAL["torch.empty"](*size, **kw)

    def zeros(*size, **kw):
        if on_cuda(kw) and plain(kw):
            return guards.dev(shape_of(size), kw.get("dtype", torch.float32), fill=0)
        return REAL["torch.zeros"](*size, **kw)

    def full(size, fill_value, **kw):
        if on_cuda(kw) and plain(kw) and "dtype" in kw:
            return guards.dev(size, kw["dtype"], fill=fill_value)
        return REAL["torch.full"](size, fill_value, **kw)

    for name, fn in (("empty", empty), ("full", full), ("zeros", zeros)):
        monkeypatch.setattr(torch, name, fn)


class GuardedNumpy:
    """numpy as a module sees it, with the five allocators handing out guarded arrays (monkeypatch.setattr(module, "np", this):
    numpy itself is never patched)"""

    def __init__(self, guards):
        self._guards = guards

    def __getattr__(self, name):
        return getattr(np, name)

    def empty(self, shape, dtype=float, order="C"):
        return self._guards.host(shape, dtype)

    def zeros(self, shape, dtype=float, order="C"):
        return self._guards.host(shape, dtype, fill=0)

    def full(self, shape, fill_value, dtype=None, order="C"):
        return self._guards.host(shape, np.asarray(fill_value).dtype if dtype is None else dtype, fill=fill_value)

    def empty_like(self, a, dtype=None):
        return self._guards.host(np.shape(a), np.asarray(a).dtype if dtype is None else dtype)

    def zeros_like(self, a, dtype=None):
        return self._guards.host(np.shape(a), np.asarray(a).dtype if dtype is None else dtype, fill=0)


class Recorder:
    """the library of one handle, recording every rag_* entry called through it"""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        if name.startswith("rag_"):
            self._seen.add(name)
        return getattr(self._lib, name)


# ---- include/rag_hip.h ---------------------------------------------------------------------------------------------------------------
def header_text():
    """the header without its comments and preprocessor lines"""
    with open(HEADER) as f:
        hdr = f.read()
    hdr = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    return re.sub(r"^[ \t]*#[^\n]*", " ", hdr, flags=re.M)


def header_declarations():
    """name -> (parameter declarations in order, return type), from every `type rag_name(...);` (they span lines)"""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?[\s\*]+)(rag_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text()):
        params = [" ".join(p.split()) for p in params.split(",") if p.strip()]
        if params == ["void"]:
            params = []
        assert name not in protos, f"{name} declared twice"
        protos[name] = (params, " ".join(ret.split()))
    return protos


def writable_parameters(params):
    """the parameters an entry may write through: pointers to non-const, other than the handle and `void* stream`"""
    out = []
    for p in params:
        if "*" not in p or re.search(r"\bconst\b", p.split("*")[0]):
            continue
        if re.fullmatch(r"void\s*\*\s*stream", p):
            continue
        out.append(p)
    return out


def entries_that_write():
    """name -> its writable parameters, for every entry that has one"""
    return {name: w for name, (params, _) in header_declarations().items() for w in [writable_parameters(params)] if w}
