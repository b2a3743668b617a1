"""One allocation seam under all of ``ops``: guard bands around, and poison inside, every tensor it allocates.

``ops.py`` reaches torch only through its module global ``torch`` and allocates only with ``torch.empty``,
``torch.empty_like``, ``torch.zeros`` and ``torch.zeros_like`` (tests/test_guarded_host.py asserts both on its text).
``guarded(ops, poison_byte)`` swaps that global for a proxy for the duration of a ``with`` block.  The proxy forwards
every attribute to the real torch, except the four allocation calls: each of those is served from a private uint8
buffer of GUARD + nbytes + GUARD bytes, filled with ``poison_byte`` throughout, of which the caller gets
``buf[GUARD:GUARD + nbytes].view(dtype).reshape(shape)`` (the ``zeros`` variants zero that view alone).  GUARD = 4096 is
a multiple of the caching allocator's 512-byte alignment, so a kernel sees the alignment it always sees.  Two errors
that parity, determinism and graph-replay tests cannot see then show:

  a write outside a buffer -- an output or a workspace the kernel overruns, or a ``rec_*_workspace_bytes`` answer
      smaller than what the host-side carve consumes -- lands in a guard instead of in a neighbouring tensor: on
      leaving the block (after ``torch.cuda.synchronize()`` on a GPU run) both guards of every allocation must still hold
      the poison byte, and the failure names the allocation, the side, the first damaged offset and the ``ops`` frames
      that asked for it;
  a read of floats nobody wrote -- a slice, a padding column or a tile of partials that no workgroup writes -- reads
      poison instead of the zeros or the last call's identical values the allocator usually holds there: 0xFF reads as
      NaN in fp32 (-1 in int32 / int64), 0x7F as 3.3962e38, finite.  Results that are finite under the first and
      bit-equal under both depend on no such float.

A second proxy stands in for ``ops.lib`` and lists which ``rec_*_workspace_bytes`` queries the block called.

``short_by=n`` hands out views whose trailing guard starts n bytes early, inside the view: a correct kernel that writes
the end of its buffer then "damages" the guard without any access outside the allocation, which shows the detector
firing on the GPU with unmodified kernels.  ``short_if`` limits that to the allocations it accepts.

Out of reach of this seam: what ``engine.py``, ``sharded.py`` and ``csrc/torch_ops.cpp`` allocate -- the fused DeepFM /
DSSM steps, the plan rings, the split-K workspace of ``ops.gemm`` and every result of a ``torch.ops.mi355rec`` operator.
"""
import contextlib
import re
import sys

import torch as _torch

GUARD = 4096
POISON_NAN, POISON_FINITE = 0xFF, 0x7F
ALLOCATORS = ("empty", "empty_like", "zeros", "zeros_like")
QUERY = re.compile(r"rec_\w+_workspace_bytes")


class GuardError(AssertionError):
    pass


class Allocation:
    """one served allocation: ``base`` the whole uint8 buffer, ``view`` what the caller got"""

    def __init__(self, index, call, base, view, nbytes, frames, short):
        self.index, self.call, self.base, self.view, self.nbytes, self.frames = index, call, base, view, nbytes, frames
        self.shape, self.dtype, self.short = tuple(view.shape), view.dtype, short

    def describe(self):
        return "#%d torch.%s(%s, %s), %d bytes, asked for by %s" % (
            self.index, self.call, list(self.shape), str(self.dtype).replace("torch.", ""), self.nbytes,
            " <- ".join(self.frames) or "?")


def _first_bad(region, poison):
    """offset of the first byte of ``region`` that is not ``poison``, or None"""
    bad = region != poison
    if not bool(bad.any()):
        return None
    return int(bad.nonzero()[0])


class Session:
    """what a ``guarded`` block saw: ``allocations`` in order, ``queries`` the workspace queries called"""

    def __init__(self, poison, short_by, short_if, filename):
        if not 0 <= poison <= 255 or short_by < 0:
            raise ValueError("poison is a byte and short_by is not negative")
        self.poison, self.short_by, self.short_if, self.filename = poison, short_by, short_if, filename
        self.allocations, self.queries = [], []

    def _frames(self):
        out, f = [], sys._getframe(3)
        while f is not None:
            if f.f_code.co_filename == self.filename:
                out.append("%s:%d" % (f.f_code.co_name, f.f_lineno))
            f = f.f_back
        return out

    def serve(self, call, shape, dtype, device, zero):
        dtype = _torch.float32 if dtype is None else dtype
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * dtype.itemsize
        base = _torch.empty(GUARD + nbytes + GUARD, dtype=_torch.uint8, device=device)
        base.fill_(self.poison)
        view = base[GUARD:GUARD + nbytes].view(dtype).reshape(shape)
        if zero:
            view.zero_()
        rec = Allocation(len(self.allocations), call, base, view, nbytes, self._frames(), 0)
        if self.short_by and (self.short_if is None or self.short_if(rec)):
            rec.short = min(self.short_by, nbytes)
        self.allocations.append(rec)
        return view

    def total_bytes(self):
        return sum(a.nbytes for a in self.allocations)

    def damage(self):
        """[(allocation, side, offset relative to the view's first / one-past-last byte)] of every damaged guard"""
        if any(a.base.is_cuda for a in self.allocations):
            _torch.cuda.synchronize()
        found = []
        for a in self.allocations:
            at = _first_bad(a.base[:GUARD], self.poison)
            if at is not None:
                found.append((a, "before", at - GUARD))
            tail = GUARD + a.nbytes - a.short
            at = _first_bad(a.base[tail:], self.poison)
            if at is not None:
                found.append((a, "after", at - a.short))
        return found

    def check(self):
        found = self.damage()
        if found:
            raise GuardError("guard bytes (0x%02X) overwritten:\n" % self.poison + "\n".join(
                "  %s the view, first damaged byte at offset %+d from its %s: %s"
                % (side, at, "start" if side == "before" else "end", a.describe()) for a, side, at in found))


def _size(args):
    """the shape of torch.empty(2, 3) / torch.empty((2, 3)) / torch.empty(torch.Size(..)) / torch.empty(7)"""
    if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
        return tuple(args[0])
    return tuple(args)


class TorchProxy:
    """the real torch, but for the four allocation calls"""

    def __init__(self, session):
        object.__setattr__(self, "_session", session)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    def _new(self, call, args, kw, zero):
        extra = set(kw) - {"dtype", "device"}
        if extra:
            raise TypeError("tests/guarded.py serves torch.%s(size, dtype=, device=) alone; extend the seam for %s"
                            % (call, sorted(extra)))
        return self._session.serve(call, _size(args), kw.get("dtype"), kw.get("device"), zero)

    def _like(self, call, t, kw, zero):
        extra = set(kw) - {"dtype", "device"}
        if extra or not t.is_contiguous():
            raise TypeError("tests/guarded.py serves torch.%s(contiguous tensor, dtype=, device=) alone; extend the seam"
                            % call)
        return self._session.serve(call, t.shape, kw.get("dtype", t.dtype), kw.get("device", t.device), zero)

    def empty(self, *args, **kw):
        return self._new("empty", args, kw, False)

    def zeros(self, *args, **kw):
        return self._new("zeros", args, kw, True)

    def empty_like(self, t, **kw):
        return self._like("empty_like", t, kw, False)

    def zeros_like(self, t, **kw):
        return self._like("zeros_like", t, kw, True)


class LibProxy:
    """the real ``ops.lib``; notes the ``rec_*_workspace_bytes`` entry points that are looked up (ops calls what it looks
    up)"""

    def __init__(self, lib, session):
        object.__setattr__(self, "_lib", lib)
        object.__setattr__(self, "_session", session)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if QUERY.fullmatch(name) and name not in self._session.queries:
            self._session.queries.append(name)
        return fn


@contextlib.contextmanager
def guarded(ops, poison=POISON_NAN, short_by=0, short_if=None, check=True):
    """``with guarded(ops, 0xFF) as g: ...`` -- every allocation of ``ops`` inside the block is guarded and poisoned; on
    leaving it (unless it raised) the guards are checked (GuardError).  ``g.allocations`` and ``g.queries`` stay."""
    session = Session(poison, short_by, short_if, getattr(ops, "__file__", None))
    real_torch, real_lib = ops.torch, ops.lib
    if real_torch is not _torch:
        raise RuntimeError("ops.torch is not torch: a guarded block inside another?")
    ops.torch, ops.lib = TorchProxy(session), LibProxy(real_lib, session)
    try:
        yield session
    finally:
        ops.torch, ops.lib = real_torch, real_lib
    if check:
        session.check()


# ---- what the tests do with the results of a driver ---------------------------------------------------------------
def flatten(tree):
    """the tensors of nested tuples / lists / dicts, in order (None and numbers are dropped)"""
    if isinstance(tree, _torch.Tensor):
        return [tree]
    if isinstance(tree, dict):
        tree = list(tree.values())
    if isinstance(tree, (tuple, list)):
        return [t for x in tree for t in flatten(x)]
    return []


def bit_equal(a, b):
    """same shape, dtype and bytes (NaN equals the same NaN, -0.0 differs from 0.0)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(_torch.equal(a.contiguous().reshape(-1).view(_torch.uint8), b.contiguous().reshape(-1).view(_torch.uint8)))
