"""A poisoned arena for the native entry points: every buffer a launch is handed is carved out of one
uint8 tensor whose bytes are all 0xFF (NaN as f32, bf16, f16 and f64; the largest 16-bit phase code),
exactly as long as the entry point asks for, with a guard gap of at least 64 KiB on both sides that is
never handed out. After the launches, verify() shows that nothing outside the buffers was written, that
inputs were not changed, that outputs were written in full and that zeroed workspaces are zero again.
Because the neighbourhood of every buffer is NaN rather than the allocator's zeros or an earlier
correct answer, a read past a buffer's end that reaches a result shows up as a difference from the
same launches on ordinary buffers (Plain below).

A plain helper module (not a conftest): the tests import it by name after putting tests/ on sys.path.
"""
import torch

ALIGN = 512          # the caching allocator's block alignment: the same launch plan as in ordinary runs
GUARD = 64 * 1024    # wider than any 32-row tile of the widest tensor the tests carve (32 x 512 x 4 bytes)
ROLES = ("input", "output", "scratch", "zeroed")
_ONES = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class ArenaError(AssertionError):
    """A broken invariant: which one, the region's name and the first offending byte offset (within the
    region's payload; for a guard, from the end of the payload it follows)."""

    def __init__(self, invariant, region, offset, detail=""):
        self.invariant, self.region, self.offset = invariant, region, int(offset)
        super().__init__(f"{invariant}: region '{region}', byte offset {int(offset)}{': ' + detail if detail else ''}")


def _align_up(v, a):
    return (v + a - 1) // a * a


def _nbytes(shape, dtype):
    n = 1
    for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
        n *= int(s)
    return n * torch.empty((), dtype=dtype).element_size(), n


class _Region:
    def __init__(self, name, role, start, nbytes, dtype, view, snapshot, zero_check):
        self.name, self.role, self.start, self.nbytes, self.dtype = name, role, start, nbytes, dtype
        self.view, self.snapshot, self.zero_check = view, snapshot, zero_check


def _first(mask):
    """Index of the first true element of a 1-D bool tensor (it has one)."""
    return int(torch.nonzero(mask)[0, 0])


class Arena:
    """One uint8 tensor of `nbytes` bytes, every byte 0xFF, and the regions carved from it."""

    def __init__(self, device, nbytes):
        self.device = torch.device(device)
        self.buf = torch.full((int(nbytes) + ALIGN,), 0xFF, dtype=torch.uint8, device=self.device)
        self.base = (-self.buf.data_ptr()) % ALIGN  # byte of buf that sits on a 512-byte boundary
        self.end = self.base + (int(nbytes) // ALIGN) * ALIGN
        self.cursor = self.base + GUARD             # a gap also precedes the first region
        self.regions = []

    def take(self, shape, dtype, *, role, offset_bytes=0, fill=None, name=None, zero_check=None):
        """A tensor view of a new region: its payload starts on a 512-byte boundary plus offset_bytes, is
        exactly numel * itemsize bytes long and is followed by at least GUARD bytes nobody gets.
          input  : `fill` (a tensor of this shape and dtype, or a scalar) is copied in and a snapshot kept
          output : left 0xFF (a `fill` is an error)
          scratch: left 0xFF, or `fill` copied in (a buffer updated in place); never checked
          zeroed : zero-filled; must be all zero again (only bytes zero_check = (lo, hi) if given)"""
        assert role in ROLES, role
        nbytes, numel = _nbytes(shape, dtype)
        item = nbytes // max(numel, 1)
        assert nbytes > 0 and offset_bytes >= 0 and offset_bytes % item == 0, (shape, dtype, offset_bytes)
        start = self.cursor + offset_bytes
        if start + nbytes + GUARD > self.end:
            raise MemoryError(f"arena of {self.end - self.base} bytes is full at region {len(self.regions)}")
        self.cursor = self.base + _align_up(start + nbytes + GUARD - self.base, ALIGN)
        view = self.buf[start:start + nbytes].view(dtype).view(shape)
        assert view.data_ptr() % ALIGN == offset_bytes % ALIGN
        snapshot = None
        if role == "output":
            assert fill is None, "an output region is handed out as 0xFF"
        elif role == "zeroed":
            assert fill is None
            view.zero_()
        elif fill is not None:
            if torch.is_tensor(fill):
                assert fill.dtype == dtype and fill.numel() == numel, (fill.dtype, dtype, fill.shape, shape)
                view.copy_(fill.reshape(view.shape))
            else:
                view.fill_(fill)
        if role == "input":
            assert fill is not None, "an input region needs its data"
            snapshot = self.buf[start:start + nbytes].clone()
        name = name if name is not None else f"{role}{len(self.regions)}"
        self.regions.append(_Region(name, role, start, nbytes, dtype, view, snapshot, zero_check))
        return view

    def freeze(self, name):
        """From here on region `name` is an input (snapshot taken now): the `saved` buffer a forward
        wrote, over the backward that must only read it."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        (r,) = [r for r in self.regions if r.name == name]
        if r.role == "output":  # an output that the next call reads: I3 now, I2 from here on
            self.check_outputs(only=r)
        r.role, r.snapshot = "input", self._payload(r).clone()

    # ------------------------------------------------------------------ the invariants
    def _payload(self, r):
        return self.buf[r.start:r.start + r.nbytes]

    def check_guards(self):
        """I1: every byte outside the payloads is still 0xFF."""
        probe = self.buf.clone()
        for r in self.regions:
            probe[r.start:r.start + r.nbytes] = 0xFF
        bad = probe != 0xFF
        if bool(bad.any()):
            at = _first(bad)
            before = [r for r in self.regions if r.start + r.nbytes <= at]
            if before:
                r = before[-1]
                raise ArenaError("I1 guard byte overwritten", r.name, at - (r.start + r.nbytes),
                                 f"after the payload's end (value {int(probe[at]):#04x})")
            r = self.regions[0] if self.regions else None
            raise ArenaError("I1 guard byte overwritten", r.name if r else "<empty arena>", at - (r.start if r else 0),
                             "before the payload's start")

    def check_inputs(self):
        """I2: every input region equals its snapshot, byte for byte."""
        for r in self.regions:
            if r.role == "input":
                bad = self._payload(r) != r.snapshot
                if bool(bad.any()):
                    raise ArenaError("I2 input changed", r.name, _first(bad))

    def unwritten(self, r):
        """Bool tensor over the elements of region r: the element still has the all-ones bit pattern."""
        item = torch.empty((), dtype=r.dtype).element_size()
        ints = self._payload(r).view(_ONES[item])
        return ints == (0xFF if item == 1 else -1)

    def check_outputs(self, only=None):
        """I3: no element of an output region still has the all-ones bit pattern (bits, not isnan: a
        NaN the kernel computed has another payload)."""
        for r in self.regions:
            if r.role == "output" and (only is None or r is only):
                bad = self.unwritten(r)
                if bool(bad.any()):
                    item = r.nbytes // bad.numel()
                    raise ArenaError("I3 output element not written", r.name, _first(bad) * item,
                                     f"{int(bad.sum())} of {bad.numel()} elements")

    def check_zeroed(self):
        """I4: every zeroed region (or its zero_check byte range) is all zero again."""
        for r in self.regions:
            if r.role == "zeroed":
                lo, hi = r.zero_check if r.zero_check is not None else (0, r.nbytes)
                bad = self._payload(r)[lo:hi] != 0
                if bool(bad.any()):
                    raise ArenaError("I4 zeroed workspace left non-zero", r.name, lo + _first(bad))

    def verify(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.check_guards()
        self.check_inputs()
        self.check_outputs()
        self.check_zeroed()

    def assert_nothing_launched(self):
        """I7: after a refused call every output is still all ones, and I1, I2, I4 hold."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.check_guards()
        self.check_inputs()
        self.check_zeroed()
        for r in self.regions:
            if r.role == "output":
                bad = ~self.unwritten(r)
                if bool(bad.any()):
                    item = r.nbytes // bad.numel()
                    raise ArenaError("I7 output written by a refused call", r.name, _first(bad) * item)


class Plain:
    """The same take() over ordinary zero-filled tensors (each its own allocation, at the same
    offset_bytes from the allocator's alignment): the run the arena run is compared with. It adds up
    what an arena for the same takes must hold (arena_bytes)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.arena_bytes = 2 * GUARD + ALIGN

    def take(self, shape, dtype, *, role, offset_bytes=0, fill=None, name=None, zero_check=None):
        assert role in ROLES, role
        nbytes, numel = _nbytes(shape, dtype)
        self.arena_bytes += _align_up(offset_bytes + nbytes + GUARD, ALIGN) + ALIGN
        raw = torch.zeros(offset_bytes + nbytes, dtype=torch.uint8, device=self.device)
        view = raw[offset_bytes:].view(dtype).view(shape)
        if fill is not None:
            assert role in ("input", "scratch")
            if torch.is_tensor(fill):
                view.copy_(fill.reshape(view.shape))
            else:
                view.fill_(fill)
        return view

    def verify(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def freeze(self, name):
        pass

    def arena(self):
        """An Arena large enough for the takes this allocator has seen."""
        return Arena(self.device, self.arena_bytes)


def same_bits(a, b):
    """I5: two tensors hold the same bytes (NaNs compared by their bits)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    item = a.element_size()
    return bool(torch.equal(a.contiguous().view(_ONES[item]), b.contiguous().view(_ONES[item])))
