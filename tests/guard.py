"""Guarded, poisoned buffers for the op tests.

A kernel test that hands the op a `torch.empty` buffer and then compares the elements the op is supposed to write misses three kinds of bug:
a store that never happened (the caching allocator returns the block the previous, correct call just freed), a store that landed outside
the output, and an input that was changed.  `Arena` makes all three visible:

* `empty` / `zeros` / `like` return a contiguous view inside a larger allocation laid out `[guard | payload | guard]`.  The WHOLE allocation is
  filled on the device with a poison bit pattern first -- a NaN for the float types, so every `rel_err(...) < tol` / `torch.equal` assertion fails
  by itself on an element the op left unwritten.
* `wide` + `cols` cover ops that write a column slice of a wider buffer: the columns outside the registered slices stay poison and are checked.
* `frozen` snapshots inputs.
* `check()` compares every guard, every untouched column range and every frozen input bit for bit (through an integer view: NaN != NaN does not
  matter) and says which tensor, which side, the first offset and how many bytes changed.
* `check_written(t)`: no element of t still carries the poison pattern.
* `scratch(shape, device, dtype)` has the signature of `mtp_amd.ops._scratch`: monkeypatched in, the ops' own workspaces get guards and poison too
  (their guards are checked; "fully written" is not: some are over-allocated on purpose).

Plain helper module: no fixtures, no plugin, any device (tests/test_guard_host.py runs it on the CPU).
"""
import torch

GUARD_MIN = 64 * 1024      # bytes per side, at least; and at least two rows of the payload; always a multiple of GUARD_ALIGN
GUARD_ALIGN = 256          # keeps the payload on the 16-byte alignment the C ABI asks for (device allocations start on >= 256 bytes)
SCRATCH_LIVE_MAX = 16 << 30   # workspaces held for the final check; beyond this they are checked and released early

# poison per dtype: (integer view dtype, pattern as a signed value of that view)
_I = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(v, bits):
    return v - (1 << bits) if v >= (1 << (bits - 1)) else v


POISON = {
    torch.float32: 0x7fc0dead,              # quiet NaN, payload 0x00dead
    torch.bfloat16: 0x7fdd,                 # NaN
    torch.float16: 0x7ddd,                  # NaN
    torch.float64: 0x7ff8dead7fc0dead,      # quiet NaN
    torch.uint8: 0xa5,
    torch.int8: 0xa5,
    torch.int16: 0xa5d5,
    torch.int32: 0xa5d5dead,
    torch.int64: 0xa5d5deada5d5dead,
}


def poison_of(dtype):
    """(integer view dtype, pattern) of `dtype`"""
    size = torch.empty((), dtype=dtype).element_size()
    view = _I[size]
    pat = POISON[dtype]
    return view, (pat if view == torch.uint8 else _signed(pat, 8 * size))


def guard_bytes(shape, dtype):
    """size of each guard for a contiguous tensor of `shape`: >= GUARD_MIN, >= 2 rows (last dimension x element size), a multiple of GUARD_ALIGN"""
    size = torch.empty((), dtype=dtype).element_size()
    row = (shape[-1] if len(shape) else 1) * size
    g = max(GUARD_MIN, 2 * row)
    return -(-g // GUARD_ALIGN) * GUARD_ALIGN


class GuardError(AssertionError):
    pass


class _Rec:
    __slots__ = ("name", "base", "guard", "nbytes", "dtype", "shape", "cols", "wide", "scratch", "view")


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _shape(shape):
    if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
        shape = shape[0]
    return tuple(int(d) for d in shape)


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.recs, self.snaps, self.n, self.scratch_live = [], [], 0, 0

    # ------------------------------------------------------------------------------------------ allocation
    def _alloc(self, shape, dtype, name, kind):
        shape = _shape(shape)
        view, pat = poison_of(dtype)
        size = torch.empty((), dtype=dtype).element_size()
        g, nbytes = guard_bytes(shape, dtype), _numel(shape) * size
        base = torch.empty(2 * g + nbytes, device=self.device, dtype=torch.uint8)
        base.view(view).fill_(pat)          # device-side fill of guards and payload alike, no host round trip
        r = _Rec()
        self.n += 1
        r.name = "%s#%d %s %s" % (name or kind, self.n, tuple(shape), str(dtype).replace("torch.", ""))
        r.base, r.guard, r.nbytes, r.dtype, r.shape, r.cols, r.wide, r.scratch = base, g, nbytes, dtype, shape, [], kind == "wide", kind == "scratch"
        r.view = base[g:g + nbytes].view(dtype).view(shape)
        assert r.view.data_ptr() % 16 == 0 and r.view.is_contiguous()
        self.recs.append(r)
        return r

    def empty(self, *shape, dtype=torch.float32, name=None):
        """poisoned output buffer: the op must write every element"""
        return self._alloc(shape, dtype, name, "empty").view

    def zeros(self, *shape, dtype=torch.float32, name=None):
        """guarded buffer whose payload starts at zero (an output the op accumulates into)"""
        t = self._alloc(shape, dtype, name, "zeros").view
        t.zero_()
        return t

    def like(self, t, dtype=None, name=None):
        """guarded buffer holding a copy of t's values (any device), as dtype or t's own"""
        out = self._alloc(tuple(t.shape), dtype or t.dtype, name, "like").view
        out.copy_(t)
        return out

    def wide(self, rows, cols, dtype=torch.float32, name=None):
        """poisoned (rows, cols) buffer for ops that write a column slice: register what they may write with cols(); every other column is
        checked like a guard"""
        return self._alloc((rows, cols), dtype, name, "wide").view

    def cols(self, w, c0, c1):
        """w[:, c0:c1] of a wide() buffer, registered as writable"""
        r = self._rec_of(w)
        assert r is not None and r.wide and 0 <= c0 <= c1 <= r.shape[1]
        r.cols.append((c0, c1))
        return w[:, c0:c1]

    def scratch(self, shape, device=None, dtype=torch.float32):
        """signature of mtp_amd.ops._scratch: a poisoned, guarded workspace"""
        if isinstance(shape, int):
            shape = (shape,)
        if self.scratch_live > SCRATCH_LIVE_MAX:
            self._release_scratch()
        r = self._alloc(tuple(shape), dtype, "workspace", "scratch")
        self.scratch_live += r.base.numel()
        return r.view

    def frozen(self, *tensors):
        """snapshot inputs: check() asserts they are bit-identical afterwards.  Returns the tensor (or the tuple of them)."""
        for t in tensors:
            self.snaps.append((t, t.detach().clone(), "input#%d %s %s" % (len(self.snaps) + 1, tuple(t.shape), str(t.dtype).replace("torch.", ""))))
        return tensors[0] if len(tensors) == 1 else tensors

    def _rec_of(self, t):
        for r in self.recs:
            if r.view.data_ptr() == t.data_ptr() and r.view.dtype == t.dtype:
                return r
        return None

    # ------------------------------------------------------------------------------------------ checks
    def _regions(self, r):
        """(label, integer-view tensor that must still be all poison) of a record"""
        view, _ = poison_of(r.dtype)
        g, nb = r.guard, r.nbytes
        out = [("leading guard", r.base[:g].view(view)), ("trailing guard", r.base[g + nb:].view(view))]
        if r.wide:
            iv, c, free = r.view.view(view), 0, []
            for c0, c1 in sorted(r.cols):
                if c0 > c:
                    free.append((c, c0))
                c = max(c, c1)
            if c < r.shape[1]:
                free.append((c, r.shape[1]))
            out += [("untouched columns [%d, %d)" % (a, b), iv[:, a:b]) for a, b in free]
        return out

    def _bad_count(self, recs, snaps):
        tot = torch.zeros((), device=self.device, dtype=torch.int64)
        for r in recs:
            _, pat = poison_of(r.dtype)
            for _, reg in self._regions(r):
                tot += (reg != pat).sum()
        for t, snap, _ in snaps:
            view = _I[t.element_size()]
            tot += (t.view(view) != snap.view(view)).sum().to(self.device)
        return int(tot.item())

    def _describe(self, r, label, reg, pat):
        size = reg.element_size()
        bad = (reg != pat).cpu()
        idx = bad.nonzero()
        # bytes that changed, counted in the byte view of the same region
        pb = torch.tensor([pat], dtype=reg.dtype).view(torch.uint8)
        rb = reg.cpu().contiguous().view(torch.uint8).reshape(-1, size)
        nbytes = int((rb != pb).sum())
        first = idx[0].tolist()
        if label == "leading guard":
            where = "changed elements from %d to %d bytes BEFORE the start of the tensor" % (r.guard - first[0] * size, r.guard - idx[-1].tolist()[0] * size)
        elif label == "trailing guard":
            off = first[0] * size
            row = (r.shape[-1] if r.shape else 1) * size
            where = "first changed element %d bytes past the END of the tensor (%d rows + %d bytes past the last element)" % (off, off // row, off % row)
        else:
            c0 = int(label.split("[")[1].split(",")[0])
            where = "first changed element at row %d, column %d" % (first[0], c0 + first[1])
        return "%s: %s was written: %s, %d elements / %d bytes changed" % (r.name, label, where, len(idx), nbytes)

    def _failures(self, recs, snaps):
        msgs = []
        for r in recs:
            _, pat = poison_of(r.dtype)
            for label, reg in self._regions(r):
                if bool((reg != pat).any()):
                    msgs.append(self._describe(r, label, reg, pat))
        for t, snap, name in snaps:
            view = _I[t.element_size()]
            bad = (t.view(view) != snap.view(view)).cpu()
            if bool(bad.any()):
                msgs.append("%s: frozen input was modified: first changed element at index %s, %d elements changed"
                            % (name, tuple(bad.nonzero()[0].tolist()), int(bad.sum())))
        return msgs

    def _release_scratch(self):
        old = [r for r in self.recs if r.scratch]
        if self._bad_count(old, []):
            raise GuardError("\n".join(self._failures(old, [])))
        self.recs = [r for r in self.recs if not r.scratch]
        self.scratch_live = 0

    def check(self):
        """every guard, every untouched column range of the wide buffers and every frozen input, bit for bit; raises GuardError naming what was hit"""
        if self._bad_count(self.recs, self.snaps):          # one device -> host transfer when all is well
            raise GuardError("\n".join(self._failures(self.recs, self.snaps)))

    def check_written(self, t, name=None):
        """no element of t still carries its dtype's poison pattern (for outputs whose values a test does not compare in full).  uint8 / int8
        outputs can hold the pattern by right: not for them."""
        view, pat = poison_of(t.dtype)
        left = (t.view(view) == pat)
        n = int(left.sum())
        if n:
            r = self._rec_of(t)
            raise GuardError("%s: %d of %d elements were never written (still poison); first at index %s"
                             % (name or (r.name if r is not None else "tensor %s" % (tuple(t.shape),)), n, t.numel(), tuple(left.nonzero()[0].tolist())))

    def close(self):
        self.recs, self.snaps, self.scratch_live = [], [], 0
