"""Guard-band harness: tensors carved out of one uint8 allocation, each with a poisoned band before and after it.

The library's contract (include/yolo355.h, Conventions) is that a call reads no byte that can change a result, and writes no
byte, outside the extents its arguments describe.  A test tensor from torch's allocator cannot show a breach of it: it is
512-byte aligned, rounded up, and its neighbours are usually zero or stale finite data.  Here every tensor

  * starts at an address a with a % (2 * align) == align: the requested alignment exactly and no more (for align = 16 an odd
    multiple of 16 past a 256-byte boundary),
  * has exactly the bytes its shape says (a 'scratch' tensor of nbytes uint8 has exactly what the size function returned),
  * lies between two guards of max(1 MiB, its own size) bytes each, so that an over-read or over-write by a whole 256-row tile
    of 1024 fp32 channels still lands in memory the test owns.

poison(byte) fills the guards and the interior of every 'out' and 'scratch' tensor; check() compares every guard byte
afterwards.  A case runs twice (run_passes): 0xFF is NaN as fp32 / bf16 / fp64 and -1 as int32, 0x7F is about 3.4e38 and a
large positive int - finite, because max / min / comparisons drop NaN and would hide a poisoned neighbour.  An input element
read from outside its tensor then shows as a difference between the two passes (or as NaN / 3.4e38 against the reference).

Works on CPU tensors as well (tests/test_guarded_cpu.py proves the detection there with plain torch functions)."""
import numpy as np
import torch

GUARD_MIN = 1 << 20          # one 256-row tile at 1024 fp32 channels
POISON_A, POISON_B = 0xFF, 0x7F
ROLES = ('in', 'out', 'inout', 'scratch')


class GuardViolation(object):
    """One modified guard.  Offsets are in bytes: on side 'before' relative to the tensor's first byte (so negative, -1 is the
    byte just in front of it), on side 'after' relative to the first byte past its end (0 is the byte just behind it)."""

    def __init__(self, name, side, first, last, count):
        self.name, self.side, self.first, self.last, self.count = name, side, first, last, count

    def __repr__(self):
        return "guard %s of '%s': %d byte(s) modified, offsets %d..%d" % (self.side, self.name, self.count, self.first, self.last)


class GuardError(AssertionError):
    def __init__(self, violations):
        AssertionError.__init__(self, '; '.join(repr(v) for v in violations))
        self.violations = violations


class _Slot(object):
    def __init__(self, name, start, nbytes, guard, role, align, view, data):
        self.name, self.start, self.nbytes, self.guard, self.role, self.align = name, start, nbytes, guard, role, align
        self.view, self.data = view, data


def _as_torch(data, dtype):
    if isinstance(data, torch.Tensor):
        return data.to(dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(data)).to(dtype)


class Arena(object):
    def __init__(self, device, capacity=48 << 20):
        """capacity: bytes of the one allocation; a tensor() that does not fit raises (raise the capacity of that case)."""
        self.device = torch.device(device)
        self.buf = torch.empty(capacity + 512, dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = 0          # first free byte (offset into buf)
        self.slots = []
        self.byte = None

    def tensor(self, name, shape, dtype, align=16, role='in', data=None):
        """A contiguous view of `shape` x `dtype` at exactly `align`-byte alignment between two guards.  data (numpy or torch,
        roles 'in' / 'inout' only) is the content load() writes into it before each pass."""
        assert role in ROLES, role
        assert align >= 1 and (align & (align - 1)) == 0, align
        assert all(s.name != name for s in self.slots), name
        if isinstance(shape, int):
            shape = (shape,)
        item = torch.empty((), dtype=dtype).element_size()
        assert align % item == 0, "alignment %d below the element size %d" % (align, item)
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        guard = max(GUARD_MIN, nbytes)
        addr = self.base + self.cursor + guard
        addr += (align - addr) % (2 * align)              # addr % (2 * align) == align
        start = addr - self.base
        end = start + nbytes + guard
        if end > self.buf.numel():
            raise MemoryError("arena: '%s' needs %d bytes past a capacity of %d" % (name, end, self.buf.numel()))
        view = self.buf[start:start + nbytes].view(dtype).view(tuple(shape))
        assert (nbytes == 0 or view.data_ptr() == addr) and view.is_contiguous()
        if data is not None:
            assert role in ('in', 'inout'), "only 'in' / 'inout' tensors carry data"
            data = _as_torch(data, dtype)
            assert tuple(data.shape) == tuple(shape), (name, tuple(data.shape), tuple(shape))
        self.slots.append(_Slot(name, start, nbytes, guard, role, align, view, data))
        self.cursor = end
        return view

    def scratch(self, name, nbytes, align=16):
        """Exactly nbytes of scratch (what a *_bytes function returned: not rounded)."""
        return self.tensor(name, (int(nbytes),), torch.uint8, align=align, role='scratch')

    def __getitem__(self, name):
        for s in self.slots:
            if s.name == name:
                return s.view
        raise KeyError(name)

    def _guards(self, s):
        return (('before', self.buf[s.start - s.guard:s.start]), ('after', self.buf[s.start + s.nbytes:s.start + s.nbytes + s.guard]))

    def poison(self, byte):
        """Fill every guard and the interior of every 'out' and 'scratch' tensor with `byte`."""
        self.byte = int(byte)
        for s in self.slots:
            for _, g in self._guards(s):
                g.fill_(self.byte)
            if s.role in ('out', 'scratch'):
                self.buf[s.start:s.start + s.nbytes].fill_(self.byte)

    def load(self):
        """(Re)write the data of every 'in' and 'inout' tensor."""
        for s in self.slots:
            if s.data is not None:
                s.view.copy_(s.data)

    def check(self):
        """Compare every guard byte with the poison; raises GuardError naming tensor, side, first / last offset and count.
        The caller has synchronised the stream the kernels ran on (the comparison itself runs on torch's current stream)."""
        assert self.byte is not None, "check() before poison()"
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        guards = [(s, side, g) for s in self.slots for side, g in self._guards(s)]
        counts = torch.stack([(g != self.byte).sum() for _, _, g in guards]).tolist()
        bad = []
        for (s, side, g), c in zip(guards, counts):
            if c:
                idx = torch.nonzero(g != self.byte).flatten()
                first, last = int(idx[0]), int(idx[-1])
                off = -s.guard if side == 'before' else 0
                bad.append(GuardViolation(s.name, side, first + off, last + off, int(c)))
        if bad:
            raise GuardError(bad)


class Spec(object):
    """One tensor of a case, before there is an arena: tensor()'s arguments.  shape / dtype default to those of `data`."""

    def __init__(self, name, role, data=None, shape=None, dtype=None, align=16):
        if data is not None:
            data = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
            shape = tuple(data.shape) if shape is None else shape
            dtype = data.dtype if dtype is None else dtype
        self.name, self.role, self.data, self.align = name, role, data, align
        self.shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.dtype = torch.float32 if dtype is None else dtype

    @property
    def nbytes(self):
        return torch.empty((), dtype=self.dtype).element_size() * int(np.prod(self.shape, dtype=np.int64))


def build(device, specs):
    """An arena of exactly the capacity the specs need, with every tensor placed."""
    specs = [s for s in specs if s is not None]
    arena = Arena(device, capacity=sum(2 * max(GUARD_MIN, s.nbytes) + s.nbytes + 4 * s.align for s in specs))
    for s in specs:
        arena.tensor(s.name, s.shape, s.dtype, align=s.align, role=s.role, data=s.data)
    return arena


def run_passes(arena, call, outputs, sync=None):
    """Run `call` once per poison byte: poison, load the inputs, call, synchronise, check the guards, keep the named outputs
    (host copies).  Returns [outputs of pass A, outputs of pass B], each a dict name -> torch CPU tensor."""
    kept = []
    for byte in (POISON_A, POISON_B):
        arena.poison(byte)
        arena.load()
        call()
        if sync is not None:
            sync()
        arena.check()
        kept.append({name: arena[name].detach().cpu().clone() for name in outputs})
    return kept


def bit_identical(a, b):
    """True when two tensors hold the same bytes (NaN == NaN, -0 != +0)."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def assert_passes_identical(kept, what=''):
    for name in kept[0]:
        assert bit_identical(kept[0][name], kept[1][name]), \
            "%s: output '%s' differs between the 0xFF and the 0x7F pass (a byte outside a buffer reached the result)" % (what, name)
