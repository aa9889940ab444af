"""The guard-band harness (tests/guarded.py) is not vacuous: with plain torch functions standing in for kernels, on CPU
tensors, it reports a write one element before and one element after a tensor (name, side, offsets), a read one element past
an input shows as a difference between the 0xFF and the 0x7F pass, tensors sit at exactly the requested alignment, and a
scratch tensor has exactly the bytes asked for."""
import numpy as np
import pytest
import torch

import guarded
from guarded import Arena, GuardError, run_passes, bit_identical, assert_passes_identical


def _raw(arena, view, lo, hi, dtype):
    """Elements [lo, hi) relative to the start of `view`, straight out of the arena's bytes: what a kernel with a pointer can
    reach, and a torch view cannot."""
    item = view.element_size()
    off = view.data_ptr() - arena.base
    return arena.buf[off + lo * item:off + hi * item].view(dtype)


def _arena():
    a = Arena('cpu', capacity=8 << 20)
    x = a.tensor('x', (5, 7), torch.float32, role='in', data=np.arange(35, dtype=np.float32).reshape(5, 7))
    y = a.tensor('y', (5, 7), torch.float32, role='out')
    return a, x, y


def test_clean_function_passes_and_outputs_are_kept():
    a, x, y = _arena()
    kept = run_passes(a, lambda: y.copy_(x * 2), ['y'])
    assert_passes_identical(kept)
    assert torch.equal(kept[0]['y'], torch.arange(35, dtype=torch.float32).reshape(5, 7) * 2)


def test_poison_fills_outputs_and_scratch_but_not_inputs():
    a, x, y = _arena()
    s = a.scratch('s', 37)
    a.poison(guarded.POISON_A)
    a.load()
    assert torch.isnan(y).all() and bool((s == 0xFF).all())
    assert torch.equal(x, torch.arange(35, dtype=torch.float32).reshape(5, 7))
    a.poison(guarded.POISON_B)
    assert bool((y > 3e38).all()) and torch.isfinite(y).all() and bool((s == 0x7F).all())
    a.check()


@pytest.mark.parametrize('byte', [guarded.POISON_A, guarded.POISON_B])
def test_write_one_element_before_is_reported(byte):
    a, x, y = _arena()
    a.poison(byte)
    a.load()
    y.copy_(x)
    _raw(a, y, -1, 0, torch.float32).fill_(1.0)              # the "kernel" stores y[-1]
    with pytest.raises(GuardError) as e:
        a.check()
    (v,) = e.value.violations
    # 1.0f is 00 00 80 3F: all four bytes differ from either poison
    assert (v.name, v.side, v.first, v.last, v.count) == ('y', 'before', -4, -1, 4)
    assert "'y'" in str(e.value) and 'before' in str(e.value)


@pytest.mark.parametrize('byte', [guarded.POISON_A, guarded.POISON_B])
def test_write_one_element_after_is_reported(byte):
    a, x, y = _arena()
    a.poison(byte)
    a.load()
    y.copy_(x)
    _raw(a, x, 35, 36, torch.float32).fill_(1.0)             # ... stores x[numel]: past the end of an *input*
    _raw(a, y, 36, 37, torch.float32).fill_(1.0)             # ... and y[numel + 1]
    with pytest.raises(GuardError) as e:
        a.check()
    got = sorted((v.name, v.side, v.first, v.last, v.count) for v in e.value.violations)
    assert got == [('x', 'after', 0, 3, 4), ('y', 'after', 4, 7, 4)]


def test_single_byte_far_into_a_guard_is_reported():
    a, x, y = _arena()
    a.poison(guarded.POISON_A)
    off = y.data_ptr() - a.base + y.numel() * 4 + guarded.GUARD_MIN - 1        # the guard's last byte
    a.buf[off] = 0
    with pytest.raises(GuardError) as e:
        a.check()
    (v,) = e.value.violations
    assert (v.name, v.side, v.first, v.last, v.count) == ('y', 'after', guarded.GUARD_MIN - 1, guarded.GUARD_MIN - 1, 1)


def test_read_one_element_past_the_input_differs_between_passes():
    a, x, y = _arena()
    s = a.tensor('s', (1,), torch.float32, role='out')

    def over_reading_max():                                  # max over x[0 .. numel]: one element too many
        s[0] = _raw(a, x, 0, 36, torch.float32).max()

    kept = run_passes(a, over_reading_max, ['s'])            # no guard byte changes: only the two passes can tell
    # pass A: the neighbour is NaN; pass B: 3.4e38 wins the max.  (A kernel's v_max would drop the NaN: pass B is what shows it.)
    assert not bit_identical(kept[0]['s'], kept[1]['s'])
    assert float(kept[1]['s'][0]) > 3e38
    with pytest.raises(AssertionError, match="'s' differs"):
        assert_passes_identical(kept, 'max')

    kept = run_passes(a, lambda: s.fill_(float(x.max())), ['s'])     # the correct function: identical, and 34
    assert_passes_identical(kept)
    assert float(kept[0]['s'][0]) == 34.0


def test_bit_identical_is_bytewise():
    nan = torch.tensor([float('nan'), 1.0])
    assert bit_identical(nan, nan.clone())
    assert not bit_identical(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not bit_identical(torch.zeros(2), torch.zeros(3))


@pytest.mark.parametrize('align', [4, 8, 16, 64, 256])
def test_placement_has_exactly_the_requested_alignment(align):
    a = Arena('cpu', capacity=16 << 20)
    for i, shape in enumerate([(3,), (5, 7), (1,), (129,)]):
        t = a.tensor('t%d' % i, shape, torch.float32, align=align)
        p = t.data_ptr()
        assert p % align == 0 and p % (2 * align) != 0, (align, hex(p))
        if align <= 128:
            assert (p % 256) // align % 2 == 1               # an odd multiple of align past a 256-byte boundary
        assert t.is_contiguous() and tuple(t.shape) == shape
    d = a.tensor('d', (3,), torch.float64, align=8)
    assert d.data_ptr() % 16 == 8
    with pytest.raises(AssertionError):
        a.tensor('bad', (3,), torch.float64, align=4)        # below the element size


def test_guards_are_a_mebibyte_or_the_tensor_and_do_not_overlap():
    a = Arena('cpu', capacity=16 << 20)
    small = a.tensor('small', (3,), torch.float32)
    big = a.tensor('big', (3 << 18,), torch.float32, role='out')     # 3 MiB
    s0, s1 = a.slots
    assert s0.guard == guarded.GUARD_MIN and s1.guard == 3 << 20
    assert s0.start - s0.guard >= 0
    assert s1.start - s1.guard >= s0.start + s0.nbytes + s0.guard
    assert s1.start + s1.nbytes + s1.guard <= a.buf.numel()
    with pytest.raises(MemoryError):
        a.tensor('toobig', (4 << 20,), torch.float32)


def test_exact_scratch_sizes_are_honoured():
    a = Arena('cpu', capacity=8 << 20)
    s = a.scratch('s', 1001)                                 # what a *_bytes function said: not rounded to 4, 16 or 512
    z = a.scratch('z', 0)
    assert s.numel() == 1001 and s.dtype == torch.uint8 and z.numel() == 0
    assert s.data_ptr() % 32 == 16
    a.poison(guarded.POISON_B)
    s.fill_(0)                                               # every byte of it may be used
    a.check()
    _raw(a, s, 1001, 1002, torch.uint8).fill_(0)             # byte 1001 is already guard
    with pytest.raises(GuardError) as e:
        a.check()
    (v,) = e.value.violations
    assert (v.name, v.side, v.first, v.last, v.count) == ('s', 'after', 0, 0, 1)
