"""The poisoned-arena helper (tests/_arena.py) on a CPU arena with planted violations: each invariant
must fail on its own violation and name the region, and a clean pass must pass. Without this the GPU
arena tests could pass without checking anything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _arena import ALIGN, GUARD, Arena, ArenaError, Plain, same_bits  # noqa: E402


def _carve(offsets=(0, 0, 0, 0, 0)):
    """An arena with one region of every role, and a kernel's work done by hand: outputs written,
    the zeroed workspace left zero."""
    a = Arena("cpu", 1 << 20)
    x = a.take((33, 3), torch.float32, role="input", fill=torch.arange(99.0).reshape(33, 3), name="x",
               offset_bytes=offsets[0])
    w = a.take((7,), torch.bfloat16, role="input", fill=torch.ones(7, dtype=torch.bfloat16), name="w",
               offset_bytes=offsets[1])
    y = a.take((33, 2), torch.float32, role="output", name="y", offset_bytes=offsets[2])
    s = a.take((129,), torch.uint8, role="scratch", name="work", offset_bytes=offsets[3])
    z = a.take((64,), torch.int32, role="zeroed", name="loss_ws", offset_bytes=offsets[4])
    y.copy_(torch.full((33, 2), float("nan")))  # a NaN the "kernel" computed is a written element
    return a, x, w, y, s, z


def test_layout_alignment_exact_payloads_and_gaps():
    a, x, w, y, s, z = _carve(offsets=(8, 2, 4, 0, 0))
    assert x.data_ptr() % ALIGN == 8 and w.data_ptr() % ALIGN == 2 and y.data_ptr() % ALIGN == 4
    assert s.data_ptr() % ALIGN == 0 and z.data_ptr() % ALIGN == 0
    regs = a.regions
    assert [r.nbytes for r in regs] == [33 * 3 * 4, 14, 33 * 2 * 4, 129, 256]
    assert regs[0].start - a.base >= GUARD
    for p, q in zip(regs, regs[1:]):
        assert q.start - (p.start + p.nbytes) >= GUARD
    assert a.end - (regs[-1].start + regs[-1].nbytes) >= GUARD
    # what was handed out: inputs hold their data, the others the fill pattern / zeros
    assert torch.equal(x, torch.arange(99.0).reshape(33, 3)) and bool((s == 0xFF).all()) and bool((z == 0).all())
    fresh = Arena("cpu", 1 << 20).take((5,), torch.float32, role="output")
    assert bool(torch.isnan(fresh).all()) and bool((fresh.view(torch.int32) == -1).all())
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert bool(torch.isnan(Arena("cpu", 1 << 20).take((3,), dt, role="output")).all())


def test_clean_pass_passes():
    a, *_ = _carve()
    a.verify()
    a, *_ = _carve(offsets=(8, 2, 4, 1, 4))
    a.verify()


def test_full_arena_raises():
    a = Arena("cpu", 4 * GUARD)
    a.take((GUARD,), torch.uint8, role="scratch")
    with pytest.raises(MemoryError):
        a.take((GUARD,), torch.uint8, role="scratch")


@pytest.mark.parametrize("where", ["after_y_1", "after_y_last", "before_x", "after_last"])
def test_i1_one_byte_in_a_guard(where):
    a, x, w, y, s, z = _carve()
    r = {r.name: r for r in a.regions}
    at, name, off = {
        "after_y_1": (r["y"].start + r["y"].nbytes, "y", 0),
        "after_y_last": (r["work"].start - 1, "y", r["work"].start - 1 - (r["y"].start + r["y"].nbytes)),
        "before_x": (r["x"].start - 1, "x", -1),
        "after_last": (r["loss_ws"].start + r["loss_ws"].nbytes + GUARD - 1, "loss_ws", GUARD - 1),
    }[where]
    a.buf[at] = 0x7F
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.invariant.startswith("I1") and e.value.region == name and e.value.offset == off
    assert f"'{name}'" in str(e.value)


def test_i1_a_store_past_the_end_through_the_view_s_storage():
    """What a kernel's stray store does: one element past the payload, written through the pointer."""
    a, x, w, y, s, z = _carve()
    past = torch.as_strided(y, (1,), (1,), storage_offset=y.storage_offset() + y.numel())
    past.fill_(1.0)
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.invariant.startswith("I1") and e.value.region == "y" and e.value.offset == 0


def test_i2_one_input_element_changed():
    a, x, w, y, s, z = _carve()
    w[5] = 2.0
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.invariant.startswith("I2") and e.value.region == "w" and e.value.offset in (10, 11)
    a, x, w, y, s, z = _carve()
    x[32, 2] = float("nan")  # bytes are compared: NaN is a change too
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.region == "x" and 98 * 4 <= e.value.offset < 99 * 4


def test_i3_one_output_element_unwritten():
    a, x, w, y, s, z = _carve()
    y.view(torch.int32)[32, 1] = -1
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.invariant.startswith("I3") and e.value.region == "y" and e.value.offset == 65 * 4
    # a NaN with any other payload counts as written
    a, x, w, y, s, z = _carve()
    y.view(torch.int32)[32, 1] = 0x7FC00000
    a.verify()


def test_i4_one_word_left_in_a_zeroed_region():
    a, x, w, y, s, z = _carve()
    z[63] = 1
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.invariant.startswith("I4") and e.value.region == "loss_ws" and e.value.offset == 63 * 4


def test_i4_zero_check_range():
    """The encoder workspace: only the ticket word behind the partial sums must stay zero."""
    a = Arena("cpu", 1 << 20)
    ws = a.take((40,), torch.int32, role="zeroed", name="enc_ws", zero_check=(32 * 4, 33 * 4))
    ws[:32] = 7
    ws[33:] = 7
    a.verify()
    ws[32] = 1
    with pytest.raises(ArenaError) as e:
        a.verify()
    assert e.value.region == "enc_ws" and e.value.offset == 128


def test_i7_refused_call_leaves_outputs_alone():
    a = Arena("cpu", 1 << 20)
    a.take((4,), torch.float32, role="input", fill=1.0, name="x")
    y = a.take((9,), torch.float32, role="output", name="y")
    a.assert_nothing_launched()
    y[3] = 0.0
    with pytest.raises(ArenaError) as e:
        a.assert_nothing_launched()
    assert e.value.invariant.startswith("I7") and e.value.region == "y" and e.value.offset == 12


def test_scratch_is_never_checked():
    a, x, w, y, s, z = _carve()
    s.fill_(3)
    a.verify()
    b = Arena("cpu", 1 << 20)
    t = b.take((3,), torch.float32, role="scratch", fill=torch.tensor([1.0, 2.0, 3.0]))
    t += 1  # a buffer updated in place
    b.verify()


def test_plain_allocator_mirrors_the_takes():
    p = Plain("cpu")
    x = p.take((5, 2), torch.float32, role="input", fill=torch.ones(5, 2), offset_bytes=8)
    y = p.take((5,), torch.float32, role="output", offset_bytes=4)
    z = p.take((16,), torch.uint8, role="zeroed")
    assert x.data_ptr() % 16 == 8 and y.data_ptr() % 8 == 4
    assert bool((x == 1).all()) and bool((y == 0).all()) and bool((z == 0).all())
    a = p.arena()
    for shape, dt, role, off in (((5, 2), torch.float32, "scratch", 8), ((5,), torch.float32, "scratch", 4),
                                 ((16,), torch.uint8, "scratch", 0)):
        a.take(shape, dt, role=role, offset_bytes=off)  # the arena it sizes holds the same takes
    p.verify()


def test_same_bits_tells_nan_payloads_apart():
    a = torch.tensor([1.0, float("nan")])
    b = a.clone()
    assert same_bits(a, b)
    b.view(torch.int32)[1] = -1
    assert not same_bits(a, b) and not same_bits(a, a.double()) and not same_bits(a, a[:1])
