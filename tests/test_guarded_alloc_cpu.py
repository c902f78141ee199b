"""tests/guarded_alloc.py on CPU tensors and a stub engine: the demonstration that its checks CAN fail -- a byte written
immediately before or after a payload or at the far end of a band is reported with its allocation and offset; a clean run
passes; `empty` is restored also after an exception; a recording keeps the base buffer; views have the requested shape,
dtype, contiguity and the 16-byte-only alignment; and an output element nobody writes shows as differing bits under the
two fills."""
import pytest
import torch

from guarded_alloc import BAND, POISON_FINITE, POISON_NAN, bits_equal, guarded, poisoned


class _Recording:
    def __init__(self):
        self.keep = []


class StubEngine:
    """What the helper relies on of PlaneSweepEngine: one `empty` method, whose tensors a recording keeps alive."""

    def __init__(self):
        self.recording = None
        self.requests = 0

    def empty(self, shape, dtype=torch.float32, device=None, **_):
        self.requests += 1
        t = torch.empty(tuple(shape) if not isinstance(shape, int) else shape, dtype=dtype, device=device)
        if self.recording is not None:
            self.recording.keep.append(t)
        return t


def _is_class_method(eng):
    return "empty" not in vars(eng) and eng.empty.__func__ is StubEngine.empty


def _base_bytes(view):
    """The flat byte buffer a payload view was carved from."""
    storage = view.untyped_storage()
    return torch.empty(0, dtype=torch.uint8).set_(storage, 0, (storage.nbytes(),))


def test_band_is_64k_plus_16_bytes():
    assert BAND == 65536 + 16 and POISON_NAN == 0xFF and POISON_FINITE == 0x7B


@pytest.mark.parametrize("fill", [POISON_NAN, POISON_FINITE])
def test_clean_run_is_left_alone(fill):
    eng = StubEngine()
    with guarded(eng, fill) as g:
        a = eng.empty((3, 5), dtype=torch.float32)
        b = eng.empty(7, dtype=torch.uint8)
        a.fill_(1.0)                       # the whole payload, first to last byte
        b.fill_(2)
    assert len(g.allocations) == 2 and eng.requests == 2
    assert _is_class_method(eng)
    assert not g.damage()


@pytest.mark.parametrize("where,offset", [("before", -1), ("after", 0), ("far_before", -BAND), ("far_after", BAND - 1)])
def test_a_one_byte_write_outside_the_payload_is_reported(where, offset):
    """`offset` is relative to the payload for the bytes in front of it and to its end for the bytes behind it."""
    eng = StubEngine()
    with pytest.raises(AssertionError) as info:
        with guarded(eng, POISON_NAN):
            eng.empty((4, 4), dtype=torch.float32)                 # request 0: stays clean
            x = eng.empty((2, 3, 5), dtype=torch.float32)          # request 1
            base = _base_bytes(x)
            nbytes = x.numel() * 4
            at = BAND + offset if where.endswith("before") else BAND + nbytes + offset
            base[at] = 0x00
    msg = str(info.value)
    want = offset if where.endswith("before") else nbytes + offset
    assert "#1" in msg and "(2, 3, 5)" in msg and "torch.float32" in msg, msg
    assert f"payload offset {want:+d}" in msg, msg
    assert "#0" not in msg
    assert _is_class_method(eng)


def test_a_write_of_the_fill_byte_value_elsewhere_does_not_hide_other_damage():
    eng = StubEngine()
    with pytest.raises(AssertionError) as info:
        with guarded(eng, POISON_FINITE):
            x = eng.empty(16, dtype=torch.uint8)
            base = _base_bytes(x)
            base[BAND - 1] = POISON_FINITE         # same value: not damage
            base[BAND + 16 + 5] = 0xFF
    assert "payload offset +21" in str(info.value)


def test_empty_is_restored_after_an_exception():
    eng = StubEngine()
    with pytest.raises(ZeroDivisionError):
        with guarded(eng, POISON_NAN):
            assert not _is_class_method(eng)
            eng.empty((2,), dtype=torch.float32)
            1 / 0
    assert _is_class_method(eng)
    assert eng.empty((2,)).untyped_storage().nbytes() == 8          # a plain allocation again


def test_a_recording_keeps_the_base_buffer():
    eng = StubEngine()
    eng.recording = _Recording()
    with guarded(eng, POISON_NAN):
        x = eng.empty((5, 3), dtype=torch.float32)
    assert len(eng.recording.keep) == 1
    kept = eng.recording.keep[0]
    assert kept.dtype == torch.uint8 and kept.numel() == 2 * BAND + 60
    assert kept.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
    assert x.data_ptr() == kept.data_ptr() + BAND


@pytest.mark.parametrize("shape,dtype", [((2, 3, 5), torch.float32), ((4, 7), torch.bfloat16), ((3, 1, 9), torch.bool),
                                         ((11,), torch.uint8), (1000, torch.uint8), ((1,), torch.float32)])
def test_views_have_shape_dtype_contiguity_and_16_byte_only_alignment(shape, dtype):
    eng = StubEngine()
    with guarded(eng, POISON_NAN) as g:
        x = eng.empty(shape, dtype=dtype)
    want = (shape,) if isinstance(shape, int) else shape
    assert tuple(x.shape) == want and x.dtype == dtype and x.is_contiguous()
    assert x.data_ptr() % 16 == 0 and x.data_ptr() % 32 == 16
    a = g.allocations[0]
    assert a.nbytes == x.numel() * x.element_size() and a.base.numel() == 2 * BAND + a.nbytes
    # the payload is poisoned too: every byte is the fill byte until somebody writes it
    assert bool((a.base == POISON_NAN).all())
    if dtype == torch.float32 and x.numel():
        assert bool(torch.isnan(x).all())


def test_finite_fill_is_a_large_finite_float():
    eng = StubEngine()
    with guarded(eng, POISON_FINITE):
        x = eng.empty((8,), dtype=torch.float32)
        tag = eng.empty((2,), dtype=torch.int32)
    assert bool(torch.isfinite(x).all()) and 1.2e36 < float(x[0]) < 1.4e36
    assert int(tag[0]) == 0x7B7B7B7B


def test_poisoned_copies_an_input_into_nan_surroundings():
    src = torch.arange(30, dtype=torch.float32).reshape(2, 3, 5).transpose(1, 2)     # not contiguous
    x = poisoned(src)
    assert torch.equal(x, src) and x.is_contiguous() and x.data_ptr() % 32 == 16
    base = _base_bytes(x)
    assert base.numel() == 2 * BAND + 120
    assert bool((base[:BAND] == 0xFF).all()) and bool((base[BAND + 120:] == 0xFF).all())
    y = poisoned(torch.tensor([True, False, True]), POISON_FINITE)
    assert y.dtype == torch.bool and y.tolist() == [True, False, True]
    assert bool((_base_bytes(y)[:BAND] == 0x7B).all())


def test_poisoned_inputs_of_a_guard_are_checked_with_its_allocations():
    eng = StubEngine()
    with pytest.raises(AssertionError) as info:
        with guarded(eng, POISON_NAN) as g:
            x = g.poisoned(torch.zeros(4, 4))
            _base_bytes(x)[BAND + 64] = 1           # an in-place "kernel" running one byte past its input
    assert "input #0" in str(info.value) and "payload offset +64" in str(info.value)


def test_bits_equal_counts_nan_payloads_and_the_sign_of_zero():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert bits_equal(a, a.clone())
    assert not torch.equal(a, a.clone())                      # (what a value comparison does with a NaN)
    assert not bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    quiet = torch.tensor([0x7FC00000, 0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert not bits_equal(quiet[:1], quiet[1:])
    assert not bits_equal(torch.zeros(2), torch.zeros(2, dtype=torch.int32))
    assert not bits_equal(torch.zeros(2), torch.zeros(3))
    assert bits_equal(torch.tensor([True, False]), torch.tensor([True, False]))
    assert bits_equal(torch.ones(2, 3).t(), torch.ones(3, 2))             # strided views compare by value order


def _stub_kernel(eng, x, skip=None):
    """out = 2 * x, written element by element -- except `skip`, which no work item covers."""
    out = eng.empty(x.shape, dtype=x.dtype)
    flat_out, flat_in = out.view(-1), x.reshape(-1)
    for i in range(flat_in.numel()):
        if i != skip:
            flat_out[i] = 2 * flat_in[i]
    return out


def test_an_output_element_nobody_writes_differs_between_the_two_fills():
    eng = StubEngine()
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    got = {}
    for skip in (None, 7):
        for fill in (POISON_NAN, POISON_FINITE):
            with guarded(eng, fill):                  # (bands intact: the fault is inside the payload)
                got[skip, fill] = _stub_kernel(eng, x, skip)
    assert bits_equal(got[None, POISON_NAN], got[None, POISON_FINITE])
    assert bits_equal(got[None, POISON_NAN], 2 * x)
    assert not bits_equal(got[7, POISON_NAN], got[7, POISON_FINITE])
    assert bool(torch.isnan(got[7, POISON_NAN].view(-1)[7]))
    # every element the kernel DID write agrees
    keep = torch.ones(12, dtype=torch.bool)
    keep[7] = False
    assert bits_equal(got[7, POISON_NAN].view(-1)[keep], got[7, POISON_FINITE].view(-1)[keep])
