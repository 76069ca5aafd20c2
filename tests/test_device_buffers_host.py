"""The pure parts of tests/device_buffers.py on arrays with planted defects (no GPU): the sentinel pattern, the guard
check, the search for entries that were never written and the decoding of what it finds."""
import numpy as np
import pytest

import device_buffers as db


def _allocation(shape, dtype, matrix_bytes):
    """A host image of a guarded allocation whose payload a 'kernel' has written completely."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    guard, padded, total = db.layout(nbytes, matrix_bytes)
    raw = db.pattern(total // 8)
    rng = np.random.default_rng(11)
    if np.dtype(dtype) == np.int32:
        data = rng.integers(-6, 40, size=shape).astype(np.int32)
    elif np.dtype(dtype) == np.float64:
        data = rng.standard_normal(shape)
    else:
        data = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    raw.view(np.uint8)[guard:guard + nbytes] = data.reshape(-1).view(np.uint8)
    return raw, guard, nbytes


def _payload(raw, guard, nbytes):
    return raw.view(np.uint8)[guard:guard + nbytes]


def test_the_sentinel_is_a_quiet_nan_with_a_payload():
    s = db.pattern(3)
    assert s.dtype == np.uint64 and (s == db.SENTINEL).all()
    assert np.isnan(s.view(np.float64)).all()
    assert int(db.SENTINEL) >> 51 == 0xFFF                      # exponent all ones, quiet bit set
    assert int(db.SENTINEL) & ((1 << 51) - 1) != 0              # and a payload: not the canonical NaN
    assert db.SENTINEL != db.CANONICAL_NAN
    assert np.array([np.nan]).view(np.uint64)[0] == db.CANONICAL_NAN


def test_guards_hold_a_whole_matrix_and_never_less_than_64_kib():
    assert db.guard_bytes(16 * 16 * 16) == 64 * 1024
    big = 1100 * 1100 * 16
    assert db.guard_bytes(big) >= big and db.guard_bytes(big) % 8 == 0
    g, p, total = db.layout(5 * 4, 0)   # five int32: the payload is padded to whole words
    assert p == 24 and total == 2 * g + 24 and g % 8 == 0


@pytest.mark.parametrize("shape,dtype", [((3, 5, 5), np.complex128), ((7,), np.int32), ((4,), np.float64)])
def test_a_clean_buffer_passes(shape, dtype):
    raw, guard, nbytes = _allocation(shape, dtype, 5 * 5 * 16)
    assert db.damaged_guard_word(raw, guard, nbytes) is None
    assert db.first_unwritten(_payload(raw, guard, nbytes), dtype) is None


def test_one_unwritten_entry_is_found_and_named():
    shape = (3, 5, 5)
    raw, guard, nbytes = _allocation(shape, np.complex128, 5 * 5 * 16)
    words = _payload(raw, guard, nbytes).view(np.uint64)
    flat = np.ravel_multi_index((1, 2, 3), shape)
    words[2 * flat] = db.SENTINEL          # the real part alone
    k = db.first_unwritten(_payload(raw, guard, nbytes), np.complex128)
    assert k == flat and db.decode_index(k, shape) == (1, 2, 3)
    assert "(item, row, column) = (1, 2, 3)" in db.describe_index(k, shape)
    words[2 * flat] = 0
    words[2 * flat + 1] = db.SENTINEL      # the imaginary part alone
    assert db.first_unwritten(_payload(raw, guard, nbytes), np.complex128) == flat
    assert db.damaged_guard_word(raw, guard, nbytes) is None


def test_an_unwritten_int32_is_found_at_either_parity():
    for k in (2, 5):
        raw, guard, nbytes = _allocation((7,), np.int32, 0)
        _payload(raw, guard, nbytes).view(np.uint32)[k] = db.pattern(1).view(np.uint32)[k % 2]
        assert db.first_unwritten(_payload(raw, guard, nbytes), np.int32) == k
        assert db.decode_index(k, (7,)) == (k,)


@pytest.mark.parametrize("shape,dtype", [((3, 5, 5), np.complex128), ((7,), np.int32)])
def test_one_overwritten_guard_word_on_each_side(shape, dtype):
    raw, guard, nbytes = _allocation(shape, dtype, 5 * 5 * 16)
    gw = guard // 8
    raw[gw - 1] = 0                        # the word in front of the payload
    assert db.damaged_guard_word(raw, guard, nbytes) == ("front", 0)
    raw[gw - 1] = db.SENTINEL
    raw[0] = np.float64(1.5).view(np.uint64)   # the far end of the front guard
    assert db.damaged_guard_word(raw, guard, nbytes) == ("front", gw - 1)
    raw[0] = db.SENTINEL
    first_back = gw + (nbytes + 7) // 8
    raw[first_back] = 0                    # the first whole word behind the payload
    side, k = db.damaged_guard_word(raw, guard, nbytes)
    assert side == "back" and k == (1 if nbytes % 8 else 0)
    raw[first_back] = db.SENTINEL
    raw[-1] = 0
    assert db.damaged_guard_word(raw, guard, nbytes)[0] == "back"
    raw[-1] = db.SENTINEL
    assert db.damaged_guard_word(raw, guard, nbytes) is None


def test_a_store_one_int_past_an_odd_int32_payload_is_seen():
    raw, guard, nbytes = _allocation((7,), np.int32, 0)
    assert nbytes % 8 == 4
    raw.view(np.uint32)[guard // 4 + 7] = 0   # the half word that pads the payload
    assert db.damaged_guard_word(raw, guard, nbytes) == ("back", 0)


def test_a_produced_canonical_nan_counts_as_written():
    shape = (2, 4, 4)
    raw, guard, nbytes = _allocation(shape, np.complex128, 4 * 4 * 16)
    _payload(raw, guard, nbytes).view(np.complex128)[5:9] = complex(np.nan, np.nan)
    assert (_payload(raw, guard, nbytes).view(np.uint64)[10:18] == db.CANONICAL_NAN).all()
    assert db.first_unwritten(_payload(raw, guard, nbytes), np.complex128) is None
