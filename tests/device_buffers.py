"""Guarded device buffers for the tests of the C ABI's device-pointer forms (test infrastructure, like
pointwise_cases.py; test_device_buffers_host.py checks the pure parts on the CPU).

One device allocation holds a front guard, the payload and a back guard, all pre-filled with one 64-bit sentinel: a
quiet NaN with a non-zero payload.  No kernel of the library produces it -- a NaN the device arithmetic makes is the
canonical 0x7FF8000000000000 -- so a payload word that still holds it was never written, and a guard word that no longer
holds it was written by somebody who had no business there.  int32 arrays are marked by the same bytes: the sentinel's
low half in even positions, its high half in odd ones, neither of them an info code.

The pointer handed to the library is the payload's, an interior pointer of the allocation.
"""
import ctypes as C

import numpy as np

SENTINEL = np.uint64(0x7FF8DEADBEEFC0DE)
CANONICAL_NAN = np.uint64(0x7FF8000000000000)
GUARD_MIN_BYTES = 64 * 1024
_ALIGN = 256


# ---- the pure parts: numpy in, numpy or indices out ----------------------------------------------------------------
def pattern(nwords):
    """nwords 8-byte words of the sentinel."""
    return np.full(int(nwords), SENTINEL, dtype=np.uint64)


def guard_bytes(matrix_bytes):
    """Size of each guard: one whole matrix of the call, never less than 64 KiB, a multiple of the alignment."""
    g = max(int(matrix_bytes), GUARD_MIN_BYTES)
    return (g + _ALIGN - 1) // _ALIGN * _ALIGN


def layout(payload_bytes, matrix_bytes):
    """(guard bytes, payload bytes rounded up to whole words, total bytes) of an allocation."""
    g = guard_bytes(matrix_bytes)
    p = (int(payload_bytes) + 7) // 8 * 8
    return g, p, 2 * g + p


def damaged_guard_word(raw, guard, payload_bytes):
    """raw: the whole allocation as uint64 words.  None if both guards (and the padding behind a payload that is not a
    whole number of words) hold nothing but the sentinel, else ("front" | "back", index of the first damaged word
    counted from the payload's edge outwards, so that index 0 is the word next to the payload)."""
    gw = guard // 8
    front = raw[:gw]
    bad = np.flatnonzero(front != SENTINEL)
    if bad.size:
        return "front", int(gw - 1 - bad[-1])
    whole, rest = divmod(int(payload_bytes), 8)
    back = raw[gw + whole + (1 if rest else 0):]
    if rest:  # the bytes of the payload's last word that lie behind its end
        tail = raw[gw + whole:gw + whole + 1].view(np.uint8)[rest:]
        if not np.array_equal(tail, pattern(1).view(np.uint8)[rest:]):
            return "back", 0
    bad = np.flatnonzero(back != SENTINEL)
    if bad.size:
        return "back", int(bad[0]) + (1 if rest else 0)
    return None


def first_unwritten(payload, dtype):
    """payload: the payload's bytes (uint8).  Index of the first element (of `dtype`) that still holds sentinel bytes,
    or None.  8- and 16-byte types: an element is unwritten if one of its 8-byte words is the sentinel; 4-byte types:
    if it holds the half of the sentinel that belongs at its position."""
    size = np.dtype(dtype).itemsize
    if size % 8 == 0:
        hit = np.flatnonzero(payload.view(np.uint64) == SENTINEL)
        return None if not hit.size else int(hit[0]) // (size // 8)
    if size != 4:
        raise TypeError("guarded buffers hold 4-, 8- or 16-byte elements")
    words = payload.view(np.uint32)
    halves = np.resize(pattern(1).view(np.uint32), words.shape)
    hit = np.flatnonzero(words == halves)
    return None if not hit.size else int(hit[0])


def decode_index(element, shape):
    """The (item, row, column) of a flat element index of a [nbatch, n, m] array (fewer axes: what there are)."""
    return tuple(int(k) for k in np.unravel_index(int(element), shape))


def describe_index(element, shape):
    names = {3: "(item, row, column)", 2: "(item, entry)", 1: "(item,)"}.get(len(shape), "index")
    return f"{names} = {decode_index(element, shape)}"


# ---- the buffer ----------------------------------------------------------------------------------------------------
_HIP = None
_H2D, _D2H = 1, 2


def _hip():
    global _HIP
    if _HIP is None:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        _HIP = hip
    return _HIP


def create_non_blocking_stream():
    st = C.c_void_p()
    assert _hip().hipStreamCreateWithFlags(C.byref(st), 1) == 0  # hipStreamNonBlocking
    return st


def destroy_stream(st):
    _hip().hipStreamDestroy(st)


class GuardedBuffer:
    """[front guard | payload of `shape` x `dtype` | back guard] in one hipMalloc, sentinel everywhere.  matrix_bytes:
    one whole matrix of the call the buffer is for (default: one item of the payload); stream: the hipStream_t every
    copy of this buffer is queued on (None: the null stream).  Reads synchronise that stream first."""

    def __init__(self, shape, dtype=np.complex128, matrix_bytes=None, stream=None):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        if matrix_bytes is None:
            matrix_bytes = self.nbytes // max(self.shape[0], 1)
        self.guard, self.padded, self.total = layout(self.nbytes, matrix_bytes)
        self.stream = stream
        self.hip = _hip()
        self.base = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.base), self.total) == 0
        self._staged = [pattern(self.total // 8)]  # (host sources of queued copies stay alive with the buffer)
        self._copy(self.base.value, self._staged[0].ctypes.data, self.total, _H2D)

    @property
    def ptr(self) -> int:
        """The payload's address: what the library is given."""
        return self.base.value + self.guard

    def _copy(self, dst, src, nbytes, kind):
        assert self.hip.hipMemcpyAsync(dst, src, nbytes, kind, self.stream) == 0

    def synchronize(self):
        assert self.hip.hipStreamSynchronize(self.stream) == 0

    def upload(self, a):
        """Queue a copy of a numpy array into the payload; returns self."""
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        self._staged.append(a.copy())
        self._copy(self.ptr, self._staged[-1].ctypes.data, self.nbytes, _H2D)
        return self

    def _raw(self):
        raw = np.empty(self.total // 8, dtype=np.uint64)
        self.synchronize()
        self._copy(raw.ctypes.data, self.base.value, self.total, _D2H)
        self.synchronize()
        return raw

    def _payload(self, raw):
        return raw.view(np.uint8)[self.guard:self.guard + self.nbytes]

    def read(self):
        """The payload as a numpy array of the buffer's shape and type."""
        return self._payload(self._raw()).copy().view(self.dtype).reshape(self.shape)

    def poke(self, byte_offset, words):
        """Write 8-byte words at a byte offset from the payload's start (negative: the front guard) -- for the test
        that shows the checks bite."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._staged.append(w)
        self._copy(self.ptr + int(byte_offset), w.ctypes.data, w.nbytes, _H2D)

    def assert_guards_intact(self):
        bad = damaged_guard_word(self._raw(), self.guard, self.nbytes)
        assert bad is None, f"{bad[0]} guard overwritten, {bad[1]} words from the payload"

    def assert_fully_written(self):
        k = first_unwritten(self._payload(self._raw()), self.dtype)
        assert k is None, f"never written: {describe_index(k, self.shape)}"

    def assert_untouched(self):
        """Nothing but the sentinel anywhere: a call that was refused wrote nothing."""
        assert np.array_equal(self._raw(), pattern(self.total // 8)), "a buffer that should hold only the sentinel does not"

    def assert_unchanged(self, original):
        """The payload is byte for byte what was uploaded."""
        a = np.ascontiguousarray(original, dtype=self.dtype)
        got = self._payload(self._raw())
        if got.tobytes() != a.tobytes():
            k = int(np.flatnonzero(got != a.reshape(-1).view(np.uint8))[0]) // self.dtype.itemsize
            raise AssertionError(f"an input the call must not modify changed: {describe_index(k, self.shape)}")

    def free(self):
        if self.base:
            self.synchronize()
            self.hip.hipFree(self.base)
            self.base = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
