"""tests/guarded_buffers.py on host memory, against small fake calls that move bytes through ctypes: one call that keeps
the buffer contract, and calls with one defect each, which check_call must report -- the harness is what the GPU buffer
tests stand on, so what it claims to see is shown here where nothing can fault: every access of every fake call lies
inside the allocations the harness made (the guard runs and the poison round an input are part of them).

The fake call, over n bytes `src`:
    dst       n bytes, src ^ 1
    pos, off  a list as the channel calls return it: the indices of the odd bytes of src, ascending, in a uint16 buffer
              of capacity n whose unlisted tail is not written, and off = (0, count) as uint32 -- absent only together
    counters  8 uint64 the call adds to: [0] += n, [1] += count; slots 2 .. 7 are not touched"""
import ctypes as C

import numpy as np
import pytest

from guarded_buffers import GUARD, PAD, SENTINEL, check_call

N = 11
SRC = np.array([3, 0, 7, 8, 250, 1, 1, 0, 90, 93, 2], np.uint8)  # (no byte of src ^ 1 is SENTINEL)
ODD = np.flatnonzero(SRC & 1)
PRELOAD = ((np.arange(8, dtype=np.uint64) + np.uint64(1)) << np.uint64(40)) | (np.uint64(0xFFFFFF00) + np.arange(8, dtype=np.uint64))


def at(pointer, dtype, count):
    """`count` elements of host memory at a c_void_p, as a numpy array that writes through"""
    size = np.dtype(dtype).itemsize * count
    return np.frombuffer((C.c_uint8 * size).from_address(pointer.value), dtype=dtype, count=count)


def fake(defect=None, seen=None):
    def call(p):
        src, dst, cnt = at(p["src"], np.uint8, N), at(p["dst"], np.uint8, N), at(p["counters"], np.uint64, 8)
        if seen is not None:
            seen.append((p["pos"] is None, p["off"] is None))
        dst[:] = src ^ 1
        if defect == "past the end":
            at(p["dst"], np.uint8, N + 1)[N] = 0  # the first byte of the guard run behind dst
        if defect == "unwritten":
            dst[N - 1] = SENTINEL  # what the byte held before the call
        if defect == "beyond the input":
            dst[N - 1] = at(p["src"], np.uint8, N + 1)[N] ^ 1  # the first byte of the poison behind src
        odd = np.flatnonzero(src & 1)
        if p["pos"] is not None:
            at(p["pos"], np.uint16, N)[:odd.size] = odd
            at(p["off"], np.uint32, 2)[:] = (0, odd.size)
        if defect == "stored":
            cnt[0] = N
        else:
            cnt[0] += np.uint64(N)
        cnt[1] += np.uint64(odd.size)
        if defect == "untouched slot":
            cnt[5] += np.uint64(0x100)  # the low word of the preload carries into the high one
        if defect == "input written":
            src[0] ^= 0xFF
        return 0
    return call


def listed(view, label):
    got = view.numpy().view(np.uint16)
    assert np.array_equal(got[:ODD.size], ODD), label
    assert (got[ODD.size:].view(np.uint8) == SENTINEL).all(), (label, "the unlisted tail was written")


def all_but_the_last(view, label):
    assert np.array_equal(view.numpy()[:N - 1], (SRC ^ 1)[:N - 1]), label


def run(call, dst=SRC ^ 1):
    want = PRELOAD.copy()
    want[0] += np.uint64(N)
    want[1] += np.uint64(ODD.size)
    outputs = {"dst": (np.uint8, N), "pos": (np.uint16, N), "off": (np.uint32, 2), "counters": (np.uint64, 8, PRELOAD)}
    expected = {"dst": dst, "pos": listed, "off": np.array([0, ODD.size], np.uint32), "counters": want}
    return check_call(call, {"src": SRC}, outputs, expected, optional=(("pos", "off"),), device="cpu", what="fake")


def test_the_correct_call_passes():
    seen = []
    out = run(fake(seen=seen))
    # all outputs under poison A, the pair absent, all outputs under poison B: the pair is never split
    assert seen == [(False, False), (True, True), (False, False)]
    assert out["counters"].data_ptr() % 16 == 8 and out["off"].data_ptr() % 8 == 4 and out["pos"].data_ptr() % 4 == 2
    assert out["dst"].data_ptr() % 2 == 1
    assert 0 < ODD.size < N and not ((SRC ^ 1) == SENTINEL).any()
    assert (PRELOAD & np.uint64(0xFFFFFFFF)).min() + np.uint64(0x100) > np.uint64(0xFFFFFFFF)  # a count of 256 carries
    assert GUARD >= 1 and PAD >= 1  # the bytes the defects below touch belong to the harness


@pytest.mark.parametrize("defect,report", [
    ("past the end", "a byte outside the buffer was written"),
    ("unwritten", "differs from the expected array"),
    ("input written", "an input was written"),
    ("stored", "differs from the expected array"),
    ("untouched slot", "differs from the expected array"),
])
def test_a_defect_is_reported(defect, report):
    with pytest.raises(AssertionError) as e:
        run(fake(defect))
    assert report in str(e.value), str(e.value)
    name = {"past the end": "dst", "unwritten": "dst", "input written": "src"}.get(defect, "counters")
    assert repr(name) in str(e.value), str(e.value)


def test_a_byte_from_beyond_an_input_is_reported():
    """against the expected array the byte shows under either poison; where the checker looks at a sample that leaves the
    byte out, the comparison of the two poisons still shows it"""
    with pytest.raises(AssertionError) as e:
        run(fake("beyond the input"))
    assert "differs from the expected array" in str(e.value) and "'dst'" in str(e.value)
    with pytest.raises(AssertionError) as e:
        run(fake("beyond the input"), dst=all_but_the_last)
    assert "the result depends on memory outside the inputs" in str(e.value) and "'dst'" in str(e.value)
    run(fake(), dst=all_but_the_last)  # (the sampled checker itself accepts the correct call)


def test_the_unlisted_tail_is_watched():
    def call(p):
        fake()(p)
        if p["pos"] is not None:
            at(p["pos"], np.uint16, N)[N - 1] = 0
        return 0
    with pytest.raises(AssertionError) as e:
        run(call)
    assert "the unlisted tail was written" in str(e.value)
