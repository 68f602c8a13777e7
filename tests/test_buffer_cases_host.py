"""What the batches of the buffer-contract modules -- tests/test_gpu_buffers_packed.py, test_gpu_buffers_wide.py,
test_gpu_buffers_interleaved.py and the later Monte-Carlo routes of test_gpu_buffers_channels.py -- are chosen for, checked
on the CPU with the oracles and models alone: a guard, a poison or an absent output proves little on a batch in which
every frame decodes, no list is empty, a call in place has nothing to correct or an extracted word is a codeword anyway.
Every batch the GPU modules run is built here by the same (cached) builder; no frame is left out of any comparison there,
and none is here."""
import numpy as np
import pytest

from channelcoding_amd import capi
import test_gpu_buffers_channels as CH
import test_gpu_buffers_interleaved as IL
import test_gpu_buffers_packed as PK
import test_gpu_buffers_wide as WD


def both_outcomes(status, B, what):
    if B >= 2:
        assert (status == 0).any() and (status != 0).any(), (what, status)


def lists_of_both_kinds(per, what):
    assert any(len(e) == 0 for e in per) and any(len(e) > 0 for e in per), (what, [len(e) for e in per])


# ------------------------------------------------ packed ------------------------------------------------
@pytest.mark.parametrize("case", PK.CORRECT_CASES, ids=str)
def test_packed_correct_batches(case):
    name, alg, B, variant = case
    b = PK.correct_batch(*case)
    assert b["rx"].shape == (B, PK.model_of(name).n) and b["words"].shape == b["out"].shape
    if name not in PK.PERFECT:
        both_outcomes(b["status"], B, case)
    if variant == "erasures":
        lists_of_both_kinds(b["per"], case)
    else:
        assert b["per"] is None and b["csr"] is None
    n = PK.model_of(name).n
    pads = PK.unpack(b["words"], 8 * b["words"].shape[1])[:, n:]
    assert pads.any() == (variant == "dirty") and not PK.unpack(b["out"], 8 * b["out"].shape[1])[:, n:].any()
    if variant == "in place":
        assert (PK.unpack(b["out"], n) != b["rx"]).any(), case


def test_packed_cases_cover_what_they_are_named_for():
    assert {B for _, _, B, _ in PK.NATIVE_CASES} == {1, 31, 33, 65}
    assert {v for _, _, _, v in PK.NATIVE_CASES} == {"plain", "dirty", "in place"}
    assert all(B == 1025 for _, _, B, _ in PK.LONG_CASES)
    for name in ("BCH(100,76)", "GF(2^11) t = 4 N = 70"):
        assert ((PK.model_of(name).n + 7) // 8) % 2 == 1  # an odd pitch
    m = PK.model_of("BCH(100,76)")
    assert ((m.n + 7) // 8, (m.l + 7) // 8) == (13, 10)
    two = PK.correct_batch("BCH(255,231)", PK.PGZ, 9, "erasures")
    assert (two["status"] == capi.FRAME_ERASURES).any() and (two["rx"][1, two["per"][1]] != 0).any()


@pytest.mark.parametrize("case", PK.DECODE_CASES, ids=str)
def test_packed_decode_batches(case):
    b = PK.decode_batch(case[0], case[2])
    both_outcomes(b["status"], case[2], case)


@pytest.mark.parametrize("case", PK.EXTRACT_CASES, ids=str)
def test_packed_extract_inputs_hold_a_non_codeword(case):
    name, _, B = case
    m = PK.model_of(name)
    words, bits, _ = PK.extract_batch(name, B)
    assert (np.asarray(m.encode(m.extract(bits))) != bits).any(axis=1).any(), case
    assert PK.unpack(words, 8 * words.shape[1])[:, m.n:].any() or m.n % 8 == 0


@pytest.mark.parametrize("case", PK.ENCODE_CASES, ids=str)
def test_packed_encode_outputs_are_words_with_clean_pad_bits(case):
    name, _, B = case
    m = PK.model_of(name)
    msg, want = PK.encode_batch(name, B)
    assert msg.shape == (B, (m.l + 7) // 8) and want.shape == (B, (m.n + 7) // 8)
    assert not PK.unpack(want, 8 * want.shape[1])[:, m.n:].any()
    assert m.l % 8 == 0 or PK.unpack(msg, 8 * msg.shape[1])[:, m.l:].any()


@pytest.mark.parametrize("case", PK.BITS_CASES, ids=str)
def test_pack_and_unpack_batches(case):
    width, n, B = case
    sym, packed = PK.pack_batch(*case)
    assert (sym > 1).any() and packed.shape == (B, (n + 7) // 8) and not PK.unpack(packed, 8 * packed.shape[1])[:, n:].any()
    assert np.array_equal(PK.unpack(packed, n), sym & 1)
    words, bits = PK.unpack_batch(*case)
    assert n % 8 == 0 or PK.unpack(words, 8 * words.shape[1])[:, n:].any()
    assert bits.shape == (B, n) and bits.max() <= 1


# ------------------------------------------------ 16-bit symbols ------------------------------------------------
@pytest.mark.parametrize("case", WD.CORRECT_CASES + WD.HOST_CASES, ids=str)
def test_wide_correct_batches(case):
    name, alg, B, with_erasures, in_place = case
    b = WD.correct_batch(name, alg, B, with_erasures)
    assert b["rx"].dtype == np.uint16 and b["out"].dtype == np.uint16
    both_outcomes(b["status"], B, case)
    if with_erasures:
        lists_of_both_kinds(b["per"], case)
    if in_place:
        assert (b["out"] != b["rx"]).any(), case


def test_wide_cases_cover_what_they_are_named_for():
    assert WD.model_of("RS(300,292)").n % 64 != 0
    assert WD.model_of("RS(1023,1015) mu=0").mu == 0
    in_place = [c for c in WD.CORRECT_CASES if c[4]]
    assert {c[0] for c in in_place} == set(WD.CODES) and any(c[3] and c[1] == WD.PGZ for c in in_place)
    # the two trials in place: a frame that fails both with a non-zero symbol at an erased position, which trial 0 zeroes
    two = WD.correct_batch("BCH(511,484)", WD.PGZ, 5, True)
    assert any(two["status"][f] != 0 and two["rx"][f, two["per"][f]].any() for f in range(5) if two["per"][f])


@pytest.mark.parametrize("case", WD.MAP_CASES, ids=str)
def test_wide_extract_inputs_hold_a_non_codeword(case):
    m = WD.model_of(case[0])
    words, _ = WD.extract_batch(*case)
    assert (np.asarray(m.encode(m.extract(words))) != words).any(axis=1).any(), case


# ------------------------------------------------ interleaved ------------------------------------------------
@pytest.mark.parametrize("case", IL.CORRECT_CASES + IL.WIDE_CORRECT_CASES + [c + (False, False) for c in IL.DECODE_CASES], ids=str)
def test_interleaved_correct_batches(case):
    name, I, B, _, with_erasures, in_place = case
    assert B % I == 0
    b = IL.correct_batch(name, I, B, with_erasures)
    width = np.uint16 if IL.CODES[name][1] > 8 else np.uint8
    assert b["rx"].dtype == width and b["out"].dtype == width and b["rx"].shape == (B, IL.model_of(name).n)
    both_outcomes(b["status"], B, case)
    if with_erasures:
        lists_of_both_kinds(b["per"], case)
    if in_place:
        assert (b["out"] != b["rx"]).any(), case


@pytest.mark.parametrize("case", IL.EXTRACT_CASES + IL.WIDE_EXTRACT_CASES, ids=str)
def test_interleaved_extract_inputs_hold_a_non_codeword(case):
    name, I, B, _ = case
    m = IL.model_of(name)
    words, _ = IL.extract_batch(name, I, B)
    assert (np.asarray(m.encode(m.extract(words))) != words).any(axis=1).any(), case


def test_interleaved_cases_cover_what_they_are_named_for():
    partial = [(I, B) for name, I, B, *_ in IL.CORRECT_CASES if 32 % I]
    assert (3, 129) in partial and (5, 135) in partial and all(B % 32 for _, B in partial)
    assert IL.model_of("RS(7,3)").l * 3 == 9  # two dwords and a one-byte tail
    assert IL.model_of("RS(204,188)").n == 204
    assert any(w == 1 and (n, I) == (63, 256) for w, n, I, _ in IL.LAYOUTS)


# ------------------------------------------------ Monte-Carlo ------------------------------------------------
@pytest.mark.parametrize("route", list(CH.LATER))
def test_monte_carlo_points(route):
    c = CH.later_predicted(route)
    frames = CH.LATER[route]["frames"]
    CH.later_point(c, frames, route)
    if route == "osd":
        assert 0 < c[capi.MC_WORD_ERRORS] < frames and c[capi.MC_FAILURES] == 0
    else:
        assert 0 < c[capi.MC_FAILURES] < frames and 0 < c[capi.MC_WORD_ERRORS]
    assert (CH.PRELOAD[0] & np.uint64(0xFFFFFFFF)) + np.uint64(frames) > np.uint64(0xFFFFFFFF)
