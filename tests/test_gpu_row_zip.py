"""The zipped order of the four-row body (minsum_diag_impl.hpp, DIAG_ROWS_FOUR_ZIPPED): the backs of row group g run row
by row between the fronts of group g + 1, and the LDS requests of either stay in flight across the other (counted
waits).  What such an order can get wrong and the shapes of test_gpu_row_groups.py do not single out: the order of a
column's additions across the seam of two groups (the last back of a group stores, the first back of the next reads the
same columns, with a front, a reduction and a wait for something else between them); the fronts of group 0 and the backs
of the last group, which run alone, in batches where some lane groups of the wavefront have no frame at all; m1 = m2 = 0.
Bar: bit for bit in out, L, iters and status against the generic kernel (a process of its own) and the oracle."""
import numpy as np
import pytest

from checkers import BCH, O1, O2, Oracle, awgn_llr
from test_gpu_row_groups import TAGS, _check, _generic

pytestmark = pytest.mark.gpu


def test_row_order_at_a_group_seam(tmp_path):
    """33 frames, MS<2> and MS<3>, stop rules O1 and O2.  Frames 0..16: |y| = 2^u, u uniform in [-6, 6], random signs --
    the addends of a column sum span a dozen binades, so adding them in any order but the reference's ascending row
    order changes bits of L.  Frames 17..32: 3.5 dB."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(47)
    wide = np.where(rng.integers(0, 2, (17, o.n)) == 1, -1.0, 1.0) * np.exp2(rng.uniform(-6.0, 6.0, (17, o.n)))
    y = np.concatenate([wide.astype(np.float32), awgn_llr(rng, np.zeros((16, o.n), np.uint8), o.l / o.n, 3.5)]).astype(np.float32)
    cases = [(it, stop) for it in (2, 3) for stop in (O1, O2)]
    spec = [{"tag": TAGS["MS"][0], "kw": {}, "iterations": it, "stop": stop, "y": "y", "erasures": None} for it, stop in cases]
    gen = _generic(tmp_path, spec, {"y": y})
    for k, (it, stop) in enumerate(cases):
        _check(o, "MS", it, stop, y, None, gen, k, ("seam", it, stop))


@pytest.mark.parametrize("name", sorted(TAGS))
def test_ragged_waves(tmp_path, name):
    """B = 1, 3, 5 and 67 frames at 3.5 dB and at 6 dB, 20 iterations, L requested: wavefronts with one to three of their
    four lane groups idle from the start or from their last frame on, while the others run prologue, zip and epilogue;
    iteration counts from 1 to 20, so the groups that do work enter the zip out of step."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(4700 + len(name))
    ys = {"y%d_%d" % (B, k): awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, e)
          for B in (1, 3, 5, 67) for k, e in enumerate((3.5, 6.0))}
    keys = sorted(ys)
    spec = [{"tag": TAGS[name][0], "kw": TAGS[name][1], "iterations": 20, "stop": O2, "y": yk, "erasures": None} for yk in keys]
    gen = _generic(tmp_path, spec, ys)
    seen = set()
    for k, yk in enumerate(keys):
        res = _check(o, name, 20, O2, ys[yk], None, gen, k, (name, yk))
        seen.update(np.asarray(res["iters"]).tolist())
    assert 1 in seen and 20 in seen, sorted(seen)


def test_erasures(tmp_path):
    """16 frames at 4 dB, MS<3>; eight of them with 1 .. 64 erased positions (channel value 0): rows with m1 = m2 = 0,
    where r = +-0 must keep the sign the reference gives it through both halves of the zip."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(470)
    y = awgn_llr(rng, np.zeros((16, o.n), np.uint8), o.l / o.n, 4.0)
    erasures = [sorted(rng.choice(o.n, 2 ** (f // 2), replace=False).tolist()) if f % 2 == 0 and f < 14 else [] for f in range(16)]
    erasures[15] = sorted(rng.choice(o.n, 3, replace=False).tolist())
    assert sum(1 for e in erasures if e) == 8
    spec = [{"tag": TAGS["MS"][0], "kw": {}, "iterations": 3, "stop": stop, "y": "y", "erasures": erasures} for stop in (O1, O2)]
    gen = _generic(tmp_path, spec, {"y": y})
    for k, stop in enumerate((O1, O2)):
        _check(o, "MS", 3, stop, y, erasures, gen, k, ("erasures", stop))
