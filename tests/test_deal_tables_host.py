"""The deal of the diagonals to lanes and slots (csrc/minsum_diag.hip: build_paired_table / build_diag_table, read
through cc_diag_table) decides which LDS bank serves an edge of the diagonal min-sum kernel.  Pinned here: the deal of
every geometry, against tables recorded from the build before the row block's LDS work was re-priced
(profiles/r26_experiments.md), and for the headline geometry the properties the kernel relies on and the bank-conflict
cost that profiles/tools/deal_model.py prices it at -- the figure every later deal has to beat."""
import ctypes as C
import json
import os
import sys

import numpy as np

import channelcoding_amd as cc
from channelcoding_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

GEOMETRIES = [(q, t) for q, ts in ((4, (1, 2, 3)), (5, (1, 2, 3, 5)), (6, (1, 2, 3, 4)), (7, (1, 2, 3, 4)), (8, (1, 2, 3, 4)))
              for t in ts]


def _table(q, t):
    code = cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(5), device=capi.DEVICE_NONE)
    out = np.zeros(1024, np.uint16)
    D, LPF, links = C.c_uint32(), C.c_uint32(), C.c_uint32()
    m = capi.lib().cc_diag_table(code._h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(D), C.byref(LPF), C.byref(links))
    assert m == D.value * LPF.value and m > 0, (q, t, m)
    return code, out[:m].reshape(D.value, LPF.value).astype(int), links.value


def test_headline_deal_and_its_modelled_cost():
    """BCH(255,231): all 112 support diagonals dealt exactly once, no empty slot, slots (0,1) and (2,3) gap-1 pairs in
    every lane; the table is the one deal_model.round2_paired_table rebuilds, and the model prices it at 10 + 10 + 10
    extra LDS cycles per row and wavefront ({cs, y} reads, cs' reads, cs' writes)."""
    import deal_model
    code, table, links = _table(8, 3)
    H = code.H()
    support = [j for j in range(code.n) if H[0, j]]
    assert support == deal_model.SUPPORT_255_231 and len(support) == 112
    assert table.shape == (7, 16) and links == 2
    assert sorted(table.ravel().tolist()) == support
    assert 0xFFFF not in table
    for p in range(2):
        assert np.array_equal(table[2 * p + 1], table[2 * p] + 1), p
    model = deal_model.round2_paired_table(support, 255)
    assert np.array_equal(np.array(model), table)
    assert deal_model.cost_round2_layout(model) == (10, 10, 10)
    assert deal_model.cost_round2_layout(table.tolist()) == (10, 10, 10)


def test_every_geometry_keeps_its_recorded_deal():
    """tests/golden/diag_tables.json: the tables of the 19 geometries as the library built them before this test existed."""
    with open(os.path.join(ROOT, "tests", "golden", "diag_tables.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted("%d,%d" % g for g in GEOMETRIES)
    for q, t in GEOMETRIES:
        _, table, links = _table(q, t)
        rec = want["%d,%d" % (q, t)]
        assert links == rec["links"] and table.tolist() == rec["table"], (q, t)
