"""profiles/tools/isa_mix.py, the LDS request-to-wait report (lds_strip): a dozen hand-written assembly lines with known
groups, counted and full waits, and the distances worked out by hand."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))

from isa_mix import blocks, lds_strip  # noqa: E402

ASM = """
.LBB0_1:
	ds_read_b64 v[0:1], v20
	ds_read_b64 v[2:3], v21 offset:8
	v_sub_f32_e32 v4, v5, v6
	v_add_f32_e32 v4, v4, v7
	ds_write_b32 v22, v4
	ds_read_b32 v8, v23
	ds_read_b32 v9, v23 offset:8
	v_min_u32_e32 v10, v11, v12
	s_waitcnt lgkmcnt(3)
	v_add_f32_e32 v0, v0, v2
	s_nop 1
	v_xor_b32_e32 v13, v14, v15
	v_mov_b32_e32 v16, v17
	s_waitcnt vmcnt(0)
	v_mov_b32_e32 v18, v19
	s_waitcnt lgkmcnt(0)
	v_add_f32_e32 v8, v8, v9
	ds_read_b32 v24, v23 offset:16
	s_cbranch_scc1 .LBB0_1
"""


def _block():
    return max((b for _, b in blocks(ASM.splitlines())), key=len)


def test_strip():
    strip, _ = lds_strip(_block())
    assert strip == ["ds_read_b64 x2", "2", "ds_write_b32 x1 + ds_read_b32 x2", "1", "lgkmcnt(3)", "1", "s_nop", "2",
                     "vmcnt(0)", "1", "lgkmcnt(0)", "1", "ds_read_b32 x1", "1"]


def test_summary():
    """The two ds_read_b64 have three younger LDS instructions behind them, so lgkmcnt(3) covers them: 2 + 1 other
    instructions after the group.  The write-and-read group is covered by lgkmcnt(0) only: 1 + 1 + 2 + 1 = 5 (the s_nop
    and the waits do not count).  The last read has no wait in the block and is left out."""
    _, s = lds_strip(_block())
    assert s == {"waits_on_lgkmcnt": 2, "waits_lgkmcnt_0": 1, "read_groups_covered": 2, "distance_min": 3,
                 "distance_median": 4.0}


def test_write_only_groups_have_no_distance():
    ins = [("ds_write_b32", "ds_write_b32 v0, v1"), ("v_mov_b32_e32", "v_mov_b32_e32 v2, v3"),
           ("s_waitcnt", "s_waitcnt lgkmcnt(0)")]
    strip, s = lds_strip(ins)
    assert strip == ["ds_write_b32 x1", "1", "lgkmcnt(0)"]
    assert s["read_groups_covered"] == 0 and s["distance_min"] is None and s["distance_median"] is None
