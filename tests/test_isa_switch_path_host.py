"""profiles/tools/isa_switch_path.py: what follows the longest basic block of a function, counted on hand-written
assembly with a known tail."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASM = """
_Z6kernelv:
	s_load_dword s0, s[4:5], 0x0
.LBB0_1:
	v_add_f32_e32 v0, v1, v2
	ds_read_b64 v[4:5], v3
	s_waitcnt lgkmcnt(0)
	v_add_f32_e32 v0, v0, v4
	ds_write_b32 v3, v0
	s_cbranch_scc1 .LBB0_3
.LBB0_2:
	ds_read2_b32 v[6:7], v3 offset1:16
	s_and_saveexec_b64 s[2:3], vcc
	v_mov_b32_e32 v8, 0
	s_waitcnt lgkmcnt(0)
	global_store_byte v[10:11], v6, off
.LBB0_3:
	s_or_b64 exec, exec, s[2:3]
	s_waitcnt vmcnt(0)
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
"""


def test_counts_behind_the_longest_block(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "tools", "isa_switch_path.py"), str(p), "kernel"],
                       capture_output=True, text=True, check=True)
    got = json.loads(r.stdout)
    assert got == {"loop_block": 6, "after": 9, "blocks_after": 2, "valu": 1, "salu": 4, "v_mov_b32": 1, "vmem": 1,
                   "saveexec": 1, "waits_on_lgkmcnt": 1, "lds": 1, "lds_by_opcode": {"ds_read2_b32": 1}}
