"""The instance-minor tables shared by the three evaluators' generated paths (awebox_amd/csrc/
im_tables.hpp), on the host: csrc/gen/check_im_tables.cpp checks the slot table of each generated
node header for d = 1..5 (first = prefix sum of cnt, cnt = d exactly for the xdot directions of a
Radau node) and the builder of the destination tables on a synthetic problem (expected arrays, and
the refusal of a duplicate, a missing and an out-of-count destination).

The d = 4 totals the checker compares against are those of the three per-evaluator tables this
header replaced (SoaSlotTab<4> of awegpu.hip, GenSlotTab(4) of awempc.hip, SlotTab(4) of
awedual_gen.hip), printed once from those constructors at the commit before they were removed."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awebox_amd", "csrc")


def test_slot_tables_and_destination_builder(tmp_path):
    exe = str(tmp_path / "check_im_tables")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "gen", "check_im_tables.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout)
    assert rec == {"ok": True, "ap2": [347, 431], "kite3": [81, 153], "dual": [860, 1067]}
