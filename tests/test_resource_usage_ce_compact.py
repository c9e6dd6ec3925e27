"""Resource gate of the kernels of the compact form of candidate elimination (vb_attn_stream.h attn_stream_rt_kernel, vb_ce.h), as
tests/test_resource_usage_formats.py holds the crop kernels: ScratchSize 0, no VGPR or SGPR spill, the run-time attention kernel inside the
256 VGPRs of two workgroups per CU and the others inside the cap of their 256-thread workgroups.  The streaming attention kernels and the
masked form's kernels must compile exactly as recorded in profiles/r6_resource_usage.txt: the new kernel shares their helpers.
Compiles vitb.hip with the Makefile's flags (tools/resource_table.py; no GPU needed; skipped where hipcc is absent)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

if shutil.which("hipcc") is None:
    pytest.skip("hipcc not on PATH: the resource gate needs the compiler", allow_module_level=True)

sys.path.insert(0, os.path.join(REPO, "tools"))

# kernel -> VGPR cap (512 VGPRs per SIMD lane over the waves of a 256-thread workgroup that must fit: one wave per SIMD -> 512; the
# attention kernel's two workgroups per CU -> 256)
NEW = {"vbs::attn_stream_rt_kernel": 256, "vbc::ce_score_rt_kernel<5>": 512, "vbc::ce_score_rt_kernel<12>": 512, "vbc::ce_score_all_rt_kernel": 512,
       "vbc::ce_select_compact_kernel": 512, "vbc::ce_gather_kernel": 512, "vbc::ce_final_norm_kernel<768>": 512, "vbc::ce_scatter_rows_kernel": 512}
KNOWN_OCC = {"vbc::ce_score_all_kernel<320>": 4}      # recorded as 5
RECORDED = re.compile(r"^(vbs::attn_stream\w*kernel<\d+>|vbc::\S+)\s+vgpr\s+(\d+)\s+scratch\s+(\d+)\s+vgpr-spill\s+(\d+)\s+sgpr-spill\s+(\d+)\s+occupancy (\d+)$")


@pytest.fixture(scope="module")
def rows():
    import resource_table as rt
    return {r["name"]: r for r in rt.table("vitb.hip")}


def test_new_kernels_have_no_scratch_and_fit_their_caps(rows):
    for name, cap in NEW.items():
        assert name in rows, (name, sorted(n for n in rows if n.startswith(("vbs::", "vbc::"))))
        r = rows[name]
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
        assert r["vgpr"] + r.get("agpr", 0) <= cap, r
    assert rows["vbs::attn_stream_rt_kernel"]["occ"] >= 2


def test_existing_attention_and_ce_rows_compile_as_recorded(rows):
    """Every vbs:: / vbc:: row of the recorded table that was there before the compact form: the same VGPRs, scratch, spills and occupancy.
    One recorded cell is known to disagree with the compile (KNOWN_OCC): the record says occupancy 5 for ce_score_all_kernel<320>, and the
    commit that recorded it compiles to 4 itself (84 VGPRs + 20 AGPRs, which the table does not list).  The recorded row is left as it
    is and the compile is held to 4."""
    seen = 0
    for ln in open(os.path.join(REPO, "profiles", "r6_resource_usage.txt")):
        m = RECORDED.match(ln.rstrip())
        if not m or m.group(1) in NEW:
            continue
        name, want = m.group(1), tuple(int(v) for v in m.groups()[1:])
        r = rows[name]
        assert (r["vgpr"], r["scratch"], r["vspill"], r["sspill"]) == want[:4], (name, r, want)
        assert r["occ"] == KNOWN_OCC.get(name, want[4]), (name, r, want)
        seen += 1
    assert seen >= 10, seen      # four streaming attention kernels, six masked-form CE kernels
