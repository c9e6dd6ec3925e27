"""Resource gate of the kernel instantiations the ViT-Small / ViT-Tiny widths add (vitb.hip at C = 384 / 192), as
tests/test_resource_usage_ce_compact.py holds the compact form's: ScratchSize 0, no VGPR or SGPR spill, inside the register cap of their
workgroups.  New code: vbm::layernorm_small_kernel (64 lanes x float2 / float x 3), the A_ANYK GEMMs (the 256 x 256 tile on the two-buffer loop,
for an odd number of k-tiles).  New instantiations of existing code: vbm::ln_finalize_kernel<6 / 3>, vbq::qkv_attn_wide_kernel<384 / 192>.
Every vitb.hip row recorded in profiles/r6_resource_usage.txt before this change must compile exactly as recorded: the wide GEMMs (EPI_VT
gained a wave-uniform early return), layernorm_kernel<768 / 1024>, the fused qkv + attention kernels at 768 / 1024.
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

# kernel -> VGPR + AGPR cap: 512 registers per SIMD lane over the waves that must fit (256-thread workgroups, one wave per SIMD: 512; the
# 512-thread GEMM and fused attention workgroups, two waves per SIMD: 256)
NEW = {"vbm::layernorm_small_kernel<384>": 512, "vbm::layernorm_small_kernel<192>": 512, "vbm::ln_finalize_kernel<6>": 512, "vbm::ln_finalize_kernel<3>": 512,
       "vbq::qkv_attn_wide_kernel<384>": 256, "vbq::qkv_attn_wide_kernel<192>": 256,
       "vbg::gemm_kernel<256, 256, 2, 4, 2, 1>": 256, "vbg::gemm_kernel<256, 256, 2, 4, 2, 5>": 256, "vbg::gemm_kernel<256, 256, 2, 4, 2, 2>": 256,
       "vbg::gemm_kernel<256, 256, 2, 4, 2, 3>": 256}
KNOWN_OCC = {"vbc::ce_score_all_kernel<320>": 4}      # recorded as 5 (tests/test_resource_usage_ce_compact.py)
ROW = re.compile(r"^(\S.*?)\s+vgpr\s+(\d+)\s+scratch\s+(\d+)\s+vgpr-spill\s+(\d+)\s+sgpr-spill\s+(\d+)\s+occupancy (\d+)$")


@pytest.fixture(scope="module")
def rows():
    import resource_table as rt
    return {r["name"]: r for r in rt.table("vitb.hip")}


def _recorded():
    """The vitb.hip section of the recorded table."""
    out, on = {}, False
    for ln in open(os.path.join(REPO, "profiles", "r6_resource_usage.txt")):
        if ln.startswith("## "):
            on = ln.startswith("## vitb.hip")
            continue
        m = ROW.match(ln.rstrip())
        if on and m:
            out[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return out


def test_new_instantiations_have_no_scratch_and_fit_their_caps(rows):
    for name, cap in NEW.items():
        assert name in rows, (name, sorted(rows))
        r = rows[name]
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
        assert r["vgpr"] + r.get("agpr", 0) <= cap, r
    assert rows["vbq::qkv_attn_wide_kernel<384>"]["occ"] >= 2 and rows["vbq::qkv_attn_wide_kernel<192>"]["occ"] >= 2
    # every kernel of the file is accounted for: recorded before, or listed above and recorded with this change
    rec = _recorded()
    assert set(rows) <= set(rec), sorted(set(rows) - set(rec))
    for name in NEW:
        assert rec[name][:4] == (rows[name]["vgpr"], 0, 0, 0), (name, rec[name], rows[name])


def test_preexisting_rows_compile_as_recorded(rows):
    seen = 0
    for name, want in _recorded().items():
        if name in NEW:
            continue
        r = rows[name]
        assert (r["vgpr"], r["scratch"], r["vspill"], r["sspill"]) == want[:4], (name, r, want)
        assert r["occ"] == KNOWN_OCC.get(name, want[4]), (name, r, want)
        seen += 1
    assert seen >= 40, seen
