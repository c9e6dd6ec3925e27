"""Resource gate of the kernels the fp32-equivalent mode adds to vitb.hip (vt_set_precision; vb_f32.h, vb_misc.h, the EPI_F32 instantiations of
vbg::gemm_kernel), as tests/test_resource_usage_vit_small.py holds the small widths': ScratchSize 0, no VGPR or SGPR spill, inside the register
cap of their workgroups, and compiled exactly as recorded in profiles/r6_resource_usage.txt.  The bf16 mode's rows are held by the other
gates (every row recorded before must compile as recorded).  Compiles vitb.hip with the Makefile's flags (tools/resource_table.py, shared
with the other gates of the process; no GPU needed; skipped where hipcc is absent)."""
import os
import shutil
import sys

import pytest

from conftest import REPO

if shutil.which("hipcc") is None:
    pytest.skip("hipcc not on PATH: the resource gate needs the compiler", allow_module_level=True)

sys.path.insert(0, os.path.join(REPO, "tools"))

# kernel -> VGPR + AGPR cap: 256-thread workgroups, one wave per SIMD: 512; the 512-thread GEMM workgroups, two waves per SIMD: 256
NEW = {"vbm::layernorm_split_kernel<1024>": 512, "vbm::layernorm_split_kernel<768>": 512, "vbm::layernorm_split_kernel<384>": 512,
       "vbm::layernorm_split_kernel<192>": 512, "vbm::gelu_split_kernel": 512, "vbf::expand_weight_kernel": 512, "vbf::patchify_split_kernel": 512,
       "vbf::patchify_u8_split_kernel": 512, "vbf::attn_f32_kernel": 512, "vbf::map_split_kernel": 512, "vbf::conv5_f32_kernel<32>": 512,
       "vbg::gemm_kernel<256, 256, 2, 4, 0, 8>": 256, "vbg::gemm_kernel<128, 64, 8, 1, 0, 8>": 256, "vbg::gemm_kernel<256, 64, 8, 1, 1, 8>": 256,
       "vbg::gemm_kernel<128, 64, 8, 1, 1, 8>": 256}


@pytest.fixture(scope="module")
def rows():
    import resource_table as rt
    return {r["name"]: r for r in rt.table("vitb.hip")}


def test_the_modes_kernels_have_no_scratch_and_fit_their_caps(rows):
    from test_resource_usage_vit_small import _recorded
    rec = _recorded()
    for name, cap in NEW.items():
        assert name in rows, (name, sorted(rows))
        r = rows[name]
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
        assert r["vgpr"] + r.get("agpr", 0) <= cap, r
        assert rec[name][:4] == (r["vgpr"], 0, 0, 0), (name, rec[name], r)
    # two workgroups of the attention kernel fit a CU's registers and LDS (32 KiB each)
    assert rows["vbf::attn_f32_kernel"]["occ"] >= 2 and rows["vbf::attn_f32_kernel"]["lds"] == 32768
    # every kernel the mode adds is listed: nothing with its namespaces' names escapes the gate
    added = {n for n in rows if n.startswith("vbf::") or "_split_kernel" in n or n.endswith(", 8>")}
    assert added == set(NEW), sorted(added ^ set(NEW))
