"""Resource gate of the pixel-format crop kernels (vt_crop_images & co.), as tests/test_resource_usage.py holds the others: ScratchSize 0,
no VGPR spill, and the crop kernels' register cap of their 256-thread workgroups.  Compiles vittrack.hip with the Makefile's flags
(tools/resource_table.py; no GPU needed; skipped where hipcc is absent)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

if shutil.which("hipcc") is None:
    pytest.skip("hipcc not on PATH: the resource gate needs the compiler", allow_module_level=True)

sys.path.insert(0, os.path.join(REPO, "tools"))

NEW = [(r"vtt::crop_image_kernel<(false|true)>", 256), (r"vtt::crop_band_image_kernel<(false|true), [456], [24]>", 256)]


@pytest.fixture(scope="module")
def rows():
    import resource_table as rt
    return rt.table("vittrack.hip")


def test_format_kernels_have_no_scratch_and_fit_the_crop_cap(rows):
    for pat, cap in NEW:
        hit = [r for r in rows if re.fullmatch(pat, r["name"])]
        # every instantiation launch_crop_images can pick: two generic, twelve band forms (T = 64 / 128 / 256, 2 / 4 items, uint8 / fp32)
        assert len(hit) == (2 if "crop_image" in pat else 12), (pat, [r["name"] for r in hit])
        for r in hit:
            assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
            assert r["vgpr"] + r.get("agpr", 0) <= cap, r
