"""Resource gate of the pixel-format crop kernels after the layouts and colour rows added to them (I420 / YV12, YUYV / UYVY, P010,
GRAY8; BT.709 and full range): the fourteen instantiations are all still there, each without scratch or spills, and the register
count -- the maximum over a kernel's format families -- stays within 128 VGPRs, the occupancy-4 step of the band kernels' 256-thread
workgroups.  Compiled as tests/test_resource_usage_formats.py does (tools/resource_table.py; no GPU needed)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

if shutil.which("hipcc") is None:
    pytest.skip("hipcc not on PATH: the resource gate needs the compiler", allow_module_level=True)

sys.path.insert(0, os.path.join(REPO, "tools"))

KERNELS = [(r"vtt::crop_image_kernel<(false|true)>", 2), (r"vtt::crop_band_image_kernel<(false|true), [456], [24]>", 12)]
CAP = 128
#: every kernel of the translation unit that existed before; anything else with "crop" and "image" in its name is new
KNOWN = re.compile(r"vtt::crop_(band_)?image_kernel<")


@pytest.fixture(scope="module")
def rows():
    import resource_table as rt
    return rt.table("vittrack.hip")


def test_existing_instantiations_stay_within_128_registers(rows):
    for pat, count in KERNELS:
        hit = [r for r in rows if re.fullmatch(pat, r["name"])]
        assert len(hit) == count, (pat, [r["name"] for r in hit])
        for r in hit:
            print(r["name"], "vgpr", r["vgpr"], "agpr", r.get("agpr", 0), "scratch", r["scratch"], "occupancy", r.get("occ"))
            assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
            assert r["vgpr"] + r.get("agpr", 0) <= CAP, r
            if "band" in r["name"]:
                assert r["occ"] >= 4, r


def test_new_image_kernels_have_no_scratch_and_no_spills(rows):
    """The added families live inside the two kernels; should a later change move one into a kernel of its own, it is held here."""
    for r in rows:
        if "image" in r["name"] and "crop" in r["name"] and not KNOWN.match(r["name"]):
            assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r

