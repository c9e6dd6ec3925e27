"""Resource gate of the pixel-format crop kernels after the wide layouts (YV16 / YV24, NV16 / NV24, P210 / P410, the planar 16-bit
layouts with their 16-bit fetch family): the fourteen instantiations are all still there under their names, each without scratch or
spills; the band kernels -- the register count is the maximum over a kernel's format families, the 16-bit one included -- stay within
128 VGPRs at occupancy 4 or more; a kernel of its own for the new family, should one appear, is without scratch.  Compiled as
tests/test_resource_usage_formats.py does (tools/resource_table.py; no GPU needed)."""
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
KNOWN = re.compile(r"vtt::crop_(band_)?image_kernel<")


@pytest.fixture(scope="module")
def rows():
    import resource_table as rt
    return rt.table("vittrack.hip")


def test_the_fourteen_instantiations_hold_their_caps(rows):
    for pat, count in KERNELS:
        hit = [r for r in rows if re.fullmatch(pat, r["name"])]
        assert len(hit) == count, (pat, [r["name"] for r in hit])
        for r in hit:
            print(r["name"], "vgpr", r["vgpr"], "agpr", r.get("agpr", 0), "scratch", r["scratch"], "occupancy", r.get("occ"))
            assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
            if "band" in r["name"]:
                assert r["vgpr"] + r.get("agpr", 0) <= CAP and r["occ"] >= 4, r
    assert sum(1 for r in rows if "image" in r["name"] and "crop" in r["name"]) >= 14


def test_a_new_crop_image_kernel_has_no_scratch(rows):
    for r in rows:
        if "image" in r["name"] and "crop" in r["name"] and not KNOWN.match(r["name"]):
            assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r


def test_the_sixteen_bit_family_is_in_the_source_of_both_kernels():
    """The family lives inside the two kernels: a 16-bit buffer load behind the uniform wide_shift branch, in crop_image_kernel and in
    crop_band_image_ext."""
    src = open(os.path.join(REPO, "vittracker_amd", "csrc", "vt_track.h")).read()
    gen = src[src.index("void crop_image_kernel("):src.index("void crop_band_image_ext(")]
    band = src[src.index("void crop_band_image_ext("):src.index("void crop_band_image_kernel(")]
    for body in (gen, band):
        assert "raw_buffer_load_b16" in body and "wide_shift(fmt)" in body
