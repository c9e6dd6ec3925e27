"""Fixture loaders and tolerances of the ViT-Large OSTrack tests (tests/test_vitl_host.py, tests/test_gpu_vitl.py): the reference's own
outputs at width 1024 / 16 heads / depth 24 (tests/golden/make_golden_vitl.py), ``ref_vitl_*`` at 128 / 256 and ``ref_vl384_*`` at
192 / 384.  State dicts are synthesised once per (seed, geometry, depth) and shared: 1.25 GB and about 9 s each at depth 24."""
import glob
import os

import numpy as np

from conftest import GOLDEN_DIR

C, HEADS, DEPTH = 1024, 16, 24
MARGIN = 0.045          # the ViT-Base rule of 0.03 x sqrt(24 / 12): the fixtures' raw and Hann top-2 margins all exceed it
#: geometry name -> template / search side, template / search tokens, map side, fixture prefix
GEO = {"256": dict(TZ=128, TX=256, LZ=64, LX=256, F=16, prefix="ref_vitl"), "384": dict(TZ=192, TX=384, LZ=144, LX=576, F=24, prefix="ref_vl384")}


def TOL_REL(n):          # tests/test_gpu_vitb.py's stated bf16 law, as written there: its per-block term is relative and does not depend on the width
    return 2.0e-3 * (n ** 0.5)


# tests/test_gpu_vitb.py's TOL_MAP / TOL_BOX (2.2e-2, 2.2e-2, 4.4e-2; 9e-3) x sqrt(24 / 12): the head reads features that carry TOL_REL(24)
TOL_MAP = {"score_map": 3.1e-2, "size_map": 3.1e-2, "offset_map": 6.2e-2}
TOL_BOX = 1.3e-2


def plain_files(geo):
    """ref_vitl_s<seed>.npz / ref_vl384_s<seed>.npz (the uint8 and tracking fixtures carry a word after the prefix)."""
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, GEO[geo]["prefix"] + "_s*.npz")))


def all_plain():
    return [(geo, p) for geo in ("256", "384") for p in plain_files(geo)]


def u8_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_vitl_u8_s*.npz")))


def track_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_vitl_track_s*.npz")))


_SD = {}


def sd_vitl(seed, geo="256", depth=DEPTH):
    from vittracker_amd import synth
    key = (seed, geo, depth)
    if key not in _SD:
        _SD[key] = synth.synth_vitb_state_dict(seed, C=C, depth=depth, heads=HEADS, len_z=GEO[geo]["LZ"], len_x=GEO[geo]["LX"])
    return _SD[key]


def drop_sd(seed, geo="256", depth=DEPTH):
    """Let go of a depth-24 state dict (1.25 GB) once every model that needs it is built."""
    _SD.pop((seed, geo, depth), None)


def load_plain(geo, path):
    """(fixture, state dict, z, x): the samples `rows` of the seed's 16-sample input pool, weights regenerated and checked."""
    from vittracker_amd import synth
    g = dict(np.load(path, allow_pickle=False))
    seed, rows = int(g["seed"]), g["rows"]
    sd = sd_vitl(seed, geo)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z, x = synth.synth_inputs(seed, int(g["pool"]), GEO[geo]["TZ"], GEO[geo]["TX"])
    assert len(rows) == int(g["B"])
    return g, sd, np.ascontiguousarray(z[rows]), np.ascontiguousarray(x[rows])


def load_u8(path):
    """(fixture, state dict, z, uint8 patches) of the uint8-patch fixture at 128 / 256."""
    from vittracker_amd import synth
    g = dict(np.load(path, allow_pickle=False))
    seed, rows = int(g["seed"]), g["rows"]
    sd = sd_vitl(seed, "256")
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z = synth.synth_inputs(seed, int(g["pool"]), 128, 256)[0]
    patches = synth.synth_patches(seed, int(g["pool"]), 256)
    assert int(patches.astype(np.uint64).sum()) == int(g["patch_checksum"]), "synth_patches drifted from the fixture generator"
    return g, sd, np.ascontiguousarray(z[rows]), np.ascontiguousarray(patches[rows])
