"""Fixture loaders of the ViT-Small / ViT-Tiny OSTrack tests (tests/test_vit_small_host.py, tests/test_gpu_vit_small.py): the reference's own
outputs at widths 384 / 6 heads and 192 / 3 heads (tests/golden/make_golden_vit_small.py).  Tolerances are tests/test_gpu_vitb.py's own,
imported there: depth <= 12 and its bf16 law has no width term."""
import os

import numpy as np

from conftest import GOLDEN_DIR

MARGIN = 0.03
#: model name -> width, heads
WIDTHS = {"vits": (384, 6), "vitt": (192, 3)}
#: geometry name -> template / search side, template / search tokens, map side
GEO = {"256": dict(TZ=128, TX=256, LZ=64, LX=256, F=16), "384": dict(TZ=192, TX=384, LZ=144, LX=576, F=24)}
#: file -> model, geometry, depth, seed, rows, activations kept
PLAIN = {"ref_vits_s502.npz": ("vits", "256", 12, 502, [1, 3, 6, 7], True),
         "ref_vits_s503.npz": ("vits", "256", 12, 503, [1, 9, 10, 15], False),
         "ref_vitt_s524.npz": ("vitt", "256", 12, 524, [4, 8, 9, 14], True),
         "ref_vitt_s527.npz": ("vitt", "256", 12, 527, [1, 9, 14, 15], False),
         "ref_vs384_s562.npz": ("vits", "384", 3, 562, [0, 1, 5], True),
         "ref_vt384_s541.npz": ("vitt", "384", 3, 541, [1, 3, 6], True)}
U8 = "ref_vits_u8_s600.npz"
TRACK = "ref_vits_track_s615.npz"
ACT_BLOCKS = {12: (0, 5, 11), 3: (0, 2)}

_SD = {}


def sd_of(model, geo, depth, seed):
    """One synthetic state dict per (model, geometry, depth, seed) for the whole session (at most 22 M parameters)."""
    from vittracker_amd import synth
    key = (model, geo, depth, seed)
    if key not in _SD:
        C, heads = WIDTHS[model]
        _SD[key] = synth.synth_vitb_state_dict(seed, C=C, depth=depth, heads=heads, len_z=GEO[geo]["LZ"], len_x=GEO[geo]["LX"])
    return _SD[key]


def path_of(name):
    return os.path.join(GOLDEN_DIR, name)


def load_plain(name):
    """(fixture, state dict, z, x): the samples `rows` of the seed's 16-sample input pool, weights regenerated and checked."""
    from vittracker_amd import synth
    model, geo, depth, seed, rows, _ = PLAIN[name]
    g = dict(np.load(path_of(name), allow_pickle=False))
    assert (int(g["seed"]), g["rows"].tolist(), int(g["depth"]), int(g["channels"]), int(g["heads"])) == (seed, rows, depth) + WIDTHS[model]
    sd = sd_of(model, geo, depth, seed)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z, x = synth.synth_inputs(seed, int(g["pool"]), GEO[geo]["TZ"], GEO[geo]["TX"])
    return g, sd, np.ascontiguousarray(z[rows]), np.ascontiguousarray(x[rows])


def load_u8():
    """(fixture, state dict, z, uint8 patches) of the ViT-Small uint8-patch fixture at 128 / 256."""
    from vittracker_amd import synth
    g = dict(np.load(path_of(U8), allow_pickle=False))
    seed, rows = int(g["seed"]), g["rows"]
    sd = sd_of("vits", "256", 12, seed)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z = synth.synth_inputs(seed, int(g["pool"]), 128, 256)[0]
    patches = synth.synth_patches(seed, int(g["pool"]), 256)
    assert int(patches.astype(np.uint64).sum()) == int(g["patch_checksum"]), "synth_patches drifted from the fixture generator"
    return g, sd, np.ascontiguousarray(z[rows]), np.ascontiguousarray(patches[rows])


def cfg_of(yaml_name):
    from conftest import REPO
    from vittracker_amd.config import fresh_cfg, update_config_from_file
    cfg = fresh_cfg()
    update_config_from_file(os.path.join(REPO, "experiments", "ostrack", yaml_name + ".yaml"), cfg)
    return cfg


def small_cfg(model, geo, ce_loc=()):
    """The cfg build_small_ostrack reads: the geometry's ViT-Base YAML with TYPE vit_base_patch16_224_ce, CHANNELS / HEADS of the model."""
    cfg = cfg_of("vitb_" + geo)
    bb = cfg.MODEL.BACKBONE
    bb.TYPE, (bb.CHANNELS, bb.HEADS) = "vit_base_patch16_224_ce", WIDTHS.get(model, model)
    bb.CE_LOC = list(ce_loc)
    bb.CE_KEEP_RATIO = [0.7] * len(ce_loc)
    return cfg
