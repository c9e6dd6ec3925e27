"""The candidate-elimination fixtures tests/golden/ref_vbce_*.npz (tests/golden/make_golden_vitb_ce.py: outputs of the reference's own
``vit_base_patch16_224_ce`` model) for tests/test_vitb_ce_host.py and tests/test_gpu_vitb_ce.py: listing, loading (weights and inputs
regenerated from the seed and checked), and the CPU oracle runs, each computed once per process and shared."""
from __future__ import annotations

import glob
import os

import numpy as np

from conftest import GOLDEN_DIR

_CACHE = {}


def files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_vbce_*.npz")))


def ids(p):
    return os.path.basename(p)[:-4]


def preprocess(patches):
    """Preprocessor.process (lib/test/tracker/data_utils.py:11-17) as the fixture generator applied it (torch on the CPU divides)."""
    import torch
    mean = torch.tensor([0.485, 0.456, 0.406]).view((1, 3, 1, 1))
    std = torch.tensor([0.229, 0.224, 0.225]).view((1, 3, 1, 1))
    img = torch.tensor(patches).float().permute((0, 3, 1, 2))
    return (((img / 255.0) - mean) / std).contiguous().numpy()


def load(path):
    """-> dict: the fixture's arrays under 'g', 'sd', 'z', 'x' (fp32 crops), 'patches' (uint8 (B,S,S,3) or None), and the configuration
    ('tz', 'tx', 'lz', 'lx', 'depth', 'loc', 'ratio', 'range', 'B', 'n')."""
    if path in _CACHE:
        return _CACHE[path]
    from vittracker_amd import synth
    g = dict(np.load(path, allow_pickle=False))
    seed, B, tz, tx, depth = (int(g[k]) for k in ("seed", "B", "template_size", "search_size", "depth"))
    lz, lx = (tz // 16) ** 2, (tx // 16) ** 2
    sd = synth.synth_vitb_state_dict(seed, depth=depth, len_z=lz, len_x=lx)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    patches = None
    if "rows" in g:
        z, x = synth.synth_inputs(seed, int(g["pool"]), tz, tx)
        z, x = z[g["rows"]], x[g["rows"]]
    elif "u8" in g:
        patches = synth.synth_patches(seed, B, tx)
        assert int(patches.astype(np.uint64).sum()) == int(g["patch_checksum"]), "synth_patches drifted from the fixture generator"
        z, x = synth.synth_inputs(seed, B, tz, tx)[0], preprocess(patches)
    else:
        z, x = synth.synth_inputs(seed, B, tz, tx)
    loc = [int(v) for v in g["ce_loc"]]
    c = {"g": g, "sd": sd, "z": np.ascontiguousarray(z), "x": np.ascontiguousarray(x), "patches": patches, "tz": tz, "tx": tx, "lz": lz, "lx": lx,
         "depth": depth, "loc": loc, "ratio": [float(v) for v in g["ce_keep_ratio"]], "range": str(g["ce_template_range"]), "B": B, "n": len(loc)}
    _CACHE[path] = c
    return c


def oracle_model(c):
    if "orc" not in c:
        from oracle import vitb_oracle_torch as ob
        c["orc"] = ob.build_from_state(c["sd"])
    return c["orc"]


def oracle_run(c, forced=None, x=None):
    """tests/vitb_ce_oracle.forward on the case (x: another search crop), with numpy keep sets in `forced`."""
    import torch
    import vitb_ce_oracle as vo
    rows = vo.template_rows(c["range"], c["tz"] // 16)
    return vo.forward(oracle_model(c), torch.from_numpy(c["z"]), torch.from_numpy(c["x"] if x is None else x), c["loc"], c["ratio"], rows, forced)


def top2(m):
    srt = np.sort(np.asarray(m).reshape(m.shape[0], -1), axis=1)
    return srt[:, -1] - srt[:, -2]
