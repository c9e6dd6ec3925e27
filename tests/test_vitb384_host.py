"""Host side of the ViT-Base 384 geometry (192 px template / 384 px search, 144 + 576 = 720 tokens, 24 x 24 maps): the pinned torch oracle
against the reference's own outputs (tests/golden/make_golden_vitb384.py), vt_create's argument checks, the ostrack parameter module on
experiments/ostrack/vitb_384.yaml.  No GPU.  Also the loaders the GPU tests of this geometry share."""
import ctypes
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, REPO

TZ, TX, LZ, LX, F = 192, 384, 144, 576, 24


def vb384_files():
    """The plain fixtures ref_vb384_s<seed>.npz (the uint8 and tracking ones carry a word after the prefix)."""
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_vb384_s*.npz")))


def vb384_u8_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_vb384_u8_s*.npz")))


_SD = {}


def sd384(seed, depth=12):
    from vittracker_amd import synth
    if (seed, depth) not in _SD:
        _SD[(seed, depth)] = synth.synth_vitb_state_dict(seed, depth=depth, len_z=LZ, len_x=LX)
    return _SD[(seed, depth)]


def load_vb384(path):
    """(fixture, state dict, z, x): the samples `rows` of the seed's 16-sample input batch, weights regenerated and checked."""
    from vittracker_amd import synth
    g = dict(np.load(path, allow_pickle=False))
    seed, rows = int(g["seed"]), g["rows"]
    sd = sd384(seed)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z, x = synth.synth_inputs(seed, int(g["pool"]), TZ, TX)
    assert len(rows) == int(g["B"])
    return g, sd, np.ascontiguousarray(z[rows]), np.ascontiguousarray(x[rows])


def load_vb384_u8(path):
    """(fixture, state dict, z, uint8 patches) of the uint8-patch fixture: the samples `rows` of the seed's 16."""
    from vittracker_amd import synth
    g = dict(np.load(path, allow_pickle=False))
    seed, rows = int(g["seed"]), g["rows"]
    sd = sd384(seed)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z = synth.synth_inputs(seed, int(g["pool"]), TZ, TX)[0]
    patches = synth.synth_patches(seed, int(g["pool"]), TX)
    assert int(patches.astype(np.uint64).sum()) == int(g["patch_checksum"]), "synth_patches drifted from the fixture generator"
    return g, sd, np.ascontiguousarray(z[rows]), np.ascontiguousarray(patches[rows])


def test_fixture_set_is_what_the_generator_writes():
    names = [os.path.basename(p) for p in vb384_files()]
    assert names == ["ref_vb384_s108.npz", "ref_vb384_s116.npz"]
    assert len(vb384_u8_files()) == 1
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "ref_vitb_*.npz")))
    for p in glob.glob(os.path.join(GOLDEN_DIR, "ref_vb384_*.npz")):
        assert os.path.getsize(p) <= largest, p
    g = dict(np.load(vb384_files()[0]))
    assert g["rows"].tolist() == [1, 6, 10, 12] and {0, 143, 144, 145, 703, 704, 719} <= set(g["act_rows"].tolist())
    assert dict(np.load(vb384_files()[1]))["rows"].tolist() == [3, 8, 13]


@pytest.mark.parametrize("path", vb384_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_torch_oracle_matches_the_reference_at_384(path):
    """oracle/vitb_oracle_torch.py built from the fixture's state dict against the reference's maps, boxes and kept activation rows, at
    the tolerances tests/test_oracle_golden.py uses for the 256 fixtures (5e-5 outputs, 2e-4 activations).  Every sample's margins > 0.03."""
    import torch
    from oracle import vitb_oracle_torch as ob
    g, sd, z, x = load_vb384(path)
    with_acts = "act_norm" in g
    if with_acts:
        z, x = z[:1], x[:1]          # the activations are the first sample's; its outputs are compared below, the others' in the second run
    m = ob.build_from_state(sd)
    acts = {}
    with torch.no_grad():
        out = m(torch.from_numpy(z), torch.from_numpy(x), acts)
    n = z.shape[0]
    for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(out[k].numpy(), g[k][:n], atol=5e-5, rtol=0, err_msg=k)
    assert out["score_map"].shape[-2:] == (F, F)
    assert min(g["margin_raw"].min(), g["margin_hann"].min()) > 0.03
    if with_acts:
        rows = g["act_rows"]
        for k in ("tokens", "block0", "block3", "block5", "block11", "norm"):
            np.testing.assert_allclose(acts[k][:1, rows].numpy(), g["act_" + k], atol=2e-4, rtol=0, err_msg=k)
        g2, _, z2, x2 = load_vb384(path)
        with torch.no_grad():
            rest = m(torch.from_numpy(z2[1:]), torch.from_numpy(x2[1:]))
        for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
            np.testing.assert_allclose(rest[k].numpy(), g2[k][1:], atol=5e-5, rtol=0, err_msg=k)
    mac = ob.macs_per_frame(TZ, TX)
    assert abs(sum(mac.values()) / sum(ob.macs_per_frame(128, 256).values()) - 2.42) < 0.02


def test_torch_oracle_matches_the_uint8_fixture_at_384():
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import synth
    g, sd, z, patches = load_vb384_u8(vb384_u8_files()[0])
    x = synth.normalise_patches(patches[:2], reciprocal=False)
    acts = {}
    with torch.no_grad():
        out = ob.build_from_state(sd)(torch.from_numpy(z[:2]), torch.from_numpy(x), acts)
    for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(out[k].numpy(), g[k][:2], atol=5e-5, rtol=0, err_msg=k)
    np.testing.assert_allclose(acts["tokens"][:2, g["act_rows"]].numpy(), g["act_tokens"], atol=2e-4, rtol=0)
    assert min(g["margin_raw"].min(), g["margin_hann"].min()) > 0.03


@pytest.mark.parametrize("cfg", [(192, 384, 768, 8, 12, 256, 16, 1), (160, 320, 768, 12, 12, 256, 16, 1), (192, 256, 768, 12, 12, 256, 16, 1)],
                         ids=["heads8", "160-320", "192-256"])
def test_vt_create_rejects_other_vitb_configurations_before_any_hip_call(cfg):
    from vittracker_amd import native
    L = native.lib()
    h = ctypes.c_void_p()
    c = native.VtConfig(*cfg)
    assert L.vt_create(ctypes.byref(c), ctypes.byref(h)) == -1
    msg = L.vt_last_error()
    assert b"unsupported ViT-Base" in msg and b"128 / search 256" in msg and b"192 / search 384" in msg, msg


def test_parameters_of_vitb_384():
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters("vitb_384")
    assert (p.search_size, p.search_factor, p.template_size, p.template_factor) == (384, 5.0, 192, 2.0)
    assert (int(p.cfg.DATA.SEARCH.SIZE), float(p.cfg.DATA.SEARCH.FACTOR), int(p.cfg.DATA.TEMPLATE.SIZE), float(p.cfg.DATA.TEMPLATE.FACTOR)) == (384, 5.0, 192, 2.0)
    assert p.checkpoint.endswith("checkpoints/train/ostrack/vitb_384/OSTrack_ep0300.pth.tar")
    assert int(p.cfg.MODEL.BACKBONE.CHANNELS) == 768 and int(p.cfg.MODEL.HEAD.NUM_CHANNELS) == 256
