"""Host side of the ViT-Large OSTrack model point (width 1024, 16 heads, depth 24, MLP 4096; 128 / 256 and 192 / 384): the pinned torch
oracle against the reference's own outputs (tests/golden/make_golden_vitl.py), build_ostrack / the parameter module / the factory on
experiments/ostrack/vitl_{256,384}.yaml, the MAC ratio the timing section of DESIGN quotes.  No GPU."""
import os

import numpy as np
import pytest

from conftest import REPO
from vitl_cases import DEPTH, GEO, HEADS, MARGIN, all_plain, drop_sd, load_plain, load_u8, plain_files, track_files, u8_files

ACT_KEYS = ("tokens", "block0", "block5", "block11", "block12", "block23", "norm")


def test_fixture_set_is_what_the_generator_writes():
    assert [os.path.basename(p) for p in plain_files("256")] == ["ref_vitl_s206.npz", "ref_vitl_s209.npz"]
    assert [os.path.basename(p) for p in plain_files("384")] == ["ref_vl384_s206.npz", "ref_vl384_s207.npz"]
    assert [os.path.basename(p) for p in u8_files()] == ["ref_vitl_u8_s284.npz"]
    assert track_files() == []          # no seed of the generator's range keeps eight Hann margins above the rule
    want_rows = {"ref_vitl_s206": [0, 1, 5, 7], "ref_vitl_s209": [0, 2, 7, 8], "ref_vl384_s206": [3, 4, 6, 8], "ref_vl384_s207": [5, 13, 14]}
    for geo, p in all_plain():
        g = dict(np.load(p))
        assert g["rows"].tolist() == want_rows[os.path.basename(p)[:-4]]
        assert os.path.getsize(p) < (1 << 20)
    for geo in ("256", "384"):
        g = dict(np.load(plain_files(geo)[0]))
        for k in ACT_KEYS:
            assert g["act_" + k].shape == (1, len(g["act_rows"]), 1024), k
    assert {0, 63, 64, 65, 319} <= set(dict(np.load(plain_files("256")[0]))["act_rows"].tolist())
    assert {0, 143, 144, 145, 703, 704, 719} <= set(dict(np.load(plain_files("384")[0]))["act_rows"].tolist())


@pytest.mark.parametrize("geo,path", all_plain(), ids=lambda v: os.path.basename(v)[:-4] if v.endswith(".npz") else v)
def test_torch_oracle_matches_the_reference(geo, path):
    """oracle/vitb_oracle_torch.build_from_state(sd, heads=16) against the reference's maps, boxes and kept activation rows at the
    tolerances of tests/test_vitb384_host.py (5e-5 outputs, 2e-4 activations); the regenerated weights' checksum equals the stored one
    (load_plain); every stored margin exceeds 0.045."""
    import torch
    from oracle import vitb_oracle_torch as ob
    g, sd, z, x = load_plain(geo, path)
    m = ob.build_from_state(sd, heads=HEADS)
    assert len(m.backbone.blocks) == DEPTH and m.backbone.norm.weight.shape[0] == 1024
    acts = {}
    with torch.no_grad():
        out = m(torch.from_numpy(z), torch.from_numpy(x), acts)
    for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(out[k].numpy(), g[k], atol=5e-5, rtol=0, err_msg=k)
    assert out["score_map"].shape[-2:] == (GEO[geo]["F"], GEO[geo]["F"])
    assert min(g["margin_raw"].min(), g["margin_hann"].min()) > MARGIN
    if "act_norm" in g:
        rows = g["act_rows"]
        for k in ACT_KEYS:
            np.testing.assert_allclose(acts[k][:1, rows].numpy(), g["act_" + k], atol=2e-4, rtol=0, err_msg=k)
    drop_sd(int(g["seed"]), geo)


def test_torch_oracle_matches_the_uint8_fixture():
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import synth
    g, sd, z, patches = load_u8(u8_files()[0])
    x = synth.normalise_patches(patches, reciprocal=False)
    acts = {}
    with torch.no_grad():
        out = ob.build_from_state(sd, heads=HEADS)(torch.from_numpy(z), torch.from_numpy(x), acts)
    for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(out[k].numpy(), g[k], atol=5e-5, rtol=0, err_msg=k)
    np.testing.assert_allclose(acts["tokens"][:2, g["act_rows"]].numpy(), g["act_tokens"], atol=2e-4, rtol=0)
    assert min(g["margin_raw"].min(), g["margin_hann"].min()) > MARGIN
    drop_sd(int(g["seed"]))


def _cfg(name):
    from vittracker_amd.config import fresh_cfg, update_config_from_file
    cfg = fresh_cfg()
    update_config_from_file(os.path.join(REPO, "experiments", "ostrack", name + ".yaml"), cfg)
    return cfg


def test_build_ostrack_on_the_vitl_yamls():
    """The TYPE decides width, heads and depth, as in the reference: CHANNELS / HEADS of the YAML are not read for it."""
    from vittracker_amd.model_vitb import build_ostrack
    cfg = _cfg("vitl_256")
    cfg.MODEL.BACKBONE.CHANNELS, cfg.MODEL.BACKBONE.HEADS = 768, 12          # not read for this TYPE
    net = build_ostrack(cfg, training=False)
    sd = net.state_dict()
    assert tuple(sd["backbone.blocks.23.mlp.fc2.weight"].shape) == (1024, 4096)
    assert tuple(sd["box_head.conv1_ctr.0.weight"].shape) == (256, 1024, 3, 3)
    assert tuple(sd["backbone.pos_embed_z"].shape) == (1, 64, 1024) and "backbone.blocks.24.norm1.weight" not in sd
    assert (net.geom["channels"], net.geom["heads"], net.depth) == (1024, 16, 24) and net.feat_sz_s == 16
    # load_state_dict(strict=False) as for ViT-Base: a partial dict is taken, the rest reported missing; a wrong shape is refused
    one = {"backbone.norm.bias": np.full(1024, 0.5, np.float32)}
    inc = net.load_state_dict(one, strict=False)
    assert "backbone.norm.weight" in inc.missing_keys and not inc.unexpected_keys
    assert float(net.state_dict()["backbone.norm.bias"][3]) == 0.5
    with pytest.raises(RuntimeError):
        net.load_state_dict({"backbone.norm.bias": np.zeros(768, np.float32)}, strict=False)
    del net, sd
    net3 = build_ostrack(_cfg("vitl_384"), training=False)
    assert tuple(net3._state["backbone.pos_embed_z"].shape) == (1, 144, 1024) and net3.box_head.feat_sz == 24 and net3.feat_sz_s == 24
    del net3
    ce = _cfg("vitl_256")
    ce.MODEL.BACKBONE.TYPE = "vit_large_patch16_224_ce"
    with pytest.raises(NotImplementedError):
        build_ostrack(ce, training=False)


@pytest.mark.parametrize("name,sizes", [("vitl_256", (256, 4.0, 128, 2.0)), ("vitl_384", (384, 5.0, 192, 2.0))])
def test_parameters_and_factory_on_the_vitl_yamls(name, sizes):
    from vittracker_amd import factory
    from vittracker_amd.model_vitb import build_ostrack
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters(name)
    assert (p.search_size, p.search_factor, p.template_size, p.template_factor) == sizes
    assert p.checkpoint.endswith(f"checkpoints/train/ostrack/{name}/OSTrack_ep0300.pth.tar")
    assert str(p.cfg.MODEL.BACKBONE.TYPE) == "vit_large_patch16_224" and int(p.cfg.MODEL.HEAD.NUM_CHANNELS) == 256
    assert factory.network_builder(_cfg(name)) is build_ostrack
    ce = _cfg(name)
    ce.MODEL.BACKBONE.TYPE = "vit_large_patch16_224_ce"
    assert factory.network_builder(ce) is build_ostrack          # the ViT path, which ends in NotImplementedError for the CE backbone
    with pytest.raises(NotImplementedError):
        factory.build_network(ce)


def test_mac_ratio_to_vit_base():
    """What DESIGN's timing subsection sets the measured time ratio against: 3.37 x the multiply-accumulates of ViT-Base per frame at
    128 / 256 (24 x 1024^2 against 12 x 768^2 = 3.56 x in the blocks' projections, 2.67 x in their attention products, 1.3 x in patch
    embedding and head), 8.03 x at 192 / 384."""
    from oracle import vitb_oracle_torch as ob
    large, base = ob.macs_per_frame(128, 256, C=1024, depth=24), ob.macs_per_frame(128, 256)
    assert abs(sum(large.values()) / sum(base.values()) - 3.37) < 0.02
    large3 = ob.macs_per_frame(192, 384, C=1024, depth=24)
    assert abs(sum(large3.values()) / sum(base.values()) - 8.03) < 0.03
