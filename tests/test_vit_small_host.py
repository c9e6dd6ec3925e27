"""Host side of the ViT-Small / ViT-Tiny OSTrack model points (widths 384 / 6 heads and 192 / 3 heads, MLP 4 x width, depth <= 12; 128 / 256
and 192 / 384): vt_create_vit's argument checks (they need no device), vt_create's unchanged choice of family, the four YAMLs, build_ostrack /
build_small_ostrack / the factory, synthetic state dicts, and the pinned torch oracle against the reference's own outputs
(tests/golden/make_golden_vit_small.py).  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from vit_small_cases import ACT_BLOCKS, GEO, MARGIN, PLAIN, TRACK, U8, WIDTHS, cfg_of, load_plain, load_u8, path_of, sd_of, small_cfg

TUPLES = ("(192, 3)", "(384, 6)", "(768, 12)", "(1024, 16)")


def _create_vit(*cfg):
    from vittracker_amd import native
    L = native.lib()
    h = ctypes.c_void_p()
    rc = L.vt_create_vit(ctypes.byref(native.VtConfig(*cfg)), ctypes.byref(h))
    return rc, L.vt_last_error().decode()


# ------------------------------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("cfg,echo", [
    ((128, 256, 384, 12, 12, 256, 16, 1), "channels=384 heads=12"),        # a ViT-Small width with ViT-Base's head count
    ((128, 256, 192, 6, 12, 256, 16, 1), "channels=192 heads=6"),
    ((128, 256, 768, 6, 12, 256, 16, 1), "channels=768 heads=6"),          # no family member: vt_create would call this a ViT-Base error
    ((128, 256, 512, 8, 12, 256, 16, 1), "channels=512 heads=8"),
    ((128, 256, 48, 1, 3, 32, 16, 1), "channels=48 heads=1"),              # the shipped vit_dist model is no patch-16 ViT
    ((128, 256, 384, 6, 13, 256, 16, 1), "depth=13"),                      # depth 13 at width 384
    ((128, 256, 192, 3, 0, 256, 16, 1), "depth=0"),
    ((128, 256, 384, 6, 12, 128, 16, 1), "head_channels=128"),
    ((128, 256, 192, 3, 12, 256, 8, 1), "stride=8"),
    ((112, 224, 384, 6, 12, 256, 16, 1), "template=112 search=224"),
    ((128, 384, 192, 3, 12, 256, 16, 1), "template=128 search=384"),
])
def test_vt_create_vit_rejects_with_the_four_tuples(cfg, echo):
    rc, msg = _create_vit(*cfg)
    assert rc == -1, (rc, msg)          # VT_ERR_ARG
    assert "unsupported ViT configuration" in msg, msg
    for t in TUPLES:
        assert t in msg, (t, msg)
    assert "template 128 / search 256" in msg and "template 192 / search 384" in msg and "HEAD.NUM_CHANNELS=256" in msg, msg
    assert echo in msg, msg


def test_vt_create_vit_is_vt_create_for_the_two_existing_tuples():
    """(768, 12) and (1024, 16) go through vt_create's own checks: the same code and the same message, word for word."""
    from vittracker_amd import native
    L = native.lib()
    h = ctypes.c_void_p()
    for cfg, word in (((100, 200, 768, 12, 12, 256, 16, 1), "unsupported ViT-Base configuration"),
                      ((128, 256, 1024, 16, 25, 256, 16, 1), "unsupported ViT-Large configuration"),
                      ((128, 256, 768, 12, 25, 256, 16, 1), "bad depth / max_batch")):
        c = native.VtConfig(*cfg)
        rc_vit = L.vt_create_vit(ctypes.byref(c), ctypes.byref(h))
        msg_vit = L.vt_last_error()
        rc = L.vt_create(ctypes.byref(c), ctypes.byref(h))
        assert rc_vit == rc == -1 and msg_vit == L.vt_last_error() and word.encode() in msg_vit, (cfg, msg_vit)
    assert L.vt_create_vit(None, ctypes.byref(h)) == -1 and b"null argument" in L.vt_last_error()


def test_vt_create_keeps_384_and_192_on_the_shape_generic_surface():
    """vt_create's choice of family does not change: 384 / 6 / 256 and 192 / 3 / 256 pass every argument check of the shape-generic vit_dist
    surface.  Without a device the call then ends in a HIP error, never in VT_ERR_ARG; what the generic surface refuses, it still refuses in
    its own words (depth 13 > 12), with no word of the ViT family."""
    from vittracker_amd import native
    L = native.lib()
    h = ctypes.c_void_p()
    for C, heads in ((384, 6), (192, 3)):
        c = native.VtConfig(128, 256, C, heads, 3, 256, 16, 1)
        rc = L.vt_create(ctypes.byref(c), ctypes.byref(h))
        assert rc != -1, L.vt_last_error()
        if rc == 0:
            q = [ctypes.c_int32() for _ in range(4)]
            assert L.vt_query(h, *[ctypes.byref(v) for v in q]) == 0 and q[3].value == C
            L.vt_destroy(h)
        else:
            assert b"ViT" not in L.vt_last_error(), L.vt_last_error()
        c = native.VtConfig(128, 256, C, heads, 13, 256, 16, 1)
        assert L.vt_create(ctypes.byref(c), ctypes.byref(h)) == -1
        assert b"bad depth" in L.vt_last_error() and b"ViT" not in L.vt_last_error()


def test_native_model_family_argument():
    from vittracker_amd import native
    with pytest.raises(ValueError, match="family"):
        native.Model(128, 256, 384, 6, 12, 256, family="levit")
    with pytest.raises(native.VtError, match="unsupported ViT configuration") as e:
        native.Model(128, 256, 384, 6, 13, 256, family="vit")
    assert "vt_create_vit" in str(e.value)
    assert "vt_create_vit" in native.SYMBOLS


# ------------------------------------------------------------------------------------------------- YAMLs, builders, factory
YAMLS = {"vits_256": ("vit_small_patch16_224", 384, 6, 256, 4.0, 128, 2.0), "vits_384": ("vit_small_patch16_224", 384, 6, 384, 5.0, 192, 2.0),
         "vitt_256": ("vit_tiny_patch16_224", 192, 3, 256, 4.0, 128, 2.0), "vitt_384": ("vit_tiny_patch16_224", 192, 3, 384, 5.0, 192, 2.0)}


@pytest.mark.parametrize("name", sorted(YAMLS))
def test_yaml_parameters_and_factory(name):
    from vittracker_amd import factory
    from vittracker_amd.config import geometry
    from vittracker_amd.model_vitb import OSTrack, build_ostrack
    from vittracker_amd.parameter import ostrack as P
    bb_type, C, heads, tx, fx, tz, fz = YAMLS[name]
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters(name)
    assert (p.search_size, p.search_factor, p.template_size, p.template_factor) == (tx, fx, tz, fz)
    assert p.checkpoint.endswith(f"checkpoints/train/ostrack/{name}/OSTrack_ep0300.pth.tar")
    cfg = cfg_of(name)
    g = geometry(cfg)
    assert str(cfg.MODEL.BACKBONE.TYPE) == bb_type and (g["channels"], g["heads"], g["head_channels"], g["stride"]) == (C, heads, 256, 16)
    assert (g["search_size"], g["template_size"], g["feat_sz"]) == (tx, tz, tx // 16)
    assert factory.network_builder(cfg) is build_ostrack
    net = factory.build_network(cfg, max_batch=2)
    assert isinstance(net, OSTrack) and net.family == "vit" and net.max_batch == 2
    assert (net.geom["channels"], net.geom["heads"], net.depth, net.feat_sz_s) == (C, heads, 12, tx // 16)


def test_build_ostrack_small_types_fix_width_heads_depth():
    """As for ViT-Large the TYPE decides: CHANNELS / HEADS of the YAML are not read for it."""
    from vittracker_amd.model_vitb import build_ostrack
    for name, C, heads in (("vits_256", 384, 6), ("vitt_384", 192, 3)):
        cfg = cfg_of(name)
        cfg.MODEL.BACKBONE.CHANNELS, cfg.MODEL.BACKBONE.HEADS = 768, 12
        net = build_ostrack(cfg, training=False)
        sd = net.state_dict()
        lz = GEO[name[-3:]]["LZ"]
        assert (net.geom["channels"], net.geom["heads"], net.depth) == (C, heads, 12)
        assert tuple(sd["backbone.blocks.11.mlp.fc2.weight"].shape) == (C, 4 * C) and "backbone.blocks.12.norm1.weight" not in sd
        assert tuple(sd["backbone.blocks.0.attn.qkv.weight"].shape) == (3 * C, C)
        assert tuple(sd["box_head.conv1_ctr.0.weight"].shape) == (256, C, 3, 3) and tuple(sd["backbone.pos_embed_z"].shape) == (1, lz, C)
        with pytest.raises(RuntimeError):
            net.load_state_dict({"backbone.norm.bias": np.zeros(768, np.float32)}, strict=False)
    with pytest.raises(NotImplementedError):
        build_ostrack(cfg_of("vits_256"), training=True)
    bad = cfg_of("vits_256")
    bad.MODEL.BACKBONE.TYPE = "vit_small_patch16_224_ce"
    with pytest.raises(NotImplementedError, match="vit_small_patch16_224 and vit_tiny_patch16_224"):
        build_ostrack(bad, training=False)
    # a vit_dist YAML of 384 channels keeps the default TYPE: still the distilled family
    from vittracker_amd import factory
    from vittracker_amd.model import build_ostrack_dist
    dist = cfg_of("vitb_256")
    dist.MODEL.BACKBONE.CHANNELS, dist.MODEL.BACKBONE.HEADS = 384, 6
    assert factory.network_builder(dist) is build_ostrack_dist


def test_build_small_ostrack_accepts_and_rejects():
    from vittracker_amd.model_vitb import OSTrack, build_small_ostrack
    for model, (C, heads) in list(WIDTHS.items()) + [("vitb", (768, 12))]:
        net = build_small_ostrack(small_cfg((C, heads), "256"), training=False, max_batch=3)
        assert isinstance(net, OSTrack) and net.family == "vit" and net.max_batch == 3
        assert (net.geom["channels"], net.geom["heads"], net.depth, net.ce_loc) == (C, heads, 3, [])
        sd = net.state_dict()
        assert "backbone.blocks.2.norm1.weight" in sd and "backbone.blocks.3.norm1.weight" not in sd
        assert tuple(sd["backbone.blocks.2.mlp.fc1.weight"].shape) == (4 * C, C)
    net = build_small_ostrack(small_cfg("vits", "384"))
    assert net.feat_sz_s == 24 and tuple(net._state["backbone.pos_embed_x"].shape) == (1, 576, 384)
    ce = build_small_ostrack(small_cfg((768, 12), "256", ce_loc=[1]), ce_form="compact")          # width 768: the existing machinery
    assert ce.ce_loc == [1] and ce.ce_keep_ratio == [0.7] and ce.depth == 3 and ce.ce_form == "compact"
    for model in ("vits", "vitt"):
        with pytest.raises(NotImplementedError, match="candidate elimination is implemented for width 768 only"):
            build_small_ostrack(small_cfg(model, "256", ce_loc=[1]))
    for pair in ((384, 12), (512, 8), (1024, 16), (192, 6)):
        with pytest.raises(NotImplementedError) as e:
            build_small_ostrack(small_cfg(pair, "256"))
        for t in ("(192, 3)", "(384, 6)", "(768, 12)"):
            assert t in str(e.value)
    with pytest.raises(NotImplementedError):
        build_small_ostrack(small_cfg("vits", "256"), training=True)
    plain = small_cfg("vits", "256")
    plain.MODEL.BACKBONE.TYPE = "vit_base_patch16_224"
    with pytest.raises(NotImplementedError):
        build_small_ostrack(plain)


@pytest.mark.parametrize("model", sorted(WIDTHS))
def test_synthetic_state_dicts_carry_the_ostrack_keys_at_these_shapes(model):
    from vittracker_amd import synth
    C, heads = WIDTHS[model]
    sd = sd_of(model, "384", 2, 26)
    base = synth.synth_vitb_state_dict(26, depth=2, len_z=144, len_x=576)
    assert set(sd) == set(base)
    want = {"backbone.patch_embed.proj.weight": (C, 3, 16, 16), "backbone.pos_embed_z": (1, 144, C), "backbone.pos_embed_x": (1, 576, C),
            "backbone.blocks.1.attn.qkv.weight": (3 * C, C), "backbone.blocks.1.attn.qkv.bias": (3 * C,), "backbone.blocks.0.attn.proj.weight": (C, C),
            "backbone.blocks.0.mlp.fc1.weight": (4 * C, C), "backbone.blocks.0.mlp.fc2.weight": (C, 4 * C), "backbone.norm.weight": (C,),
            "box_head.conv1_size.0.weight": (256, C, 3, 3), "box_head.conv2_ctr.0.weight": (128, 256, 3, 3), "box_head.conv5_offset.weight": (2, 32, 1, 1)}
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    for k in sd:
        if not k.startswith("backbone."):
            assert sd[k].shape[1:] == base[k].shape[1:] or "conv1_" in k, k


# ------------------------------------------------------------------------------------------------- fixtures
def test_fixture_set_is_what_the_generator_writes():
    for name, (model, geo, depth, seed, rows, acts) in PLAIN.items():
        p = path_of(name)
        assert os.path.getsize(p) < (1 << 20)
        g = dict(np.load(p))
        C = WIDTHS[model][0]
        assert g["rows"].tolist() == rows and min(g["margin_raw"].min(), g["margin_hann"].min()) > MARGIN
        assert ("act_norm" in g) == acts
        if acts:
            for k in ["tokens", "norm"] + [f"block{i}" for i in ACT_BLOCKS[depth]]:
                assert g["act_" + k].shape == (1, len(g["act_rows"]), C), (name, k)
    for name in (U8, TRACK):
        assert os.path.getsize(path_of(name)) < (1 << 20)
    t = dict(np.load(path_of(TRACK)))
    assert t["margin_hann"].shape == (2, 4) and t["margin_hann"].min() > MARGIN


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_torch_oracle_matches_the_reference(name):
    """oracle/vitb_oracle_torch.build_from_state(sd, heads) against the reference's maps, boxes and kept activation rows at the tolerances of
    tests/test_vitl_host.py (5e-5 outputs, 2e-4 activations)."""
    import torch
    from oracle import vitb_oracle_torch as ob
    model, geo, depth, _, _, acts_kept = PLAIN[name]
    g, sd, z, x = load_plain(name)
    m = ob.build_from_state(sd, heads=WIDTHS[model][1])
    assert len(m.backbone.blocks) == depth and m.backbone.norm.weight.shape[0] == WIDTHS[model][0]
    acts = {}
    with torch.no_grad():
        out = m(torch.from_numpy(z), torch.from_numpy(x), acts)
    for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(out[k].numpy(), g[k], atol=5e-5, rtol=0, err_msg=k)
    assert out["score_map"].shape[-2:] == (GEO[geo]["F"], GEO[geo]["F"])
    if acts_kept:
        rows = g["act_rows"]
        for k in ["tokens", "norm"] + [f"block{i}" for i in ACT_BLOCKS[depth]]:
            np.testing.assert_allclose(acts[k][:1, rows].numpy(), g["act_" + k], atol=2e-4, rtol=0, err_msg=k)


def test_torch_oracle_matches_the_uint8_fixture():
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import synth
    g, sd, z, patches = load_u8()
    x = synth.normalise_patches(patches, reciprocal=False)
    acts = {}
    with torch.no_grad():
        out = ob.build_from_state(sd, heads=6)(torch.from_numpy(z), torch.from_numpy(x), acts)
    for k in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(out[k].numpy(), g[k], atol=5e-5, rtol=0, err_msg=k)
    np.testing.assert_allclose(acts["tokens"][:2, g["act_rows"]].numpy(), g["act_tokens"], atol=2e-4, rtol=0)
    assert min(g["margin_raw"].min(), g["margin_hann"].min()) > MARGIN
