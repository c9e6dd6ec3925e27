"""CPU side of the ViT-Base OSTrack tracker: the new fixtures against the pinned oracle, the parameter / plugin / factory surface, the
normalisation fold of the uint8 route in emulation (the bound the GPU test uses is shown to discriminate), and the resource gate of
the new kernels."""
import glob
import os
import re
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, REPO

import vitb_u8_fold as vf


def ostrack_u8_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_ostrack_u8_*.npz")))


def load_ostrack_u8(path):
    from vittracker_amd import synth
    g = dict(np.load(path, allow_pickle=False))
    seed, B = int(g["seed"]), int(g["B"])
    sd = synth.synth_vitb_state_dict(seed)
    assert synth.state_checksum(sd) == str(g["state_checksum"]), "synth_vitb_state_dict drifted from the fixture generator"
    z = synth.synth_inputs(seed, B, 128, 256)[0]
    patches = synth.synth_patches(seed, B, 256)
    assert int(patches.astype(np.uint64).sum()) == int(g["patch_checksum"]), "synth_patches drifted from the fixture generator"
    return g, sd, z, patches


def test_fixtures_exist_and_hold_the_margin_rule():
    files = ostrack_u8_files()
    assert files
    for p in files:
        g = np.load(p)
        assert min(g["margin_raw"].min(), g["margin_hann"].min()) > 0.03
        assert g["act_tokens"].shape[0] == 2          # sample 0 (noise) and sample 1 (smooth, black band)
    tr = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_ostrack_track_*.npz")))
    assert tr
    for p in tr:
        g = np.load(p)
        assert g["margin_hann"].shape == (2, 4) and g["margin_hann"].min() > 0.03


@pytest.mark.parametrize("path", ostrack_u8_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_pinned_oracle_reproduces_the_u8_fixture(path):
    """oracle/vitb_oracle_torch.py on the Preprocessor-normalised patch (CPU: a true division by 255, as the generator) against the
    reference's outputs, at the 5e-5 tests/test_oracle_golden.py uses for ViT-Base."""
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import synth
    g, sd, z, patches = load_ostrack_u8(path)
    x = synth.normalise_patches(patches, reciprocal=False)
    acts = {}
    with torch.no_grad():
        out = ob.build_from_state(sd)(torch.from_numpy(z), torch.from_numpy(x), acts)
    for k in ("score_map", "size_map", "offset_map"):
        np.testing.assert_allclose(out[k].numpy(), g[k], atol=5e-5, rtol=0, err_msg=k)
    np.testing.assert_allclose(acts["tokens"][:2, g["act_rows"]].numpy(), g["act_tokens"], atol=5e-5, rtol=0)


def _params(yaml_name="vitb_256"):
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    return P.parameters(yaml_name)


def test_ostrack_parameters():
    p = _params()
    assert (p.template_size, p.search_size, p.template_factor, p.search_factor) == (128, 256, 2.0, 4.0)
    assert p.checkpoint.endswith("checkpoints/train/ostrack/vitb_256/OSTrack_ep0300.pth.tar")
    assert p.save_all_boxes is False and int(p.cfg.MODEL.BACKBONE.CHANNELS) == 768


def test_tracker_finds_the_ostrack_plugin():
    from vittracker_amd.evaluation.tracker import Tracker
    from vittracker_amd.tracker.ostrack import OSTrack, get_tracker_class
    from vittracker_amd.tracker.vit_dist import Vit_dist
    t = Tracker("ostrack", "vitb_256", "synthetic")
    assert t.tracker_class is OSTrack is get_tracker_class() and issubclass(OSTrack, Vit_dist)
    for name in ("initialize", "track", "map_box_back", "map_box_back_batch"):
        assert callable(getattr(OSTrack, name))


def test_factory_picks_the_model_class_of_both_yaml_families():
    from vittracker_amd import factory
    from vittracker_amd.config import fresh_cfg, update_config_from_file
    from vittracker_amd.model import OstrackDist, build_ostrack_dist
    from vittracker_amd.model_vitb import OSTrack, build_ostrack
    want = {"ostrack/vitb_256": (build_ostrack, OSTrack), "vit_dist/vit_48_h32_noKD": (build_ostrack_dist, OstrackDist),
            "vit_dist/vit_48_h32_g128": (build_ostrack_dist, OstrackDist)}
    for y, (fn, cls) in want.items():
        c = fresh_cfg()
        update_config_from_file(os.path.join(REPO, "experiments", y + ".yaml"), c)
        assert factory.network_builder(c) is fn, y
        assert type(factory.build_network(c, max_batch=2)) is cls and factory.build_network(c, max_batch=2).max_batch == 2


def test_the_ostrack_plugin_refuses_a_vit_dist_cfg():
    from vittracker_amd.parameter import vit_dist as P
    from vittracker_amd.tracker.ostrack import OSTrack
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    with pytest.raises(ValueError, match="ViT-Base"):
        OSTrack(P.parameters("vit_48_h32_g128"), "synthetic")


def test_centred_fold_is_inside_the_token_bound_and_the_uncentred_fold_is_not():
    """The fold of vitb.hip fold_patch_u8 in numpy with bf16 emulated by torch, against fp64 tokens, error relative to the centred row
    norm.  Centred bytes with the bias from the unrounded weights: every sample inside 3.2e-3.  Uncentred: a noise sample is over it --
    so the bound the GPU test holds the stem to tells the two apart."""
    from vittracker_amd import synth
    sd = synth.synth_vitb_state_dict(26)
    patches = synth.synth_patches(7, 4, 256)
    truth = vf.tokens_truth(sd, patches)
    cen = [vf.rel_c(vf.tokens_folded(sd, patches[b:b + 1], 128.0), truth[b:b + 1]) for b in range(4)]
    unc = [vf.rel_c(vf.tokens_folded(sd, patches[b:b + 1], 0.0), truth[b:b + 1]) for b in range(4)]
    fp32 = [vf.rel_c(vf.tokens_fp32_route(sd, patches[b:b + 1]), truth[b:b + 1]) for b in range(4)]
    print("centred", cen, "uncentred", unc, "fp32 route", fp32)
    assert max(cen) <= vf.TOL_TOKENS
    assert max(unc[0], unc[2]) > vf.TOL_TOKENS          # even samples: noise
    assert max(fp32) <= vf.TOL_TOKENS


def test_fold_bias_comes_from_the_unrounded_weights():
    """With the ROUNDED weights in the compensation the centred form is algebraically the uncentred one."""
    from vittracker_amd import synth
    sd = synth.synth_vitb_state_dict(26)
    patches = synth.synth_patches(7, 1, 256)
    Wf, b0 = vf.fold(sd["backbone.patch_embed.proj.weight"], sd["backbone.patch_embed.proj.bias"], 0.0)
    Wr = vf.bf16(Wf.astype(np.float32))
    pos = np.asarray(sd["backbone.pos_embed_x"], np.float64)[0]
    rounded_comp = (vf.operand(patches) - 128.0) @ Wr.T + (b0 + 128.0 * Wr.sum(1)) + pos
    uncentred = vf.operand(patches) @ Wr.T + b0 + pos
    np.testing.assert_allclose(rounded_comp, uncentred, atol=1e-9, rtol=0)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH: the resource gate needs the compiler")
def test_new_vitb_kernels_have_no_scratch_and_fit_the_register_cap():
    """vbm::patchify_u8_kernel (256 threads) and the row-mapped patch GEMM: ScratchSize 0, no spill, at most 256 VGPRs + AGPRs."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table as rt
    rows = rt.table("vitb.hip")
    for pat in (r"vbm::patchify_u8_kernel", r"vbg::gemm_kernel<256, 256, 2, 4, 0, 6>"):
        hit = [r for r in rows if re.fullmatch(pat, r["name"])]
        assert len(hit) == 1, (pat, [r["name"] for r in rows])
        r = hit[0]
        assert r["scratch"] == 0 and r["vspill"] == 0, r
        assert r["vgpr"] + r.get("agpr", 0) <= 256, r
    pu8 = [r for r in rows if r["name"] == "vbm::patchify_u8_kernel"][0]
    assert pu8["sspill"] == 0, pu8
