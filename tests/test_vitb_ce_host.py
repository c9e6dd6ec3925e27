"""CPU: the host side of candidate elimination on the ViT-Base path (the device half: tests/test_gpu_vitb_ce.py).

  * tests/vitb_ce_oracle.py, unforced, reproduces every fixture tests/golden/ref_vbce_*.npz (outputs of the reference's own
    vit_base_patch16_224_ce model): keep sets exactly, maps and boxes within 5e-5; forced to the fixture's sets it gives the same.
  * keep counts (180 / 126 / 89 and 404 / 283 / 199), template rows per CE_TEMPLATE_RANGE and map side, the two YAMLs and parameters();
  * every refusal that stays: a _ce TYPE without CE_LOC, ViT-Large CE, GT_BOX, unequal lengths, and the argument errors of
    vt_set_candidate_elimination that need no model (the library validates n, loc and keep_ratio before it looks at the model, so they are
    reachable without a GPU, as vt_create's are);
  * the inputs of the device's selection test keep at most ce_budget.BAND_CAP of a frame's candidates inside the band, with the fp64
    truth and the bf16 oracle alone."""
import ctypes
import os

import numpy as np
import pytest

import ce_budget as cb
import vbce_cases as vc
from conftest import REPO


def _cfg(name):
    from vittracker_amd import config
    c = config.fresh_cfg()
    config.update_config_from_file(os.path.join(REPO, f"experiments/ostrack/{name}.yaml"), c)
    return c


def test_the_four_fixtures_are_there():
    names = sorted(vc.ids(p).split("_")[2] for p in vc.files())
    assert names == ["256", "384", "d3", "d5"]
    for p in vc.files():
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("path", vc.files(), ids=vc.ids)
def test_oracle_reproduces_the_reference_fixture(path):
    c = vc.load(path)
    g = c["g"]
    o = vc.oracle_run(c)
    assert len(o["keep"]) == c["n"]
    for k in range(c["n"]):
        assert np.array_equal(o["keep"][k].numpy(), g[f"keep{k}"]), f"stage {k}: keep set"
        assert np.array_equal(o["removed"][k].numpy(), g[f"removed{k}"]), f"stage {k}: removed set"
        np.testing.assert_allclose(o["scores"][k].numpy(), g[f"scores{k}"], atol=2e-8, rtol=1e-4, equal_nan=True)
    for key in ("score_map", "size_map", "offset_map", "pred_boxes"):
        np.testing.assert_allclose(o[key].numpy(), g[key], atol=5e-5, rtol=0, err_msg=key)
    np.testing.assert_allclose(o["feat"].numpy()[:, :, ::8], g["feat"], atol=5e-5, rtol=0)
    # removed tokens come back as zeros, kept ones do not
    last = np.zeros((c["B"], c["lx"]), bool)
    np.put_along_axis(last, g[f"keep{c['n'] - 1}"], True, axis=1)
    feat = o["feat"].numpy()
    assert (feat[~last] == 0).all() and (np.abs(feat[last]).max(-1) > 0).all()
    # forced to the fixture's own sets: the same function
    f = vc.oracle_run(c, forced=[g[f"keep{k}"] for k in range(c["n"])])
    for key in ("score_map", "size_map", "offset_map", "pred_boxes"):
        assert np.array_equal(f[key].numpy(), o[key].numpy()), key


def test_keep_counts():
    from vittracker_amd import native
    import vitb_ce_oracle as vo
    assert native.ce_keep_counts(256, [0.7] * 3) == [180, 126, 89] == vo.keep_counts(256, [0.7] * 3)
    assert native.ce_keep_counts(576, [0.7] * 3) == [404, 283, 199] == vo.keep_counts(576, [0.7] * 3)
    assert native.ce_keep_counts(256, [1.0, 0.5, 1.0]) == [256, 128, 128]
    with pytest.raises(native.VtError):
        native.ce_keep_counts(256, [0.0])
    for p in vc.files():
        c = vc.load(p)
        assert [c["g"][f"keep{k}"].shape[1] for k in range(c["n"])] == native.ce_keep_counts(c["lx"], c["ratio"])


def test_template_rows_per_range_and_map_side():
    from vittracker_amd.model_vitb import ce_template_rows
    import vitb_ce_oracle as vo
    want = {("CTR_POINT", 8): [27], ("CTR_POINT", 12): [65], ("CTR_REC", 8): [27, 28, 35, 36], ("CTR_REC", 12): [65, 66, 77, 78]}
    for (tr, side), rows in want.items():
        got = ce_template_rows(tr, side)
        assert len(got) == side * side and [i for i, v in enumerate(got) if v] == rows
        assert np.flatnonzero(vo.template_rows(tr, side).numpy()).tolist() == rows
    assert ce_template_rows("ALL", 8) is None and ce_template_rows("ALL", 12) is None
    with pytest.raises(NotImplementedError, match="GT_BOX"):
        ce_template_rows("GT_BOX", 8)
    with pytest.raises(NotImplementedError):
        ce_template_rows("CTR_POINT", 9)


@pytest.mark.parametrize("name,sizes,lz", [("vitb_256_mae_ce_32x4_ep300", (256, 4.0, 128, 2.0), 64), ("vitb_384_mae_ce_32x4_ep300", (384, 5.0, 192, 2.0), 144)])
def test_ce_yamls_parameters_and_config_surface(name, sizes, lz):
    from vittracker_amd import factory
    from vittracker_amd.model_vitb import build_ostrack
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters(name)
    assert (p.search_size, p.search_factor, p.template_size, p.template_factor) == sizes
    assert p.checkpoint.endswith(f"checkpoints/train/ostrack/{name}/OSTrack_ep0300.pth.tar")
    bbc = p.cfg.MODEL.BACKBONE
    assert str(bbc.TYPE) == "vit_base_patch16_224_ce" and list(bbc.CE_LOC) == [3, 6, 9] and list(bbc.CE_KEEP_RATIO) == [0.7, 0.7, 0.7]
    assert str(bbc.CE_TEMPLATE_RANGE) == "CTR_POINT"
    c = _cfg(name)
    assert factory.network_builder(c) is build_ostrack
    net = factory.build_network(c)
    assert net.ce_loc == [3, 6, 9] and net.ce_keep_ratio == [0.7, 0.7, 0.7] and net.depth == 12
    assert [i for i, v in enumerate(net.ce_rows) if v] == ([27] if lz == 64 else [65]) and len(net.ce_rows) == lz
    assert net.state_dict()["backbone.pos_embed_z"].shape == (1, lz, 768)
    with pytest.raises(NotImplementedError, match="ce_keep_rate"):
        net.forward(None, np.zeros((1, 3, 8, 8)), ce_keep_rate=0.5)


def test_refusals_that_stay():
    from vittracker_amd import factory
    from vittracker_amd.model_vitb import build_ostrack
    c = _cfg("vitb_256")
    c.MODEL.BACKBONE.TYPE = "vit_base_patch16_224_ce"                 # no CE_LOC: says what to give
    with pytest.raises(NotImplementedError, match="CE_LOC"):
        build_ostrack(c, training=False)
    c.MODEL.BACKBONE.CE_LOC, c.MODEL.BACKBONE.CE_KEEP_RATIO = [3], []
    with pytest.raises(NotImplementedError, match="vit_base_patch16_224"):
        build_ostrack(c, training=False)
    c.MODEL.BACKBONE.CE_LOC, c.MODEL.BACKBONE.CE_KEEP_RATIO = [3, 6], [0.7]
    with pytest.raises(ValueError, match="same length"):
        build_ostrack(c, training=False)
    c.MODEL.BACKBONE.CE_LOC, c.MODEL.BACKBONE.CE_KEEP_RATIO, c.MODEL.BACKBONE.CE_TEMPLATE_RANGE = [3], [0.7], "GT_BOX"
    with pytest.raises(NotImplementedError, match="GT_BOX"):
        build_ostrack(c, training=False)
    large = _cfg("vitl_256")
    large.MODEL.BACKBONE.TYPE = "vit_large_patch16_224_ce"
    large.MODEL.BACKBONE.CE_LOC, large.MODEL.BACKBONE.CE_KEEP_RATIO = [3], [0.7]
    assert factory.network_builder(large) is build_ostrack
    with pytest.raises(NotImplementedError):
        factory.build_network(large)
    plain = build_ostrack(_cfg("vitb_256"), training=False)
    with pytest.raises(NotImplementedError):
        plain.forward(None, None, ce_template_mask=np.zeros(1))
    with pytest.raises(NotImplementedError):
        plain.forward(None, None, ce_keep_rate=0.7)


def test_vt_create_still_names_both_geometries():
    from vittracker_amd import native
    L = native.lib()
    h = ctypes.c_void_p()
    for tz, tx, heads in ((160, 320, 12), (192, 256, 12), (128, 256, 8)):
        cfg = native.VtConfig(tz, tx, 768, heads, 12, 256, 16, 1)
        assert L.vt_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
        msg = L.vt_last_error()
        assert b"unsupported ViT-Base" in msg and b"template 128 / search 256" in msg and b"template 192 / search 384" in msg


def test_set_candidate_elimination_argument_errors_without_a_model():
    """n, loc and keep_ratio are checked before the model is looked at, so a bad stage list is refused (VT_ERR_ARG, with its reason) on a
    machine without a GPU; a good one then reaches the null-model check."""
    from vittracker_amd import native
    L = native.lib()

    def call(loc, ratio, n=None):
        n = len(loc) if n is None else n
        rc = L.vt_set_candidate_elimination(None, n, (ctypes.c_int32 * max(len(loc), 1))(*loc), (ctypes.c_double * max(len(ratio), 1))(*ratio), None)
        return rc, L.vt_last_error()
    for loc, ratio, n, what in (([], [], 0, b"n >= 1"), ([3, 3], [0.7, 0.7], None, b"strictly increasing"), ([6, 3], [0.7, 0.7], None, b"strictly increasing"),
                                ([-1], [0.7], None, b"strictly increasing"), ([3], [0.0], None, b"(0, 1]"), ([3], [1.5], None, b"(0, 1]"),
                                ([3], [float("nan")], None, b"(0, 1]")):
        rc, msg = call(loc, ratio, n)
        assert rc == -1 and what in msg, (loc, ratio, msg)
    rc, msg = call([3, 6, 9], [0.7, 0.7, 0.7])
    assert rc == -1 and b"null model" in msg
    assert L.vt_ce_result(None, 1, None, None, None) == -1 and b"null model" in L.vt_last_error()
    assert L.vt_set_candidate_elimination(None, 1, None, None, None) == -1 and b"null" in L.vt_last_error()


@pytest.mark.parametrize("L", [320, 720])
@pytest.mark.parametrize("name", cb.SCORE_REGIMES)
def test_selection_inputs_keep_the_band_small(name, L):
    """A condition on the INPUTS of test_gpu_vitb_ce.py::test_score_and_selection, with the truth and the oracle alone: the band
    2 x 1.65 x E_o either side of the cut holds at most BAND_CAP of each frame's candidates in every case of ce_budget.BAND_CASES, the
    cases the selection is held on (else that test would bind nothing).  Prints the shares of all cases."""
    r = cb.score_refs(name, L)
    for tr in cb.RANGES:
        keep, drop, share = cb.band(r[tr]["truth"], r["count"], r[tr]["e_o"])
        print(f"{name} {L} {tr}: E_o {r[tr]['e_o']:.3e}, score median {np.median(r[tr]['truth']):.3e}, band share per frame {np.round(share, 3)}")
        if (name, L, tr) in cb.BAND_CASES:
            assert max(share) <= cb.BAND_CAP, (name, L, tr, share)
        assert (keep.sum(1) <= r["count"]).all() and (drop.sum(1) <= L - r["lz"] - r["count"]).all()
