"""CPU: the fp32-equivalent mode of the patch-16 ViT path (vt_set_precision) -- its arithmetic emulated in numpy, the bound the GPU tests
hold it to, and its interface where no device is needed.

  * split3 is exact on normal fp32 values whose pieces are normal too (|x| >= 2^-100; below 2^128 (1 - 2^-9), where bf16(x) is finite), the regimes' extremes of tests/bf16_budget.py included;
  * the emulated expanded product (six terms, fp32 accumulator over 32-deep partial sums) lies within the fp32 accumulator's own rounding
    of the float64 product at K = 192, 768, 3072 on the "plain", "common_mode" and "peaked" rows; the single-piece bf16 product does not;
  * 8 x E_ref is below the fp32 caps and E_ref is above zero for ref_vitb_s26_b2 (a property of the fixture and the CPU oracle alone);
  * set_precision's argument checks, the precedence of precision= / params.precision / VB_PRECISION, the two refusals with candidate
    elimination at model level, tracking/test.py --precision."""
import importlib.util
import os
import re

import numpy as np
import pytest

import bf16_budget as bb
import vit_fp32_cases as vc
from conftest import REPO
from vit_small_cases import cfg_of


def _rows(name, C, n=64):
    """n token rows of a regime at width C, through norm1 (what a GEMM of the mode reads)."""
    sd, X = bb.regime(name, 320, w=bb.WIDTHS[C], B=1)
    x = X[0, :n].astype(np.float64)
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    g, b = sd["backbone.blocks.0.norm1.weight"].astype(np.float64), sd["backbone.blocks.0.norm1.bias"].astype(np.float64)
    return sd, ((x - mu) / np.sqrt(var + bb.LN_EPS) * g + b).astype(np.float32)


def test_split3_is_exact():
    rs = np.random.RandomState(0)
    vals = [rs.standard_normal(20000).astype(np.float32) * s for s in (1e-20, 1e-3, 1.0, 1e3, 1e20)]
    for C, amps in bb.AMPS.items():
        vals.append(np.array([v for v in amps.values()] + [-v for v in amps.values()], np.float32) * np.float32(1.0 + 2.0 ** -23))
    vals.append(np.array([1.0, -1.0, 255.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 3.0e38, 0.0], np.float32))
    x = np.concatenate(vals)
    h, m, l = vc.split3(x)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    for p in (h, m, l):      # every piece is a bf16 value
        assert np.array_equal(vc._bf16(p), p)
    b = np.arange(256, dtype=np.float32)      # a byte is exact in ONE piece: the uint8 form needs three terms
    assert np.array_equal(vc._bf16(b), b)


@pytest.mark.parametrize("regime", ("plain", "common_mode", "peaked"))
@pytest.mark.parametrize("K", (192, 768, 3072))
def test_emulated_product_is_fp32_accurate_and_single_piece_bf16_is_not(K, regime):
    """The bound: an fp32 accumulator that takes n = 6 K / 32 partial sums rounds n times, each by at most 2^-24 of the running sum, whose
    size is at most S = sum_k |x_k w_k|; random roundings add as sqrt(n).  4 sqrt(n) 2^-24 S is a few ulps of the sums' own scale.  (K = 3072:
    fc2's depth; its rows are the regime's rows tiled four times, which is as good as any hidden row for a rounding argument.)"""
    C = min(K, 768)
    sd, x = _rows(regime, C)
    x = np.tile(x, (1, K // C))
    w = np.tile(sd["backbone.blocks.0.attn.qkv.weight"][5].astype(np.float32), K // C)
    exact = x.astype(np.float64) @ w.astype(np.float64)
    S = np.abs(x.astype(np.float64) * w.astype(np.float64)).sum(-1)
    tol = 4.0 * np.sqrt(6 * K / 32) * 2.0 ** -24 * S
    emu = vc.emulated_product(x, w).astype(np.float64)
    assert np.all(np.abs(emu - exact) <= tol), float((np.abs(emu - exact) / tol).max())
    one = vc.mfma_dot(vc._bf16(x), vc._bf16(w)).astype(np.float64)
    assert np.abs(one - exact).max() > 20 * tol.max(), "the single-piece bf16 product is inside the fp32 band: the test cannot tell the modes apart"
    # the layouts: six k-ranges, xh in the second range against wl, wh in the third against xl
    xe, we = vc.expand_x(x), vc.expand_w(w)
    assert xe.shape[-1] == 6 * K and np.array_equal(xe[:, K:2 * K], vc.split3(x)[0]) and np.array_equal(we[2 * K:3 * K], vc.split3(w)[0])


def test_bound_of_ref_vitb_s26_b2_is_a_bound_below_the_caps():
    e = vc.e_ref("ref_vitb_s26_b2")
    print({k: "%.3e" % v for k, v in e.items()})
    for k, v in e.items():
        assert v > 0.0, k
        assert vc.FACTOR * v < vc.CAPS[k], (k, v)
    # the float64 decode agrees with the oracle's own boxes
    t = vc.truth("ref_vitb_s26_b2")
    g = vc.load("ref_vitb_s26_b2")[0]
    assert np.abs(t["pred_boxes"] - g["pred_boxes"][:, 0]).max() < 1e-5 and np.abs(t["hann_boxes"] - g["hann_boxes"]).max() < 1e-5


def test_fixture_listing_covers_four_widths_and_both_geometries():
    seen = {(s[1][0], s[2]) for s in vc.PLAIN.values()}
    assert seen == {(c, g) for c in (1024, 768, 384, 192) for g in ("256", "384")}
    for name in list(vc.PLAIN) + list(vc.U8):
        assert os.path.exists(os.path.join(REPO, "tests", "golden", name + ".npz")), name


# ---------------------------------------------------------------------------------------------- interface
def test_header_declares_and_native_binds_the_two_symbols():
    from vittracker_amd import native
    hdr = open(os.path.join(REPO, "include", "vittrack.h")).read()
    assert re.search(r"^int vt_set_precision\(vt_model\* m, int32_t precision\);", hdr, re.M)
    assert re.search(r"^int vt_precision\(const vt_model\* m\);", hdr, re.M)
    assert re.search(r"^#define VT_PRECISION_BF16 0$", hdr, re.M) and re.search(r"^#define VT_PRECISION_FP32 1$", hdr, re.M)
    assert "vt_set_precision" in native.SYMBOLS and "vt_precision" in native.SYMBOLS
    assert native.VIT_PRECISIONS == {"bf16": 0, "fp32": 1}
    for which in ("f32", "f16"):
        L = native.lib(which)
        assert L.vt_set_precision(None, 1) == -1 and b"null model" in L.vt_last_error()
        assert L.vt_precision(None) == -1 and b"null model" in L.vt_last_error()


def test_precision_names_and_their_precedence(monkeypatch):
    from vittracker_amd import factory, native
    from vittracker_amd.model_vitb import OSTrack, build_ostrack, build_small_ostrack
    from vittracker_amd.parameter import ostrack as P
    monkeypatch.delenv("VB_PRECISION", raising=False)
    assert native.vit_precision_name() == "bf16" and native.vit_precision_name("fp32") == "fp32"
    for bad in ("f32", "fp16", "", 1):
        with pytest.raises(native.VtError, match="ViT precision"):
            native.vit_precision_name(bad)
    c = cfg_of("vitb_256")
    assert build_ostrack(c).precision == "bf16" and build_ostrack(c, precision="fp32").precision == "fp32"
    assert OSTrack(c, depth=2, precision="fp32").precision == "fp32" and factory.build_network(c, precision="fp32").precision == "fp32"
    monkeypatch.setenv("VB_PRECISION", "fp32")
    assert build_ostrack(c).precision == "fp32" and build_ostrack(c, precision="bf16").precision == "bf16"
    monkeypatch.setenv("VB_PRECISION", "")
    assert build_ostrack(c).precision == "bf16"
    monkeypatch.setenv("VB_PRECISION", "double")
    with pytest.raises(native.VtError, match="ViT precision"):
        build_ostrack(c)
    monkeypatch.delenv("VB_PRECISION")
    assert P.parameters("vitb_256").precision is None
    from vit_small_cases import small_cfg
    assert build_small_ostrack(small_cfg("vitt", "384"), precision="fp32").precision == "fp32"
    with pytest.raises(native.VtError, match="ViT precision"):
        build_ostrack(c, precision="f16")
    from vittracker_amd.config import fresh_cfg, update_config_from_file
    v48 = fresh_cfg()
    update_config_from_file(os.path.join(REPO, "experiments", "vit_dist", "vit_48_h32_noKD.yaml"), v48)
    with pytest.raises(ValueError, match="vit_48 family"):
        factory.build_network(v48, precision="fp32")


def test_fp32_mode_and_candidate_elimination_exclude_each_other_at_model_level(monkeypatch):
    from vittracker_amd.model_vitb import build_ostrack
    monkeypatch.delenv("VB_PRECISION", raising=False)
    ce = cfg_of("vitb_256_mae_ce_32x4_ep300")
    assert build_ostrack(ce).precision == "bf16"
    with pytest.raises(NotImplementedError, match="(?s)fp32.*candidate elimination"):
        build_ostrack(ce, precision="fp32")
    monkeypatch.setenv("VB_PRECISION", "fp32")
    with pytest.raises(NotImplementedError, match="(?s)fp32.*candidate elimination"):
        build_ostrack(ce)


def _cli():
    spec = importlib.util.spec_from_file_location("tracking_test_cli_fp32", os.path.join(REPO, "tracking", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_cli_takes_the_precision(monkeypatch, tmp_path):
    cli = _cli()
    seen = {}
    monkeypatch.setattr(cli, "run_tracker", lambda *a, **kw: seen.update(args=a, kw=kw))
    for argv, want in ((["--precision", "fp32"], {"precision": "fp32"}), (["--precision", "bf16"], {"precision": "bf16"}), ([], {})):
        monkeypatch.setattr("sys.argv", ["test.py", "ostrack", "vitb_256"] + argv)
        cli.main()
        assert seen["args"][:2] == ("ostrack", "vitb_256") and seen["kw"] == want, seen
    monkeypatch.setattr("sys.argv", ["test.py", "ostrack", "vitb_256", "--precision", "fp64"])
    with pytest.raises(SystemExit):
        cli.main()
    cli = _cli()
    import vittracker_amd.evaluation.running as running
    got = {}
    monkeypatch.setattr(running, "run_dataset_batched", lambda dataset, tracker, **kw: got.update(params=tracker.get_parameters()))
    monkeypatch.setenv("VITTRACK_PRJ_DIR", REPO)
    monkeypatch.setenv("VITTRACK_SAVE_DIR", str(tmp_path))
    cli.run_tracker("ostrack", "vitb_256", dataset_name="synthetic:2x4", batch=2, synthetic_weights=True, precision="fp32")
    assert got["params"].precision == "fp32" and got["params"].allow_synthetic_weights
    cli.run_tracker("ostrack", "vitb_256", dataset_name="synthetic:2x4", batch=2)
    assert got["params"].precision is None
