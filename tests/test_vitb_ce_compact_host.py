"""CPU: the host side of the compact form of candidate elimination on the ViT-Base path (the device half:
tests/test_gpu_vitb_ce_compact.py).

  * the padded frame lengths per stage (256 / 192 / 160 and 560 / 432 / 352), and the tails the attention test's keep ratios give;
  * the `form` argument: unknown names, the VB_CE_FORM fallback, the model-level pass-through, ViT-Large;
  * vt_set_ce_form: declared in the header, bound in the native table, null model refused;
  * the inputs of the device's stage-2 selection test keep at most ce_budget.BAND_CAP of a frame's candidates inside the band, with the bf16
    oracle's residual stream and stage-1 keep set in the device's place."""
import os
import re

import numpy as np
import pytest

import ce_budget as cb
import ce_compact_cases as cc
from conftest import REPO


def _cfg(name):
    from vittracker_amd import config
    c = config.fresh_cfg()
    config.update_config_from_file(os.path.join(REPO, f"experiments/ostrack/{name}.yaml"), c)
    return c


def test_compact_lengths():
    from vittracker_amd import native
    assert native.ce_compact_lengths(64, 256, [0.7] * 3) == [256, 192, 160]
    assert native.ce_compact_lengths(144, 576, [0.7] * 3) == [560, 432, 352]
    assert native.ce_compact_lengths(64, 256, [1.0, 0.5, 1.0]) == [320, 192, 192]
    for ratio, (live, rows) in cc.ATTN_RATIOS.items():      # the tails of the attention test
        assert 64 + native.ce_keep_counts(256, [ratio])[0] == live and native.ce_compact_lengths(64, 256, [ratio]) == [rows]
    assert native.ce_compact_lengths(144, 576, [0.7]) == [560] and 144 + native.ce_keep_counts(576, [0.7])[0] == 548
    with pytest.raises(native.VtError):
        native.ce_compact_lengths(64, 256, [0.0])


def test_form_names_and_the_environment_fallback(monkeypatch):
    from vittracker_amd import native
    monkeypatch.delenv("VB_CE_FORM", raising=False)
    assert native.ce_form_name() == "masked" and native.ce_form_name("compact") == "compact" and native.ce_form_name("masked") == "masked"
    monkeypatch.setenv("VB_CE_FORM", "compact")
    assert native.ce_form_name() == "compact" and native.ce_form_name("masked") == "masked"
    monkeypatch.setenv("VB_CE_FORM", "")
    assert native.ce_form_name() == "masked"
    for bad in ("dense", "COMPACT", 1):
        with pytest.raises(native.VtError, match="one of"):
            native.ce_form_name(bad)
    monkeypatch.setenv("VB_CE_FORM", "squeezed")
    with pytest.raises(native.VtError, match="squeezed"):
        native.ce_form_name()
    assert native.CE_FORMS == {"masked": 0, "compact": 1} and native.Model.ce_form == "masked"


def test_model_level_pass_through(monkeypatch):
    from vittracker_amd import factory, native
    from vittracker_amd.model_vitb import build_ostrack
    from vittracker_amd.parameter import ostrack as P
    monkeypatch.delenv("VB_CE_FORM", raising=False)
    c = _cfg("vitb_256_mae_ce_32x4_ep300")
    assert build_ostrack(c).ce_form == "masked" and build_ostrack(c, ce_form="compact").ce_form == "compact"
    assert factory.build_network(c, ce_form="compact").ce_form == "compact"
    monkeypatch.setenv("VB_CE_FORM", "compact")
    assert build_ostrack(c).ce_form == "compact" and build_ostrack(c, ce_form="masked").ce_form == "masked"
    with pytest.raises(native.VtError, match="one of"):
        build_ostrack(c, ce_form="packed")
    monkeypatch.setenv("VITTRACK_PRJ_DIR", REPO)
    assert P.parameters("vitb_256_mae_ce_32x4_ep300").ce_form is None
    with pytest.raises(ValueError, match="vit_48"):
        factory.build_network(_cfg_vit48(), ce_form="compact")
    large = _cfg("vitl_256")      # ViT-Large CE stays refused, whatever the form
    large.MODEL.BACKBONE.TYPE = "vit_large_patch16_224_ce"
    large.MODEL.BACKBONE.CE_LOC, large.MODEL.BACKBONE.CE_KEEP_RATIO = [3], [0.7]
    with pytest.raises(NotImplementedError):
        factory.build_network(large, ce_form="compact")


def _cfg_vit48():
    from vittracker_amd import config
    c = config.fresh_cfg()
    config.update_config_from_file(os.path.join(REPO, "experiments/vit_dist/vit_48_h32_noKD.yaml"), c)
    return c


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tracking_test_cli", os.path.join(REPO, "tracking", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_cli_takes_the_form(monkeypatch, tmp_path):
    """tracking/test.py --ce_form: parsed, handed to run_tracker, refused when it is neither form; run_tracker puts it on the parameters
    every front end builds its network from (BatchedVitTracker, the sharded tracker's shards, the plugin)."""
    cli = _cli()
    seen = {}
    monkeypatch.setattr(cli, "run_tracker", lambda *a: seen.update(args=a))
    for argv, want in ((["--ce_form", "compact"], "compact"), (["--ce_form", "masked"], "masked"), ([], None)):
        monkeypatch.setattr("sys.argv", ["test.py", "ostrack", "vitb_256_mae_ce_32x4_ep300"] + argv)
        cli.main()
        assert seen["args"][:2] == ("ostrack", "vitb_256_mae_ce_32x4_ep300") and seen["args"][-1] == want, seen
    monkeypatch.setattr("sys.argv", ["test.py", "ostrack", "vitb_256_mae_ce_32x4_ep300", "--ce_form", "dense"])
    with pytest.raises(SystemExit):
        cli.main()
    # run_tracker: the form lands on the tracker's parameters (the dataset run itself is replaced)
    cli = _cli()
    import vittracker_amd.evaluation.running as running
    got = {}
    monkeypatch.setattr(running, "run_dataset_batched", lambda dataset, tracker, **kw: got.update(params=tracker.get_parameters(), kw=kw))
    monkeypatch.setenv("VITTRACK_PRJ_DIR", REPO)
    monkeypatch.setenv("VITTRACK_SAVE_DIR", str(tmp_path))
    cli.run_tracker("ostrack", "vitb_256_mae_ce_32x4_ep300", dataset_name="synthetic:2x4", batch=2, shards=2, synthetic_weights=True, ce_form="compact")
    assert got["params"].ce_form == "compact" and got["params"].allow_synthetic_weights and got["kw"]["shards"] == 2
    cli.run_tracker("ostrack", "vitb_256_mae_ce_32x4_ep300", dataset_name="synthetic:2x4", batch=2)
    assert got["params"].ce_form is None


def test_header_declares_and_native_binds_vt_set_ce_form():
    from vittracker_amd import native
    hdr = open(os.path.join(REPO, "include", "vittrack.h")).read()
    assert re.search(r"^int vt_set_ce_form\(vt_model\* m, int32_t form\);", hdr, re.M)
    assert re.search(r"^#define VT_CE_MASKED 0$", hdr, re.M) and re.search(r"^#define VT_CE_COMPACT 1$", hdr, re.M)
    L = native.lib()
    assert L.vt_set_ce_form.argtypes is not None and len(L.vt_set_ce_form.argtypes) == 2
    assert L.vt_set_ce_form(None, 1) == -1 and b"null model" in L.vt_last_error()


@pytest.mark.parametrize("L", [320, 720])
def test_stage2_inputs_keep_the_band_small(L):
    """A condition on the INPUTS of test_gpu_vitb_ce_compact.py::test_stage2_on_compacted_rows: with the bf16 oracle's residual after block 0
    and its stage-1 keep set in the device's place, the band 2 x 1.65 x E_o either side of stage 2's cut holds at most BAND_CAP of each
    frame's candidates at every template range."""
    for tr in cb.RANGES:
        r = cc.stage2_cpu(L, tr)
        print(f"stage 2 {L} {tr} seed {cc.STAGE2_SEEDS[L]}: E_o {r['e_o']:.3e}, band share per frame {np.round(r['share'], 3)}")
        assert r["keep1"].shape == (2, r["count1"]) and (np.isnan(r["truth"]).sum(1) == L - cb.bb.GEOS[L][0] - r["count1"]).all()
        assert max(r["share"]) <= cb.BAND_CAP, (L, tr, r["share"])
        assert (r["must_keep"].sum(1) <= r["count2"]).all() and (r["must_drop"].sum(1) <= r["count1"] - r["count2"]).all()
