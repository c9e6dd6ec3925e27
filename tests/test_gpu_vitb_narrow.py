"""GPU: the narrow 128 x 64 tile of the ViT-Base / ViT-Large GEMMs (vb_gemm.h: a ring of four k-tile stages; vitb.hip narrow_pick) against
the 256 x 256 tile.  Every output element keeps its whole sum in one workgroup, in the same order, through the same epilogue arithmetic:
the two forms give the same BITS, which is what lets the form be chosen per launch from the launch's shape alone.

  1  bit identity     a VB_GEMM_NARROW=0 and a VB_GEMM_NARROW=1 model on the same weights (the switch is read at model creation): stem
                      tokens, blocks (residual stream and final norm), forward, forward_u8, two tracking steps, ce_result -- torch.equal on
                      the raw bits, outputs filled with NaN first.  Shapes: ViT-Base 128 / 256 depth 2 at B = 1 (M = 320: a partial last
                      tile row), 2 (640: whole 128-row tiles) and 5 (1600); ViT-Base 192 / 384 depth 1 at B = 3 (2160 rows, the row-count
                      patch epilogue, the qk GEMM of the streaming route); ViT-Large depth 1 at B = 1 (N = 1024, K = 4096); a depth-3
                      compacted candidate-elimination model at B = 2 (512 then 384 rows).
  2  the form ran     vt_gemm_form: every bit of a kind the model launches under =1, none under =0; the automatic choice is narrow at
                      B = 1 and wide at B = 256.
  3  reference        the ref_vitb_* and one ref_vb384_* fixture through a =1 model at the tolerances of the wide-tile tests (imported).
  4  plumbing, =1     eager == captured == second replay; a slot of a three-sequence BatchedVitTracker == the one-sequence plugin; two
                      consecutive eager runs are equal (the ring's counted waits leave no race that shows)."""
import os

import numpy as np
import pytest

from conftest import REPO, load_vitb_case, vitb_golden_files
from test_gpu_vitb import TOL_BOX, TOL_MAP
from test_vitb384_host import load_vb384, vb384_files
from vitb_u8_fold import MEAN, STD

pytestmark = pytest.mark.gpu

KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
H, W = 120, 160
# name -> geometry, width, heads, depth, max_batch, candidate elimination (loc, keep ratios; compact form)
KINDS = {
    "base256": dict(tz=128, tx=256, C=768, heads=12, depth=2, maxB=5, ce=None),
    "base384": dict(tz=192, tx=384, C=768, heads=12, depth=1, maxB=3, ce=None),
    "large256": dict(tz=128, tx=256, C=1024, heads=16, depth=1, maxB=1, ce=None),
    "ce256": dict(tz=128, tx=256, C=768, heads=12, depth=3, maxB=2, ce=([0, 1], [0.7, 0.7])),      # frames of 256 then 192 rows
}
CASES = [("base256", 1), ("base256", 2), ("base256", 5), ("base384", 3), ("large256", 1), ("ce256", 2)]
_SD, _MODELS = {}, {}


def _sd(kind):
    from vittracker_amd import synth
    k = KINDS[kind]
    if kind not in _SD:
        _SD[kind] = synth.synth_vitb_state_dict(26, C=k["C"], depth=k["depth"], heads=k["heads"], len_z=(k["tz"] // 16) ** 2, len_x=(k["tx"] // 16) ** 2)
    return _SD[kind]


def _build(kind, narrow, sd=None, maxB=None, depth=None):
    """A model created under VB_GEMM_NARROW=<narrow> (None: unset, the automatic choice)."""
    from vittracker_amd import native
    k = KINDS[kind]
    old = os.environ.pop("VB_GEMM_NARROW", None)
    if narrow is not None:
        os.environ["VB_GEMM_NARROW"] = str(narrow)
    try:
        m = native.Model(k["tz"], k["tx"], channels=k["C"], heads=k["heads"], depth=depth or k["depth"], head_channels=256, max_batch=maxB or k["maxB"])
    finally:
        os.environ.pop("VB_GEMM_NARROW", None)
        if old is not None:
            os.environ["VB_GEMM_NARROW"] = old
    m.load_state_dict(sd if sd is not None else _sd(kind))
    if k["ce"]:
        m.set_candidate_elimination(*k["ce"], form="compact")
    return m


def _pair(kind):
    """(wide, narrow): one pair of models per kind for the whole module."""
    if kind not in _MODELS:
        _MODELS[kind] = (_build(kind, 0), _build(kind, 1))
    for m in _MODELS[kind]:
        m.set_open_loop(False)
    return _MODELS[kind]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64 if t.element_size() == 8 else torch.uint8)


def _equal(a, b, what):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), what


def _nan_outputs(B, F):
    from vittracker_amd import native
    o = native.Outputs(B, F, "cuda")
    for k in KEYS:
        getattr(o, k).fill_(float("nan"))
    return o


def _run(m, kind, B):
    """Everything the two forms are compared on, every output buffer NaN before the call that writes it."""
    import torch
    from vittracker_amd import native, synth
    k = KINDS[kind]
    tz, tx, C, F = k["tz"], k["tx"], k["C"], k["tx"] // 16
    L, LX = (tz // 16) ** 2 + F * F, F * F
    z, x = synth.synth_inputs(3, B, tz, tx)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    pd = torch.from_numpy(synth.synth_patches(3, B, tx)).cuda()
    nan = float("nan")
    got = {}
    tok = torch.full((B, L, C), nan, device="cuda")
    native._check(m._L.vt_stem(m._h, native._ptr(zd), native._ptr(xd), B, native._stream(None), native._ptr(tok)), "vt_stem", m._L)
    got["stem"] = tok
    feat, resid = torch.full((B, LX, C), nan, device="cuda"), torch.full((B, L, C), nan, device="cuda")
    native._check(m._L.vt_blocks(m._h, native._ptr(tok), B, -1, native._stream(None), native._ptr(feat), native._ptr(resid)), "vt_blocks", m._L)
    got["feat"], got["resid_out"] = feat, resid
    if k["ce"]:
        got["ce_removed"], got["ce_scores"] = m.ce_result(B)
    out = m.forward(zd, xd, out=_nan_outputs(B, F))
    for key in KEYS:
        got["forward." + key] = getattr(out, key).clone()
    out = m.forward_u8(zd, pd, out=_nan_outputs(B, F))
    for key in KEYS:
        got["forward_u8." + key] = getattr(out, key).clone()
    # two tracking steps on fixed frames from fixed boxes
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, (3, B, H, W, 3)).astype(np.uint8)).cuda()
    states = torch.from_numpy(np.stack([[30 + b, 20 + b, 30 + (b % 7), 24 + (b % 5)] for b in range(B)]).astype(np.float64)).cuda()
    zc, rf = m.crop(frames[0], states, 2.0, tz, MEAN, STD)
    m.set_template(zc)
    xw, rec = torch.empty(B, 3, tx, tx, device="cuda"), torch.full((B, 5), nan, dtype=torch.float64, device="cuda")
    for f in (1, 2):
        out = _nan_outputs(B, F)
        m.track_step(frames[f], states, 4.0, MEAN, STD, xw, rf, out, record=rec)
        torch.cuda.synchronize()
        got[f"step{f}.record"], got[f"step{f}.states"] = rec.clone(), states.clone()
        for key in KEYS:
            got[f"step{f}." + key] = getattr(out, key).clone()
    if k["ce"]:
        got["step.ce_removed"], got["step.ce_scores"] = m.ce_result(B)
    torch.cuda.synchronize()
    return got


# ------------------------------------------------------------------------------------------------- 1: bit identity
@pytest.mark.parametrize("kind,B", CASES, ids=[f"{k}-B{b}" for k, b in CASES])
def test_narrow_tiles_give_the_wide_tiles_bits(kind, B):
    import torch
    wide, narrow = _pair(kind)
    assert wide.gemm_form(B) == 0 and narrow.gemm_form(B) != 0
    a, b = _run(wide, kind, B), _run(narrow, kind, B)
    assert a.keys() == b.keys()
    for key in a:
        _equal(a[key], b[key], key)
        if "ce_scores" not in key and not (KINDS[kind]["ce"] and key == "resid_out"):      # (scores: NaN for tokens removed earlier, by contract)
            assert torch.isfinite(a[key].double()).all(), key
    assert not torch.equal(a["step1.states"], a["step2.states"])


# ------------------------------------------------------------------------------------------------- 2: the form really ran
def test_gemm_form_reports_what_runs():
    from vittracker_amd import native as N
    every = N.GEMM_PATCH | N.GEMM_PROJ | N.GEMM_FC1 | N.GEMM_FC2 | N.GEMM_HEAD
    for kind in ("base256", "large256"):       # the fused qkv + attention kernel: no q | k GEMM to report
        wide, narrow = _pair(kind)
        assert narrow.gemm_form(1) == every and wide.gemm_form(1) == 0
        assert narrow.gemm_form(256) == every and wide.gemm_form(256) == 0
    for kind in ("base384", "ce256"):          # qk GEMM + v GEMM + the streaming attention kernel
        wide, narrow = _pair(kind)
        assert narrow.gemm_form(1) == every | N.GEMM_QK and wide.gemm_form(1) == 0
    auto = _build("base256", None, maxB=1, depth=1)
    try:
        assert auto.gemm_form(1) != 0 and auto.gemm_form(256) == 0
        assert auto.gemm_form(1) & N.GEMM_PROJ and auto.gemm_form(1) & N.GEMM_FC2      # N = 768: 6 wide tiles at B = 1
    finally:
        auto.close()
    small = N.Model(128, 256, max_batch=1)      # vit_48 path
    try:
        assert small.gemm_form(1) == 0
    finally:
        small.close()


# ------------------------------------------------------------------------------------------------- 3: reference fixtures
def _against_fixture(out, g, tag):
    for k, tol in TOL_MAP.items():
        err = float(np.abs(getattr(out, k).cpu().numpy() - g[k]).max())
        print(tag, k, err)
        assert err < tol, (k, err)
    eb = float(np.abs(out.pred_boxes.cpu().numpy() - g["pred_boxes"][:, 0]).max())
    eh = float(np.abs(out.hann_boxes.cpu().numpy() - g["hann_boxes"]).max())
    ec = float(np.abs(out.conf.cpu().numpy() - g["conf"]).max())
    print(tag, "pred_boxes", eb, "hann_boxes", eh, "conf", ec)
    assert eb < TOL_BOX and eh < TOL_BOX and ec < TOL_MAP["score_map"], (eb, eh, ec)


@pytest.mark.parametrize("path", vitb_golden_files() + vb384_files()[:1], ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixtures_through_the_narrow_tiles(path):
    import torch
    is384 = os.path.basename(path).startswith("ref_vb384")
    g, sd, z, x = load_vb384(path) if is384 else load_vitb_case(path)
    B = z.shape[0]
    m = _build("base384" if is384 else "base256", 1, sd=sd, maxB=B, depth=12)
    try:
        assert m.gemm_form(B) != 0
        out = m.forward(torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda(), out=_nan_outputs(B, (384 if is384 else 256) // 16))
        _against_fixture(out, g, os.path.basename(path))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------- 4: plumbing under =1
@pytest.mark.parametrize("kind,B", [("base256", 1), ("base256", 5), ("base384", 3)])
def test_eager_captured_and_replayed_steps_agree(kind, B):
    import torch
    from vittracker_amd import synth
    k = KINDS[kind]
    _, m = _pair(kind)
    z, x = synth.synth_inputs(5, B, k["tz"], k["tx"])
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    F = k["tx"] // 16
    first = m.forward(zd, xd, out=_nan_outputs(B, F))
    again = m.forward(zd, xd, out=_nan_outputs(B, F))      # two consecutive eager runs
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.isfinite(getattr(first, key)).all(), key
        _equal(getattr(first, key), getattr(again, key), key)
    graph, out = m.capture(zd, xd, out=_nan_outputs(B, F))
    for _ in range(2):
        graph.launch()
        torch.cuda.synchronize()
        for key in KEYS:
            _equal(getattr(first, key), getattr(out, key), key)
            getattr(out, key).fill_(float("nan"))
    del graph


def _params():
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters("vitb_256")
    p.allow_synthetic_weights = True
    p.checkpoint = None
    p.host_crop = False
    return p


def test_a_batched_slot_equals_the_one_sequence_tracker(monkeypatch):
    """BatchedVitTracker with three sequences against the ostrack plugin on the first of them, both created under VB_GEMM_NARROW=1: the same
    boxes and confidences, bit for bit (B = 3 is 960 rows, B = 1 is 320: other tile counts, other partial tiles)."""
    from vittracker_amd import native as N
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    from vittracker_amd.tracker import vit_dist as plugin_mod
    from vittracker_amd.tracker.ostrack import OSTrack
    monkeypatch.setenv("VB_GEMM_NARROW", "1")
    seqs = [synthetic_sequence(f"s{q}", 4, seed=1000 * 126 + q) for q in range(3)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]
    bt = BatchedVitTracker(_params(), 3)
    bt.initialize(np.stack([s.frames[0] for s in seqs]), box0)
    assert bt.net._native().gemm_form(3) & N.GEMM_FC1
    recs = [bt.track_record(np.stack([s.frames[t] for s in seqs])).copy() for t in range(1, 4)]
    assert np.isfinite(np.asarray(recs)).all()
    del bt
    plugin_mod._PIPELINES.clear()
    tr = OSTrack(_params(), "synthetic")
    tr.initialize(seqs[0].frames[0], {"init_bbox": box0[0]})
    for t in range(1, 4):
        got = tr.track(seqs[0].frames[t])
        assert got["target_bbox"] == recs[t - 1][0][:4].tolist(), t
        assert got["confidence"] == float(np.float32(recs[t - 1][0][4])), t
    plugin_mod._PIPELINES.clear()
