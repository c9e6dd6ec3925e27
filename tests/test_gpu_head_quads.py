"""GPU: conv3 / conv4 of the G128 fused head (head_fused3_kernel, vt_head3.h) on the 4 x 4-block fp32 MFMA, lane = pixel, from fp32
quad-planar LDS maps without halo columns, the 1 x 1 conv in conv4's epilogue and conv3's partial sums exchanged through LDS.

Every case runs at G128 with a batch of 3 (or 1) under set_form_batch(256), so that the kernel the headline bench times runs: three
workgroups.  What can go wrong there and nowhere else as clearly: a dx = +-1 tap of column 0 / 7 that reads a neighbour row instead
of the zero tail, a border row that still holds the bytes of another map, LDS left behind by the block kernel, and a race in the
exchange of conv3's partial sums."""
import numpy as np
import pytest

import fp32_budget as fb
from conftest import GEOMS

pytestmark = pytest.mark.gpu

OUT_KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
B = 3
F = 8
# (row, column) of the one live search token: the four corners, one pixel on each edge, one interior pixel
PIXELS = [(0, 0), (0, 7), (7, 0), (7, 7), (0, 3), (4, 0), (7, 5), (2, 7), (3, 4)]
TOL_ONE_TOKEN = 1e-5      # max-abs on the three maps against the numpy oracle at float64


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sd():
    from vittracker_amd import synth
    return synth.synth_state_dict(0, len_z=16, len_x=64)


@pytest.fixture(scope="module")
def model(sd):
    from vittracker_amd import native
    tz, tx = GEOMS["G128"]
    m = native.Model(tz, tx, max_batch=B)
    m.load_state_dict(sd)
    m.set_form_batch(256)
    yield m
    m.close()


def test_one_live_token_at_every_border_and_corner(model, sd):
    """Features that are zero except for ONE search token (magnitude about 1 in all 48 channels): its 3 x 3 neighbourhoods grow layer
    by layer into the borders, so a wrong redirect into the zero tail or an uncleared border row changes the maps at once."""
    rng = np.random.default_rng(5)
    feat = np.zeros((len(PIXELS), F * F, 48), np.float32)
    for i, (y, x) in enumerate(PIXELS):
        feat[i, y * F + x] = (rng.uniform(0.5, 1.5, 48) * rng.choice([-1.0, 1.0], 48)).astype(np.float32)
    want = fb.head(sd, feat, np.float64)
    fails = []
    for b0 in range(0, len(PIXELS), B):
        out = model.head(_dev(feat[b0:b0 + B]))
        _torch().cuda.synchronize()
        for k in fb.MAPS:
            got = getattr(out, k).cpu().numpy().astype(np.float64)
            for j in range(B):
                err = float(np.abs(got[j] - want[k][b0 + j]).max())
                print(f"token {PIXELS[b0 + j]} {k}: max-abs {err:.2e}")
                if not err <= TOL_ONE_TOKEN:
                    fails.append((PIXELS[b0 + j], k, err))
    assert not fails, fails


def test_head_does_not_depend_on_what_the_block_kernel_left_in_lds(model):
    """forward() runs the head right behind the block kernel on the same CU; the stage-by-stage chain runs it behind a synchronise.
    Bit for bit on all six outputs; a frame alone equals the frame in its batch; a permuted batch permutes the outputs."""
    from vittracker_amd import synth
    torch = _torch()
    z, x = synth.synth_inputs(9, B, 64, 128)
    zd, xd = _dev(z), _dev(x)
    whole = {k: getattr(model.forward(zd, xd), k).clone() for k in OUT_KEYS}
    feat = model.blocks(model.stem(zd, xd))
    torch.cuda.synchronize()
    staged = model.head(feat)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(getattr(staged, k), whole[k]), k
    for i in range(B):
        one = model.forward(zd[i:i + 1].contiguous(), xd[i:i + 1].contiguous())
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(getattr(one, k)[0], whole[k][i]), (i, k)
    perm = [2, 0, 1]
    pd = torch.tensor(perm, device="cuda")
    permuted = model.forward(zd[pd].contiguous(), xd[pd].contiguous())
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(getattr(permuted, k), whole[k][pd]), k
    assert not torch.equal(whole["score_map"][0], whole["score_map"][1])


def test_exchange_of_partial_sums_is_deterministic_over_replays(model):
    """One captured step replayed 20 times gives the same bytes: conv3's partial sums are added in a fixed order behind a barrier,
    not in the order the waves arrive."""
    from vittracker_amd import synth
    torch = _torch()
    z, x = synth.synth_inputs(3, B, 64, 128)
    zd, xd = _dev(z), _dev(x)
    graph, gout = model.capture(zd, xd)
    graph.launch()
    torch.cuda.synchronize()
    first = {k: getattr(gout, k).clone() for k in OUT_KEYS}
    assert torch.isfinite(first["score_map"]).all()
    for it in range(20):
        graph.launch()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(getattr(gout, k), first[k]), (it, k)


def test_head_stage_within_the_fp32_budget(model, sd):
    """The head stage on the fp64 truth's normalised features (plain regime, the case of tests/test_gpu_fp32_budget.py): the three maps
    within fp32_budget.FACTORS (4.0) of the fp32 oracle's own error against the truth, rel-L2 and max-abs."""
    from vittracker_amd import synth
    z, x = synth.synth_inputs(0, B, 64, 128)
    _, N = fb.stage_inputs(sd, z, x)
    truth, o32 = fb.head(sd, N, np.float64), fb.head(sd, N, np.float32)
    out = model.head(_dev(N))
    _torch().cuda.synchronize()
    recs = [fb.judge(k, getattr(out, k).cpu().numpy(), truth[k], o32[k]) for k in fb.MAPS]
    for r in recs:
        print(fb.fmt(r))
        assert r["oracle_rel"] > 0 and r["oracle_abs"] > 0, r       # the budget is not degenerate on this seed
    assert all(r["ok"] for r in recs), [fb.fmt(r) for r in recs if not r["ok"]]
