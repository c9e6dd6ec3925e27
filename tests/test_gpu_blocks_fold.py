"""GPU: the folded odd K chunk of the G128 balanced frame form (vt_bf3.h mma_odd, vt_blocks.h FOLD).  A lone 16-deep chunk's six
bf16 terms are three K = 32 MFMAs, two terms each, at every site of the block kernel: tile48 (qkv, q k^T, proj, fc1), the owners'
and the guests' P.V, the guests' fc1 and their K-split fc2.

Every case runs B = 3 frames with the form batch set to 256, so the frame form runs on three workgroups -- the smallest shape that
reaches every folded site: three tiles of search tokens on owner waves, the template tile on the guests, all three blocks, the
last block's guest skip.  The reference's fixtures are those of a batch of one; the three frames are that frame three times, and
each is held to the fixture at the tolerance tests/test_gpu_parity.py uses for the stage."""
import numpy as np
import pytest

from conftest import GEOMS, golden_files, load_case

pytestmark = pytest.mark.gpu

TOL_ACT = 1e-4      # tests/test_gpu_parity.py
B = 3
OUT_KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
CASES = [p for p in golden_files("ref_G128") if "_b1" in p]
assert CASES, "no ref_G128_*_b1 golden file: every test of this module would be deselected"


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _model(sd):
    from vittracker_amd import native
    tz, tx = GEOMS["G128"]
    m = native.Model(tz, tx, max_batch=B)
    m.load_state_dict(sd)
    m.set_form_batch(256)
    return m


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", params=CASES, ids=lambda p: p.split("/")[-1][:-4])
def case(request):
    """(fixture, state dict, z, x, the reference's act_stem tokens) of one golden file, every per-frame array three times."""
    g, sd, z, x = load_case(request.param)

    def tok(a, pos):
        n, C, H, W = a.shape
        return a.reshape(n, C, H * W).transpose(0, 2, 1) + pos
    ref_tokens = np.concatenate([tok(g["act_stem3_z"], sd["pos_embed_z"]), tok(g["act_stem3_x"], sd["pos_embed_x"])], 1).astype(np.float32)
    rep = lambda a: np.repeat(np.asarray(a), B, axis=0)
    return g, sd, rep(z), rep(x), rep(ref_tokens)


def _set_bf3(monkeypatch, bf3):
    if bf3 is None:
        monkeypatch.delenv("VT_BLOCKS_BF3", raising=False)
    else:
        monkeypatch.setenv("VT_BLOCKS_BF3", bf3)      # read at vt_create


@pytest.mark.parametrize("bf3", [None, "1"], ids=["default", "a3_off"])
def test_blocks_from_reference_tokens_with_the_guest_skip(case, bf3, monkeypatch):
    """No residual requested: the last block's guests stop after k / v^T.  The search rows' features against act_norm."""
    _set_bf3(monkeypatch, bf3)
    g, sd, _, _, tokens = case
    m = _model(sd)
    feat = m.blocks(_dev(tokens)).cpu().numpy()
    want = g["act_norm"][:, -m.len_x:]
    for f in range(B):
        err = float(np.abs(feat[f] - want[0]).max())
        print(f"fold: bf3={bf3} frame {f} norm max|err| {err:.3e}")
        np.testing.assert_allclose(feat[f], want[0], atol=TOL_ACT, rtol=0, err_msg=f"norm, frame {f}")


@pytest.mark.parametrize("bf3", [None, "1"], ids=["default", "a3_off"])
def test_blocks_from_reference_tokens_with_the_residual(case, bf3, monkeypatch):
    """The residual requested: nothing is skipped, so the guests' proj / fc1 / K-split fc2 run folded in every block.  The
    residual stream after each block against act_block{0,1,2}, the features against act_norm."""
    _set_bf3(monkeypatch, bf3)
    g, sd, _, _, tokens = case
    m = _model(sd)
    td = _dev(tokens)
    for nb in (1, 2, 3):
        feat, resid = m.blocks(td, nblocks=nb, want_resid=True)
        got, want = resid.cpu().numpy(), g[f"act_block{nb - 1}"]
        for f in range(B):
            print(f"fold: bf3={bf3} frame {f} block {nb - 1} max|err| guests {float(np.abs(got[f, :16] - want[0, :16]).max()):.3e} "
                  f"owners {float(np.abs(got[f, 16:] - want[0, 16:]).max()):.3e}")
            np.testing.assert_allclose(got[f, :16], want[0, :16], atol=TOL_ACT, rtol=0, err_msg=f"template rows (guests) after block {nb - 1}, frame {f}")
            np.testing.assert_allclose(got[f, 16:], want[0, 16:], atol=TOL_ACT, rtol=0, err_msg=f"search rows (owners) after block {nb - 1}, frame {f}")
    want = g["act_norm"][:, -m.len_x:]
    for f in range(B):
        np.testing.assert_allclose(feat.cpu().numpy()[f], want[0], atol=TOL_ACT, rtol=0, err_msg=f"norm, frame {f}")


def test_template_cache_store_then_load_equals_cache_off(case):
    """vt_set_template runs block 0's guest qkv in cache mode 1 (compute and store), forward(None, x) in mode 2 (load): both equal
    to the step without the cache, bit for bit -- owners and guests share the one folded helper."""
    torch = _torch()
    _, sd, z, x, _ = case
    m = _model(sd)
    zd, xd = _dev(z), _dev(x)
    off = m.forward(zd, xd)
    ref = {k: getattr(off, k).clone() for k in OUT_KEYS}
    m.set_template(zd)
    on = m.forward(None, xd)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(getattr(on, k), ref[k]), k


def test_ten_replays_of_one_graph_are_bit_identical(case):
    """The accumulator hazard vt_bf3.h records (a chain that mixes the two MFMA kinds read a stale accumulator, and every replay
    differed): all of a tile's instructions are one kind now.  Ten replays of one captured step, no more."""
    torch = _torch()
    _, sd, z, x, _ = case
    m = _model(sd)
    graph, gout = m.capture(_dev(z), _dev(x))
    graph.launch()
    torch.cuda.synchronize()
    first = {k: getattr(gout, k).clone() for k in OUT_KEYS}
    assert all(torch.isfinite(v).all() for v in first.values())
    for it in range(1, 10):
        graph.launch()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.equal(getattr(gout, k), first[k]), (it, k)
