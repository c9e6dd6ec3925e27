"""GPU: the role map of the balanced G128 block kernel (vt_blocks.h).  With a one-tile template the four guest waves share the
TEMPLATE tile (rows 0-15) and the owner waves own the four search tiles; in the last block the guests stop after publishing k and
v^T, and with the template cached they load block 0's q / k / v^T images instead of computing them.

Every test runs a batch of 1 or 3 with the form batch set to 256, so the frame form -- the kernel the headline bench times -- runs:
one frame exercises every tile role, an odd batch the per-frame addressing."""
import numpy as np
import pytest

from conftest import GEOMS, golden_files, load_case

pytestmark = pytest.mark.gpu

TOL_ACT = 1e-4      # tests/test_gpu_parity.py
TOL_MAP = 1e-4
OUT_KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _model(sd, B, precision="f32"):
    from vittracker_amd import native
    tz, tx = GEOMS["G128"]
    m = native.Model(tz, tx, max_batch=B, precision=precision)
    m.load_state_dict(sd)
    m.set_form_batch(256)
    return m


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("bf3", [None, "0", "1"], ids=["default", "fp32_mfma", "qkv_mlp_bf16x3"])
def test_last_block_skip_drops_nothing_the_search_rows_need(bf3, monkeypatch):
    """Without the residual output the guests skip the last block after k / v^T; with it nothing is skipped.  The search rows'
    features must not notice: bit for bit."""
    from vittracker_amd import synth
    torch = _torch()
    if bf3 is None:
        monkeypatch.delenv("VT_BLOCKS_BF3", raising=False)
    else:
        monkeypatch.setenv("VT_BLOCKS_BF3", bf3)      # read at vt_create
    sd = synth.synth_state_dict(7, len_z=16, len_x=64)
    z, x = synth.synth_inputs(7, 3, 64, 128)
    m = _model(sd, 3)
    tokens = m.stem(_dev(z), _dev(x))
    skipped = m.blocks(tokens, nblocks=3, want_resid=False).clone()
    full, resid = m.blocks(tokens, nblocks=3, want_resid=True)
    torch.cuda.synchronize()
    assert torch.isfinite(resid).all()
    assert torch.equal(skipped, full)


@pytest.mark.parametrize("path", [p for p in golden_files("ref_G128") if "_b1" in p], ids=lambda p: p.split("/")[-1][:-4])
def test_roles_against_reference_activations_per_tile(path):
    """The residual stream after each block, from the REFERENCE's tokens, separately for the guests' tile (rows 0-15) and the
    owners' tiles (rows 16-79): a swapped or stale tile names itself."""
    g, sd, z, x = load_case(path)
    m = _model(sd, 1)

    def tok(a, pos):
        B, C, H, W = a.shape
        return a.reshape(B, C, H * W).transpose(0, 2, 1) + pos
    ref_tokens = np.concatenate([tok(g["act_stem3_z"], sd["pos_embed_z"]), tok(g["act_stem3_x"], sd["pos_embed_x"])], 1)
    tokens = _dev(ref_tokens.astype(np.float32))
    for nb in (1, 2, 3):
        feat, resid = m.blocks(tokens, nblocks=nb, want_resid=True)
        got, want = resid.cpu().numpy(), g[f"act_block{nb - 1}"]
        np.testing.assert_allclose(got[:, :16], want[:, :16], atol=TOL_ACT, rtol=0, err_msg=f"template rows (guests) after block {nb - 1}")
        np.testing.assert_allclose(got[:, 16:], want[:, 16:], atol=TOL_ACT, rtol=0, err_msg=f"search rows (owners) after block {nb - 1}")
    np.testing.assert_allclose(feat.cpu().numpy(), g["act_norm"][:, -m.len_x:], atol=TOL_ACT, rtol=0, err_msg="norm")


def test_peaked_softmax_through_the_frame_form():
    """The scaled-qkv case of test_gpu_parity.py::test_peaked_attention_and_odd_batches (seed 21, q / k rows x 3) on the frame form:
    the guests' merge of per-key-tile partial softmaxes now serves the template queries."""
    from oracle import vt_oracle_np as onp
    from vittracker_amd import synth
    B = 3
    sd = synth.synth_state_dict(21, len_z=16, len_x=64)
    for blk in range(3):
        sd[f"blocks.{blk}.attn.qkv.weight"][:96] *= 3.0
        sd[f"blocks.{blk}.attn.qkv.bias"][:96] *= 3.0
    z, x = synth.synth_inputs(21, B, 64, 128)
    ref = onp.forward(sd, z, x, want_acts=True)
    m = _model(sd, B)
    tokens = m.stem(_dev(z), _dev(x))
    acts = ref["acts"]
    scale = max(1.0, float(np.abs(acts["block2"]).max()))
    for nb in (1, 2, 3):
        feat, resid = m.blocks(tokens, nblocks=nb, want_resid=True)
        np.testing.assert_allclose(resid.cpu().numpy(), acts[f"block{nb - 1}"], atol=TOL_ACT * scale, rtol=0,
                                   err_msg=f"residual after block {nb - 1}")
    out = m.forward(_dev(z), _dev(x))
    for k in ("score_map", "size_map", "offset_map"):
        np.testing.assert_allclose(getattr(out, k).cpu().numpy(), ref[k], atol=TOL_MAP * scale, rtol=0, err_msg=k)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_template_cache_on_the_guest_path_is_exact(precision):
    """vt_set_template stores the guests' q / k / v^T images of block 0 (mode 1); forward(None, x) loads them (mode 2): equal to the
    uncached step bit for bit, on a second search crop too."""
    from vittracker_amd import synth
    torch = _torch()
    B = 3
    m = _model(synth.synth_state_dict(0, len_z=16, len_x=64), B, precision)
    z, x = synth.synth_inputs(11, B, 64, 128)
    _, x2 = synth.synth_inputs(12, B, 64, 128)
    zd, xd, x2d = _dev(z), _dev(x), _dev(x2)
    refs = []
    for xx in (xd, x2d):
        o = m.forward(zd, xx)
        refs.append({k: getattr(o, k).clone() for k in OUT_KEYS})
    m.set_template(zd)
    for xx, ref in zip((xd, x2d), refs):
        got = m.forward(None, xx)
        for k in OUT_KEYS:
            assert torch.equal(getattr(got, k), ref[k]), (precision, k)
    assert not torch.equal(refs[0]["score_map"], refs[1]["score_map"])


def test_frame_form_is_deterministic_over_replays():
    """20 replays of the captured step, and 20 runs of the block stage, give the same bytes (the guests' rendezvous and the
    exchange areas they share with the staged weights are ordered, not racing)."""
    from vittracker_amd import synth
    torch = _torch()
    B = 3
    m = _model(synth.synth_state_dict(3, len_z=16, len_x=64), B)
    z, x = synth.synth_inputs(3, B, 64, 128)
    zd, xd = _dev(z), _dev(x)
    tokens = m.stem(zd, xd)
    feat0 = m.blocks(tokens).clone()
    graph, gout = m.capture(zd, xd)
    graph.launch()
    torch.cuda.synchronize()
    first = {k: getattr(gout, k).clone() for k in OUT_KEYS}
    for it in range(20):
        graph.launch()
        feat = m.blocks(tokens)
        torch.cuda.synchronize()
        assert torch.equal(feat, feat0), it
        for k in OUT_KEYS:
            assert torch.equal(getattr(gout, k), first[k]), (it, k)
