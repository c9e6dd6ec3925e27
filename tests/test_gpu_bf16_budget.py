"""GPU: the four ViT-Base attention routes against the fp64 truth, held to a multiple of the bf16 oracle's own error on the same input
(tests/bf16_budget.py), in every softmax regime:

  fused       vbq::qkv_attn_kernel            the default at 128 / 256 (320 tokens)
  unfused     vba::attn_kernel<320, 64>       VB_FUSED_QKV=0
  stream320   vbs::attn_stream_kernel<320>    VB_FUSED_QKV=0 VB_ATTN_STREAM=1
  stream720   vbs::attn_stream_kernel<720>    192 / 384 (720 tokens: 11 whole 64-key chunks + 16 real and 16 pad keys)

Attention alone: a depth-1 model with identity proj and zero fc2 (bf16_budget.attn_only) at max_batch = B = 2, so frame 0's reads past
its last token land in frame 1's rows and frame 1's in the zero-filled workspace tail; resid - x is the kernel's bf16 output of every
frame, head and row, all B x L x 768 values compared.  Full block: depth 2 with the regime's real weights, the residual after 1 and
after 2 blocks from the fp32 tokens, all rows of both frames, rel-L2 against the rows' centred norm.

Asserted: finite everywhere, and err(kernel) <= FACTORS[stage] x err(oracle) + floor for rel-L2, for max-abs and for the rel-L2 of every
(frame, head, 16-query tile) slot; in below_zero, last_keys and first_keys at 720 tokens each frame on its own as well.  The oracle is the
whole-row form for fused / unfused and the 64-key chunked form for the streaming kernels.  On attention alone the kernel - oracle distance
is held to bf16_budget.KO_FRAC of the oracle's error as well (measured <= 0.23 of it); after whole blocks it is printed, not asserted.  Every case prints its bf16_budget.fmt row;
the CPU references are built once per (geometry, regime) per module, a case is one or two launches."""
import numpy as np
import pytest

import bf16_budget as bb

pytestmark = pytest.mark.gpu

ROUTES = {                      # name -> (tokens, environment read at model creation, the oracle's softmax form)
    "fused": (320, {}, None),
    "unfused": (320, {"VB_FUSED_QKV": "0"}, None),
    "stream320": (320, {"VB_FUSED_QKV": "0", "VB_ATTN_STREAM": "1"}, bb.KC),
    "stream720": (720, {}, bb.KC),
}
B = 2
_REF = {}


def _ref(kind, L, name, chunk):
    """CPU references, once per module: ('attn' | 'full', tokens, regime) -> state dict, tokens, truth, and per softmax form the oracle."""
    key = (kind, L, name)
    if key not in _REF:
        if kind == "attn":
            sd, X = bb.regime(name, L, B=B)
            q, k, v = bb.qkv(sd, X, 0, "bf16")
            _REF[key] = {"sd": bb.attn_only(sd), "X": X, "truth": bb.attention(*bb.qkv(sd, X, 0, "truth")), "qkv": (q, k, v), "oracle": {}}
        else:
            sd, X = bb.regime(name, L, B=B, depth=2)
            _REF[key] = {"sd": sd, "X": X, "truth": bb.run(sd, X, 2, "truth")[0], "oracle": {}}
    r = _REF[key]
    if chunk not in r["oracle"]:
        r["oracle"][chunk] = bb.attention(*r["qkv"], "bf16", chunk=chunk) if kind == "attn" else bb.run(r["sd"], r["X"], 2, "bf16", chunk=chunk)[0]
    return r, r["oracle"][chunk]


def _model(route, depth, sd, monkeypatch):
    from vittracker_amd import native
    L, env, _ = ROUTES[route]
    for k in ("VB_FUSED_QKV", "VB_ATTN_STREAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tz, tx = bb.SIZES[L]
    m = native.Model(tz, tx, channels=768, heads=12, depth=depth, head_channels=256, max_batch=B)
    m.load_state_dict(sd)
    assert m.L == L
    return m


def _check(r, tag):
    print(tag, bb.fmt(r))
    assert r["finite"], (tag, "not finite")
    assert r["ok"], (tag, bb.fmt(r))


@pytest.mark.parametrize("name", bb.REGIMES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_attention_alone(route, name, monkeypatch):
    import torch
    L, _, chunk = ROUTES[route]
    ref, oracle = _ref("attn", L, name, chunk)
    m = _model(route, 1, ref["sd"], monkeypatch)
    try:
        x = torch.from_numpy(ref["X"]).cuda()
        _, resid = m.blocks(x, nblocks=1, want_resid=True)
        resid = resid.cpu().numpy().astype(np.float64)
    finally:
        m.close()
    assert np.isfinite(resid).all()
    X = ref["X"].astype(np.float64)
    got, at = resid - X, X + ref["truth"]
    _check(bb.judge("attn", got, ref["truth"], oracle, at=at), f"{route} {name}")
    if L == 720 and name in ("below_zero", "last_keys", "first_keys"):       # the pad keys and the partial chunk: each frame on its own
        for f in range(B):
            _check(bb.judge("attn", got[f:f + 1], ref["truth"][f:f + 1], oracle[f:f + 1], at=at[f:f + 1]), f"{route} {name} frame {f}")


@pytest.mark.parametrize("name", bb.FULL_REGIMES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_full_block(route, name, monkeypatch):
    import torch
    L, _, chunk = ROUTES[route]
    ref, oracle = _ref("full", L, name, chunk)
    m = _model(route, 2, ref["sd"], monkeypatch)
    try:
        x = torch.from_numpy(ref["X"]).cuda()
        got = [m.blocks(x, nblocks=k, want_resid=True)[1].cpu().numpy().astype(np.float64) for k in (1, 2)]
    finally:
        m.close()
    for k in (1, 2):
        assert np.isfinite(got[k - 1]).all()
        _check(bb.judge(f"resid{k}", got[k - 1], ref["truth"][k - 1], oracle[k - 1], centred=True), f"{route} {name} after {k}")
