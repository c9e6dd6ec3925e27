"""GPU: the attention routes at widths 1024 / 16 heads (ViT-Large), 384 / 6 (ViT-Small) and 192 / 3 (ViT-Tiny) against the fp64 truth, held to
a multiple of the bf16 oracle's own error on the same input at the same width (tests/bf16_budget.py, ``w=``) -- tests/test_gpu_bf16_budget.py's
statement, FACTORS and KO_FRAC at the three widths it does not run:

  fused       vbq::qkv_attn_wide_kernel<C>    the default at 128 / 256 (320 tokens): row pitch C, q / k / v sections C apart, 16 / 6 / 3 k-tiles,
                                              4 of 16 / all 6 / all 3 heads walked together
  unfused     vba::attn_kernel<320, 64>       VB_FUSED_QKV=0: the qk GEMM at N = 2 C, the transposed-store v GEMM at N = C, K = C
  stream320   vbs::attn_stream_kernel<320>    VB_FUSED_QKV=0 VB_ATTN_STREAM=1, heads = 16 / 6 / 3 at run time
  stream720   vbs::attn_stream_kernel<720>    192 / 384 (720 tokens: 11 whole 64-key chunks + 16 real and 16 pad keys)

Attention alone: a depth-1 model with identity proj and zero fc2 (bf16_budget.attn_only) at max_batch = B = 2, so frame 0's reads past its
last token land in frame 1's rows and frame 1's in the zero-filled workspace tail; resid - x is the kernel's bf16 output of every frame, head
and row, all B x L x C values compared.  fused and stream720 (the default routes, which carry the width-specific code) run all eight regimes
at the width's amplitudes (bf16_budget.AMPS); unfused and stream320 (the 768 kernels over the GEMMs and LayerNorm at the width) run plain,
peaked, last_keys, below_zero, common_mode.  Full block: depth 2 with the regime's real weights on fused and stream720, the residual after 1
and after 2 blocks from the fp32 tokens, all rows of both frames, rel-L2 against the rows' centred norm -- vbm::layernorm_small_kernel,
ln_finalize_kernel<16 / 6 / 3>, fc1 / fc2 at K = C and 4 C under the budget.

Asserted: finite everywhere, and err(kernel) <= FACTORS[stage] x err(oracle) + floor for rel-L2, for max-abs and for the rel-L2 of every
(frame, head, 16-query tile) slot; in below_zero, last_keys and first_keys at 720 tokens each frame on its own as well.  The oracle is the
whole-row form for fused / unfused and the 64-key chunked form for the streaming kernels.  On attention alone the kernel - oracle distance is
held to bf16_budget.KO_FRAC of the oracle's error as well; after whole blocks it is printed, not asserted.  Every case prints its
bf16_budget.fmt row.  At B = 2 the GEMMs take the narrow 128 x 64 tile by default; tests/test_gpu_vit_small.py and
tests/test_gpu_vitb_narrow.py hold narrow == wide bit for bit, so the default alone runs here.  The CPU references are built once per (width,
geometry, regime) in the module's order of cases (width, regime, route), a case is one or two launches.

Measured on one MI355X run of every case (102 cases, 144 judged rows; NOTES.md has the table), kernel error / oracle error as rel-L2 /
max-abs / worst slot [kernel - oracle as a fraction of the oracle's error], widths 1024 | 384 | 192:
  attention alone   fused = unfused   x1.00 / x1.00 / x1.00-1.04, common_mode slot x1.08 | x1.03 | x1.03        [0.01-0.07, common_mode 0.19 | 0.18 | 0.12]
                    stream320         x1.00 / x1.00 / x1.00-1.05, common_mode slot x1.07 | x1.02 | x1.04        [0.01-0.06, common_mode 0.19 | 0.17 | 0.12]
                    stream720         x1.00 / x1.00 (192: ramp_up x0.96, ramp_down x0.84) / x1.01-1.04, peaked slot x1.18 | x1.07 | x1.01;
                                      each frame of below_zero / last_keys / first_keys on its own x1.00 / x1.00 / <= x1.02      [0.02-0.10, common_mode 0.22 | 0.19 | 0.17]
  after 1 block     fused, stream720  x1.00 / x0.94-1.05 / x1.00-1.05                                           [0.02-0.23, common_mode 0.27-0.39]
  after 2 blocks    fused, stream720  x0.99-1.00 / x0.86-1.09 / x1.03-1.09                                      [0.09-0.65, common_mode 0.64-0.70]
The figures are the 768 ones (bf16_budget.FACTORS' comment): no width, route or regime stands out, nothing was over its bound, no kernel and
no part of the oracle changed.  The largest slot ratio, x1.18 (width 1024, stream720, peaked, frame 1 / head 9 / tile 27), is one 16-query
tile of a regime whose P is nearly one-hot; the case's rel-L2 and max-abs are x1.00."""
import numpy as np
import pytest

import bf16_budget as bb

pytestmark = pytest.mark.gpu

WIDTHS = (1024, 384, 192)
ROUTES = {                      # name -> (tokens, environment read at model creation, the oracle's softmax form)
    "fused": (320, {}, None),
    "unfused": (320, {"VB_FUSED_QKV": "0"}, None),
    "stream320": (320, {"VB_FUSED_QKV": "0", "VB_ATTN_STREAM": "1"}, bb.KC),
    "stream720": (720, {}, bb.KC),
}
DEFAULT_ROUTES = ("fused", "stream720")          # all eight regimes; the full-block cases
GEMM_REGIMES = ("plain", "peaked", "last_keys", "below_zero", "common_mode")          # unfused, stream320
B = 2
_REF = {}


def _ref(kind, C, L, name, chunk):
    """CPU references: ('attn' | 'full', width, tokens, regime) -> state dict, tokens, truth, and per softmax form the oracle.  One entry
    per (kind, tokens) is kept -- the cases of a (width, regime) are neighbours -- so the module never holds more than four state dicts."""
    w = bb.WIDTHS[C]
    if _REF.get((kind, L), {}).get("key") != (C, name):
        if kind == "attn":
            sd, X = bb.regime(name, L, B=B, w=w)
            _REF[(kind, L)] = {"key": (C, name), "sd": bb.attn_only(sd, w=w), "X": X, "truth": bb.attention(*bb.qkv(sd, X, 0, "truth", w=w)),
                               "qkv": bb.qkv(sd, X, 0, "bf16", w=w), "oracle": {}}
        else:
            sd, X = bb.regime(name, L, B=B, depth=2, w=w)
            _REF[(kind, L)] = {"key": (C, name), "sd": sd, "X": X, "truth": bb.run(sd, X, 2, "truth", w=w)[0], "oracle": {}}
    r = _REF[(kind, L)]
    if chunk not in r["oracle"]:
        r["oracle"][chunk] = (bb.attention(*r["qkv"], "bf16", chunk=chunk) if kind == "attn"
                              else bb.run(r["sd"], r["X"], 2, "bf16", chunk=chunk, w=w)[0])
    return r, r["oracle"][chunk]


def _model(C, route, depth, sd, monkeypatch):
    from vittracker_amd import native
    L, env, _ = ROUTES[route]
    for k in ("VB_FUSED_QKV", "VB_ATTN_STREAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tz, tx = bb.SIZES[L]
    family = {} if C == 1024 else {"family": "vit"}          # as tests/test_gpu_vitl.py and tests/test_gpu_vit_small.py create theirs
    m = native.Model(tz, tx, channels=C, heads=bb.WIDTHS[C].heads, depth=depth, head_channels=256, max_batch=B, **family)
    try:
        assert m.channels == C and m.L == L
        m.load_state_dict(sd)
    except BaseException:
        m.close()
        raise
    return m


def _check(r, tag):
    print(tag, bb.fmt(r))
    assert r["finite"], (tag, "not finite")
    assert r["ok"], (tag, bb.fmt(r))


def _cases(routes_regimes):
    return [pytest.param(C, route, name, id=f"{C}-{route}-{name}") for C in WIDTHS for name in bb.REGIMES for route, names in routes_regimes
            if name in names]


@pytest.mark.parametrize("C,route,name", _cases([(r, bb.REGIMES if r in DEFAULT_ROUTES else GEMM_REGIMES) for r in ROUTES]))
def test_attention_alone(C, route, name, monkeypatch):
    import torch
    L, _, chunk = ROUTES[route]
    w = bb.WIDTHS[C]
    ref, oracle = _ref("attn", C, L, name, chunk)
    m = _model(C, route, 1, ref["sd"], monkeypatch)
    try:
        x = torch.from_numpy(ref["X"]).cuda()
        _, resid = m.blocks(x, nblocks=1, want_resid=True)
        resid = resid.cpu().numpy().astype(np.float64)
    finally:
        m.close()
    assert resid.shape == (B, L, C) and np.isfinite(resid).all()
    X = ref["X"].astype(np.float64)
    got, at = resid - X, X + ref["truth"]
    _check(bb.judge("attn", got, ref["truth"], oracle, at=at, w=w), f"{C} {route} {name}")
    if L == 720 and name in ("below_zero", "last_keys", "first_keys"):       # the pad keys and the partial chunk: each frame on its own
        for f in range(B):
            _check(bb.judge("attn", got[f:f + 1], ref["truth"][f:f + 1], oracle[f:f + 1], at=at[f:f + 1], w=w), f"{C} {route} {name} frame {f}")


@pytest.mark.parametrize("C,route,name", _cases([(r, bb.FULL_REGIMES) for r in DEFAULT_ROUTES]))
def test_full_block(C, route, name, monkeypatch):
    import torch
    L, _, chunk = ROUTES[route]
    w = bb.WIDTHS[C]
    ref, oracle = _ref("full", C, L, name, chunk)
    m = _model(C, route, 2, ref["sd"], monkeypatch)
    try:
        x = torch.from_numpy(ref["X"]).cuda()
        got = [m.blocks(x, nblocks=k, want_resid=True)[1].cpu().numpy().astype(np.float64) for k in (1, 2)]
    finally:
        m.close()
    for k in (1, 2):
        assert got[k - 1].shape == (B, L, C) and np.isfinite(got[k - 1]).all()
        _check(bb.judge(f"resid{k}", got[k - 1], ref["truth"][k - 1], oracle[k - 1], centred=True, w=w), f"{C} {route} {name} after {k}")
