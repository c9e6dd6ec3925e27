"""The accuracy budget of candidate elimination by key masking (vb_ce.h, vbs::attn_stream_masked_kernel), in the manner of
tests/bf16_budget.py and on its ``qkv``, ``bf16``, ``f32`` and ``regime``: the ranking score and the masked attention in fp64 truth and in
the form that rounds to bf16 where the device does.  A plain helper for tests/test_vitb_ce_host.py (CPU) and tests/test_gpu_vitb_ce.py.

Score (``score``).  attn[:, :, :lens_t, lens_t:] -> the selected template rows -> mean(2).mean(1) of lib/models/layers/attn_blocks.py:43-56,
with the softmax restricted to the present keys.  Truth: q, k of ``bb.qkv(.., "truth")``.  Oracle: q, k of ``bb.qkv(.., "bf16")`` -- the
values the qk GEMM leaves in the workspace, which the device reads -- and everything after them in fp64 (the device: f32 dot products,
exp2 against the row maximum, f32 sums in a fixed order: ~1e-7 relative, far below bf16's 2^-9 on q and k).

Selection (``band``).  Neighbouring scores lie 1e-6 apart, the bf16 rounding of q and k moves a score by more: a device's keep set cannot
be compared token for token with the truth's.  What can be held: every token whose truth score clears the cut by more than the device may
be wrong is kept, every token below it by as much is dropped, and the count is exact.  The cut is the midpoint between the count-th and
(count + 1)-th truth scores of a frame; the band is 2 x FACTORS["attn"] x E_o either side (E_o: the oracle's own max error against the
truth on that input; FACTORS["attn"] x E_o is what the device's score may be off by, and two scores are compared).  ``band`` also reports
the share of a frame's candidates inside the band: the inputs of a test must keep it at or below BAND_CAP, or the test says nothing.

Masked attention (``masked_attention``).  softmax(q k^T) v over the present keys only.  Oracle: bb.attention's 64-key chunked form -- P
rounded to bf16 for P.V, the row sum from the unrounded P, the running maximum per chunk with l and O rescaled -- with the chunks at the
ORIGINAL key positions (no compaction: an absent key's logit is -inf where it stands, a chunk without a present key leaves m, l, O alone).

What one MI355X run of tests/test_gpu_vitb_ce.py measured against these bounds is the table at FACTORS_SEEN."""
from __future__ import annotations

import numpy as np

import bf16_budget as bb

FACTOR = bb.FACTORS["attn"]      # 1.65: the project's figure for the same q.k arithmetic
BAND_CAP = 0.25

# device error / oracle error seen in tests 1-3 of tests/test_gpu_vitb_ce.py (the bound is FACTOR = 1.65), one MI355X run:
#   1 score      all 12 cases (plain, peaked x 320, 720 x CTR_POINT, CTR_REC, ALL): x1.00; device - oracle 5e-8 .. 2.9e-6 where E_o is
#                2.2e-6 (plain 720 ALL) .. 2.4e-3 (peaked 320 CTR_POINT): the device's error IS the bf16 rounding of q and k
#   2 selection  no token outside the band on the wrong side in any of the 12 cases (asserted on BAND_CASES); counts exact
#   3 masked     plain / peaked / last_keys / ramp_up x 320 / 720: rel-L2 x1.00, max-abs x1.00, worst slot x1.01-1.09 (ramp_up 720),
#                kernel - oracle 0.02-0.07 of the oracle's error (KO_FRAC allows 0.69)
#   whole model  stage 1 against the fixtures' scores: x0.56 (256), x0.64 (384), x1.00 (d3), x1.44 (d5) of an E_o whose chain only
#                approximates the centring of the stage block's bf16 copy; the band there is 2 x 1.65 x E_o, and held
FACTORS_SEEN = {"score": 1.00, "masked_rel": 1.00, "masked_abs": 1.00, "masked_slot": 1.09, "masked_ko_frac": 0.07}


def present_mask(L, lz, keep=None):
    """(B, L) bool from per-frame kept GLOBAL search indices (B, n); None -> every key."""
    if keep is None:
        return None
    keep = np.asarray(keep)
    m = np.zeros((keep.shape[0], L), bool)
    m[:, :lz] = True
    for b in range(keep.shape[0]):
        m[b, lz + keep[b]] = True
    return m


def score(q, k, lz, rows=None, present=None):
    """(B, Lx) float64: the mean over heads and the selected template rows of softmax(q k^T) over the present keys, at each search key;
    NaN where the key is absent.  q (pre-scaled), k: (B, heads, L, 64)."""
    B, H, L, _ = q.shape
    rows = np.arange(lz) if rows is None else np.flatnonzero(np.asarray(rows))
    out = np.empty((B, L - lz))
    for b in range(B):
        S = q[b][:, rows] @ k[b].transpose(0, 2, 1)              # (H, R, L)
        if present is not None:
            S[..., ~present[b]] = -np.inf
        P = np.exp(S - S.max(-1, keepdims=True))
        P /= P.sum(-1, keepdims=True)
        out[b] = P[..., lz:].mean(1).mean(0)
        if present is not None:
            out[b, ~present[b, lz:]] = np.nan
    return out


def band(truth, count, e_o):
    """Per frame of truth scores (B, Lx) (NaN = absent): (must_keep, must_drop) bool arrays and the share of the candidates inside
    the band of 2 x FACTOR x e_o either side of the midpoint between the count-th and (count + 1)-th score."""
    half = 2.0 * FACTOR * e_o
    keep = np.zeros(truth.shape, bool)
    drop = np.zeros(truth.shape, bool)
    share = []
    for b in range(truth.shape[0]):
        s = truth[b]
        cand = ~np.isnan(s)
        srt = np.sort(s[cand])[::-1]
        mid = 0.5 * (srt[count - 1] + srt[count])
        keep[b] = cand & (s > mid + half)
        drop[b] = cand & (s < mid - half)
        share.append(float((cand & ~keep[b] & ~drop[b]).sum()) / float(cand.sum()))
    return keep, drop, share


def masked_attention(q, k, v, present=None, mode="truth", chunk=None):
    """bb.attention with per-frame present keys (B, L) bool; chunk = bb.KC: the streaming kernel's online softmax, chunks at the original
    key positions."""
    B, H, L, _ = q.shape
    rnd = bb.bf16 if mode != "truth" else (lambda a: a)
    out = np.empty((B, L, H * bb.HD))
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            S = q[b] @ k[b].transpose(0, 2, 1)
            if present is not None:
                S[..., ~present[b]] = -np.inf
            if chunk is None:
                P = np.exp(S - S.max(-1, keepdims=True))
                O = (rnd(P) @ v[b]) / P.sum(-1, keepdims=True)
            else:
                m = np.full(S.shape[:2] + (1,), -1e30)
                l = np.zeros_like(m)
                O = np.zeros(S.shape[:2] + (bb.HD,))
                for c in range(0, L, chunk):
                    Sc = S[..., c:c + chunk]
                    mx = np.maximum(m, Sc.max(-1, keepdims=True))
                    alpha = np.exp(m - mx)
                    P = np.exp(Sc - mx)
                    l = l * alpha + P.sum(-1, keepdims=True)
                    O = O * alpha + rnd(P) @ v[b][:, c:c + chunk]
                    m = mx
                O = O / l
            out[b] = rnd(O).transpose(1, 0, 2).reshape(L, H * bb.HD)
    return out


RANGES = ("CTR_POINT", "CTR_REC", "ALL")
SCORE_REGIMES = ("plain", "peaked")
SCORE_B, KEEP_RATIO = 2, 0.7
# The regime seed per (regime, tokens), and the (regime, tokens, range) cases whose inputs keep the band at or below BAND_CAP of a frame's
# candidates -- a property of the INPUTS, found with the truth and the oracle alone on the CPU (band share per frame, seeds 26-29):
#   plain   320  seed 26: CTR_POINT 0.20 / 0.20, CTR_REC 0.10 / 0.07, ALL 0.04 / 0.07   (seeds 27, 28: CTR_POINT 0.26-0.27)
#   plain   720  seed 27: CTR_POINT 0.21 / 0.17, CTR_REC 0.21 / 0.22, ALL 0.06 / 0.05   (seed 26: CTR_POINT 0.44; 28: 0.56; 29: CTR_REC 0.34)
#   peaked  320 / 720, every seed: CTR_POINT 0.93-0.98, CTR_REC 0.76-0.91 (one or four rows of a peaked softmax: E_o ~ 2e-3 is the size
#           of the scores themselves), ALL 0.11-0.20
# so the selection is held on plain at all three ranges and on peaked at ALL; the score itself is held everywhere.
SEEDS = {("plain", 320): 26, ("plain", 720): 27, ("peaked", 320): 26, ("peaked", 720): 26}
BAND_CASES = {(n, L, tr) for n in SCORE_REGIMES for L in (320, 720) for tr in RANGES if n == "plain" or tr == "ALL"}
_REFS = {}


def range_rows(trange, L):
    """Template rows of a CE_TEMPLATE_RANGE at L tokens (lib/utils/ce_utils.py:15-49), as a bool vector; None for ALL."""
    import vitb_ce_oracle as vo
    r = vo.template_rows(trange, {320: 8, 720: 12}[L])
    return None if r is None else r.numpy()


def score_refs(name, L):
    """Once per process: regime `name` at L tokens (SCORE_B frames, depth 1) -> state dict, tokens, and per template range the truth
    score, the bf16 oracle's score and E_o = the oracle's max error against the truth."""
    key = (name, L)
    if key not in _REFS:
        sd, X = bb.regime(name, L, seed=SEEDS[key], B=SCORE_B)
        lz = bb.GEOS[L][0]
        qt, kt, _ = bb.qkv(sd, X, 0, "truth")
        qo, ko, _ = bb.qkv(sd, X, 0, "bf16")
        r = {"sd": sd, "X": X, "lz": lz, "count": int(np.ceil(KEEP_RATIO * (L - lz)))}
        for tr in RANGES:
            rows = range_rows(tr, L)
            t, o = score(qt, kt, lz, rows), score(qo, ko, lz, rows)
            r[tr] = {"truth": t, "oracle": o, "e_o": float(np.abs(o - t).max())}
        _REFS[key] = r
    return _REFS[key]


def kept_rows(a, ref, present):
    """`a` with the rows of absent tokens replaced by `ref`'s: a comparison then sees the kept rows alone (the rows of removed tokens go
    on being computed on the device and are unspecified)."""
    a = np.array(a, np.float64)
    if present is not None:
        a[~present] = np.asarray(ref, np.float64)[~present]
    return a
