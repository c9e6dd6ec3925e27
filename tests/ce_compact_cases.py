"""Helpers of the compact form of candidate elimination (vb_ce.h: the kept tokens gathered into shorter frames behind every stage), for
tests/test_vitb_ce_compact_host.py (CPU) and tests/test_gpu_vitb_ce_compact.py, on tests/ce_budget.py and tests/bf16_budget.py.

  * ``model``: a native ViT-Base model with the stages set in a given form.
  * ``compact_attention``: the attention oracle over the COMPACTED key order -- a frame's template keys, then its kept search keys in
    ascending global index, 64-key chunks counted from there (the masked form's oracle, cb.masked_attention, chunks the original positions).
  * ``stage2_case`` / ``stage2_refs``: the second stage of a depth-2 model (CE_LOC [0, 1], ratios 0.7, 0.7; block 0 attention-only, so that
    the bf16 copy block 1 reads is centred on its rows' own mean) -- the fp64 truth score and the bf16 oracle's from a residual stream
    after block 0 and a stage-1 keep set, with E_o and the band.  On the CPU both come from the bf16 oracle, on the GPU from the device."""
from __future__ import annotations

import numpy as np

import bf16_budget as bb
import ce_budget as cb

# (keep ratio, live rows, frame rows) at 64 + 256 tokens: the tails the run-time attention kernel meets
ATTN_RATIOS = {0.7: (244, 256), 0.5: (192, 192), 0.43: (175, 176), 0.35: (154, 160), 0.1: (90, 96)}
STAGE2_RATIOS = [0.7, 0.7]
# The seed of the plain regime per token count for the stage-2 selection, chosen on the CPU among ce_budget's 26 / 27 and their neighbours
# 24-30 as the one that leaves the most room under cb.BAND_CAP (0.25) -- the device's stage-1 keep set differs from the oracle's by the
# tokens inside stage 1's band, so the share it sees differs a little.  Worst band share per frame over CTR_POINT / CTR_REC / ALL, with the
# bf16 oracle's stage-1 keep set (tests/test_vitb_ce_compact_host.py asserts the chosen ones):
#   320: seed 26 0.128 (27 0.139, 24 0.139, 30 0.133, 29 0.183, 25 0.200, 28 0.244)
#   720: seed 29 0.114 (24 0.205, 30 0.208, 26 0.225, 28 0.230, 27 0.267, 25 0.297)
STAGE2_SEEDS = {320: 26, 720: 29}
_CASES, _REFS = {}, {}


def model(L_or_sizes, depth, sd, B, loc, ratio, rows=None, form="compact"):
    from vittracker_amd import native
    tz, tx = bb.SIZES[L_or_sizes] if isinstance(L_or_sizes, int) else L_or_sizes
    m = native.Model(tz, tx, channels=768, heads=12, depth=depth, head_channels=256, max_batch=B)
    m.load_state_dict(sd)
    if loc is not None:
        m.set_candidate_elimination(loc, ratio, rows, form=form)
    return m


def top_keep(scores, count):
    """(B, count) ascending global indices of the `count` largest scores of each frame (NaN = absent), the lower index winning a tie."""
    out = []
    for s in scores:
        cand = np.flatnonzero(~np.isnan(s))
        order = cand[np.argsort(-s[cand], kind="stable")]
        out.append(np.sort(order[:count]))
    return np.stack(out)


def compact_attention(q, k, v, keep, lz, mode="bf16", chunk=None):
    """softmax(q k^T) v over each frame's template + kept keys IN COMPACTED ORDER (bb.attention on the gathered rows), scattered back to
    (B, L, 768); rows of removed tokens are 0.  keep: (B, n) ascending global search indices."""
    B, _, L, _ = q.shape
    idx = np.concatenate([np.tile(np.arange(lz), (B, 1)), lz + np.asarray(keep)], axis=1)      # (B, lz + n)

    def take(a):
        return np.stack([a[b][:, idx[b]] for b in range(B)])
    o = bb.attention(take(q), take(k), take(v), mode, chunk=chunk)
    out = np.zeros((B, L, o.shape[-1]))
    for b in range(B):
        out[b, idx[b]] = o[b]
    return out


def stage2_case(L, seed=None):
    """(state dict, tokens) of the stage-2 model at L tokens: the plain regime, depth 2, block 0 attention-only."""
    seed = STAGE2_SEEDS[L] if seed is None else seed
    if (L, seed) not in _CASES:
        sd, X = bb.regime("plain", L, seed=seed, B=2, depth=2)
        _CASES[(L, seed)] = (bb.attn_only(sd, 0), X)
    return _CASES[(L, seed)]


def stage2_refs(sd, r1, keep1, lz, rows, count2):
    """Stage 2 from the dense residual after block 0 (r1; rows of removed tokens are never read) under the stage-1 keep set keep1:
    fp64 truth score, bf16 oracle score, E_o, and the band around the count2-th score (cb.band)."""
    L = r1.shape[1]
    present = cb.present_mask(L, lz, keep1)
    r1 = np.asarray(r1, np.float64)
    qt, kt, _ = bb.qkv(sd, r1, 1, "truth")
    qo, ko, _ = bb.qkv(sd, r1, 1, "bf16", centre=r1.mean(-1))
    truth, oracle = cb.score(qt, kt, lz, rows, present), cb.score(qo, ko, lz, rows, present)
    live = ~np.isnan(truth)
    e_o = float(np.abs(oracle - truth)[live].max())
    must_keep, must_drop, share = cb.band(truth, count2, e_o)
    return {"truth": truth, "oracle": oracle, "e_o": e_o, "must_keep": must_keep, "must_drop": must_drop, "share": share, "present": present}


def stage2_cpu(L, trange, seed=None):
    """Once per process: stage 2 with the bf16 oracle in the device's place -- its residual after block 0 and its stage-1 keep set."""
    seed = STAGE2_SEEDS[L] if seed is None else seed
    key = (L, trange, seed)
    if key not in _REFS:
        sd, X = stage2_case(L, seed)
        lz, lx = bb.GEOS[L]
        rows = cb.range_rows(trange, L)
        c1 = int(np.ceil(STAGE2_RATIOS[0] * lx))
        c2 = int(np.ceil(STAGE2_RATIOS[1] * c1))
        if ("r1", L, seed) not in _REFS:
            _REFS[("r1", L, seed)] = (bb.run(sd, X, 1, "bf16", chunk=bb.KC)[0][-1], bb.qkv(sd, X, 0, "bf16")[:2])
        r1, (qo, ko) = _REFS[("r1", L, seed)]
        keep1 = top_keep(cb.score(qo, ko, lz, rows), c1)
        _REFS[key] = dict(stage2_refs(sd, r1, keep1, lz, rows, c2), keep1=keep1, count1=c1, count2=c2)
    return _REFS[key]
