"""CPU oracle (PyTorch, fp32) of the candidate-elimination ViT-Base OSTrack (``MODEL.BACKBONE.TYPE: vit_base_patch16_224_ce``):
``oracle.vitb_oracle_torch``'s modules walked block by block with the elimination of ``lib/models/layers/attn_blocks.py:20-85`` and the
recovery of ``lib/models/ostrack/vit_ce.py:151-186`` restated -- in the reference's COMPACTED form (the kept tokens are gathered and the
rest of the network runs on the shorter sequence), so that a device that only masks keys is held to what the reference computes, not to
its own scheme.  TEST INFRASTRUCTURE ONLY.

Pinned by tests/test_vitb_ce_host.py against tests/golden/ref_vbce_*.npz (outputs of the reference's own code).

``forced`` (optional): per stage a (B, keep_k) integer array of the GLOBAL search indices to keep, replacing the oracle's own ranking:
the device's ranking of bf16 rows cannot be compared token for token with an fp32 one (neighbouring scores lie 1e-6 apart), so
everything downstream of a selection is compared under the device's own keep sets.

Kept tokens stay in ascending global order here (the reference orders them by descending score); attention, LayerNorm and the MLP do not
see the order, and the final scatter restores the positions either way."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import vitb_oracle_torch as ob


def keep_counts(len_x, ratios):
    out, n = [], int(len_x)
    for r in ratios:
        n = math.ceil(float(r) * n)      # attn_blocks.py:39
        out.append(n)
    return out


def template_rows(template_range, feat_sz_z):
    """generate_mask_cond (lib/utils/ce_utils.py:15-49) for one sample: a bool vector of feat_sz_z ** 2, None for ALL."""
    if template_range == "ALL":
        return None
    sl = {"CTR_POINT": {8: slice(3, 4), 12: slice(5, 6)}, "CTR_REC": {8: slice(3, 5), 12: slice(5, 7)}}[template_range][feat_sz_z]
    m = torch.zeros(feat_sz_z, feat_sz_z)
    m[sl, sl] = 1
    return m.flatten().to(torch.bool)


def _attention(attn, xn):
    """vit.py:51-66 / attn.py:33-57: (projected output, attention weights (B, heads, N, N))."""
    B, N, C = xn.shape
    qkv = attn.qkv(xn).reshape(B, N, 3, attn.heads, C // attn.heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a = ((q @ k.transpose(-2, -1)) * attn.scale).softmax(dim=-1)
    return attn.proj((a @ v).transpose(1, 2).reshape(B, N, C)), a


def forward(model: ob.OracleOSTrack, template, search, ce_loc, ce_keep_ratio, rows=None, forced=None):
    """-> dict: the four output maps / boxes, 'feat' (B, Lx, C) the backbone's search rows (zeros where removed), and per stage (lists,
    no-op stages skipped as the reference's early return skips them) 'keep' / 'removed' (B, n) ascending global search indices and
    'scores' (B, Lx) the stage's attn_t at global positions, NaN for tokens removed earlier."""
    bb = model.backbone
    with torch.no_grad():
        x = bb.patch_embed(search) + bb.pos_embed_x
        z = bb.patch_embed(template) + bb.pos_embed_z
        t = torch.cat((z, x), dim=1)
        B, lz, lx = t.shape[0], z.shape[1], x.shape[1]
        gi = torch.arange(lx).repeat(B, 1)                                     # global index of each search token still there
        keep_l, removed_l, scores_l = [], [], []
        stage = 0
        ce_loc = [int(v) for v in ce_loc]
        for i, blk in enumerate(bb.blocks):
            xo, a = _attention(blk.attn, blk.norm1(t))
            t = t + xo
            if i in ce_loc:
                ratio = float(ce_keep_ratio[ce_loc.index(i)])
                lens_s = t.shape[1] - lz
                keep = math.ceil(ratio * lens_s)
                if keep != lens_s:
                    at = a[:, :, :lz, lz:]
                    if rows is not None:
                        at = at[:, :, rows, :]
                    score = at.mean(dim=2).mean(dim=1)                         # (B, lens_s)
                    full = torch.full((B, lx), float("nan"))
                    full.scatter_(1, gi, score)
                    if forced is not None:
                        want = torch.as_tensor(np.asarray(forced[stage]), dtype=torch.int64)
                        assert tuple(want.shape) == (B, keep), (tuple(want.shape), (B, keep))
                        member = torch.zeros(B, lx, dtype=torch.bool).scatter_(1, want, True)
                        sel = member.gather(1, gi)                             # which of the present tokens are kept
                        assert bool((sel.sum(1) == keep).all()), "a forced keep set names a token that was removed earlier"
                    else:
                        order = torch.sort(score, dim=1, descending=True, stable=True).indices      # ties: the lower index
                        sel = torch.zeros(B, lens_s, dtype=torch.bool).scatter_(1, order[:, :keep], True)
                    pos = torch.sort((~sel).to(torch.uint8), dim=1, stable=True).indices             # kept first, both in index order
                    kp, rm = pos[:, :keep], pos[:, keep:]
                    keep_l.append(gi.gather(1, kp))
                    removed_l.append(gi.gather(1, rm))
                    scores_l.append(full)
                    ts = t[:, lz:]
                    t = torch.cat([t[:, :lz], ts.gather(1, kp.unsqueeze(-1).expand(B, -1, ts.shape[-1]))], dim=1)
                    gi = gi.gather(1, kp)
                    stage += 1
            t = t + blk.mlp(blk.norm2(t))
        t = bb.norm(t)
        C = t.shape[-1]
        feat = torch.zeros(B, lx, C).scatter_(1, gi.unsqueeze(-1).expand(B, -1, C), t[:, lz:])       # vit_ce.py:170-181
        F = model.feat_sz
        score, bbox, size, offset = model.box_head(feat.transpose(1, 2).reshape(B, C, F, F).contiguous())
    return {"pred_boxes": bbox.view(B, 1, 4), "score_map": score, "size_map": size, "offset_map": offset, "feat": feat,
            "keep": keep_l, "removed": removed_l, "scores": scores_l}
