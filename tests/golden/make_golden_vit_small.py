#!/usr/bin/env python3
"""Golden vectors for the small patch-16 OSTrack models -- ViT-Small (width 384, 6 heads) and ViT-Tiny (width 192, 3 heads), MLP 4 x width
-- at both geometries, produced by the REFERENCE's own classes.

    python tests/golden/make_golden_vit_small.py [plain] [search]     # build container only; no argument = both

The reference is imported as make_golden_vitb.py imports it.  Its ``build_ostrack`` knows no such TYPE and its ``build_small_ostrack``
reads a pretrain path, so the model is put together from the classes those builders use (lib/models/ostrack/ostrack.py:288-342):

    backbone = lib.models.ostrack.vit.VisionTransformer(patch_size=16, embed_dim=C, depth=d, num_heads=h)
    backbone.finetune_track(cfg=cfg, patch_start_index=1)
    net = OSTrack(backbone, build_box_head(cfg, C), aux_loss=False, head_type="CENTER").eval()

Weights are ``synth.synth_vitb_state_dict(seed, C, depth, heads, len_z, len_x)``: no missing and no unexpected key (asserted).

A fixture is a SELECTION of samples of one seed's 16-sample pool (``synth_inputs(seed, 16, TZ, TX)``; ``rows``).  MARGIN RULE: every sample
in ``rows`` has a raw AND a Hann-windowed top-2 score margin above 0.03 -- the ViT-Base rule, unscaled: depth <= 12 and the bf16 error law
TOL_REL(n) = 2e-3 sqrt(n) of tests/test_gpu_vitb.py does not depend on the width.  Asserted when a file is written; the tests excuse no
argmax flip.  File names (``ref_vits_*``, ``ref_vitt_*`` at 128 / 256; ``ref_vs384_*``, ``ref_vt384_*`` at 192 / 384) match no glob of
tests/conftest.py.

``plain``: the table PLAIN below -- maps, boxes, Hann boxes, conf, margins; where activations are kept, the geometry's token rows
(``make_golden_vitb.ACT_ROWS`` / ``make_golden_vitb384.ACT_ROWS``) of the first of ``rows`` entering block 0, leaving blocks 0, 5, 11
(depth 3: 0, 2) and the final norm.  The 192 / 384 fixtures are depth 3: what ``build_small_ostrack`` builds.

``search``: one walk over the seeds [600, 640) at ViT-Small, 128 / 256, depth 12, for a uint8 fixture (``ref_vits_u8_s<seed>.npz``: the first
seed with two qualifying samples of ``synth_patches(seed, 16, 256)``) and a tracking fixture (``ref_vits_track_s<seed>.npz``: 2 sequences x 4
frames, all eight Hann margins above the rule), by make_golden_vitl.py's recipe.  When the range yields none this script says so and those
routes are tested by their exactness properties."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_vitb as mv  # noqa: E402
import make_golden_vitb384 as m384  # noqa: E402

from vittracker_amd import synth  # noqa: E402

MARGIN = 0.03
NPOOL = 16
WIDTHS = {"vits": (384, 6), "vitt": (192, 3)}
GEO = {256: dict(TZ=128, TX=256, LZ=64, LX=256, F=16, act_rows=mv.ACT_ROWS), 384: dict(TZ=192, TX=384, LZ=144, LX=576, F=24, act_rows=m384.ACT_ROWS)}
ACT_BLOCKS = {12: (0, 5, 11), 3: (0, 2)}
#: file, model, geometry, depth, seed, rows, activations of the first row
PLAIN = (("ref_vits_s502.npz", "vits", 256, 12, 502, [1, 3, 6, 7], True),
         ("ref_vits_s503.npz", "vits", 256, 12, 503, [1, 9, 10, 15], False),
         ("ref_vitt_s524.npz", "vitt", 256, 12, 524, [4, 8, 9, 14], True),
         ("ref_vitt_s527.npz", "vitt", 256, 12, 527, [1, 9, 14, 15], False),
         ("ref_vs384_s562.npz", "vits", 384, 3, 562, [0, 1, 5], True),
         ("ref_vt384_s541.npz", "vitt", 384, 3, 541, [1, 3, 6], True))
SEARCH_SEEDS = range(600, 640)
top2 = m384.top2


def build_reference(ostrack, config, model, geo, depth):
    C, heads = WIDTHS[model]
    g = GEO[geo]
    cfg = config.cfg
    cfg.MODEL.HEAD.TYPE, cfg.MODEL.HEAD.NUM_CHANNELS = "CENTER", 256
    cfg.MODEL.BACKBONE.STRIDE = 16
    cfg.DATA.SEARCH.SIZE, cfg.DATA.TEMPLATE.SIZE = g["TX"], g["TZ"]
    cfg.TEST.SEARCH_SIZE, cfg.TEST.TEMPLATE_SIZE = g["TX"], g["TZ"]
    vit = sys.modules["lib.models.ostrack.vit"]
    backbone = vit.VisionTransformer(patch_size=16, embed_dim=C, depth=depth, num_heads=heads)
    backbone.finetune_track(cfg=cfg, patch_start_index=1)
    box_head = sys.modules["lib.models.layers.head"].build_box_head(cfg, C)
    return ostrack.OSTrack(backbone, box_head, aux_loss=False, head_type="CENTER").eval()


def load_net(ostrack, config, model, geo, depth, seed):
    C, heads = WIDTHS[model]
    g = GEO[geo]
    net = build_reference(ostrack, config, model, geo, depth)
    sd = synth.synth_vitb_state_dict(seed, C=C, depth=depth, heads=heads, len_z=g["LZ"], len_x=g["LX"])
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    assert net.box_head.feat_sz == g["F"] and len(net.backbone.blocks) == depth and net.backbone.norm.weight.shape[0] == C
    return net, sd


def forward(net, hann_mod, z, x, acts=None, depth=12):
    """make_golden_vitb384.forward with this file's activation blocks."""
    hooks = []
    if acts is not None:
        def grab(name, inp=False):
            return lambda _m, i, o: acts.__setitem__(name, (i[0] if inp else o).detach().clone().numpy())
        hooks.append(net.backbone.blocks[0].register_forward_hook(grab("tokens", inp=True)))
        for i in ACT_BLOCKS[depth]:
            hooks.append(net.backbone.blocks[i].register_forward_hook(grab(f"block{i}")))
        hooks.append(net.backbone.norm.register_forward_hook(grab("norm")))
    try:
        return m384.forward(net, hann_mod, z, x)
    finally:
        for h in hooks:
            h.remove()


def run_plain(ostrack, config, hann_mod, model, geo, depth, seed, rows, with_acts):
    g = GEO[geo]
    net, sd = load_net(ostrack, config, model, geo, depth, seed)
    z, x = synth.synth_inputs(seed, NPOOL, g["TZ"], g["TX"])
    acts = {} if with_acts else None
    res = forward(net, hann_mod, torch.from_numpy(z[rows]), torch.from_numpy(x[rows]), acts, depth)
    assert min(res["margin_raw"].min(), res["margin_hann"].min()) > MARGIN, (seed, rows, res["margin_raw"], res["margin_hann"])
    res.update({"model": model + ("384" if geo == 384 else ""), "channels": WIDTHS[model][0], "heads": WIDTHS[model][1], "depth": depth, "seed": seed,
                "pool": NPOOL, "rows": np.array(rows), "B": len(rows), "state_checksum": synth.state_checksum(sd)})
    if with_acts:
        res["act_rows"] = np.array(g["act_rows"])
        for k, v in acts.items():
            res["act_" + k] = v[:1, g["act_rows"]].astype(np.float32)      # the first of `rows`, selected token rows, every channel
    return res


def search(ostrack, config, hann_mod):
    """make_golden_vitl.py's search at ViT-Small: its run_u8 / run_track with this file's margin and model."""
    import make_golden_vitl as ml
    box_ops = sys.modules["lib.utils.box_ops"]
    ml.MARGIN = MARGIN
    ml.forward = lambda net, hm, z, x, acts=None: forward(net, hm, z, x, acts, 12)
    ml.GEO[256] = dict(ml.GEO[256], model="vits")
    need_u8, need_track = True, True
    for seed in SEARCH_SEEDS:
        if not (need_u8 or need_track):
            break
        net, sd = load_net(ostrack, config, "vits", 256, 12, seed)
        if need_u8:
            res = ml.run_u8(net, sd, hann_mod, seed)
            if res is not None:
                np.savez_compressed(os.path.join(HERE, f"ref_vits_u8_s{seed}.npz"), **res)
                print(f"ref_vits_u8_s{seed}.npz: rows {res['rows'].tolist()} margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)}", flush=True)
                need_u8 = False
        if need_track:
            res = ml.run_track(net, sd, box_ops, hann_mod, seed)
            if res is not None:
                np.savez_compressed(os.path.join(HERE, f"ref_vits_track_s{seed}.npz"), **res)
                print(f"ref_vits_track_s{seed}.npz: hann margins {np.round(res['margin_hann'].reshape(-1), 4)}", flush=True)
                need_track = False
    if need_u8:
        print(f"u8: no seed in [{SEARCH_SEEDS.start}, {SEARCH_SEEDS.stop}) yields two samples above {MARGIN}: no uint8 fixture; the uint8 route is "
              "tested by its agreement with vt_forward on the normalised patch")
    if need_track:
        print(f"track: no seed in [{SEARCH_SEEDS.start}, {SEARCH_SEEDS.stop}) keeps all eight margins above {MARGIN}: no tracking fixture")


def main():
    torch.manual_seed(0)
    ostrack, config, hann_mod = mv.import_reference_ostrack()
    what = sys.argv[1:] or ["plain", "search"]
    if "plain" in what:
        for name, model, geo, depth, seed, rows, with_acts in PLAIN:
            res = run_plain(ostrack, config, hann_mod, model, geo, depth, seed, rows, with_acts)
            np.savez_compressed(os.path.join(HERE, name), **res)
            print(f"{name}: rows {rows} margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)}", flush=True)
    if "search" in what:
        search(ostrack, config, hann_mod)


if __name__ == "__main__":
    main()
