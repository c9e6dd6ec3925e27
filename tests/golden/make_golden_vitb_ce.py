#!/usr/bin/env python3
"""Golden vectors for the candidate-elimination ViT-Base OSTrack (``MODEL.BACKBONE.TYPE: vit_base_patch16_224_ce``), produced by the
REFERENCE's own code.

    python tests/golden/make_golden_vitb_ce.py          # writes tests/golden/ref_vbce_*.npz   (build container only)

What runs: ``lib/models/ostrack/ostrack.py::build_ostrack(cfg, training=False)`` with the reference's real ``lib/models/ostrack/vit_ce.py``
(``VisionTransformerCE``), ``lib/models/layers/attn_blocks.py`` (``CEBlock``, ``candidate_elimination``), ``lib/models/layers/attn.py``
(``Attention``) and ``lib/utils/ce_utils.py::generate_mask_cond`` (the ``ce_template_mask`` the reference's tracker passes,
``lib/test/tracker/ostrack.py:57-62``), loaded from the reference tree under make_golden_vitb.py's stand-ins.  Two more stand-ins:
``lib.models.layers.rpe`` (``attn.py`` imports one name from it that ``rpe=False`` never calls), and the depth: ``build_ostrack`` calls
``vit_base_patch16_224_ce(...)`` with its default depth 12; for the two shallow cases the name it calls is bound to the same function with
``depth=`` given (``vit_ce.py:220`` takes it as a keyword).

Cases (weights ``synth_vitb_state_dict(seed, depth, len_z, len_x)``, CE_KEEP_RATIO 0.7 at every stage).  The files are ``ref_vbce_*``, not
``ref_vitb_ce_*``: ``conftest.vitb_golden_files`` globs ``ref_vitb_*`` for the plain-model tests.

  ref_vbce_256_s<seed>.npz    the published configuration: depth 12, CE_LOC [3, 6, 9], CTR_POINT, 128 / 256, B = 2.  The search crop is
                              ``Preprocessor.process`` of ``synth_patches(seed, 2, 256)`` (make_golden_u8.preprocess), so the same
                              fixture serves the fp32 and the uint8 entry points; the template crops are ``synth_inputs(seed, 2, ..)[0]``.
  ref_vbce_384_s<seed>.npz    the same at 192 / 384: ``rows`` = 2 samples of the seed's 16-sample ``synth_inputs`` pool (make_golden_vitb384.py).
  ref_vbce_d5_s<seed>.npz     depth 5, CE_LOC [1, 2, 3], CTR_REC, 128 / 256, B = 3, ``synth_inputs(seed, 3, 128, 256)``.
  ref_vbce_d3_s<seed>.npz     depth 3, CE_LOC [0, 1], ALL, 128 / 256, B = 2, ``synth_inputs(seed, 2, 128, 256)``.

Seeds are searched, as the other generators do, for samples whose raw and Hann-windowed top-2 margins all exceed 0.03.  Stored: the
outputs, the backbone's search rows ``feat`` every 8th channel, per stage the kept and removed GLOBAL search indices (ascending) and the
``attn_t`` scores at global positions (NaN for tokens removed earlier; taken from the attention weights the blocks return, masked and
averaged as ``attn_blocks.py:43-56`` does), the margins and the state checksum."""
from __future__ import annotations

import functools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_vitb as mv  # noqa: E402
from make_golden_u8 import preprocess  # noqa: E402

from vittracker_amd import synth  # noqa: E402

MARGIN = 0.03
NPOOL = 16
CASES = {      # name -> template, search, depth, CE_LOC, CE_TEMPLATE_RANGE, B, input kind, first seed of the search
    "256": (128, 256, 12, [3, 6, 9], "CTR_POINT", 2, "u8", 300),
    "384": (192, 384, 12, [3, 6, 9], "CTR_POINT", 2, "pool", 320),
    "d5": (128, 256, 5, [1, 2, 3], "CTR_REC", 3, "f32", 340),
    "d3": (128, 256, 3, [0, 1], "ALL", 2, "f32", 360),
}
RATIO = 0.7


def import_reference_ce():
    ostrack, config, hann = mv.import_reference_ostrack()
    rpe = types.ModuleType("lib.models.layers.rpe")
    rpe.generate_2d_concatenated_self_attention_relative_positional_encoding_index = None      # only called when rpe=True
    sys.modules["lib.models.layers.rpe"] = rpe
    mg._load("lib.models.layers.attn", "lib/models/layers/attn.py")
    mg._load("lib.models.layers.attn_blocks", "lib/models/layers/attn_blocks.py")
    vit_ce = mg._load("lib.models.ostrack.vit_ce", "lib/models/ostrack/vit_ce.py")
    mg._pkg("lib.utils")
    ce_utils = mg._load("lib.utils.ce_utils", "lib/utils/ce_utils.py")
    return ostrack, config, hann, vit_ce, ce_utils


def build(ostrack, config, vit_ce, tz, tx, depth, loc, trange):
    cfg = config.cfg
    cfg.MODEL.BACKBONE.TYPE = "vit_base_patch16_224_ce"
    cfg.MODEL.BACKBONE.CE_LOC, cfg.MODEL.BACKBONE.CE_KEEP_RATIO = list(loc), [RATIO] * len(loc)
    cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE = trange
    cfg.MODEL.HEAD.TYPE, cfg.MODEL.HEAD.NUM_CHANNELS = "CENTER", 256
    cfg.DATA.SEARCH.SIZE, cfg.DATA.TEMPLATE.SIZE = tx, tz
    cfg.TEST.SEARCH_SIZE, cfg.TEST.TEMPLATE_SIZE = tx, tz
    ostrack.vit_base_patch16_224_ce = functools.partial(vit_ce.vit_base_patch16_224_ce, depth=depth)
    net = ostrack.build_ostrack(cfg, training=False).eval()
    assert len(net.backbone.blocks) == depth and type(net.backbone).__name__ == "VisionTransformerCE"
    return net, cfg


def top2(m, B):
    srt = np.sort(np.asarray(m).reshape(B, -1), axis=1)
    return srt[:, -1] - srt[:, -2]


def run(net, cfg, hann_mod, ce_utils, z, x, loc):
    """The reference forward on (z, x) with generate_mask_cond's mask; outputs and the per-stage record."""
    B, lz = z.shape[0], net.backbone.pos_embed_z.shape[1]
    lx = net.backbone.pos_embed_x.shape[1]
    mask = ce_utils.generate_mask_cond(cfg, B, z.device, None)
    attns = {}
    hooks = [net.backbone.blocks[i].register_forward_hook(lambda _m, _i, o, i=i: attns.__setitem__(i, o[4].detach().clone())) for i in loc]
    with torch.no_grad():
        out = net(template=z, search=x, ce_template_mask=mask)
        F = net.box_head.feat_sz
        win = hann_mod.hann2d(torch.tensor([F, F]).long(), centered=True)
        hbox = net.box_head.cal_bbox(win * out["score_map"], out["size_map"], out["offset_map"])
        conf = out["score_map"].flatten(1).max(dim=1).values
    for h in hooks:
        h.remove()
    res = {"margin_raw": top2(out["score_map"].numpy(), B), "margin_hann": top2((win * out["score_map"]).numpy(), B),
           "score_map": out["score_map"].numpy(), "size_map": out["size_map"].numpy(), "offset_map": out["offset_map"].numpy(),
           "pred_boxes": out["pred_boxes"].numpy(), "hann_boxes": hbox.numpy(), "conf": conf.numpy(),
           "feat": out["backbone_feat"][:, lz:, ::8].numpy().astype(np.float32)}
    present = torch.arange(lx).repeat(B, 1)                    # global indices in the order the reference holds them
    for k, i in enumerate(loc):
        rem = out["removed_indexes_s"][k].to(torch.int64)      # descending score, as floats
        a = attns[i][:, :, :lz, lz:]                           # attn_blocks.py:43-56
        if mask is not None:
            a = a[mask.unsqueeze(1).unsqueeze(-1).expand(-1, a.shape[1], -1, a.shape[-1])].view(B, a.shape[1], -1, a.shape[-1])
        score = a.mean(dim=2).mean(dim=1)
        full = torch.full((B, lx), float("nan")).scatter_(1, present, score)
        order = torch.sort(score, dim=1, descending=True).indices
        keep_n = present.shape[1] - rem.shape[1]
        assert torch.equal(present.gather(1, order[:, keep_n:]), rem), "the hook's scores do not reproduce the reference's removal"
        present = present.gather(1, order[:, :keep_n])
        res[f"keep{k}"] = np.sort(present.numpy(), axis=1)
        res[f"removed{k}"] = np.sort(rem.numpy(), axis=1)
        res[f"scores{k}"] = full.numpy()
    return res


def case(name, ostrack, config, hann_mod, vit_ce, ce_utils):
    tz, tx, depth, loc, trange, B, kind, seed = CASES[name]
    lz, lx = (tz // 16) ** 2, (tx // 16) ** 2
    net, cfg = build(ostrack, config, vit_ce, tz, tx, depth, loc, trange)
    while True:
        sd = synth.synth_vitb_state_dict(seed, depth=depth, len_z=lz, len_x=lx)
        missing, unexpected = net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        extra = {}
        if kind == "pool":
            z, x = synth.synth_inputs(seed, NPOOL, tz, tx)
            probe = run(net, cfg, hann_mod, ce_utils, torch.from_numpy(z), torch.from_numpy(x), loc)
            ok = [i for i in range(NPOOL) if min(probe["margin_raw"][i], probe["margin_hann"][i]) > MARGIN]
            print(f"{name} seed {seed}: qualifying samples {ok}")
            if len(ok) < B:
                seed += 1
                continue
            rows = ok[:B]
            z, x = torch.from_numpy(z[rows]), torch.from_numpy(x[rows])
            extra = {"pool": NPOOL, "rows": np.array(rows)}
        elif kind == "u8":
            patches = synth.synth_patches(seed, B, tx)
            z, x = torch.from_numpy(synth.synth_inputs(seed, B, tz, tx)[0]), preprocess(patches)
            extra = {"u8": 1, "patch_checksum": int(patches.astype(np.uint64).sum())}
        else:
            z, x = (torch.from_numpy(a) for a in synth.synth_inputs(seed, B, tz, tx))
        res = run(net, cfg, hann_mod, ce_utils, z, x, loc)
        ok = min(res["margin_raw"].min(), res["margin_hann"].min()) > MARGIN
        print(f"{name} seed {seed}: margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)} -> {'keep' if ok else 'skip'}")
        if ok:
            break
        seed += 1
    res.update(extra)
    res.update({"model": "vitb_ce", "case": name, "seed": seed, "B": B, "template_size": tz, "search_size": tx, "depth": depth,
                "ce_loc": np.array(loc), "ce_keep_ratio": np.array([RATIO] * len(loc)), "ce_template_range": trange,
                "state_checksum": synth.state_checksum(sd)})
    fn = f"ref_vbce_{name}_s{seed}.npz"
    np.savez_compressed(os.path.join(HERE, fn), **res)
    print(f"{fn}: kept {[res[f'keep{k}'].shape[1] for k in range(len(loc))]}, {os.path.getsize(os.path.join(HERE, fn))} bytes")


def main():
    torch.manual_seed(0)
    mods = import_reference_ce()
    ostrack, config, hann_mod, vit_ce, ce_utils = mods
    for name in (sys.argv[1:] or list(CASES)):
        case(name, ostrack, config, hann_mod, vit_ce, ce_utils)


if __name__ == "__main__":
    main()
