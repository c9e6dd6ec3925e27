#!/usr/bin/env python3
"""Golden vectors for the ViT-Large OSTrack path (width 1024, 16 heads, depth 24, MLP 4096) at both geometries, produced by the
REFERENCE's own code.

    python tests/golden/make_golden_vitl.py [plain256] [plain384] [search]     # build container only; no argument = all three

The reference is imported exactly as make_golden_vitb.py imports it (its loader and stand-ins are reused) and the recipe is
make_golden_vitb384.py's, with three differences:

* ``cfg.MODEL.BACKBONE.TYPE = "vit_large_patch16_224"`` and ``cfg.MODEL.PRETRAIN_FILE = ""``: the reference's ``build_ostrack`` joins the
  pretrain path unconditionally for this TYPE, and with the config's default file name ``torch.load`` fails on a missing file; with the
  empty string no load happens (the reference then builds a 311.9 M-parameter model).
* weights are ``synth.synth_vitb_state_dict(seed, C=1024, depth=24, heads=16[, len_z=144, len_x=576])``: no missing or unexpected key.
* file names are ``ref_vitl_*`` (128 / 256) and ``ref_vl384_*`` (192 / 384), which tests/conftest.py's ``ref_vitb_*`` / ``ref_vb384_*``
  globs do not match.

A fixture is a SELECTION of samples of one seed's 16-sample pool (``synth_inputs(seed, 16, .., ..)``; ``rows`` = the samples the
reference was run on).  MARGIN RULE: every sample in ``rows`` has a raw AND a Hann-windowed top-2 score margin above 0.045 -- the
ViT-Base rule of 0.03 scaled by sqrt(24 / 12), the growth of the bf16 error law TOL_REL(n) = 2e-3 sqrt(n) (tests/test_gpu_vitb.py) from
12 to 24 blocks.  Asserted here when a file is written; the tests excuse no argmax flip.

1. ``ref_vitl_s206.npz`` (rows 0, 1, 5, 7; activations of row 0) and ``ref_vitl_s209.npz`` (rows 0, 2, 7, 8): maps, boxes, Hann boxes,
   conf, margins.  Activations: the token rows ``make_golden_vitb.ACT_ROWS`` entering block 0 and leaving blocks 0, 5, 11, 12, 23 and the
   final norm.
2. ``ref_vl384_s206.npz`` (rows 3, 4, 6, 8; activations of row 3, token rows ``make_golden_vitb384.ACT_ROWS``) and ``ref_vl384_s207.npz``
   (rows 5, 13, 14).
3. ``search``: one walk over the seeds [270, 310), weights synthesised once per seed, for
   ``ref_vitl_u8_s<seed>.npz``     make_golden_ostrack_u8.py's recipe at 128 / 256 on ``synth_patches(seed, 16, 256)``: the first seed with at
                                   least two qualifying samples (at most 3 kept; token rows of the first two).  When the range has none this
                                   script says so, and the uint8 route is tested by its agreement with vt_forward on the normalised patch.
   ``ref_vitl_track_s<seed>.npz``  2 synthetic sequences x 4 tracked frames at factors 2.0 / 4.0: the first seed whose eight Hann margins
                                   all exceed the rule; not written when there is none (the step is then tested by its exactness properties)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_vitb as mv  # noqa: E402
import make_golden_vitb384 as m384  # noqa: E402
from make_golden_u8 import preprocess  # noqa: E402

from vittracker_amd import host_ops, synth  # noqa: E402
from vittracker_amd.evaluation.data import synthetic_sequence  # noqa: E402

MARGIN = 0.045                   # 0.03 sqrt(24 / 12), rounded up
C, HEADS, DEPTH = 1024, 16, 24
NPOOL = 16
ACT_BLOCKS = (0, 5, 11, 12, 23)
GEO = {256: dict(TZ=128, TX=256, LZ=64, LX=256, F=16, act_rows=mv.ACT_ROWS, prefix="ref_vitl", model="vitl"),
       384: dict(TZ=192, TX=384, LZ=144, LX=576, F=24, act_rows=m384.ACT_ROWS, prefix="ref_vl384", model="vitl384")}
PLAIN = {256: ((206, [0, 1, 5, 7], True), (209, [0, 2, 7, 8], False)),
         384: ((206, [3, 4, 6, 8], True), (207, [5, 13, 14], False))}
SEARCH_SEEDS = range(270, 310)
N_SEQ, N_FRAMES, TEMPLATE_FACTOR, SEARCH_FACTOR = 2, 4, 2.0, 4.0
top2 = m384.top2


def build_reference_vitl(ostrack, config, g):
    cfg = config.cfg
    cfg.MODEL.BACKBONE.TYPE = "vit_large_patch16_224"
    cfg.MODEL.PRETRAIN_FILE = ""
    cfg.MODEL.HEAD.TYPE, cfg.MODEL.HEAD.NUM_CHANNELS = "CENTER", 256
    cfg.DATA.SEARCH.SIZE, cfg.DATA.TEMPLATE.SIZE = g["TX"], g["TZ"]
    cfg.TEST.SEARCH_SIZE, cfg.TEST.TEMPLATE_SIZE = g["TX"], g["TZ"]
    return ostrack.build_ostrack(cfg, training=False).eval()


def load_net(ostrack, config, g, seed):
    net = build_reference_vitl(ostrack, config, g)
    sd = synth.synth_vitb_state_dict(seed, C=C, depth=DEPTH, heads=HEADS, len_z=g["LZ"], len_x=g["LX"])
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    assert net.box_head.feat_sz == g["F"] and len(net.backbone.blocks) == DEPTH and net.backbone.norm.weight.shape[0] == C
    return net, sd


def forward(net, hann_mod, z, x, acts=None):
    """make_golden_vitb384.forward with this file's ACT_BLOCKS."""
    hooks = []
    if acts is not None:
        def grab(name, inp=False):
            return lambda _m, i, o: acts.__setitem__(name, (i[0] if inp else o).detach().clone().numpy())
        hooks.append(net.backbone.blocks[0].register_forward_hook(grab("tokens", inp=True)))
        for i in ACT_BLOCKS:
            hooks.append(net.backbone.blocks[i].register_forward_hook(grab(f"block{i}")))
        hooks.append(net.backbone.norm.register_forward_hook(grab("norm")))
    try:
        return m384.forward(net, hann_mod, z, x)
    finally:
        for h in hooks:
            h.remove()


def run_plain(ostrack, config, hann_mod, geo, seed, rows, with_acts):
    g = GEO[geo]
    net, sd = load_net(ostrack, config, g, seed)
    z, x = synth.synth_inputs(seed, NPOOL, g["TZ"], g["TX"])
    acts = {} if with_acts else None
    res = forward(net, hann_mod, torch.from_numpy(z[rows]), torch.from_numpy(x[rows]), acts)
    assert min(res["margin_raw"].min(), res["margin_hann"].min()) > MARGIN, (seed, rows, res["margin_raw"], res["margin_hann"])
    res.update({"model": g["model"], "seed": seed, "pool": NPOOL, "rows": np.array(rows), "B": len(rows), "state_checksum": synth.state_checksum(sd)})
    if with_acts:
        res["act_rows"] = np.array(g["act_rows"])
        for k, v in acts.items():
            res["act_" + k] = v[:1, g["act_rows"]].astype(np.float32)      # the first of `rows`, selected token rows, all 1024 channels
    return res


def run_u8(net, sd, hann_mod, seed):
    g = GEO[256]
    z = synth.synth_inputs(seed, NPOOL, g["TZ"], g["TX"])[0]
    patches = synth.synth_patches(seed, NPOOL, g["TX"])
    x = preprocess(patches)
    probe = forward(net, hann_mod, torch.from_numpy(z), x)
    ok = [i for i in range(NPOOL) if min(probe["margin_raw"][i], probe["margin_hann"][i]) > MARGIN]
    print(f"u8 seed {seed}: qualifying samples {ok}", flush=True)
    if len(ok) < 2:
        return None
    rows = ok[:3]
    acts = {}
    res = forward(net, hann_mod, torch.from_numpy(z[rows]), x[rows], acts)
    assert min(res["margin_raw"].min(), res["margin_hann"].min()) > MARGIN
    res.update({"model": g["model"], "seed": seed, "pool": NPOOL, "rows": np.array(rows), "B": len(rows), "state_checksum": synth.state_checksum(sd),
                "patch_checksum": int(patches.astype(np.uint64).sum()), "act_rows": np.array(g["act_rows"]),
                "act_tokens": acts["tokens"][:2, g["act_rows"]].astype(np.float32)})
    return res


def seq_seed(seed, q):
    return 1000 * seed + q


def run_track(net, sd, box_ops, hann_mod, seed):
    """make_golden_vitb384.run_track at 128 / 256 and factors 2.0 / 4.0; None as soon as a frame's Hann margin is below the rule."""
    g = GEO[256]
    TZ, TX, F = g["TZ"], g["TX"], g["F"]
    win = hann_mod.hann2d(torch.tensor([F, F]).long(), centered=True)
    keys = ("state_before", "box_after", "conf", "resize_factor", "margin_hann")
    rec = {k: [] for k in keys}
    for q in range(N_SEQ):
        seq = synthetic_sequence(f"track_{q}", N_FRAMES + 1, seed=seq_seed(seed, q))
        state = [float(v) for v in seq.ground_truth_rect[0]]
        z_arr, _, _ = host_ops.sample_target(seq.frames[0], state, TEMPLATE_FACTOR, output_sz=TZ)
        z = preprocess(z_arr[None])
        for t in range(1, N_FRAMES + 1):
            frame = seq.frames[t]
            H, W, _ = frame.shape
            x_arr, rf, _ = host_ops.sample_target(frame, state, SEARCH_FACTOR, output_sz=TX)
            with torch.no_grad():
                out = net(template=z, search=preprocess(x_arr[None]))
                resp = win * out["score_map"]
                pred_boxes = net.box_head.cal_bbox(resp, out["size_map"], out["offset_map"]).view(-1, 4)
                conf = float(out["score_map"].flatten(1).max(dim=1).values[0])
            margin = float(top2(resp.numpy(), 1)[0])
            if margin <= MARGIN:
                print(f"track seed {seed}: sequence {q} frame {t} margin {margin:.4f} -> skip", flush=True)
                return None
            pred_box = (pred_boxes.mean(dim=0) * TX / rf).tolist()
            cx_prev, cy_prev = state[0] + 0.5 * state[2], state[1] + 0.5 * state[3]
            cx, cy, w, h = pred_box
            half_side = 0.5 * TX / rf
            mapped = [cx + (cx_prev - half_side) - 0.5 * w, cy + (cy_prev - half_side) - 0.5 * h, w, h]
            new = [float(v) for v in box_ops.clip_box(mapped, H, W, margin=10)]
            for k, v in zip(keys, (state, new, conf, rf, margin)):
                rec[k].append(v)
            state = new
    res = {k: np.asarray(v, np.float64).reshape(N_SEQ, N_FRAMES, -1).squeeze(-1) if k not in ("state_before", "box_after")
           else np.asarray(v, np.float64).reshape(N_SEQ, N_FRAMES, 4) for k, v in rec.items()}
    res.update({"model": g["model"], "seed": seed, "seq_seeds": np.array([seq_seed(seed, q) for q in range(N_SEQ)]), "n_frames": N_FRAMES,
                "template_factor": TEMPLATE_FACTOR, "search_factor": SEARCH_FACTOR, "state_checksum": synth.state_checksum(sd)})
    return res


def main():
    torch.manual_seed(0)
    ostrack, config, hann_mod = mv.import_reference_ostrack()
    box_ops = sys.modules["lib.utils.box_ops"]
    what = sys.argv[1:] or ["plain256", "plain384", "search"]
    for geo in (256, 384):
        if f"plain{geo}" not in what:
            continue
        for seed, rows, with_acts in PLAIN[geo]:
            res = run_plain(ostrack, config, hann_mod, geo, seed, rows, with_acts)
            name = f"{GEO[geo]['prefix']}_s{seed}.npz"
            np.savez_compressed(os.path.join(HERE, name), **res)
            print(f"{name}: rows {rows} margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)}", flush=True)
    if "search" in what:
        need_u8, need_track = True, True
        for seed in SEARCH_SEEDS:
            if not (need_u8 or need_track):
                break
            net, sd = load_net(ostrack, config, GEO[256], seed)
            if need_u8:
                res = run_u8(net, sd, hann_mod, seed)
                if res is not None:
                    np.savez_compressed(os.path.join(HERE, f"ref_vitl_u8_s{seed}.npz"), **res)
                    print(f"ref_vitl_u8_s{seed}.npz: rows {res['rows'].tolist()} margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)}",
                          flush=True)
                    need_u8 = False
            if need_track:
                res = run_track(net, sd, box_ops, hann_mod, seed)
                if res is not None:
                    np.savez_compressed(os.path.join(HERE, f"ref_vitl_track_s{seed}.npz"), **res)
                    print(f"ref_vitl_track_s{seed}.npz: hann margins {np.round(res['margin_hann'].reshape(-1), 4)}", flush=True)
                    need_track = False
        if need_u8:
            print(f"u8: no seed in [{SEARCH_SEEDS.start}, {SEARCH_SEEDS.stop}) yields two samples above {MARGIN}: no uint8 fixture; the uint8 route is "
                  "tested by its agreement with vt_forward on the normalised patch")
        if need_track:
            print(f"track: no seed in [{SEARCH_SEEDS.start}, {SEARCH_SEEDS.stop}) keeps all eight margins above {MARGIN}: no tracking fixture")


if __name__ == "__main__":
    main()
