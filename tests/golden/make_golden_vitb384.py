#!/usr/bin/env python3
"""Golden vectors for the ViT-Base OSTrack path at the 384 geometry (192 px template / 384 px search: 144 + 576 = 720 tokens, 24 x 24
maps), produced by the REFERENCE's own code.

    python tests/golden/make_golden_vitb384.py          # writes tests/golden/ref_vb384_*.npz   (build container only)

The reference is imported exactly as make_golden_vitb.py imports it (its loader and stand-ins are reused); what differs is
``DATA.SEARCH.SIZE = 384``, ``DATA.TEMPLATE.SIZE = 192`` in the config ``build_ostrack`` is built from.

At 24 x 24 the random-weight score maps saturate and few samples keep a usable argmax margin, so a fixture is a SELECTION of samples of one
seed's 16-sample input batch: weights ``synth_vitb_state_dict(seed, len_z=144, len_x=576)``, inputs ``synth_inputs(seed, 16, 192, 384)``,
and the stored ``rows`` = the samples the reference was run on.  Every sample in ``rows`` has a raw AND a Hann-windowed top-2 margin above
0.03 (asserted here when the file is written); the tests run exactly ``rows`` and excuse no argmax flip.

1. ``ref_vb384_s108.npz`` (rows 1, 6, 10, 12; activations of row 1) and ``ref_vb384_s116.npz`` (rows 3, 8, 13): maps, boxes, conf, margins.
   Activations: the token rows ``ACT_ROWS`` (0, 143 | 144, 145: the template / search boundary; 703 | 704: both sides of the last whole
   32-key chunk; 719: the last token) entering block 0 and leaving blocks 0, 3, 5, 11 and the final norm.
2. ``ref_vb384_u8_s<seed>.npz``: make_golden_ostrack_u8.py's recipe at 384: the template crops of ``synth_inputs(seed, 16, 192, 384)``,
   the search crop that ``synth_patches(seed, 16, 384)`` becomes under ``Preprocessor.process``'s line; ``rows`` as above, token rows of
   the first two of them.
3. ``ref_vb384_track_s<seed>.npz``: 2 synthetic sequences x 4 tracked frames at factors 2.0 / 5.0, searched over 40 seeds for a seed whose
   eight Hann margins all exceed 0.03; not written when there is none (the tracking step is then tested by its exactness properties)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_vitb as mv  # noqa: E402
from make_golden_u8 import preprocess  # noqa: E402

from vittracker_amd import host_ops, synth  # noqa: E402
from vittracker_amd.evaluation.data import synthetic_sequence  # noqa: E402

MARGIN = 0.03
TZ, TX, LZ, LX = 192, 384, 144, 576
NPOOL = 16                                                   # samples of a seed's input batch
ACT_ROWS = [0, 72, 143, 144, 145, 288, 432, 576, 640, 688, 703, 704, 712, 719]
ACT_BLOCKS = (0, 3, 5, 11)
PLAIN = ((108, [1, 6, 10, 12], True), (116, [3, 8, 13], False))
N_SEQ, N_FRAMES, TEMPLATE_FACTOR, SEARCH_FACTOR = 2, 4, 2.0, 5.0


def build_reference_384(ostrack, config):
    cfg = config.cfg
    cfg.MODEL.BACKBONE.TYPE = "vit_base_patch16_224"
    cfg.MODEL.HEAD.TYPE, cfg.MODEL.HEAD.NUM_CHANNELS = "CENTER", 256
    cfg.DATA.SEARCH.SIZE, cfg.DATA.TEMPLATE.SIZE = TX, TZ
    cfg.TEST.SEARCH_SIZE, cfg.TEST.TEMPLATE_SIZE = TX, TZ
    return ostrack.build_ostrack(cfg, training=False).eval()


def load_net(ostrack, config, seed):
    net = build_reference_384(ostrack, config)
    sd = synth.synth_vitb_state_dict(seed, len_z=LZ, len_x=LX)
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    assert net.box_head.feat_sz == 24
    return net, sd


def top2(m, B):
    srt = np.sort(np.asarray(m).reshape(B, -1), axis=1)
    return srt[:, -1] - srt[:, -2]


def forward(net, hann_mod, z, x, acts=None):
    hooks = []
    if acts is not None:
        def grab(name, inp=False):
            return lambda _m, i, o: acts.__setitem__(name, (i[0] if inp else o).detach().clone().numpy())
        hooks.append(net.backbone.blocks[0].register_forward_hook(grab("tokens", inp=True)))
        for i in ACT_BLOCKS:
            hooks.append(net.backbone.blocks[i].register_forward_hook(grab(f"block{i}")))
        hooks.append(net.backbone.norm.register_forward_hook(grab("norm")))
    B = z.shape[0]
    with torch.no_grad():
        out = net(template=z, search=x)
        F = net.box_head.feat_sz
        win = hann_mod.hann2d(torch.tensor([F, F]).long(), centered=True)
        hbox = net.box_head.cal_bbox(win * out["score_map"], out["size_map"], out["offset_map"])
        conf = out["score_map"].flatten(1).max(dim=1).values
    for h in hooks:
        h.remove()
    return {"margin_raw": top2(out["score_map"].numpy(), B), "margin_hann": top2((win * out["score_map"]).numpy(), B),
            "score_map": out["score_map"].numpy(), "size_map": out["size_map"].numpy(), "offset_map": out["offset_map"].numpy(),
            "pred_boxes": out["pred_boxes"].numpy(), "hann_boxes": hbox.numpy(), "conf": conf.numpy()}


def run_plain(ostrack, config, hann_mod, seed, rows, with_acts):
    net, sd = load_net(ostrack, config, seed)
    z, x = synth.synth_inputs(seed, NPOOL, TZ, TX)
    acts = {} if with_acts else None
    res = forward(net, hann_mod, torch.from_numpy(z[rows]), torch.from_numpy(x[rows]), acts)
    assert min(res["margin_raw"].min(), res["margin_hann"].min()) > MARGIN, (seed, rows, res["margin_raw"], res["margin_hann"])
    res.update({"model": "vitb384", "seed": seed, "pool": NPOOL, "rows": np.array(rows), "B": len(rows), "state_checksum": synth.state_checksum(sd)})
    if with_acts:
        res["act_rows"] = np.array(ACT_ROWS)
        for k, v in acts.items():
            res["act_" + k] = v[:1, ACT_ROWS].astype(np.float32)      # the first of `rows`, selected token rows, all 768 channels
    return res


def run_u8(ostrack, config, hann_mod, seed):
    """One seed's 16 patches through the reference; the qualifying samples (at most 3), or None when fewer than 2 qualify."""
    net, sd = load_net(ostrack, config, seed)
    z = synth.synth_inputs(seed, NPOOL, TZ, TX)[0]
    patches = synth.synth_patches(seed, NPOOL, TX)
    x = preprocess(patches)
    probe = forward(net, hann_mod, torch.from_numpy(z), x)
    ok = [i for i in range(NPOOL) if min(probe["margin_raw"][i], probe["margin_hann"][i]) > MARGIN]
    print(f"u8 seed {seed}: qualifying samples {ok}")
    if len(ok) < 2:
        return None
    rows = ok[:3]
    acts = {}
    res = forward(net, hann_mod, torch.from_numpy(z[rows]), x[rows], acts)
    assert min(res["margin_raw"].min(), res["margin_hann"].min()) > MARGIN
    res.update({"model": "vitb384", "seed": seed, "pool": NPOOL, "rows": np.array(rows), "B": len(rows), "state_checksum": synth.state_checksum(sd),
                "patch_checksum": int(patches.astype(np.uint64).sum()), "act_rows": np.array(ACT_ROWS),
                "act_tokens": acts["tokens"][:2, ACT_ROWS].astype(np.float32)})
    return res


def seq_seed(seed, q):
    return 1000 * seed + q


def run_track(ostrack, config, box_ops, hann_mod, seed):
    """make_golden_ostrack_u8.run_track at 192 / 384 and factors 2.0 / 5.0; None as soon as a frame's Hann margin is below the rule."""
    net, sd = load_net(ostrack, config, seed)
    F = net.box_head.feat_sz
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
                print(f"track seed {seed}: sequence {q} frame {t} margin {margin:.4f} -> skip")
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
    res.update({"model": "vitb384", "seed": seed, "seq_seeds": np.array([seq_seed(seed, q) for q in range(N_SEQ)]), "n_frames": N_FRAMES,
                "template_factor": TEMPLATE_FACTOR, "search_factor": SEARCH_FACTOR, "state_checksum": synth.state_checksum(sd)})
    return res


def main():
    torch.manual_seed(0)
    ostrack, config, hann_mod = mv.import_reference_ostrack()
    box_ops = sys.modules["lib.utils.box_ops"]
    what = sys.argv[1:] or ["plain", "u8", "track"]
    if "plain" in what:
        for seed, rows, with_acts in PLAIN:
            res = run_plain(ostrack, config, hann_mod, seed, rows, with_acts)
            np.savez_compressed(os.path.join(HERE, f"ref_vb384_s{seed}.npz"), **res)
            print(f"ref_vb384_s{seed}.npz: rows {rows} margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)}")
    if "u8" in what:
        for seed in range(170, 210):
            res = run_u8(ostrack, config, hann_mod, seed)
            if res is not None:
                np.savez_compressed(os.path.join(HERE, f"ref_vb384_u8_s{seed}.npz"), **res)
                print(f"ref_vb384_u8_s{seed}.npz: rows {res['rows'].tolist()} margins raw {np.round(res['margin_raw'], 4)} hann {np.round(res['margin_hann'], 4)}")
                break
    if "track" in what:
        for seed in range(170, 210):
            res = run_track(ostrack, config, box_ops, hann_mod, seed)
            if res is not None:
                np.savez_compressed(os.path.join(HERE, f"ref_vb384_track_s{seed}.npz"), **res)
                print(f"ref_vb384_track_s{seed}.npz: hann margins {np.round(res['margin_hann'].reshape(-1), 4)}")
                break
        else:
            print("track: no seed in [170, 210) keeps all eight margins above 0.03: no tracking fixture")


if __name__ == "__main__":
    main()
