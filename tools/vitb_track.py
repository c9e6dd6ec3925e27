#!/usr/bin/env python3
"""The ViT-Base OSTrack tracker step against the forward-only step: what tracking costs on top of evaluating.

    python tools/vitb_track.py [--batch 256] [--rounds 5] [--replays 10]            # in-step chains by the default (two from 64 frames)
    VT_GRAPH_CHAINS=1 python tools/vitb_track.py --only T                            # the same step as one chain

One process, B sequences, 1920 x 1080 frames on the device, open loop (vt_set_open_loop) around held 30-90 px boxes, as
tracking/track_batch_demo.py --hold-boxes.  Captured graphs, timed in interleaved rounds (tools/frame_formats.py's method: the order
rotates every round, one synchronisation per region, best round reported), the shader clock probed before and after:
  A     forward-only graph on fp32 crops with the template given (vt_graph_capture: the path bench.py --config vitb times)
  A2    A captured a second time: |A - A2| is this run's own spread
  N     the network alone on the uint8 patch with the cached template (vt_forward_u8(NULL, patch))
  T     the whole tracker step (vt_track_step: crop -> patchify_u8 -> network -> tail)
  crop  the uint8 crop alone (vt_crop_u8), per launch out of `--reps` launches per replay
Held: T - A <= crop + |A - A2|.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_formats import MEAN, STD, _capture, _interleaved  # noqa: E402

H, W = 1080, 1920


def main():
    import torch
    from vittracker_amd import native, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--only", default="", help="comma-separated subset of A,A2,N,T,crop")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    B = a.batch
    want = set(a.only.split(",")) if a.only else {"A", "A2", "N", "T", "crop"}
    clock0 = native.probe_clock(20000, 1)[0]
    m = native.Model(128, 256, channels=768, heads=12, depth=12, head_channels=256, max_batch=B)
    m.load_state_dict(synth.synth_vitb_state_dict(26))
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    rs = np.random.RandomState(0)
    distinct = torch.randint(0, 256, (a.distinct, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    frames = distinct[torch.arange(B, device="cuda") % a.distinct].contiguous()
    states = torch.tensor([[rs.uniform(120, W - 240), rs.uniform(120, H - 240), rs.uniform(30, 90), rs.uniform(30, 90)] for _ in range(B)],
                          dtype=torch.float64).cuda()
    z, rf = m.crop(frames, states, 2.0, 128, MEAN, STD)
    xf, _ = m.crop(frames, states, 4.0, 256, MEAN, STD)
    m.set_template(z)
    m.set_open_loop(True)
    patch = torch.empty(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    m.crop_u8(frames, states, 4.0, 256, out=patch, resize_factor=rf)
    x = torch.empty(B, 3, 256, 256, device="cuda")
    rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
    outs = {k: native.Outputs(B, 16, "cuda") for k in ("A", "A2", "N", "T")}
    graphs, keep = {}, []

    class _Native:          # vt_graph_launch behind the replay() the timing loop calls
        def __init__(self, gr):
            self.gr = gr

        def replay(self):
            self.gr.launch()
    for k in ("A", "A2"):
        if k in want:
            gr, _ = m.capture(z, xf, outs[k])
            graphs[k] = _Native(gr)
    if "N" in want:
        graphs["N"] = _capture(lambda cs: m.forward_u8(None, patch, out=outs["N"], stream=cs))
    if "T" in want:
        graphs["T"] = _capture(lambda cs: m.track_step(frames, states, 4.0, MEAN, STD, x, rf, outs["T"], record=rec, stream=cs))
    row = _interleaved(graphs, 1, a.rounds, a.replays)
    res = {"B": B, "frame": [H, W], "rounds": a.rounds, "replays": a.replays, "graph_chains_env": os.environ.get("VT_GRAPH_CHAINS", ""),
           "ms_per_step": {k: round(v / 1e3, 4) for k, v in row.items()}}
    if "crop" in want:
        def crops(cs):
            for _ in range(a.reps):
                m.crop_u8(frames, states, 4.0, 256, out=patch, resize_factor=rf, stream=cs)
        res["crop_us"] = _interleaved({"crop": _capture(crops)}, a.reps, a.rounds, a.replays)["crop"]
    ms = res["ms_per_step"]
    if {"A", "A2", "T"} <= set(ms) and "crop_us" in res:
        spread = abs(ms["A"] - ms["A2"])
        res["T_minus_A_ms"] = round(ms["T"] - ms["A"], 4)
        res["allowance_ms"] = round(res["crop_us"] / 1e3 + spread, 4)
        res["held"] = bool(ms["T"] - ms["A"] <= res["crop_us"] / 1e3 + spread)
        if "N" in ms:
            res["N_minus_A_ms"] = round(ms["N"] - ms["A"], 4)
    if "T" in ms:
        res["frames_per_s_T"] = round(B / ms["T"] * 1e3, 1)
    res["clock_mhz"] = [round(clock0, 1), round(native.probe_clock(20000, 1)[0], 1)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
