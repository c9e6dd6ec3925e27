#!/usr/bin/env python3
"""The ViT OSTrack tracker step at a few sequences: the narrow 128 x 64 GEMM tile against the 256 x 256 one.

    python tools/vitb_latency.py [--models base256,base384,large256,ce256] [--batches 1,2,4,8,16,32,64] [--rounds 5] [--replays 20]
    python tools/vitb_latency.py --models base256 --fills 25,100          # the automatic choice at other thresholds (VB_GEMM_NARROW_FILL)
    rocprofv3 --kernel-trace --stats -d out -- python tools/vitb_latency.py --models base256 --batches 1 --steps-only auto
                                                                            # the per-kernel split of one form's step (a run of its own)

One process per invocation.  Per model point four models on the same weights, created under VB_GEMM_NARROW=0 (W, the 256 x 256 tile
everywhere: the code path before the narrow tile existed), =1 (N, narrow wherever an instantiation exists) and unset (A, the per-launch
choice of vitb.hip narrow_pick), plus one per --fills value.  Per batch size a captured vt_track_step graph of each on 1920 x 1080 device
frames, open loop around held boxes (tools/vitb_track.py's set-up), the wide form a second time as a model and a graph of its own (W2:
|W - W2| is the point's own spread, the placement of a model's buffers included), all timed in interleaved rounds
(tools/frame_formats.py's method, best round reported), the shader clock probed before and after.
Prints one JSON line per (model point, batch): us per step of every form, the spread, vt_gemm_form of A, and the two verdicts
    faster   A is faster than W by more than the spread      (expected wherever A runs some GEMM narrow)
    held     A is not slower than W by more than the spread  (expected everywhere)
ce256 is the compacted candidate-elimination model (stages behind blocks 3, 6, 9, keep ratio 0.7) and is swept at B = 1 and 8 only."""
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
POINTS = {
    "base256": dict(tz=128, tx=256, C=768, heads=12, depth=12, zf=2.0, xf=4.0, ce=None),
    "base384": dict(tz=192, tx=384, C=768, heads=12, depth=12, zf=2.0, xf=5.0, ce=None),
    "large256": dict(tz=128, tx=256, C=1024, heads=16, depth=24, zf=2.0, xf=4.0, ce=None),
    "ce256": dict(tz=128, tx=256, C=768, heads=12, depth=12, zf=2.0, xf=4.0, ce=([3, 6, 9], [0.7, 0.7, 0.7])),
}
CE_BATCHES = (1, 8)


def _model(p, sd, maxB, env):
    """A model of point p created under the given VB_GEMM_* environment."""
    from vittracker_amd import native
    saved = {k: os.environ.pop(k, None) for k in ("VB_GEMM_NARROW", "VB_GEMM_NARROW_FILL")}
    os.environ.update(env)
    try:
        m = native.Model(p["tz"], p["tx"], channels=p["C"], heads=p["heads"], depth=p["depth"], head_channels=256, max_batch=maxB)
    finally:
        for k in saved:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    m.load_state_dict(sd)
    if p["ce"]:
        m.set_candidate_elimination(*p["ce"], form="compact")
    m.set_open_loop(True)
    return m


def main():
    import torch
    from vittracker_amd import native, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="base256,base384,large256,ce256")
    ap.add_argument("--batches", default="1,2,4,8,16,32,64")
    ap.add_argument("--fills", default="", help="comma-separated VB_GEMM_NARROW_FILL values: one more automatic model each (F<value>)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps-only", default="", help="W, N or auto: run 20 eager steps of that form per batch and time nothing (profiler runs)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    batches = [int(b) for b in a.batches.split(",")]
    fills = [int(f) for f in a.fills.split(",")] if a.fills else []
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    distinct = torch.randint(0, 256, (a.distinct, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    for name in a.models.split(","):
        p = POINTS[name]
        bs = [b for b in batches if not p["ce"] or b in CE_BATCHES]
        if not bs:
            continue
        maxB = max(bs)
        sd = synth.synth_vitb_state_dict(26, C=p["C"], depth=p["depth"], heads=p["heads"], len_z=(p["tz"] // 16) ** 2, len_x=(p["tx"] // 16) ** 2)
        envs = {"W": {"VB_GEMM_NARROW": "0"}, "W2": {"VB_GEMM_NARROW": "0"}, "N": {"VB_GEMM_NARROW": "1"}, "A": {}}
        envs.update({f"F{f}": {"VB_GEMM_NARROW_FILL": str(f)} for f in fills})
        if a.steps_only:
            envs = {a.steps_only: envs[{"auto": "A"}.get(a.steps_only, a.steps_only)]}
        models = {k: _model(p, sd, maxB, env) for k, env in envs.items()}
        del sd
        for B in bs:
            rs = np.random.RandomState(B)
            frames = distinct[torch.arange(B, device="cuda") % a.distinct].contiguous()
            boxes = torch.tensor([[rs.uniform(120, W - 240), rs.uniform(120, H - 240), rs.uniform(30, 90), rs.uniform(30, 90)] for _ in range(B)],
                                 dtype=torch.float64).cuda()
            F = p["tx"] // 16
            graphs, keep = {}, []
            for k, m in models.items():
                states = boxes.clone()
                z, rf = m.crop(frames, states, p["zf"], p["tz"], MEAN, STD)
                m.set_template(z)
                x = torch.empty(B, 3, p["tx"], p["tx"], device="cuda")
                out, rec = native.Outputs(B, F, "cuda"), torch.empty(B, 5, dtype=torch.float64, device="cuda")
                keep.append((states, rf, x, out, rec))

                def step(cs, m=m, states=states, rf=rf, x=x, out=out, rec=rec):
                    m.track_step(frames, states, p["xf"], MEAN, STD, x, rf, out, record=rec, stream=cs)
                if a.steps_only:
                    for _ in range(20):
                        step(torch.cuda.current_stream())
                    torch.cuda.synchronize()
                else:
                    graphs[k] = _capture(step)
            if a.steps_only:
                continue
            clock0 = native.probe_clock(20000, 1)[0]
            us = _interleaved(graphs, 1, a.rounds, a.replays)
            spread = abs(us["W"] - us["W2"])
            wide = min(us["W"], us["W2"])
            res = {"model": name, "B": B, "us_per_step": us, "spread_us": round(spread, 2), "gemm_form_auto": models["A"].gemm_form(B),
                   "speedup_auto": round(wide / us["A"], 3), "speedup_narrow": round(wide / us["N"], 3),
                   "faster": bool(us["A"] < wide - spread), "held": bool(us["A"] <= max(us["W"], us["W2"]) + spread),
                   "frames_per_s_auto": round(B / us["A"] * 1e6, 1),
                   "clock_mhz": [round(clock0, 1), round(native.probe_clock(20000, 1)[0], 1)]}
            print(json.dumps(res), flush=True)
            del graphs, keep
        for m in models.values():
            m.close()


if __name__ == "__main__":
    main()
