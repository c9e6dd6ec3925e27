#!/usr/bin/env python3
"""Frame tables against the dense path, and continuous against grouped batching.

    python tools/mixed_batch.py crop  [--geom 128] [--iters 50]     # (a) the crop alone: vt_crop_u8 vs vt_crop_u8_frames, B = 256, one size
    python tools/mixed_batch.py step  [--geom 128] [--iters 200]    # (b) the tracker step: vt_track_step vs vt_track_step_frames
    python tools/mixed_batch.py runner [--seqs 512] [--frames 20] [--batch 256]   # (c) sequences/s, run_dataset_continuous vs _batched

(a) is meant to run under `rocprofv3 --kernel-trace --stats -- python tools/mixed_batch.py crop`: the kernel statistics separate the
dense crop_band_kernel<..., 4 template arguments> from its table twin crop_band_kernel<..., vtt::TableFrames>.  The wall times printed here are host-timed with one synchronisation
per region.  Prints one JSON line per mode."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _model(geom, B):
    from vittracker_amd import native, synth
    m = native.Model(geom // 2, geom, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(0, len_z=(geom // 32) ** 2, len_x=(geom // 16) ** 2))
    return m


def _setup(geom, B, H=360, W=480):
    import torch
    from vittracker_amd.native import FrameTable
    rs = np.random.RandomState(0)
    frames = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda()
    states = torch.tensor([[rs.uniform(60, W - 120), rs.uniform(60, H - 120), rs.uniform(30, 90), rs.uniform(30, 90)] for _ in range(B)],
                          dtype=torch.float64).cuda()
    tab = FrameTable(B, "cuda")
    for b in range(B):
        tab.set_tensor(b, frames[b])
    tab.upload()
    return frames, states, tab


def _time(fn, iters):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def crop(a):
    m = _model(a.geom, a.batch)
    frames, states, tab = _setup(a.geom, a.batch)
    dense = _time(lambda: m.crop_u8(frames, states, 4.0, a.geom), a.iters)
    table = _time(lambda: m.crop_u8_frames(tab, states, 4.0, a.geom), a.iters)
    return {"mode": "crop", "geom": a.geom, "B": a.batch, "dense_us": round(dense, 2), "table_us": round(table, 2), "ratio": round(table / dense, 4)}


def step(a):
    import torch
    from vittracker_amd.native import Outputs
    B, S = a.batch, a.geom
    m = _model(S, B)
    m.set_open_loop(True)            # held boxes: both forms crop the same windows every step
    frames, states, tab = _setup(S, B)
    m.set_template(torch.zeros(B, 3, S // 2, S // 2, device="cuda"))
    x = torch.empty(B, 3, S, S, device="cuda")
    rf = torch.empty(B, dtype=torch.float64, device="cuda")
    out = Outputs(B, S // 16, "cuda")
    rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
    graphs = {}
    for name, fn in (("dense", lambda cs: m.track_step(frames, states, 4.0, MEAN, STD, x, rf, out, record=rec, stream=cs)),
                     ("table", lambda cs: m.track_step_frames(tab, states, 4.0, MEAN, STD, x, rf, out, record=rec, stream=cs))):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=side):
            fn(torch.cuda.current_stream())
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = g
    res = {}
    for _ in range(3):       # interleaved rounds, the best of each
        for name, g in graphs.items():
            res[name] = min(res.get(name, 1e30), _time(g.replay, a.iters))
    return {"mode": "step", "geom": S, "B": B, "dense_us": round(res["dense"], 2), "table_us": round(res["table"], 2),
            "ratio": round(res["table"] / res["dense"], 4), "dense_frames_per_s": round(B / res["dense"] * 1e6)}


def runner(a):
    from vittracker_amd.evaluation import Tracker, get_dataset
    from vittracker_amd.evaluation.running import run_dataset_batched, run_dataset_continuous
    ds = get_dataset(f"synthetic_mixed:{a.seqs}x{a.frames}")
    nframes = sum(len(s) for s in ds)
    res = {"mode": "runner", "sequences": len(ds), "frames": nframes, "batch": a.batch}
    for name, run in (("grouped", lambda t: run_dataset_batched(ds, t, batch=a.batch)), ("continuous", lambda t: run_dataset_continuous(ds, t, batch=a.batch))):
        with tempfile.TemporaryDirectory() as d:
            os.environ["VITTRACK_SAVE_DIR"] = d
            os.environ["VITTRACK_PRJ_DIR"] = ROOT
            t = Tracker("vit_dist", "vit_48_h32_g128", "synthetic")
            get = t.get_parameters

            def params(get=get):
                p = get()
                p.allow_synthetic_weights = True
                return p
            t.get_parameters = params
            import contextlib
            import io
            log = io.StringIO()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(log):
                run(t)
            wall = time.perf_counter() - t0
            written = sum(1 for s in ds if os.path.exists(os.path.join(t.results_dir, s.name + ".txt")))
        if written != len(ds):      # a runner reports a failing group / sequence and goes on: then the timing means nothing
            raise SystemExit(f"{name}: {written} of {len(ds)} result files written\n" + log.getvalue()[-3000:])
        res[name + "_s"] = round(wall, 2)
        res[name + "_seq_per_s"] = round(len(ds) / wall, 1)
    res["speedup"] = round(res["grouped_s"] / res["continuous_s"], 3)
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("mode", choices=("crop", "step", "runner"))
    p.add_argument("--geom", type=int, default=128)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--seqs", type=int, default=512)
    p.add_argument("--frames", type=int, default=20)
    a = p.parse_args()
    import torch
    torch.cuda.set_device(0)
    print(json.dumps({"crop": crop, "step": step, "runner": runner}[a.mode](a)))


if __name__ == "__main__":
    main()
