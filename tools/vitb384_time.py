#!/usr/bin/env python3
"""ViT-Base at both geometries -- OSTrack-256 (128 / 256, 320 tokens) and OSTrack-384 (192 / 384, 720 tokens) -- timed in the same process.

    python tools/vitb384_time.py [--batch 256,64] [--rounds 5] [--replays 10] [--no-split]

Per batch size B: the captured step of B frames (vt_graph_capture on fixed fp32 crops) of each geometry, replayed in `--rounds` interleaved
rounds (the order rotates every round; a round is a host-timed region of `--replays` replays behind one synchronisation), the shader clock
probed before and after (vt_probe_clock: a throttled or shared chip shows there, not in a ratio).  Printed: ms per step and frames/s per
geometry (best round and the [min, max] over the rounds), the measured per-frame time ratio 384 / 256 next to the MAC ratio of
oracle.vitb_oracle_torch.macs_per_frame(192, 384) over (128, 256) (about 2.42).

The per-kernel split of one step (largest B) comes from a child process per geometry under `rocprofv3 --kernel-trace --stats` (this
file with --child: it only replays), summed per kernel and divided by the replays.  --no-split, or no rocprofv3 on PATH: skipped.
VB_FUSED_QKV / VB_ATTN_STREAM are the library's switches (read at model creation) and are passed on as set.

One JSON line at the end.  Reads nothing outside the repository."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

GEOMS = {"256": (128, 256), "384": (192, 384)}
CHILD_REPLAYS = 6


def _graph(geom, B):
    import torch
    from vittracker_amd import native, synth
    tz, tx = GEOMS[geom]
    m = native.Model(tz, tx, channels=768, heads=12, depth=12, head_channels=256, max_batch=B)
    m.load_state_dict(synth.synth_vitb_state_dict(26, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2))
    z, x = synth.synth_inputs(0, min(B, 8), tz, tx)          # the content does not change the cost: 8 distinct frames, repeated
    rep = (B + z.shape[0] - 1) // z.shape[0]
    zd = torch.from_numpy(z).cuda().repeat(rep, 1, 1, 1)[:B].contiguous()
    xd = torch.from_numpy(x).cuda().repeat(rep, 1, 1, 1)[:B].contiguous()
    g, out = m.capture(zd, xd)
    g.launch()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.score_map).all())
    return m, g, out, (zd, xd)


def _child(geom, B):
    import torch
    m, g, out, keep = _graph(geom, B)
    for _ in range(CHILD_REPLAYS):
        g.launch()
    torch.cuda.synchronize()
    print("CHILD-OK")


def _split(geom, B, script=None):
    """{kernel: us per step} of one geometry's step from a rocprofv3 child, or a string saying why not.  script: the file whose
    `--child <geom> --batch B` replays the step (this one; tools/vitl_time.py passes itself)."""
    if shutil.which("rocprofv3") is None:
        return "rocprofv3 not on PATH"
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(script or __file__),
                            "--child", geom, "--batch", str(B)], capture_output=True, text=True, timeout=900, cwd=d)
        if p.returncode != 0 or "CHILD-OK" not in p.stdout:
            return "child failed: " + (p.stdout + p.stderr)[-400:]
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return "no kernel_stats.csv written"
        rows, calls = {}, {}
        for r in csv.DictReader(open(files[0])):
            name = r["Name"].split("(")[0].replace("void ", "")
            rows[name] = rows.get(name, 0.0) + float(r["TotalDurationNs"]) * 1e-3
            calls[name] = calls.get(name, 0) + int(r["Calls"])
    # every step (the capture's eager warm-up and the capture's own replay included) launches conv5 exactly once: vbm::conv5_kernel, in
    # fp32 mode vbf::conv5_f32_kernel
    steps = next((n for name, n in calls.items() if "conv5_kernel" in name or "conv5_f32_kernel" in name), 0)
    if not steps:
        return "no conv5 kernel launch in the trace"
    return {k: {"us_per_step": round(v / steps, 1), "launches_per_step": round(calls[k] / steps, 2),
                "us_per_launch": round(v / calls[k], 1)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="256,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return _child(a.child, int(a.batch))
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import native
    mac = {g: sum(ob.macs_per_frame(*GEOMS[g]).values()) for g in GEOMS}
    res = {"mac_ratio": round(mac["384"] / mac["256"], 3), "gmac_per_frame": {g: round(v / 1e9, 2) for g, v in mac.items()},
           "switches": {k: os.environ.get(k) for k in ("VB_FUSED_QKV", "VB_ATTN_STREAM")}, "batches": {}}
    batches = [int(b) for b in a.batch.split(",")]
    for B in batches:
        clock0 = native.probe_clock(20000, 1)[0]
        models = {g: _graph(g, B) for g in GEOMS}
        every = {g: [] for g in GEOMS}
        names = list(GEOMS)
        for r in range(a.rounds):
            for g in names[r % 2:] + names[:r % 2]:
                graph = models[g][1]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.replays):
                    graph.launch()
                torch.cuda.synchronize()
                every[g].append((time.perf_counter() - t0) / a.replays * 1e3)
        clock1 = native.probe_clock(20000, 1)[0]
        row = {"clock_probe": [round(clock0, 1), round(clock1, 1)]}
        for g in GEOMS:
            best = min(every[g])
            row[g] = {"ms_per_step": round(best, 3), "ms_min_max": [round(min(every[g]), 3), round(max(every[g]), 3)], "frames_per_s": round(B / best * 1e3, 1)}
            print(f"B {B:4d}  geometry {g}: {best:8.3f} ms/step  [{min(every[g]):.3f}, {max(every[g]):.3f}]  {B / best * 1e3:9.1f} frames/s")
        row["time_ratio_384_over_256"] = round(row["384"]["ms_per_step"] / row["256"]["ms_per_step"], 3)
        print(f"B {B:4d}  per-frame time ratio 384 / 256 = {row['time_ratio_384_over_256']:.3f}   MAC ratio = {res['mac_ratio']:.3f}   clock probe {row['clock_probe']}")
        res["batches"][str(B)] = row
        del models
        torch.cuda.empty_cache()
    if not a.no_split:
        B = max(batches)
        res["split_batch"] = B
        res["split"] = {}
        for g in GEOMS:
            s = _split(g, B)
            res["split"][g] = s
            if isinstance(s, str):
                print(f"per-kernel split, geometry {g}: {s}")
                continue
            print(f"per-kernel split of one step, geometry {g}, B {B} (us per step | launches per step | us per launch):")
            for k, v in s.items():
                print(f"  {k[:70]:70s} {v['us_per_step']:10.1f} {v['launches_per_step']:7.2f} {v['us_per_launch']:9.1f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
