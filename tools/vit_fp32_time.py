#!/usr/bin/env python3
"""The fp32-equivalent mode (vt_set_precision) against the bf16 mode of the same model, timed in the same process by the method of
tools/vit_small_time.py.

    python tools/vit_fp32_time.py [--batch 256,8] [--geoms 256,384] [--models vitb,vitt] [--rounds 5] [--replays 10] [--no-split]

Per geometry, batch size B and model: the captured forward of B frames (vt_graph_capture on fixed fp32 crops) in bf16 mode and in fp32 mode
(<model>_fp32), replayed in `--rounds` interleaved rounds (the order rotates every round; a round is a host-timed region of `--replays`
replays behind one synchronisation), the shader clock probed before and after (vt_probe_clock).  Printed: ms per step and frames/s (best round
and [min, max]) and the ratio fp32 / bf16 of the SAME rounds.

The per-kernel split of one fp32-mode forward (largest B, 128 / 256) comes from a child process per model under `rocprofv3 --kernel-trace
--stats` (this file with --child: it only replays).  --no-split, or no rocprofv3 on PATH: skipped.

One JSON line at the end.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vit_small_time as vs      # its models, captured graphs and interleaved rounds


def _graph(name, geom, B):
    """vit_small_time's captured forward; <model>_fp32: the same model switched to fp32 mode before the capture."""
    import torch
    from vittracker_amd import synth
    base, fp32 = (name[:-5], True) if name.endswith("_fp32") else (name, False)
    m = vs._model(base, geom, B)
    if fp32:
        m.set_precision("fp32")
    tz, tx = vs.GEOMS[geom][:2]
    z, x = synth.synth_inputs(0, min(B, 8), tz, tx)
    rep = (B + z.shape[0] - 1) // z.shape[0]
    zd = torch.from_numpy(z).cuda().repeat(rep, 1, 1, 1)[:B].contiguous()
    xd = torch.from_numpy(x).cuda().repeat(rep, 1, 1, 1)[:B].contiguous()
    g, out = m.capture(zd, xd)
    g.launch()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.score_map).all())
    return m, g, out, (zd, xd)


def _child(name, B):
    import torch
    m, g, out, keep = _graph(name, "256", B)
    for _ in range(vs.CHILD_REPLAYS):
        g.launch()
    torch.cuda.synchronize()
    print("CHILD-OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="256,8")
    ap.add_argument("--geoms", default="256,384")
    ap.add_argument("--models", default="vitb,vitt")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return _child(a.child, int(a.batch))
    import torch
    import vitb384_time as vt          # its rocprofv3 child runner and CSV reduction
    from vittracker_amd import native
    batches = [int(b) for b in a.batch.split(",")]
    models = a.models.split(",")
    res = {"depth": vs.DEPTH, "forward": {}}
    for geom in a.geoms.split(","):
        for B in batches:
            for base in models:
                names = [base, base + "_fp32"]
                clock0 = native.probe_clock(20000, 1)[0]
                live = {n: _graph(n, geom, B) for n in names}
                every = vs._rounds({n: live[n][1].launch for n in names}, a.rounds, a.replays)
                clock1 = native.probe_clock(20000, 1)[0]
                row = {n: {"ms_per_step": round(min(v), 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)],
                           "frames_per_s": round(B / min(v) * 1e3, 1)} for n, v in every.items()}
                row["fp32_over_bf16"] = round(min(every[names[1]]) / min(every[names[0]]), 3)
                row["clock_probe"] = [round(clock0, 1), round(clock1, 1)]
                print(f"forward {geom} B {B:4d}  {base}: bf16 {row[names[0]]['ms_per_step']:.4f} ms  fp32 {row[names[1]]['ms_per_step']:.4f} ms  "
                      f"[{row[names[1]]['ms_min_max'][0]:.4f}, {row[names[1]]['ms_min_max'][1]:.4f}]  fp32 / bf16 = {row['fp32_over_bf16']:.3f}  "
                      f"clock probe {row['clock_probe']}", flush=True)
                res["forward"][f"{geom}/{B}/{base}"] = row
                for m in live.values():
                    m[0].close()
                del live
                torch.cuda.empty_cache()
    vs._SD.clear()
    if not a.no_split:
        B = max(batches)
        res["split_batch"], res["split"] = B, {}
        for base in models:
            s = vt._split(base + "_fp32", B, script=__file__)
            res["split"][base] = s
            if isinstance(s, str):
                print(f"per-kernel split, {base} fp32: {s}")
                continue
            print(f"per-kernel split of one fp32-mode forward, {base}, 128 / 256, B {B} (us per step | launches per step | us per launch):")
            for k, v in s.items():
                print(f"  {k[:70]:70s} {v['us_per_step']:10.1f} {v['launches_per_step']:7.2f} {v['us_per_launch']:9.1f}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
