#!/usr/bin/env python3
"""ViT-Large against ViT-Base -- ViT-Base 128 / 256, ViT-Large 128 / 256 and ViT-Large 192 / 384 -- timed in the same process, by the method of
tools/vitb384_time.py.

    python tools/vitl_time.py [--batch 256,64] [--rounds 5] [--replays 10] [--no-split]

Per batch size B: the captured step of B frames (vt_graph_capture on fixed fp32 crops) of each configuration, replayed in `--rounds`
interleaved rounds (the order rotates every round; a round is a host-timed region of `--replays` replays behind one synchronisation), the
shader clock probed before and after (vt_probe_clock).  Printed: ms per step and frames/s per configuration (best round and the [min, max]
over the rounds), the per-frame time ratio to the ViT-Base figure OF THIS RUN next to the MAC ratio of oracle.vitb_oracle_torch.macs_per_frame
(3.37 at 128 / 256, 8.03 at 192 / 384).

The per-kernel split of one step (largest B) comes from a child process per configuration under `rocprofv3 --kernel-trace --stats` (this file
with --child: it only replays), summed per kernel and divided by the steps.  --no-split, or no rocprofv3 on PATH: skipped.

One JSON line at the end.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

#: name -> (template, search, width, heads, depth)
CONFIGS = {"vitb_256": (128, 256, 768, 12, 12), "vitl_256": (128, 256, 1024, 16, 24), "vitl_384": (192, 384, 1024, 16, 24)}
CHILD_REPLAYS = 6
_SD = {}


def _graph(name, B):
    import torch
    from vittracker_amd import native, synth
    tz, tx, C, heads, depth = CONFIGS[name]
    if name not in _SD:
        _SD[name] = synth.synth_vitb_state_dict(26, C=C, depth=depth, heads=heads, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
    m = native.Model(tz, tx, channels=C, heads=heads, depth=depth, head_channels=256, max_batch=B)
    m.load_state_dict(_SD[name])
    z, x = synth.synth_inputs(0, min(B, 8), tz, tx)          # the content does not change the cost: 8 distinct frames, repeated
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
    m, g, out, keep = _graph(name, B)
    for _ in range(CHILD_REPLAYS):
        g.launch()
    torch.cuda.synchronize()
    print("CHILD-OK")


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
    import vitb384_time as vt          # its rocprofv3 child runner and CSV reduction
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import native
    mac = {n: sum(ob.macs_per_frame(c[0], c[1], C=c[2], depth=c[4]).values()) for n, c in CONFIGS.items()}
    res = {"mac_ratio_to_vitb_256": {n: round(v / mac["vitb_256"], 3) for n, v in mac.items()}, "gmac_per_frame": {n: round(v / 1e9, 2) for n, v in mac.items()},
           "switches": {k: os.environ.get(k) for k in ("VB_FUSED_QKV", "VB_ATTN_STREAM", "VB_QA_HGROUP")}, "batches": {}}
    batches = [int(b) for b in a.batch.split(",")]
    names = list(CONFIGS)
    for B in batches:
        clock0 = native.probe_clock(20000, 1)[0]
        models = {n: _graph(n, B) for n in names}
        every = {n: [] for n in names}
        for r in range(a.rounds):
            k = r % len(names)
            for n in names[k:] + names[:k]:
                graph = models[n][1]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.replays):
                    graph.launch()
                torch.cuda.synchronize()
                every[n].append((time.perf_counter() - t0) / a.replays * 1e3)
        clock1 = native.probe_clock(20000, 1)[0]
        row = {"clock_probe": [round(clock0, 1), round(clock1, 1)]}
        for n in names:
            best = min(every[n])
            row[n] = {"ms_per_step": round(best, 3), "ms_min_max": [round(min(every[n]), 3), round(max(every[n]), 3)], "frames_per_s": round(B / best * 1e3, 1)}
            print(f"B {B:4d}  {n}: {best:8.3f} ms/step  [{min(every[n]):.3f}, {max(every[n]):.3f}]  {B / best * 1e3:9.1f} frames/s", flush=True)
        for n in names[1:]:
            row[n]["time_ratio_to_vitb_256"] = round(row[n]["ms_per_step"] / row["vitb_256"]["ms_per_step"], 3)
            print(f"B {B:4d}  per-frame time ratio {n} / vitb_256 = {row[n]['time_ratio_to_vitb_256']:.3f}   MAC ratio = {res['mac_ratio_to_vitb_256'][n]:.3f}   "
                  f"clock probe {row['clock_probe']}", flush=True)
        res["batches"][str(B)] = row
        del models
        torch.cuda.empty_cache()
    _SD.clear()
    if not a.no_split:
        B = max(batches)
        res["split_batch"] = B
        res["split"] = {}
        for n in names:
            s = vt._split(n, B, script=__file__)
            res["split"][n] = s
            if isinstance(s, str):
                print(f"per-kernel split, {n}: {s}")
                continue
            print(f"per-kernel split of one step, {n}, B {B} (us per step | launches per step | us per launch):")
            for k, v in s.items():
                print(f"  {k[:70]:70s} {v['us_per_step']:10.1f} {v['launches_per_step']:7.2f} {v['us_per_launch']:9.1f}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
