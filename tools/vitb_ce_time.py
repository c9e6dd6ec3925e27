#!/usr/bin/env python3
"""Candidate elimination by key masking against the plain ViT-Base model, at both geometries, timed in the same process.

    python tools/vitb_ce_time.py [--batch 256] [--rounds 5] [--replays 10] [--range CTR_POINT] [--no-split]

Per geometry (OSTrack-256: 128 / 256, OSTrack-384: 192 / 384) two models on the same weights: the plain one and the published CE
configuration (CE_LOC [3, 6, 9], CE_KEEP_RATIO 0.7, --range rows).  Their captured steps of --batch frames are replayed in --rounds
interleaved rounds (the order rotates; a round is a host-timed region of --replays replays behind one synchronisation), the shader clock
probed before and after, as tools/vitb384_time.py does (whose graph and rocprofv3 helpers this file reuses).  The masked form removes no
work: expect CE slower than plain at 256 (blocks 3-11 leave the fused qkv + attention kernel for qk GEMM + v GEMM + the streaming
kernel) and about equal at 384 (that route already).

The per-kernel split (score, select, masked attention, zeroing among the rest) comes from a rocprofv3 child per variant.  One JSON line at
the end.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vitb384_time as vt  # noqa: E402

LOC, RATIO = [3, 6, 9], [0.7, 0.7, 0.7]


def _graph(variant, B):
    """variant: '<geometry>:plain' or '<geometry>:<CE_TEMPLATE_RANGE>'."""
    import torch
    from vittracker_amd import native, synth
    from vittracker_amd.model_vitb import ce_template_rows
    geom, kind = variant.split(":")
    tz, tx = vt.GEOMS[geom]
    m = native.Model(tz, tx, channels=768, heads=12, depth=12, head_channels=256, max_batch=B)
    m.load_state_dict(synth.synth_vitb_state_dict(26, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2))
    if kind != "plain":
        m.set_candidate_elimination(LOC, RATIO, ce_template_rows(kind, tz // 16))
    z, x = synth.synth_inputs(0, min(B, 8), tz, tx)
    rep = (B + z.shape[0] - 1) // z.shape[0]
    zd = torch.from_numpy(z).cuda().repeat(rep, 1, 1, 1)[:B].contiguous()
    xd = torch.from_numpy(x).cuda().repeat(rep, 1, 1, 1)[:B].contiguous()
    g, out = m.capture(zd, xd)
    g.launch()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.score_map).all())
    return m, g, out, (zd, xd)


def _child(variant, B):
    import torch
    m, g, out, keep = _graph(variant, B)
    for _ in range(vt.CHILD_REPLAYS):
        g.launch()
    torch.cuda.synchronize()
    print("CHILD-OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--range", default="CTR_POINT")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return _child(a.child, a.batch)
    import torch
    from vittracker_amd import native
    B = a.batch
    res = {"batch": B, "range": a.range, "geometries": {}}
    for geom in vt.GEOMS:
        names = [f"{geom}:plain", f"{geom}:{a.range}"]
        clock0 = native.probe_clock(20000, 1)[0]
        models = {n: _graph(n, B) for n in names}
        every = {n: [] for n in names}
        for r in range(a.rounds):
            for n in names[r % 2:] + names[:r % 2]:
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
            row[n.split(":")[1]] = {"ms_per_step": round(best, 3), "ms_min_max": [round(min(every[n]), 3), round(max(every[n]), 3)]}
            print(f"B {B:4d}  {n:16s}: {best:8.3f} ms/step  [{min(every[n]):.3f}, {max(every[n]):.3f}]  {B / best * 1e3:9.1f} frames/s")
        row["ce_over_plain"] = round(row[a.range]["ms_per_step"] / row["plain"]["ms_per_step"], 3)
        print(f"B {B:4d}  geometry {geom}: CE / plain = {row['ce_over_plain']:.3f}   clock probe {row['clock_probe']}")
        res["geometries"][geom] = row
        del models
        torch.cuda.empty_cache()
    if not a.no_split:
        res["split"] = {}
        for geom in vt.GEOMS:
            n = f"{geom}:{a.range}"
            s = vt._split(n, B, script=__file__)
            res["split"][n] = s
            if isinstance(s, str):
                print(f"per-kernel split, {n}: {s}")
                continue
            print(f"per-kernel split of one step, {n}, B {B} (us per step | launches per step | us per launch):")
            for k, v in s.items():
                print(f"  {k[:70]:70s} {v['us_per_step']:10.1f} {v['launches_per_step']:7.2f} {v['us_per_launch']:9.1f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
