#!/usr/bin/env python3
"""Candidate elimination in both forms -- key masking and compacted -- against the plain ViT-Base model, at both geometries, timed in
the same process.

    python tools/vitb_ce_time.py [--batch 256] [--rounds 5] [--replays 10] [--range CTR_POINT] [--no-split]

Per geometry (OSTrack-256: 128 / 256, OSTrack-384: 192 / 384) three models on the same weights: the plain one and the published CE
configuration (CE_LOC [3, 6, 9], CE_KEEP_RATIO 0.7, --range rows) in the masked and in the compact form.  Their captured steps of --batch
frames are replayed in --rounds interleaved rounds (the order rotates; a round is a host-timed region of --replays replays behind one
synchronisation), the shader clock probed before and after, as tools/vitb384_time.py does (whose graph and rocprofv3 helpers this file
reuses).  Printed per geometry: ms per step of the three, masked / plain, compact / plain and compact / masked.  The masked form removes no
work (slower than plain at 256, where blocks 3-11 leave the fused qkv + attention kernel, about equal at 384); the compact form runs
0.77 / 0.75 of the plain model's token-blocks in every GEMM.

The per-kernel split comes from a rocprofv3 child per CE variant (masked: score, select, masked attention, zeroing among the rest;
compact: score, select, gather, the final norm's scatter, the GEMMs).  The compact form's run-time attention kernel is one name at three
frame lengths: a second child of that variant, captured as ONE chain (VT_GRAPH_CHAINS=1) so that a step's launches follow each other in
block order, gives its time per stage length from the kernel trace.  One JSON line at the end.  Reads nothing outside the repository."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vitb384_time as vt  # noqa: E402

LOC, RATIO = [3, 6, 9], [0.7, 0.7, 0.7]
RT_ATTN = "attn_stream_rt_kernel"


def _graph(variant, B):
    """variant: '<geometry>:plain', '<geometry>:<CE_TEMPLATE_RANGE>' (masked) or '<geometry>:<CE_TEMPLATE_RANGE>:compact'."""
    import torch
    from vittracker_amd import native, synth
    from vittracker_amd.model_vitb import ce_template_rows
    geom, kind, form = (variant.split(":") + ["masked"])[:3]
    tz, tx = vt.GEOMS[geom]
    m = native.Model(tz, tx, channels=768, heads=12, depth=12, head_channels=256, max_batch=B)
    m.load_state_dict(synth.synth_vitb_state_dict(26, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2))
    if kind != "plain":
        m.set_candidate_elimination(LOC, RATIO, ce_template_rows(kind, tz // 16), form=form)
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


def _attention_per_length(variant, B, lengths):
    """{frame length: us per launch} of the compact form's run-time attention kernel, from the kernel trace of a one-chain child: sorted
    by start time, a step's launches of it are blocks LOC[0] + 1 .. 11 in order.  A string says why not."""
    if shutil.which("rocprofv3") is None:
        return "rocprofv3 not on PATH"
    per_step = 11 - LOC[0]
    stage_of = [sum(1 for loc in LOC[1:] if blk > loc) for blk in range(LOC[0] + 1, 12)]      # launch index in a step -> stage (0-based)
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", variant, "--batch", str(B)], capture_output=True, text=True, timeout=900, cwd=d,
                           env=dict(os.environ, VT_GRAPH_CHAINS="1"))
        if p.returncode != 0 or "CHILD-OK" not in p.stdout:
            return "child failed: " + (p.stdout + p.stderr)[-400:]
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return "no kernel_trace.csv written"
        rows = [r for r in csv.DictReader(open(files[0])) if RT_ATTN in r.get("Kernel_Name", "")]
    if not rows or "Start_Timestamp" not in rows[0] or len(rows) % per_step:
        return f"{len(rows)} launches of {RT_ATTN} in the trace: not whole steps of {per_step}"
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = {}
    for i, r in enumerate(rows):
        us.setdefault(lengths[stage_of[i % per_step]], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {str(k): {"us_per_launch": round(sum(v) / len(v), 1), "launches_per_step": round(len(v) / (len(rows) / per_step), 2)} for k, v in us.items()}


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
        variants = {"plain": f"{geom}:plain", "masked": f"{geom}:{a.range}", "compact": f"{geom}:{a.range}:compact"}
        names = list(variants)
        clock0 = native.probe_clock(20000, 1)[0]
        models = {n: _graph(variants[n], B) for n in names}
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
            row[n] = {"ms_per_step": round(best, 3), "ms_min_max": [round(min(every[n]), 3), round(max(every[n]), 3)]}
            print(f"B {B:4d}  {geom}:{n:8s}: {best:8.3f} ms/step  [{min(every[n]):.3f}, {max(every[n]):.3f}]  {B / best * 1e3:9.1f} frames/s")
        ms = {n: row[n]["ms_per_step"] for n in names}
        row["masked_over_plain"] = round(ms["masked"] / ms["plain"], 3)
        row["compact_over_plain"] = round(ms["compact"] / ms["plain"], 3)
        row["compact_over_masked"] = round(ms["compact"] / ms["masked"], 3)
        print(f"B {B:4d}  geometry {geom}: masked / plain = {row['masked_over_plain']:.3f}   compact / plain = {row['compact_over_plain']:.3f}   "
              f"compact / masked = {row['compact_over_masked']:.3f}   clock probe {row['clock_probe']}")
        res["geometries"][geom] = row
        del models
        torch.cuda.empty_cache()
    if not a.no_split:
        res["split"], res["compact_attention"] = {}, {}
        for geom in vt.GEOMS:
            tz, tx = vt.GEOMS[geom]
            for n in (f"{geom}:{a.range}", f"{geom}:{a.range}:compact"):
                s = vt._split(n, B, script=__file__)
                res["split"][n] = s
                if isinstance(s, str):
                    print(f"per-kernel split, {n}: {s}")
                    continue
                print(f"per-kernel split of one step, {n}, B {B} (us per step | launches per step | us per launch):")
                for k, v in s.items():
                    print(f"  {k[:70]:70s} {v['us_per_step']:10.1f} {v['launches_per_step']:7.2f} {v['us_per_launch']:9.1f}")
            n = f"{geom}:{a.range}:compact"
            s = _attention_per_length(n, B, native.ce_compact_lengths((tz // 16) ** 2, (tx // 16) ** 2, RATIO))
            res["compact_attention"][n] = s
            print(f"{RT_ATTN} per frame length, {n}, B {B}, one chain: {s}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
