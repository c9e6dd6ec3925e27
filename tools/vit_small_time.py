#!/usr/bin/env python3
"""ViT-Small and ViT-Tiny against ViT-Base at both geometries, timed in the same process by the method of tools/vitl_time.py.

    python tools/vit_small_time.py [--batch 256,64] [--geoms 256,384] [--rounds 5] [--replays 10] [--no-split] [--no-step]

Per geometry and batch size B (192 / 384: the largest B only): the captured forward of B frames (vt_graph_capture on fixed fp32 crops) of
    vitb / vits / vitt           the default routes (depth 12)
    vits_unfused / vitt_unfused  128 / 256 only: VB_FUSED_QKV=0 -- qk GEMM + v GEMM + vba::attn_kernel instead of the fused qkv + attention kernel
replayed in `--rounds` interleaved rounds (the order rotates every round; a round is a host-timed region of `--replays` replays behind one
synchronisation), the shader clock probed before and after (vt_probe_clock).  Printed: ms per step and frames/s (best round and [min, max]),
the per-frame time ratio to the ViT-Base figure of the SAME rounds next to the MAC ratio of oracle.vitb_oracle_torch.macs_per_frame.
The switches are read at model creation, so all variants live in one process.

The tracking step (vt_track_step on 1920 x 1080 device frames, open loop around held boxes: tools/vitb_latency.py's set-up) of the three
default models at B = 1, 8 and the largest B, 128 / 256, in interleaved rounds of its own (--no-step: skipped).

The per-kernel split of one forward (largest B, 128 / 256) comes from a child process per model under `rocprofv3 --kernel-trace --stats`
(this file with --child: it only replays), summed per kernel and divided by the steps.  --no-split, or no rocprofv3 on PATH: skipped.

One JSON line at the end.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

#: name -> (width, heads, environment at model creation)
MODELS = {"vitb": (768, 12, {}), "vits": (384, 6, {}), "vitt": (192, 3, {}),
          "vits_unfused": (384, 6, {"VB_FUSED_QKV": "0"}), "vitt_unfused": (192, 3, {"VB_FUSED_QKV": "0"})}
GEOMS = {"256": (128, 256, 2.0, 4.0), "384": (192, 384, 2.0, 5.0)}
SWITCHES = ("VB_FUSED_QKV", "VB_GEMM_NARROW", "VB_LN_FOLD")
DEPTH = 12
CHILD_REPLAYS = 6
H, W = 1080, 1920
_SD = {}


def _model(name, geom, B):
    from vittracker_amd import native, synth
    C, heads, env = MODELS[name]
    tz, tx = GEOMS[geom][:2]
    key = (C, geom)
    if key not in _SD:
        _SD[key] = synth.synth_vitb_state_dict(26, C=C, depth=DEPTH, heads=heads, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        m = native.Model(tz, tx, channels=C, heads=heads, depth=DEPTH, head_channels=256, max_batch=B, family="vit")
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    m.load_state_dict(_SD[key])
    return m


def _graph(name, geom, B):
    import torch
    from vittracker_amd import synth
    tz, tx = GEOMS[geom][:2]
    m = _model(name, geom, B)
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
    m, g, out, keep = _graph(name, "256", B)
    for _ in range(CHILD_REPLAYS):
        g.launch()
    torch.cuda.synchronize()
    print("CHILD-OK")


def _rounds(launchers, rounds, replays):
    """{name: [ms per replay of every round]}, interleaved, the order rotating."""
    import torch
    names, every = list(launchers), {n: [] for n in launchers}
    for r in range(rounds):
        k = r % len(names)
        for n in names[k:] + names[:k]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replays):
                launchers[n]()
            torch.cuda.synchronize()
            every[n].append((time.perf_counter() - t0) / replays * 1e3)
    return every


def _report(tag, B, every, base, mac_ratio):
    row = {}
    for n, v in every.items():
        best = min(v)
        row[n] = {"ms_per_step": round(best, 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)], "frames_per_s": round(B / best * 1e3, 1)}
    for n in every:
        row[n]["time_ratio_to_vitb"] = round(row[n]["ms_per_step"] / row[base]["ms_per_step"], 4)
        mr = mac_ratio.get(n.split("_")[0])
        print(f"{tag} B {B:4d}  {n:13s} {row[n]['ms_per_step']:9.4f} ms/step  [{min(every[n]):.4f}, {max(every[n]):.4f}]  {row[n]['frames_per_s']:10.1f} frames/s   "
              f"time / vitb = {row[n]['time_ratio_to_vitb']:.4f}   MACs / vitb = {mr:.4f}", flush=True)
    return row


def _steps(names, B, rounds, replays):
    """The captured tracking step of each model at batch B, 128 / 256."""
    import torch
    from frame_formats import MEAN, STD, _capture
    from vittracker_amd import native
    tz, tx, zf, xf = GEOMS["256"]
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    distinct = torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    frames = distinct[torch.arange(B, device="cuda") % 8].contiguous()
    rs = np.random.RandomState(B)
    boxes = torch.tensor([[rs.uniform(120, W - 240), rs.uniform(120, H - 240), rs.uniform(30, 90), rs.uniform(30, 90)] for _ in range(B)],
                         dtype=torch.float64).cuda()
    graphs, keep = {}, []
    for n in names:
        m = _model(n, "256", B)
        m.set_open_loop(True)
        states = boxes.clone()
        z, rf = m.crop(frames, states, zf, tz, MEAN, STD)
        m.set_template(z)
        x = torch.empty(B, 3, tx, tx, device="cuda")
        out, rec = native.Outputs(B, tx // 16, "cuda"), torch.empty(B, 5, dtype=torch.float64, device="cuda")
        keep.append((m, states, rf, x, out, rec))

        def step(cs, m=m, states=states, rf=rf, x=x, out=out, rec=rec):
            m.track_step(frames, states, xf, MEAN, STD, x, rf, out, record=rec, stream=cs)
        graphs[n] = _capture(step)
    every = _rounds({n: graphs[n].replay for n in names}, rounds, replays)
    del graphs, keep
    return every


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="256,64")
    ap.add_argument("--geoms", default="256,384")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return _child(a.child, int(a.batch))
    import torch
    import vitb384_time as vt          # its rocprofv3 child runner and CSV reduction
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import native
    batches = [int(b) for b in a.batch.split(",")]
    res = {"depth": DEPTH, "forward": {}, "mac_ratio_to_vitb": {}, "gmac_per_frame": {}}
    for geom in a.geoms.split(","):
        tz, tx = GEOMS[geom][:2]
        mac = {n: sum(ob.macs_per_frame(tz, tx, C=MODELS[n][0], depth=DEPTH).values()) for n in ("vitb", "vits", "vitt")}
        ratio = {n: v / mac["vitb"] for n, v in mac.items()}
        res["mac_ratio_to_vitb"][geom] = {n: round(v, 4) for n, v in ratio.items()}
        res["gmac_per_frame"][geom] = {n: round(v / 1e9, 3) for n, v in mac.items()}
        names = [n for n in a.models.split(",") if geom == "256" or not n.endswith("_unfused")]      # 192 / 384 has no fused route
        for B in (batches if geom == "256" else batches[:1]):
            clock0 = native.probe_clock(20000, 1)[0]
            models = {n: _graph(n, geom, B) for n in names}
            every = _rounds({n: models[n][1].launch for n in names}, a.rounds, a.replays)
            clock1 = native.probe_clock(20000, 1)[0]
            row = _report(f"forward {geom}", B, every, "vitb", ratio)
            row["clock_probe"] = [round(clock0, 1), round(clock1, 1)]
            print(f"forward {geom} B {B:4d}  clock probe {row['clock_probe']}", flush=True)
            res["forward"][f"{geom}/{B}"] = row
            for m in models.values():
                m[0].close()
            del models
            torch.cuda.empty_cache()
    if not a.no_step:
        res["track_step"] = {}
        ratio = {n: res["mac_ratio_to_vitb"].get("256", {}).get(n, float("nan")) for n in ("vitb", "vits", "vitt")}
        for B in sorted({1, 8, max(batches)}):
            every = _steps(["vitb", "vits", "vitt"], B, a.rounds, a.replays if B > 8 else 4 * a.replays)
            res["track_step"][str(B)] = _report("track_step 256", B, every, "vitb", ratio)
            torch.cuda.empty_cache()
    _SD.clear()
    if not a.no_split:
        B = max(batches)
        res["split_batch"], res["split"] = B, {}
        for n in ("vitb", "vits", "vitt"):
            s = vt._split(n, B, script=__file__)
            res["split"][n] = s
            if isinstance(s, str):
                print(f"per-kernel split, {n}: {s}")
                continue
            print(f"per-kernel split of one forward, {n}, 128 / 256, B {B} (us per step | launches per step | us per launch):")
            for k, v in s.items():
                print(f"  {k[:70]:70s} {v['us_per_step']:10.1f} {v['launches_per_step']:7.2f} {v['us_per_launch']:9.1f}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
