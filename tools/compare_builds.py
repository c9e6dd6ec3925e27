#!/usr/bin/env python3
"""Two builds of the library must produce bit-identical outputs: same device code, same forms, same arguments -> same bytes.

    python tools/compare_builds.py OTHER.so [B,B,...]                  ViT-Base forward only (k-loop variants of the GEMMs accumulate every
                                                                       output element in the same order: k-tile by k-tile)
    python tools/compare_builds.py OTHER.so --matrix [--f16 OTHER_F16.so] [--envs a,b] [--configs g128,vitb] [--batches 1,96] [--out FILE]

--matrix: one child process per (library, environment); the current build against OTHER.  Environments: the default, every entry of
VARIANTS in tests/test_gpu_variants.py, VT_TRACK_U8=0, VT_GRAPH_CHAINS=2 and 3, and the crop forms tests/test_gpu_patch_u8.py forces
(crop_bytes, crop_fast_off, crop_band_off, crop_band4, crop_band2, crop_band4_unaligned), and the ViT-Base attention routes the default never
takes: vb_unfused (attn_kernel<320, 64>), vb_stream (attn_stream_kernel<320>), vb_nofold.  Configs: g128, g256, generic (112, 224), f16 (the f16
build at G128, needs --f16), vitb, vitb384 (192 / 384, depth 12), vitbce, vitbce384 (candidate elimination, below), vitpoints (below).  Batches 1, 5, 7, 96, 256
(vitb 1, 96; vitb384 1, 5; vitbce, vitbce384 1, 5).  Entries: forward, forward on the cached template, forward_u8,
capture + replay, track_step, track_step_frames, track_step_images (NV12, and I420 under BT.709: the other body of the band image kernel)
-- four steps each for the tracker entries, so the state
feeds back.  A child prints sha256 over the bytes of all six outputs (+ states and record) per case, or the library's error code where it
refuses the case: both libraries must refuse with the same code.  Children run one after the other.

vitbce / vitbce384: a depth-4 ViT-Base model with CE_LOC [0, 1, 2] and keep ratios 0.7 at either geometry, in the masked and the compact
form, under CE_TEMPLATE_RANGE CTR_POINT (the plain score loop), ALL (the MFMA score) and ALL with VB_CE_SCORE_PLAIN=1 (the plain loop at 64 /
144 rows); entries forward and capture + replay.  The hash covers the six outputs and both arrays of ce_result as bytes, NaN scores included.

vitpoints: the patch-16 ViT at every model point -- shallow models (depth 2) at each of the four widths (192 / 3, 384 / 6, 768 / 12,
1024 / 16), both geometries, both precisions (bf16, fp32), batches 1 and 3 (whatever --batches says).  Not among the default --configs (256
cases per environment, and only the ViT path's own environments touch it): ask for it by name.  Entries: forward, forward_u8 with a
given template, forward and forward_u8 on the cached template, set_template_slots followed by forward(None, x), capture + two replays, and the
stage API stem -> blocks(tokens, nblocks=1, want_resid=True) -> blocks(resid) -> head(feat), every tensor it returns in the hash: that chain
runs the LayerNorm kernels on outside tokens, the feature-to-map kernels on outside features and the final norm alone."""
import argparse, json, os, subprocess, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
VITB_BATCHES = {"vitb": (1, 96), "vitb384": (1, 5), "vitbce": (1, 5), "vitbce384": (1, 5)}      # the ViT-Base configs and the batches of --batches each of them runs
CE_GEOMS = {"vitbce": (128, 256), "vitbce384": (192, 384)}      # the candidate-elimination configs
CE_LOC, CE_RATIO, CE_DEPTH = [0, 1, 2], [0.7, 0.7, 0.7], 4
CE_RANGES = (("CTR_POINT", "0"), ("ALL", "0"), ("ALL", "1"))      # (CE_TEMPLATE_RANGE, VB_CE_SCORE_PLAIN: read when the model is created)
# the vitpoints config: (channels, heads) of the four model points, the two geometries, the two precisions, its depth and batches
POINTS, POINT_GEOMS, POINT_PRECISIONS, POINT_DEPTH, POINT_BATCHES = ((192, 3), (384, 6), (768, 12), (1024, 16)), ((128, 256), (192, 384)), ("bf16", "fp32"), 2, (1, 3)

VITB_CHILD = r"""
import sys, json, hashlib
sys.path.insert(0, %(root)r)
import torch
from vittracker_amd import native, synth
if %(lib)r: native.LIB_PATH = %(lib)r
res = {}
sd = synth.synth_vitb_state_dict(26)
for B in %(sizes)r:
    m = native.Model(128, 256, channels=768, heads=12, depth=12, head_channels=256, max_batch=B)
    m.load_state_dict(sd)
    z, x = synth.synth_inputs(B + 1, B, 128, 256)
    o = m.forward(torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda())
    h = hashlib.sha256()
    for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf"):
        h.update(getattr(o, k).cpu().numpy().tobytes())
    res[B] = h.hexdigest()[:16]
    m.close()
print("RESULT " + json.dumps(res))
"""


def child(configs, batches):
    """Runs in the child process (the library and the environment are fixed by then)."""
    import hashlib, re
    import numpy as np, torch
    from vittracker_amd import native, synth
    from vittracker_amd.native import FrameTable, Image, ImageTable, Outputs
    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    res = {}

    def digest(out, *more):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for k in KEYS:
            h.update(getattr(out, k).cpu().numpy().tobytes())
        for t in more:
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def case(name, fn):
        try:
            res[name] = fn()
        except native.VtError as e:      # refused: the error code, which the other library must return too
            code = re.search(r"\((-?\d+)\)", str(e))
            res[name] = "refused " + (code.group(1) if code else str(e)[:60])

    def ce_cases(cfg):
        from vittracker_amd.model_vitb import ce_template_rows
        tz, tx = CE_GEOMS[cfg]
        sd = synth.synth_vitb_state_dict(26, depth=CE_DEPTH, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
        for B in (b for b in batches if b in VITB_BATCHES[cfg]):
            z, x = synth.synth_inputs(40 + B, B, tz, tx)
            zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
            for form in ("masked", "compact"):
                for trange, plain in CE_RANGES:
                    def make():
                        os.environ["VB_CE_SCORE_PLAIN"] = plain
                        m = native.Model(tz, tx, channels=768, heads=12, depth=CE_DEPTH, head_channels=256, max_batch=B)
                        m.load_state_dict(sd)
                        m.set_candidate_elimination(CE_LOC, CE_RATIO, ce_template_rows(trange, tz // 16), form=form)
                        return m
                    tag = f"{cfg}/{form}/{trange}{'+plain' if plain == '1' else ''}/B{B}/"

                    def forward():
                        m = make()
                        try:
                            return digest(m.forward(zd, xd), *m.ce_result(B))
                        finally:
                            m.close()

                    def captured():
                        m = make()
                        try:
                            g, out = m.capture(zd, xd)
                            g.launch()
                            g.launch()
                            h = digest(out, *m.ce_result(B))
                            del g
                            return h
                        finally:
                            m.close()
                    case(tag + "forward", forward)
                    case(tag + "capture", captured)
        os.environ.pop("VB_CE_SCORE_PLAIN", None)

    def point_cases():
        for (ch, heads), (tz, tx), prec in ((p, g, q) for p in POINTS for g in POINT_GEOMS for q in POINT_PRECISIONS):
            sd = synth.synth_vitb_state_dict(26, C=ch, depth=POINT_DEPTH, heads=heads, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
            for B in POINT_BATCHES:
                m = native.Model(tz, tx, channels=ch, heads=heads, depth=POINT_DEPTH, head_channels=256, max_batch=B, family="vit")
                m.load_state_dict(sd)
                m.set_precision(prec)
                z, x = synth.synth_inputs(60 + B, B, tz, tx)
                z2 = synth.synth_inputs(80 + B, B, tz, tx)[0]
                zd, xd, z2d = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(z2).cuda()
                xp = torch.from_numpy(synth.synth_patches(9 + B, B, tx)).cuda()
                tag = f"vitpoints/{ch}/{tz}-{tx}/{prec}/B{B}/"
                case(tag + "forward", lambda: digest(m.forward(zd, xd)))
                case(tag + "forward_u8_given", lambda: digest(m.forward_u8(zd, xp)))
                case(tag + "set_template", lambda: m.set_template(zd) or "ok")
                case(tag + "forward_cached", lambda: digest(m.forward(None, xd)))
                case(tag + "forward_u8", lambda: digest(m.forward_u8(None, xp)))

                def slots():      # the last slot alone takes another template
                    m.set_template_slots(z2d[B - 1:], [B - 1])
                    return digest(m.forward(None, xd))
                case(tag + "template_slots", slots)

                def stages():
                    tok = m.stem(zd, xd)
                    feat1, resid = m.blocks(tok, nblocks=1, want_resid=True)
                    feat = m.blocks(resid)
                    return digest(m.head(feat), tok, feat1, resid, feat)
                case(tag + "stages", stages)

                def captured():
                    g, out = m.capture(zd, xd)
                    g.launch()
                    g.launch()
                    h = digest(out)
                    del g
                    return h
                case(tag + "capture", captured)
                m.close()

    for cfg in configs:
        if cfg in CE_GEOMS:
            ce_cases(cfg)
            continue
        if cfg == "vitpoints":
            point_cases()
            continue
        tz, tx = {"g128": (64, 128), "g256": (128, 256), "generic": (112, 224), "f16": (64, 128), "vitb": (128, 256), "vitb384": (192, 384)}[cfg]
        if cfg in VITB_BATCHES:
            sd = synth.synth_vitb_state_dict(26, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
            make = lambda B: native.Model(tz, tx, channels=768, heads=12, depth=12, head_channels=256, max_batch=B)
        else:
            sd = synth.synth_state_dict(5, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
            make = lambda B: native.Model(tz, tx, max_batch=B, precision="f16" if cfg == "f16" else "f32")
        for B in ([b for b in batches if b in VITB_BATCHES[cfg]] if cfg in VITB_BATCHES else batches):
            m = make(B)
            m.load_state_dict(sd)
            z, x = synth.synth_inputs(40 + B, B, tz, tx)
            zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
            xp = torch.from_numpy(synth.synth_patches(7 + B, B, tx)).cuda()
            rs = np.random.RandomState(900 + B)
            H, W = 120, 160
            frames = [torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda() for _ in range(4)]
            luma = [torch.from_numpy(rs.randint(0, 256, (B, H, W)).astype(np.uint8)).cuda() for _ in range(4)]
            chroma = [torch.from_numpy(rs.randint(0, 256, (B, H // 2, W // 2, 2)).astype(np.uint8)).cuda() for _ in range(4)]
            planar = [c.permute(0, 3, 1, 2).contiguous() for c in chroma]      # (B, 2, H/2, W/2): a frame's U and V planes back to back
            box0 = torch.tensor([[rs.uniform(0, 90), rs.uniform(0, 60), rs.uniform(10, 60), rs.uniform(10, 50)] for _ in range(B)],
                                dtype=torch.float64).cuda()
            tag = f"{cfg}/B{B}/"
            case(tag + "forward", lambda: digest(m.forward(zd, xd)))
            case(tag + "forward_u8_given", lambda: digest(m.forward_u8(zd, xp)))

            def captured():
                g, out = m.capture(zd, xd)
                g.launch()
                g.launch()
                return digest(out)
            case(tag + "capture", captured)
            case(tag + "set_template", lambda: m.set_template(zd) or "ok")
            case(tag + "forward_cached", lambda: digest(m.forward(None, xd)))
            case(tag + "forward_u8", lambda: digest(m.forward_u8(None, xp)))

            def captured_cached():
                g, out = m.capture(None, xd)
                g.launch()
                return digest(out)
            case(tag + "capture_cached", captured_cached)

            def tracked(kind):
                st = box0.clone()
                ws = torch.empty(B, 3, tx, tx, device="cuda")
                rf = torch.empty(B, dtype=torch.float64, device="cuda")
                out = Outputs(B, tx // 16, "cuda")
                recs = []
                for t in range(4):
                    rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
                    if kind == "dense":
                        m.track_step(frames[t], st, 4.0, MEAN, STD, ws, rf, out, record=rec)
                    elif kind == "frames":
                        tab = FrameTable(B, "cuda")
                        for b in range(B):
                            tab.set_tensor(b, frames[t][b])
                        tab.upload()
                        m.track_step_frames(tab, st, 4.0, MEAN, STD, ws, rf, out, record=rec)
                    else:
                        tab = ImageTable(B, "cuda")
                        for b in range(B):
                            if kind == "i420":      # the NV12 frame's U and V as two planes
                                tab.set_image(b, Image.i420(luma[t][b], planar[t][b, 0], planar[t][b, 1], matrix="bt709"))
                            else:
                                tab.set_image(b, Image.nv12(luma[t][b], chroma[t][b]))
                        tab.upload()
                        m.track_step_images(tab, st, 4.0, MEAN, STD, ws, rf, out, record=rec)
                    recs.append(rec)
                return digest(out, st, *recs)
            case(tag + "track_step", lambda: tracked("dense"))
            case(tag + "track_step_frames", lambda: tracked("frames"))
            case(tag + "track_step_images", lambda: tracked("images"))
            case(tag + "track_step_images_i420", lambda: tracked("i420"))
            m.close()
    print("RESULT " + json.dumps(res))


def environments():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    ns = {}
    src = open(os.path.join(ROOT, "tests", "test_gpu_variants.py")).read()
    start = src.index("VARIANTS = {")
    exec(src[start:src.index("\n}\n", start) + 3], ns)      # the dict literal only: the module itself needs pytest and a GPU
    envs = {"default": {}}
    envs.update(ns["VARIANTS"])
    envs.update({"track_u8_off": {"VT_TRACK_U8": "0"}, "chains2": {"VT_GRAPH_CHAINS": "2"}, "chains3": {"VT_GRAPH_CHAINS": "3"}})
    envs.update({"crop_bytes": {"VT_CROP_BYTES": "1"}, "crop_fast_off": {"VT_CROP_FAST": "0"}, "crop_band_off": {"VT_CROP_BAND": "0"},
                 "crop_band4": {"VT_CROP_BAND": "-4"}, "crop_band2": {"VT_CROP_BAND": "-2"},
                 "crop_band4_unaligned": {"VT_CROP_BAND": "-4", "VT_CROP_ALIGNED": "0"}})
    envs.update({"vb_unfused": {"VB_FUSED_QKV": "0"}, "vb_stream": {"VB_FUSED_QKV": "0", "VB_ATTN_STREAM": "1"},
                 "vb_nofold": {"VB_LN_FOLD": "0", "VB_FUSED_QKV": "0"}})
    return envs


def run_child(code, env=None):
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1200, env=env)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode or not line:
        return None, (p.returncode, p.stdout[-300:], p.stderr[-800:])
    return json.loads(line[0][7:]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("sizes", nargs="?", default="1,5,37,96,256")
    ap.add_argument("--matrix", action="store_true")
    ap.add_argument("--f16", default="")
    ap.add_argument("--envs", default="")
    ap.add_argument("--configs", default="g128,g256,generic,f16,vitb,vitb384,vitbce,vitbce384")
    ap.add_argument("--batches", default="1,5,7,96,256")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    other = os.path.abspath(a.other)
    if not a.matrix:
        out = {}
        for name, lib in (("cur", ""), ("other", other)):
            out[name], err = run_child(VITB_CHILD % {"root": ROOT, "lib": lib, "sizes": [int(v) for v in a.sizes.split(",")]})
            if err:
                print(name, "FAILED", *err); sys.exit(2)
        same = out["cur"] == out["other"]
        print(out)
        print("builds agree bit for bit:", same)
        sys.exit(0 if same else 1)
    envs = environments()
    names = a.envs.split(",") if a.envs else list(envs)
    configs = [c for c in a.configs.split(",") if c != "f16" or a.f16]
    batches = [int(v) for v in a.batches.split(",")]
    report, bad = {}, 0
    for name in names:
        got = {}
        for which, lib, lib16 in (("cur", "", ""), ("other", other, os.path.abspath(a.f16) if a.f16 else "")):
            code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nfrom vittracker_amd import native\n" % (ROOT, os.path.dirname(__file__))
                    + ("native.LIB_PATH = %r\n" % lib if lib else "") + ("native.LIB_PATH_F16 = %r\n" % lib16 if lib16 else "")
                    + "import compare_builds\ncompare_builds.child(%r, %r)\n" % (configs, batches))
            env = {k: v for k, v in os.environ.items() if k != "VITTRACK_LIB"}
            env.update(envs[name])
            got[which], err = run_child(code, env)
            if err:
                print(name, which, "FAILED", *err, flush=True)
                # a child that died may have faulted the device: nothing more is started
                if a.out:
                    json.dump(report, open(a.out, "w"), indent=1)
                sys.exit(2)
        diff = sorted(k for k in got["cur"] if got["cur"][k] != got["other"].get(k))
        refused = sorted(k for k, v in got["cur"].items() if str(v).startswith("refused"))
        report[name] = {"cases": len(got["cur"]), "differ": diff, "refused_by_both": [k for k in refused if k not in diff], "hashes": got["cur"]}
        bad += len(diff)
        print(f"{name}: {len(got['cur'])} cases, {len(diff)} differ, {len(refused)} refused {diff[:6]}", flush=True)
        if a.out:
            json.dump(report, open(a.out, "w"), indent=1)
    print("builds agree bit for bit:", bad == 0)
    sys.exit(0 if bad == 0 else 1)


if __name__ == "__main__":
    main()
