#!/usr/bin/env python3
"""Pixel formats on the device: what reading NV12 / NV21, BGR and RGBA / BGRA directly costs against RGB, and what the
other layouts and colour rows (P010, I420, YUYV / UYVY, GRAY8; BT.709, full range) cost against NV12 BT.601.

    python tools/frame_formats.py [--batch 256] [--rounds 5] [--reps 20] [--distinct 32] [--sections crop,step,small,convert,new,parent,planar,wide]
                                  [--parent-lib OTHER.so]

Fixed seeds, 1920 x 1080 frames (`--distinct` different frames, cycled over the sequences) with 30-120 px boxes:
  crop_us[T][form]        B = 256: the uint8 table crop per launch, T = 128 and 256: "rgb_frames" is vt_crop_u8_frames on the RGB
                          frames, every other form vt_crop_u8_images on that format
  step_us[G][form]        B = 256: the G128 / G256 tracker step in open loop (vt_set_open_loop): vt_track_step_frames on RGB against
                          vt_track_step_images on NV12
  small_batch_us          B = 1 (the plugin's per-frame step and small template crops, which take crop_image_kernel: single-byte
                          tap fetches): the T = 128 uint8 crop and the G128 step, frame route on RGB against the image route
  convert_step_us[G]      B = 256: the caller's alternative without this route: the whole NV12 frames converted to RGB with unfused
                          int32 torch ops (one kernel per op), then vt_track_step_frames
  new_crop_us[T][form]    (section "new") B = 256: the uint8 table crop of every added layout / colour row, NV12 BT.601 and the RGB
                          frame route in the same interleaved rounds; ratio_vs_nv12 and the kernel family each form runs
  parent_ab               (section "parent", --parent-lib: the parent commit's libvittrack_hip.so) the six first layouts' families and
                          the added ones (NV12 BT.709, P010, I420, YUYV, GRAY8: the second body of the band image kernel), crops
                          (T = 128 / 256) and G128 / G256 steps at B = 256, this build and the parent's loaded side by side in ONE
                          process and timed in the same interleaved rounds: per form the median and the [min, max] over the rounds;
                          inside_parent_range = this build's median lies inside the parent's own round-to-round range
  planar                  (section "planar") B = 256 on ONE (B, 3, H, W) uint8 tensor, every sequence its own frame: crop_us[T][form] = the
                          uint8 table crop of RGBP / BGRP (native.images_from_chw), I444 and I422 (the same planes read as Y, U, V) next to
                          I420 (the byte-fetch family they share) and the RGB frame route on the permuted copy; step_us[G][form] = the
                          open-loop G128 / G256 step on those tables; permute_step_us[G] = what a caller does without the layout --
                          hwc.copy_(chw.permute(0, 2, 3, 1)) inside the captured, timed graph, then vt_track_step_frames -- against the
                          step on the CHW frames (ratio = permute + step over CHW step)
  wide                    (section "wide") B = 256: crop_us[T][form] = the uint8 table crop of I010, I210, I410 (the 16-bit fetch family), P210,
                          NV16 and GRAY16 (byte fetch) next to I420 (byte fetch), P010 (aligned windows) and the RGB frame route in the same
                          interleaved rounds, ratio_vs_i420 / ratio_vs_rgb_frames; step_us[G][form] = the open-loop G128 / G256 step on
                          those tables; convert_step_us[G] = what a caller does without the layout -- the whole I010 frames shifted down
                          to bytes ((t >> 2).to(uint8), two torch kernels) inside the captured, timed graph, then the step on the I420
                          frames -- against the step on the I010 frames (ratio = convert + step over I010 step)
Method: every form is a captured graph (`--reps` launches for a crop, one step for a step; outputs preallocated, no host work
inside); the forms are timed in `--rounds` interleaved rounds (the order rotates every round), each a host-timed region of replays
with one synchronisation, and the best round of each form is reported.  The shader clock is probed (vt_probe_clock, a dense MFMA
loop) before and after.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
H, W = 1080, 1920
FORMATS = ("rgb", "bgr", "rgba", "bgra", "nv12", "nv21")


def _model(geom, B):
    from vittracker_amd import native, synth
    m = native.Model(geom // 2, geom, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(0, len_z=(geom // 32) ** 2, len_x=(geom // 16) ** 2))
    return m


def _capture(fn):
    """fn(stream) captured into a graph (after one eager warm-up call)."""
    import torch
    fn(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        fn(torch.cuda.current_stream())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return g


def _interleaved(graphs, per_replay, rounds, replays, all_rounds=False):
    """{name: best us per unit} over `rounds` interleaved rounds of `replays` replays each; `per_replay` units per replay.
    all_rounds: {name: [us of every round]} instead."""
    import torch
    best, every = {}, {}
    names = list(graphs)
    for g in graphs.values():           # warm-up
        g.replay()
    torch.cuda.synchronize()
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            g = graphs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replays):
                g.replay()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / (replays * per_replay) * 1e6
            best[name] = min(best.get(name, 1e30), us)
            every.setdefault(name, []).append(round(us, 2))
    if all_rounds:
        return every
    return {k: round(v, 2) for k, v in best.items()}


def _planes(fmt, n, g):
    """n frames in `fmt`, as device tensors (random bytes: the content does not change the cost)."""
    import torch
    mk = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g)      # noqa: E731
    if fmt in ("rgb", "bgr"):
        return [(mk(H, W, 3),) for _ in range(n)]
    if fmt in ("rgba", "bgra"):
        return [(mk(H, W, 4),) for _ in range(n)]
    return [(mk(H, W), mk(H // 2, W // 2, 2)) for _ in range(n)]


#: the added layouts and colour rows: name -> (constructor, keywords, planes of an H x W frame as uint8 shapes, the band kernel's family)
NEW_FORMS = {
    "nv12_709": ("nv12", dict(matrix="bt709"), lambda: ((H, W), (H // 2, W // 2, 2)), "NV aligned windows, coefficients from registers"),
    "nv12_601_full": ("nv12", dict(range="full"), lambda: ((H, W), (H // 2, W // 2, 2)), "NV aligned windows, coefficients from registers"),
    "nv21_709_full": ("nv21", dict(matrix="bt709", range="full"), lambda: ((H, W), (H // 2, W // 2, 2)), "NV aligned windows, coefficients from registers"),
    "p010_709": ("p010", dict(matrix="bt709"), lambda: ((H, 2 * W), (H // 2, W // 2, 4)), "P010 aligned windows (8 + 12 bytes)"),
    "i420": ("i420_buffer", {}, lambda: ((3 * H // 2, W),), "byte fetch"),
    "i420_709": ("i420_buffer", dict(matrix="bt709"), lambda: ((3 * H // 2, W),), "byte fetch"),
    "yuyv": ("yuyv", {}, lambda: ((H, W, 2),), "byte fetch"),
    "uyvy_709": ("uyvy", dict(matrix="bt709"), lambda: ((H, W, 2),), "byte fetch"),
    "gray": ("gray", {}, lambda: ((H, W),), "byte fetch (luma only)"),
}


def _new_tables(B, n, g):
    """{form: ImageTable} of the added forms, `n` distinct random frames each, cycled over B sequences."""
    import torch
    from vittracker_amd.native import Image, ImageTable
    tabs, keep = {}, []
    for name, (ctor, kw, shapes, _) in NEW_FORMS.items():
        frames = [tuple(torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g) for s in shapes()) for _ in range(n)]
        keep.append(frames)
        t = ImageTable(B, "cuda")
        for b in range(B):
            t.set_image(b, getattr(Image, ctor)(*frames[b % n], **kw))
        t.upload()
        tabs[name] = t
    return tabs, keep


def _second_native(lib_path):
    """vittracker_amd.native once more, as a module of its own bound to another build of the library: both in one process."""
    import importlib.util
    from vittracker_amd import native
    spec = importlib.util.spec_from_file_location("vittracker_amd.native_other", native.__file__)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(lib_path)
    return mod


def _stats(rounds):
    v = sorted(rounds)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def _parent_ab(a, B, n, g, states):
    """The formats that existed, this build against the parent's library, in the same interleaved rounds."""
    import torch
    from vittracker_amd import native, synth
    other = _second_native(a.parent_lib)
    forms = ("rgb", "bgr", "rgba", "nv12")
    new_forms = ("nv12_709", "p010_709", "i420", "yuyv", "gray")      # the rows that reach crop_band_image_ext, one per family and more
    frames = {f: _planes(f, n, g) for f in forms}
    for f in new_forms:
        frames[f] = [tuple(torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g) for s in NEW_FORMS[f][2]()) for _ in range(n)]
    res = {"crop_us": {}, "step_us": {}}

    def tables(nat):
        tabs = {}
        for f in forms:
            t = nat.ImageTable(B, "cuda")
            for b in range(B):
                t.set_image(b, getattr(nat.Image, f)(*frames[f][b % n]))
            t.upload()
            tabs[f] = t
        for f in new_forms:
            t = nat.ImageTable(B, "cuda")
            for b in range(B):
                t.set_image(b, getattr(nat.Image, NEW_FORMS[f][0])(*frames[f][b % n], **NEW_FORMS[f][1]))
            t.upload()
            tabs[f] = t
        ft = nat.FrameTable(B, "cuda")
        for b in range(B):
            ft.set_tensor(b, frames["rgb"][b % n][0])
        ft.upload()
        return tabs, ft

    def model(nat, geom):
        m = nat.Model(geom // 2, geom, max_batch=B)
        m.load_state_dict(synth.synth_state_dict(0, len_z=(geom // 32) ** 2, len_x=(geom // 16) ** 2))
        return m
    sides = {"this": (native,) + tables(native), "parent": (other,) + tables(other)}
    identical = True
    mods = {k: model(v[0], 128) for k, v in sides.items()}
    for T in (128, 256):
        graphs, outs = {}, {}
        for side, (nat, tabs, ft) in sides.items():
            m = mods[side]
            for name, t in [("rgb_frames", ft)] + list(tabs.items()):
                o = torch.empty(B, T, T, 3, dtype=torch.uint8, device="cuda")
                rf = torch.empty(B, dtype=torch.float64, device="cuda")
                outs[(side, name)] = (o, rf)
                call = m.crop_u8_frames if name == "rgb_frames" else m.crop_u8_images

                def fn(cs, call=call, t=t, o=o, rf=rf):
                    for _ in range(a.reps):
                        call(t, states, 4.0, T, out=o, resize_factor=rf, stream=cs)
                graphs[f"{side}:{name}"] = _capture(fn)
        rounds = _interleaved(graphs, a.reps, a.rounds, a.replays, all_rounds=True)
        row = {}
        for name in ["rgb_frames"] + list(forms) + list(new_forms):
            identical = identical and torch.equal(outs[("this", name)][0], outs[("parent", name)][0]) and \
                torch.equal(outs[("this", name)][1], outs[("parent", name)][1])
            me, pa = _stats(rounds[f"this:{name}"]), _stats(rounds[f"parent:{name}"])
            row[name] = {"this": me, "parent": pa, "inside_parent_range": pa["min"] <= me["median"] <= pa["max"]}
        res["crop_us"][str(T)] = row
    del mods
    for S in (128, 256):
        graphs, keep = {}, []
        for side, (nat, tabs, ft) in sides.items():
            m = model(nat, S)
            m.set_open_loop(True)
            m.set_template(torch.zeros(B, 3, S // 2, S // 2, device="cuda"))
            x = torch.empty(B, 3, S, S, device="cuda")
            rf = torch.empty(B, dtype=torch.float64, device="cuda")
            out = nat.Outputs(B, S // 16, "cuda")
            rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
            keep.append((m, x, rf, out, rec))
            for name, (f, t) in {"rgb_frames": (m.track_step_frames, ft), "nv12": (m.track_step_images, tabs["nv12"])}.items():
                graphs[f"{side}:{name}"] = _capture(lambda cs, f=f, t=t, x=x, rf=rf, out=out, rec=rec:
                                                    f(t, states, 4.0, MEAN, STD, x, rf, out, record=rec, stream=cs))
        rounds = _interleaved(graphs, 1, a.rounds, a.replays * 5, all_rounds=True)
        row = {}
        for name in ("rgb_frames", "nv12"):
            me, pa = _stats(rounds[f"this:{name}"]), _stats(rounds[f"parent:{name}"])
            row[name] = {"this": me, "parent": pa, "inside_parent_range": pa["min"] <= me["median"] <= pa["max"]}
        identical = identical and torch.equal(keep[0][4], keep[1][4])
        res["step_us"][f"G{S}"] = row
        del graphs, keep
    res["outputs_bit_identical"] = bool(identical)
    return res


def _planar(a, B, g, states):
    """Section planar: one (B, 3, H, W) batch as RGBP / BGRP / I444 / I422 tables, I420 and the permuted RGB copy beside it."""
    import torch
    from vittracker_amd import native
    from vittracker_amd.native import FrameTable, Image, ImageTable
    chw = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    i420 = [torch.randint(0, 256, (3 * H // 2, W), dtype=torch.uint8, device="cuda", generator=g) for _ in range(B)]
    forms = {"rgbp": native.images_from_chw(chw), "bgrp": native.images_from_chw(chw, "bgr"),
             "i444": [Image.i444(f[0], f[1], f[2]) for f in chw],
             "i422": [Image.i422(f[0], f[1, :, :W // 2], f[2, :, :W // 2]) for f in chw],      # chroma rows at pitch W, planes W H apart
             "i420": [Image.i420_buffer(f) for f in i420]}
    tabs = {k: ImageTable.of(v) for k, v in forms.items()}
    ft = FrameTable(B, "cuda")
    for b in range(B):
        ft.set_tensor(b, hwc[b])
    ft.upload()
    res = {"crop_us": {}, "step_us": {}, "permute_step_us": {}, "batch_bytes": int(chw.numel())}
    m = _model(128, B)
    for T in (128, 256):
        graphs, outs = {}, []
        for name, t in [("rgb_frames", ft)] + list(tabs.items()):
            o = torch.empty(B, T, T, 3, dtype=torch.uint8, device="cuda")
            rf = torch.empty(B, dtype=torch.float64, device="cuda")
            outs.append((o, rf))
            call = m.crop_u8_frames if name == "rgb_frames" else m.crop_u8_images

            def fn(cs, call=call, t=t, o=o, rf=rf):
                for _ in range(a.reps):
                    call(t, states, 4.0, T, out=o, resize_factor=rf, stream=cs)
            graphs[name] = _capture(fn)
        rounds = _interleaved(graphs, a.reps, a.rounds, a.replays, all_rounds=True)
        row = {k: _stats(v) for k, v in rounds.items()}
        row["ratio_vs_rgb_frames"] = {k: round(min(v) / min(rounds["rgb_frames"]), 3) for k, v in rounds.items()}
        row["ratio_vs_i420"] = {k: round(min(v) / min(rounds["i420"]), 3) for k, v in rounds.items()}
        row["rgbp_equals_rgb_frames"] = bool(torch.equal(outs[0][0], outs[1][0]))
        res["crop_us"][str(T)] = row
    del m, graphs
    for S in (128, 256):
        m = _model(S, B)
        step_forms = {"rgb_frames": (m.track_step_frames, ft)}
        step_forms.update({k: (m.track_step_images, tabs[k]) for k in ("rgbp", "i444", "i422")})
        graphs, (x, rf, out, rec) = _step_graphs(m, S, B, states, step_forms)

        def permute_then_step(cs):      # today's caller: the whole batch transposed, then the RGB step on it
            hwc.copy_(chw.permute(0, 2, 3, 1))
            m.track_step_frames(ft, states, 4.0, MEAN, STD, x, rf, out, record=rec, stream=cs)
        graphs["permute_then_step"] = _capture(permute_then_step)
        graphs["permute_alone"] = _capture(lambda cs: hwc.copy_(chw.permute(0, 2, 3, 1)))
        rounds = _interleaved(graphs, 1, a.rounds, a.replays * 5, all_rounds=True)
        row = {k: _stats(v) for k, v in rounds.items() if not k.startswith("permute")}
        row["ratio_vs_rgb_frames"] = {k: round(min(v) / min(rounds["rgb_frames"]), 3) for k, v in rounds.items() if not k.startswith("permute")}
        res["step_us"][f"G{S}"] = row
        res["permute_step_us"][f"G{S}"] = {"permute_then_step": _stats(rounds["permute_then_step"]), "permute_alone": _stats(rounds["permute_alone"]),
                                           "chw_step": _stats(rounds["rgbp"]),
                                           "ratio": round(min(rounds["permute_then_step"]) / min(rounds["rgbp"]), 2)}
        del m, graphs
    return res


def _wide(a, B, n, g, states):
    """Section wide: the 16-bit and two-plane layouts beside I420, P010 and the RGB frame route; the I010 step against shifting whole
    frames down to I420 first."""
    import torch
    from vittracker_amd.native import FrameTable, Image, ImageTable
    mk = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g)      # noqa: E731
    # every sequence its own I010 frame, in one (B, 3H/2, W) buffer of 16-bit words laid out as an I420 buffer is; its 8-bit twin
    w16 = torch.randint(0, 1024, (B, 3 * H // 2, W), dtype=torch.int16, device="cuda", generator=g)
    tmp16, b8 = torch.empty_like(w16), torch.empty(B, 3 * H // 2, W, dtype=torch.uint8, device="cuda")

    def convert():
        torch.bitwise_right_shift(w16, 2, out=tmp16)      # (t >> 2).to(torch.uint8) without an allocation
        b8.copy_(tmp16)
    convert()

    def i010(f):
        c = f[H:].reshape(H, W // 2)
        return Image.i010(f[:H], c[:H // 2], c[H // 2:])
    keep = {k: [mk(*sh) for _ in range(n)] for k, sh in (("y16", (H, 2 * W)), ("y8", (H, W)), ("c210", (2 * H, W)), ("c410", (2 * H, 2 * W)),
                                                        ("p210", (H, W // 2, 4)), ("nv16", (H, W // 2, 2)), ("p010", (H // 2, W // 2, 4)),
                                                        ("rgb", (H, W, 3)))}
    k = lambda name, b: keep[name][b % n]      # noqa: E731
    forms = {"i420": [Image.i420_buffer(f) for f in b8],
             "p010": [Image.p010(k("y16", b), k("p010", b)) for b in range(B)],
             "i010": [i010(f) for f in w16],
             "i210": [Image.yuv16(k("y16", b), k("c210", b)[:H], k("c210", b)[H:], depth=10, sub="422") for b in range(B)],
             "i410": [Image.yuv16(k("y16", b), k("c410", b)[:H], k("c410", b)[H:], depth=10, sub="444") for b in range(B)],
             "p210": [Image.p210(k("y16", b), k("p210", b)) for b in range(B)],
             "nv16": [Image.nv16(k("y8", b), k("nv16", b)) for b in range(B)],
             "gray16": [Image.gray16(k("y16", b), depth=16) for b in range(B)]}
    tabs = {name: ImageTable.of(v) for name, v in forms.items()}
    ft = FrameTable(B, "cuda")
    for b in range(B):
        ft.set_tensor(b, k("rgb", b))
    ft.upload()
    res = {"crop_us": {}, "step_us": {}, "convert_step_us": {},
           "family": {"i420": "byte fetch", "p010": "P010 aligned windows", "i010": "16-bit fetch", "i210": "16-bit fetch", "i410": "16-bit fetch",
                      "p210": "byte fetch (high bytes)", "nv16": "byte fetch", "gray16": "byte fetch (high bytes, luma only)"}}
    m = _model(128, B)
    for T in (128, 256):
        graphs, outs = {}, []
        for name, t in [("rgb_frames", ft)] + list(tabs.items()):
            o = torch.empty(B, T, T, 3, dtype=torch.uint8, device="cuda")
            rf = torch.empty(B, dtype=torch.float64, device="cuda")
            outs.append((o, rf))
            call = m.crop_u8_frames if name == "rgb_frames" else m.crop_u8_images

            def fn(cs, call=call, t=t, o=o, rf=rf):
                for _ in range(a.reps):
                    call(t, states, 4.0, T, out=o, resize_factor=rf, stream=cs)
            graphs[name] = _capture(fn)
        rounds = _interleaved(graphs, a.reps, a.rounds, a.replays, all_rounds=True)
        row = {name: _stats(v) for name, v in rounds.items()}
        row["ratio_vs_rgb_frames"] = {name: round(min(v) / min(rounds["rgb_frames"]), 3) for name, v in rounds.items()}
        row["ratio_vs_i420"] = {name: round(min(v) / min(rounds["i420"]), 3) for name, v in rounds.items()}
        names = ["rgb_frames"] + list(tabs)
        row["i010_equals_i420_of_its_top_bits"] = bool(torch.equal(outs[names.index("i010")][0], outs[names.index("i420")][0]))
        res["crop_us"][str(T)] = row
    del m, graphs
    for S in (128, 256):
        m = _model(S, B)
        step_forms = {"rgb_frames": (m.track_step_frames, ft)}
        step_forms.update({name: (m.track_step_images, t) for name, t in tabs.items()})
        graphs, (x, rf, out, rec) = _step_graphs(m, S, B, states, step_forms)

        def convert_then_step(cs):      # today's caller: the whole frames shifted down to bytes, then the I420 step on them
            convert()
            m.track_step_images(tabs["i420"], states, 4.0, MEAN, STD, x, rf, out, record=rec, stream=cs)
        graphs["convert_then_step"] = _capture(convert_then_step)
        graphs["convert_alone"] = _capture(lambda cs: convert())
        rounds = _interleaved(graphs, 1, a.rounds, a.replays * 5, all_rounds=True)
        row = {name: _stats(v) for name, v in rounds.items() if not name.startswith("convert")}
        row["ratio_vs_rgb_frames"] = {name: round(min(v) / min(rounds["rgb_frames"]), 3) for name, v in rounds.items() if not name.startswith("convert")}
        row["ratio_vs_i420"] = {name: round(min(v) / min(rounds["i420"]), 3) for name, v in rounds.items() if not name.startswith("convert")}
        res["step_us"][f"G{S}"] = row
        res["convert_step_us"][f"G{S}"] = {"convert_then_step": _stats(rounds["convert_then_step"]), "convert_alone": _stats(rounds["convert_alone"]),
                                           "i010_step": _stats(rounds["i010"]), "i420_step": _stats(rounds["i420"]),
                                           "ratio": round(min(rounds["convert_then_step"]) / min(rounds["i010"]), 2)}
        del m, graphs
    return res


def _nv12_to_rgb(y, uv):
    """The whole frames (n, H, W) / (n, H/2, W/2, 2) -> (n, H, W, 3) uint8 with unfused int32 torch ops: BT.601 limited range,
    OpenCV's fixed point."""
    import torch
    Y = (y.to(torch.int32) - 16).clamp_min_(0) * 1220542
    c = uv.to(torch.int32) - 128
    c = c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    u, v = c[..., 0], c[..., 1]
    r = (Y + 1673527 * v + (1 << 19)) >> 20
    gg = (Y - 852492 * v - 409993 * u + (1 << 19)) >> 20
    b = (Y + 2116026 * u + (1 << 19)) >> 20
    return torch.stack([r, gg, b], dim=-1).clamp_(0, 255).to(torch.uint8)


def _tables(frames, B, n):
    from vittracker_amd.native import FrameTable, Image, ImageTable
    tabs = {}
    for f in FORMATS:
        t = ImageTable(B, "cuda")
        for b in range(B):
            t.set_image(b, getattr(Image, f)(*frames[f][b % n]))
        t.upload()
        tabs[f] = t
    ftab = FrameTable(B, "cuda")
    for b in range(B):
        ftab.set_tensor(b, frames["rgb"][b % n][0])
    ftab.upload()
    return tabs, ftab


def _step_graphs(m, S, B, states, forms):
    """{name: captured open-loop step} for forms {name: (native method, table)}."""
    import torch
    from vittracker_amd.native import Outputs
    m.set_open_loop(True)         # held boxes: every form crops the same windows every step
    m.set_template(torch.zeros(B, 3, S // 2, S // 2, device="cuda"))
    x = torch.empty(B, 3, S, S, device="cuda")
    rf = torch.empty(B, dtype=torch.float64, device="cuda")
    out = Outputs(B, S // 16, "cuda")
    rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
    graphs = {name: _capture(lambda cs, f=f, t=t: f(t, states, 4.0, MEAN, STD, x, rf, out, record=rec, stream=cs))
              for name, (f, t) in forms.items()}
    return graphs, (x, rf, out, rec)


def main():
    import torch
    from vittracker_amd import native
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--sections", default="crop,step,small,convert", help="of crop, step, small, convert, new, parent, planar, wide")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libvittrack_hip.so (section parent)")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    torch.cuda.set_device(0)
    B, n = a.batch, a.distinct
    clock0 = native.probe_clock(20000, 1)[0]
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    rs = np.random.RandomState(0)
    states = torch.tensor([[rs.uniform(120, W - 240), rs.uniform(120, H - 240), rs.uniform(30, 120), rs.uniform(30, 120)] for _ in range(B)],
                          dtype=torch.float64).cuda()
    res = {"B": B, "frame": [H, W], "distinct_frames": n, "rounds": a.rounds, "crop_us": {}, "step_us": {}, "small_batch_us": {},
           "convert_step_us": {}}
    if "parent" in sections:
        if not a.parent_lib:
            raise SystemExit("section parent needs --parent-lib")
        res["parent_ab"] = _parent_ab(a, B, n, g, states)
    if "planar" in sections:
        res["planar"] = _planar(a, B, g, states)
    if "wide" in sections:
        res["wide"] = _wide(a, B, n, g, states)
    frames = {f: _planes(f, n, g) for f in (FORMATS if sections & {"crop", "step", "small", "convert"} else ("rgb", "nv12"))}
    if "new" in sections:
        # (0) the added layouts and colour rows against NV12 BT.601 and the RGB frame route
        from vittracker_amd.native import FrameTable, Image, ImageTable
        ntabs, nkeep = _new_tables(B, n, g)
        nv = ImageTable(B, "cuda")
        ft = FrameTable(B, "cuda")
        for b in range(B):
            nv.set_image(b, Image.nv12(*frames["nv12"][b % n]))
            ft.set_tensor(b, frames["rgb"][b % n][0])
        nv.upload(), ft.upload()
        m = _model(128, B)
        res["new_crop_us"] = {"family": {k: v[3] for k, v in NEW_FORMS.items()}}
        for T in (128, 256):
            outs, graphs = [], {}
            for name, t in [("rgb_frames", ft), ("nv12", nv)] + list(ntabs.items()):
                o = torch.empty(B, T, T, 3, dtype=torch.uint8, device="cuda")
                rf = torch.empty(B, dtype=torch.float64, device="cuda")
                outs.append((o, rf))
                call = m.crop_u8_frames if name == "rgb_frames" else m.crop_u8_images

                def fn(cs, call=call, t=t, o=o, rf=rf):
                    for _ in range(a.reps):
                        call(t, states, 4.0, T, out=o, resize_factor=rf, stream=cs)
                graphs[name] = _capture(fn)
            rounds = _interleaved(graphs, a.reps, a.rounds, a.replays, all_rounds=True)
            row = {k: _stats(v) for k, v in rounds.items()}
            row["ratio_vs_nv12"] = {k: round(min(v) / min(rounds["nv12"]), 3) for k, v in rounds.items()}
            res["new_crop_us"][str(T)] = row
        del m, graphs, ntabs, nkeep
    if not sections & {"crop", "step", "small", "convert"}:
        clock1 = native.probe_clock(20000, 1)[0]
        res["clock_mhz"] = [round(clock0), round(clock1)]
        print(json.dumps(res))
        return
    tabs, ftab = _tables(frames, B, n)
    # (1) crops, B sequences
    m = _model(128, B)
    for T in (128, 256):
        outs = {}

        def crop_form(name, t):
            o = torch.empty(B, T, T, 3, dtype=torch.uint8, device="cuda")
            rf = torch.empty(B, dtype=torch.float64, device="cuda")
            outs[name] = (o, rf)
            call = m.crop_u8_frames if name == "rgb_frames" else m.crop_u8_images

            def fn(cs):
                for _ in range(a.reps):
                    call(t, states, 4.0, T, out=o, resize_factor=rf, stream=cs)
            return _capture(fn)
        graphs = {"rgb_frames": crop_form("rgb_frames", ftab)}
        graphs.update({f: crop_form(f, tabs[f]) for f in FORMATS})
        row = _interleaved(graphs, a.reps, a.rounds, a.replays)
        row["ratio_vs_rgb_frames"] = {f: round(row[f] / row["rgb_frames"], 3) for f in FORMATS}
        res["crop_us"][str(T)] = row
    del m
    # (2) the tracker step, B sequences, NV12 against RGB, in interleaved rounds
    for S in (128, 256):
        m = _model(S, B)
        graphs, keep = _step_graphs(m, S, B, states, {"rgb_frames": (m.track_step_frames, ftab), "nv12": (m.track_step_images, tabs["nv12"])})
        row = _interleaved(graphs, 1, a.rounds, a.replays * 5)
        row["nv12_rate_vs_rgb"] = round(row["rgb_frames"] / row["nv12"], 3)
        res["step_us"][f"G{S}"] = row
        del m, graphs, keep
    # (3) small batches: B = 1, the plugin's form (crop_image_kernel against crop_fast_kernel)
    st1 = states[:1].contiguous()
    t1 = {f: _one_table(frames, f) for f in ("rgb", "bgr", "nv12")}
    f1 = native.FrameTable(1, "cuda")
    f1.set_tensor(0, frames["rgb"][0][0])
    f1.upload()
    m = _model(128, 1)
    o1 = torch.empty(1, 128, 128, 3, dtype=torch.uint8, device="cuda")
    r1 = torch.empty(1, dtype=torch.float64, device="cuda")

    def crop1(call, t):
        def fn(cs):
            for _ in range(a.reps):
                call(t, st1, 4.0, 128, out=o1, resize_factor=r1, stream=cs)
        return _capture(fn)
    graphs = {"crop_rgb_frames": crop1(m.crop_u8_frames, f1)}
    graphs.update({f"crop_{f}": crop1(m.crop_u8_images, t) for f, t in t1.items()})
    row = _interleaved(graphs, a.reps, a.rounds, a.replays)
    graphs, keep = _step_graphs(m, 128, 1, st1, {"step_rgb_frames": (m.track_step_frames, f1), "step_bgr": (m.track_step_images, t1["bgr"]),
                                                   "step_nv12": (m.track_step_images, t1["nv12"])})
    row.update(_interleaved(graphs, 1, a.rounds, a.replays * 5))
    res["small_batch_us"] = {"B": 1, "T": 128, "geom": "G128", **row}
    del m, graphs, keep
    # (4) the alternative: whole frames converted with torch ops, then the frame-table step
    idx = torch.arange(B, device="cuda") % n
    ys = torch.stack([p[0] for p in frames["nv12"]])[idx]
    uvs = torch.stack([p[1] for p in frames["nv12"]])[idx]
    rgb_all = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
    ctab = native.FrameTable(B, "cuda")
    for b in range(B):
        ctab.set_tensor(b, rgb_all[b])
    ctab.upload()
    for S in (128, 256):
        m = _model(S, B)
        graphs, (x, rf, out, rec) = _step_graphs(m, S, B, states, {"nv12": (m.track_step_images, tabs["nv12"])})

        def convert_then_step():
            rgb_all.copy_(_nv12_to_rgb(ys, uvs))
            m.track_step_frames(ctab, states, 4.0, MEAN, STD, x, rf, out, record=rec)
        best = 1e30
        for _ in range(3):
            convert_then_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                convert_then_step()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / 5 * 1e6)
        nv = _interleaved(graphs, 1, a.rounds, a.replays * 5)["nv12"]
        res["convert_step_us"][f"G{S}"] = {"torch_int32_convert_then_step": round(best, 2), "nv12_step": nv, "speedup": round(best / nv, 2)}
        del m, graphs
    clock1 = native.probe_clock(20000, 1)[0]
    res["clock_mhz"] = [round(clock0), round(clock1)]
    print(json.dumps(res))


def _one_table(frames, fmt):
    """A one-entry image table on frame 0 of `fmt`."""
    from vittracker_amd.native import Image, ImageTable
    t = ImageTable(1, "cuda")
    t.set_image(0, getattr(Image, fmt)(*frames[fmt][0]))
    t.upload()
    return t


if __name__ == "__main__":
    main()
