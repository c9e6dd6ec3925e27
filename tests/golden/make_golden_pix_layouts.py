#!/usr/bin/env python3
"""Records what the host side of the image route does, layout by layout, into tests/golden/ref_pix_layouts.json.

    python tests/golden/make_golden_pix_layouts.py          # numpy only, no GPU, no library

It goes through the public names of vittracker_amd.native alone (ImageTable.check, the Image constructors, pack_image_offsets), so the
file recorded at one commit can be replayed against a later one: tests/test_pix_layout_table.py calls record() and compares entry by
entry.  The committed file was recorded before the layout table existed (the commit message names that commit and the file's sha256).

Outcomes are short strings.  ImageTable.check: "p0,p1" (the two pitches it returns) or "!F" / "!F@K" -- F the index in FRAGMENTS of the
first fragment found in the message, K the plane the message names; the out-of-buffer message is kept whole ("!plane 1: needs 64 bytes").
Per layout code the outcomes of all cases are joined with ";", and codes with the same string share one entry."""
from __future__ import annotations

import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_pix_layouts.json")

#: what the tests match in the messages, in the order they are looked for
FRAGMENTS = ("unknown pixel format", "null", "shorter than a row", "reserved", "no matrix or range", "even H and W", "even W", "W even", "odd",
             "plane K: needs N bytes", "beyond the 32-bit offsets", "not back to back", "back to back", "one row pitch", "must be",
             "chroma plane must be", "not contiguous", "dense", "(3, H, W)", "(B, 3, H, W)", "order", "uint8", "depth", "sub")
_NEEDS = re.compile(r"plane \d+: needs \d+ bytes")
_PLANE = re.compile(r"plane (\d+):")

SIZES = ((1, 1), (2, 2), (3, 4), (4, 3), (6, 10))
ONE = (4, 8)                    # the size of the colour, address and buffer sweeps
BASE = 0x10000                  # plane 0; plane 1 lies 0x8000 behind it
#: (matrix bits, range bits, bits 16-31): the four legal tags, an illegal matrix, an illegal range, a high bit
COLOURS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 0, 0), (0, 2, 0), (0, 0, 1))


def rejected(msg: str) -> str:
    m = _NEEDS.search(msg)
    for i, f in enumerate(FRAGMENTS):
        if f == "plane K: needs N bytes":
            if m:
                return "!" + m.group(0)
        elif f in msg:
            k = _PLANE.search(msg)
            return f"!{i}" + (f"@{k.group(1)}" if k else "")
    return "!?" + msg


def sweep_check(native):
    """{joined outcomes: [codes]} and the labels of the cases, in order."""
    check, VtError = native.ImageTable.check, native.VtError
    labels, per_code = [], {}

    def run(out, label, *a, **kw):
        if out is per_code[0]:
            labels.append(label)
        try:
            r = check(*a, **kw)
            out.append(f"{r[0]},{r[1]}")
            return r
        except VtError as e:
            out.append(rejected(str(e)))
            return None

    def quiet(*a, **kw):
        try:
            return check(*a, **kw)
        except VtError:
            return None

    for code in range(256):
        out = per_code.setdefault(code, [])
        p0, p1 = BASE, BASE + 0x8000
        H, W = ONE
        for m, r, hi in COLOURS:
            run(out, f"colour {m}/{r}/{hi}", code | m << 8 | r << 12 | hi << 16, p0, p1, H, W)
        run(out, "reserved", code, p0, p1, H, W, 0, 0, 1)
        run(out, "reserved, colour", code | 1 << 8, p0, p1, H, W, 0, 0, 1)
        run(out, "H 0", code, p0, p1, 0, W)
        run(out, "colour, odd size, null", code | 1 << 8, 0, p1, 3, 3)
        run(out, "odd size, short pitch, null", code, 0, 0, 3, 3, 1, 1)
        for h, w in SIZES:
            rb = quiet(code, p0, p1, h, w) or quiet(code, p0, p1, h, w + 1) or (w + 1, w + 1)      # the default pitches: the rows' bytes
            run(out, f"{h}x{w}", code, p0, p1, h, w)
            for d in (1, 2):
                run(out, f"{h}x{w} pitch0 +{d}", code, p0, p1, h, w, rb[0] + d, 0)
                run(out, f"{h}x{w} pitch1 +{d}", code, p0, p1, h, w, 0, rb[1] + d)
            run(out, f"{h}x{w} pitch0 -1", code, p0, p1, h, w, rb[0] - 1, 0)
            run(out, f"{h}x{w} pitch1 -1", code, p0, p1, h, w, 0, max(rb[1] - 1, 1))
        for a in range(4):
            for b in range(4):
                run(out, f"address +{a} +{b}", code, p0 + a, p1 + b, H, W)
        run(out, "address +1 +0 pitch +1", code, p0 + 1, p1, H, W, 2 * W + 1, 2 * W + 1)
        run(out, "null 0", code, 0, p1, H, W)
        run(out, "null 1", code, p0, 0, H, W)
        # bytes needed per plane: the smallest buffer check() takes (0 where it does not look at the plane)
        need = []
        for k in (0, 1):
            lo, hi = 0, 1 << 16
            kw = lambda n: {"nbytes0": n} if k == 0 else {"nbytes1": n}      # noqa: E731
            if quiet(code, p0, p1, H, W) is None:
                need.append(0)
                continue
            while lo < hi:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if quiet(code, p0, p1, H, W, **kw(mid)) else (mid + 1, hi)
            need.append(lo)
        run(out, "buffers exact", code, p0, p1, H, W, nbytes0=need[0], nbytes1=need[1])
        run(out, "buffer 0 short", code, p0, p1, H, W, nbytes0=need[0] - 1, nbytes1=need[1])
        run(out, "buffer 1 short", code, p0, p1, H, W, nbytes0=need[0], nbytes1=need[1] - 1)
        run(out, "buffers short, pitch +2", code, p0, p1, H, W, 4 * W + 2, 4 * W + 2, nbytes0=need[0], nbytes1=need[1])
        out.append(f"need {need[0]},{need[1]}")
        if code == 0:
            labels.append("bytes needed")
    groups = {}
    for code, out in per_code.items():
        groups.setdefault(";".join(out), []).append(code)
    return labels, groups


# ---- the constructors -------------------------------------------------------------------------------------------------------------
#: name -> (kind, arguments of the kind).  kinds: "packed" (bytes a pixel), "gray" (bytes a sample), "pairs" / "three" (chroma column
#: shift, chroma row shift, bytes a sample), "chw" (order), "buffer"
CONSTRUCTORS = {
    "rgb": ("packed", 3), "bgr": ("packed", 3), "rgba": ("packed", 4), "bgra": ("packed", 4), "yuyv": ("packed", 2), "uyvy": ("packed", 2),
    "gray": ("gray", 1), "gray16": ("gray", 2),
    "nv12": ("pairs", 1, 1, 1), "nv21": ("pairs", 1, 1, 1), "p010": ("pairs", 1, 1, 2),
    "nv16": ("pairs", 1, 0, 1), "nv24": ("pairs", 0, 0, 1), "p210": ("pairs", 1, 0, 2), "p410": ("pairs", 0, 0, 2),
    "i420": ("three", 1, 1, 1), "yv12": ("three", 1, 1, 1), "i422": ("three", 1, 0, 1), "i444": ("three", 0, 0, 1),
    "yv16": ("three", 1, 0, 1), "yv24": ("three", 0, 0, 1), "rgb_planar": ("three", 0, 0, 1), "bgr_planar": ("three", 0, 0, 1),
    "i010": ("three", 1, 1, 2), "i420_buffer": ("buffer",), "chw": ("chw",),
}
for _s, (_cs, _rs) in {"420": (1, 1), "422": (1, 0), "444": (0, 0)}.items():
    for _d in (10, 12, 16):
        CONSTRUCTORS[f"yuv16:{_s}:{_d}"] = ("three", _cs, _rs, 2)
for _d in (10, 12):
    CONSTRUCTORS[f"gray16:{_d}"] = ("gray", 2)
CON_SIZES = ((6, 10), (2, 4), (1, 2))          # (2, 4): a single row of 4:2:0 chroma; (1, 2): a single row of everything
#: how the planes are cut from the buffer: tight rows; rows padded by 4 bytes; (three planes) tight with the last plane 16 bytes late
VARIANTS = ("tight", "padded", "apart")


def _cut(buf, off, rows, rb, pad, item=1, wide=False):
    """A (rows, rb) plane of bytes at buf[off], rows rb + pad apart, as (rows, rb // item, item) where item > 1 and as uint16 where
    `wide`.  Returns (plane, bytes it spans rounded up to whole pitches)."""
    pitch = rb + pad
    a = buf[off:off + rows * pitch].reshape(rows, pitch)[:, :rb]
    if wide:
        a = a.view(np.uint16)
    if item > 1:
        a = a.reshape(rows, a.shape[1] // item, item)
    return a, rows * pitch


def _planes(kind, H, W, variant, buf):
    """The arguments of a constructor of this kind, cut from buf (None: the variant does not apply)."""
    pad = 4 if variant == "padded" else 0
    k = kind[0]
    if k == "packed":
        return None if variant == "apart" else [_cut(buf, 64, H, W * kind[1], pad, kind[1])[0]]
    if k == "gray":
        return None if variant == "apart" else [_cut(buf, 64, H, W * kind[1], pad, 1, wide=kind[1] == 2 and not pad)[0]]
    if k == "buffer":
        return None if variant != "tight" else [_cut(buf, 64, 3 * H // 2, W, 0)[0]]
    if k == "chw":
        if variant == "apart":
            return None
        pitch = W + pad
        return [np.lib.stride_tricks.as_strided(buf[64:], (3, H, W), (H * pitch, pitch, 1))]
    cs, rs, spp = kind[1:]
    wide = spp == 2 and not pad                  # 16-bit planes: uint16 arrays when tight, their byte views when padded
    y, n = _cut(buf, 64, H, W * spp, pad, wide=wide)
    off = 64 + n + 64
    cw, ch = W >> cs, H >> rs
    if k == "pairs":
        return None if variant == "apart" else [y, _cut(buf, off, ch, 2 * cw * spp, pad, 2 * spp if not wide else 2, wide=wide)[0]]
    c1, n = _cut(buf, off, ch, cw * spp, pad, wide=wide)
    c2, _ = _cut(buf, off + n + (16 if variant == "apart" else 0), ch, cw * spp, pad, wide=wide)
    return [y, c1, c2]


def sweep_constructors(native):
    Image, VtError = native.Image, native.VtError
    out = {}
    for name, kind in CONSTRUCTORS.items():
        fn, _, rest = name.partition(":")
        kw = {}
        if fn == "yuv16":
            kw = {"sub": rest.split(":")[0], "depth": int(rest.split(":")[1])}
        elif fn == "gray16" and rest:
            kw = {"depth": int(rest)}
        for H, W in CON_SIZES:
            for variant in VARIANTS:
                buf = np.zeros(4096, np.uint8)
                base = Image._address(buf)
                try:
                    args = _planes(kind, H, W, variant, buf)
                except ValueError:               # the size does not cut into these planes
                    args = None
                if args is None:
                    continue
                for tag in (("", {}), ("bt709 full", {"matrix": "bt709", "range": "full"})) if variant == "tight" and (H, W) == CON_SIZES[0] else (("", {}),):
                    if tag[1] and fn in ("rgb", "bgr", "rgba", "bgra", "gray", "gray16", "rgb_planar", "bgr_planar", "chw"):
                        continue
                    key = f"{name} {H}x{W} {variant}" + (" " + tag[0] if tag[0] else "")
                    try:
                        im = getattr(Image, fn)(*args, **kw, **tag[1])
                    except VtError as e:
                        out[key] = rejected(str(e))
                        continue
                    out[key] = {"image": [im.format, im.H, im.W, list(im.pitches)], "plane_rows": [list(r) for r in im.plane_rows()],
                                "offsets": [Image._address(p) - base for p in im.planes],
                                "host_planes": [list(p.shape) for p in im.host_planes()],
                                "descriptor": list(im.descriptor([1 << 20, 1 << 21][:len(im.plane_rows())], [r[1] for r in im.plane_rows()])),
                                "pack": [list(map(list, (o := native.pack_image_offsets([im, im], start=96))[0])), o[1]]}
    # the odd ones: a permuted HWC view through chw, the BGR order, a batch, what the constructors refuse
    buf = np.zeros(4096, np.uint8)
    hwc = buf[:6 * 10 * 3].reshape(6, 10, 3)
    extra = {"chw permuted": lambda: Image.chw(hwc.transpose(2, 0, 1)), "chw bgr": lambda: Image.chw(buf[:180].reshape(3, 6, 10), "bgr"),
             "chw permuted bgr": lambda: Image.chw(hwc.transpose(2, 0, 1), order="bgr"),
             "chw order": lambda: Image.chw(buf[:180].reshape(3, 6, 10), "gbr"), "chw shape": lambda: Image.chw(buf[:240].reshape(4, 6, 10)),
             "chw sparse": lambda: Image.chw(buf[:360].reshape(3, 6, 20)[:, :, ::2]),
             "batch": lambda: native.images_from_chw(buf[:360].reshape(2, 3, 6, 10))[1], "batch shape": lambda: native.images_from_chw(buf[:180].reshape(3, 6, 10)),
             "rgb float": lambda: Image.rgb(np.zeros((6, 10, 3), np.float32)), "rgb shape": lambda: Image.rgb(buf[:240].reshape(6, 10, 4)),
             "nv12 odd": lambda: Image.nv12(buf[:15].reshape(3, 5), buf[64:68].reshape(1, 2, 2)),
             "nv12 chroma": lambda: Image.nv12(buf[:60].reshape(6, 10), buf[64:94].reshape(3, 10)),
             "nv16 odd": lambda: Image.nv16(buf[:15].reshape(3, 5), buf[64:76].reshape(3, 2, 2)),
             "yuyv odd": lambda: Image.yuyv(buf[:30].reshape(3, 5, 2)), "i422 odd": lambda: Image.i422(buf[:15].reshape(3, 5), buf[64:70].reshape(3, 2), buf[70:76].reshape(3, 2)),
             "i420 pitches": lambda: Image.i420(buf[:60].reshape(6, 10), buf[64:79].reshape(3, 5), buf[128:152].reshape(3, 8)[:, :5]),
             "i444 pitches": lambda: Image.i444(buf[:60].reshape(6, 10), buf[64:124].reshape(6, 10), buf[128:200].reshape(6, 12)[:, :10]),
             "yuv16 sub": lambda: Image.yuv16(hwc, hwc, hwc, 10, "gray"), "yuv16 depth": lambda: Image.yuv16(hwc, hwc, hwc, 14, "420"),
             "gray16 depth": lambda: Image.gray16(buf[:120].reshape(6, 20), depth=8),
             "p010 big endian": lambda: Image.p010(np.zeros((6, 10), ">u2"), np.zeros((3, 5, 2), ">u2")),
             "i420 buffer shape": lambda: Image.i420_buffer(buf[:50].reshape(5, 10))}
    for key, f in extra.items():
        try:
            im = f()
            out[key] = {"image": [im.format, im.H, im.W, list(im.pitches)], "plane_rows": [list(r) for r in im.plane_rows()],
                        "offsets": [Image._address(p) - Image._address(buf) for p in im.planes]}
        except VtError as e:
            out[key] = rejected(str(e))
    return out


def record(native):
    labels, groups = sweep_check(native)
    return {"fragments": list(FRAGMENTS), "check_cases": labels, "check": {k: v for k, v in sorted(groups.items(), key=lambda kv: kv[1])},
            "constructors": sweep_constructors(native), "names": {str(k): v for k, v in sorted(native.PIX_LAYOUT_NAMES.items())}}


def main():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from vittracker_amd import native
    with open(OUT, "w") as f:
        json.dump(record(native), f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
