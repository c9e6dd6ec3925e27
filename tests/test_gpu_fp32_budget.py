"""Every fp32 kernel form held to the fp32 accuracy budget of tests/fp32_budget.py: error against the fp64 truth at most a stated
multiple of the fp32 oracle's own error, stage by stage.

Each stage is fed the fp64 truth's upstream activation rounded to fp32 -- vt_stem from the crops, vt_blocks(nblocks = 1, 2, 3) and
the final norm from the truth's tokens, vt_head from the truth's normalised search features -- then one whole vt_forward is
judged on its maps.  The truth is the numpy oracle at float64 on the same fp32 inputs, so the bounds scale with the oracle's own
error and need no per-regime tolerance.

Forms: G128 at form batch 0 / 128 / 256 (tile blocks, stem_a / stem_b, per-tower head + decode ... stem_fused, the frame-form block
kernel, head_fused3), G256 at form batch 0 / 160 / 256 (split head ... stem_stream, the frame-form block kernel, head_seq3), the
generic kernels (112 / 224 px and the 64 / 2 / 64 width), the uint8 entry, and the switch levels VT_BLOCKS_BF3 / VT_HEAD_BF3 /
VT_STEM_BF3 in child processes.  Regimes: plain synth weights, peaked attention (q and k rows x 3), a residual stream on a
common-mode offset (+20 on both pos-embeds) and a hot head (the centre tower's bias shifted until >= 10 % of the score pixels sit
on the 1 - 1e-4 clamp).

Boxes: pred_boxes / hann_boxes / conf equal, bit for bit, the first-index decode of the kernel's own maps (the window is the
reference's torch window, host_ops.hann2d); they pick the truth's cell wherever the truth's top-2 margin exceeds 10 x the score
map's budget.  In the hot-head regime, where ties on the clamp decide, only the first check applies.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fp32_budget as fb
from oracle import vt_oracle_np as onp
from vittracker_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GEOM = {"G128": (64, 128, 3), "G256": (128, 256, 2)}
FORMS = {"G128": (0, 128, 256), "G256": (0, 160, 256)}
REGIMES = ("plain", "peaked", "common_mode", "hot_head")
HOT_SHIFT = 9.0           # measured on the CPU: 69 % (G128) / 15 % (G256) of the truth's score pixels clamped; +6 clamps none
KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")


def _weights(tz, tx, regime="plain", C=48, W=32, seed=0):
    sd = synth.synth_state_dict(seed, C=C, head_ch=W, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
    if regime == "peaked":
        for blk in range(3):
            sd[f"blocks.{blk}.attn.qkv.weight"][:2 * C] *= 3.0
            sd[f"blocks.{blk}.attn.qkv.bias"][:2 * C] *= 3.0
    elif regime == "common_mode":
        sd["pos_embed_z"] += 20.0
        sd["pos_embed_x"] += 20.0
    elif regime == "hot_head":
        sd["box_head.conv5_ctr.bias"] += HOT_SHIFT
    else:
        assert regime == "plain", regime
    return sd


_REFS = {}


def _refs(key, sd, z, x, heads=1):
    if key not in _REFS:
        _REFS[key] = fb.references(sd, z, x, heads)
    return _REFS[key]


def kernel_stages(m, z, x, T, N, patches=None):
    """The kernels' outputs of every stage (numpy): vt_stem / vt_stem_u8, vt_blocks from T, vt_head from N, vt_forward(_u8)."""
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    zd = dev(z)
    if patches is None:
        xd = dev(x)
        out = {"tokens": m.stem(zd, xd)}
        fwd = m.forward(zd, xd)
    else:
        pd = dev(patches)
        out = {"tokens": m.stem_u8(pd, torch.zeros(z.shape[0], m.L, m.channels, device="cuda"))}
        fwd = m.forward_u8(zd, pd)
    Td = dev(T)
    for k in (1, 2, 3):
        feat, out[f"resid{k}"] = m.blocks(Td, nblocks=k, want_resid=True)
    out["norm"] = feat
    h = m.head(dev(N))
    out.update({k: getattr(h, k) for k in fb.MAPS})
    out.update({"fwd_" + k: getattr(fwd, k) for k in KEYS})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _judge(label, kern, refs, F, frame, clamp=False, len_z=None):
    """Records of every stage plus the box checks; returns (records, failures).  frame: the frame-form block kernel ran, whose
    block stages and whole-forward maps are held to fp32_budget.FRAME_FORM (its measured error model)."""
    T, N, truth, o32, f64, f32 = refs
    recs = []
    for s in fb.STAGES:
        k, t, o = kern[s], truth[s], o32[s]
        if s == "tokens" and len_z is not None:          # vt_stem_u8 writes the search rows only
            k, t, o = k[:, len_z:], t[:, len_z:], o[:, len_z:]
        recs.append(fb.judge(s, k, t, o, fb.FRAME_FORM.get(s) if frame and s not in fb.MAPS else None))
    for s in fb.MAPS:
        r = fb.judge(s, kern["fwd_" + s], f64[s], f32[s], fb.FRAME_FORM[s] if frame else None)
        r["stage"] = "fwd " + s
        recs.append(r)
    fails = [f"{label} {r['stage']}" for r in recs if not r["ok"]]
    # boxes: the first-index decode of the kernel's own maps, bit for bit
    from vittracker_amd.host_ops import hann2d
    win = hann2d((F, F)).numpy()
    score, size, off = kern["fwd_score_map"], kern["fwd_size_map"], kern["fwd_offset_map"]
    bbox, mx, idx = onp.cal_bbox(score, size, off, F)
    hbox, _, hidx = onp.cal_bbox(win * score, size, off, F)
    for name, got, want in (("pred_boxes", kern["fwd_pred_boxes"], bbox), ("hann_boxes", kern["fwd_hann_boxes"], hbox),
                            ("conf", kern["fwd_conf"], mx)):
        if not np.array_equal(got, want):
            fails.append(f"{label} {name} != decode of its own maps")
    if not clamp:
        # the truth's cell wherever its top-2 margin is 10 x the score map's budget
        margin = 10 * recs[-3]["bound_abs"]
        w64 = win.astype(np.float64)
        _, _, tidx = onp.cal_bbox(f64["score_map"], f64["size_map"], f64["offset_map"], F)
        _, _, thidx = onp.cal_bbox(w64 * f64["score_map"], f64["size_map"], f64["offset_map"], F)
        ok = onp.top2_margin(f64["score_map"]) > margin
        okh = onp.top2_margin(w64 * f64["score_map"]) > margin
        if not (np.array_equal(idx[ok], tidx[ok]) and np.array_equal(hidx[okh], thidx[okh])):
            fails.append(f"{label} boxes pick another cell than the truth's")
        if not ok.any():
            fails.append(f"{label}: no frame with a clear argmax (margin {margin:.1e})")
    print(f"--- {label}")
    for r in recs:
        print(fb.fmt(r))
    return recs, fails


def _model(tz, tx, B, sd, form_batch=0, **kw):
    from vittracker_amd import native
    m = native.Model(tz, tx, max_batch=B, **kw)
    m.load_state_dict(sd)
    if form_batch:
        m.set_form_batch(form_batch)
    return m


def _case(geom, regime, seed=0):
    tz, tx, B = GEOM[geom]
    sd = _weights(tz, tx, regime)
    z, x = synth.synth_inputs(seed, B, tz, tx)
    refs = _refs((geom, regime), sd, z, x)
    if regime == "hot_head":
        frac = float((refs[4]["score_map"] >= np.float32(1 - 1e-4)).mean())
        assert frac >= 0.1, frac
    return tz, tx, B, sd, z, x, refs


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("geom", sorted(GEOM))
def test_every_form_within_the_fp32_budget(geom, regime):
    tz, tx, B, sd, z, x, refs = _case(geom, regime)
    fails = []
    for form in FORMS[geom]:
        m = _model(tz, tx, B, sd, form)
        kern = kernel_stages(m, z, x, refs[0], refs[1])
        fails += _judge(f"{geom} {regime} form {form}", kern, refs, tx // 16, form > 0, clamp=regime == "hot_head")[1]
        m.close()
    assert not fails, fails


@pytest.mark.parametrize("tz,tx,C,heads,W", [(112, 224, 48, 1, 32), (128, 256, 64, 2, 64)])
def test_generic_kernels_within_the_fp32_budget(tz, tx, C, heads, W):
    B = 3
    sd = _weights(tz, tx, C=C, W=W, seed=4)
    z, x = synth.synth_inputs(4, B, tz, tx)
    refs = _refs(("generic", tz, tx, C), sd, z, x, heads)
    m = _model(tz, tx, B, sd, channels=C, heads=heads, head_channels=W)
    kern = kernel_stages(m, z, x, refs[0], refs[1])
    m.close()
    fails = _judge(f"generic {tz}/{tx} {C}/{heads}/{W}", kern, refs, tx // 16, False)[1]
    assert not fails, fails


@pytest.mark.parametrize("geom", sorted(GEOM))
def test_uint8_entry_within_the_fp32_budget(geom):
    """vt_stem_u8 / vt_forward_u8 on uint8 patches, form batch 256; the truth is the fp64 net on synth.normalise_patches."""
    tz, tx, B = GEOM[geom]
    sd = _weights(tz, tx)
    z, _ = synth.synth_inputs(5, B, tz, tx)
    patches = synth.synth_patches(5, B, tx)
    x = synth.normalise_patches(patches)
    refs = _refs(("u8", geom), sd, z, x)
    m = _model(tz, tx, B, sd, 256)
    assert m.patch_u8_supported(B)
    kern = kernel_stages(m, z, x, refs[0], refs[1], patches=patches)
    fails = _judge(f"{geom} uint8", kern, refs, tx // 16, True, len_z=m.len_z)[1]
    m.close()
    assert not fails, fails


CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_fp32_budget as t
for path in sys.argv[1:]:
    a = dict(np.load(path))
    sd = {k[3:]: v for k, v in a.items() if k.startswith("sd.")}
    tz, tx, B = (int(v) for v in a["geom"])
    m = t._model(tz, tx, B, sd, 256)
    np.savez(path[:-4] + ".out.npz", **t.kernel_stages(m, a["z"], a["x"], a["T"], a["N"]))
    m.close()
print("OK")
"""

SWITCHES = {"VT_BLOCKS_BF3=1": {"VT_BLOCKS_BF3": "1"}, "VT_BLOCKS_BF3=0": {"VT_BLOCKS_BF3": "0"},
            "VT_HEAD_BF3=0": {"VT_HEAD_BF3": "0"}, "VT_STEM_BF3=0": {"VT_STEM_BF3": "0"}}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_switch_levels_within_the_fp32_budget(switch, tmp_path):
    """The kernels' precision levels, read at vt_create: one child process per level, both geometries at form batch 256."""
    paths, cases = [], {}
    for geom in sorted(GEOM):
        tz, tx, B, sd, z, x, refs = _case(geom, "plain")
        p = str(tmp_path / f"{geom}.npz")
        np.savez(p, geom=np.array([tz, tx, B]), z=z, x=x, T=refs[0], N=refs[1], **{"sd." + k: v for k, v in sd.items()})
        paths.append(p)
        cases[p] = (geom, tx, refs)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VT_")}
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}] + paths,
                       env=dict(env, **SWITCHES[switch]), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])
    fails = []
    for p, (geom, tx, refs) in cases.items():
        kern = dict(np.load(p[:-4] + ".out.npz"))
        fails += _judge(f"{geom} {switch} form 256", kern, refs, tx // 16, True)[1]
    assert not fails, fails
