"""The fp32 accuracy budget: a kernel's error against the fp64 truth, held to a multiple of the fp32 oracle's own error.

A plain helper for tests/test_fp32_budget.py (CPU: the budget has teeth) and tests/test_gpu_fp32_budget.py (the HIP kernels).

For one stage the inputs are three arrays computed from the SAME fp32 input: the kernel's output, the fp64 truth (the numpy
oracle at dtype float64) and the fp32 oracle (the reference's arithmetic, oracle/vt_oracle_np.py at float32).  Both the kernel
and the fp32 oracle are measured against the truth, as rel-L2 and as max-abs, and the kernel must satisfy, for both metrics,

    error(kernel) <= FACTORS[stage] * error(fp32 oracle) + floor,

the floor being FLOOR_ULPS fp32 ulps (of 1 for rel-L2, of max |truth| for max-abs): an output rounded to fp32 costs that much.
The fp32 oracle's error on this net is about 2e-6 on the residual stream and 3e-7 to 2e-6 on the maps; a GEMM that keeps only
bf16x2-level products sits 7-40 times above it at some stage (tests/test_fp32_budget.py emulates such defects), while the old
absolute tolerances of 1e-4 let every one of them pass.

Every stage is fed the fp64 truth's upstream activation rounded to fp32 (``stage_inputs``), so an error is charged to the stage
that makes it: stem tokens from the images; the residual after blocks 1, 2, 3 and the final norm from the truth's tokens; the
three maps from the truth's normalised search features.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import vt_oracle_np as onp

STAGES = ("tokens", "resid1", "resid2", "resid3", "norm", "score_map", "size_map", "offset_map")
MAPS = ("score_map", "size_map", "offset_map")

EPS32 = 2.0 ** -23
FLOOR_ULPS = 0.5

# error(kernel) / error(fp32 oracle) allowed per stage, for both metrics.  Set from one MI355X run of tests/test_gpu_fp32_budget.py
# (every form, switch level and regime; the largest ratio in brackets, rel-L2 / max-abs) with headroom, and kept at most a third of
# the smallest ratio an emulated defect reaches at that stage (tests/test_fp32_budget.py, both geometries).  The "fwd" maps of a
# whole forward use the map factors.
FACTORS = {
    # stem: fp32 fma chains / three-piece products with BN folded into the weights in fp64 at load (1.7 / 2.0)
    "tokens": 3.0,
    # blocks (tile form, generic kernels): three-piece products, v_rsq LayerNorm, fitted GELU, exp2 softmax -- about 1.0 / 1.3 on
    # plain weights; with the residual stream on a common-mode offset of 20, 2.1 / 2.6, because the tile form adds bias and
    # product to x one after the other (two roundings at the magnitude of x where the reference rounds once).  The LayerNorm-eps
    # defect reaches only 9.4 / 11.7 at G256, so these cannot go above 3.6
    "resid1": 3.0,
    "resid2": 3.0,
    "resid3": 3.0,
    "norm": 3.0,
    # head: fp32 or three-piece conv towers with BN folded in fp64, sigmoid through exp (2.2 / 3.0, the whole forward's maps of the
    # tile form and the generic kernels 2.1 / 2.5); a BN-eps defect reaches 20 / 6.6
    "score_map": 4.0,
    "size_map": 4.0,
    "offset_map": 4.0,
}

# The frame-form block kernel (blocks_kernel, every batch the tile form does not take: form batch >= 81, the uint8 step, both
# geometries, all three VT_BLOCKS_BF3 levels) has a measured error model of its own.  It accumulates proj and fc2 onto the residual
# stream (the MFMA accumulator starts at x + b), so each of the GEMM's K-steps rounds at the magnitude of x where the reference
# rounds once, after the sum: on plain weights 2.6-3.6x the oracle in rel-L2 and 6-8x in max-abs on the residual (2.6-4.8 fp32 ulps
# rel-L2, ~8 ulps of max |x| in max-abs, at every level VT_BLOCKS_BF3 = 0 / 1 / 2 alike), and 7-10x with the stream riding on a
# common-mode offset of 20, where ulp(x) grows while the oracle's own error does not.  The maps of a whole forward inherit it (up to
# 7.6x).  These factors cover that model (largest ratios seen: 8.7 / 10.5 on the blocks, 7.4 / 7.6 on the whole forward's maps);
# they still fail every emulated GEMM, GELU and BN defect, but not a LayerNorm eps of 1e-6 at G256.
FRAME_FORM = {"resid1": 14.0, "resid2": 14.0, "resid3": 14.0, "norm": 14.0,
              "score_map": 10.0, "size_map": 10.0, "offset_map": 10.0}


# ----------------------------------------------------------------------------- oracle stage runs
def tokens(sd, z, x, dtype):
    """Stem + pos-embed of the oracle at `dtype`: the (B, Lz + Lx, C) token matrix (vit_dist.py:78-84)."""
    sd = onp._cast(sd, dtype)
    zt, _ = onp.stem(z.astype(dtype), sd)
    xt, _ = onp.stem(x.astype(dtype), sd)
    return np.concatenate([zt + sd["pos_embed_z"], xt + sd["pos_embed_x"]], axis=1)


def blocks(sd, T, num_heads, dtype, depth=3):
    """[residual after block 1, .., block depth] and the final norm's search rows, from tokens T, at `dtype`."""
    sd = onp._cast(sd, dtype)
    X = T.astype(dtype)
    res = []
    for i in range(depth):
        X = onp.block(X, sd, i, num_heads)
        res.append(X)
    len_x = sd["pos_embed_x"].shape[1]
    return res, onp.layer_norm(X, sd["norm.weight"], sd["norm.bias"])[:, -len_x:]


def head(sd, feat, dtype):
    """The three maps from normalised search features (B, Lx, C) at `dtype` (vit_dist.py:126-129, head.py:182-201)."""
    sd = onp._cast(sd, dtype)
    B, Lx, C = feat.shape
    F = int(round(math.sqrt(Lx)))
    f = feat.astype(dtype).transpose(0, 2, 1).reshape(B, C, F, F)
    ctr, _ = onp.head_tower(f, sd, "ctr")
    off, _ = onp.head_tower(f, sd, "offset")
    siz, _ = onp.head_tower(f, sd, "size")
    return {"score_map": onp.sigmoid_clamped(ctr), "size_map": onp.sigmoid_clamped(siz), "offset_map": off}


def stage_inputs(sd, z, x, num_heads=1):
    """The fp64 truth's activations rounded to fp32: tokens T (input of the blocks) and search features N (input of the head)."""
    T = tokens(sd, z, x, np.float64).astype(np.float32)
    _, norm = blocks(sd, T, num_heads, np.float64)
    return T, np.ascontiguousarray(norm.astype(np.float32))


def stages(sd, z, x, T, N, num_heads, dtype):
    """Every stage of the oracle at `dtype`, each from its fp32 input: stem from (z, x), blocks from T, head from N."""
    res, norm = blocks(sd, T, num_heads, dtype)
    out = {"tokens": tokens(sd, z, x, dtype), "norm": norm}
    out.update({f"resid{i + 1}": r for i, r in enumerate(res)})
    out.update(head(sd, N, dtype))
    return out


def references(sd, z, x, num_heads=1):
    """What a stage-wise check needs: (T, N, truth stages, fp32-oracle stages, truth forward, fp32-oracle forward)."""
    T, N = stage_inputs(sd, z, x, num_heads)
    truth = stages(sd, z, x, T, N, num_heads, np.float64)
    o32 = stages(sd, z, x, T, N, num_heads, np.float32)
    f64 = onp.forward(sd, z, x, num_heads=num_heads, dtype=np.float64)
    f32 = onp.forward(sd, z, x, num_heads=num_heads, dtype=np.float32)
    return T, N, truth, o32, f64, f32


# ----------------------------------------------------------------------------- the budget
def errors(got, truth):
    """(rel-L2, max-abs) of `got` against `truth`, in fp64."""
    d = np.asarray(got, np.float64) - np.asarray(truth, np.float64)
    t = np.asarray(truth, np.float64)
    return float(np.linalg.norm(d) / max(np.linalg.norm(t), 1e-300)), float(np.abs(d).max())


def judge(stage, kernel, truth, oracle, factor=None):
    """One stage: the kernel's and the fp32 oracle's (rel-L2, max-abs) against the truth, the bounds, and whether both hold."""
    f = FACTORS[stage] if factor is None else factor
    k_rel, k_abs = errors(kernel, truth)
    o_rel, o_abs = errors(oracle, truth)
    b_rel = f * o_rel + FLOOR_ULPS * EPS32
    b_abs = f * o_abs + FLOOR_ULPS * EPS32 * float(np.abs(np.asarray(truth, np.float64)).max())
    return {"stage": stage, "kernel_rel": k_rel, "kernel_abs": k_abs, "oracle_rel": o_rel, "oracle_abs": o_abs,
            "bound_rel": b_rel, "bound_abs": b_abs,
            "ratio_rel": k_rel / max(o_rel, 1e-300), "ratio_abs": k_abs / max(o_abs, 1e-300),
            "ok": k_rel <= b_rel and k_abs <= b_abs}


def fmt(r):
    return (f"{r['stage']:>10}: rel {r['kernel_rel']:.2e} (oracle {r['oracle_rel']:.2e}, x{r['ratio_rel']:.2f}, bound {r['bound_rel']:.2e})"
            f"  abs {r['kernel_abs']:.2e} (oracle {r['oracle_abs']:.2e}, x{r['ratio_abs']:.2f}, bound {r['bound_abs']:.2e})"
            + ("" if r["ok"] else "  OVER"))
