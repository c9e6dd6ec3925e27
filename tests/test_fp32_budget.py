"""The fp32 budget of tests/fp32_budget.py has teeth (CPU only).

The numpy oracle is monkeypatched to make, at fp32, the mistakes an fp32 kernel of this net could make without the old 1e-4
tolerances noticing: GEMMs with bf16x2-level products (three-piece operands with the small terms dropped, the split rule of
tests/test_bf3_arithmetic.py), the m*m term dropped, a LayerNorm or BatchNorm eps that is not the reference's, the tanh GELU in
place of the erf one.  Each is run stage-wise exactly as tests/test_gpu_fp32_budget.py runs the kernels.  The budget must pass the
plain fp32 oracle and the exact six-term products the kernels issue, fail every defect at some stage, and at every stage keep
its bound at most a third of the smallest error a defect acting there reaches.
"""
import numpy as np
import pytest

import fp32_budget as fb
from oracle import vt_oracle_np as onp
from test_bf3_arithmetic import split3
from vittracker_amd import synth

SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))    # pieces h = 0, m = 1, l = 2 of (activation, weight)
THREE = SIX[:3]                                           # vt3::mma_small dropped: h h + h m + m h
FIVE = SIX[:5]                                            # the m m term dropped
BLOCK_STAGES = ("resid1", "resid2", "resid3", "norm")
BN_STAGES = ("tokens",) + fb.MAPS


def _which(w):
    """Name of a block linear from its weight's shape (out, in) at width C."""
    o, i = w.shape
    return {3 * i: "qkv", i: "proj", 4 * i: "fc1"}.get(o, "fc2" if i == 4 * o else None)


def _split_linear(terms, names):
    orig = onp.linear

    def linear(x, w, b):
        if x.dtype != np.float32 or _which(w) not in names:
            return orig(x, w, b)
        xs, ws = split3(x)[:3], split3(w)[:3]
        acc = sum(xs[i].astype(np.float64) @ ws[j].astype(np.float64).T for i, j in terms)   # exact piece products, one rounding
        return acc.astype(np.float32) + b
    return linear


def _eps(fn, eps):
    return lambda *a, **k: fn(*a, **dict(k, eps=eps))


def _gelu_tanh(x):
    t = x.dtype.type
    return (t(0.5) * x * (1 + np.tanh(t(np.sqrt(2 / np.pi)) * (x + t(0.044715) * x ** 3)))).astype(x.dtype)


LINEARS = ("qkv", "proj", "fc1", "fc2")
# name -> (oracle attribute, replacement, stages whose code the defect changes)
DEFECTS = {
    **{f"{n}_three_term": ("linear", _split_linear(THREE, (n,)), BLOCK_STAGES) for n in LINEARS},
    "every_linear_without_mm": ("linear", _split_linear(FIVE, LINEARS), BLOCK_STAGES),
    "layer_norm_eps_1e-6": ("layer_norm", _eps(onp.layer_norm, 1e-6), BLOCK_STAGES),
    "batch_norm_eps_1e-6": ("batchnorm_eval", _eps(onp.batchnorm_eval, 1e-6), BN_STAGES),
    "gelu_tanh": ("gelu_erf", _gelu_tanh, BLOCK_STAGES),
}
GOOD = {
    "fp32_oracle": None,
    "six_term_products_everywhere": ("linear", _split_linear(SIX, LINEARS), ()),
}

CASES = {"G128": (64, 128, 8), "G256": (128, 256, 2)}
FRAME_FORM_MISSES = {("G256", "layer_norm_eps_1e-6")}      # 9.4 / 11.7 x the oracle: inside FRAME_FORM's 14


def _run(sd, z, x, T, N, patch, monkeypatch):
    with monkeypatch.context() as mp:
        if patch is not None:
            mp.setattr(onp, patch[0], patch[1])
        return fb.stages(sd, z, x, T, N, 1, np.float32)


@pytest.mark.parametrize("geom", sorted(CASES))
def test_budget_passes_fp32_and_fails_every_defect(geom, monkeypatch):
    tz, tx, B = CASES[geom]
    sd = synth.synth_state_dict(0, len_z=(tz // 16) ** 2, len_x=(tx // 16) ** 2)
    z, x = synth.synth_inputs(0, B, tz, tx)
    T, N = fb.stage_inputs(sd, z, x)
    truth = fb.stages(sd, z, x, T, N, 1, np.float64)
    o32 = fb.stages(sd, z, x, T, N, 1, np.float32)
    report = []
    for name, patch in GOOD.items():
        got = _run(sd, z, x, T, N, patch, monkeypatch)
        res = [fb.judge(s, got[s], truth[s], o32[s]) for s in fb.STAGES]
        report += [f"{name}:"] + [fb.fmt(r) for r in res]
        assert all(r["ok"] for r in res), "\n".join(report)
    worst = {s: [] for s in fb.STAGES}     # per stage: the errors of the defects acting there
    for name, (attr, fn, acts) in DEFECTS.items():
        got = _run(sd, z, x, T, N, (attr, fn), monkeypatch)
        res = {s: fb.judge(s, got[s], truth[s], o32[s]) for s in fb.STAGES}
        report += [f"{name}:"] + [fb.fmt(r) for r in res.values()]
        assert not all(r["ok"] for r in res.values()), f"{geom}: {name} passes every stage\n" + "\n".join(report)
        # the frame-form block kernel's looser model (fp32_budget.FRAME_FORM) still fails it, except where that comment says not
        frame = [fb.judge(s, got[s], truth[s], o32[s], fb.FRAME_FORM.get(s) if s not in fb.MAPS else None) for s in fb.STAGES]
        if (geom, name) not in FRAME_FORM_MISSES:
            assert not all(r["ok"] for r in frame), f"{geom}: {name} passes the frame-form budget\n" + "\n".join(map(fb.fmt, frame))
        for s in acts:
            worst[s].append((res[s]["kernel_rel"], res[s]["kernel_abs"], name))
    print("\n".join(report))
    for s, errs in worst.items():
        r = fb.judge(s, o32[s], truth[s], o32[s])
        for rel, ab, name in errs:
            assert r["bound_rel"] <= rel / 3 or r["bound_abs"] <= ab / 3, (geom, s, name, r, rel, ab)
