"""The folded odd K chunk of vt_bf3.h (mma_odd), stated on the CPU (numpy; no GPU, no library call).

A lone 16-deep chunk of K used to cost six K = 16 MFMAs, one per kept term of the three-piece product.  The two 16-deep halves of
a K = 32 instruction need not be the same piece pair, so the six terms are three instructions, two terms each, small terms first:

    step 0:  [wh | wl] . [xl | xh] = wh xl + wl xh
    step 1:  [wh | wm] . [xm | xh] = wh xm + wm xh
    step 2:  [wh | wm] . [xh | xm] = wh xh + wm xm

These tests restate that grouping with fp32 accumulation and check, for random operands and for the adversarial exponents and
mantissas of tests/test_bf3_arithmetic.py, that it sums exactly the six kept terms (and no dropped one), and that a K = 48
contraction issued that way (chunk pair 0 as six K = 32 terms, chunk 2 folded, in the kernel's issue order) stays inside the bounds
test_bf3_arithmetic.py states for the six-term product."""
import numpy as np

from test_bf3_arithmetic import _fp32_fma_dot, _operands, split3

H, M, L = 0, 1, 2
# (w piece, x piece) of a step's first and second 16-deep half: vt_bf3.h mma_odd<0..2>
FOLD_STEPS = (((H, L), (L, H)), ((H, M), (M, H)), ((H, H), (M, M)))
KEPT = {(H, H), (H, M), (M, H), (H, L), (L, H), (M, M)}
DROPPED = {(M, L), (L, M), (L, L)}
# chunk pair 0's six K = 32 terms in mma_small / mma_large order (TW / TX of vt_blocks.h)
PAIR_TERMS = ((L, H), (H, L), (M, M), (M, H), (H, M), (H, H))


def _pieces(a):
    h, m, l, _, _ = split3(a)
    return (h, m, l)


def _mfma(acc, wa, xa):
    """One MFMA pass: exact bf16 x bf16 products added into an fp32 accumulator, k by k (a conservative model of the instruction:
    the hardware rounds no more often)."""
    for k in range(wa.shape[-1]):
        acc = (acc.astype(np.float64) + wa[..., k].astype(np.float64) * xa[..., k].astype(np.float64)).astype(np.float32)
    return acc


def _fold_step(acc, w, x, step):
    """Step `step` on one 16-deep chunk: a K = 32 pass whose halves are two different piece pairs of the same 16 k."""
    (w0, x0), (w1, x1) = FOLD_STEPS[step]
    return _mfma(acc, np.concatenate([w[w0], w[w1]], -1), np.concatenate([x[x0], x[x1]], -1))


def _tile48_dot(a, b):
    """sum_k a[k] b[k], K = 48, the way tile48, mlp_first3 and fc1_terms3 issue it: one chain; the pair term, then a folded step
    behind terms 1, 3 and 5.  (With the folded steps IN FRONT of terms 0, 3 and 5 this model misses the 4e-7 bound on the
    adversarial exponents, at 4.7e-7: the kernel uses this one order at every K = 48 site.)"""
    w0, x0 = _pieces(a[..., :32]), _pieces(b[..., :32])
    w2, x2 = _pieces(a[..., 32:]), _pieces(b[..., 32:])
    acc = np.zeros(a.shape[:-1], dtype=np.float32)
    for e, (pw, px) in enumerate(PAIR_TERMS):
        acc = _mfma(acc, w0[pw], x0[px])
        if e in (1, 3, 5):
            acc = _fold_step(acc, w2, x2, (1, 3, 5).index(e))
    return acc


def test_the_grouping_is_the_six_kept_terms_and_no_dropped_one():
    pairs = [p for step in FOLD_STEPS for p in step]
    assert len(pairs) == 6 and set(pairs) == KEPT and not set(pairs) & DROPPED
    # small terms first: the step that holds h h is the last
    assert (H, H) in FOLD_STEPS[2] and all(L in p for p in FOLD_STEPS[0])


def test_the_folded_steps_sum_exactly_the_kept_products():
    """Numerically, element by element: bf16 x bf16 products and their six-term sums are exact in fp64 (at most 46 bits apart),
    so the comparison is for equality -- on the operand mix of test_bf3_arithmetic.py and on its adversarial mantissa."""
    rs = np.random.RandomState(5)
    a, b = _operands(rs, 100_000), _operands(rs, 100_000)
    worst = np.uint32(0x3F80FFFF).view(np.float32)          # leading piece 1.0000000, all ones below it
    a[:64] = worst * np.exp2(np.arange(-32, 32)).astype(np.float32)
    b[:64] = -worst
    w, x = [p.astype(np.float64) for p in _pieces(a)], [p.astype(np.float64) for p in _pieces(b)]
    folded = sum(w[w0] * x[x0] + w[w1] * x[x1] for (w0, x0), (w1, x1) in FOLD_STEPS)
    kept = w[H] * x[H] + w[H] * x[M] + w[M] * x[H] + w[H] * x[L] + w[L] * x[H] + w[M] * x[M]
    assert np.array_equal(folded, kept)
    ab = a.astype(np.float64) * b.astype(np.float64)
    nz = ab != 0
    rel = np.abs(ab - folded)[nz] / np.abs(ab)[nz]
    assert rel.max() < 2.0 ** -21 and rel.mean() < 2.0 ** -24          # test_bf3_arithmetic.py::test_dropped_terms_bound


def _errors(a, b):
    exact = (a.astype(np.float64) * b.astype(np.float64)).sum(-1)
    scale = (np.abs(a.astype(np.float64)) * np.abs(b.astype(np.float64))).sum(-1)
    ok = scale > 0
    e9 = np.abs(_tile48_dot(a, b).astype(np.float64) - exact)[ok] / scale[ok]
    ef = np.abs(_fp32_fma_dot(a, b).astype(np.float64) - exact)[ok] / scale[ok]
    return e9, ef


def _check_against_fp64(a, b, what):
    e9, ef = _errors(a, b)
    # the bounds of test_bf3_arithmetic.py::test_six_term_product_is_as_accurate_as_an_fp32_fma_chain
    assert e9.max() <= 4e-7, (what, float(e9.max()))
    assert e9.max() <= 2.0 * ef.max() + 1e-8, (what, float(e9.max()), float(ef.max()))
    assert e9.mean() <= 1.5 * ef.mean() + 1e-9, (what, float(e9.mean()), float(ef.mean()))


def test_folded_k48_is_as_accurate_as_an_fp32_fma_chain():
    rs = np.random.RandomState(1)
    a = rs.standard_normal((4000, 48)).astype(np.float32)
    b = (rs.standard_normal((4000, 48)) * 0.2).astype(np.float32)
    _check_against_fp64(a, b, "normal")


def test_folded_k48_on_adversarial_exponents():
    """Magnitudes over twenty octaves, exact zeros and powers of two (test_bf3_arithmetic.py::_operands): the same bounds.
    Rows of that file's adversarial mantissa (every product's dropped part at its maximum, signs alternating): there the six-term
    product itself is off by up to 2^-21 of |a b| per product (test_dropped_terms_bound: any operands), which no grouping changes;
    the folded sum is held to that plus the accumulation bound above."""
    rs = np.random.RandomState(6)
    a, b = _operands(rs, 4000 * 48).reshape(4000, 48), _operands(rs, 4000 * 48).reshape(4000, 48)
    _check_against_fp64(a, b, "octaves")
    worst = np.uint32(0x3F80FFFF).view(np.float32)
    a2 = np.full((64, 48), worst, dtype=np.float32) * np.exp2(rs.randint(-10, 10, (64, 48))).astype(np.float32)
    b2 = np.full((64, 48), worst, dtype=np.float32) * np.where(np.arange(48) % 2, -1.0, 1.0).astype(np.float32)
    e9, ef = _errors(a2, b2)
    assert e9.max() <= 2.0 ** -21 + 2.0 * ef.max() + 1e-8, (float(e9.max()), float(ef.max()))
