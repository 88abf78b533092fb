"""CPU: the numpy model of the split-operand arithmetic (tests/split_model.py) against float64 on the stress operands of the
GPU tests -- the correct model stays under its per-output bound T, and every single defect a kernel could have (a lost l half of
one tap or one 16-channel chunk, 2^-10 for 2^-11, flushed subnormal halves) exceeds the 4 T the GPU tests allow.  This is what
shows that tests/test_hip_split_stress.py can fail."""
import numpy as np
import pytest

import split_model as M

KINDS = ('tame', 'pos', 'signed', 'big')
CHANNELS = (32, 128, 512)              # K = 288, 1152, 4608


def operands(kind, C, seed=0):
    rng = np.random.default_rng([seed, C, KINDS.index(kind)])
    a = M.stress_acts(rng, (1, C, 16, 16), kind)[0]
    if kind == 'tame':
        w = (rng.standard_normal((64, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    else:
        w = M.stress_weights(rng, 64, C)
    return M.im2col(a), M.w2col(w)


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("kind", KINDS)
def test_model_stays_under_its_bound(kind, C):
    """Measured max(err / T) over 256 pixels x 64 channels, K = 288 / 1152 / 4608 -- PARTS 2: tame 0.59 / 0.76 / 0.86,
    pos 0.66 / 0.70 / 0.82, signed 0.74 / 0.66 / 0.71, big 0.60 / 0.62 / 0.76; PARTS 1: 0.44 .. 0.55 over the twelve sets.
    Anything >= 1 means the model or the bound is wrong."""
    A, W = operands(kind, C)
    ref = A.astype(np.float64) @ W.astype(np.float64)
    for parts in (2, 1):
        T = M.threshold_gemm(A, W, ref, parts)
        r = M.ratio_report(f"model PARTS {parts} {kind} K={A.shape[1]}", M.model_gemm(A, W, parts), ref, T)
        assert r.max() < 1.0


@pytest.mark.parametrize("defect,kind,C", [(d, k, c) for d in M.DEFECTS for k in KINDS for c in CHANNELS
                                           if not (d == 'flush_subnormal_h' and k == 'tame')])
def test_single_defects_exceed_the_allowed_error(defect, kind, C):
    """Measured max(err / T) of the defective models, smallest .. largest over the operand sets and K: l_w of one tap lost
    200 .. 763, l_a of one 16-channel chunk lost 47 .. 750, 2^-10 for 2^-11 728 .. 2173, subnormal h flushed 3.0e4 .. 1.1e5:
    the mildest exceeds the 4 T of the GPU tests by a factor 11.  Flushed subnormals need operands below 2^-14: the tame set
    (normal draws) has none that matter and is left out for that defect alone."""
    A, W = operands(kind, C)
    ref = A.astype(np.float64) @ W.astype(np.float64)
    T = M.threshold_gemm(A, W, ref, 2)
    r = M.ratio_report(f"defect {defect} {kind} K={A.shape[1]}", M.model_gemm(A, W, 2, defect), ref, T)
    assert r.max() > M.FACTOR


def silu64(a):
    a = a.astype(np.float64)
    return a / (1.0 + np.exp(-a))


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("kind", ('tame', 'signed'))
def test_staged_silu_model_and_defects_against_the_enlarged_bound(kind, C):
    """The bound's extra 2^-21 Q for a SiLU applied while staging, with the SiLU INSIDE the model (every step rounded to float32) and the
    reference float64 SiLU(A) @ W: the model must stay under 1 T and every defect above 4 T of the ENLARGED bound.  (Positive-only operands
    are left out: SiLU of the 'pos' / 'big' sets is the set itself to a few per cent.)  Measured over the six sets: model 0.36 .. 0.72 T;
    l_w of one tap lost 172 .. 378 T, l_a of one chunk lost 43 .. 357 T, 2^-10 for 2^-11 532 .. 1,101 T, subnormal h flushed 2.1e4 .. 4.9e4 T."""
    A, W = operands(kind, C, seed=1)
    S = silu64(A)
    ref = S @ W.astype(np.float64)
    T = M.threshold_gemm(S, W, ref, 2, pre_silu=True)
    r = M.ratio_report(f"model + staged SiLU {kind} K={A.shape[1]}", M.model_gemm(A, W, 2, pre_silu=True), ref, T)
    assert r.max() < 1.0
    for defect in M.DEFECTS:
        if defect == 'flush_subnormal_h' and kind == 'tame':
            continue
        r = M.ratio_report(f"defect {defect} + staged SiLU {kind} K={A.shape[1]}", M.model_gemm(A, W, 2, defect, pre_silu=True), ref, T)
        assert r.max() > M.FACTOR, defect


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("kind", KINDS)
def test_h_only_defects_exceed_the_allowed_error(kind, C):
    """What 4 T of the PARTS 1 bound (coefficient 2^-9) still catches on the h-only forms: one 16-channel chunk of one tap not multiplied,
    and subnormal halves flushed (where the operands have any).  Measured over the twelve sets: 120 .. 567 T and 7.5 .. 69 T."""
    A, W = operands(kind, C)
    ref = A.astype(np.float64) @ W.astype(np.float64)
    T = M.threshold_gemm(A, W, ref, 1)
    for defect in M.DEFECTS_H:
        if defect == 'flush_subnormal_h' and kind == 'tame':
            continue
        r = M.ratio_report(f"PARTS 1 defect {defect} {kind} K={A.shape[1]}", M.model_gemm(A, W, 1, defect), ref, T)
        assert r.max() > M.FACTOR, defect
