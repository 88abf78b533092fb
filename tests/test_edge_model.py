"""CPU: the float64 models of tests/edge_model.py (the forward's edge layers and glue kernels) against torch float64 statements of the
operations, their bounds against float32 restatements of the kernels' own steps (worst ratio printed, at most 1) on every operand set of
the GPU module's case tables, and single defects against the bounds (each must exceed its bound on every case that exercises its code
path).  The exact operations against independent reshape / transpose statements.  The GPU counterpart is tests/test_hip_edge_layers.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_model as M


def show(name, r):
    print(f"[bound] {name}: worst |restatement - model| / bound = {r:.3f}")
    return r


def close(a, b, axis=-1):
    """|a - b| <= 1e-12 (|b| + the largest |b| along every axis but `axis`): relative to the element's own channel, not to the loudest one."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    other = tuple(i for i in range(b.ndim) if i != axis % b.ndim)
    scale = np.abs(b) + np.abs(b).max(axis=other, keepdims=True)
    return bool(np.all(np.abs(a - b) <= 1e-12 * scale))


T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
nchw = lambda a: T(a).permute(0, 3, 1, 2)


def staged(x, ub):
    """float32(x / ub) formed by torch in float32 -- the kernels' own first step and an exact operand of the float64 statement."""
    x = torch.from_numpy(np.array(x, np.float32))
    if ub is None:
        return x.double()
    return (x / torch.from_numpy(np.array(ub, np.float32)).view(-1, *([1] * (x.dim() - 1)))).double()


# ---------------------------------------------------------------------------------------------------------------------------
# the models are the operations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.CONV_IN_SHAPES)
def test_conv_in_model_equals_float64_conv2d(shape):
    ops = M.conv_in_operands(*shape)
    for has_ub, has_bias, slope in M.CONV_IN_VARIANTS:
        x, ub, w, bias = M.pick(ops, (True, has_ub, True, has_bias))
        a = staged(x, ub).permute(0, 3, 1, 2)
        ref = F.leaky_relu(F.conv2d(a, T(w), None if bias is None else T(bias), padding=1), float(np.float32(slope)))
        assert close(M.conv_in_model(x, ub, w, bias, slope)[0], ref.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("shape", M.CONV_OUT_SHAPES)
def test_conv_out_model_equals_float64_statement(shape):
    ops = M.conv_out_operands(*shape)
    for has_x, has_ub, has_bias in M.CONV_OUT_VARIANTS:
        feat, w, bias, x, ub = M.pick(ops, (True, True, has_bias, has_x, has_ub))
        ref = F.conv2d(nchw(feat), T(w)[:, :, None, None], None if bias is None else T(bias))
        if x is not None:
            ref = ref + staged(x, ub).permute(0, 3, 1, 2)
        if ub is not None:
            ref = ref * T(ub).view(-1, 1, 1, 1)
        assert close(M.conv_out_model(feat, w, bias, x, ub)[0], ref.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("has_ub", [True, False])
def test_film_model_equals_float64_modules(has_ub):
    """The archs modules' formulas written out: gamma / sfm1 = conv1x1(SiLU(conv1x1(t))), beta = conv1x1(SiLU(gamma)), sfm2 likewise from t; the
    epilogue pairs fold the conv biases: (s1, t1) = (m1, cb1 m1 + beta) / (m1, cb1 m1), (s2, t2) = (1, cb2) / (m2, cb2 m2)."""
    t, ub = M.film_t(7)
    ub = ub if has_ub else None
    tv = staged(t, ub).view(-1, 1, 1, 1)
    for d in M.film_descs():
        C = d['C']
        c1 = lambda v, wv, bv: F.conv2d(v, T(wv).reshape(C, -1, 1, 1), T(bv))
        m1 = c1(F.silu(c1(tv, d['w_a0'], d['b_a0'])), d['w_a2'], d['b_a2'])
        cb1, cb2 = T(d['cb1']).view(1, C, 1, 1), T(d['cb2']).view(1, C, 1, 1)
        if d['kind'] == 0:
            ref = {'s1': m1, 't1': cb1 * m1 + c1(F.silu(m1), d['w_b'], d['b_b']), 's2': torch.ones_like(m1), 't2': cb2.expand_as(m1)}
        else:
            m2 = c1(F.silu(c1(tv, d['w_b0'], d['b_b0'])), d['w_b'], d['b_b'])
            ref = {'s1': m1, 't1': cb1 * m1, 's2': m2, 't2': cb2 * m2}
        mod = M.film_model(d, t, ub)
        for k in M.FILM_OUT:
            assert close(mod[k][0], ref[k].reshape(-1, C).numpy()), (d['kind'], C, k)


@pytest.mark.parametrize("shape", M.EST_CONV_IN_SHAPES)
def test_est_conv_in_model_equals_float64_conv2d(shape):
    x, w, bias = M.est_conv_in_operands(*shape)
    ref = F.relu(F.conv2d(T(x)[:, None], T(w).reshape(-1, 1, 3, 3), T(bias), padding=1))
    assert close(M.est_conv_in_model(x, w, bias)[0], ref.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("case", M.EST_HEAD_CASES)
def test_est_head_model_equals_float64_conv2d_square_mean(case):
    H, W, Cin, nc, sq = case
    feat, w, bias = M.est_head_operands(M.EST_HEAD_N, H, W, Cin, nc)
    ref = F.conv2d(nchw(feat), T(w)[:, :, None, None], T(bias))
    if sq:
        ref = ref * ref
    assert close(M.est_head_model(feat, w, bias, sq, 0)[0], ref.numpy(), axis=1)
    assert close(M.est_head_model(feat, w, bias, sq, 1)[0], ref.mean(dim=(2, 3)).numpy(), axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds hold the kernels' own steps and bite on single defects, on every operand set of the GPU module's tables
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.CONV_IN_SHAPES)
def test_conv_in_bound_holds_restatement_and_bites(shape):
    ops = M.conv_in_operands(*shape)
    for has_ub, has_bias, slope in M.CONV_IN_VARIANTS:
        x, ub, w, bias = M.pick(ops, (True, has_ub, True, has_bias))
        val, bnd = M.conv_in_model(x, ub, w, bias, slope)
        tag = f"conv_in {shape} ub {has_ub} bias {has_bias} slope {slope}"
        assert show(tag, M.ratio(M.conv_in_f32(x, ub, w, bias, slope), val, bnd)) <= 1.0, tag
        for d in M.conv_in_defects(shape, has_ub, has_bias):
            assert M.ratio(M.conv_in_f32(x, ub, w, bias, slope, defect=d), val, bnd) > 1.0, (tag, d)


def test_conv_in_defect_list_is_complete():
    seen = {d for s in M.CONV_IN_SHAPES for u, b, _ in M.CONV_IN_VARIANTS for d in M.conv_in_defects(s, u, b)}
    assert seen == {'taps_dxdy', 'tap9_w8', 'bias_group', 'plane_off', 'ub_prev'}


@pytest.mark.parametrize("shape,variant", M.conv_out_cases())
def test_conv_out_bound_holds_restatement_and_bites(shape, variant):
    has_x, has_ub, has_bias = variant
    feat, w, bias, x, ub = M.pick(M.conv_out_operands(*shape), (True, True, has_bias, has_x, has_ub))
    val, bnd = M.conv_out_model(feat, w, bias, x, ub)
    tag = f"conv_out {shape} x {has_x} ub {has_ub} bias {has_bias}"
    assert show(tag, M.ratio(M.conv_out_f32(feat, w, bias, x, ub), val, bnd)) <= 1.0, tag
    for d in M.conv_out_defects(has_x, has_ub):
        assert M.ratio(M.conv_out_f32(feat, w, bias, x, ub, defect=d), val, bnd) > 1.0, (tag, d)


@pytest.mark.parametrize("N", M.FILM_N)
@pytest.mark.parametrize("has_ub", [True, False])
def test_film_bound_holds_restatement_and_bites(N, has_ub):
    t, ub = M.film_t(N)
    ub = ub if has_ub else None
    seen = set()
    for d in M.film_descs():
        mod = M.film_model(d, t, ub)
        tag = f"film kind {d['kind']} C {d['C']} N {N} ub {has_ub}"
        assert show(tag, M.film_check(M.film_f32(d, t, ub), mod, d['C'])) <= 1.0, tag
        for df in M.film_defects(d, has_ub):
            seen.add(df)
            assert M.film_check(M.film_f32(d, t, ub, defect=df), mod, d['C']) > 1.0, (tag, df)
    assert seen == {'clamp_row', 'snr_t2_m1'} | ({'t_no_ub'} if has_ub else set())


@pytest.mark.parametrize("shape", M.EST_CONV_IN_SHAPES)
def test_est_conv_in_bound_holds_restatement_and_bites(shape):
    x, w, bias = M.est_conv_in_operands(*shape)
    val, bnd = M.est_conv_in_model(x, w, bias)
    assert show(f"est_conv_in {shape}", M.ratio(M.est_conv_in_f32(x, w, bias), val, bnd)) <= 1.0
    if shape[1] > 1 or shape[2] > 1:
        assert M.ratio(M.est_conv_in_f32(x, w, bias, defect='taps_dxdy'), val, bnd) > 1.0


@pytest.mark.parametrize("case", M.EST_HEAD_CASES)
def test_est_head_bound_holds_restatement_and_bites(case):
    H, W, Cin, nc, sq = case
    feat, w, bias = M.est_head_operands(M.EST_HEAD_N, H, W, Cin, nc)
    for pge in (0, 1):
        val, bnd = M.est_head_model(feat, w, bias, sq, pge)
        tag = f"est_head {case} pge {pge}"
        assert show(tag, M.ratio(M.est_head_f32(feat, w, bias, sq, pge), val, bnd)) <= 1.0, tag
        for d in M.est_head_defects(sq, pge):
            assert M.ratio(M.est_head_f32(feat, w, bias, sq, pge, defect=d), val, bnd) > 1.0, (tag, d)


def test_est_head_cases_cover_every_value():
    cs = M.EST_HEAD_CASES
    assert {c[2] for c in cs} == {4, 32, 60, 256} and {c[3] for c in cs} == {1, 2, 3, 4} and {c[4] for c in cs} == {0, 1}
    assert {c[0] * c[1] for c in cs} == {1, 15, 17, 8193}
    assert all(c[0] * c[1] % M.EST_PPI for c in cs)                  # the strided count never equals HW: 'mean_strided' is always exercised


# ---------------------------------------------------------------------------------------------------------------------------
# the exact operations against independent statements
# ---------------------------------------------------------------------------------------------------------------------------
def test_conv_in_pack_layout():
    w = np.arange(64 * 4 * 9, dtype=np.float32).reshape(64, 4, 3, 3) + 1
    p = M.conv_in_pack(w).reshape(2, 5, 2, 32, 4)
    for ct, up, h, j, e in [(0, 0, 0, 0, 0), (1, 3, 1, 17, 2), (0, 4, 0, 31, 3), (1, 2, 0, 5, 1)]:
        tap = 2 * up + h
        assert p[ct, up, h, j, e] == w[ct * 32 + j, e, tap // 3, tap % 3]
    assert np.all(p[:, 4, 1] == 0) and np.count_nonzero(p) == w.size
    q = np.arange(2 * 3 * 5 * 8, dtype=np.float32).reshape(2, 3, 5, 8)                  # NHWC, C = 8
    p4 = np.empty((2, 2, 15, 4), np.float32)                                            # [N][C/4][H*W][4]
    for n in range(2):
        for y in range(3):
            for x in range(5):
                p4[n, 0, y * 5 + x], p4[n, 1, y * 5 + x] = q[n, y, x, :4], q[n, y, x, 4:]
    assert np.array_equal(M.planes4_to_nhwc(p4.reshape(-1), 2, 3, 5, 8), q)


@pytest.mark.parametrize("shape", M.MAXPOOL_SHAPES)
def test_maxpool2_model(shape):
    N, H, W, C = shape
    assert (N * (H // 2) * (W // 2) * (C // 4)) % 256 != 0
    for kind in ('mixed', 'negative', 'neginf'):
        x = M.maxpool_operands(shape, kind)
        ref = x.reshape(N, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))
        assert np.array_equal(M.maxpool2_model(x), ref)
        assert np.array_equal(M.maxpool2_model(x), F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy())
        assert kind == 'mixed' or (x < 0).all()
        assert kind != 'neginf' or np.isneginf(M.maxpool2_model(x)[0, 0, 0]).all()


def test_layout_models():
    b = M.exact_operands((6, 10))
    p = b.reshape(3, 2, 5, 2).transpose(0, 2, 1, 3).reshape(3, 5, 4)
    assert np.array_equal(M.bayer2rggb_model(b), p) and np.array_equal(M.rggb2bayer_model(p), b)
    x = M.exact_operands((3, 4, 5, 7))
    assert np.array_equal(M.nchw4_to_nhwc4_model(x), x.transpose(0, 2, 3, 1))
    assert np.array_equal(M.nhwc4_to_nchw4_model(x.transpose(0, 2, 3, 1)), x)
    s = M.exact_operands((2, 10, 14))
    for k in range(-1, 6):
        ref = {0: s, 1: s.transpose(0, 2, 1)[:, ::-1, :], 2: s[:, ::-1, ::-1], 3: s.transpose(0, 2, 1)[:, :, ::-1]}[k % 4]
        assert np.array_equal(M.rot90_model(s, k), ref)
    assert np.array_equal(M.rot90_model(M.rot90_model(s, 1), 3), s)


def test_image_max_model_and_operands():
    for N in M.IMAGE_MAX_N:
        for elems in M.IMAGE_MAX_ELEMS[:4]:
            for kind in M.IMAGE_MAX_KINDS:
                x = M.image_max_operands(N, elems, kind)
                got = M.image_max_model(x)
                for n in range(N):
                    v = x[n][~np.isnan(x[n])]
                    assert got[n] == (v.max() if v.size else -np.inf)
                assert kind == 'nan' or (x < 0).all()
    x = M.image_max_operands(3, M.IMAGE_MAX_ELEMS[-1], 'tail')
    assert np.all(np.argmax(x, axis=1) == 256 * 4096)                 # the one element the 256 workgroups reach only in their 17th pass
    x = M.image_max_operands(3, 4097, 'nan')
    assert np.isnan(x[1]).all() and np.isneginf(M.image_max_model(x)[1]) and np.isnan(x[0, 0]) and M.image_max_model(x)[0] == np.float32(-0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# host guard of the FiLM launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_film_plan_refuses_blocks_wider_than_the_kernel_stages():
    """film_kernel stages a block's vector in 1024 floats of LDS: DenoiserPlan._film must refuse a wider block before it allocates or
    launches anything (a plan made by __new__ has no device, no parameters and no library: reaching any of them would raise AttributeError)."""
    from yond_public_amd.engine import DenoiserPlan, FILM_MAX_C
    assert FILM_MAX_C == 1024
    plan = DenoiserPlan.__new__(DenoiserPlan)
    plan._film_spec = [('conv5_1', 2048)]
    plan._film_cache = {}
    with pytest.raises(ValueError, match='1024'):
        plan._film(None, None, 1)
    assert plan._film_cache == {}
