"""CPU: the restatements of tests/trainmm_model.py (wgrad_split, the fp32 weight gradient, gemm_split) against float64 -- each stays below
1 T of its derived bound and equals the integer reference bit for bit on the exact operands -- and every single defect either exceeds the
FACTOR T the GPU tests allow or breaks bit-equality (the [trainmm] lines say which; profiles/trainmm_report.txt records them).  The
geometry of every wgrad_split case comes from the library's own plan query (host code, no GPU), never from a copy of its planner."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trainmm_model as M


@functools.lru_cache(maxsize=None)
def plan(case):
    import __graft_entry__ as g
    g.build()
    from yond_public_amd import _lib as L
    out = (ctypes.c_int * 5)()
    assert L.load().yond_conv_wgrad_split_plan(*case, out) == 0
    return tuple(out)


def say(msg):
    print(f"[trainmm] {msg}")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# references and geometry
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,stride,H,W", [(0, 1, 5, 7), (0, 2, 5, 7), (0, 2, 4, 6), (1, 2, 3, 5), (2, 1, 3, 5)])
def test_numpy_reference_equals_conv2d_autograd(mode, stride, H, W):
    """wgrad_ref (the reference of every test here) against torch's float64 autograd of the layer itself."""
    rng = np.random.default_rng(mode + stride)
    N, ci, co = 2, 3, 4
    x = rng.standard_normal((N, H, W, ci))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    if mode == 0:
        w = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xt, w, stride=stride, padding=1)
    elif mode == 1:
        w = torch.zeros(ci, co, 2, 2, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(xt, w, stride=2)
    else:
        w = torch.zeros(co, ci, 1, 1, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xt, w)
    dy = rng.standard_normal(tuple(y.permute(0, 2, 3, 1).shape))
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    got = M.wgrad_ref(x, dy, mode, stride)                                     # [taps][co][ci]
    want = w.grad.numpy()
    want = want.transpose(2, 3, 0, 1).reshape(-1, co, ci) if mode != 1 else want.transpose(2, 3, 1, 0).reshape(-1, co, ci)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_wgrad_split_cases_reach_their_geometry():
    """Every case of WGS_CASES reaches the configuration, slice structure, boundary kind and ring wraps it is listed for, by the library's plan;
    the first unsupported widths have no plan and no workspace.  The widths the [trainmm] lines record are the query's, not a reading of the code."""
    from yond_public_amd import _lib as L
    for case, want in M.WGS_CASES:
        p = plan(case)
        f = M.check_facts(case, p, want)
        say(f"plan {case}: cfg {p[0]} nslices {p[1]} steps/slice {p[2]} ring {p[3]} lds {p[4]}; steps {f['steps']} boundaries {sorted(f['boundaries'])} "
            f"wraps {f['wraps']} ring % SK {f['ring_mod']} lead > SK {f['lead_gt_sk']} last step's pixels {f['tail']}")
    for case in M.WGS_UNSUPPORTED:
        assert plan(case) == (0, 0, 0, 0, 0) and L.load().yond_conv_wgrad_split_ws_bytes(*case) == 0
        prev = (case[0], case[1], case[2] - 1) + case[3:]
        assert plan(prev)[0] != 0
        say(f"plan {case}: unsupported (W = {case[2] - 1} is cfg {plan(prev)[0]})")
    lib = L.load()
    assert lib.yond_conv_wgrad_split_plan(1, 2, 3, 32, 32, None) == -1                 # a null out is refused
    for bad in ((1, 2, 3, 24, 32), (1, 2, 3, 32, 48), (0, 2, 3, 32, 32), (1, 0, 3, 32, 32), (1, 2, 0, 32, 32)):
        assert plan(bad) == (0, 0, 0, 0, 0) and lib.yond_conv_wgrad_split_ws_bytes(*bad) == 0
    for case, _ in M.WGS_CASES:                                                        # the workspace is the plan's slices, with room for the bias sums
        assert lib.yond_conv_wgrad_split_ws_bytes(*case) == plan(case)[1] * (9 * case[3] * case[4] + case[4]) * 4
    kinds = set()
    for case, want in M.WGS_CASES:
        kinds |= M.wgs_facts(case, plan(case))['boundaries']
    assert kinds == {'in_row', 'halo_col', 'image'}
    assert {want['cfg'] for _, want in M.WGS_CASES} == {1, 2, 3, 4, 5}


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad_split
# ---------------------------------------------------------------------------------------------------------------------------
def hard(case):
    return M.hard_wgrad(np.random.default_rng([41] + list(case)), *case)


@pytest.mark.parametrize("case", M.WGS_HARD)
def test_wgrad_split_model_stays_under_its_bound(case):
    x, dy = hard(case)
    p = plan(case)
    ref, T, dbref, Tdb = M.wgs_threshold(x, dy, p)
    dw, db = M.wgs_model(x, dy, p)
    r, rb = M.ratio(dw, ref, T), M.ratio(db, dbref, Tdb)
    ci, co = case[3], case[4]
    share = M.zero_share(T)
    say(f"wgrad_split model {case} cfg {p[0]}: dw {r:.3f} T, db {rb:.3f} T; T = 0 on {100 * share:.2f} % of dw (the zero channels: {100 * (ci + co - 1) / (ci * co):.2f} %), "
        f"dy below 2^-14: {100 * np.mean((dy != 0) & (np.abs(dy) < 2.0 ** -14)):.0f} %")
    assert r <= 1.0 and rb <= 1.0
    assert share == (ci + co - 1) / (ci * co) and M.zero_share(Tdb) == 1 / co           # only the deliberately zero channels
    assert np.all(dw[:, 5] == 0) and np.all(dw[:, :, 3] == 0) and db[5] == 0


DENSE = [(c, k) for c in ((3, 7, 33, 32, 32), (2, 9, 40, 64, 64), (1, 5, 38, 64, 64), (1, 70, 1, 64, 64), (3, 7, 33, 32, 64), (1, 5, 6, 384, 192))
         for k in ('plain', 'lx', 'ldy')]


def dense(case, kind):
    return M.dense_wgrad(np.random.default_rng([43] + list(case)), *case, kind=kind)


@pytest.mark.parametrize("case,kind", DENSE)
def test_wgrad_split_model_is_exact_on_dense_operands(case, kind):
    x, dy = dense(case, kind)
    ref = M.wgrad_ref(x, dy).astype(np.float32)
    dbref = dy.astype(np.float64).reshape(-1, case[4]).sum(0).astype(np.float32)
    dw, db = M.wgs_model(x, dy, plan(case), with_bias=3)
    assert np.array_equal(bits(dw), bits(M.to_oihw(ref))) and np.array_equal(bits(db), bits(dbref))
    assert np.array_equal(bits(M.wgs_model(x, dy, plan(case), with_bias=0)[0]), bits(ref))


def test_wgrad_split_defects_are_caught():
    """Every defect of WGS_DEFECTS on every hard case (worst err / T) and every dense case (bit-equal or not).  A defect must be caught by one of
    the two; the table says by which.  Known by construction: P_from_v cannot show on dense operands (an fp16-exact value has P = 2^11 h either
    way) -- the bound catches it where dy lies below fp16's normal range; the l halves show on the dense kinds that have them (lx, ldy)."""
    table = {}
    for d in M.WGS_DEFECTS:
        wb = 3 if d == 'oihw_swap' else 1
        by_bound, by_bits = [], []
        for case in M.WGS_HARD:
            x, dy = hard(case)
            p = plan(case)
            ref, T, dbref, Tdb = M.wgs_threshold(x, dy, p)
            dw, db = M.wgs_model(x, dy, p, with_bias=wb, defect=d)
            r = max(M.ratio(dw, M.to_oihw(ref) if wb & 2 else ref, M.to_oihw(T) if wb & 2 else T), M.ratio(db, dbref, Tdb))
            if r > M.FACTOR:
                by_bound.append((case, r))
        for case, kind in DENSE:
            x, dy = dense(case, kind)
            p = plan(case)
            ref = M.wgrad_ref(x, dy).astype(np.float32)
            dbref = dy.astype(np.float64).reshape(-1, case[4]).sum(0).astype(np.float32)
            dw, db = M.wgs_model(x, dy, p, with_bias=wb, defect=d)
            if not (np.array_equal(bits(dw), bits(M.to_oihw(ref) if wb & 2 else ref)) and np.array_equal(bits(db), bits(dbref))):
                by_bits.append((case, kind))
        table[d] = (by_bound, by_bits)
        short = lambda c: "x".join(str(v) for v in c[:3]) + f":{c[3]}>{c[4]}"
        say(f"defect {d}: over {M.FACTOR:g} T on {len(by_bound)} of {len(M.WGS_HARD)} hard cases"
            + (" [" + ", ".join(f"{short(c)} {r:.3g}" for c, r in by_bound) + "]" if by_bound else " -- INVISIBLE to the bound")
            + f"; breaks bit-equality on {len(by_bits)} of {len(DENSE)} dense cases"
            + (" [" + ", ".join(f"{short(c)} {k}" for c, k in by_bits) + "]" if by_bits else " -- INVISIBLE to the exact operands (the bound is what catches it)"))
    for d, (by_bound, by_bits) in table.items():
        assert by_bound or by_bits, d
        if d != 'P_from_v':
            assert by_bits, d
    for d in ('drop_l_dy_step', 'drop_l_x_step', 'P_from_v', 'scale_2e-10', 'halo_leak', 'oihw_swap'):
        assert table[d][0], d


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32-MFMA weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def out_shape(mode, stride, H, W):
    return ((H + stride - 1) // stride, (W + stride - 1) // stride) if mode == 0 else ((2 * H, 2 * W) if mode == 1 else (H, W))


WG32 = [(0, 1, 3, 7, 33, 32, 32), (0, 2, 3, 7, 33, 64, 32), (1, 2, 3, 7, 5, 32, 32), (2, 1, 3, 7, 33, 32, 64)]


@pytest.mark.parametrize("mode,stride,N,H,W,ci,co", WG32)
def test_fp32_wgrad_sim_under_its_bound_and_exact(mode, stride, N, H, W, ci, co):
    """The structure-faithful float32 simulation with a chunk of two K-space rows per wave (chunks straddle the images: H = 7): below 1 T on the
    hard operands, workspace and atomics; bit-equal on integers; the half-empty last pair of an odd row, dropped, is caught by both."""
    Ho, Wo = out_shape(mode, stride, H, W)
    rng = np.random.default_rng([47, mode, stride])
    x, _ = M.hard_wgrad(rng, N, H, W, ci, co)
    _, dy = M.hard_wgrad(rng, N, Ho, Wo, ci, co)
    chunk = 2
    for use_ws in (True, False):
        ref, T = M.wg32_threshold(x, dy, mode, stride, chunk, use_ws)
        r = M.ratio(M.wg32_sim(x, dy, mode, stride, chunk, use_ws), ref, T)
        rd = M.ratio(M.wg32_sim(x, dy, mode, stride, chunk, use_ws, defect='drop_odd_tail'), ref, T)
        say(f"fp32 wgrad sim mode {mode} stride {stride} {'workspace' if use_ws else 'atomics'}: {r:.3f} T; last pixel of an odd row dropped: {rd:.3g} T; "
            f"T = 0 on {100 * M.zero_share(T):.2f} %")
        assert r <= 1.0 and rd > M.FACTOR
        assert M.zero_share(T) == (ci + co - 1) / (ci * co)
    xi = M.dense_int(rng, x.shape, 8, N * H * W, 8)
    di = M.dense_int(rng, dy.shape, 8, N * H * W, 8)
    want = M.wgrad_ref(xi, di, mode, stride).astype(np.float32)
    for use_ws in (True, False):
        assert np.array_equal(bits(M.wg32_sim(xi, di, mode, stride, chunk, use_ws)), bits(want))
        assert not np.array_equal(bits(M.wg32_sim(xi, di, mode, stride, chunk, use_ws, defect='drop_odd_tail')), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_split
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_forward_case(rng, P, c0, c1, cout, ints):
    """A 1x1 convolution over one or two sources, channels padded to 32 with NONZERO padding columns in x (the k mask must kill them).
    Returns xs (padded), the flat weight, the sources' descriptions for gemm_B, bias."""
    rup = lambda c: (c + 31) // 32 * 32
    cin = c0 + c1
    if ints:
        w = M.dense_int(rng, (cout, cin), 31, rup(c0) + rup(c1), 8)
        xs = [M.dense_int(rng, (P, rup(c)), 8, rup(c0) + rup(c1), 31) for c in (c0, c1) if c]
        b = M.dense_int(rng, (cout,), 100, 1, 1)
    else:
        xa, w = M.hard_gemm(rng, P, cin, cout)
        xs, o = [], 0
        for c in (c0, c1):
            if c:
                q = (rng.standard_normal((P, rup(c))) * 100).astype(np.float32)
                q[:, :c] = xa[:, o:o + c]
                xs.append(q)
                o += c
        b = (10.0 ** rng.uniform(-2, 2, cout)).astype(np.float32)
    return xs, w, b


def gemm_forward(xs, w, b, c0, c1, cout, defect=None):
    rup = lambda c: (c + 31) // 32 * 32
    cin, n_p = c0 + c1, rup(cout)
    flat = w.reshape(-1)
    Bs, off = [], 0
    for x, c in zip(xs, [c for c in (c0, c1) if c]):
        Bs.append(M.gemm_B(flat[off:], 1, 0, 1 << 30, x.shape[1], c, cin, 0, 1 << 30, n_p, cout, defect))
        off += c
    return Bs, M.gemm_bias(b, 1 << 30, n_p, cout)


@pytest.mark.parametrize("P,c0,c1,cout", [(129, 32, 32, 32), (127, 40, 24, 8), (257, 96, 0, 40)])
def test_gemm_split_model_bound_exactness_and_masks(P, c0, c1, cout):
    rng = np.random.default_rng([53, P])
    xs, w, b = gemm_forward_case(rng, P, c0, c1, cout, ints=False)
    Bs, bn = gemm_forward(xs, w, b, c0, c1, cout)
    ref, T = M.gemm_threshold(xs, Bs, bn)
    r = M.ratio(M.gemm_model(xs, Bs, bn), ref, T)
    say(f"gemm_split model P {P} {c0}+{c1}->{cout}: {r:.3f} T; T = 0 on {100 * M.zero_share(T):.2f} % (the zero weight row and the padding columns)")
    assert r <= 1.0
    xi, wi, bi = gemm_forward_case(rng, P, c0, c1, cout, ints=True)
    Bi, bni = gemm_forward(xi, wi, bi, c0, c1, cout)
    want = (np.concatenate(xi, 1).astype(np.float64) @ np.concatenate(Bi, 0).astype(np.float64) + bni).astype(np.float32)
    assert np.array_equal(bits(M.gemm_model(xi, Bi, bni)), bits(want))
    assert np.all(want[:, cout:] == 0)
    for d in ('k_mask_block', 'n_mask_block'):
        padded = (c0 % 32 or c1 % 32) if d == 'k_mask_block' else cout % 32
        Bd, bd = gemm_forward(xs, w, b, c0, c1, cout, d)
        rd = M.ratio(M.gemm_model(xs, Bd, bd), ref, T)
        Bdi, bdi = gemm_forward(xi, wi, bi, c0, c1, cout, d)
        broke = not np.array_equal(bits(M.gemm_model(xi, Bdi, bdi)), bits(want))
        say(f"defect {d} P {P} {c0}+{c1}->{cout}: {rd:.3g} T, breaks bit-equality: {broke}" + ("" if padded else " (no padding in this case: nothing to see)"))
        assert (rd > M.FACTOR and broke) if padded else (rd <= 1.0 and not broke)


def test_gemm_split_shuffle_store_and_its_swap():
    """The transposed 2x2 layer: weights [ci][co][2][2] read in place (sk_lo = 4 cout, nblk = cop, sn_lo = 4, sn_hi = 1), n = j cop + co stored to
    pixel (2 yy + j / 2, 2 xx + j % 2) -- against conv_transpose2d in float64; the swapped store is caught by bound and bits."""
    rng = np.random.default_rng(59)
    N, H, W, cin, cout = 2, 3, 5, 40, 24
    cip, cop = 64, 32
    for ints in (False, True):
        if ints:
            x, w, b = M.dense_int(rng, (N * H * W, cip), 8, cip, 31), M.dense_int(rng, (cin, cout, 2, 2), 31, cip, 8), M.dense_int(rng, (cout,), 100, 1, 1)
        else:
            xa, wa = M.hard_gemm(rng, N * H * W, cin, 4 * cout, zero_n=7)
            x = (rng.standard_normal((N * H * W, cip)) * 100).astype(np.float32)
            x[:, :cin] = xa
            w = np.ascontiguousarray(wa.reshape(cout, 2, 2, cin).transpose(3, 0, 1, 2))
            b = (10.0 ** rng.uniform(-2, 2, cout)).astype(np.float32)
        B = M.gemm_B(w, 4 * cout, 0, 1 << 30, cip, cin, 4, 1, cop, 4 * cop, cout)
        bn = M.gemm_bias(b, cop, 4 * cop, cout)
        ref, T = M.gemm_threshold([x], [B], bn)
        ref, T = M.shuffle_store(ref, N, H, W), M.shuffle_store(T, N, H, W)
        want = F.conv_transpose2d(torch.from_numpy(x[:, :cin].astype(np.float64).reshape(N, H, W, cin)).permute(0, 3, 1, 2), torch.from_numpy(w.astype(np.float64)),
                                  torch.from_numpy(b.astype(np.float64)), stride=2).permute(0, 2, 3, 1).numpy()
        assert np.allclose(ref[..., :cout], want, rtol=1e-12, atol=1e-9) and np.all(ref[..., cout:] == 0)
        got, bad = M.gemm_model([x], [B], bn, (N, H, W)), M.gemm_model([x], [B], bn, (N, H, W), defect='shuffle_swap')
        if ints:
            assert np.array_equal(bits(got), bits(ref.astype(np.float32))) and not np.array_equal(bits(bad), bits(ref.astype(np.float32)))
        else:
            r, rd = M.ratio(got, ref, T), M.ratio(bad, ref, T)
            say(f"gemm_split model transposed 2x2 {N}x{H}x{W} {cin}->{cout}: {r:.3f} T; defect shuffle_swap {rd:.3g} T")
            assert r <= 1.0 and rd > M.FACTOR
