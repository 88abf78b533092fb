"""GPU: the training step's three matrix-core kernels -- yond_conv_wgrad_split_f32 (csrc/wgrad_split.hip), yond_conv_wgrad_ws_f32 / yond_conv_wgrad_f32
(csrc/train.hip: wgrad_rows_kernel, wgrad_reduce64_kernel) and yond_gemm_split_f32 (csrc/gemm_split.hip) -- against the float64 references and the
derived per-element bounds of tests/trainmm_model.py, at the kernels' own tiling edges.

Two kinds of operands.  Dense exact ones (small integers, or integers times a power of two whose l halves are nonzero): every product and every
partial sum in any order is exact, so the kernel must equal the reference BIT FOR BIT -- one wrong, lost or doubled product anywhere shows.  Hard
ones (split_model's stress statistics, gradients below fp16's normal range, a quiet, a zero output channel and a zero input channel): err <= FACTOR T
per element.  Every wgrad_split case asserts, through yond_conv_wgrad_split_plan, that it reaches the geometry it is listed for
(trainmm_model.WGS_CASES).  Every output lives in a NaN-filled guard-banded buffer, every workspace starts as NaN.
The [parity] lines are what profiles/trainmm_report.txt records."""
import ctypes
import types

import numpy as np
import pytest
import torch

import trainmm_model as M
from test_hip_train_edges import Guard, wgrad_chunk, dev, bits, lib_, DEV

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -2


def plan(case):
    _, lib = lib_()
    out = (ctypes.c_int * 5)()
    assert lib.yond_conv_wgrad_split_plan(*case, out) == 0
    return tuple(out)


def parity(msg):
    print(f"[parity] {msg}")


def run_wgs(x, dy, with_bias, expect_status=0):
    """yond_conv_wgrad_split_f32 on NHWC numpy operands: (dw flat, db or None) from a guarded buffer, the workspace pre-filled with NaN."""
    L, lib = lib_()
    N, H, W, ci = x.shape
    co = dy.shape[-1]
    need = int(lib.yond_conv_wgrad_split_ws_bytes(N, H, W, ci, co))
    p = plan((N, H, W, ci, co))
    assert need == p[1] * (9 * co * ci + co) * 4 > 0
    ws = torch.full((need // 4,), float('nan'), device=DEV)
    g = Guard(9 * co * ci + (co if with_bias & 1 else 0))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    xd, dyd = dev(x), dev(dy)
    L.check(lib.yond_conv_wgrad_split_f32(L.ptr(xd), L.ptr(dyd), N, H, W, ci, co, g.ptr(), with_bias, L.ptr(ws), need, L.ptr(status), L.stream()), "wgrad_split")
    torch.cuda.synchronize()
    assert int(status.item()) == expect_status
    got = g.get(allow_nan=bool(expect_status))
    return got[:9 * co * ci], (got[9 * co * ci:] if with_bias & 1 else None)


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad_split
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,want", M.WGS_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}" for c, _ in M.WGS_CASES])
def test_wgrad_split_is_exact_on_dense_operands(case, want):
    """dw and the riding db, bit for bit, for with_bias 0, 1 and 3 (OIHW against the permuted reference) on the three exact operand kinds
    (plain integers; X with nonzero l halves; dY with nonzero l halves) -- after asserting that the plan reaches the case's geometry."""
    p = plan(case)
    f = M.check_facts(case, p, want)
    co = case[4]
    for kind in ('plain', 'lx', 'ldy'):
        x, dy = M.dense_wgrad(np.random.default_rng([43] + list(case)), *case, kind=kind)
        ref = M.wgrad_ref(x, dy).astype(np.float32)
        dbref = dy.astype(np.float64).reshape(-1, co).sum(0).astype(np.float32)
        for wb in (0, 1, 3):
            dw, db = run_wgs(x, dy, wb)
            want_dw = (M.to_oihw(ref) if wb & 2 else ref).reshape(-1)
            assert np.array_equal(bits(dw), bits(want_dw)), f"{kind} with_bias {wb}: {int((dw != want_dw).sum())} of {dw.size} elements differ"
            if wb & 1:
                assert np.array_equal(bits(db), bits(dbref)), f"{kind} with_bias {wb}: db differs in {int((db != dbref).sum())} channels"
    parity(f"wgrad_split dense {case}: cfg {p[0]} nslices {p[1]} steps/slice {p[2]} ring {p[3]} (boundaries {sorted(f['boundaries'])}, wraps {f['wraps']}, "
           f"last step's pixels {f['tail']}): dw and db bit-equal, 3 operand kinds x with_bias 0 / 1 / 3")


@pytest.mark.parametrize("case", M.WGS_UNSUPPORTED, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}")
def test_wgrad_split_first_unsupported_width_falls_back(case):
    """The first width without a plan: no workspace, the entry answers YOND_EUNSUPPORTED and writes nothing, and train.py's dispatch returns the
    fp32 kernel's weight gradient (exact on integers) and the column sums, in both of its forms."""
    L, lib = lib_()
    from yond_public_amd import train as TR
    N, H, W, ci, co = case
    assert plan(case) == (0, 0, 0, 0, 0) and int(lib.yond_conv_wgrad_split_ws_bytes(*case)) == 0
    assert plan((N, H, W - 1, ci, co))[0] != 0
    x, dy = M.dense_wgrad(np.random.default_rng([61] + list(case)), *case)
    xd, dyd = dev(x), dev(dy)
    g, ws = Guard(9 * co * ci + co), torch.full((1024,), float('nan'), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.yond_conv_wgrad_split_f32(L.ptr(xd), L.ptr(dyd), N, H, W, ci, co, g.ptr(), 1, L.ptr(ws), 4096, L.ptr(status), L.stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.buf).all()) and bool(torch.isnan(ws).all())
    ref = M.wgrad_ref(x, dy).astype(np.float32)
    dbref = dy.astype(np.float64).reshape(-1, co).sum(0).astype(np.float32)
    pl = types.SimpleNamespace(lib=lib, train_conv='split', wgrad_ws=None, gen=0, status=status)
    dw, db = TR._wgrad(pl, xd, dyd, 0, 1, 9, with_bias=True, oihw=True)
    dw2 = TR._wgrad(pl, xd, dyd, 0, 1, 9)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dw.cpu().numpy().reshape(co, ci, 9)), bits(M.to_oihw(ref))) and np.array_equal(bits(db.cpu().numpy()), bits(dbref))
    assert np.array_equal(bits(dw2.cpu().numpy()), bits(ref))
    parity(f"wgrad_split {case}: unsupported, the dispatch's fp32 result bit-equal to the integer reference")


@pytest.mark.parametrize("case", M.WGS_HARD, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}")
def test_wgrad_split_hard_operands_within_bound(case):
    """One shape per configuration on the hard operands: dw per element and the riding db per channel within FACTOR T, the zero channels exactly
    zero, the status word clean at max|dy| = 31.89; the OIHW form holds the same values."""
    x, dy = M.hard_wgrad(np.random.default_rng([41] + list(case)), *case)
    p = plan(case)
    ci, co = case[3], case[4]
    ref, T, dbref, Tdb = M.wgs_threshold(x, dy, p)
    assert M.zero_share(T) == (ci + co - 1) / (ci * co)
    dw, db = run_wgs(x, dy, 1)
    dw = dw.reshape(9, co, ci)
    r, rb = M.ratio(dw, ref, T), M.ratio(db, dbref, Tdb)
    quiet = M.ratio(dw[:, 7], ref[:, 7], T[:, 7])
    parity(f"wgrad_split hard {case} cfg {p[0]}: dw {r:.3f} T (quiet channel {quiet:.3f} T), db {rb:.3f} T, T = 0 on {100 * M.zero_share(T):.2f} %")
    assert r <= M.FACTOR and rb <= M.FACTOR
    assert np.all(dw[:, 5] == 0) and np.all(dw[:, :, 3] == 0) and db[5] == 0
    dwo, dbo = run_wgs(x, dy, 3)
    assert np.array_equal(bits(dwo.reshape(co, ci, 9)), bits(M.to_oihw(dw))) and np.array_equal(bits(dbo), bits(db))


def test_wgrad_split_status_word_at_the_limit():
    """amax.below(31.9f): the status word stays 0 up to the float32 just below 31.9f and carries bit 0 from 31.9f itself on, for either sign, for
    infinity and for NaN."""
    case = (2, 3, 2, 64, 32)
    x, dy = M.hard_wgrad(np.random.default_rng(67), *case)
    lim = np.float32(31.9)
    dy[0, 0, 0, 0] = 31.89
    assert np.abs(dy).max() == np.float32(31.89)
    run_wgs(x, dy, 1, expect_status=0)
    for v, want in ((np.nextafter(lim, np.float32(0)), 0), (-np.nextafter(lim, np.float32(0)), 0), (lim, 1), (-lim, 1), (np.float32(np.inf), 1),
                    (np.float32(np.nan), 1)):
        d = dy.copy()
        d[1, 2, 1, 17] = v
        run_wgs(x, d, 1, expect_status=want)
    parity("wgrad_split status: 0 at 31.89 and at the float32 below 31.9f; bit 0 at +-31.9f, inf, NaN")


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32-MFMA weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def out_shape(mode, stride, H, W):
    return ((H + stride - 1) // stride, (W + stride - 1) // stride) if mode == 0 else ((2 * H, 2 * W) if mode == 1 else (H, W))


def run_wg32(x, dy, mode, stride, use_ws):
    L, lib = lib_()
    N, H, W, ci = x.shape
    _, Ho, Wo, co = dy.shape
    taps = {0: 9, 1: 4, 2: 1}[mode]
    nws = int(lib.yond_conv_wgrad_ws_bytes(N, H, W, ci, Ho, Wo, co, mode, stride))
    assert nws > 0
    ws = torch.full((nws // 4,), float('nan'), device=DEV)
    g = Guard(taps * co * ci)
    xd, dyd = dev(x), dev(dy)
    L.check(lib.yond_conv_wgrad_ws_f32(L.ptr(xd), L.ptr(dyd), N, H, W, ci, Ho, Wo, co, mode, stride, g.ptr(), L.ptr(ws) if use_ws else None,
                                       nws if use_ws else 0, L.stream()), "wgrad_ws")
    torch.cuda.synchronize()
    return g.get((taps, co, ci)), nws


def wg32_geometry(mode, stride, N, H, W, ci, co):
    """(chunk, Hk, Wk, nco) from wgrad_chunk of tests/test_hip_train_edges.py."""
    Ho, Wo = out_shape(mode, stride, H, W)
    Hk, Wk = (H, W) if mode == 1 else (Ho, Wo)
    nco = 2 if (co % 64 == 0 and mode != 1) else 1
    return wgrad_chunk(mode, nco, N, Hk, Wk, ci, co), Hk, Wk, nco


@pytest.mark.parametrize("N,H,W", [(3, 7, 33), (1, 2, 5)])
@pytest.mark.parametrize("ci,co", [(32, 32), (64, 64)])
@pytest.mark.parametrize("mode,stride", [(0, 1), (0, 2), (1, 2), (2, 1)])
def test_fp32_wgrad_exact_and_within_the_gamma_bound(mode, stride, ci, co, N, H, W):
    """yond_conv_wgrad_ws_f32, workspace and atomics: bit-equal on integers, within FACTOR T of the gamma bound on the hard operands.  3 x 7 x 33:
    odd W (the last pixel pair of a row is half empty), odd H under stride 2, wave chunks that straddle two images (asserted); 1 x 2 x 5: fewer
    rows than the workgroup has waves.  32 output channels run NCO 1, 64 run NCO 2 (modes 0 and 2)."""
    _, lib = lib_()
    Ho, Wo = out_shape(mode, stride, H, W)
    chunk, Hk, Wk, nco = wg32_geometry(mode, stride, N, H, W, ci, co)
    rows = N * Hk
    if N == 3:
        assert Wk % 2 == 1 and any(r0 // Hk != (min(r0 + chunk, rows) - 1) // Hk for r0 in range(0, rows, chunk)), "no chunk straddles two images"
        assert (mode, stride) != (0, 2) or H % 2 == 1
    else:
        assert rows < 4
    assert nco == (2 if co == 64 and mode != 1 else 1)
    rng = np.random.default_rng([71, mode, stride, ci, N])
    xi = M.dense_int(rng, (N, H, W, ci), 8, N * Hk * Wk, 8)
    di = M.dense_int(rng, (N, Ho, Wo, co), 8, N * Hk * Wk, 8)
    want = M.wgrad_ref(xi, di, mode, stride).astype(np.float32)
    x, _ = M.hard_wgrad(rng, N, H, W, ci, co)
    _, dy = M.hard_wgrad(rng, N, Ho, Wo, ci, co)
    rs = []
    for use_ws in (True, False):
        got, nws = run_wg32(xi, di, mode, stride, use_ws)
        _, wgchunks, _ = M.wg32_geometry(N, Hk, Wk, chunk)
        assert nws == wgchunks * want.size * 4                                 # the chunk geometry the bound counts is the library's
        assert np.array_equal(bits(got), bits(want)), f"ws {use_ws}: {int((got != want).sum())} of {want.size} elements differ"
        ref, T = M.wg32_threshold(x, dy, mode, stride, chunk, use_ws)
        got, _ = run_wg32(x, dy, mode, stride, use_ws)
        rs.append(M.ratio(got, ref, T))
        assert np.all(got[:, 5] == 0) and np.all(got[:, :, 3] == 0)
    parity(f"fp32 wgrad mode {mode} stride {stride} {ci}->{co} {N}x{H}x{W} (chunk {chunk} rows, NCO {nco}): integers bit-equal; hard operands workspace "
           f"{rs[0]:.3f} T, atomics {rs[1]:.3f} T")
    assert max(rs) <= M.FACTOR


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_split
# ---------------------------------------------------------------------------------------------------------------------------
BIG = 1 << 30
rup = lambda c: (c + 31) // 32 * 32


def run_gemm(xs, wflat, srcs, P, n_p, n_real, sn_lo, sn_hi, nblk, bias, out_elems, ldy, shuffle=0, H=0, W=0):
    """srcs: (index into xs, offset into wflat in elements, sk_lo, sk_hi, k, kblk, k_real) per source.  Returns the guarded output (flat) after
    checking both status words are clean."""
    from test_hip_train import _gemm_split
    xd, wd = [dev(x) for x in xs], dev(wflat)
    bd = None if bias is None else dev(bias)
    g = Guard(out_elems)
    desc = [(xd[i].data_ptr(), wd.data_ptr() + 4 * off, sk_lo, sk_hi, xs[i].shape[1], k, kblk, k_real) for i, off, sk_lo, sk_hi, k, kblk, k_real in srcs]
    assert _gemm_split(desc, P, n_p, n_real, sn_lo, sn_hi, nblk, bd, g.view, ldy, shuffle, H, W) == 0
    return g.get()


def gemm_check(name, xs, wflat, srcs, P, n_p, n_real, sn_lo, sn_hi, nblk, bias, exact, shuffle=None):
    Bs = [M.gemm_B(wflat[off:], sk_lo, sk_hi, kblk, k, k_real, sn_lo, sn_hi, nblk, n_p, n_real) for _, off, sk_lo, sk_hi, k, kblk, k_real in srcs]
    bn = None if bias is None else M.gemm_bias(bias, nblk, n_p, n_real)
    ref, T = M.gemm_threshold([xs[i] for i, *_ in srcs], Bs, bn)
    if shuffle:
        N, H, W = shuffle
        ref, T = M.shuffle_store(ref, N, H, W), M.shuffle_store(T, N, H, W)
        got = run_gemm(xs, wflat, srcs, P, n_p, n_real, sn_lo, sn_hi, nblk, bias, ref.size, n_p // 4, 1, H, W).reshape(ref.shape)
    else:
        got = run_gemm(xs, wflat, srcs, P, n_p, n_real, sn_lo, sn_hi, nblk, bias, ref.size, n_p).reshape(ref.shape)
    if exact:
        assert np.array_equal(bits(got), bits(ref.astype(np.float32))), f"{name}: {int((got != ref).sum())} of {ref.size} elements differ"
        return 0.0
    r = M.ratio(got, ref, T)
    assert r <= M.FACTOR, f"{name}: {r:.3f} T"
    return r


def fwd_operands(rng, P, c0, c1, cout, ints):
    """x per source with NONZERO padding columns (the k mask must kill them), w [cout][c0 + c1], bias."""
    cin = c0 + c1
    cs = [c for c in (c0, c1) if c]
    if ints:
        w = M.dense_int(rng, (cout, cin), 31, sum(rup(c) for c in cs), 8)
        xs = [M.dense_int(rng, (P, rup(c)), 8, sum(rup(c) for c in cs), 31) for c in cs]
        b = M.dense_int(rng, (cout,), 100, 1, 1)
    else:
        xa, w = M.hard_gemm(rng, P, cin, cout)
        xs, o = [], 0
        for c in cs:
            q = (rng.standard_normal((P, rup(c))) * 100).astype(np.float32)
            q[:, :c] = xa[:, o:o + c]
            xs.append(q)
            o += c
        b = (10.0 ** rng.uniform(-2, 2, cout)).astype(np.float32)
    return xs, w, b


@pytest.mark.parametrize("P", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("c0,c1,cout", [(32, 32, 32), (40, 24, 8), (96, 0, 40)])
def test_gemm_split_conv1x1_and_data_gradient(P, c0, c1, cout):
    """A 1x1 convolution over one or two sources and the data gradient of its first source (the weight read transposed through the strides), on
    integers (|w| < 32) bit for bit and on the hard operands per element.  P on either side of one and two 128-pixel workgroups and P = 1;
    40 + 24 -> 8: k_real < k in both sources with nonzero values in x's padding columns, n_real smaller than a tile, the zero padding columns
    written; 96 -> 40: the 64-wide tile with 24 padding columns."""
    rng = np.random.default_rng([73, P, cout])
    cin, n_p = c0 + c1, rup(cout)
    cs = [c for c in (c0, c1) if c]
    out = []
    for ints in (True, False):
        xs, w, b = fwd_operands(rng, P, c0, c1, cout, ints)
        srcs, off = [], 0
        for i, c in enumerate(cs):
            srcs.append((i, off, 1, 0, rup(c), BIG, c))
            off += c
        out.append(gemm_check("forward", xs, w.reshape(-1), srcs, P, n_p, cout, cin, 0, BIG, b, ints))
        # data gradient of source 0: dx[p][ci] = sum_co dy[p][co] w[co][ci]; dy's padding columns hold values the k mask must kill
        dy = M.dense_int(rng, (P, n_p), 8, n_p, 31) if ints else np.where(np.arange(n_p)[None, :] < cout, M.hard_gemm(rng, P, n_p, 8)[0],
                                                                          np.float32(100.0) * rng.standard_normal((P, n_p)).astype(np.float32))
        out.append(gemm_check("data gradient", [dy], w.reshape(-1), [(0, 0, cin, 0, n_p, BIG, cout)], P, rup(c0), c0, 1, 0, BIG, None, ints))
    parity(f"gemm_split 1x1 P {P} {c0}+{c1}->{cout}: integers bit-equal (forward, data gradient); hard operands forward {out[2]:.3f} T, data gradient {out[3]:.3f} T")


@pytest.mark.parametrize("N,H,W,cin,cout", [(2, 3, 5, 40, 24), (1, 9, 3, 64, 32), (1, 1, 1, 32, 8)])
def test_gemm_split_transposed_conv_and_data_gradient(N, H, W, cin, cout):
    """ConvTranspose2d 2x2 stride 2: the weights [ci][co][2][2] read in place, the pixel-shuffle store; and its data gradient on the unshuffled
    gradient, a two-level k index (kblk = cop, k_real = cout per block) whose padding columns hold nonzero values."""
    rng = np.random.default_rng([79, N, H, cout])
    P, cip, cop = N * H * W, rup(cin), rup(cout)
    out = []
    for ints in (True, False):
        if ints:
            x, w, b = M.dense_int(rng, (P, cip), 8, cip, 31), M.dense_int(rng, (cin, cout, 2, 2), 31, 4 * cop, 8), M.dense_int(rng, (cout,), 100, 1, 1)
            gu = M.dense_int(rng, (P, 4 * cop), 8, 4 * cop, 31)
        else:
            xa, wa = M.hard_gemm(rng, P, cin, 4 * cout, zero_n=7)
            x = (rng.standard_normal((P, cip)) * 100).astype(np.float32)
            x[:, :cin] = xa
            w = np.ascontiguousarray(wa.reshape(cout, 2, 2, cin).transpose(3, 0, 1, 2))
            b = (10.0 ** rng.uniform(-2, 2, cout)).astype(np.float32)
            gu = (rng.standard_normal((P, 4, cop)) * 100).astype(np.float32)
            gu[:, :, :cout] = M.hard_gemm(rng, P, 4 * cout, 8)[0].reshape(P, 4, cout)
            gu = gu.reshape(P, 4 * cop)
        out.append(gemm_check("transposed forward", [x], w.reshape(-1), [(0, 0, 4 * cout, 0, cip, BIG, cin)], P, 4 * cop, cout, 4, 1, cop, b, ints, shuffle=(N, H, W)))
        out.append(gemm_check("transposed data gradient", [gu], w.reshape(-1), [(0, 0, 4, 1, 4 * cop, cop, cout)], P, cip, cin, 4 * cout, 0, BIG, None, ints))
    parity(f"gemm_split transposed 2x2 {N}x{H}x{W} {cin}->{cout}: integers bit-equal (shuffle store, data gradient); hard operands forward {out[2]:.3f} T, "
           f"data gradient {out[3]:.3f} T")
