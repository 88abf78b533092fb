"""GPU: the kernels at the two ends of every forward (csrc/conv_misc.hip: conv_in and its weight packer, conv_out, maxpool2, the FiLM
launch; csrc/estnet.hip: est_conv_in, est_head; csrc/vst.hip: image_max and the layout copies), through the C ABI, each against its float64
model and derived per-element bound of tests/edge_model.py -- never against another kernel -- or, for the exact operations, bit for bit
against a NumPy statement.  The shapes are the smallest that reach each code path (tile edges, a second channel tile, the capped grids'
stride loops); tests/test_edge_model.py holds the same operand sets on the CPU and shows that each bound bites.

Rules of every case: each output lives inside a NaN-filled allocation with MARGIN elements in front and behind; the margins must stay NaN
bit for bit, everything the entry promises to write must not be NaN, padding it promises not to write must still be NaN.  The [parity]
lines (worst |kernel - model| / bound per kernel and case; at most 1) are what profiles/edge_layers_report.txt records."""
import ctypes

import numpy as np
import pytest
import torch

import edge_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 1024                       # elements: 4 KiB (float32) on both sides
EINVAL, EUNSUPPORTED = -1, -2
FMT_NHWC, FMT_SPLIT_PLANES, FMT_PLANES4 = 0, 1, 2


def lib_():
    from yond_public_amd import _lib as L
    return L, L.load()


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Guard:
    """n elements inside a NaN-filled allocation with margins of MARGIN elements; a pure output, NaN until the kernel writes it."""

    def __init__(self, n, dtype=torch.float32):
        self.n = int(n)
        self.buf = torch.full((MARGIN + self.n + MARGIN,), float('nan'), dtype=dtype, device=DEV)
        self.ref = self.buf.cpu().numpy().copy()
        self.view = self.buf[MARGIN:MARGIN + self.n]

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def get(self, shape=None, allow_nan=False):
        """The interior as numpy, after checking that the margins hold their NaN bit for bit and (unless allow_nan) that nothing inside is NaN."""
        now = self.buf.cpu().numpy()
        raw = np.uint32 if now.dtype == np.float32 else np.uint64
        for sl in (slice(0, MARGIN), slice(MARGIN + self.n, None)):
            assert np.array_equal(now[sl].view(raw), self.ref[sl].view(raw)), "a margin was written"
        out = now[MARGIN:MARGIN + self.n]
        assert allow_nan or not np.isnan(out).any(), "the interior was not fully overwritten"
        return out if shape is None else out.reshape(shape)


def parity(name, r):
    print(f"[parity] {name}: worst |kernel - model| / bound = {r:.3f}")
    return r


def launch(rc, what):
    L, _ = lib_()
    L.check(rc, what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# conv_in
# ---------------------------------------------------------------------------------------------------------------------------
def test_conv_in_weight_packer_layout():
    """yond_pack_conv_in_weight_f32 (host): [Cout/32][5 tap pairs][2][32][4] with zeros in the tap-9 slots, inside NaN margins."""
    _, lib = lib_()
    for cout in (32, 96):
        w = M.conv_in_operands(1, 17, 65, 96)[2][:cout].copy()
        dst = np.full(MARGIN + cout * 40 + MARGIN, np.nan, np.float32)
        assert lib.yond_pack_conv_in_weight_f32(w.ctypes.data_as(ctypes.c_void_p), cout, ctypes.c_void_p(dst.ctypes.data + 4 * MARGIN)) == 0
        assert np.isnan(dst[:MARGIN]).all() and np.isnan(dst[-MARGIN:]).all()
        got = dst[MARGIN:-MARGIN]
        assert np.array_equal(bits(got), bits(M.conv_in_pack(w)))
        assert np.all(bits(got.reshape(cout // 32, 5, 2, 32, 4)[:, 4, 1]) == 0)           # tap 9: +0.0
    q = np.zeros(48 * 40, np.float32)
    assert lib.yond_pack_conv_in_weight_f32(q.ctypes.data_as(ctypes.c_void_p), 48, q.ctypes.data_as(ctypes.c_void_p)) == EINVAL


@pytest.mark.parametrize("shape", M.CONV_IN_SHAPES)
def test_conv_in_vs_model(shape):
    """yond_conv_in_f32 at one pixel, one full tile (8 x 32 x 32), tiles cut on both sides with a second channel tile, three images, and
    three channel tiles; ub and bias present and NULL; slope 0.01, 0.2, 0; NHWC within the bound and PLANES4 bit-equal to it."""
    L, lib = lib_()
    N, H, W, Cout = shape
    ops = M.conv_in_operands(*shape)
    wpk = np.empty(Cout * 40, np.float32)
    assert lib.yond_pack_conv_in_weight_f32(ops[2].ctypes.data_as(ctypes.c_void_p), Cout, wpk.ctypes.data_as(ctypes.c_void_p)) == 0
    xd, wd = dev(ops[0]), dev(wpk)
    for has_ub, has_bias, slope in M.CONV_IN_VARIANTS:
        x, ub, w, bias = M.pick(ops, (True, has_ub, True, has_bias))
        ubd, bd = dev(ub), dev(bias)
        outs = {}
        for fmt in (FMT_NHWC, FMT_PLANES4):
            g = Guard(N * H * W * Cout)
            launch(lib.yond_conv_in_f32(L.ptr(xd), L.ptr(ubd), N, H, W, Cout, L.ptr(wd), L.ptr(bd), slope, g.ptr(), fmt, L.stream()), "conv_in")
            outs[fmt] = g.get()
        got = outs[FMT_NHWC].reshape(N, H, W, Cout)
        tag = f"conv_in {shape} ub {has_ub} bias {has_bias} slope {slope}"
        assert np.array_equal(bits(M.planes4_to_nhwc(outs[FMT_PLANES4], N, H, W, Cout)), bits(got)), tag + ": PLANES4 differs from NHWC"
        assert parity(tag, M.ratio(got, *M.conv_in_model(x, ub, w, bias, slope))) <= 1.0, tag


def test_conv_in_refusals():
    L, lib = lib_()
    q = torch.zeros(64 * 40, device=DEV)
    call = lambda N, Cout, fmt: lib.yond_conv_in_f32(L.ptr(q), None, N, 2, 2, Cout, L.ptr(q), None, 0.01, L.ptr(q), fmt, L.stream())
    assert call(1, 48, FMT_NHWC) == EUNSUPPORTED
    assert call(0, 32, FMT_NHWC) == EINVAL
    assert call(1, 32, FMT_SPLIT_PLANES) == EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# conv_out
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", M.conv_out_cases())
def test_conv_out_vs_model(shape, variant):
    """yond_conv_out_f32 at Cin = 32 .. 256 on a few pixels (one workgroup and less), every combination of x and ub, bias NULL once, and
    once above the grid's cap (262,644 pixels: the workgroups walk a second pass of 500 pixels)."""
    L, lib = lib_()
    N, H, W, Cin = shape
    has_x, has_ub, has_bias = variant
    feat, w, bias, x, ub = M.pick(M.conv_out_operands(*shape), (True, True, has_bias, has_x, has_ub))
    fd, wd, bd, xd, ubd = (dev(a) for a in (feat, w, bias, x, ub))
    g = Guard(N * H * W * 4)
    launch(lib.yond_conv_out_f32(L.ptr(fd), Cin, L.ptr(wd), L.ptr(bd), L.ptr(xd), L.ptr(ubd), N, H, W, g.ptr(), L.stream()), "conv_out")
    tag = f"conv_out {shape} x {has_x} ub {has_ub} bias {has_bias}"
    assert parity(tag, M.ratio(g.get((N, H, W, 4)), *M.conv_out_model(feat, w, bias, x, ub))) <= 1.0, tag


def test_conv_out_refusals():
    L, lib = lib_()
    q = torch.zeros(256, device=DEV)
    assert lib.yond_conv_out_f32(L.ptr(q), 48, L.ptr(q), None, None, None, 1, 1, 1, L.ptr(q), L.stream()) == EUNSUPPORTED
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# maxpool2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.MAXPOOL_SHAPES)
def test_maxpool2_bit_exact(shape):
    L, lib = lib_()
    N, H, W, C = shape
    for kind in ('mixed', 'negative', 'neginf'):
        x = M.maxpool_operands(shape, kind)
        xd = dev(x)
        g = Guard(N * (H // 2) * (W // 2) * C)
        launch(lib.yond_maxpool2_f32(L.ptr(xd), N, H, W, C, g.ptr(), L.stream()), "maxpool2")
        assert np.array_equal(bits(g.get((N, H // 2, W // 2, C))), bits(M.maxpool2_model(x))), (shape, kind)


def test_maxpool2_refusals():
    L, lib = lib_()
    q = torch.zeros(1024, device=DEV)
    for H, W, C in ((3, 4, 4), (4, 3, 4), (4, 4, 6)):
        assert lib.yond_maxpool2_f32(L.ptr(q), 1, H, W, C, L.ptr(q), L.stream()) == EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# film
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_ub", [True, False])
@pytest.mark.parametrize("N", M.FILM_N)
def test_film_vs_model(N, has_ub):
    """yond_film_f32, one launch of eight descriptors (both kinds x C = 8, 40, 264, 1024; ld = C rounded up to 32): below 8 images the grid
    has all 32 row tiles, from 8 on 8 tiles and a stride loop.  The padding [C:ld] of all four outputs stays NaN."""
    L, lib = lib_()
    t, ub = M.film_t(N)
    ub = ub if has_ub else None
    descs = M.film_descs()
    arr = (L.YondFilmDesc * len(descs))()
    keep, outs = [], []
    for d, a in zip(descs, arr):
        assert d['C'] <= 1024
        a.kind, a.C, a.ld = d['kind'], d['C'], d['ld']
        for k in ('w_a0', 'b_a0', 'w_a2', 'b_a2', 'w_b0', 'b_b0', 'w_b', 'b_b', 'cb1', 'cb2'):
            tns = dev(d[k])
            keep.append(tns)
            setattr(a, k, None if tns is None else tns.data_ptr())
        g = {k: Guard(N * d['ld']) for k in M.FILM_OUT}
        a.s1, a.t1, a.s2, a.t2 = (g[k].view.data_ptr() for k in M.FILM_OUT)
        outs.append(g)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    td, ubd = dev(t), dev(ub)
    launch(lib.yond_film_f32(L.ptr(raw), len(descs), L.ptr(td), L.ptr(ubd), N, L.stream()), "film")
    for d, g in zip(descs, outs):
        C, ld = d['C'], d['ld']
        got = {k: g[k].get((N, ld), allow_nan=True) for k in M.FILM_OUT}
        tag = f"film kind {d['kind']} C {C} N {N} ub {has_ub}"
        for k in M.FILM_OUT:
            assert not np.isnan(got[k][:, :C]).any(), f"{tag}: {k} not fully written"
            assert np.isnan(got[k][:, C:]).all(), f"{tag}: the padding of {k} was written"
        assert parity(tag, M.film_check(got, M.film_model(d, t, ub), C)) <= 1.0, tag


# ---------------------------------------------------------------------------------------------------------------------------
# image_max
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", M.IMAGE_MAX_N)
@pytest.mark.parametrize("elems", M.IMAGE_MAX_ELEMS)
def test_image_max_bit_exact(elems, N):
    """yond_image_max_f32 with one workgroup per image, two, and 256 with a strided 17th pass; all-negative data with the maximum at the
    first element, the last, in the strided tail; -inf entries; and NaN, which the entry DROPS (include/yond_hip.h): the maximum of the
    other elements, -inf for an image that is all NaN."""
    L, lib = lib_()
    for kind in M.IMAGE_MAX_KINDS:
        x = M.image_max_operands(N, elems, kind)
        xd = dev(x)
        part, out = Guard(N * 256), Guard(N)
        launch(lib.yond_image_max_f32(L.ptr(xd), N, elems, part.ptr(), out.ptr(), L.stream()), "image_max")
        part.get(allow_nan=True)
        want = M.image_max_model(x)
        assert not np.isnan(want).any()
        assert np.array_equal(bits(out.get()), bits(want)), (elems, N, kind)


# ---------------------------------------------------------------------------------------------------------------------------
# the layout copies
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.BAYER_SHAPES)
def test_bayer_rggb_bit_exact_and_round_trip(shape):
    L, lib = lib_()
    H, W = shape
    b = M.exact_operands(shape, 3)
    b[0, 0], b[-1, -1] = -0.0, 0.0
    bd = dev(b)
    g = Guard(H * W)
    launch(lib.yond_bayer2rggb_f32(L.ptr(bd), H, W, g.ptr(), L.stream()), "bayer2rggb")
    assert np.array_equal(bits(g.get((H // 2, W // 2, 4))), bits(M.bayer2rggb_model(b)))
    g2 = Guard(H * W)
    launch(lib.yond_rggb2bayer_f32(g.ptr(), H // 2, W // 2, g2.ptr(), L.stream()), "rggb2bayer")
    assert np.array_equal(bits(g2.get((H, W))), bits(M.rggb2bayer_model(M.bayer2rggb_model(b))))
    assert torch.equal(g2.view.view(torch.int32), bd.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("shape", M.NCHW4_SHAPES)
def test_nchw4_nhwc4_bit_exact_and_round_trip(shape):
    L, lib = lib_()
    N, H, W = shape
    x = M.exact_operands((N, 4, H, W), 4)
    x.reshape(-1)[0] = -0.0
    xd = dev(x)
    g = Guard(x.size)
    launch(lib.yond_nchw4_to_nhwc4_f32(L.ptr(xd), g.ptr(), N, H, W, L.stream()), "nchw4_to_nhwc4")
    assert np.array_equal(bits(g.get((N, H, W, 4))), bits(M.nchw4_to_nhwc4_model(x)))
    g2 = Guard(x.size)
    launch(lib.yond_nhwc4_to_nchw4_f32(g.ptr(), g2.ptr(), N, H, W, L.stream()), "nhwc4_to_nchw4")
    assert np.array_equal(bits(g2.get((N, 4, H, W))), bits(M.nhwc4_to_nchw4_model(M.nchw4_to_nhwc4_model(x))))
    assert torch.equal(g2.view.view(torch.int32), xd.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("shape", sorted({s for s, _ in M.ROT90_CASES}))
def test_rot90_bit_exact_and_round_trip(shape):
    L, lib = lib_()
    N, H, W = shape
    x = M.exact_operands(shape, 5)
    x.reshape(-1)[0] = -0.0
    xd = dev(x)
    for k in [k for s, k in M.ROT90_CASES if s == shape]:
        g = Guard(x.size)
        launch(lib.yond_rot90_f32(L.ptr(xd), N, H, W, k, g.ptr(), L.stream()), "rot90")
        want = M.rot90_model(x, k)
        assert np.array_equal(bits(g.get(want.shape)), bits(want)), (shape, k)
        g2 = Guard(x.size)
        launch(lib.yond_rot90_f32(g.ptr(), N, want.shape[1], want.shape[2], -k, g2.ptr(), L.stream()), "rot90 back")
        g2.get()
        assert torch.equal(g2.view.view(torch.int32), xd.reshape(-1).view(torch.int32)), (shape, k)


# ---------------------------------------------------------------------------------------------------------------------------
# est_conv_in, est_head
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.EST_CONV_IN_SHAPES)
def test_est_conv_in_vs_model(shape):
    """yond_est_conv_in_f32 (tile 8 x 64) at one pixel, tiles cut on both sides, Cout = 96 (16 threads of a workgroup without a pixel) and
    Cout = 1024 (one pixel per workgroup pass)."""
    L, lib = lib_()
    N, H, W, Cout = shape
    x, w, bias = M.est_conv_in_operands(*shape)
    xd, wd, bd = dev(x), dev(w), dev(bias)
    g = Guard(N * H * W * Cout)
    launch(lib.yond_est_conv_in_f32(L.ptr(xd), N, H, W, Cout, L.ptr(wd), L.ptr(bd), g.ptr(), L.stream()), "est_conv_in")
    assert parity(f"est_conv_in {shape}", M.ratio(g.get((N, H, W, Cout)), *M.est_conv_in_model(x, w, bias))) <= 1.0


@pytest.mark.parametrize("case", M.EST_HEAD_CASES)
def test_est_head_vs_model(case):
    """yond_est_head_f32: the map [N][out_nc][H][W] and the mean [N][out_nc], Cin from one 16-byte group to four per lane, HW from one pixel
    to 8193 (the workgroups stride).  The mean is bit-identical over three calls."""
    L, lib = lib_()
    H, W, Cin, nc, sq = case
    N = M.EST_HEAD_N
    feat, w, bias = M.est_head_operands(N, H, W, Cin, nc)
    fd, wd, bd = dev(feat), dev(w), dev(bias)
    g = Guard(N * nc * H * W)
    launch(lib.yond_est_head_f32(L.ptr(fd), N, H, W, Cin, L.ptr(wd), L.ptr(bd), nc, sq, 0, g.ptr(), None, L.stream()), "est_head map")
    assert parity(f"est_head {case} map", M.ratio(g.get((N, nc, H, W)), *M.est_head_model(feat, w, bias, sq, 0))) <= 1.0
    ws = lib.yond_est_head_ws_bytes(N, nc)
    assert ws == N * M.EST_HEAD_BLOCKS * nc * 8
    means = []
    for _ in range(3):
        part, out = Guard(ws // 8, dtype=torch.float64), Guard(N * nc)
        launch(lib.yond_est_head_f32(L.ptr(fd), N, H, W, Cin, L.ptr(wd), L.ptr(bd), nc, sq, 1, out.ptr(), part.ptr(), L.stream()), "est_head mean")
        part.get(allow_nan=True)
        means.append(out.get((N, nc)))
    assert np.array_equal(bits(means[0]), bits(means[1])) and np.array_equal(bits(means[0]), bits(means[2]))
    assert parity(f"est_head {case} mean", M.ratio(means[0], *M.est_head_model(feat, w, bias, sq, 1))) <= 1.0


def test_est_refusals():
    """Cout and Cin the kernels do not cover, out_nc = 5, the mean without its workspace, and the one size whose LDS (64 KiB of weights
    beside 512 static bytes) cannot launch: YOND_EUNSUPPORTED from the guard, not a runtime error code.  Nothing is launched."""
    L, lib = lib_()
    q = torch.zeros(4096 * 4, device=DEV)
    o = Guard(64)
    conv = lambda Cout: lib.yond_est_conv_in_f32(L.ptr(q), 1, 1, 1, Cout, L.ptr(q), L.ptr(q), o.ptr(), L.stream())
    assert conv(48) == EUNSUPPORTED and conv(1056) == EUNSUPPORTED
    head = lambda Cin, nc, pge, part: lib.yond_est_head_f32(L.ptr(q), 1, 1, 1, Cin, L.ptr(q), L.ptr(q), nc, 0, pge, o.ptr(), part, L.stream())
    assert head(32, 5, 0, None) == EUNSUPPORTED
    assert head(6, 1, 0, None) == EUNSUPPORTED
    assert head(32, 1, 1, None) == EINVAL
    assert head(4096, 4, 0, None) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert np.isnan(o.get(allow_nan=True)).all()
