"""GPU: K1 (yond_pack_vst_norm*), K4 (yond_denorm_ivst_unpack*) and N1 (yond_block_metrics_f32) at their edges, against the plain float64
references of tests/vst_model.py.

K1 / K4: EVERY element within ulp32 / 2 + band of the staged float64 evaluation (vst_model.ulp_check: the header's promise), for all six K1
and all four K4 entry points, each held to the reference and not to another entry point.  N1: per block the sum of squared error and the
summed SSIM map, at the tolerances of test_block_metrics_vs_oracle (1e-9 on the mean SSIM, 1e-6 dB on PSNR).  Every output tensor is the
front part of a NaN-filled allocation whose tail must still be NaN afterwards.  The [accuracy] lines are what profiles/vst_edges_report.txt
records."""
import os
import warnings

import numpy as np
import pytest
import torch

import vst_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAIL = 1024
SCALE = M.SCALE
K1_CASES = M.k1_cases()
K4_CASES = M.k4_cases()


def canary(n, dtype=torch.float32):
    """An allocation of n + TAIL elements, all NaN: the kernel writes the first n, the tail must stay NaN."""
    return torch.full((n + TAIL,), float('nan'), dtype=dtype, device=DEV)


def tail_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all().item())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def acc(line):
    print(f"[accuracy] {line}")


# ---------------------------------------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------------------------------------
def device_lut(bc, K, s, mx):
    """The LUT a case hands to the kernels: (x_dev float64, y_dev, two_d).  get_bias' ordinates are built on the device; a pair the LDS
    kernel does not cover (YOND_EUNSUPPORTED) takes them from the oracle.  The model later reads back what the kernel was given."""
    import yond_oracle as O
    from yond_public_amd import _lib as L, pipeline as P
    if bc is False:
        return None
    if bc == '2d':
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "biaslut.npz"))
        row = P.BiasLUT(table=g["table"], x_lut=g["x_lut"], sg_lut=g["sg_lut"]).row(np.float64(K), np.float64(s), DEV)
        assert row is not None
        return row.x, row.y, True
    ub = np.ceil(np.float32(mx)) + 1                              # float32: the last run's knots are float32 values (NumPy 2)
    lams, x_dev = P._knots_on_device(ub, DEV)
    assert np.array_equal(np.asarray(lams, np.float64), np.asarray(M.bias_knots(ub), np.float64))
    if bc == 'synthetic':
        return x_dev, dev(M.synthetic_ordinates(np.asarray(lams, np.float64))), False
    y_dev = torch.empty(len(lams), dtype=torch.float32, device=DEV)
    rc = L.load().yond_bias_lut_f64(L.ptr(x_dev), len(lams), float(K), float(s), L.ptr(y_dev), L.stream())
    if rc == -2:
        lams_o, bias = O.get_bias_table(np.float32(mx), np.float64(s), np.float64(K))
        assert np.array_equal(np.asarray(lams_o, np.float64), np.asarray(lams, np.float64))
        y_dev = dev(np.asarray(bias, np.float32))
    else:
        L.check(rc, "yond_bias_lut_f64")
    return x_dev, y_dev, False


def prm_block(K, s, lo, hi, n):
    from yond_public_amd import pipeline as P
    prm = np.zeros(16, np.float64)
    prm[P.PRM['gain']], prm[P.PRM['sigma']], prm[P.PRM['lo']], prm[P.PRM['hi']] = K, s, lo, hi
    prm[P.PRM['flags']], prm[P.PRM['lut_n']] = 0.0, float(n)
    return dev(prm)


def lut_table(lut):
    """yond_lut_table_f64 on the case's knots (n given, no parameter block): the prepared table the _dev / _chain forms read."""
    from yond_public_amd import _lib as L, pipeline as P
    lib = L.load()
    ws = torch.zeros(int(lib.yond_lut_ws_bytes(P.LUT_CAP)), dtype=torch.uint8, device=DEV)
    x_dev, y_dev, two_d = lut
    assert not two_d and len(x_dev) <= P.LUT_CAP
    L.check(lib.yond_lut_table_f64(L.ptr(x_dev), L.ptr(y_dev), len(x_dev), None, L.ptr(ws), L.stream()), "yond_lut_table_f64")
    return ws


def k1_entries(lut, mode=1):
    if mode == 0:
        return ('general',)
    if lut is None:
        return ('general', 'batch', 'dev', 'batch_dev')
    if lut[2]:
        return ('biaslut', 'batch')
    return ('general', 'batch', 'dev', 'batch_dev', 'chain')


def run_k1(entry, frames, pads, K, s, lo, hi, lut, mode=1):
    """One K1 entry point on frames [B][H][W] (B = 1 for the per-frame forms).  Returns (out [B][Hp][Wp][4], img_max [B]) as numpy; asserts
    that nothing beyond the outputs was written.  img_max is pre-filled with garbage: the call zeroes it itself."""
    from yond_public_amd import _lib as L, pipeline as P
    lib = L.load()
    B, H, W = frames.shape
    pl, pr, pt, pb = pads
    Hp, Wp = H // 2 + pt + pb, W // 2 + pl + pr
    n_out = B * Hp * Wp * 4
    x = dev(frames)
    out, mx = canary(n_out), canary(B)
    mx[:B] = 7.0
    st = L.stream()
    lx, ly, n = (L.ptr(lut[0]), L.ptr(lut[1]), len(lut[0])) if lut is not None else (None, None, 0)
    prm = None
    if entry in ('general', 'biaslut', 'chain', 'dev'):
        assert B == 1
    if entry == 'general':
        rc = lib.yond_pack_vst_norm_f32(L.ptr(x), H, W, L.ptr(out), pl, pr, pt, pb, mode, SCALE, float(K), float(s), float(lo), float(hi), lx, ly, n,
                                        L.ptr(mx), st)
    elif entry == 'biaslut':
        rc = lib.yond_pack_vst_norm_biaslut_f32(L.ptr(x), H, W, L.ptr(out), pl, pr, pt, pb, SCALE, float(K), float(s), float(lo), float(hi), lx, ly, n,
                                                L.ptr(mx), st)
    elif entry == 'batch':
        rc = lib.yond_pack_vst_norm_batch_f32(L.ptr(x), B, H, W, L.ptr(out), pl, pr, pt, pb, SCALE, float(K), float(s), float(lo), float(hi), lx, ly, n,
                                              1 if (lut is not None and lut[2]) else 0, L.ptr(mx), st)
    else:
        prm = prm_block(K, s, lo, hi, n)
        ws = lut_table(lut) if lut is not None else None
        cap = P.LUT_CAP if lut is not None else 0
        if entry == 'dev':
            rc = lib.yond_pack_vst_norm_dev_f32(L.ptr(x), H, W, L.ptr(out), pl, pr, pt, pb, SCALE, L.ptr(prm), L.ptr(ws), cap, L.ptr(mx), st)
        elif entry == 'batch_dev':
            rc = lib.yond_pack_vst_norm_batch_dev_f32(L.ptr(x), B, H, W, L.ptr(out), pl, pr, pt, pb, SCALE, L.ptr(prm), L.ptr(ws), cap, L.ptr(mx), st)
        else:
            rc = lib.yond_pack_vst_norm_chain_f32(L.ptr(x), H, W, L.ptr(out), pl, pr, pt, pb, SCALE, L.ptr(prm), L.ptr(ws), cap, L.ptr(mx), st)
    L.check(rc, f"K1 {entry}")
    torch.cuda.synchronize()
    assert tail_intact(out, n_out) and tail_intact(mx, B), f"K1 {entry}: wrote beyond its outputs"
    if prm is not None:
        assert int(prm.cpu().numpy()[P.PRM['flags']]) == 0, entry
    return out[:n_out].cpu().numpy().reshape(B, Hp, Wp, 4), mx[:B].cpu().numpy()


def k1_case_setup(case):
    name, H, W, pads, K, s, bc, top, seed = case
    mx = M.frame_max_dn(M.k1_frame_base(H, W, K, s, top, seed))
    lut = device_lut(bc, K, s, mx)
    lx = None if lut is None else lut[0].cpu().numpy()
    ly = None if lut is None else lut[1].cpu().numpy()
    f = M.k1_frame(H, W, K, s, top, seed, None if (lut is None or lut[2]) else lx)
    lo, hi = M.lo_hi(K, s)
    return f, lut, lx, ly, lo, hi


@pytest.mark.parametrize("ci", range(len(K1_CASES)), ids=[c[0].replace(' ', '_') for c in K1_CASES])
def test_k1_every_entry_point_within_half_ulp_plus_band(ci):
    """Per case: the general entry point (the 2-D LUT's own for a '2d' case) first, then every other form that takes the case's LUT, each
    against k1_ref; img_max equals the output's maximum exactly."""
    case = K1_CASES[ci]
    name, H, W, pads, K, s, bc, top, seed = case
    f, lut, lx, ly, lo, hi = k1_case_setup(case)
    u, band = M.k1_ref(f, pads, 1, SCALE, K, s, lo, hi, lx, ly, bool(lut and lut[2]))
    wc = M.well_conditioned(lo, hi)
    worst, farther = 0.0, []
    fails = []
    for entry in k1_entries(lut):
        got, mx = run_k1(entry, f[None], pads, K, s, lo, hi, lut)
        ratio, share, far = M.ulp_stats(got[0], u, band)
        worst = max(worst, ratio)
        farther.append(f"{entry} {far}")
        assert float(mx[0]) == float(got.max()), (entry, mx, got.max())
        try:
            M.ulp_check(got[0], u, band, f"K1 {entry} {name}")
        except AssertionError as e:
            fails.append(str(e))
    acc(f"K1 {name}: {u.size} elements, worst |got - v64| / (ulp/2 + band) = {worst:.4f}, two-answer share {share:.2e} "
        f"({'well' if wc else 'ill'}-conditioned), farther neighbour taken: {', '.join(farther)}")
    assert not fails, "\n".join(fails)
    if wc:
        assert share <= M.SHARE_MAX


@pytest.mark.parametrize("gi", (1, 2, 4, 10))
def test_k1_mode_0_is_pack_pad_clamp(gi):
    gname, H, W, pads = M.K1_GEOMS[gi]
    f = M.k1_frame_base(H, W, 4.37, 6.27, 1.0, 77 + gi)
    f = (f * np.float32(1.4) - np.float32(0.2)).astype(np.float32)                   # below 0 and above 1
    f.reshape(-1)[:4] = (0.0, 1.0, 1e-45, -0.0)
    u, band = M.k1_ref(f, pads, 0, SCALE, 1.0, 0.0, 0.0, 1.0)
    got, mx = run_k1('general', f[None], pads, 1.0, 0.0, 0.0, 1.0, None, mode=0)
    acc(f"K1 mode 0 {gname}: {int((got[0] != u).sum())} of {u.size} elements differ")
    assert np.array_equal(got[0].astype(np.float64), u) and float(mx[0]) == float(got.max()) == 1.0


@pytest.mark.parametrize("bi", range(len(M.K1_BATCH)))
@pytest.mark.parametrize("bc", (True, False))
def test_k1_batch_rows_cross_frames_inside_a_workgroup(bi, bc):
    """B * Hp > 1536 rows with Hp not a multiple of the rows per workgroup: a workgroup's row range crosses from one frame to the next and
    flushes the frame maximum in the middle of its loop.  Every frame has its maximum at a different place and of a different size;
    img_max[b] must be frame b's."""
    B, H, W, pads = M.K1_BATCH[bi]
    K, s = 4.37, 6.27
    lo, hi = M.lo_hi(K, s)
    tops = [0.15 + 0.85 * ((b * 0.6180339887) % 1.0) for b in range(B)]
    frames = np.stack([M.k1_frame_base(H, W, K, s, tops[b], 500 + b) for b in range(B)])
    for b in range(B):                                            # the frame's maximum (k1_frame_base puts it last) to a place of its own
        fl = frames[b].reshape(-1)
        j = (b * 131 + 17) % fl.size
        fl[j], fl[-1] = fl[-1], fl[j]
    lut = device_lut(bc, K, s, M.frame_max_dn(frames))
    lx, ly = (lut[0].cpu().numpy(), lut[1].cpu().numpy()) if lut else (None, None)
    refs = [M.k1_ref(frames[b], pads, 1, SCALE, K, s, lo, hi, lx, ly) for b in range(B)]
    u, band = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    Hp = H // 2 + pads[2] + pads[3]
    rows = B * Hp
    per = -(-rows // 1536)
    cross = M.batch_crossings(B, Hp)
    assert rows > 1536 and (cross > 0 or bi == 0)
    assert len({round(float(u[b].max()), 6) for b in range(B)}) > B // 2
    for entry in ('batch', 'batch_dev'):
        got, mx = run_k1(entry, frames, pads, K, s, lo, hi, lut)
        ratio, share, far = M.ulp_stats(got, u, band)
        acc(f"K1 {entry} B={B} Hp={Hp} ({per} rows per workgroup, {cross} frames start inside one) bias={int(bc)}: worst ratio {ratio:.4f}, two-answer share {share:.2e}, farther {far}")
        M.ulp_check(got, u, band, f"K1 {entry} B={B}")
        assert share <= M.SHARE_MAX
        assert np.array_equal(mx, got.reshape(B, -1).max(axis=1)), entry


def test_k1_chain_refuses_a_table_of_another_shape():
    """The chain form takes get_bias' knot grid (<= 3 evenly spaced runs).  A table of another shape -- a log grid, which the table builder
    leaves to the bisection -- must set YOND_PRM_FLAG_LUT_CAPACITY and write nothing."""
    from yond_public_amd import _lib as L, pipeline as P
    lib = L.load()
    H, W, pads = 16, 24, (1, 1, 1, 1)
    K, s = 4.37, 6.27
    lo, hi = M.lo_hi(K, s)
    lx = np.concatenate(([0.0], 1.0 * 1.006 ** np.arange(1199)))
    lut = (dev(lx), dev(M.synthetic_ordinates(lx)), False)
    ws = lut_table(lut)
    prm = prm_block(K, s, lo, hi, len(lx))
    f = M.k1_frame_base(H, W, K, s, 1.0, 9)
    Hp, Wp = H // 2 + 2, W // 2 + 2
    out, mx = canary(Hp * Wp * 4), canary(1)
    L.check(lib.yond_pack_vst_norm_chain_f32(L.ptr(dev(f)), H, W, L.ptr(out), *pads, SCALE, L.ptr(prm), L.ptr(ws), P.LUT_CAP, L.ptr(mx), L.stream()), "chain")
    torch.cuda.synchronize()
    assert int(prm.cpu().numpy()[P.PRM['flags']]) & P.PRM_LUT_CAPACITY
    assert bool(torch.isnan(out).all().item())
    # the general form evaluates the same table by bisection, within the bound
    u, band = M.k1_ref(f, pads, 1, SCALE, K, s, lo, hi, lx, lut[1].cpu().numpy())
    got, _ = run_k1('general', f[None], pads, K, s, lo, hi, lut)
    M.ulp_check(got[0], u, band, "K1 general on a log grid")


def test_k1_nan_and_inf_pixels():
    """include/yond_hip.h: a NaN pixel gives 0 through every entry point (fmaxf returns its other operand; torch.clamp would keep the NaN),
    -inf gives 0, +inf gives 1 without a LUT; the pixels around them and img_max are what they are without them."""
    name, H, W, pads, K, s, bc, top, seed = [c for c in K1_CASES if c[0] == "main K=4.37 s=6.27 bc=1 top=1.0"][0]
    for use_lut in (True, False):
        case = (name, H, W, pads, K, s, use_lut, top, seed)
        f, lut, lx, ly, lo, hi = k1_case_setup(case)
        f = f.copy()
        twin = f.copy()
        fl, tl = f.reshape(-1), twin.reshape(-1)
        fl[[5, 300, 301, 2 * W + 9]] = np.nan
        fl[[700, 9000]] = -np.inf
        tl[[5, 300, 301, 2 * W + 9, 700, 9000]] = -1.0             # firmly below the clamp: exactly 0
        if not use_lut:
            fl[[1200, 4001]] = np.inf
            tl[[1200, 4001]] = 1e6                                  # firmly above: exactly 1
        u, band = M.k1_ref(twin, pads, 1, SCALE, K, s, lo, hi, lx, ly)
        for entry in k1_entries(lut):
            got, mx = run_k1(entry, f[None], pads, K, s, lo, hi, lut)
            assert np.isfinite(got).all() and np.isfinite(mx).all(), entry
            M.ulp_check(got[0], u, band, f"K1 {entry} with NaN / Inf pixels")
            assert float(mx[0]) == float(got.max())
    g = np.array([[np.nan, np.inf], [-np.inf, 0.25]], np.float32)
    got, mx = run_k1('general', g[None], (0, 0, 0, 0), 1.0, 0.0, 0.0, 1.0, None, mode=0)
    assert got.reshape(-1).tolist() == [0.0, 1.0, 0.0, 0.25] and float(mx[0]) == 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# K4
# ---------------------------------------------------------------------------------------------------------------------------
def k4_entries(mode):
    return ('plain', 'batch') if mode == 0 else ('plain', 'batch', 'dev', 'batch_dev')


def run_k4(entry, y, pt, pl, h, w, mode, K, s, lo, hi, clip):
    """One K4 entry point on y [B][Hp][Wp][4]; returns [B][2h][2w]."""
    from yond_public_amd import _lib as L
    lib = L.load()
    B, Hp, Wp, _ = y.shape
    n_out = B * 4 * h * w
    yd = dev(y)
    out = canary(n_out)
    st = L.stream()
    if entry in ('plain', 'dev'):
        assert B == 1
    if entry == 'plain':
        rc = lib.yond_denorm_ivst_unpack_f32(L.ptr(yd), Hp, Wp, pt, pl, h, w, L.ptr(out), mode, SCALE, float(K), float(s), float(lo), float(hi), clip, st)
    elif entry == 'batch':
        rc = lib.yond_denorm_ivst_unpack_batch_f32(L.ptr(yd), B, Hp, Wp, pt, pl, h, w, L.ptr(out), mode, SCALE, float(K), float(s), float(lo), float(hi),
                                                   clip, st)
    else:
        prm = prm_block(K, s, lo, hi, 0)
        if entry == 'dev':
            rc = lib.yond_denorm_ivst_unpack_dev_f32(L.ptr(yd), Hp, Wp, pt, pl, h, w, L.ptr(out), mode, SCALE, L.ptr(prm), clip, st)
        else:
            rc = lib.yond_denorm_ivst_unpack_batch_dev_f32(L.ptr(yd), B, Hp, Wp, pt, pl, h, w, L.ptr(out), mode, SCALE, L.ptr(prm), clip, st)
    L.check(rc, f"K4 {entry}")
    torch.cuda.synchronize()
    assert tail_intact(out, n_out), f"K4 {entry}: wrote beyond its output"
    return out[:n_out].cpu().numpy().reshape(B, 2 * h, 2 * w)


@pytest.mark.parametrize("ci", range(len(K4_CASES)), ids=[c[0].replace(' ', '_') for c in K4_CASES])
def test_k4_every_entry_point_within_half_ulp_plus_band(ci):
    case = K4_CASES[ci]
    name, (gname, Hp, Wp, pt, pl, h, w), mode, clip, K, s, lo, hi, zmin, seed = case
    y = M.k4_case_input(case)
    r, band = M.k4_ref(y, pt, pl, h, w, mode, SCALE, K, s, lo, hi, clip)
    wc = mode == 0 or M.well_conditioned(lo, hi)
    worst, farther, fails = 0.0, [], []
    for entry in k4_entries(mode):
        got = run_k4(entry, y[None], pt, pl, h, w, mode, K, s, lo, hi, clip)[0]
        ratio, share, far = M.ulp_stats(got, r, band)
        worst = max(worst, ratio)
        farther.append(f"{entry} {far}")
        try:
            M.ulp_check(got, r, band, f"K4 {entry} {name}")
        except AssertionError as e:
            fails.append(str(e))
    acc(f"K4 {name} ({gname}): {r.size} elements, worst |got - v64| / (ulp/2 + band) = {worst:.4f}, two-answer share {share:.2e} "
        f"({'well' if wc else 'ill'}-conditioned), farther neighbour taken: {', '.join(farther)}")
    assert not fails, "\n".join(fails)
    if wc:
        assert share <= M.SHARE_MAX


@pytest.mark.parametrize("mode,clip", ((1, 1), (2, 0), (0, 0)))
def test_k4_batch_grid_stride(mode, clip):
    """B * h > 4096 rows: more rows than workgroups, the grid-stride path of the batched forms."""
    B, Hp, Wp, pt, pl, h, w = M.K4_BATCH
    K, s = 4.37, 6.27
    lo, hi = M.lo_hi(K, s)
    y = np.stack([M.k4_input(Hp, Wp, lo, hi, 900 + b) for b in range(B)])
    refs = [M.k4_ref(y[b], pt, pl, h, w, mode, SCALE, K, s, lo, hi, clip) for b in range(B)]
    r, band = np.stack([v[0] for v in refs]), np.stack([v[1] for v in refs])
    assert B * h > 4096
    for entry in (('batch',) if mode == 0 else ('batch', 'batch_dev')):
        got = run_k4(entry, y, pt, pl, h, w, mode, K, s, lo, hi, clip)
        ratio, share, far = M.ulp_stats(got, r, band)
        acc(f"K4 {entry} B={B} h={h} mode {mode} clip {clip}: worst ratio {ratio:.4f}, two-answer share {share:.2e}, farther {far}")
        M.ulp_check(got, r, band, f"K4 {entry} B={B}")


def test_k4_nan_and_inf_inputs():
    """include/yond_hip.h: the input clamp takes a NaN (and -inf) as 0 and +inf as 1: the output is finite for any input."""
    gname, Hp, Wp, pt, pl, h, w = M.K4_GEOMS[0]
    K, s = 4.37, 6.27
    lo, hi = M.lo_hi(K, s)
    y = M.k4_input(Hp, Wp, lo, hi, 31)
    twin = y.copy()
    idx = np.arange(0, y.size, 97)
    y.reshape(-1)[idx[0::3]], twin.reshape(-1)[idx[0::3]] = np.nan, 0.0
    y.reshape(-1)[idx[1::3]], twin.reshape(-1)[idx[1::3]] = -np.inf, 0.0
    y.reshape(-1)[idx[2::3]], twin.reshape(-1)[idx[2::3]] = np.inf, 1.0
    for mode in (0, 1, 2):
        r, band = M.k4_ref(twin, pt, pl, h, w, mode, SCALE, K, s, lo, hi, 0)
        for entry in k4_entries(mode):
            got = run_k4(entry, y[None], pt, pl, h, w, mode, K, s, lo, hi, 0)[0]
            assert np.isfinite(got).all()
            M.ulp_check(got, r, band, f"K4 {entry} mode {mode} with NaN / Inf inputs")


# ---------------------------------------------------------------------------------------------------------------------------
# N1
# ---------------------------------------------------------------------------------------------------------------------------
SSIM_TOL, PSNR_TOL = 1e-9, 1e-6           # the tolerances of test_block_metrics_vs_oracle
# Why they hold with margin: C1 = 6.5 and C2 = 58.5 bound both denominators away from 0; a float64 moment of values up to 255^2 carries
# about 1e-10 of rounding over 121 taps, which is about 2e-12 on an SSIM value.


def run_n1(dn, hr, bh, bw):
    """yond_block_metrics_f32 -> per-tile sums [nblocks][ntiles][2], and pipeline.block_metrics' (psnr, ssim) with warnings as errors."""
    from yond_public_amd import _lib as L, pipeline as P
    lib = L.load()
    H, W = dn.shape
    nblk, nt = (H // bh) * (W // bw), lib.yond_block_metrics_tiles(bh, bw)
    assert nt == -(-bh // 32) * -(-bw // 32)
    out = canary(nblk * nt * 2, torch.float64)
    a, b = dev(dn), dev(hr)
    L.check(lib.yond_block_metrics_f32(L.ptr(a), L.ptr(b), H, W, bh, bw, L.ptr(out), L.stream()), "yond_block_metrics_f32")
    torch.cuda.synchronize()
    assert tail_intact(out, nblk * nt * 2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        psnr, ssim = P.block_metrics(a, b, bh=bh, bw=bw)
    return out[:nblk * nt * 2].cpu().numpy().reshape(nblk, nt, 2), psnr, ssim


def check_n1(tag, dn, hr, bh, bw):
    tiles, psnr, ssim = run_n1(dn, hr, bh, bw)
    nvalid = (bh - 10) * (bw - 10)
    ntx = -(-bw // 32)
    worst_s, worst_p = 0.0, 0.0
    for k, (a, b) in enumerate(zip(M.blocks(dn, bh, bw), M.blocks(hr, bh, bw))):
        se, ss = tiles[k, :, 0].sum(), tiles[k, :, 1].sum()
        se_ref, smap = M.se_ref(a, b), M.ssim_map_ref(a, b)
        ds = abs(ss - smap.sum()) / nvalid
        worst_s = max(worst_s, ds, abs(ssim[k] - smap.sum() / nvalid))
        assert ds <= SSIM_TOL and abs(ssim[k] - smap.sum() / nvalid) <= SSIM_TOL, (tag, k, ss, smap.sum())
        if se_ref == 0:
            assert se == 0.0 and psnr[k] == np.inf and ss == float(nvalid), (tag, k, se, ss)       # identical images: exact
        else:
            dp = abs(10 * np.log10(se / se_ref))
            worst_p = max(worst_p, dp, abs(psnr[k] - M.psnr_ref(a, b)))
            assert dp <= PSNR_TOL and abs(psnr[k] - M.psnr_ref(a, b)) <= PSNR_TOL, (tag, k, se, se_ref)
        # per tile: its own pixels' squared error; a tile wholly outside the 'valid' map adds exactly 0 to the SSIM sum
        d2 = (a.astype(np.float64) - b.astype(np.float64)) ** 2
        for t in range(tiles.shape[1]):
            y0, x0 = (t // ntx) * 32, (t % ntx) * 32
            want = d2[y0:y0 + 32, x0:x0 + 32].sum()
            assert abs(tiles[k, t, 0] - want) <= 1e-12 * max(want, 1e-300) + 0.0, (tag, k, t)
            vy, vx = max(0, min(32, bh - 10 - y0)), max(0, min(32, bw - 10 - x0))
            if vy * vx == 0:
                assert tiles[k, t, 1] == 0.0, (tag, k, t)
            else:
                want_s = smap[y0:y0 + vy, x0:x0 + vx].sum()
                assert abs(tiles[k, t, 1] - want_s) <= SSIM_TOL * vy * vx, (tag, k, t)
    return worst_s, worst_p, float(np.min(ssim)), float(np.max(ssim))


@pytest.mark.parametrize("gi", range(len(M.N1_GEOMS)), ids=[g[0].replace(' ', '_') for g in M.N1_GEOMS])
def test_n1_blocks_against_the_direct_float64_sums(gi):
    gname, H, W, bh, bw = M.N1_GEOMS[gi]
    for pi, kind in enumerate(M.N1_PAIRS):
        dn, hr = M.n1_pair(kind, H, W, bh, bw, seed=gi * 16 + pi)
        ws, wp, smin, smax = check_n1(f"{gname} {kind}", dn, hr, bh, bw)
        acc(f"N1 {gname} {kind}: worst |SSIM - ref| = {ws:.2e}, worst |PSNR - ref| = {wp:.2e} dB, SSIM in [{smin:.4f}, {smax:.4f}]")


@pytest.mark.parametrize("kind", ('near', 'independent'))
def test_n1_whole_frame_1000x1502(kind):
    """YOND_full.py's call: bh = H, bw = W on a whole frame whose last row and column of tiles are ragged."""
    H, W = 1000, 1502
    dn, hr = M.n1_pair(kind, H, W, H, W, seed=99)
    ws, wp, smin, smax = check_n1(f"whole 1000x1502 {kind}", dn, hr, H, W)
    acc(f"N1 whole 1000x1502 {kind}: worst |SSIM - ref| = {ws:.2e}, worst |PSNR - ref| = {wp:.2e} dB, SSIM {smin:.4f}")


def test_n1_low_zero_and_negative_ssim_are_reached():
    dn, hr = M.n1_pair('inverted', 74, 75, 74, 75, seed=5)
    assert M.ssim_ref(dn, hr) < -0.5
    dn, hr = M.n1_pair('independent', 74, 75, 74, 75, seed=5)
    assert abs(M.ssim_ref(dn, hr)) < 0.05


def test_n1_refuses_more_tiles_than_the_launch_holds():
    """Host side only: no launch of such a size is attempted."""
    from yond_public_amd import _lib as L, pipeline as P
    lib = L.load()
    assert lib.yond_block_metrics_tiles(8192 + 32, 8192 + 32) == -2               # YOND_EUNSUPPORTED: 257 * 257 = 66,049 tiles
    assert lib.yond_block_metrics_tiles(8160, 8160) == 255 * 255 and lib.yond_block_metrics_tiles(8160, 8192) == 255 * 256
    assert lib.yond_block_metrics_tiles(10, 300) == -1 and lib.yond_block_metrics_tiles(11, 11) == 1
    big = np.broadcast_to(np.float32(0), (8224, 8224))
    with pytest.raises(L.YondHipError, match="65535"):
        P.block_metrics(big, big, bh=8224, bw=8224)
