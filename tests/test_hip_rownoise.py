"""GPU: the row-noise kernels (csrc/rownoise.hip, include/yond_hip.h M5) against the float64 model tests/rownoise_model.py, stage by stage
so that each bound is tight (the bounds are derived in the model's docstring):

  1. sums     against math.fsum, |err| <= (W / 2) * 2^-53 * sum |x| per entry; two calls give the same bits;
  2. offsets  against the model's filter evaluated on the kernel's OWN sums, read back: what remains is the device exp, the divisions and
              2 d additions -- offset_band;
  3. output   against float32(float64(in) - offsets_gpu): bit for bit;
  4. end to end against the model: half a float32 ulp of the result plus the band of stages 1 and 2 carried through -- e2e_band.

Shapes, in both `per` modes: 2 x 2 and 2 x 64 (one row per parity: the offset is exactly 0, out is in); 4 x 6 and 6 x 10 (W % 4 != 0: one
element per lane); 8 x 64 one float into a larger buffer (4-byte aligned only); 10 x 8 (d = 25 is wider than the sequence: the clamp on
every tap); 52 x 16 (interior rows and both borders); 2050 x 8 (more rows than the capped grid holds: the stride loop); 4 x 6004 and
4 x 16388 (a row longer than one pass of a wave's 64 x 4 x 4 elements); d = 1 (offset 0) and d = YOND_ROWNOISE_MAX_D; in place.  Data:
levels around 500 with row offsets of a few units; an 80-unit step across rows (more than 3 sigma_color: the range weight matters);
values times 10^U(-3, 3); one NaN pixel, one +inf pixel, a whole NaN row; every refusal.
"""
import numpy as np
import pytest

import rownoise_model as M

pytestmark = pytest.mark.gpu
SC, SS = 10.0, 9.0
#        name            H     W      d   frame keywords
CASES = {
    '2x2':          (2,    2,     25, {}),
    '2x64':         (2,    64,    25, {}),
    '4x6':          (4,    6,     25, {}),
    '6x10':         (6,    10,    25, {}),
    '10x8':         (10,   8,     25, {}),
    '52x16':        (52,   16,    25, {}),
    '52x16_step':   (52,   16,    25, {'step': 80.0}),
    '52x16_heavy':  (52,   16,    25, {'heavy': True}),
    '52x16_d1':     (52,   16,    1,  {}),
    '52x16_dmax':   (52,   16,    63, {}),
    '140x8_dmax':   (140,  8,     63, {}),
    '2050x8':       (2050, 8,     25, {}),
    '4x6004':       (4,    6004,  25, {}),
    '4x16388':      (4,    16388, 25, {}),
}
PARAMS = [(name, per) for name in CASES for per in (M.ROW, M.PLANE)]


def _frame(name):
    H, W, d, kw = CASES[name]
    x = M.frame(1000 + sorted(CASES).index(name), H, W, **kw).astype(np.float32)
    x.setflags(write=False)
    return x, d


@pytest.fixture(scope="module")
def models():
    """name -> (frame, d, fsum sums, sums bound): computed once, shared, never modified."""
    out = {}
    for name in CASES:
        x, d = _frame(name)
        out[name] = (x, d, M.row_sums(x), M.sums_bound(x))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _stages(x, d, per, sums_gpu, offsets_gpu, out_gpu, what, sums_model=None, sums_bound=None):
    """Stages 1 to 4 on what one run returned; every figure is printed before it is asserted."""
    H, W = x.shape
    sums_model = M.row_sums(x) if sums_model is None else sums_model
    sums_bound = M.sums_bound(x) if sums_bound is None else sums_bound
    fin = np.isfinite(sums_model)
    assert np.array_equal(np.isfinite(sums_gpu), fin)
    with np.errstate(invalid='ignore'):
        err1 = np.abs(sums_gpu - sums_model)[fin]
    print(f"[rownoise] {what}: sums: max err / bound = {float((err1 / sums_bound[fin]).max()) if err1.size else 0.0:.3f} "
          f"(max err {float(err1.max()) if err1.size else 0.0:.3e})")
    assert (err1 <= sums_bound[fin]).all()
    # 2: the filter on the kernel's own sums
    want_off = M.offsets_from_sums(sums_gpu, W, per, d, SC, SS)
    band2 = M.offset_band(sums_gpu, W, per, d, SC, SS)
    err2 = np.abs(offsets_gpu - want_off)
    print(f"[rownoise] {what}: offsets: max |gpu - model on the gpu's sums| = {float(err2.max()):.3e}, band there "
          f"{float(band2[np.unravel_index(err2.argmax(), err2.shape)]):.3e}, max |offset| {float(np.abs(want_off).max()):.3e}")
    assert np.isfinite(offsets_gpu).all() and (err2 <= band2).all()
    if per == M.ROW:
        assert np.array_equal(_bits(offsets_gpu[:, 0]), _bits(offsets_gpu[:, 1]))
    # 3: one subtraction, one rounding
    want_out, _ = M.apply(x, offsets_gpu)
    assert np.array_equal(_bits(out_gpu), _bits(want_out))
    # 4: end to end
    _, off_model, z = M.row_denoise(x, per, d, SC, SS, sums=sums_model)
    band4 = M.per_pixel(M.e2e_band(x, per, d, SC, SS), W)
    ok = np.isfinite(z)
    with np.errstate(invalid='ignore'):
        err4 = np.abs(out_gpu.astype(np.float64) - z)
        lim4 = 0.5 * np.spacing(np.abs(out_gpu)).astype(np.float64) + band4
    print(f"[rownoise] {what}: end to end: max err {float(err4[ok].max()):.3e}, max err / bound {float((err4[ok] / lim4[ok]).max()):.3f}, "
          f"band {float(band4.max()):.3e}")
    assert (err4[ok] <= lim4[ok]).all()
    assert np.array_equal(_bits(out_gpu)[~ok], _bits(x)[~ok])            # a non-finite pixel is copied
    return off_model


def _run(x, d, per, offset_floats=0):
    """(sums, sums again, offsets, out) as NumPy from the device; offset_floats > 0: the frame starts that many floats into its buffer."""
    import torch
    from yond_public_amd import rownoise as RN
    H, W = x.shape
    buf = torch.zeros(H * W + 4, dtype=torch.float32, device='cuda')
    dev = buf[offset_floats:offset_floats + H * W].view(H, W)
    dev.copy_(torch.from_numpy(np.array(x)))
    assert dev.data_ptr() % 16 == 4 * offset_floats and dev.is_contiguous()
    s1, s2 = RN.row_sums(dev), RN.row_sums(dev)
    out, off = RN.row_denoise(dev, sigma_color=SC, sigma_space=SS, d=d, per=per, return_offsets=True)
    torch.cuda.synchronize()
    assert out.data_ptr() != dev.data_ptr() and out.dtype == torch.float32 and off.dtype == torch.float64 and tuple(off.shape) == (H, 2)
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(x))            # the input is left alone
    return s1.cpu().numpy(), s2.cpu().numpy(), off.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("name,per", PARAMS)
def test_stages_against_the_model(models, name, per):
    x, d, sums_model, sums_bound = models[name]
    s1, s2, off, out = _run(x, d, per)
    assert np.array_equal(_bits(s1), _bits(s2))                          # the same call gives the same bits
    _stages(x, d, per, s1, off, out, f"{name} {per}", sums_model, sums_bound)
    if x.shape[0] == 2 or d == 1:
        assert (off == 0).all() and np.array_equal(_bits(out), _bits(x))  # one row per parity, or one tap: exactly 0, out is in
    elif 'heavy' not in name:
        assert np.abs(off).max() > 0.1                                   # the case does remove something


@pytest.mark.parametrize("per", [M.ROW, M.PLANE])
@pytest.mark.parametrize("offset_floats", [1, 2])
def test_a_frame_that_is_only_4_byte_aligned(per, offset_floats):
    x = M.frame(77, 8, 64).astype(np.float32)
    s1, s2, off, out = _run(x, 25, per, offset_floats)
    assert np.array_equal(_bits(s1), _bits(s2))
    _stages(x, 25, per, s1, off, out, f"8x64 +{offset_floats} floats {per}")
    # the 16-byte path on the same frame: its sums may differ in the order of the additions, within stage 1's bound on either side
    a1, _, _, _ = _run(x, 25, per, 0)
    assert (np.abs(a1 - s1) <= 2 * M.sums_bound(x)).all()


def test_step_edge_needs_the_range_weight(models):
    """The kernel's offsets on the step frame are the model's and not the variant's without a range weight."""
    x, d, sums_model, _ = models['52x16_step']
    _, _, off, _ = _run(x, d, M.ROW)
    no_range = M.offsets_from_sums(sums_model, x.shape[1], M.ROW, d, SC, SS, defect='no_range_weight')
    model = M.offsets_from_sums(sums_model, x.shape[1], M.ROW, d, SC, SS)
    print(f"[rownoise] step: max |gpu - model| {np.abs(off - model).max():.3e}, max |gpu - no_range_weight| {np.abs(off - no_range).max():.3e}")
    assert np.abs(off - no_range).max() > 10 and (np.abs(off - model) <= M.e2e_band(x, M.ROW, d, SC, SS)).all()


@pytest.mark.parametrize("name,per", [('52x16', M.ROW), ('52x16', M.PLANE), ('4x6004', M.ROW), ('6x10', M.PLANE)])
def test_in_place(models, name, per):
    import torch
    from yond_public_amd import _lib as L
    from yond_public_amd import rownoise as RN
    x, d, sums_model, sums_bound = models[name]
    H, W = x.shape
    dev = torch.from_numpy(np.array(x)).cuda()
    sums = RN.row_sums(dev)
    off = torch.empty((H, 2), dtype=torch.float64, device='cuda')
    L.check(L.load().yond_rownoise_apply_f32(L.ptr(dev), L.ptr(dev), H, W, L.ptr(sums), RN.PER[per], d, SC, SS, L.ptr(off), L.stream()), "apply in place")
    torch.cuda.synchronize()
    _stages(x, d, per, sums.cpu().numpy(), off.cpu().numpy(), dev.cpu().numpy(), f"{name} {per} in place", sums_model, sums_bound)
    # without an offsets buffer: the same frame
    dev2 = torch.from_numpy(np.array(x)).cuda()
    L.check(L.load().yond_rownoise_apply_f32(L.ptr(dev2), L.ptr(dev2), H, W, L.ptr(sums), RN.PER[per], d, SC, SS, None, L.stream()), "apply in place")
    assert torch.equal(dev2, dev)


CONTAIN = {'nan pixel': ((9, 5), np.nan), '+inf pixel': ((30, 2), np.inf), 'nan row': ((21, slice(None)), np.nan)}


@pytest.mark.parametrize("per", [M.ROW, M.PLANE])
@pytest.mark.parametrize("kind", list(CONTAIN))
def test_non_finite_values_are_contained(kind, per):
    """The affected row (per='plane': its affected column phase) has offset 0 and passes through bit for bit; every other row is the
    model's; nothing else is non-finite."""
    where, value = CONTAIN[kind]
    x = M.frame(88, 52, 16).astype(np.float32)
    x[where] = value
    y0 = where[0]
    s1, _, off, out = _run(x, 25, per)
    _stages(x, 25, per, s1, off, out, f"{kind} {per}")
    phases = [0, 1] if per == M.ROW or isinstance(where[1], slice) else [where[1] & 1]
    for c in phases:
        assert off[y0, c] == 0.0 and np.array_equal(_bits(out[y0, c::2]), _bits(x[y0, c::2]))
    assert np.array_equal(np.isfinite(out), np.isfinite(x)) and np.isfinite(off).all()
    clean = np.delete(off, y0, axis=0)
    assert np.abs(clean).max() > 0.1                                     # the neighbours are still denoised


def test_refusals_leave_out_untouched():
    import torch
    from yond_public_amd import _lib as L
    from yond_public_amd import rownoise as RN
    H, W = 8, 16
    dev = torch.from_numpy(M.frame(5, H, W).astype(np.float32)).cuda()
    sums = RN.row_sums(dev)
    out = torch.full((H * W + 4,), -7.0, dtype=torch.float32, device='cuda')
    off = torch.full((H, 2), -7.0, dtype=torch.float64, device='cuda')
    f = L.load().yond_rownoise_apply_f32
    o, st = L.ptr(out), L.stream()
    import ctypes
    shifted = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    ok = (RN.PER['row'], 25, SC, SS)
    calls = [(None, o, H, W, L.ptr(sums), *ok), (L.ptr(dev), None, H, W, L.ptr(sums), *ok), (L.ptr(dev), o, H, W, None, *ok),
             (shifted(dev, 2), o, H, W, L.ptr(sums), *ok), (L.ptr(dev), shifted(out, 2), H, W, L.ptr(sums), *ok),
             (L.ptr(dev), o, H, W, shifted(sums, 4), *ok),
             (L.ptr(dev), o, 7, W, L.ptr(sums), *ok), (L.ptr(dev), o, H, 15, L.ptr(sums), *ok), (L.ptr(dev), o, 0, W, L.ptr(sums), *ok),
             (L.ptr(dev), o, H, -2, L.ptr(sums), *ok), (L.ptr(dev), o, 65536, 32768, L.ptr(sums), *ok)]
    big = torch.full((2 * H * W,), -7.0, dtype=torch.float32, device='cuda')
    calls += [(L.ptr(big), shifted(big, 4 * n), H, W, L.ptr(sums), *ok) for n in (1, W, H * W - 1)]        # out overlaps in without being in
    calls += [(shifted(big, 4 * W), L.ptr(big), H, W, L.ptr(sums), *ok)]
    calls += [(L.ptr(dev), o, H, W, L.ptr(sums), RN.PER['row'], d, SC, SS) for d in (0, -3, 24, RN.MAX_D + 1, RN.MAX_D + 2)]
    calls += [(L.ptr(dev), o, H, W, L.ptr(sums), RN.PER['row'], 25, sc, ss)
              for sc, ss in ((0.0, SS), (-1.0, SS), (SC, 0.0), (SC, -1.0), (float('nan'), SS), (SC, float('nan')), (float('inf'), SS), (SC, float('inf')))]
    calls += [(L.ptr(dev), o, H, W, L.ptr(sums), per, 25, SC, SS) for per in (-1, 2)]
    for args in calls:
        assert f(*args, L.ptr(off), st) == -1, args[2:]
    assert f(L.ptr(dev), o, H, W, L.ptr(sums), *ok, shifted(off, 4), st) == -1
    g = L.load().yond_rownoise_sums_f32
    poison = torch.full((H, 2), -7.0, dtype=torch.float64, device='cuda')
    for args in ((None, H, W, L.ptr(poison)), (L.ptr(dev), H, W, None), (shifted(dev, 2), H, W, L.ptr(poison)), (L.ptr(dev), H, W, shifted(poison, 4)),
                 (L.ptr(dev), 7, W, L.ptr(poison)), (L.ptr(dev), H, 15, L.ptr(poison)), (L.ptr(dev), 65536, 32768, L.ptr(poison))):
        assert g(*args, st) == -1, args[1:3]
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((off == -7.0).all()) and bool((poison == -7.0).all()) and bool((big == -7.0).all())
    # the wrapper's own errors
    with pytest.raises(ValueError):
        RN.row_denoise(dev)                                              # sigma_space=None needs iso
    with pytest.raises(ValueError):
        RN.row_denoise(dev, 1600, d=24)
    with pytest.raises(L.YondHipError):
        RN.row_denoise(dev[:7], 1600)
    with pytest.raises(L.YondHipError):
        RN.row_denoise(dev.double(), 1600)


def test_the_reference_seam(tmp_path):
    """utils.isp_algos.row_denoise(path, iso, data=None): the reference's signature, a device tensor or a .npy file."""
    import torch
    from yond_public_amd import rownoise as RN
    from yond_public_amd.utils import isp_algos
    x = M.frame(6, 20, 16).astype(np.float32)
    dev = torch.from_numpy(x).cuda()
    want = RN.row_denoise(dev, 800)
    assert torch.equal(isp_algos.row_denoise(None, 800, data=dev), want)
    np.save(tmp_path / "dark.npy", x)
    assert torch.equal(isp_algos.row_denoise(str(tmp_path / "dark.npy"), 800), want)
    _, _, z = M.row_denoise(x, M.ROW, 25, 10.0, 1 + 800 / 200)
    got = want.cpu().numpy()
    lim = 0.5 * np.spacing(np.abs(got)).astype(np.float64) + M.per_pixel(M.e2e_band(x, M.ROW, 25, 10.0, 1 + 800 / 200), 16)
    assert (np.abs(got.astype(np.float64) - z) <= lim).all()
