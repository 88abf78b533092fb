"""The noise generators' Philox streams, replayed element by element: a NumPy model of the contract that csrc/philox.h,
csrc/pgnoise_sampler.h, csrc/camnoise_sampler.h and csrc/img2raw.hip document -- which counter words, which tag, which key, which word
feeds which draw, how many bits -- written from those comments, not from the code.  tests/test_noise_replay_model.py holds it to the
published Philox vectors and to the host-compiled samplers; tests/test_hip_noise_replay.py holds the kernels to it.

What is float64 here: Box-Muller, the Tukey-lambda quantile -- the values a kernel's float32 result is compared with under a
tolerance.  What is float32 here, step for step: the Poisson COUNT (pg_counts).  A count is an integer that hangs on float32
comparisons (u < cdf, floor(...), log V <= log f(k)), so a float64 evaluation would disagree with any float32 sampler at a few
elements in 10^4 at large lambda; the model therefore takes the sampler's float32 operations (+ - * / sqrt are correctly rounded in
NumPy, in the host build and, with -ffp-contract=off, on the device) and a CORRECTLY ROUNDED logf / expf / log1pf.  What is left to
differ between model, host build and device is the last bits of those functions, and robust_mask measures which elements hang on them.
"""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PG_TAG, CAM_TAG, CAM_ROW_TAG = 0x50474E31, 0x43414D31, 0x43524F57
PG_SWITCH_PTRS, PG_SWITCH_NORMAL, PG_INV_MAX, PG_MAX_ATTEMPTS = 10.0, 8388608.0, 64, 64
NUDGE_ULPS = 4
FRAGILE_SHARE_MAX = 1e-3

# Largest |host build - model| seen on the CPU (tests/test_noise_replay_model.py measures them again and fails if one is exceeded;
# profiles/noise_replay_report.txt has the run).  z, zs, row: absolute.  tl: relative to max(1, |model|) -- the variate reaches 1468 at
# lam = -0.26 and float32 holds it relatively.  The GPU tolerances are TOL_FACTOR times these: host and device functions are each a
# few ulps from the truth, so the device lies within a small multiple of the host's own distance; a contract defect is an O(1) error.
HOST_DEV = {"z": 1.5e-6, "zs": 1.5e-6, "row": 1.5e-6, "tl": 4.0e-7}
TOL_FACTOR = 4.0

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(v):
    return np.asarray(v).astype(np.uint64) & _M32


# -- Philox4x32-10 ----------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Salmon et al., SC 2011: ten rounds of two 32 x 32 -> 64 multiplies (0xD2511F53 on word 0, 0xCD9E8D57 on word 2), the key bumped
    by the Weyl constants (0x9E3779B9, 0xBB67AE85) after each.  uint64 arrays holding 32-bit values in, four such arrays out."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) for v in (c0, c1, c2, c3, k0, k1)))
    m0, m1, w0, w1 = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85))
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                                  # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def _stream(index, draw, tag, key, slot, d):
    """The four words of counter (index low, index high, draw, tag), key (key, slot), under the seeded defects `d`."""
    index = np.asarray(index).astype(np.uint64)
    k0, k1 = (slot, key) if d.get("swap_key") else (key, slot)
    return philox4x32_10(index & _M32, index >> _S32, draw, 0 if d.get("drop_tag") else tag, k0, k1, rounds=d.get("rounds", 10))


# -- uniforms (float64 holds each exactly) ------------------------------------------------------------------------------------------
def u24_pos(w):
    """((w >> 8) + 1) 2^-24 in (0, 1]"""
    return ((_u64(w) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def u24(w):
    """(w >> 8) 2^-24 in [0, 1)"""
    return (_u64(w) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def u33(w):
    """(w + 1) 2^-33 in [2^-33, 1/2], as float32 forms it: w and w + 1 each rounded to 24 bits (camnoise_sampler.h: "float32 keeps 24 of
    them RELATIVE to u").  The rounded u IS the draw: the quantile is taken of it."""
    return ((_u64(w).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -33)).astype(np.float64)


def u23_sym(w):
    """((w >> 9) + 0.5) 2^-23 - 0.5 in (-0.5, 0.5)"""
    return ((_u64(w) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23 - 0.5


def ptrs_uv(wu, wv):
    """PTRS's U = ((wu >> 8) - 2^23 + 0.5) 2^-24 in (-0.5, 0.5), never 0, and V = ((wv >> 8) + 1) 2^-24 in (0, 1]"""
    U = ((_u64(wu) >> np.uint64(8)).astype(np.float64) - 2.0 ** 23 + 0.5) * 2.0 ** -24
    return U, u24_pos(wv)


def box_muller(a, b):
    """(z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2), u1 = u24_pos(a), u2 = u24(b), float64"""
    r = np.sqrt(-2.0 * np.log(u24_pos(a)))
    t = 2.0 * np.pi * u24(b)
    return r * np.cos(t), r * np.sin(t)


def tukey_quantile(lam, u):
    """Q_lam(u) = (u^lam - (1 - u)^lam) / lam, log u - log(1 - u) at lam = 0; float64 (through expm1: the powers are 1 + O(lam))"""
    lam = float(np.float32(lam))
    lu, l1u = np.log(u), np.log1p(-u)
    if lam == 0.0:
        return lu - l1u
    return (np.expm1(lam * lu) - np.expm1(lam * l1u)) / lam


# -- the streams ------------------------------------------------------------------------------------------------------------------
def img2raw_normals(key, slot, groups, **d):
    """[groups][4]: group q's normals, counter (q, 0, 0, 0), key (patch.key, patch.slot); words 0, 1 -> z0, z1 and 2, 3 -> z2, z3."""
    w = _stream(np.arange(groups), 0, 0, key, slot, dict(d, drop_tag=False))
    z0, z1 = box_muller(w[0], w[1])
    z2, z3 = box_muller(w[2], w[3])
    return np.stack([z0, z1, z2, z3], axis=1)


def pg_z(key, slot, index, **d):
    """The read-noise normal of pg_draw: Box-Muller on words 0, 1 of draw 0, first value."""
    w = _stream(index, 0, PG_TAG, key, slot, d)
    a, b = d.get("z_words", (0, 1))
    return box_muller(w[a], w[b])[0]


def cam_draw(key, slot, index, lam, **d):
    """(tl, uq, zs) of camnoise_sampler.h's element draw: counter (index low, index high, 0, CAM_TAG)."""
    w = _stream(index, 0, CAM_TAG, key, slot, d)
    q = tukey_quantile(lam, u33(w[0]))
    sign = (w[d.get("sign_word", 1)] & np.uint64(1)).astype(bool)
    return np.where(sign, -q, q), u23_sym(w[2]), box_muller(w[3], w[1])[0]


def cam_row_normal(key, slot, row, **d):
    """counter (row low, row high, 0, CAM_ROW_TAG): Box-Muller on words 0, 1, first value"""
    w = _stream(row, 0, CAM_ROW_TAG, key, slot, d)
    return box_muller(w[0], w[1])[0]


def cam_rows(n, row_len):
    """The row of each of an item's n elements as csrc/camnoise.hip defines it: index / row_len, in either layout."""
    return np.arange(n) // int(row_len)


# -- the Poisson count, float32 step for step ----------------------------------------------------------------------------------------
_F = np.float32


def _r32(f, x):
    return f(np.asarray(x, np.float64)).astype(np.float32)


def _x_minus_log1p(x):
    big = np.abs(x) > _F(0.3)
    with np.errstate(all="ignore"):
        far = x - _r32(np.log1p, x)
        s = x / (_F(2.0) + x)
        t = s * s
        p = np.full_like(x, _F(1.0) / _F(15.0))
        for c in (13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            p = p * t + _F(1.0) / _F(c)
        near = s * x - _F(2.0) * (s * t) * p
    return np.where(big, far, near)


_LOG_FACT = np.array([0.0, 0.0, 0.69314718, 1.79175947, 3.17805383, 4.78749174, 6.57925121, 8.52516136, 10.60460290, 12.80182748], np.float32)


def _log_pmf(k, lam, loglam):
    with np.errstate(all="ignore"):
        small = k < _F(10.0)
        tab = k * loglam - lam - _LOG_FACT[np.clip(k, 0, 9).astype(np.int64)]
        d = k - lam
        x = d / lam
        rk = _F(1.0) / k
        rk2 = rk * rk
        stirling = rk * (_F(1.0) / _F(12.0) - rk2 * (_F(1.0) / _F(360.0) - rk2 * (_F(1.0) / _F(1260.0))))
        big = k * _x_minus_log1p(x) - d * x - _F(0.5) * _r32(np.log, _F(6.283185307179586) * k) - stirling
    return np.where(small, tab, big)


def pg_counts(key, slot, index, lam, **d):
    """k of pg_draw for every element, as float64.  lam: float32 values, one per element or one for all.  Regimes, thresholds, words and
    draw numbers as pgnoise_sampler.h states them: draw 0 words 2, 3 the first attempt (word 2 the inversion's uniform), draw j >= 1
    words (0, 1) and (2, 3) attempts 2j - 1 and 2j; zn the second Box-Muller value of draw 0.  Seeded defect `retry_shift`: added to the
    draw number of every retry."""
    index = np.asarray(index).astype(np.uint64)
    lam = np.broadcast_to(np.asarray(lam, np.float32), index.shape).copy()
    n = index.size
    k = np.zeros(n, np.float32)
    w = _stream(index, 0, PG_TAG, key, slot, d)
    # inversion
    inv = (lam > 0) & (lam < _F(PG_SWITCH_PTRS))
    if inv.any():
        l = lam[inv]
        u = (w[2][inv] >> np.uint64(8)).astype(np.float32) * _F(2.0 ** -24)
        p = _r32(np.exp, -l)
        cdf, kk, live = p.copy(), np.zeros_like(l), np.ones(l.shape, bool)
        for _ in range(PG_INV_MAX):
            live &= ~((u < cdf) | ((kk > l) & (p < _F(1.4901161e-8))))
            if not live.any():
                break
            kk = np.where(live, kk + _F(1.0), kk)
            pn = p * l / np.maximum(kk, _F(1.0))
            p = np.where(live, pn, p)
            cdf = np.where(live, cdf + p, cdf)
        k[inv] = kk
    # the normal regime's value (also what 64 refused attempts fall back to)
    a_, b_ = d.get("z_words", (0, 1))
    r = np.sqrt(_F(-2.0) * _r32(np.log, u24_pos(w[a_]).astype(np.float32)))
    zn = r * _r32(lambda t: np.sin(2.0 * np.pi * t), u24(w[b_]))
    with np.errstate(invalid="ignore"):
        slam = np.sqrt(lam)
        normal = np.maximum(0.0, np.rint(lam.astype(np.float64) + slam.astype(np.float64) * zn.astype(np.float64))).astype(np.float32)
    nor = lam > _F(PG_SWITCH_NORMAL)
    k[nor] = normal[nor]
    # PTRS
    pt = np.flatnonzero((lam >= _F(PG_SWITCH_PTRS)) & (lam <= _F(PG_SWITCH_NORMAL)))
    if pt.size:
        l, sl = lam[pt], slam[pt]
        loglam = _r32(np.log, l)
        b = _F(0.931) + _F(2.53) * sl
        a = _F(-0.059) + _F(0.02483) * b
        inv_alpha = _F(1.1239) + _F(1.1328) / (b - _F(3.4))
        vr = _F(0.9277) - _F(3.6224) / (b - _F(2.0))
        live = np.arange(pt.size)
        words = [x[pt] for x in w]
        for att in range(PG_MAX_ATTEMPTS):
            if live.size == 0:
                break
            if att & 1:
                fresh = _stream(index[pt[live]], ((att + 1) >> 1) + d.get("retry_shift", 0), PG_TAG, key, slot, d)
                for j in range(4):
                    words[j][live] = fresh[j]
            wu, wv = (words[0], words[1]) if att & 1 else (words[2], words[3])
            ll, aa, bb = l[live], a[live], b[live]
            U = ((wu[live] >> np.uint64(8)).astype(np.float64) - 8388608.0).astype(np.float32)
            U = (U + _F(0.5)) * _F(2.0 ** -24)
            V = ((wv[live] >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * _F(2.0 ** -24)
            us = _F(0.5) - np.abs(U)
            kd = np.floor(((_F(2.0) * aa / us + bb) * U).astype(np.float64) + ll.astype(np.float64) + 0.43)
            kf = kd.astype(np.float32)
            fast = (us >= _F(0.07)) & (V <= vr[live])
            skip = ~fast & ((kd < 0.0) | ((us < _F(0.013)) & (V > us)))
            with np.errstate(all="ignore"):
                lhs = _r32(np.log, V * inv_alpha[live] / (aa / (us * us) + bb))
                slow = ~fast & ~skip & (lhs <= _log_pmf(np.maximum(kf, _F(0.0)), ll, loglam[live]))
            done = fast | slow
            k[pt[live[done]]] = kf[done]
            live = live[~done]
        k[pt[live]] = normal[pt[live]]
    return k.astype(np.float64)


# -- the host builds of the samplers ----------------------------------------------------------------------------------------------------
def cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


_LIBS = {}
_DIR = []


def host_lib(which, nudge=None):
    """tests/<which>_host_sampler.cpp ("pgnoise" or "camnoise") built with the host compiler and loaded; nudge = k builds with
    -DYOND_NUDGE_ULPS=k.  Built once per process into a temporary directory."""
    if (which, nudge) in _LIBS:
        return _LIBS[which, nudge]
    if not _DIR:
        _DIR.append(tempfile.mkdtemp(prefix="noise_replay_"))
        atexit.register(shutil.rmtree, _DIR[0], ignore_errors=True)
    so = os.path.join(_DIR[0], f"lib{which}_host_{'plain' if nudge is None else nudge}.so")
    flags = [] if nudge is None else [f"-DYOND_NUDGE_ULPS=({int(nudge)})"]
    subprocess.run([cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", *flags, "-o", so,
                    os.path.join(ROOT, "tests", f"{which}_host_sampler.cpp")], check=True)
    lib = ctypes.CDLL(so)
    P, U, Q, Z, F = ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_float
    lib.yond_host_philox.argtypes = [Z] + [P] * 7
    lib.yond_host_philox.restype = None
    if which == "pgnoise":
        lib.pg_host_draw.argtypes = [U, U, Q, Z, P, Z, P, P]
        lib.pg_host_draw.restype = None
    else:
        lib.cam_host_draw.argtypes = [U, U, Q, Z, F, P, P, P]
        lib.cam_host_rows.argtypes = [U, U, Q, Z, P]
        lib.cam_host_draw.restype = lib.cam_host_rows.restype = None
    _LIBS[which, nudge] = lib
    return lib


def host_philox(c0, c1, c2, c3, k0, k1, which="pgnoise"):
    """[n][4] uint32: philox.h itself, compiled for the CPU"""
    arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint32), np.shape(c0))) for v in (c0, c1, c2, c3, k0, k1)]
    out = np.empty((arrs[0].size, 4), np.uint32)
    host_lib(which).yond_host_philox(arrs[0].size, *(a.ctypes.data for a in arrs), out.ctypes.data)
    return out


def host_pg_draw(key, slot, first, n, lam, nudge=None):
    """(k, z) float32 of pg_draw for elements first .. first + n - 1; element i takes lam[i % len(lam)]"""
    lam = np.ascontiguousarray(np.atleast_1d(np.asarray(lam, np.float32)))
    k, z = np.empty(n, np.float32), np.empty(n, np.float32)
    host_lib("pgnoise", nudge).pg_host_draw(int(key), int(slot), int(first), n, lam.ctypes.data, lam.size, k.ctypes.data, z.ctypes.data)
    return k, z


def host_cam_draw(key, slot, first, n, lam):
    tl, uq, zs = (np.empty(n, np.float32) for _ in range(3))
    host_lib("camnoise").cam_host_draw(int(key), int(slot), int(first), n, float(lam), tl.ctypes.data, uq.ctypes.data, zs.ctypes.data)
    return tl, uq, zs


def host_cam_rows(key, slot, first_row, n):
    z = np.empty(n, np.float32)
    host_lib("camnoise").cam_host_rows(int(key), int(slot), int(first_row), n, z.ctypes.data)
    return z


def robust_mask(key, slot, first, n, lam):
    """(mask, k): mask[i] is True where the builds nudged by 0, +NUDGE_ULPS and -NUDGE_ULPS give element i the same count (k, the
    unnudged build's).  Why 4 ulps: the device's and glibc's logf / expf / log1pf are each specified to a few ulps of the true value,
    so they differ from one another by at most about that.  The figure is not measured on the device."""
    k0 = host_pg_draw(key, slot, first, n, lam)[0]
    kp = host_pg_draw(key, slot, first, n, lam, nudge=NUDGE_ULPS)[0]
    km = host_pg_draw(key, slot, first, n, lam, nudge=-NUDGE_ULPS)[0]
    return (k0 == kp) & (k0 == km), k0


# -- the comparisons the GPU tests make (the seeded-defect test applies the same ones to host output against a broken model) ------------
def compare_counts(got, want, mask, lam):
    """Failures (list of str) of counts `got` against `want`: equal on every robust element (mask), the fragile share at most
    FRAGILE_SHARE_MAX; where lam > 2^23 (the count hangs on the Box-Muller normal) every element within 1 instead, none left out."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    lam = np.broadcast_to(np.asarray(lam, np.float32), got.shape)
    nor = lam > np.float32(PG_SWITCH_NORMAL)
    fails = []
    off = np.abs(got - want)
    if nor.any() and off[nor].max() > 1:
        fails.append(f"normal regime: {int((off[nor] > 1).sum())} of {int(nor.sum())} counts differ by more than 1 (worst {off[nor].max():.0f})")
    rest = ~nor
    if rest.any():
        share = float((~mask[rest]).mean())
        if share > FRAGILE_SHARE_MAX:
            fails.append(f"fragile share {share:.2e} > {FRAGILE_SHARE_MAX:.0e}")
        bad = rest & mask & (got != want)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            fails.append(f"{int(bad.sum())} robust counts differ, first at element {i}: {got[i]:.0f} vs {want[i]:.0f} (lambda {lam[i]})")
    return fails


def compare_values(got, want, tol, scale=None, what="value"):
    """Failures of `got` against the float64 `want`: |got - want| <= tol (an array or a number), times max(1, |want|) with scale='rel'."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return [f"{what}: shape {got.shape} vs {want.shape}"]
    bound = np.broadcast_to(np.asarray(tol, np.float64), want.shape) * (np.maximum(1.0, np.abs(want)) if scale == "rel" else 1.0)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        return [f"{what}: {int(bad.sum())} of {bad.size} outside the tolerance, first at {i}: {got.ravel()[i]!r} vs {want.ravel()[i]!r} "
                f"(bound {bound.ravel()[i]:.2e})"]
    return []


def deviation(got, want, scale=None):
    """The largest |got - want| (over max(1, |want|) with scale='rel'): the figure a tolerance is derived from"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (np.maximum(1.0, np.abs(want)) if scale == "rel" else 1.0)).max())


# -- img2raw's gather, moved here from tests/test_img2raw_host.py -----------------------------------------------------------------------
def gather_model(crop, table, rgb2cam, gain, k):
    """The kernel's per-element map in numpy (csrc/img2raw.hip): rotated-mosaic site -> source pixel -> curve -> CCM -> mask."""
    H, W, _ = crop.shape
    ho, wo = (W // 2, H // 2) if k & 1 else (H // 2, W // 2)
    c, y, x = np.meshgrid(np.arange(4), np.arange(ho), np.arange(wo), indexing="ij")
    i, j = 2 * y + (c >> 1), 2 * x + (c & 1)
    Y, X = [(i, j), (j, W - 1 - i), (H - 1 - i, W - 1 - j), (H - 1 - j, i)][k]
    ch = (Y & 1) + (X & 1)
    v = table[crop[Y, X].astype(np.int64)]                               # [4][ho][wo][3]
    cam = np.einsum("...j,cj->...c", v, rgb2cam.astype(np.float32)).astype(np.float32)
    gray = cam.sum(-1, dtype=np.float32) / np.float32(3)
    mask = (np.maximum(gray - np.float32(0.9), 0) / np.float32(0.1)) ** 2
    gc = gain[ch]
    o = np.take_along_axis(cam, ch[..., None], -1)[..., 0] * np.maximum(mask + (1 - mask) * gc, gc)
    return np.clip(o, 0, 1).astype(np.float32)
