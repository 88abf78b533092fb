"""Camera noise on the GPU: what a sensor adds to Poisson-Gaussian noise at the exposure ratios of the low-light drivers -- heavy-tailed
(Tukey-lambda) read noise, row noise (banding), quantisation noise and a dark bias -- for a whole batch or frame in one HIP launch
(csrc/camnoise.hip, yond_camera_noise_f32).  The model is the reference's generate_noisy_obs (data_process/process.py:631-671) with
its noise codes, MultiFrameMean, the `ratio` exposure and its clip; the per-camera parameter prior is its sample_params (:394-452).

Noise is Philox4x32-10 on the device, keyed by (key, slot) per item and counted by the element index (the row index for the row
noise): an element's value depends on its item's parameters, its index, its clean value and the frame geometry only.  NumPy's
realisation is not reproduced.  The host keeps what is per item: the parameter prior (sample_camera_params, on a parameter table that
is PASSED IN: this package carries no camera tables), the YondCamItem array (plan) and the Poisson-Gaussian level the blind estimator
should find under it (effective_pg).  There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

ITEM_DTYPE = np.dtype([('beta1', '<f4'), ('sig_read', '<f4'), ('lam', '<f4'), ('sig_row', '<f4'), ('q_step', '<f4'), ('bias', '<f4', (4,)),
                       ('exposure', '<f4'), ('mfm', '<f4'), ('clip_lo', '<f4'), ('clip_hi', '<f4'), ('flags', '<u4'), ('key', '<u4'),
                       ('slot', '<u4')])
assert ITEM_DTYPE.itemsize == 64                                # YondCamItem of include/yond_hip.h

FLAG_POISSON, FLAG_TUKEY, FLAG_CLIP = 1, 2, 4                   # YOND_CAM_* of include/yond_hip.h
LAYOUT_PLANAR, LAYOUT_BAYER = 0, 1                              # [4][h][w] packed planes / [H][W] mosaic
NOISE_CODES = 'pgrqdb'


def _zeta(k):
    """Riemann zeta at an integer k >= 2: 30 terms and the Euler-Maclaurin tail (k >= 5: error < 1e-17), constants below."""
    if k == 2:
        return math.pi ** 2 / 6
    if k == 3:
        return 1.2020569031595942
    if k == 4:
        return math.pi ** 4 / 90
    N = 30.0
    return (math.fsum(n ** -float(k) for n in range(1, 30)) + N ** (1 - k) / (k - 1) + 0.5 * N ** -k + k * N ** (-k - 1) / 12
            - k * (k + 1) * (k + 2) * N ** (-k - 3) / 720)


def tukeylambda_variance(lam):
    """Variance of the Tukey-lambda law of shape `lam` and scale 1 (scipy.stats.tukeylambda.var): the closed form
    2 / lam^2 * (1 / (1 + 2 lam) - Gamma(lam + 1)^2 / Gamma(2 lam + 2)), pi^2 / 3 at 0 (the logistic law), infinite for lam <= -1/2.
    For |lam| > 1/4 the bracket goes through math.lgamma as it stands.  Nearer 0 it is a difference of two numbers near 1 that leaves
    O(lam^2), and lgamma's last bits would be most of it; there the ratio of Gammas is taken from the series of log Gamma(1 + x) =
    -gamma x + sum_{k >= 2} zeta(k) (-x)^k / k, in which the terms linear in lam cancel on paper:
        Gamma(lam + 1)^2 / Gamma(2 lam + 2) = exp(S) / (1 + 2 lam),   S = sum_{k >= 2} zeta(k) (-lam)^k (2 - 2^k) / k = O(lam^2)
        variance = -2 expm1(S) / (lam^2 (1 + 2 lam)),   with S / lam^2 summed as it stands (a lam whose square underflows is fine)
    (|2 lam| <= 1/2: 60 terms leave 2^-60 / 60)."""
    lam = float(lam)
    if math.isnan(lam):
        return float('nan')
    if lam <= -0.5:
        return float('inf')
    if lam == 0.0:
        return math.pi ** 2 / 3
    if abs(lam) <= 0.25:
        T = math.fsum(_zeta(k) * (-lam) ** (k - 2) * (2.0 - 2.0 ** k) / k for k in range(2, 62))      # S / lam^2
        S = T * lam * lam
        return -2.0 * T * (math.expm1(S) / S if S != 0.0 else 1.0) / (1.0 + 2.0 * lam)
    g = 2.0 * math.lgamma(lam + 1.0) - math.lgamma(2.0 * lam + 2.0)
    return 2.0 / (lam * lam) * (1.0 / (1.0 + 2.0 * lam) - math.exp(g))


def _code(noise_code):
    code = str(noise_code).lower()
    if not code or any(ch not in NOISE_CODES for ch in code):
        raise ValueError(f"noise code {noise_code!r}: letters of {NOISE_CODES!r} (p Poisson shot, g Tukey-lambda read, r row, q quantisation, "
                         "d dark bias, b black: shot only)")
    return code


def sample_camera_params(rs, table, camera_name=None, ln_ratio=False):
    """The reference's sample_params (data_process/process.py:394-452) on the numpy.random.RandomState `rs` and a parameter table that
    is passed in: log K uniform in [Kmin, Kmax], the logs of sigTL, sigR, sigGs and of the bias normal around the camera's regression
    lines in log K, then the exposure ratio (uniform in [100, 300], or exp(uniform(-0.01, high)) with ln_ratio, high = 1 for a name
    holding 'CRVD', else 5).  The draws are the reference's, in its order, so the result equals the reference's after
    np.random.seed(s) bit for bit.

    table: {camera type: parameters} with `camera_name` naming the camera, or one camera's parameters (camera_name None).  The
    parameters are what the reference's get_camera_noisy_params returns: Kmin, Kmax, lam, q, wp, bl, sigTLk/b/sig, sigRk/b/sig,
    sigGsk/b/sig and, where measured, uReadk/b/sig.
      - dual ISO: a table holding '<name>_lowISO' and '<name>_highISO' but not '<name>' draws randint(2) first and takes one of them;
      - point ISO: parameters with 'K_points' (system gains) and 'log_sigGs_points' (the matching means of log sigGs) draw
        randint(len(K_points)) and take that point instead of a uniform log K (the reference's CRVD branch).
    A table without uRead* (the reference raises KeyError: 'uReadk' for such a regression camera -- NikonD850, IMX686) gives
    bias = 1.0 here: the value the reference's point-ISO branch yields for a camera without uRead*, exp(0).
    Returns {K, sigTL, sigR, sigGs, bias, lam, q, ratio, wp, bl}, DN of a (wp - bl)-DN range at capture."""
    name = '' if camera_name is None else str(camera_name)
    if camera_name is None:
        params = table
    else:
        if name not in table and f'{name}_lowISO' in table and f'{name}_highISO' in table:
            choice = rs.randint(2)
            name += '_lowISO' if choice < 1 else '_highISO'
        params = table[name]
    wp, bl, lam, q = params['wp'], params['bl'], params['lam'], params['q']
    mu_bias = None
    if 'K_points' in params:
        a_list = np.asarray(params['K_points'], np.float64)
        K_points = np.log(a_list)
        Gs_points = np.asarray(params['log_sigGs_points'], np.float64)
        choice = rs.randint(len(a_list))
        log_K = K_points[choice]
        K = a_list[choice]
        mu_TL = params['sigTLk'] * log_K + params['sigTLb'] if 'sigTLk' in params else 0
        mu_R = params['sigRk'] * log_K + params['sigRb'] if 'sigRk' in params else 0
        mu_Gs = Gs_points[choice]
    else:
        log_K = rs.uniform(low=params['Kmin'], high=params['Kmax'])
        K = np.exp(log_K)
        mu_TL = params['sigTLk'] * log_K + params['sigTLb'] if 'sigTLk' in params else q
        mu_R = params['sigRk'] * log_K + params['sigRb'] if 'sigRk' in params else q
        mu_Gs = params['sigGsk'] * log_K + params['sigGsb'] if 'sigGsk' in params else q
        if 'uReadk' in params:
            mu_bias = params['uReadk'] * log_K + params['uReadb']
    log_sigTL = rs.normal(loc=mu_TL, scale=params['sigTLsig']) if 'sigTLk' in params else 0
    log_sigR = rs.normal(loc=mu_R, scale=params['sigRsig']) if 'sigRk' in params else 0
    log_sigGs = rs.normal(loc=mu_Gs, scale=params['sigGssig']) if 'sigGsk' in params else q
    log_bias = rs.normal(loc=mu_bias, scale=params['uReadsig']) if mu_bias is not None else 0
    sigTL, sigR, sigGs, bias = np.exp(log_sigTL), np.exp(log_sigR), np.exp(log_sigGs), np.exp(log_bias)
    if ln_ratio:
        high = 1 if 'CRVD' in name else 5
        ratio = np.exp(rs.uniform(low=-0.01, high=high))
    else:
        ratio = rs.uniform(low=100, high=300)
    return {'K': K, 'sigTL': sigTL, 'sigR': sigR, 'sigGs': sigGs, 'bias': bias, 'lam': lam, 'q': q, 'ratio': ratio, 'wp': wp, 'bl': bl}


def _bias4(bias):
    b = np.asarray(0.0 if bias is None else bias, np.float64).reshape(-1)
    if b.size not in (1, 4):
        raise ValueError(f"bias: one value or one per CFA channel (4), got {b.size}")
    return np.broadcast_to(b, (4,)).copy()


def effective_pg(params, noise_code, mfm=1):
    """(K, sigma_eff) in DN: the Poisson-Gaussian level with the first two moments of the camera noise `noise_code` draws from
    `params` -- what a blind Poisson-Gaussian estimator should find.  With M = MultiFrameMean (`mfm`) and the reference's divisions
    (process.py:646-656: shot, read and row terms by sqrt(M), the quantisation term not):
        K = params['K'] / sqrt(M)
        sigma_eff^2 = (read variance) / M + sigR^2 / M [r] + 1 / 12 [q]
    read variance = sigTL^2 * tukeylambda_variance(lam) with 'g' (sigTL is the law's SCALE), else sigGs^2; nothing but shot noise with
    'b'.  Without 'p' the shot term is the Gaussian approximation of the same variance.  The dark bias [d] is a mean offset, not
    noise: dark_bias returns it."""
    code = _code(noise_code)
    M = float(mfm)
    if not (np.isfinite(M) and M > 0):
        raise ValueError(f"MultiFrameMean must be finite and > 0, got {mfm!r}")
    K = float(params['K']) / math.sqrt(M)
    if 'b' in code:
        return K, 0.0
    if 'g' in code:
        var = float(params['sigTL']) ** 2 * tukeylambda_variance(params['lam'])
    else:
        var = float(params.get('sigGs', 0.0)) ** 2
    var /= M
    if 'r' in code:
        var += float(params['sigR']) ** 2 / M
    if 'q' in code:
        var += 1.0 / 12.0
    return K, math.sqrt(var)


def dark_bias(params, noise_code):
    """The per-channel mean offset in DN that `noise_code` adds: params['bias'] (one value or four) with 'd' and without 'b', else 0."""
    code = _code(noise_code)
    return _bias4(params.get('bias')) if 'd' in code and 'b' not in code else np.zeros(4)


def plan(B, K, sig_read, scale, key, slots, lam=0.0, sig_row=0.0, q_step=0.0, bias=None, exposure=1.0, mfm=1.0, clip=None, poisson=True,
         tukey=False):
    """The YondCamItem array of one launch (host numpy, 64 bytes per item) from parameters in DN: beta1 = K / scale, and sig_read (the
    Gaussian deviation, or with `tukey` the Tukey-lambda scale), sig_row, q_step (the WIDTH of the quantisation noise: 1 for the
    reference's +-0.5 DN) and bias (one value or four per item) likewise / scale.  exposure = 1 / ratio; mfm = MultiFrameMean, the
    number of averaged frames (the item holds its root); clip: None or (lo, hi) in the normalised scale.  Every parameter is a scalar
    or a sequence of B values (bias: [4] or [B][4]).  Refused: anything non-finite, sig_* or q_step < 0, exposure or mfm <= 0,
    lam <= -0.5 (no variance)."""
    def per(v, what, dtype=np.float64):
        v = np.asarray(v, dtype)
        if v.ndim and v.shape != (B,):
            raise ValueError(f"{what}: shape {v.shape} for {B} items")
        return np.broadcast_to(v, (B,))
    it = np.zeros(B, ITEM_DTYPE)
    scale = per(scale, 'scale')
    b = np.asarray(0.0 if bias is None else bias, np.float64)
    if b.shape not in ((), (1,), (4,), (B, 1), (B, 4)):
        raise ValueError(f"bias: shape {b.shape} for {B} items of 4 channels")
    b = np.broadcast_to(b, (B, 4))
    mfm = per(mfm, 'mfm')
    if not (np.isfinite(mfm).all() and (mfm > 0).all()):
        raise ValueError("MultiFrameMean must be finite and > 0")
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        it['beta1'] = per(K, 'K') / scale
        it['sig_read'] = per(sig_read, 'sig_read') / scale
        it['sig_row'] = per(sig_row, 'sig_row') / scale
        it['q_step'] = per(q_step, 'q_step') / scale
        it['bias'] = b / scale[:, None]
    it['lam'] = per(lam, 'lam')
    it['exposure'] = per(exposure, 'exposure')
    it['mfm'] = np.sqrt(mfm)
    lo, hi = (0.0, 0.0) if clip is None else clip
    it['clip_lo'], it['clip_hi'] = per(lo, 'clip lo'), per(hi, 'clip hi')
    it['flags'] = (per(poisson, 'poisson', bool) * FLAG_POISSON + per(tukey, 'tukey', bool) * FLAG_TUKEY
                   + (FLAG_CLIP if clip is not None else 0)).astype(np.uint32)
    it['key'] = per(key, 'key', np.uint32)
    it['slot'] = per(slots, 'slots', np.uint32)
    for f in ('beta1', 'sig_read', 'sig_row', 'q_step', 'bias', 'lam', 'clip_lo', 'clip_hi'):
        if not np.isfinite(it[f]).all():
            raise ValueError(f"{f} must be finite (after the division by scale)")
    for f in ('sig_read', 'sig_row', 'q_step'):
        if (it[f] < 0).any():
            raise ValueError(f"{f} must be >= 0")
    if not (it['lam'] > -0.5).all():
        raise ValueError("lam must be > -0.5: the Tukey-lambda law has no variance below")
    if not (np.isfinite(it['exposure']).all() and (it['exposure'] > 0).all()):
        raise ValueError("exposure must be finite and > 0")
    if (it['clip_lo'] > it['clip_hi']).any():
        raise ValueError("clip: lo > hi")
    return it


def needs_geometry(items):
    """True if an item has row noise or a dark bias: the launch then needs the frame's layout and row length."""
    return bool((items['sig_row'] != 0).any() or (items['bias'] != 0).any())


def launch(clean, items, layout=LAYOUT_PLANAR, row_len=None, out=None):
    """yond_camera_noise_f32 over `clean` ([B][...], device float32, contiguous; any 4-byte-aligned view) for the host item array
    `items` (copied to the device on the current stream).  layout: LAYOUT_PLANAR, items of packed planes [4][h][row_len], or
    LAYOUT_BAYER, mosaics [H][row_len]; row_len defaults to clean's last dimension.  Items without row noise and bias need no
    geometry: any shape goes.  out: None for a new tensor, `clean` itself for in-place."""
    _lib.require_cuda(clean, "clean")
    B = len(items)
    if clean.numel() == 0 or clean.numel() % B:
        raise ValueError(f"{tuple(clean.shape)} does not hold {B} items of one size")
    out = torch.empty_like(clean) if out is None else _lib.require_cuda(out, "out")
    if out.shape != clean.shape:
        raise ValueError(f"out is {tuple(out.shape)}, clean is {tuple(clean.shape)}")
    if layout not in (LAYOUT_PLANAR, LAYOUT_BAYER):
        raise ValueError(f"layout {layout!r}: {LAYOUT_PLANAR} (packed planes) or {LAYOUT_BAYER} (Bayer mosaic)")
    n = clean.numel() // B
    if needs_geometry(items):
        row_len = int(clean.shape[-1] if row_len is None else row_len)
        unit = n // 4 if layout == LAYOUT_PLANAR else n
        if row_len < 1 or (layout == LAYOUT_PLANAR and n % 4) or unit % row_len:
            raise ValueError(f"row noise / bias: rows of {row_len} do not divide items of {n} elements in layout {layout}")
    else:
        row_len = 0
    d_items = torch.from_numpy(np.ascontiguousarray(items).view(np.uint8)).to(clean.device)
    lib = _lib.load()
    _lib.check(lib.yond_camera_noise_f32(_lib.ptr(clean), _lib.ptr(out), n, B, C.c_void_p(d_items.data_ptr()), int(layout), row_len,
                                         _lib.stream()), "yond_camera_noise_f32")
    return out


def items_for(params, noise_code, scale, key, slots, ratio=1, mfm=1, clip=None):
    """plan() from the reference's parameter dicts ({K, sigTL, sigR, sigGs, bias, lam, wp, bl}, one or one per slot) and a noise code."""
    code = _code(noise_code)
    slots = np.atleast_1d(np.asarray(slots, np.uint32))
    B = len(slots)
    ps = [params] * B if isinstance(params, dict) else list(params)
    if len(ps) != B:
        raise ValueError(f"{len(ps)} parameter sets for {B} items")
    black = 'b' in code
    tl = 'g' in code and not black
    col = lambda name, default=0.0: [float(p.get(name, default)) for p in ps]
    if clip is None:
        bounds = None
    elif clip == '01':
        bounds = (0.0, 1.0)
    elif clip == 'sensor':
        bounds = ([-float(p['bl']) / float(p['wp']) for p in ps], 1.0)
    else:
        raise ValueError(f"clip {clip!r}: None, '01' or 'sensor'")
    return plan(B, col('K'), [0.0] * B if black else col('sigTL' if tl else 'sigGs'), scale, key, slots,
                lam=col('lam') if tl else 0.0, sig_row=col('sigR') if 'r' in code and not black else 0.0,
                q_step=1.0 if 'q' in code and not black else 0.0,
                bias=np.stack([dark_bias(p, code) for p in ps]), exposure=1.0 / np.asarray(ratio, np.float64), mfm=mfm, clip=bounds,
                poisson='p' in code, tukey=tl)


def add_camera_noise(clean, params, noise_code, scale, key, slots, layout=LAYOUT_PLANAR, ratio=1, mfm=1, clip=None, out=None,
                     row_len=None):
    """The reference's generate_noisy_obs (data_process/process.py:631-671) per element, on the device:

        noisy = clip(shot + read + row + q + bias + min(x, 0) e) / e,    e = 1 / ratio, y = max(x, 0) e, m = sqrt(mfm)

    noise_code, the reference's letters, case-insensitive:
        p   Poisson shot noise k beta1 / m, k ~ Poisson(m y / beta1); without it the Gaussian approximation of the same variance
        g   TUKEY-LAMBDA read noise of scale sigTL and shape lam (the reference's naming: WITHOUT g the read noise is Gaussian, sigGs)
        r   row noise sigR, one draw per row
        q   quantisation noise, uniform on +-0.5 DN (not divided by m)
        d   dark bias params['bias'], one value or one per CFA channel
        b   black: shot noise only, whatever else the code holds
    clean: [B, ...] device float32 with one item per entry of `slots`, or a single frame when `slots` holds one value.  layout:
    LAYOUT_PLANAR for items [4][h][w] (a row is a row of ONE plane, the reference's (c, h, 1) draw; the channel is the plane),
    LAYOUT_BAYER for mosaics [H][W] (a row is a sensor row; channel 2 (row & 1) + (col & 1), as bayer2rggb).
    params: the reference's parameter dict in DN at capture (sample_camera_params), one or one per item; scale = wp - bl;
    ratio, mfm (MultiFrameMean), key: scalars or per-item sequences.  The same (key, slot) gives the same noise.
    clip: None (none: the reference always clips), '01' for [0, 1] (the reference's clip=True), 'sensor' for the reference's default
    [-bl / wp, 1].  That bound is bl / wp, not bl / (wp - bl), although it is applied in the (wp - bl) scale: the reference's quirk,
    kept.  The clip stands before the multiplication by ratio, as in the reference.
    Returns the device tensor (`out` if given; `out=clean` works in place)."""
    return launch(clean, items_for(params, noise_code, scale, key, slots, ratio=ratio, mfm=mfm, clip=clip), layout=layout,
                  row_len=row_len, out=out)


def camera_noise_arg(text):
    """argparse type of `--camera-noise SPEC`: a comma list of key=value in DN at capture (before the ratio), e.g.
    code=pgrq,K=0.22,sigTL=0.76,sigGs=1.26,sigR=0.23,lam=-0.026.  Keys: code (letters of 'pgrqdb'), K (> 0), sigGs, sigTL, sigR (>= 0),
    lam (> -0.5), bias=b0/b1/b2/b3 (or one value), mfm (MultiFrameMean, > 0), clip (none | 01 | sensor).  What the code uses must be
    given: sigTL and lam with g, sigR with r, bias with d.  Returns {code, K, sigGs, sigTL, sigR, lam, bias [4], mfm, clip}."""
    import argparse

    def bad(msg):
        return argparse.ArgumentTypeError(f"{msg}; expected e.g. code=pgrq,K=0.22,sigTL=0.76,sigGs=1.26,sigR=0.23,lam=-0.026, got {text!r}")
    spec = {'code': None, 'K': None, 'sigGs': 0.0, 'sigTL': None, 'sigR': None, 'lam': None, 'bias': None, 'mfm': 1.0, 'clip': None}
    seen = set()
    for part in str(text).split(','):
        k, sep, v = part.partition('=')
        k, v = k.strip(), v.strip()
        if not sep or k not in spec or k in seen or not v:
            raise bad(f"{part!r} is not one key=value of {sorted(spec)}")
        seen.add(k)
        try:
            if k == 'code':
                spec[k] = _code(v)
            elif k == 'clip':
                if v not in ('none', '01', 'sensor'):
                    raise ValueError
                spec[k] = None if v == 'none' else v
            elif k == 'bias':
                spec[k] = _bias4([float(t) for t in v.split('/')])
            else:
                spec[k] = float(v)
        except ValueError:
            raise bad(f"{k}={v!r} does not parse") from None
    code = spec['code']
    if code is None or spec['K'] is None:
        raise bad("code= and K= are required")
    need = [k for k, ch in (('sigTL', 'g'), ('lam', 'g'), ('sigR', 'r'), ('bias', 'd')) if ch in code and spec[k] is None]
    if need:
        raise bad(f"code {code!r} needs {', '.join(need)}")
    spec['sigTL'], spec['sigR'], spec['lam'] = (0.0 if spec[k] is None else spec[k] for k in ('sigTL', 'sigR', 'lam'))
    spec['bias'] = np.zeros(4) if spec['bias'] is None else spec['bias']
    nums = [spec[k] for k in ('K', 'sigGs', 'sigTL', 'sigR', 'lam', 'mfm')] + list(spec['bias'])
    if not np.isfinite(nums).all():
        raise bad("every number must be finite")
    if not (spec['K'] > 0 and spec['mfm'] > 0 and min(spec['sigGs'], spec['sigTL'], spec['sigR']) >= 0 and spec['lam'] > -0.5):
        raise bad("K and mfm must be > 0, sigGs, sigTL and sigR >= 0, lam > -0.5")
    return spec
