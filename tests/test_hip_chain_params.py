"""GPU: the device frame chain's parameter block, knots, ordinates and flags (csrc/frame_params.h as compiled into
frame_params_kernel and into bias_lut_kernel's one-launch chain) against the float64 model of tests/chain_model.py -- every case
through yond_frame_params_f64 (+ yond_bias_lut_dev_f64 + yond_lut_table_f64) and through yond_frame_chain_f64, each compared with
the MODEL: beta within the model's bound of the exact rational fit, everything downstream against params() at the kernel's own
beta (<= 4 float64 ulp: an allowance for sqrt and the divisions, not a measurement; t <= 1 float32 ulp), flags and knot counts
exactly, knots bit for bit against the oracle's np.linspace calls."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import chain_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCALE, TFAC = 959.0, 1.03
SENT = -7.25                                  # prefill of the parameter block
HDR_FILL = 0x55                               # prefill of the table workspace (header n reads 0x55555555)
WORST = {}                                    # quantity -> (largest observed error, case)
BITEQ = [0, 0]                                # downstream values bit-equal to the model / compared


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k in sorted(WORST):
        print(f"[chain] worst {k}: {WORST[k][0]:.3g} ({WORST[k][1]})")
    print(f"[chain] downstream values bit-equal to the model: {BITEQ[0]} of {BITEQ[1]}")


def note(key, val, case):
    if np.isfinite(val) and val >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (float(val), case)


def cloud(b1, b2, n_ns=200, n_sat=0, wiggle=1e-4, lo=0.01, hi=0.75):
    """n_ns points around v = b1 m + b2 (a fixed relative pattern of +-wiggle) with non-saturated means, n_sat saturated points
    (mean >= 0.8) on ANOTHER line (2 b1 m + b2 + 1e-3): which sums were fitted shows in the answer."""
    pts = []
    for i in range(n_ns):
        m = lo + (hi - lo) * (i + 0.5) / n_ns
        pts.append((m, (b1 * m + b2) * (1.0 + wiggle * (((i * 7919) % 13) - 6) / 6.0)))
    for i in range(n_sat):
        m = 0.8 + 0.19 * (i + 0.5) / n_sat
        pts.append((m, 2 * b1 * m + b2 + 1e-3))
    return M.moments_of(pts)


def case(name, mom, mode=0, mx=0.9, lut_cap=None, flags=None, key=False, lut_ref=False, **kw):
    m_all, m_ns = mom
    return dict(name=name, all=np.asarray(m_all, np.float64), ns=np.asarray(m_ns, np.float64), mode=mode, mx=np.float32(mx), lut_cap=lut_cap,
                flags=flags, key=key, lut_ref=lut_ref, sel=(7.0, 0.0123, 40.0, 3.5e-5), **kw)


def build_cases():
    cs = []
    for K in (0.6, 4.0, 40.0):
        for s in (0.0, 2.0, 40.0):
            cs.append(case(f"fit_K{K:g}_s{s:g}", cloud(K / SCALE, (s / SCALE) ** 2), flags=0))
    b1, b2 = 4.0 / SCALE, (6.0 / SCALE) ** 2
    cs.append(case("ns_2_percent_used", cloud(b1, b2, 4, 196), used='ns', flags=0))
    cs.append(case("ns_exactly_1_percent_rejected", cloud(b1, b2, 2, 198), used='all', flags=0))
    cs.append(case("ns_half_percent_rejected", cloud(b1, b2, 1, 199), used='all', flags=0))
    cs.append(case("ns_empty", cloud(b1, b2, 0, 200), used='all', flags=0))
    # rank-deficient designs
    cs.append(case("rank_one_point", M.moments_of([(0.3, 2e-3)]), branch='rank', flags=0))
    cs.append(case("rank_constant_mean_1000", M.moments_of([(0.25, 1e-3 + 1e-6 * i) for i in range(1000)]), branch='rank', flags=0))
    for r, br in ((0.5e-12, 'rank'), (2e-12, 'fit')):
        m = [1000.0, 300.0, 2.0, 90.0 * (1.0 + r), 0.6 * (1.0 + r)]
        cs.append(case(f"det_{r / 1e-12:g}x_limit", (m, [0.0] * 5), branch=br))
    cs.append(case("no_points", ([0.0] * 5, [0.0] * 5), branch='empty', flags=M.NO_FLAT_AREA | M.BAD_ESTIMATE))
    # modes and flags
    neg = cloud(18.2 / SCALE, -1e-4)
    cs.append(case("mode0_b2_negative_sigma0_K18", neg, mode=0, mx=0.35, flags=0, lut_ref=True, sigma0=True))
    cs.append(case("mode1_b2_negative_b1_squared", neg, mode=1, flags=0, rule=True))
    cs.append(case("mode1_plain", cloud(b1, b2), mode=1, flags=0))
    down = cloud(-2e-3, 2e-3)
    cs.append(case("mode0_b1_negative", down, mode=0, flags=M.BAD_ESTIMATE))
    cs.append(case("mode1_b1_negative", down, mode=1, flags=M.ROUND_ABORTED | M.BAD_ESTIMATE))
    v = 2.0 ** -10                                   # means 0.25, 0.5, 0.75, 0.5 with one variance: b1 = 0 exactly
    cs.append(case("b1_zero", ([4.0, 2.0, 4 * v, 1.125, 2 * v], [4.0, 2.0, 4 * v, 1.125, 2 * v]), flags=M.BAD_ESTIMATE))
    cs.append(case("nan_in_sxy", ([100.0, 30.0, 0.3, 10.0, np.nan], [0.0] * 5), flags=M.BAD_ESTIMATE, nan=True))
    # maximum source and knot count
    cs.append(case("max_from_key", cloud(b1, b2), key=True, flags=0))
    cs.append(case("max_from_key_small", cloud(b1, b2), key=True, mx=0.031, flags=0))
    cs.append(case("max_negative", cloud(b1, b2), mx=-0.5, flags=M.LUT_CAPACITY))
    cs.append(case("max_nan", cloud(b1, b2), mx=np.nan, flags=M.LUT_CAPACITY))
    cs.append(case("max_nan_from_key", cloud(b1, b2), mx=np.nan, key=True, flags=M.LUT_CAPACITY))
    cs.append(case("knots_equal_capacity", cloud(b1, b2), mx=0.004, lut_cap=52, flags=0, nk=52))
    cs.append(case("knots_capacity_plus_one", cloud(b1, b2), mx=0.004, lut_cap=51, flags=M.LUT_CAPACITY, nk=0))
    cs.append(case("knots_over_default_capacity", cloud(b1, b2), mx=7.0, flags=M.LUT_CAPACITY, nk=0))
    # LDS capacity of the device LUT entries: 6144 doubles lie between rmax = 472 and 473 at K ~ 40 (13 rmax + 3 doubles)
    cs.append(case("lds_one_step_under", cloud(40.0 / SCALE, (64.7 / SCALE) ** 2), mx=0.35, flags=0, lut_ref=True, lds=13 * 472 + 3))
    cs.append(case("lds_one_step_over", cloud(40.0 / SCALE, (65.2 / SCALE) ** 2), mx=0.35, lds=13 * 473 + 3, lds_over=True))
    return cs


CASES = build_cases()


def _lib():
    from yond_public_amd import _lib as L
    return L, L.load()


def workspace(c):
    """A zeroed estimator workspace with the ten moment sums, the selection and (key path) the maximum's key written."""
    from yond_public_amd import pipeline as P
    L, lib = _lib()
    _, off_sel, off_mom, _, off_max = P._nle_layout()
    head = np.zeros(max(off_sel + 32, off_mom + 80, off_max + 4), np.uint8)
    head[off_mom:off_mom + 80] = np.concatenate([c['all'], c['ns']]).view(np.uint8)
    head[off_sel:off_sel + 32] = np.array(c['sel'], np.float64).view(np.uint8)
    if c['key']:
        head[off_max:off_max + 4] = np.array([M.float2key(c['mx'])], np.uint32).view(np.uint8)
    ws = torch.zeros(int(lib.yond_nle_ws_bytes(1024)), dtype=torch.uint8, device=DEV)
    ws[:len(head)] = torch.from_numpy(head).to(DEV)
    return ws


def buffers():
    from yond_public_amd import pipeline as P
    _, lib = _lib()
    nan = float('nan')
    return dict(prm=torch.full((16,), SENT, dtype=torch.float64, device=DEV), t=torch.full((1,), nan, dtype=torch.float32, device=DEV),
                lx=torch.full((P.LUT_CAP,), nan, dtype=torch.float64, device=DEV), ly=torch.full((P.LUT_CAP,), nan, dtype=torch.float32, device=DEV),
                lw=torch.full((int(lib.yond_lut_ws_bytes(P.LUT_CAP)),), HDR_FILL, dtype=torch.uint8, device=DEV))


def run(c, entry, use_key=None):
    """One case through an entry point.  Returns host copies: prm0 (the block as yond_frame_params_f64 left it; None for the chain),
    prm, t, lx, ly, header n."""
    from yond_public_amd import pipeline as P
    L, lib = _lib()
    key = c['key'] if use_key is None else use_key
    ws = workspace(dict(c, key=key))
    b = buffers()
    cap = c['lut_cap'] or P.LUT_CAP
    mxd = None if key else torch.tensor([c['mx']], dtype=torch.float32, device=DEV)
    prm0 = None
    if entry == 'params':
        L.check(lib.yond_frame_params_f64(L.ptr(ws), L.ptr(mxd), c['mode'], SCALE, SCALE, TFAC, cap, L.ptr(b['prm']), L.ptr(b['t']), L.ptr(b['lx']),
                                          L.stream()), "params")
        prm0 = b['prm'].clone()
        L.check(lib.yond_bias_lut_dev_f64(L.ptr(b['lx']), cap, L.ptr(b['prm']), L.ptr(b['ly']), L.stream()), "lut")
        L.check(lib.yond_lut_table_f64(L.ptr(b['lx']), L.ptr(b['ly']), -1, L.ptr(b['prm']), L.ptr(b['lw']), L.stream()), "table")
    else:
        L.check(lib.yond_frame_chain_f64(L.ptr(ws), L.ptr(mxd), c['mode'], SCALE, SCALE, TFAC, cap, L.ptr(b['prm']), L.ptr(b['t']), L.ptr(b['lx']),
                                         L.ptr(b['ly']), L.ptr(b['lw']), L.stream()), "chain")
    torch.cuda.synchronize()
    return dict(prm0=None if prm0 is None else prm0.cpu().numpy(), prm=b['prm'].cpu().numpy(), t=b['t'].cpu().numpy(), lx=b['lx'].cpu().numpy(),
                ly=b['ly'].cpu().numpy(), hdr_n=int(b['lw'][:4].cpu().numpy().view(np.int32)[0]))


_LUT_REF = {}


def oracle_lut(mx, sigma, K):
    """O.get_bias for the block's (K, sigma), once per case (shared by both entries)."""
    import yond_oracle as O
    k = (float(mx), float(sigma), float(K))
    if k not in _LUT_REF:
        _LUT_REF[k] = O.get_bias(np.float32(mx) * np.float32(SCALE), np.float64(sigma), np.float64(K))
    return _LUT_REF[k]


def check(c, r, entry):
    import yond_oracle as O
    from yond_public_amd import pipeline as P
    I = P.PRM
    name = f"{c['name']}/{entry}"
    cap = c['lut_cap'] or P.LUT_CAP
    prm = r['prm']
    f = M.fit(c['all'], c['ns'])
    for k in ('used', 'branch'):
        if k in c:
            assert f[k] == c[k], (name, k, f[k])
    b1k, b2k = prm[I['beta1']], prm[I['beta2']]
    exp_flags = 0 if c['all'][0] > 0 else M.NO_FLAT_AREA
    if c.get('nan'):
        assert np.isnan(b1k) and np.isnan(b2k)
        exp_flags |= M.BAD_ESTIMATE
        gain_k = sigma_k = np.nan
    else:
        # beta against the exact rational fit, within the model's bound
        d1 = abs(float(Fraction(float(b1k)) - f['b1']))
        note("|beta1 - exact| / bound", d1 / f['e1'] if f['e1'] else d1, name)
        assert d1 <= f['e1'], (name, d1, f['e1'])
        rule = c['mode'] == 1 and float(f['b2']) < 0
        if rule:
            assert float(f['b2']) + f['e2'] < 0, name                # (the case is clear of the branch)
            b2_in = float(f['b2'])
        else:
            if c['mode'] == 1:
                assert float(f['b2']) - f['e2'] >= 0, name
            d2 = abs(float(Fraction(float(b2k)) - f['b2']))
            note("|beta2 - exact| / bound", d2 / f['e2'] if f['e2'] else d2, name)
            assert d2 <= f['e2'], (name, d2, f['e2'])
            b2_in = b2k
        assert bool(c.get('rule')) == rule
        p = M.params(b1k, b2_in, c['mode'], SCALE, SCALE, TFAC)
        assert np.array_equal(np.float64(b2k).view(np.uint64), p['b2'].view(np.uint64)), (name, b2k, p['b2'])     # (mode 1: beta2 stored as b1^2)
        for q in ('gain', 'sigma', 'lo', 'hi', 'nsr'):
            u = M.ulps64(prm[I[q]], p[q])
            note(f"{q} ulp", u, name)
            BITEQ[0] += u == 0
            BITEQ[1] += 1
            assert u <= 4, (name, q, prm[I[q]], p[q])
        tk = prm[I['t']]
        assert np.isnan(tk) or np.float64(np.float32(tk)) == tk          # (a float32 stored in the float64 block)
        u = M.ulps32(np.float32(tk), p['t'])
        note("t ulp (float32)", u, name)
        BITEQ[0] += u == 0
        BITEQ[1] += 1
        assert u <= 1, (name, tk, p['t'])
        exp_flags |= p['flags']
        gain_k, sigma_k = prm[I['gain']], prm[I['sigma']]
        if c.get('sigma0'):
            assert sigma_k == 0.0 and b2k < 0
    # t_out, pass-through values
    t32 = np.float32(prm[I['t']])
    assert (np.isnan(r['t'][0]) and np.isnan(t32)) or r['t'][0].view(np.uint32) == t32.view(np.uint32), (name, r['t'][0], t32)
    assert prm[I['nsel']] == c['all'][0] and prm[I['th']] == c['sel'][1] and prm[I['pct']] == c['sel'][2]
    fm = prm[I['frame_max']]
    assert (np.isnan(fm) and np.isnan(c['mx'])) or fm == np.float64(c['mx']), (name, fm)
    assert np.all(prm[14:] == SENT)
    # knots
    (n1, n2, n3, nk), kfl = M.knot_shape(c['mx'], SCALE, cap)
    if 'nk' in c:
        assert nk == c['nk']
    exp_params_flags = exp_flags | kfl
    exp_final = exp_params_flags
    if not (exp_final & (M.BAD_ESTIMATE | M.LUT_CAPACITY)):
        need = M.lds_doubles(float(gain_k), float(sigma_k))
        if 'lds' in c:
            assert need == c['lds'], (name, need, gain_k, sigma_k)
        if need > M.BIAS_DEV_SMEM_DOUBLES:
            exp_final |= M.LUT_CAPACITY
    if c.get('lds_over'):
        assert exp_final == M.LUT_CAPACITY and exp_params_flags == 0
    if c['flags'] is not None:
        assert exp_final == c['flags'], (name, exp_final)
    if r['prm0'] is not None:
        assert int(r['prm0'][I['flags']]) == exp_params_flags, (name, r['prm0'][I['flags']], exp_params_flags)
        keep = [i for i in range(16) if i != I['flags']]
        assert np.array_equal(r['prm0'][keep].view(np.uint64), prm[keep].view(np.uint64))       # (the later launches touch the flags only)
    assert int(prm[I['flags']]) == exp_final, (name, prm[I['flags']], exp_final)
    assert int(prm[I['lut_n']]) == nk, (name, prm[I['lut_n']], nk)
    lx, ly = r['lx'], r['ly']
    assert np.all(np.isnan(lx[nk:]))
    if nk:
        with np.errstate(all='ignore'):
            ub = np.float32(np.ceil(c['mx'] * np.float32(SCALE))) + np.float32(1)
        want = np.asarray(O.bias_knots(ub), np.float64)
        assert len(want) == nk and np.array_equal(lx[:nk], want), name
    # ordinates and table header
    if exp_final & (M.BAD_ESTIMATE | M.LUT_CAPACITY):
        assert np.all(np.isnan(ly)), name                      # nothing written
        assert r['hdr_n'] == 0, (name, r['hdr_n'])
        return
    assert r['hdr_n'] == nk and np.all(np.isnan(ly[nk:])) and not np.any(np.isnan(ly[:nk])), name
    L, lib = _lib()
    xs = torch.from_numpy(lx[:nk].copy()).to(DEV)
    ys = torch.full((nk,), float('nan'), dtype=torch.float32, device=DEV)
    L.check(lib.yond_bias_lut_f64(L.ptr(xs), nk, float(gain_k), float(sigma_k), L.ptr(ys), L.stream()), "host-parameter LUT")
    torch.cuda.synchronize()
    assert np.array_equal(ys.cpu().numpy().view(np.uint32), ly[:nk].view(np.uint32)), name
    if c['lut_ref']:
        ref = oracle_lut(c['mx'], sigma_k, gain_k)
        assert np.array_equal(np.asarray(ref.x, np.float64), lx[:nk])
        want = np.asarray(ref.y, np.float64)
        err = float(np.abs(ly[:nk].astype(np.float64) - want).max())
        note("bias LUT ordinate vs oracle", err, name)
        print(f"[chain] {name}: K {gain_k:.4f} sigma {sigma_k:.4f}, {nk} knots, max |ordinate - oracle| = {err:.3e}, |bias| <= {np.abs(want).max():.3e}")
        assert err <= 2e-7 * max(1.0, float(np.abs(want).max())), name


@pytest.mark.parametrize("entry", ["params", "chain"])
@pytest.mark.parametrize("c", CASES, ids=[c['name'] for c in CASES])
def test_frame_params_against_model(c, entry):
    r = run(c, entry)
    p = r['prm']
    print(f"[chain] {c['name']}/{entry}: beta ({p[0]:.6e}, {p[1]:.6e}) K {p[2]:.5f} sigma {p[3]:.5f} flags {p[8]:.0f} knots {p[9]:.0f}")
    check(c, r, entry)
    if c['key']:                                  # the key path gives the block that the value passed in max_dev gives
        r2 = run(c, entry, use_key=False)
        assert np.array_equal(r2['prm'].view(np.uint64), p.view(np.uint64)) and np.array_equal(r2['lx'].view(np.uint64), r['lx'].view(np.uint64))
        assert np.array_equal(r2['ly'].view(np.uint32), r['ly'].view(np.uint32))


def test_chain_twice_on_one_workspace_and_no_t_out():
    """t_out = NULL is accepted by both entries; the chain's arrival counter is back at zero, so a second call on the same
    workspace gives the same block."""
    from yond_public_amd import pipeline as P
    L, lib = _lib()
    c = CASES[4]                                  # K 4, sigma 2
    ws = workspace(c)
    mxd = torch.tensor([c['mx']], dtype=torch.float32, device=DEV)
    outs = []
    for rep in range(2):
        b = buffers()
        L.check(lib.yond_frame_chain_f64(L.ptr(ws), L.ptr(mxd), 0, SCALE, SCALE, TFAC, P.LUT_CAP, L.ptr(b['prm']), None, L.ptr(b['lx']), L.ptr(b['ly']),
                                         L.ptr(b['lw']), L.stream()), "chain")
        outs.append(b)
    b3 = buffers()
    L.check(lib.yond_frame_params_f64(L.ptr(ws), L.ptr(mxd), 0, SCALE, SCALE, TFAC, P.LUT_CAP, L.ptr(b3['prm']), None, L.ptr(b3['lx']), L.stream()), "params")
    torch.cuda.synchronize()
    ref = run(c, 'chain')
    for b in outs:
        assert np.array_equal(b['prm'].cpu().numpy().view(np.uint64), ref['prm'].view(np.uint64))
        assert np.array_equal(b['ly'].cpu().numpy().view(np.uint32), ref['ly'].view(np.uint32))
        assert int(b['lw'][:4].cpu().numpy().view(np.int32)[0]) == ref['hdr_n'] > 0
        assert np.isnan(b['t'].item())                                # (never written)
    assert np.array_equal(b3['prm'].cpu().numpy().view(np.uint64), ref['prm'].view(np.uint64))


def test_argument_checks_launch_nothing():
    """YOND_EINVAL without a launch -- the sentinel block stays -- for mode 2, a scale or scale_est that is 0 or NaN, lut_cap < 2,
    lut_cap > LUT_MAX (the chain entry), and null pointers."""
    from yond_public_amd import pipeline as P
    L, lib = _lib()
    c = CASES[4]
    ws = workspace(c)
    mxd = torch.tensor([c['mx']], dtype=torch.float32, device=DEV)
    b = buffers()
    EINVAL = -1
    nan = float('nan')

    def params(ws_=ws, mode=0, se=SCALE, sc=SCALE, cap=P.LUT_CAP, prm=b['prm'], lx=b['lx']):
        return lib.yond_frame_params_f64(L.ptr(ws_), L.ptr(mxd), mode, se, sc, TFAC, cap, L.ptr(prm), L.ptr(b['t']), L.ptr(lx), L.stream())

    def chain(ws_=ws, mode=0, se=SCALE, sc=SCALE, cap=P.LUT_CAP, prm=b['prm'], lx=b['lx'], ly=b['ly'], lw=b['lw']):
        return lib.yond_frame_chain_f64(L.ptr(ws_), L.ptr(mxd), mode, se, sc, TFAC, cap, L.ptr(prm), L.ptr(b['t']), L.ptr(lx), L.ptr(ly), L.ptr(lw),
                                        L.stream())
    bad = [dict(mode=2), dict(mode=-1), dict(sc=0.0), dict(sc=nan), dict(se=0.0), dict(se=nan), dict(sc=-959.0), dict(cap=1), dict(cap=0),
           dict(ws_=None), dict(prm=None), dict(lx=None)]
    for kw in bad:
        assert params(**kw) == EINVAL, kw
        assert chain(**kw) == EINVAL, kw
    for kw in (dict(cap=4097), dict(ly=None), dict(lw=None)):
        assert chain(**kw) == EINVAL, kw
    assert lib.yond_bias_lut_dev_f64(None, P.LUT_CAP, L.ptr(b['prm']), L.ptr(b['ly']), L.stream()) == EINVAL
    assert lib.yond_bias_lut_dev_f64(L.ptr(b['lx']), 1, L.ptr(b['prm']), L.ptr(b['ly']), L.stream()) == EINVAL
    assert lib.yond_bias_lut_dev_f64(L.ptr(b['lx']), 4097, L.ptr(b['prm']), L.ptr(b['ly']), L.stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(b['prm'] == SENT) and torch.all(torch.isnan(b['t'])) and torch.all(torch.isnan(b['lx'])) and torch.all(torch.isnan(b['ly']))
    assert torch.all(b['lw'] == HDR_FILL)


def test_knot_sweep_every_integer_ub():
    """yond_frame_params_f64's knot grid for EVERY integer ub from 1 to 1536 (1536 launches in one stream, one synchronisation):
    count and knots bit-equal to the reference's np.linspace calls (O.bias_knots), NumPy 2's float32 runs included, nothing
    written beyond the count and no flag (ub 1536 needs 1057 knots of the 1536 the buffers hold)."""
    import yond_oracle as O
    from yond_public_amd import pipeline as P
    L, lib = _lib()
    N = 1536
    ubs = np.arange(1, N + 1)
    mx = (ubs - 1).astype(np.float32) - np.float32(0.3)            # ceil(mx) + 1 == ub at scale 1
    assert np.array_equal(np.ceil(mx) + 1, ubs.astype(np.float32))
    c = CASES[4]
    ws = workspace(c)
    mxd = torch.from_numpy(mx).to(DEV)
    prm = torch.full((N, 16), SENT, dtype=torch.float64, device=DEV)
    lx = torch.full((N, P.LUT_CAP), float('nan'), dtype=torch.float64, device=DEV)
    st = L.stream()
    for i in range(N):
        rc = lib.yond_frame_params_f64(L.ptr(ws), C.c_void_p(mxd.data_ptr() + 4 * i), 0, 1.0, 1.0, TFAC, P.LUT_CAP, C.c_void_p(prm.data_ptr() + 128 * i),
                                       None, C.c_void_p(lx.data_ptr() + 8 * P.LUT_CAP * i), st)
        assert rc == 0
    torch.cuda.synchronize()
    prm, lx = prm.cpu().numpy(), lx.cpu().numpy()
    for i, ub in enumerate(ubs):
        want = np.asarray(O.bias_knots(np.ceil(mx[i]) + 1), np.float64)
        n = int(prm[i, P.PRM['lut_n']])
        assert n == len(want) == M.knot_shape(mx[i], 1.0, P.LUT_CAP)[0][3], ub
        assert int(prm[i, P.PRM['flags']]) == 0, ub
        assert np.array_equal(lx[i, :n], want) and np.all(np.isnan(lx[i, n:])), ub
