"""CPU: the model of the device frame chain's parameter block (tests/chain_model.py) against the oracle's restatement of the
reference -- polyfit / scipy.linalg.lstsq, VST, bias_knots, the mode rules of IterDenoise -- and the two clipped frames the
takeover tests (tests/test_hip_chain_takeover.py) rest on."""
from fractions import Fraction

import numpy as np
import pytest

import chain_model as M


def line_points(n, b1, b2, lo=0.01, hi=0.75, wiggle=1e-3, sat=0, sat_off=0.05):
    """n points on v = b1 m + b2 (1 +- wiggle, a fixed pattern) with means spread over [lo, hi], plus `sat` saturated points
    (mean >= 0.8) that lie OFF the line: a fit that includes them gives another answer."""
    pts = []
    for i in range(n):
        m = lo + (hi - lo) * (i + 0.5) / n
        pts.append((m, (b1 * m + b2) * (1.0 + wiggle * (((i * 7919) % 13) - 6) / 6.0)))
    for i in range(sat):
        m = 0.8 + 0.19 * (i + 0.5) / sat
        pts.append((m, b1 * m + b2 + sat_off * (1 + (i % 3))))
    return pts


def exact_on_points(pts):
    """Exact rational least-squares solution over the points themselves (minimum norm when the design is rank-deficient)."""
    P = [(Fraction(m), Fraction(v)) for m, v in pts]
    n = Fraction(len(P))
    sx, sy = sum(m for m, _ in P), sum(v for _, v in P)
    sxx, sxy = sum(m * m for m, _ in P), sum(m * v for m, v in P)
    det = n * sxx - sx * sx
    if det == 0:
        mbar, vbar = sx / n, sy / n
        return vbar * mbar / (mbar * mbar + 1), vbar / (mbar * mbar + 1)
    return (n * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det


FIT_SETS = {
    "well_K4_s6": (line_points(400, 4.0 / 959, (6.0 / 959) ** 2), 'ns', 'fit'),
    "well_K0.6_s0": (line_points(50, 0.6 / 959, 0.0), 'ns', 'fit'),
    "well_K40_s40_dark": (line_points(300, 40.0 / 959, (40.0 / 959) ** 2, 0.002, 0.2), 'ns', 'fit'),
    "ns_1.1_percent": (line_points(11, 4.0 / 959, 4e-5, sat=989), 'ns', 'fit'),
    "ns_exactly_1_percent": (line_points(10, 4.0 / 959, 4e-5, sat=990), 'all', 'fit'),
    "ns_0.9_percent": (line_points(9, 4.0 / 959, 4e-5, sat=991), 'all', 'fit'),
    # (lstsq finds rank 1 from COMPUTED singular values: at n = 1000 the second one comes out as 2.8e-14, above its eps * s_max
    # cut, and the routine returns -1.7e11; at 100 and 1024 points it is below the cut and the minimum-norm solution comes back)
    "constant_mean_100": ([(0.25, 1e-3 + 1e-5 * i) for i in range(100)], 'ns', 'rank'),
    "constant_mean_1024": ([(0.3, 1e-3 + 1e-5 * i) for i in range(1024)], 'ns', 'rank'),
    "one_point": ([(0.3, 2e-3)], 'ns', 'rank'),
}


@pytest.mark.parametrize("name", sorted(FIT_SETS))
def test_fit_matches_lstsq(name):
    """fit() on the moment sums against scipy.linalg.lstsq on [m, 1] (the routine O.polyfit calls): well-conditioned clouds, the
    non-saturated share on both sides of the 1 % rule, and the rank-deficient designs where lstsq returns the minimum-norm
    solution.  Tolerance: the model's own bound plus lstsq's error against the exact rational solution on the points it used."""
    import yond_oracle as O
    pts, used, branch = FIT_SETS[name]
    m_all, m_ns = M.moments_of(pts)
    f = M.fit(m_all, m_ns)
    assert (f['used'], f['branch']) == (used, branch)
    x, y = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    ref = O.polyfit(x, y)
    sel = [p for p in pts if 1e-4 < p[0] < 0.8] if used == 'ns' else pts
    ex = exact_on_points(sel)
    for i, key in enumerate(("b1", "b2")):
        resid = abs(float(Fraction(float(ref[i])) - ex[i]))
        err = abs(float(f[key] - Fraction(float(ref[i]))))
        print(f"[model] fit {name} {key}: model {float(f[key]):.17e}, lstsq {ref[i]:.17e}, |diff| {err:.2e}, bound {f['e' + key[1]]:.2e}, "
              f"lstsq residual {resid:.2e}")
        assert resid <= 1e-10 * max(abs(float(ex[0])), abs(float(ex[1])))          # (lstsq itself is sound on these sets)
        assert err <= f['e' + key[1]] + resid
    if name.startswith("ns_"):                                    # the other choice of sums gives a visibly different line
        other = M.fit(m_all, [0.0] * 5) if used == 'ns' else M.fit(m_ns, m_ns)
        assert abs(float(other['b2'] - f['b2'])) > 1e3 * (f['e2'] + other['e2'])


def test_fit_rule_and_rank_edges():
    """The 1 % rule is strict and in float64; det at half / twice the 1e-12 limit takes the minimum-norm / the normal-equation
    branch; n = 0 gives (0, 0); a NaN sum gives NaN."""
    m_all = np.array([200.0, 80.0, 1.0, 40.0, 0.5])
    assert M.fit(m_all, [2.0, 0.5, 0.01, 0.2, 0.003])['used'] == 'all'        # 2 > 0.01 * 200 is false
    assert M.fit(m_all, [3.0, 0.9, 0.01, 0.3, 0.004])['used'] == 'ns'
    assert M.fit(m_all, [0.0] * 5)['used'] == 'all'
    for r, branch in ((0.5e-12, 'rank'), (2e-12, 'fit')):
        m = np.array([1000.0, 300.0, 2.0, 90.0 * (1.0 + r), 0.6 * (1.0 + r)])
        f = M.fit(m, [0.0] * 5)
        assert f['branch'] == branch and 0.4 * r < f['det'] / f['lim'] < 1.1 * r
    f = M.fit([0.0] * 5, [0.0] * 5)
    assert (f['branch'], f['b1'], f['b2']) == ('empty', 0, 0)
    f = M.fit([100.0, 30.0, 0.3, 10.0, np.nan], [0.0] * 5)
    assert f['branch'] == 'fit' and np.isnan(f['b1']) and np.isnan(f['b2'])


@pytest.mark.parametrize("b1,b2", [(4.0 / 959, (6.0 / 959) ** 2), (0.6 / 959, 0.0), (40.0 / 959, -3e-4), (18.2 / 959, -1e-5),
                                   (-2e-3, 1e-4), (-2e-3, -1e-4), (0.0, 1e-4)])
def test_params_match_reference_lines(b1, b2):
    """params() against YOND_SIDD.py:356 (round 1), :438-447 (round 2) and :264-268, :284-285 (lower, upper, nsr, t) as
    O.IterDenoise / O.VST state them."""
    import yond_oracle as O
    scale = np.float64(959.0)
    for mode in (0, 1):
        reg = (np.float64(b1), np.float64(b2))
        with np.errstate(all='ignore'):
            if mode == 0:
                gain, sigma = reg[0] * scale, np.sqrt(max(reg[1], 0)) * scale            # :356
                aborted = False
            else:
                if reg[1] < 0:                                                            # :438-440
                    reg = (reg[0], reg[0] ** 2)
                gain, sigma = reg[0] * scale, np.sqrt(reg[1]) * scale                     # :442
                aborted = bool(reg[0] < 0)                                                # :445-447
            lower, upper = O.VST(0, sigma, gain=gain), O.VST(scale, sigma, gain=gain)     # :264-265
            nsr = 1 / (upper - lower)                                                     # :268
            t = np.float32(nsr * 1.03)                                                    # :284-285
        p = M.params(b1, b2, mode, 959.0, 959.0, 1.03, n_all=10.0)
        assert p['b2'] == reg[1] and p['gain'] == gain and p['sigma'] == sigma
        # (O.VST takes the root as ** 0.5: allow the one ulp between pow and sqrt, and what it does to 1 / (upper - lower))
        assert M.ulps64(p['lo'], lower) <= 1 and M.ulps64(p['hi'], upper) <= 1
        if np.isfinite(nsr):
            assert abs(p['nsr'] - nsr) <= 4 * M.U * abs(nsr) * (abs(upper) + abs(lower)) / abs(upper - lower)
            assert M.ulps32(p['t'], t) <= 1
        want = (M.ROUND_ABORTED if aborted else 0) | (0 if (gain > 0 and sigma >= 0) else M.BAD_ESTIMATE)
        assert p['flags'] == want
    assert M.params(b1, b2, 0, 959.0, 959.0, 1.03, n_all=0.0)['flags'] & M.NO_FLAT_AREA
    assert M.params(np.nan, np.nan, 1, 959.0, 959.0, 1.03)['flags'] == M.BAD_ESTIMATE


def test_knot_shape_matches_bias_knots():
    """knot_shape() against len(O.bias_knots(ub)) for every integer ub from 1 to 1600, and the capacity flag at nk and nk - 1."""
    import yond_oracle as O
    for ub in range(1, 1601):
        mx = np.float32(ub - 1.0) - np.float32(0.3)
        assert np.ceil(mx) + 1 == np.float32(ub)
        want = len(O.bias_knots(np.ceil(mx) + 1))
        (n1, n2, n3, nk), fl = M.knot_shape(mx, 1.0, 4096)
        assert (nk, fl) == (want, 0) and n1 + n2 + n3 == nk, ub
        assert M.knot_shape(mx, 1.0, want) == ((n1, n2, n3, nk), 0)
        assert M.knot_shape(mx, 1.0, want - 1) == ((0, 0, 0, 0), M.LUT_CAPACITY)
    assert M.knot_shape(np.float32(0.004), 959.0, 51) == ((0, 0, 0, 0), M.LUT_CAPACITY)             # ub = 5: 52 knots
    assert M.knot_shape(np.float32(0.004), 959.0, 52) == ((52, 0, 0, 52), 0)
    assert M.knot_shape(np.float32(-0.5), 959.0, 4096) == ((0, 0, 0, 0), M.LUT_CAPACITY)
    assert M.knot_shape(np.float32(np.nan), 959.0, 4096) == ((0, 0, 0, 0), M.LUT_CAPACITY)
    assert M.knot_shape(np.float32(-0.0), 959.0, 4096)[0][3] == len(O.bias_knots(np.float32(1.0)))


def test_float2key_round_trip():
    from yond_public_amd import pipeline as P
    tiny = np.array([1], np.uint32).view(np.float32)[0]
    big = np.finfo(np.float32).max
    vals = [-big, -1.0, -3.5e-3, -tiny, -0.0, 0.0, tiny, np.float32(1e-40), 0.4375, 1.0, big]       # ascending (the key orders -0 below +0)
    keys = []
    for v in vals:
        k = M.float2key(v)
        back = P._key2float(k)
        assert 0 < k <= 0xFFFFFFFF
        assert np.array([back], np.float32).view(np.uint32)[0] == np.array([v], np.float32).view(np.uint32)[0]
        keys.append(k)
    assert all(a < b for a, b in zip(keys[:-1], keys[1:]))
    assert M.float2key(-0.0) == 0x7FFFFFFF and M.float2key(0.0) == 0x80000000 and M.float2key(1.0) == 0xBF800000


def test_lds_doubles_edge():
    """The 48 KB allotment of the device LUT entries sits between rmax = 472 and 473 at K = 40 (pho = 6: 13 rmax + 3 doubles)."""
    assert M.lds_doubles(40.0, 64.5) == 13 * 472 + 3 <= M.BIAS_DEV_SMEM_DOUBLES < M.lds_doubles(40.0, 65.0) == 13 * 473 + 3
    assert M.lds_doubles(0.6, 0.0) == 2 * int(0.6 * 50 * (1 / 0.6) * 2 + 30 + 10 + 1) + 1 + int(0.6 * 50 * (1 / 0.6) * 2 + 30 + 10 + 1) + 2


def clipped_frame(which):
    """The two frames of tests/test_hip_chain_takeover.py: a clipped black region (A), a flat grey one (B)."""
    import yond_oracle as O
    x = O.synth_noisy(128, 192, 4.0, 6.0, 11)[0].copy()
    if which == 'A':
        x[:, :66] = 0.0
    else:
        x[:, :96] = 0.25
    return x


@pytest.mark.parametrize("which", ["A", "B"])
def test_oracle_facts_of_the_clipped_frames(which):
    """What the GPU takeover tests assume about frames A and B, checked with the oracle: A -- 10.4 % of the lap map is exactly 0,
    so the selected threshold is 0, nothing lies below it and the 25 % backup threshold (0.0298) takes over (nsel 6144,
    K ~ 4.36, sigma ~ 27.6 DN); B -- threshold and backup are both 0, every pixel is fitted (nsel 0), K ~ 18.2 and beta2 < 0."""
    import yond_oracle as O
    x = clipped_frame(which)
    rggb = O.bayer2rggb(x)
    k = 29
    mean = O.box_blur(rggb, k)
    lap = O.stdfilt(O.box_blur(rggb, k // 3 * 2 + 1), k)
    th, _ = O.get_threshold_score3(lap, mean, step=5)
    backup = O.percentile_linear(lap, [25.0])[0]
    reg, info = O.SimpleNLF(x, k=k, setting={'mode': 'self'}, full=True)
    K, b2 = reg[0] * 959.0, reg[1]
    print(f"[model] frame {which}: th {th!r}, backup {backup!r}, zeros {np.mean(lap == 0):.4f}, nsel {info['nsel']}, K {K:.4f}, beta2 {b2:.4e}")
    assert th == 0.0 and np.count_nonzero(lap < th) == 0
    if which == 'A':
        assert abs(np.mean(lap == 0) - 0.104) < 0.002
        assert abs(backup - 0.0298) < 1e-4 and info['th'] == backup and info['nsel'] == 6144
        assert abs(K - 4.36) < 0.01 and abs(np.sqrt(b2) * 959.0 - 27.6) < 0.1
    else:
        assert backup == 0.0 and info['nsel'] == 0
        assert abs(K - 18.2) < 0.1 and b2 < 0
