"""Test helper: a plain NumPy restatement of the noise-model KLD (utils/sidd_utils.py:280-304 get_histogram / cal_kld) as the kernels
of csrc/noisehist.hip and yond_public_amd/noisekld.py compute it -- the edges, the binning rule, the intensity bands, the CFA split, the
finish -- and the seeded cases of tests/golden/noisekld.npz (tools/gen_golden_noisekld.py runs the reference on them).

Binning rule (np.histogram's): bin i holds edges[i] <= r < edges[i + 1], compared in float64; the last bin also r == edges[-1]; a
residual outside the edges, NaN or infinite is in no bin (index -1).  `defect` switches in ONE deliberate error:
    'right_open_last'   the last bin does not keep r == edges[-1]
    'edges_recomputed'  the inner edges formed as -R + i * bw instead of taken from np.arange
    'n_counted'         histograms normalised by the number of counted values, not by the number of values
"""
import numpy as np

DEFECTS = ('right_open_last', 'edges_recomputed', 'n_counted')
HALF_RANGE, N_BINS = 0.1, 64


def edges(half_range=HALF_RANGE, n_bins=N_BINS, defect=None):
    R = float(half_range)
    bw = 2 * R / n_bins
    if defect == 'edges_recomputed':
        inner = np.array([-R + i * bw for i in range(n_bins + 1)], np.float64)
    else:
        inner = np.arange(-R, R + 1e-9, bw)
    return np.concatenate(([-1000.0], inner, [1000.0]), axis=0)


def bin_index(r, e, defect=None):
    """The bin of every residual (any shape, float32 or float64), -1 where it is counted nowhere."""
    rd = np.asarray(r).astype(np.float64)
    idx = np.searchsorted(e, rd, side='right').astype(np.int64) - 1           # the last i with edges[i] <= r (NaN sorts to the end)
    nbin = e.size - 1
    if defect != 'right_open_last':
        idx = np.where(rd == e[-1], nbin - 1, idx)
    ok = np.isfinite(rd) & (idx >= 0) & (idx < nbin)
    return np.where(ok, idx, -1)


def hist_counts(data, e=None, defect=None):
    """Marginal counts [nbin] (int64) of any array of values."""
    e = edges(defect=defect) if e is None else e
    idx = bin_index(np.asarray(data).reshape(-1), e, defect)
    return np.bincount(idx[idx >= 0], minlength=e.size - 1).astype(np.int64)


def band_index(clean, thresholds):
    """The number of thresholds <= clean, compared in float32; a NaN clean value is in band 0."""
    c = np.asarray(clean, np.float32)
    t = np.asarray(thresholds, np.float32).reshape(-1)
    b = np.zeros(c.shape, np.int64)
    for v in t:
        b += (v <= c)
    return b


def cfa_index(shape):
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    return (y & 1) * 2 + (x & 1)


def residual(noisy, clean):
    """ONE float32 subtraction (NumPy's lr - hr on float32 arrays)."""
    with np.errstate(invalid='ignore'):
        return np.asarray(noisy, np.float32) - np.asarray(clean, np.float32)


def counts(noisy, clean, e=None, thresholds=(), defect=None):
    """[nb][4][nbin] int64 of one Bayer frame [H][W] (or [B][nb][4][nbin] of a stack)."""
    noisy, clean = np.asarray(noisy, np.float32), np.asarray(clean, np.float32)
    if noisy.ndim == 3:
        return np.stack([counts(noisy[i], clean[i], e, thresholds, defect) for i in range(noisy.shape[0])])
    e = edges(defect=defect) if e is None else e
    nb, nbin = len(thresholds) + 1, e.size - 1
    g = bin_index(residual(noisy, clean), e, defect)
    flat = (band_index(clean, thresholds) * 4 + cfa_index(clean.shape)) * nbin + g
    return np.bincount(flat[g >= 0], minlength=nb * 4 * nbin).astype(np.int64).reshape(nb, 4, nbin)


def kld(p_counts, q_counts, n_p, n_q, defect=None):
    """(kl_fwd, kl_inv, kl_sym): the reference's expression in float64."""
    p_counts, q_counts = np.asarray(p_counts, np.float64).reshape(-1), np.asarray(q_counts, np.float64).reshape(-1)
    if defect == 'n_counted':
        n_p, n_q = p_counts.sum(), q_counts.sum()
    p, q = p_counts / n_p, q_counts / n_q
    idx = (p > 0) & (q > 0)
    p, q = p[idx], q[idx]
    logp, logq = np.log(p), np.log(q)
    fwd = np.sum(p * (logp - logq))
    inv = np.sum(q * (logq - logp))
    return float(fwd), float(inv), float((fwd + inv) / 2.0)


def kld_bound(p_counts, q_counts, n_p, n_q):
    """The derived bound on |kl_fwd - reference|: the counts are exact, so only the finish rounds -- per term one rounding each of
    log p, log q, their difference, the product and the running sum of at most 66 terms: 70 * 2^-52 * sum p (|log p| + |log q|)."""
    p, q = np.asarray(p_counts, np.float64).reshape(-1) / n_p, np.asarray(q_counts, np.float64).reshape(-1) / n_q
    idx = (p > 0) & (q > 0)
    p, q = p[idx], q[idx]
    return 70 * 2.0 ** -52 * float(np.sum(p * (np.abs(np.log(p)) + np.abs(np.log(q)))))


def cal_kld(p_data, q_data, defect=None):
    e = edges(defect=defect)
    return kld(hist_counts(p_data, e, defect), hist_counts(q_data, e, defect), np.size(p_data), np.size(q_data), defect)[0]


# ---- the seeded cases (functions of their name alone) ---------------------------------------------------------------------------------

SCALE = 959.0
PG_LEVELS = {'pg_low': (0.5, 1.0), 'pg_mid': (4.0, 6.0), 'pg_high': (16.0, 20.0)}        # (K, sigma) in DN
CASES = ('pg_low', 'pg_mid', 'pg_high', 'gain20', 'one_bin', 'edge_values', 'disjoint')
PG_SHAPE = (64, 64)


def pg_residual(rs, clean, K, sigma):
    noisy = (rs.poisson(clean.astype(np.float64) * SCALE / K) * K + rs.normal(0.0, sigma, clean.shape)) / SCALE
    return residual(noisy.astype(np.float32), clean)


def edge_values():
    """float32 values on and beside every float64 edge (np.nextafter in float32 on both sides), +-1000 and beyond, +-0, NaN, +-inf."""
    e = edges()
    v = []
    for x in e:
        f = np.float32(x)
        v += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    v += [np.float32(x) for x in (1000.0, -1000.0, 1000.5, -1000.5, 2000.0, -3.0e38, 3.0e38, 0.0, -0.0, np.nan, np.inf, -np.inf,
                                  1e-45, -1e-45, 0.05, -0.05)]
    return np.array(v, np.float32)


def make_case(name):
    """(p_data, q_data): two float32 arrays."""
    rs = np.random.RandomState(CASES.index(name) + 100)
    if name in PG_LEVELS or name == 'gain20':
        clean = rs.uniform(0.0, 1.0, PG_SHAPE).astype(np.float32)
        K, sigma = PG_LEVELS.get(name, (5.0, 3.0))
        return pg_residual(rs, clean, K, sigma), pg_residual(rs, clean, K * (1.2 if name == 'gain20' else 1.0), sigma)
    if name == 'one_bin':
        return np.full((8, 8), 0.001, np.float32), np.full((6, 10), 0.0012, np.float32)
    if name == 'edge_values':
        p = edge_values()
        q = np.concatenate([p[::2], rs.normal(0.0, 0.03, p.size - p[::2].size).astype(np.float32)])
        return p, q[rs.permutation(q.size)]
    if name == 'disjoint':
        return rs.uniform(0.011, 0.019, (4, 6)).astype(np.float32), rs.uniform(-0.019, -0.011, (4, 6)).astype(np.float32)
    raise KeyError(name)
