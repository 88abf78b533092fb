"""CPU: the NumPy model of the noise-model KLD (tests/noisekld_model.py) against the reference's outputs in tests/golden/noisekld.npz
(tools/gen_golden_noisekld.py: utils/sidd_utils.py:280-304 run on the seeded cases): counts equal to the reference's hist * n exactly,
the KLD within the derived bound of the finish's roundings, every single-defect variant of the model breaking at least one case; and
the host side of yond_public_amd/noisekld.py (edges, thresholds, finish, argument parsing), which needs no GPU."""
import numpy as np
import pytest

import noisekld_model as M


@pytest.fixture(scope="module")
def fx(golden):
    return golden("noisekld")


def test_fixture_is_the_seeded_cases(fx):
    assert list(fx["names"]) == list(M.CASES)
    assert fx["edges"].tobytes() == M.edges().tobytes() and fx["edges"].shape == (67,)
    for name in M.CASES:
        p, q = M.make_case(name)
        assert fx[f"{name}_p"].tobytes() == p.tobytes() and fx[f"{name}_q"].tobytes() == q.tobytes()
        assert fx[f"{name}_hist_p"].shape == (66,) and fx[f"{name}_hist_p"].dtype == np.float64


def test_edges_are_not_round_numbers(fx):
    e = fx["edges"]
    assert e[0] == -1000.0 and e[-1] == 1000.0 and e[1] == -0.1
    assert e[33] != 0.0 and abs(e[33]) < 1e-16                       # the middle inner edge (8.3e-17)
    assert e[-2] > 0.1 and e[-2] == 0.10000000000000017              # the last inner edge
    bad = M.edges(defect='edges_recomputed')
    assert bad[33] == 0.0 and not np.array_equal(bad, e)


def test_cases_hold_what_they_must(fx):
    e = fx["edges"]
    p = fx["edge_values_p"]
    for x in e:                                                     # on and beside every edge, in float32
        f = np.float32(x)
        for v in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
            assert (p == v).any()
    assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any() and (p > 1000).any() and (p < -1000).any()
    assert (p == 0).sum() >= 2 and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
    hp, hq = fx["one_bin_hist_p"], fx["one_bin_hist_q"]
    assert (hp > 0).sum() == 1 and (hq > 0).sum() == 1 and hp.max() == 1.0 and np.argmax(hp) == np.argmax(hq)
    assert not ((fx["disjoint_hist_p"] > 0) & (fx["disjoint_hist_q"] > 0)).any() and fx["disjoint_kld"] == 0.0


@pytest.mark.parametrize("name", M.CASES)
def test_model_counts_and_kld(fx, name):
    p, q = fx[f"{name}_p"], fx[f"{name}_q"]
    cp, cq = M.hist_counts(p), M.hist_counts(q)
    assert np.array_equal(cp, np.rint(fx[f"{name}_hist_p"] * p.size)) and np.array_equal(cp / p.size, fx[f"{name}_hist_p"])
    assert np.array_equal(cq, np.rint(fx[f"{name}_hist_q"] * q.size)) and np.array_equal(cq / q.size, fx[f"{name}_hist_q"])
    ref, got, bound = float(fx[f"{name}_kld"]), M.cal_kld(p, q), M.kld_bound(cp, cq, p.size, q.size)
    print(f"[noisekld] {name}: model {got:.17g}, reference {ref:.17g}, |delta| {abs(got - ref):.3e}, bound {bound:.3e}")
    assert abs(got - ref) <= bound
    fwd, inv, sym = M.kld(cp, cq, p.size, q.size)
    assert fwd == got and sym == (fwd + inv) / 2.0


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_defects_break_a_case(fx, defect):
    broken = []
    for name in M.CASES:
        p, q = fx[f"{name}_p"], fx[f"{name}_q"]
        cp, cq = M.hist_counts(p), M.hist_counts(q)
        e = M.edges(defect=defect)
        same = np.array_equal(M.hist_counts(p, e, defect), cp) and np.array_equal(M.hist_counts(q, e, defect), cq)
        if not same or not abs(M.cal_kld(p, q, defect=defect) - float(fx[f"{name}_kld"])) <= M.kld_bound(cp, cq, p.size, q.size):
            broken.append(name)
    print(f"[noisekld] defect {defect}: breaks {broken}")
    assert broken


def test_frame_counts_split_the_marginal():
    rs = np.random.RandomState(5)
    clean = rs.uniform(0, 1, (6, 10)).astype(np.float32)
    clean[0, 0], clean[1, 1], clean[2, 3] = 0.25, np.nan, 0.5
    noisy = (clean + rs.normal(0, 0.05, clean.shape)).astype(np.float32)
    t = np.array([0.25, 0.5, 0.75], np.float32)
    c = M.counts(noisy, clean, thresholds=t)
    assert c.shape == (4, 4, 66)
    assert np.array_equal(c.sum((0, 1)), M.hist_counts(M.residual(noisy, clean)))
    assert np.array_equal(c.sum(0), M.counts(noisy, clean)[0])
    assert M.band_index(clean, t)[0, 0] == 1 and M.band_index(clean, t)[2, 3] == 2 and M.band_index(clean, t)[1, 1] == 0   # on a threshold: the band above; NaN: band 0
    assert M.cfa_index((2, 2)).tolist() == [[0, 1], [2, 3]]
    assert c.sum() == clean.size - 1                                                  # the NaN pixel's residual is counted nowhere


def test_library_host_side(fx):
    """What yond_public_amd/noisekld.py does on the host: the edges, the thresholds, the finish, the switch's argument."""
    import argparse
    from yond_public_amd import noisekld as NK
    assert NK.kld_edges().tobytes() == fx["edges"].tobytes()
    assert NK.kld_edges(0.05, 32).shape == (35,) and NK.kld_edges(0.05, 32)[1] == -0.05
    assert NK.band_thresholds(None).size == 0 and NK.band_thresholds(0).size == 0 and NK.band_thresholds(1).size == 0
    assert NK.band_thresholds(4).tolist() == [0.25, 0.5, 0.75] and NK.band_thresholds(4).dtype == np.float32
    assert NK.band_thresholds(3).tobytes() == np.linspace(0, 1, 4)[1:-1].astype(np.float32).tobytes()
    with pytest.raises(ValueError):
        NK.band_thresholds([0.5, 0.25])
    for name in M.CASES:
        p, q = fx[f"{name}_p"], fx[f"{name}_q"]
        cp, cq = M.hist_counts(p), M.hist_counts(q)
        got = NK.kld_from_counts(cp, cq, p.size, q.size)
        assert got == M.kld(cp, cq, p.size, q.size)
        assert abs(got[0] - float(fx[f"{name}_kld"])) <= M.kld_bound(cp, cq, p.size, q.size)
    assert NK.noise_kld_arg('est') == ('est',) and NK.noise_kld_arg('4,6') == ('pg', 4.0, 6.0)
    kind, spec = NK.noise_kld_arg('cam:code=p,K=0.22,sigGs=1.26')
    assert kind == 'cam' and spec['code'] == 'p'
    with pytest.raises(argparse.ArgumentTypeError):
        NK.noise_kld_arg('4')
    assert NK.noise_kld_of({}) == (None, 0.1, 0)
    assert NK.noise_kld_of({'noise_kld': '8,6', 'noise_kld_range': 0.05, 'noise_kld_bands': 4}) == (('pg', 8.0, 6.0), 0.05, 4)
    ns = argparse.Namespace(noise_kld=('est',), kld_range=None, kld_bands=2)
    assert NK.noise_kld_of({'noise_kld': '8,6', 'noise_kld_range': 0.05}, ns) == (('est',), 0.05, 2)
    # the report's marginal is the integer sum of the split counts
    rs = np.random.RandomState(2)
    clean = rs.uniform(0, 1, (8, 12)).astype(np.float32)
    a = M.counts((clean + rs.normal(0, 0.02, clean.shape)).astype(np.float32), clean, thresholds=NK.band_thresholds(2))
    b = M.counts((clean + rs.normal(0, 0.03, clean.shape)).astype(np.float32), clean, thresholds=NK.band_thresholds(2))
    rep = NK.kld_report(a, b, clean.size)
    assert rep['kld'] == M.kld(a.sum((0, 1)), b.sum((0, 1)), clean.size, clean.size)[0]
    assert len(rep['kld_cfa']) == 4 and len(rep['kld_bands']) == 2
    assert rep['kld_cfa'][3] == M.kld(a[:, 3].sum(0), b[:, 3].sum(0), clean.size / 4, clean.size / 4)[0]
