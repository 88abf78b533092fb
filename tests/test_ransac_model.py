"""CPU: the NumPy model of polyfit(ransac=True) (tests/ransac_model.py) against the reference's own results
(tests/golden/ransac.npz, written by tools/gen_golden_ransac.py), and the host pieces of the product's fit that need no GPU:
the subset draw, the dynamic-trials rule and the selection loop on a trial table."""
import numpy as np
import pytest

import ransac_model as RM


@pytest.fixture(scope="module")
def fits():
    return {name: RM.fit(*RM.make_points(name)) for name in RM.CASES}


def within_fit_bound(got, ref):
    """beta1 relative <= 1e-5, beta2 absolute <= 1e-5 beta1 + 1e-9."""
    return abs(got[0] - ref[0]) <= 1e-5 * abs(ref[0]) and abs(got[1] - ref[1]) <= 1e-5 * abs(ref[0]) + 1e-9


@pytest.mark.parametrize("name", list(RM.CASES))
def test_model_reproduces_reference(golden, fits, name):
    g, r = golden("ransac"), fits[name]
    assert int(g[f"{name}_seed"]) == RM.CASES[name]["seed"]
    assert (r["n"], r["m"]) == (int(g[f"{name}_n"]), int(g[f"{name}_m"]))
    assert r["thr"].dtype == np.float32 and r["thr"] == g[f"{name}_thr"]
    assert r["n_inliers"] == int(g[f"{name}_n_inliers"]) and r["n_trials"] == int(g[f"{name}_n_trials"])
    print(f"{name}: winner {r['winner']}, |d beta1| / beta1 = {abs(r['res'][0] - g[f'{name}_res'][0]) / abs(g[f'{name}_res'][0]):.2e}, "
          f"|d beta2| = {abs(r['res'][1] - g[f'{name}_res'][1]):.2e}")
    assert within_fit_bound(r["res"], g[f"{name}_res"])


@pytest.mark.parametrize("name", [n for n, c in RM.CASES.items() if c["winner"]])
def test_winner_cases_are_admissible(fits, name):
    r = fits[name]
    print(f"{name}: margin {r['margin']}, borderline {r['borderline']} (all trials run: {r['borderline_all']})")
    assert r["margin"] > r["borderline"]


def test_cases_cover_the_paths(fits):
    assert 1 < fits["n64_early"]["n_trials"] < RM.TRIALS and fits["n64_early"]["m"] == 8          # the dynamic rule stops early
    assert fits["n3000_mask"]["masked"] and fits["n3000_mask"]["n"] < 3000                      # the non-saturation rule applies
    assert not fits["n1500_nomask"]["masked"] and fits["n1500_nomask"]["n"] == 1500             # < 1 % qualify: all kept
    x, _ = RM.make_points("n1500_nomask")
    assert 0 < np.logical_and(x > 1e-4, x < 0.8).sum() <= 0.01 * 1500
    assert fits["n5000_c20"]["n"] % 1024 and fits["n5000_c20"]["n"] > 2 * 2048                  # ragged tiles, three scoring chunks


def test_host_draw_and_rule_equal_the_model():
    from yond_public_amd import pipeline as P
    for n, m in ((300, 17), (4096, 64), (64, 8)):
        a, b = P.ransac_subsets(n, m), RM.draw_subsets(n, m)
        assert a.dtype == np.int32 and a.shape == (100, m) and np.array_equal(a, b)
        draw = P._ransac_drawer(n, m)
        assert np.array_equal(np.concatenate([draw(k) for k in P.RANSAC_BATCHES]), b) and sum(P.RANSAC_BATCHES) == P.RANSAC_TRIALS
        assert all(len(set(row)) == m for row in a.tolist()) and a.min() >= 0 and a.max() < n
    for args in ((58, 64, 8), (64, 64, 8), (3545, 4096, 64), (1, 300, 17)):
        assert P._ransac_dynamic_max_trials(*args) == RM.dynamic_max_trials(*args)
    assert P._ransac_dynamic_max_trials(1, 300, 17) == float("inf") and P._ransac_dynamic_max_trials(64, 64, 8) == 1


def test_selection_loop_on_a_table(fits):
    """pipeline._ransac_select on a table built from the model's own lines: the same winner, count and trials run."""
    from yond_public_amd import pipeline as P
    for name in ("n300_c30", "n64_early"):
        r = fits[name]
        x, y, _ = RM.nonsat(*RM.make_points(name))
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        tab = np.zeros((RM.TRIALS, 10))
        for t in range(RM.TRIALS):
            a, b = r["lines"][t]
            res = np.abs(yd - (a * xd + b))
            i = res <= np.float64(r["thr"])
            tab[t] = [a, b, i.sum(), xd[i].sum(), yd[i].sum(), (xd[i] ** 2).sum(), (xd[i] * yd[i]).sum(), (yd[i] ** 2).sum(), (res[i] ** 2).sum(),
                      r["thr"]]
        assert P._ransac_select(tab, r["n"], r["m"]) == (r["winner"], r["n_inliers"], r["n_trials"])
        # on the first rows only (the product computes the table in batches): undecided until the loop's last trial is there
        for rows in np.cumsum(P.RANSAC_BATCHES):
            got = P._ransac_select(tab[:rows], r["n"], r["m"], total=RM.TRIALS)
            assert got == ((r["winner"], r["n_inliers"], r["n_trials"]) if rows >= r["n_trials"] else None)
        reg = P._fit_from_moments(tab[r["winner"], 2:7], tab[r["winner"], 2:7])
        assert within_fit_bound(reg, r["res"])
    # ties: equal counts keep the trial with the higher R^2, and a lower-scoring later tie is skipped
    tab = np.zeros((3, 10))
    tab[:, 2] = 10
    tab[:, 4], tab[:, 7] = 10.0, 20.0                              # Sy, Syy: variance sum 10
    tab[:, 8] = [2.0, 1.0, 1.5]                                    # Srr
    assert P._ransac_select(tab, 1000, 31)[0] == 1
    with pytest.raises(P.L.YondHipError):
        P._ransac_select(np.zeros((4, 10)), 100, 10)


def test_est_fit_key():
    from yond_public_amd import pipeline as P
    assert P.est_fit_of({}) == 'lsq' and P.est_fit_of({'est_fit': 'ransac'}) == 'ransac'
    with pytest.raises(P.L.YondHipError):
        P.est_fit_of({'est_fit': 'huber'})
    assert not P.stream_applies({'full_dn': True, 'iter': 'once', 'est_fit': 'ransac'}) and P.stream_applies({'full_dn': True, 'iter': 'once'})
