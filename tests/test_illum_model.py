"""CPU: the float64 model of the illuminance correction (tests/illum_model.py) against the reference's outputs in
tests/golden/illum.npz (tools/gen_golden_illum.py: data_process/__init__.py:140-171 run on the seeded cases), at the guaranteed bound
of a float32 sum of n non-negative terms, and every single-defect variant of the model outside that bound."""
import numpy as np
import pytest

import illum_model as M


@pytest.fixture(scope="module")
def fx(golden):
    return golden("illum")


def test_fixture_is_the_seeded_cases(fx):
    assert list(fx["names"]) == list(M.CASES)
    for name in M.CASES:
        pred, source = M.make_case(name)
        assert fx[f"{name}_pred"].tobytes() == pred.tobytes() and fx[f"{name}_source"].tobytes() == source.tobytes()
        assert fx[f"{name}_pred"].shape == M.CASES[name][0] and fx[f"{name}_out"].shape == M.CASES[name][0]
        assert fx[f"{name}_out"].dtype == np.float32 and fx[f"{name}_gain_dist"].shape == (pred.shape[0],)


def test_case3_holds_what_it_must(fx):
    pred, source = fx["c3_62x130_pred"], fx["c3_62x130_source"]
    sat = float((source == 1).mean())
    assert 0.05 <= sat <= 0.10
    assert (source == np.nextafter(np.float32(1), np.float32(0))).any() and (source > 1).any()
    far = float(((pred >= 3) | (pred <= -2)).mean())
    assert 0.02 <= far <= 0.05
    gain = M.gain_of(M.sums(pred[0], source[0])[4])
    assert abs(float(gain) - 1) > 0.1                                   # a true gain away from 1


@pytest.mark.parametrize("name", list(M.CASES))
def test_model_within_the_float32_sum_bound(fx, name):
    pred, source, ref = fx[f"{name}_pred"], fx[f"{name}_source"], fx[f"{name}_out"]
    for i in range(pred.shape[0]):
        s = source[i if source.shape[0] != 1 else 0]
        out, sums = M.correct(pred[i], s)
        n_incl = int(sums[4, 2])
        assert n_incl == int((s != 1).sum())
        d = M.assert_within(ref[i], out, M.out_bound(n_incl), f"{name}[{i}]")
        print(f"[illum] {name}[{i}]: n_incl={n_incl}, model - reference {d:.3e} relative, bound {M.out_bound(n_incl):.3e}, "
              f"recorded gain distance {fx[f'{name}_gain_dist'][i]:.3e}")
        assert fx[f"{name}_gain_dist"][i] <= M.out_bound(n_incl)
    assert np.array_equal(M.forward(pred, source), np.stack([M.correct(pred[i], source[i if source.shape[0] != 1 else 0])[0]
                                                             for i in range(pred.shape[0])]))


@pytest.mark.parametrize("defect", [d for d in M.DEFECTS if d != 'groups_transposed'])
@pytest.mark.parametrize("name", list(M.CASES))
def test_defects_leave_the_bound(fx, name, defect):
    assert M.exercises(name, defect)
    pred, source, ref = fx[f"{name}_pred"], fx[f"{name}_source"], fx[f"{name}_out"]
    M.assert_outside(ref, M.forward(pred, source, defect=defect), pred, source, f"{name} {defect}")


def _cfa_frame(layout):
    """A frame whose four groups carry different black-level offsets (groups 1 and 2 far apart: a transposition shows)."""
    rng = np.random.RandomState(21)
    shape = (6, 10) if layout == M.BAYER else (15, 4)
    source = rng.uniform(0.05, 0.9, shape).astype(np.float32)
    source.reshape(-1)[::7] = 1.0
    g = M.groups(shape, layout)
    pred = (source / np.float32(1.25) + np.array([0.0, 0.05, -0.03, 0.01], np.float32)[g] + rng.normal(0, 0.01, shape)).astype(np.float32)
    pred.reshape(-1)[3::11] = 3.0
    return pred, source


@pytest.mark.parametrize("layout", [M.BAYER, M.PACKED4])
def test_layouts_and_cfa_mode(layout):
    pred, source = _cfa_frame(layout)
    s = M.sums(pred, source, layout)
    flat = M.sums(pred, source, M.FLAT)
    assert s[4].tolist() == flat[4].tolist() == flat[0].tolist() and (flat[1:4] == 0).all()
    assert s[:4, 2].sum() == s[4, 2] == (source != 1).sum()
    np.testing.assert_allclose(s[:4].sum(axis=0), s[4], rtol=4 * 2.0 ** -53)
    # group k's sums are the FLAT sums of its elements alone
    g = M.groups(pred.shape, layout)
    for k in range(4):
        assert M.sums(pred[g == k], source[g == k])[4].tolist() == s[k].tolist()
    if layout == M.BAYER:
        assert g[0, 1] == 1 and g[1, 0] == 2 and g[1, 1] == 3
    else:
        assert g[0].tolist() == [0, 1, 2, 3]
    frame = M.apply(pred, s, 'frame', layout=layout)
    cfa = M.apply(pred, s, 'cfa', layout=layout)
    assert np.array_equal(frame, (M.gain_of(s[4]) * M.clamp01(pred)).astype(np.float32))
    for k in range(4):
        assert np.array_equal(cfa[g == k], (M.gain_of(s[k]) * M.clamp01(pred)[g == k]).astype(np.float32))
    # per-group gains fit their own offsets: the squared error over the included set does not grow
    m = source != 1
    assert ((cfa - source)[m].astype(np.float64) ** 2).sum() <= ((frame - source)[m].astype(np.float64) ** 2).sum()
    # the transposed groups are another function, in the sums and in the output
    st = M.sums(pred, source, layout, defect='groups_transposed')
    assert st[1].tolist() == s[2].tolist() and st[2].tolist() == s[1].tolist() and st[1].tolist() != s[1].tolist()
    bad = M.apply(pred, s, 'cfa', layout=layout, defect='groups_transposed')
    assert M.rel_dist(bad, cfa) > M.out_bound(int(s[4, 2]))
    # clip: nothing above 1, the rest untouched
    big = np.array([[2.0, 0.5, 0.0]] * 5, np.float64)
    clipped = M.apply(pred, big, 'frame', clip=True, layout=layout)
    plain = M.apply(pred, big, 'frame', layout=layout)
    assert clipped.max() == 1.0 and (plain > 1).any() and np.array_equal(clipped[plain <= 1], plain[plain <= 1])


def test_special_values():
    one, below, above = np.float32(1), np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    pred = np.array([0.5, 0.5, 0.5, 0.25], np.float32)
    s = M.sums(pred, np.array([one, below, above, 0.5], np.float32))
    assert s[4, 2] == 3 and s[4, 1] == 0.25 + 0.25 + 0.0625
    # every target saturated: count 0, 0 / 0
    out, s = M.correct(pred, np.ones(4, np.float32))
    assert s[4].tolist() == [0.0, 0.0, 0.0] and np.isnan(M.gain_of(s[4])) and np.isnan(out).all()
    # a NaN prediction: its sums and its pixel are NaN, also through the clip; under a saturated target it is left out
    pn = np.array([np.nan, 0.5, 0.5, 0.25], np.float32)
    out, s = M.correct(pn, np.array([0.5, 0.5, 0.5, 0.5], np.float32), clip=True)
    assert np.isnan(s[4, :2]).all() and s[4, 2] == 4 and np.isnan(out).all()
    out, s = M.correct(pn, np.array([1.0, 0.5, 0.5, 0.5], np.float32), clip=True)
    assert not np.isnan(s).any() and np.isnan(out[0]) and not np.isnan(out[1:]).any()
    assert np.isnan(M.clamp01(np.float32(np.nan)))
