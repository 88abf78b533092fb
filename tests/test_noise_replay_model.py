"""CPU: the replay model of the noise generators (tests/noise_replay.py) against what it can be held to without a GPU -- the published
Random123 vectors, csrc/philox.h compiled for the CPU, and the host builds of csrc/pgnoise_sampler.h and csrc/camnoise_sampler.h, the
source the kernels run -- and the comparison of tests/test_hip_noise_replay.py against seeded defects of the contract.
Every test prints its largest host-versus-model deviation as a `[replay]` line (profiles/noise_replay_report.txt keeps one run); the
GPU tolerances are NR.TOL_FACTOR times NR.HOST_DEV, and these tests fail if a measured deviation exceeds its NR.HOST_DEV entry."""
import numpy as np
import pytest

import noise_replay as NR
import pgnoise_stats as PS
from yond_public_amd import pgnoise as PG

KEY = 20261018
CAM_KEY = 20261019
N = 2 ** 16
ACROSS = 0xFFFFFFF0                       # first index of a range that crosses 2^32: counter word 1 becomes non-zero
CAM_LAMS = (-0.26, -0.026, 0.0, 0.015, 0.102)

# Random123 kat_vectors, philox4x32 10 rounds: counter / key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_numpy_philox_known_answers():
    for ctr, key, out in KAT:
        got = tuple(int(w) for w in NR.philox4x32_10(*ctr, *key))
        assert got == out, ([hex(w) for w in got], [hex(w) for w in out])
    # vectorised: the three at once
    c = np.array([k[0] for k in KAT], np.uint64).T
    k = np.array([k[1] for k in KAT], np.uint64).T
    assert np.array_equal(np.stack(NR.philox4x32_10(*c, *k), 1), np.array([k[2] for k in KAT], np.uint64))
    assert tuple(int(w) for w in NR.philox4x32_10(0, 0, 0, 0, 0, 0, rounds=9)) != KAT[0][2]


@pytest.mark.parametrize("which", ["pgnoise", "camnoise"])
def test_host_philox_is_the_models(which):
    for ctr, key, out in KAT:
        assert tuple(int(w) for w in NR.host_philox(*([v] for v in ctr + key), which=which)[0]) == out
    rng = np.random.default_rng(1)
    args = [rng.integers(0, 2 ** 32, N, dtype=np.uint64) for _ in range(6)]
    assert np.array_equal(NR.host_philox(*args, which=which), np.stack(NR.philox4x32_10(*args), 1).astype(np.uint32))
    # the samplers' own counter layout across 2^32
    idx = np.uint64(ACROSS) + np.arange(N, dtype=np.uint64)
    lo, hi = idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32)
    assert hi.min() == 0 and hi.max() == 1
    got = NR.host_philox(lo, hi, np.zeros(N), np.full(N, NR.PG_TAG), np.full(N, KEY), np.full(N, 3), which=which)
    assert np.array_equal(got, np.stack(NR._stream(idx, 0, NR.PG_TAG, KEY, 3, {}), 1).astype(np.uint32))


def test_host_pg_normal():
    worst = 0.0
    for first, slot in ((0, 0), (ACROSS, 1)):
        _, z = NR.host_pg_draw(KEY, slot, first, N, [0.0])
        want = NR.pg_z(KEY, slot, first + np.arange(N, dtype=np.uint64))
        dev = NR.deviation(z, want)
        print(f"[replay] host pg_draw z, first {first:#x}: max |host - model| {dev:.3e} over {N}")
        worst = max(worst, dev)
    assert worst <= NR.HOST_DEV["z"], worst
    # the normal does not depend on lambda
    assert np.array_equal(NR.host_pg_draw(KEY, 0, 0, 4096, [50.0])[1], NR.host_pg_draw(KEY, 0, 0, 4096, [0.0])[1])


def test_nudged_builds_move_the_functions():
    """-DYOND_NUDGE_ULPS=k is not a no-op: z = sqrt(-2 logf(u1)) (cos, sin) grows in magnitude with logf moved away from zero, shrinks
    with it moved towards zero, by a few float32 ulps -- so a count that survives both does not hang on those bits."""
    z0 = NR.host_pg_draw(KEY, 0, 0, N, [0.0])[1].astype(np.float64)
    zp = NR.host_pg_draw(KEY, 0, 0, N, [0.0], nudge=NR.NUDGE_ULPS)[1].astype(np.float64)
    zm = NR.host_pg_draw(KEY, 0, 0, N, [0.0], nudge=-NR.NUDGE_ULPS)[1].astype(np.float64)
    assert (np.abs(zp) >= np.abs(z0)).all() and (np.abs(zm) <= np.abs(z0)).all()
    # u1 = 1 gives logf = 0, which no nudge moves; a z within 4 ulps of a power of two can round back
    assert (zp != z0).mean() > 0.9 and (zm != z0).mean() > 0.9
    print(f"[replay] nudge +-{NR.NUDGE_ULPS} ulps: z moves by at most {np.abs(zp - z0).max():.2e} / {np.abs(zm - z0).max():.2e}")
    assert max(np.abs(zp - z0).max(), np.abs(zm - z0).max()) < 1e-5


def test_host_pg_counts_over_the_ladder():
    """Per lambda of the ladder, 2^16 elements, key 20261018, slot = ladder position: the host build's count equals the model's on
    every robust element, and at most 0.1 % of the elements are fragile (lambda <= 2^23); above 2^23 every count is within 1."""
    idx = np.arange(N, dtype=np.uint64)
    bad, worst_share = [], 0.0
    for slot, lam in enumerate(PS.ladder(PG.SWITCH_LAMBDAS)):
        mask, k = NR.robust_mask(KEY, slot, 0, N, [lam])
        model = NR.pg_counts(KEY, slot, idx, np.float32(lam))
        fails = NR.compare_counts(k, model, mask, lam)
        regime = "normal" if lam > PG.SWITCH_LAMBDAS[1] else ("ptrs" if lam >= PG.SWITCH_LAMBDAS[0] else "inversion")
        frag, diff = int((~mask).sum()), int((k != model).sum())
        print(f"[replay] lambda {lam:14.6f} ({regime:9s}): fragile {frag:3d} of {N} ({frag / N:.4%}), host != model at {diff} "
              f"(max |dk| {np.abs(k - model).max():.0f})" + ("   FAIL: " + "; ".join(fails) if fails else ""))
        bad += [f"lambda {lam}: {f}" for f in fails]
        if regime != "normal":
            worst_share = max(worst_share, frag / N)
    print(f"[replay] worst fragile share below 2^23: {worst_share:.4%} (bound {NR.FRAGILE_SHARE_MAX:.1%})")
    assert worst_share <= NR.FRAGILE_SHARE_MAX
    assert not bad, bad


def test_host_pg_mixed_and_across():
    """Ladder values tiled over the elements, and the same across 2^32."""
    lams = np.array(PS.ladder(PG.SWITCH_LAMBDAS), np.float32)
    for first in (0, ACROSS):
        idx = np.uint64(first) + np.arange(N, dtype=np.uint64)
        lam = lams[np.arange(N) % lams.size]
        mask, k = NR.robust_mask(KEY, 0, first, N, lams)
        fails = NR.compare_counts(k, NR.pg_counts(KEY, 0, idx, lam), mask, lam)
        print(f"[replay] mixed ladder, first {first:#x}: fragile {int((~mask).sum())} of {N}" + ("   FAIL: " + "; ".join(fails) if fails else ""))
        assert not fails, fails


def test_host_cam_draw():
    worst = {"tl": 0.0, "zs": 0.0}
    for slot, lam in enumerate(CAM_LAMS):
        for first in (0, ACROSS):
            idx = np.uint64(first) + np.arange(N, dtype=np.uint64)
            tl, uq, zs = NR.host_cam_draw(CAM_KEY, slot, first, N, lam)
            mtl, muq, mzs = NR.cam_draw(CAM_KEY, slot, idx, lam)
            assert np.array_equal(uq.astype(np.float64), muq), lam                 # 23 bits of word 2, exact
            dt, dz = NR.deviation(tl, mtl, "rel"), NR.deviation(zs, mzs)
            print(f"[replay] host cam_draw lam {lam:7.3f}, first {first:#x}: tl max |host - model| / max(1, |model|) {dt:.3e} "
                  f"(|tl| up to {np.abs(mtl).max():.1f}), zs {dz:.3e}")
            worst = {"tl": max(worst["tl"], dt), "zs": max(worst["zs"], dz)}
            nz = mtl != 0
            assert np.array_equal(np.sign(tl[nz]), np.sign(mtl[nz])), lam         # the sign is word 1 bit 0
    assert worst["tl"] <= NR.HOST_DEV["tl"] and worst["zs"] <= NR.HOST_DEV["zs"], worst


def test_host_cam_row_normal():
    worst = 0.0
    for first in (0, ACROSS):
        z = NR.host_cam_rows(CAM_KEY, 2, first, N)
        dev = NR.deviation(z, NR.cam_row_normal(CAM_KEY, 2, np.uint64(first) + np.arange(N, dtype=np.uint64)))
        print(f"[replay] host cam_row_normal, first row {first:#x}: max |host - model| {dev:.3e}")
        worst = max(worst, dev)
    assert worst <= NR.HOST_DEV["row"], worst


def test_tolerances_are_derived():
    tol = {k: NR.TOL_FACTOR * v for k, v in NR.HOST_DEV.items()}
    print(f"[replay] GPU tolerances = {NR.TOL_FACTOR:g} x recorded host deviation: " + ", ".join(f"{k} {v:.1e}" for k, v in tol.items()))
    assert NR.TOL_FACTOR == 4.0 and max(tol.values()) < 1e-5                       # a contract defect is an O(1) error


# -- the comparison bites -----------------------------------------------------------------------------------------------------------
BITE_LAMS = (3.0, 50.0, 1000.0)
ROW_LEN = 6


@pytest.fixture(scope="module")
def host_outputs():
    """What the GPU test reads from the device, here from the host builds: never modified."""
    out = {"z": NR.host_pg_draw(KEY, 5, 0, N, [0.0])[1], "rows": NR.host_cam_rows(CAM_KEY, 5, 0, N // ROW_LEN + 1)[NR.cam_rows(N, ROW_LEN)]}
    out["counts"] = {lam: NR.robust_mask(KEY, 5, 0, N, [lam]) for lam in BITE_LAMS}
    out["cam"] = NR.host_cam_draw(CAM_KEY, 5, 0, N, -0.026)
    return out


def _battery(h, row_of=None, **d):
    """Every comparison of tests/test_hip_noise_replay.py with the model built under the seeded defects d: {check: failures}."""
    idx = np.arange(N, dtype=np.uint64)
    tol = {k: NR.TOL_FACTOR * v for k, v in NR.HOST_DEV.items()}
    res = {"pg z": NR.compare_values(h["z"], NR.pg_z(KEY, 5, idx, **d), tol["z"], what="z")}
    for lam, (mask, k) in h["counts"].items():
        res[f"pg counts {lam:g}"] = NR.compare_counts(k, NR.pg_counts(KEY, 5, idx, np.float32(lam), **d), mask, lam)
    tl, uq, zs = NR.cam_draw(CAM_KEY, 5, idx, -0.026, **d)
    res["cam tl"] = NR.compare_values(h["cam"][0], tl, tol["tl"], "rel", what="tl")
    res["cam uq"] = [] if np.array_equal(h["cam"][1].astype(np.float64), uq) else ["uq differs"]
    res["cam zs"] = NR.compare_values(h["cam"][2], zs, tol["zs"], what="zs")
    rows = NR.cam_rows(N, ROW_LEN) if row_of is None else row_of
    res["cam row"] = NR.compare_values(h["rows"], NR.cam_row_normal(CAM_KEY, 5, rows, **d), tol["row"], what="row")
    return res


def test_the_comparison_passes_without_a_defect(host_outputs):
    res = _battery(host_outputs)
    assert not any(res.values()), res


@pytest.mark.parametrize("name, defect, caught_by", [
    ("9 rounds", dict(rounds=9), ["pg z", "pg counts 3", "pg counts 50", "pg counts 1000", "cam tl", "cam uq", "cam zs", "cam row"]),
    ("swapped key words", dict(swap_key=True), ["pg z", "pg counts 3", "pg counts 50", "pg counts 1000", "cam tl", "cam uq", "cam zs", "cam row"]),
    ("tag dropped", dict(drop_tag=True), ["pg z", "pg counts 3", "pg counts 50", "pg counts 1000", "cam tl", "cam uq", "cam zs", "cam row"]),
    ("PTRS retry draw number off by one", dict(retry_shift=1), ["pg counts 50", "pg counts 1000"]),
    ("z from words (2, 3)", dict(z_words=(2, 3)), ["pg z"]),
    ("Tukey sign from word 0", dict(sign_word=0), ["cam tl"]),
    ("row counter fed the element index", dict(row_of=np.arange(N, dtype=np.uint64)), ["cam row"]),
])
def test_the_comparison_bites(host_outputs, name, defect, caught_by):
    res = _battery(host_outputs, **defect)
    caught = [k for k, v in res.items() if v]
    print(f"[replay] seeded defect '{name}': caught by {caught}")
    assert caught == caught_by, (name, res)
