"""CPU: the host half of the camera-noise path (yond_public_amd/camnoise.py) -- the per-camera parameter prior against the reference's
draws (tests/golden/camnoise.npz, tools/gen_golden_camnoise.py), the Tukey-lambda variance, the effective Poisson-Gaussian level, the
item layout, every refusal of plan / camera_noise_arg / the C ABI, the kernel's resource report -- and the sampler itself: the source
the kernel runs (csrc/camnoise_sampler.h) compiled for the CPU, its Tukey-lambda variates against scipy.stats.tukeylambda."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import camnoise_stats as CS
from yond_public_amd import camnoise as CN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 20261019


def _tables(g):
    """{camera type: parameters} as the golden file carries them; CRVD with its ISO points."""
    t = {}
    for cam in ("SonyA7S2_lowISO", "SonyA7S2_highISO", "CRVD"):
        t[cam] = {str(k): float(v) for k, v in zip(g[f"table_{cam}_names"], g[f"table_{cam}_values"])}
        for k in ("wp", "bl"):
            t[cam][k] = int(t[cam][k])
    t["CRVD"].update(K_points=g["CRVD_K_points"], log_sigGs_points=g["CRVD_log_sigGs_points"])
    return t


def test_prior_draws_are_the_references(golden):
    g = golden("camnoise")
    fields = [str(f) for f in g["fields"]]
    assert fields == ["K", "sigTL", "sigR", "sigGs", "bias", "lam", "q", "ratio", "wp", "bl"] and len(g["seeds"]) == 8
    tables = _tables(g)
    lams, points = set(), set()
    for cam in ("SonyA7S2", "CRVD"):
        for ln in (False, True):
            for s in g["seeds"]:
                p = CN.sample_camera_params(np.random.RandomState(int(s)), tables, cam, ln_ratio=ln)
                assert sorted(p) == sorted(fields)
                got, want = np.array([p[f] for f in fields], np.float64), g[f"params_{cam}_{int(ln)}_{int(s)}"]
                assert np.array_equal(got, want), (cam, ln, int(s), got, want)
                (lams if cam == "SonyA7S2" else points).add(float(p["lam"] if cam == "SonyA7S2" else p["K"]))
                assert (1 <= p["ratio"] * 1.0101 and p["ratio"] <= math.exp(1 if cam == "CRVD" else 5)) if ln else 100 <= p["ratio"] <= 300
    assert lams == {-0.026, -0.025} and len(points) >= 3          # both ISO branches of the dual-ISO camera, several ISO points
    # one camera's parameters passed as they are: the low-ISO branch without the randint
    rs = np.random.RandomState(3)
    one = CN.sample_camera_params(rs, tables["SonyA7S2_lowISO"])
    assert one["lam"] == -0.026 and math.exp(-1.67214) <= one["K"] <= math.exp(0.42228) and one["bias"] != 1.0
    assert CN.sample_camera_params(rs, tables["SonyA7S2_lowISO"])["K"] != one["K"]


def test_table_without_uread_gives_bias_one(golden):
    tables = _tables(golden("camnoise"))
    bare = {k: v for k, v in tables["SonyA7S2_lowISO"].items() if not k.startswith("uRead")}
    rs_a, rs_b = np.random.RandomState(5), np.random.RandomState(5)
    p, full = CN.sample_camera_params(rs_a, bare), CN.sample_camera_params(rs_b, tables["SonyA7S2_lowISO"])
    assert p["bias"] == 1.0 and full["bias"] != 1.0
    assert (p["K"], p["sigTL"], p["sigR"], p["sigGs"]) == (full["K"], full["sigTL"], full["sigR"], full["sigGs"])
    assert CN.sample_camera_params(np.random.RandomState(0), tables, "CRVD")["bias"] == 1.0        # the reference's own case


def test_tukeylambda_variance():
    from scipy import stats
    for lam in CS.LAMS:
        got, want = CN.tukeylambda_variance(lam), float(stats.tukeylambda.var(lam))
        assert abs(got - want) <= 1e-12 * want, (lam, got, want)
    assert CN.tukeylambda_variance(0) == math.pi ** 2 / 3
    assert CN.tukeylambda_variance(-0.5) == math.inf and CN.tukeylambda_variance(-0.7) == math.inf
    assert CN.tukeylambda_variance(1.0) == pytest.approx(1 / 3, rel=1e-14)             # lam 1: uniform on (-1, 1)
    assert CN.tukeylambda_variance(1e-200) == pytest.approx(math.pi ** 2 / 3, rel=1e-14)
    for lam in (0.25, -0.25):                                                          # the two branches meet
        assert CN.tukeylambda_variance(lam) == pytest.approx(CN.tukeylambda_variance(lam * (1 + 1e-9)), rel=1e-7)


def test_effective_pg_by_hand():
    p = dict(K=0.25, sigTL=0.5, sigGs=2.0, sigR=1.5, lam=0.0, bias=[1.0, 2.0, 3.0, 4.0])
    assert CN.effective_pg(p, "p") == (0.25, 2.0)
    assert CN.effective_pg(p, "P") == (0.25, 2.0) and CN.effective_pg(p, "d") == (0.25, 2.0)
    assert CN.effective_pg(p, "pr") == (0.25, 2.5)                                     # sqrt(4 + 2.25)
    K, s = CN.effective_pg(p, "prq")
    assert K == 0.25 and s == pytest.approx(math.sqrt(6.25 + 1 / 12), rel=1e-15)
    K, s = CN.effective_pg(p, "pg")                                                    # logistic of scale 0.5: variance 0.25 pi^2 / 3
    assert s == pytest.approx(0.5 * math.pi / math.sqrt(3), rel=1e-15)
    K, s = CN.effective_pg(p, "pgrq", mfm=4)                                           # shot / 2, read and row variance / 4, q as it is
    assert K == 0.125 and s == pytest.approx(math.sqrt((0.25 * math.pi ** 2 / 3 + 2.25) / 4 + 1 / 12), rel=1e-15)
    assert CN.effective_pg(p, "pgrqdb") == (0.25, 0.0)                                 # black: shot only
    assert list(CN.dark_bias(p, "pd")) == [1.0, 2.0, 3.0, 4.0] and list(CN.dark_bias(p, "p")) == [0.0] * 4
    assert list(CN.dark_bias(p, "pdb")) == [0.0] * 4 and list(CN.dark_bias(dict(p, bias=0.5), "d")) == [0.5] * 4
    for bad in ("", "px", "pg r"):
        with pytest.raises(ValueError, match="noise code"):
            CN.effective_pg(p, bad)
    with pytest.raises(ValueError, match="MultiFrameMean"):
        CN.effective_pg(p, "p", mfm=0)


def test_item_layout_matches_the_header():
    assert CN.ITEM_DTYPE.itemsize == 64
    offs = [(n, CN.ITEM_DTYPE.fields[n][1]) for n in CN.ITEM_DTYPE.names]
    assert offs == [("beta1", 0), ("sig_read", 4), ("lam", 8), ("sig_row", 12), ("q_step", 16), ("bias", 20), ("exposure", 36), ("mfm", 40),
                    ("clip_lo", 44), ("clip_hi", 48), ("flags", 52), ("key", 56), ("slot", 60)]
    h = open(os.path.join(ROOT, "include", "yond_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} YondCamItem;", h)
    decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for part in decl.split(";") if part.strip() for n in part.strip().split(None, 1)[1].split(",")]
    assert names == ["beta1", "sig_read", "lam", "sig_row", "q_step", "bias", "exposure", "mfm", "clip_lo", "clip_hi", "flags", "key", "slot"]
    assert "float bias[4]" in decl and "uint32_t flags" in decl and "uint32_t key, slot" in decl
    flags = {n: int(v) for n, v in re.findall(r"#define YOND_CAM_(\w+) (\d+)u", h)}
    assert flags == {"POISSON": CN.FLAG_POISSON, "TUKEY": CN.FLAG_TUKEY, "CLIP": CN.FLAG_CLIP}
    it = CN.plan(2, [1.0, 2.0], 8.0, 959.0, 77, [5, 6], lam=-0.026, sig_row=0.5, q_step=1.0, bias=[1, 2, 3, 4], exposure=0.01, mfm=4,
                 clip=(-0.0625, 1.0), tukey=True)
    f4 = lambda *v: np.array(v, "<f4").tobytes()
    want = (f4(2.0 / 959, 8.0 / 959, -0.026, 0.5 / 959, 1.0 / 959, 1 / 959, 2 / 959, 3 / 959, 4 / 959, 0.01, 2.0, -0.0625, 1.0)
            + np.array([7, 77, 6], "<u4").tobytes())
    assert it.tobytes()[64:] == want
    assert CN.plan(1, 1.0, 0.0, 1.0, 0, [0], poisson=False)["flags"][0] == 0


def test_plan_refusals():
    ok = dict(K=1.0, sig_read=1.0, scale=959.0, key=0, slots=[0, 1, 2])
    CN.plan(3, **ok)
    for bad in (dict(K=[1.0, 2.0]), dict(K=float("nan")), dict(sig_read=-1.0), dict(sig_read=float("inf")), dict(sig_row=-0.5),
                dict(sig_row=float("nan")), dict(q_step=-1.0), dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=float("inf")),
                dict(scale=0.0), dict(lam=-0.5), dict(lam=-0.7), dict(lam=float("nan")), dict(lam=float("inf")), dict(mfm=0),
                dict(mfm=float("nan")), dict(bias=[1.0, 2.0]), dict(bias=[0, 0, 0, float("inf")]), dict(clip=(1.0, 0.0)),
                dict(clip=(float("nan"), 1.0))):
        with pytest.raises(ValueError):
            CN.plan(3, **dict(ok, **bad))
    # the reference's letters
    p = dict(K=2.0, sigTL=0.5, sigGs=3.0, sigR=0.25, lam=0.102, bias=[1, 2, 3, 4], wp=1023, bl=64)
    it = CN.items_for(p, "PGRQD", 959.0, 1, [0], ratio=100, mfm=4, clip="sensor")[0]
    assert it["flags"] == 7 and it["sig_read"] == np.float32(0.5 / 959) and it["lam"] == np.float32(0.102) and it["mfm"] == 2.0
    assert it["q_step"] == np.float32(1 / 959) and it["sig_row"] == np.float32(0.25 / 959) and it["exposure"] == np.float32(0.01)
    assert (it["clip_lo"], it["clip_hi"]) == (np.float32(-64 / 1023), 1.0)             # bl / wp, the reference's quirk
    it = CN.items_for(p, "r", 959.0, 1, [0], clip="01")[0]
    assert it["flags"] == 4 and it["sig_read"] == np.float32(3.0 / 959) and it["lam"] == 0 and (it["bias"] == 0).all()
    it = CN.items_for(p, "pgrqdb", 959.0, 1, [0])[0]
    assert it["flags"] == 1 and it["sig_read"] == 0 and it["sig_row"] == 0 and it["q_step"] == 0 and (it["bias"] == 0).all()
    with pytest.raises(ValueError, match="clip"):
        CN.items_for(p, "p", 959.0, 1, [0], clip="sensor01")
    with pytest.raises(ValueError, match="parameter sets"):
        CN.items_for([p, p], "p", 959.0, 1, [0])


def test_camera_noise_arg():
    import argparse
    s = CN.camera_noise_arg("code=pgrq,K=0.22,sigTL=0.76,sigGs=1.26,sigR=0.23,lam=-0.026")
    assert (s["code"], s["K"], s["sigTL"], s["sigGs"], s["sigR"], s["lam"], s["mfm"], s["clip"]) == ("pgrq", 0.22, 0.76, 1.26, 0.23, -0.026, 1.0,
                                                                                                    None)
    assert list(s["bias"]) == [0.0] * 4
    s = CN.camera_noise_arg("code=PD, K=4, bias=1/-2/3/0.5, mfm=4, clip=sensor")
    assert (s["code"], s["K"], s["sigGs"], s["mfm"], s["clip"]) == ("pd", 4.0, 0.0, 4.0, "sensor") and list(s["bias"]) == [1.0, -2.0, 3.0, 0.5]
    assert list(CN.camera_noise_arg("code=d,K=1,bias=0.25")["bias"]) == [0.25] * 4
    assert CN.camera_noise_arg("code=p,K=1,clip=none")["clip"] is None and CN.camera_noise_arg("code=p,K=1,clip=01")["clip"] == "01"
    for bad in ("", "pgrq", "code=pgrq", "K=1", "code=px,K=1", "code=p,K=0", "code=p,K=-1", "code=p,K=nan", "code=p,K=one", "code=p,K=1,K=2",
                "code=p,K=1,sigGs=-1", "code=p,K=1,sigGs=inf", "code=pg,K=1,sigTL=1", "code=pg,K=1,lam=0.1", "code=pg,K=1,sigTL=1,lam=-0.5",
                "code=pr,K=1", "code=pd,K=1", "code=pd,K=1,bias=1/2", "code=pd,K=1,bias=1/2/3/x", "code=p,K=1,mfm=0", "code=p,K=1,clip=yes",
                "code=p,K=1,gain=2", "code=p,K=1,", "code=p,K="):
        with pytest.raises(argparse.ArgumentTypeError):
            CN.camera_noise_arg(bad)


def test_parsers_and_drivers_take_camera_noise(capsys):
    from yond_public_amd.YOND_SIDD import YOND_SIDD, YONDParser
    a = YONDParser().parse(["--camera-noise", "code=pgrq,K=0.22,sigTL=0.76,sigGs=1.26,sigR=0.23,lam=-0.026"])
    assert a.camera_noise["code"] == "pgrq" and a.synth_noise is None
    assert YONDParser().parse([]).camera_noise is None
    with pytest.raises(SystemExit):
        YONDParser().parse(["--camera-noise", "code=pg,K=1"])
    assert "--camera-noise" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="--camera-noise belongs to the full-frame drivers"):
        YOND_SIDD(["--camera-noise", "code=p,K=4,sigGs=6"])


def test_abi_argument_checks_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from yond_public_amd import _lib
    f = _lib.load().yond_camera_noise_f32
    d = ctypes.c_void_p(16)                       # never dereferenced: every call below is refused before a launch
    ok = dict(clean=d, noisy=d, n=4 * 6 * 8, B=1, items=d, layout=0, row_len=8, stream=None)

    def call(**kw):
        return f(*dict(ok, **kw).values())
    for name in ("clean", "noisy", "items"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(B=-3) == -1 and call(B=65536) == -1
    assert call(n=0) == -1
    assert call(clean=ctypes.c_void_p(18)) == -1 and call(noisy=ctypes.c_void_p(17)) == -1     # not 4-byte aligned
    assert call(layout=2) == -1 and call(layout=-1) == -1
    assert call(row_len=-1) == -1
    assert call(row_len=7) == -1 and call(row_len=5) == -1                                     # 48 per plane
    assert call(n=4 * 6 * 8 + 2, row_len=2) == -1                                              # layout 0 needs four planes
    assert call(layout=1, row_len=7) == -1 and call(layout=1, n=35, row_len=8) == -1
    assert call(layout=1, n=2 ** 32, row_len=8) == -1                                          # rows and columns are 32-bit


def test_kernel_has_no_vgpr_spills():
    from yond_public_amd import build as B
    B.build_lib(verbose=False)
    rep = [r for r in B.resource_report() if "cam_noise" in r["name"]]
    assert len(rep) == 1, (rep, len(B.resource_report()))
    assert (rep[0]["vgpr_spill"], rep[0]["scratch"], rep[0]["lds"]) == (0, 0, 0), rep
    assert rep[0]["vgprs"] <= 128, rep                                                         # four waves per SIMD at least


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def host_sampler(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("camnoise") / "libcamnoise_host.so")
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "camnoise_host_sampler.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.cam_host_draw.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_float, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p]
    lib.cam_host_rows.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_void_p]
    lib.cam_host_tail.argtypes = [ctypes.c_float, ctypes.c_void_p]
    lib.cam_host_draw.restype = lib.cam_host_rows.restype = lib.cam_host_tail.restype = None
    return lib


def test_sampler_on_the_cpu(host_sampler):
    """2^20 draws per shape of csrc/camnoise_sampler.h built for the CPU: the Tukey-lambda variate against scipy.stats.tukeylambda
    (chi-square on 64 equiprobable bins, quartiles, mean, and the variance where the law has a fourth moment), the quantisation uniform
    and the two normals by their moments, and that the three draws of one element are uncorrelated."""
    n, bad = 2 ** 20, []
    for slot, lam in enumerate(CS.LAMS):
        tl, uq, zs = (np.empty(n, np.float32) for _ in range(3))
        host_sampler.cam_host_draw(KEY, slot, 0, n, lam, tl.ctypes.data, uq.ctypes.data, zs.ctypes.data)
        row, fails = CS.check_tukeylambda(tl, float(np.float32(lam)))
        print(row + ("   FAIL: " + "; ".join(fails) if fails else ""))
        bad += [f"lam {lam}: {f}" for f in fails]
        assert np.abs(uq).max() < 0.5
        bad += CS.check_moments(uq, 0.0, 1 / 12, 1 / 80, f"lam {lam}: quantisation uniform")
        bad += CS.check_moments(zs, 0.0, 1.0, 3.0, f"lam {lam}: shot normal")
        r = np.tanh(tl.astype(np.float64))                       # bounded: a correlation with a standard error whatever the tails
        for a, b, what in ((r, uq, "tl, uq"), (r, zs, "tl, zs"), (uq, zs, "uq, zs")):
            c = np.corrcoef(a, b)[0, 1]
            if abs(c) > 5 / math.sqrt(n):
                bad.append(f"lam {lam}: corr({what}) {c:.2e}")
    z = np.empty(n, np.float32)
    host_sampler.cam_host_rows(KEY, 0, 0, n, z.ctypes.data)
    bad += CS.check_moments(z, 0.0, 1.0, 3.0, "row normal")
    z2 = np.empty(16, np.float32)
    host_sampler.cam_host_rows(KEY, 0, 100, 16, z2.ctypes.data)
    assert np.array_equal(z2, z[100:116])                        # a function of (key, slot, row)
    host_sampler.cam_host_rows(KEY, 1, 100, 16, z2.ctypes.data)
    assert not np.array_equal(z2, z[100:116])
    assert not bad, bad


def test_tail_truncation_is_the_documented_one(host_sampler):
    from scipy import stats
    for lam, bound in ((-0.26, 1468.0), (0.0, 22.9), (0.102, 8.85)):
        q = np.empty(2, np.float32)
        host_sampler.cam_host_tail(lam, q.ctypes.data)
        want = float(stats.tukeylambda.ppf(2.0 ** -33, float(np.float32(lam))))
        assert q[0] == pytest.approx(want, rel=2e-5) and abs(q[0]) <= bound * 1.001 and abs(q[0]) >= bound * 0.99, (lam, q, want)
        assert q[1] == 0.0
    src = open(os.path.join(ROOT, "yond_public_amd", "csrc", "camnoise_sampler.h")).read()
    assert "1468 at lam = -0.26" in src and "8.85 at lam = 0.102" in src
