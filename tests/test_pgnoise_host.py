"""CPU: the host half of the Poisson-Gaussian noise path (yond_public_amd/pgnoise.py) -- the camera-noise prior against the reference's
draws (tests/golden/pgnoise.npz, tools/gen_golden_pgnoise.py), the item layout, the C ABI's argument checks, the kernel's resource
report -- and the surfaces that name it: --synth-noise in both parsers, DIV2K_PG_Dataset in trainer_AWGN's namespace."""
import ctypes
import os
import re

import numpy as np
import pytest

from yond_public_amd import pgnoise as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prior_draws_are_the_references(golden):
    g = golden("pgnoise")
    assert len(g["seeds"]) == 8
    fields = [str(f) for f in g["fields"]]
    assert fields == ["K", "sigma", "beta1", "beta2", "wp", "bl", "scale"]
    for s in g["seeds"]:
        p = PG.sample_pg_params(np.random.RandomState(int(s)))
        assert sorted(p) == sorted(fields)
        got = np.array([p[f] for f in fields], np.float64)
        assert np.array_equal(got, g[f"params_{int(s)}"]), (int(s), got, g[f"params_{int(s)}"])
    assert {str(k): float(v) for k, v in zip(g["prior_names"], g["prior_values"])} == {k: float(v) for k, v in PG.NOISE_PRIOR.items()}
    # consecutive draws on one stream differ and stay inside the prior's K range
    rs = np.random.RandomState(5)
    ks = [PG.sample_pg_params(rs)["K"] for _ in range(200)]
    assert len(set(ks)) == 200 and np.exp(-2.5) <= min(ks) and max(ks) <= np.exp(3.5)


def test_item_layout_matches_the_header():
    assert PG.ITEM_DTYPE.itemsize == 20
    assert [(n, PG.ITEM_DTYPE.fields[n][1]) for n in PG.ITEM_DTYPE.names] == [("beta1", 0), ("sigma_n", 4), ("exposure", 8), ("key", 12),
                                                                             ("slot", 16)]
    h = open(os.path.join(ROOT, "include", "yond_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} YondPGItem;", h)
    decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for part in decl.split(";") if part.strip() for n in part.strip().split(None, 1)[1].split(",")]
    assert names == list(PG.ITEM_DTYPE.names)
    assert "float beta1" in decl and "float sigma_n" in decl and "float exposure" in decl and "uint32_t key, slot" in decl
    it = PG.plan(3, [1.0, 2.0, 4.0], 8.0, 959.0, 77, [5, 6, 7], exposure=0.01)
    assert it.tobytes()[20:40] == np.array([2.0 / 959.0, 8.0 / 959.0, 0.01], "<f4").tobytes() + np.array([77, 6], "<u4").tobytes()
    for bad in (dict(K=[1.0, 2.0]), dict(sigma=-1.0), dict(exposure=0.0), dict(exposure=float("inf")), dict(scale=0.0)):
        with pytest.raises(ValueError):
            PG.plan(3, **dict(dict(K=1.0, sigma=1.0, scale=959.0, key=0, slots=[0, 1, 2]), **bad))
    # the regimes' thresholds are the sampler's own constants
    src = open(os.path.join(ROOT, "yond_public_amd", "csrc", "pgnoise_sampler.h")).read()
    consts = [float(re.search(rf"#define {n} ([0-9.]+)f", src).group(1)) for n in ("PG_SWITCH_PTRS", "PG_SWITCH_NORMAL")]
    assert consts == list(PG.SWITCH_LAMBDAS)


def test_abi_argument_checks_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from yond_public_amd import _lib
    f = _lib.load().yond_pg_noise_f32
    d = ctypes.c_void_p(16)                       # never dereferenced: every call below is refused before a launch
    ok = dict(clean=d, noisy=d, n=64, B=1, items=d, clip=0, stream=None)

    def call(**kw):
        return f(*dict(ok, **kw).values())
    for name in ("clean", "noisy", "items"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(n=0) == -1
    assert call(clip=2) == -1 and call(clip=-1) == -1
    assert call(clean=ctypes.c_void_p(18)) == -1 and call(noisy=ctypes.c_void_p(17)) == -1     # not 4-byte aligned


def test_kernel_has_no_spills():
    from yond_public_amd import build as B
    B.build_lib(verbose=False)
    rep = [r for r in B.resource_report() if "pg_noise" in r["name"]]
    assert len(rep) == 1, (rep, len(B.resource_report()))
    assert (rep[0]["vgpr_spill"], rep[0]["sgpr_spill"], rep[0]["scratch"]) == (0, 0, 0), rep


def test_sampler_on_the_cpu(tmp_path):
    """csrc/pgnoise_sampler.h is plain C++ as well: the source the kernel runs, compiled with the host compiler, through the ladder of
    tests/test_hip_pgnoise.py (2^17 draws per lambda; the bounds are the ladder's, they scale with N) -- regimes, thresholds and the
    Stirling-difference acceptance test are checked where no GPU exists.  Also: count and normal of one element are uncorrelated."""
    import shutil
    import subprocess
    import pgnoise_stats as PS
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    so = str(tmp_path / "libpgnoise_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "pgnoise_host_sampler.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.pg_host_draw.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_void_p, ctypes.c_void_p]
    lib.pg_host_draw.restype = None
    n, bad = 2 ** 17, []
    for slot, lam in enumerate(PS.ladder(PG.SWITCH_LAMBDAS)):
        lam32 = np.array([lam], np.float32)
        k, z = np.empty(n, np.float32), np.empty(n, np.float32)
        lib.pg_host_draw(20261018, slot, 0, n, lam32.ctypes.data, 1, k.ctypes.data, z.ctypes.data)
        row, fails = PS.check_counts(k.astype(np.float64), lam)
        if lam > 0 and k.std() > 0 and abs(np.corrcoef(k, z)[0, 1]) > 5 / np.sqrt(n):
            fails.append(f"corr(k, z) {np.corrcoef(k, z)[0, 1]:.2e}")
        print(row + ("   FAIL: " + "; ".join(fails) if fails else ""))
        bad += [f"lambda {lam}: {f}" for f in fails]
    assert not bad, bad


def test_parsers_take_synth_noise(capsys):
    from yond_public_amd.trainer_AWGN import AWGN_Parser
    from yond_public_amd.YOND_SIDD import YONDParser
    for parser in (AWGN_Parser, YONDParser):
        assert parser().parse(["--synth-noise", "4,6"]).synth_noise == (4.0, 6.0)
        assert parser().parse(["--synth-noise", "0.5,0"]).synth_noise == (0.5, 0.0)
        assert parser().parse([]).synth_noise is None
        for bad in ("4", "4,6,8", "four,6", "0,6", "-1,6", "4,-6", "nan,6", "4,inf"):
            with pytest.raises(SystemExit):
                parser().parse(["--synth-noise", bad])
            assert "--synth-noise" in capsys.readouterr().err, bad


def test_pg_dataset_is_named_and_refuses_est(tmp_path):
    from yond_public_amd import trainer_AWGN as TA
    assert TA.DIV2K_PG_Dataset is vars(TA)["DIV2K_PG_Dataset"] and issubclass(TA.DIV2K_PG_Dataset, TA.DIV2K_Img2Raw_Dataset)
    args = dict(root_dir=str(tmp_path), mode="train", H=8, W=8, command="est")
    with pytest.raises(NotImplementedError, match="command: est"):
        TA.DIV2K_PG_Dataset(args)
    # packed raw patches: this dataset synthesises from sRGB
    (tmp_path / "train").mkdir()
    np.save(tmp_path / "train" / "a.npy", np.zeros((4, 4, 4), np.float32))
    with pytest.raises(ValueError, match="synthesises its raw pairs from sRGB"):
        TA.DIV2K_PG_Dataset(dict(args, command="cache"))
    os.remove(tmp_path / "train" / "a.npy")
    np.save(tmp_path / "train" / "a.npy", np.zeros((8, 8, 3), np.uint8))
    ds = TA.DIV2K_PG_Dataset(dict(args, command="cache"))
    assert ds.p == PG.sample_pg_params(np.random.RandomState(0)) and ds.noise_params == PG.NOISE_PRIOR
    ds = TA.DIV2K_PG_Dataset(dict(args, command="cache", K=2.0, sigma_dn=8.0))
    assert (ds.p["K"], ds.p["sigma"], ds.p["beta1"], ds.p["beta2"]) == (2.0, 8.0, 2.0 / 959, (8.0 / 959) ** 2)
    with pytest.raises(ValueError, match="both"):
        TA.DIV2K_PG_Dataset(dict(args, command="cache", K=2.0))
    import yaml
    # a guided architecture is refused while the runfile is read: before a device, a dataset or a network exists
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "Unet_PG_norm_noclip.yml")).read(), Loader=yaml.FullLoader)
    cfg["arch"] = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "GRU_5to50_norm_mix.yml")).read(), Loader=yaml.FullLoader)["arch"]
    (tmp_path / "guided.yml").write_text(yaml.dump(cfg))
    with pytest.raises(ValueError, match="guided"):
        TA.AWGN_Trainer(["-f", str(tmp_path / "guided.yml"), "-m", "train"])
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "Unet_PG_norm_noclip.yml")).read(), Loader=yaml.FullLoader)
    assert {cfg[s]["dataset"] for s in ("dst", "dst_train", "dst_eval", "dst_test")} == {"DIV2K_PG_Dataset"}
    assert cfg["dst"]["clip"] is False and "guided" not in cfg["arch"]
