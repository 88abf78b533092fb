"""CPU: the host side of the row-noise feature -- the two entry points' argument checks (they run before any launch, so a made-up pointer
is never dereferenced), the header / export / prototype wiring, the drivers' argument parser, the runfile key and the unit conversion."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
A, B, S, O = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000))      # never read: every call below is refused


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from yond_public_amd import _lib
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from yond_public_amd import _lib
    from yond_public_amd import rownoise as RN
    header = open(os.path.join(ROOT, "include", "yond_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("yond_rownoise_sums_f32", "yond_rownoise_apply_f32"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(raw, name) and name in _lib.PROTOTYPES
    assert lib.yond_abi_version() == 8                       # additive: the version stays
    assert int(re.search(r"#define\s+YOND_ROWNOISE_MAX_D\s+(\d+)", header).group(1)) == RN.MAX_D
    assert int(re.search(r"#define\s+YOND_ROWNOISE_ROW\s+(\d+)", header).group(1)) == RN.PER['row']
    assert int(re.search(r"#define\s+YOND_ROWNOISE_PLANE\s+(\d+)", header).group(1)) == RN.PER['plane']


def test_sums_entry_refuses_before_any_launch(lib):
    f = lib.yond_rownoise_sums_f32
    assert f(None, 64, 64, S, None) == EINVAL
    assert f(A, 64, 64, None, None) == EINVAL
    assert f(ctypes.c_void_p(0x10002), 64, 64, S, None) == EINVAL        # a float pointer off its 4 bytes
    assert f(A, 64, 64, ctypes.c_void_p(0x30004), None) == EINVAL        # a double pointer off its 8 bytes
    for H, W in ((63, 64), (64, 63), (0, 64), (64, 0), (-2, 64), (64, -2), (65536, 32768), (65536, 65536)):
        assert f(A, H, W, S, None) == EINVAL, (H, W)


def test_apply_entry_refuses_before_any_launch(lib):
    from yond_public_amd import rownoise as RN
    f = lib.yond_rownoise_apply_f32
    ok = (0, 25, 10.0, 9.0)
    assert f(None, B, 64, 64, S, *ok, O, None) == EINVAL
    assert f(A, None, 64, 64, S, *ok, O, None) == EINVAL
    assert f(A, B, 64, 64, None, *ok, O, None) == EINVAL
    assert f(ctypes.c_void_p(0x10002), B, 64, 64, S, *ok, None, None) == EINVAL
    assert f(A, ctypes.c_void_p(0x20001), 64, 64, S, *ok, None, None) == EINVAL
    assert f(A, B, 64, 64, ctypes.c_void_p(0x30004), *ok, None, None) == EINVAL
    assert f(A, B, 64, 64, S, *ok, ctypes.c_void_p(0x40004), None) == EINVAL
    for H, W in ((63, 64), (64, 63), (0, 64), (64, 0), (-2, 64), (64, -2), (65536, 32768)):
        assert f(A, B, H, W, S, *ok, None, None) == EINVAL, (H, W)
    for d in (0, -1, 2, 24, RN.MAX_D + 1, RN.MAX_D + 2):
        assert f(A, B, 64, 64, S, 0, d, 10.0, 9.0, None, None) == EINVAL, d
    for sc, ss in ((0.0, 9.0), (-1.0, 9.0), (10.0, 0.0), (10.0, -3.0), (float('nan'), 9.0), (10.0, float('nan')), (float('inf'), 9.0),
                   (10.0, float('inf')), (1e-200, 9.0)):
        assert f(A, B, 64, 64, S, 0, 25, sc, ss, None, None) == EINVAL, (sc, ss)
    for shift in (4, 64 * 4, 64 * 64 * 4 - 4, -4, -64 * 4):               # out overlaps in without being in: waves would race
        assert f(A, ctypes.c_void_p(0x10000 + shift), 64, 64, S, *ok, None, None) == EINVAL, shift
    for per in (-1, 2, 7):
        assert f(A, B, 64, 64, S, per, 25, 10.0, 9.0, None, None) == EINVAL, per


def test_row_denoise_arg():
    from yond_public_amd import rownoise as RN
    default = {'sc': 10.0, 'ss': 'auto', 'd': 25, 'per': 'row'}
    assert RN.row_denoise_arg('on') == default and RN.row_denoise_arg('') == default and RN.row_denoise_arg(True) == default
    assert RN.row_denoise_arg('sc=4.5') == dict(default, sc=4.5)
    assert RN.row_denoise_arg('ss=9') == dict(default, ss=9.0) and RN.row_denoise_arg('ss=auto') == default
    assert RN.row_denoise_arg('d=31') == dict(default, d=31)
    assert RN.row_denoise_arg('per=plane') == dict(default, per='plane') and RN.row_denoise_arg('per=row') == default
    assert RN.row_denoise_arg('sc=10,ss=9,d=25,per=plane') == {'sc': 10.0, 'ss': 9.0, 'd': 25, 'per': 'plane'}
    for bad in ('d=24', 'd=0', 'd=65', 'd=2.5', 'sc=0', 'sc=-1', 'sc=nan', 'ss=0', 'ss=-2', 'ss=inf', 'k=3', 'sigma=3', 'per=col', 'per=', 'sc', 'sc=x', 'off'):
        with pytest.raises(argparse.ArgumentTypeError):
            RN.row_denoise_arg(bad)


def test_row_denoise_of_reads_the_runfile_key_and_the_flag_overrides_it():
    from yond_public_amd import rownoise as RN
    from yond_public_amd._lib import YondHipError
    default = RN.row_denoise_arg('on')
    assert RN.row_denoise_of({}, None) is None and RN.row_denoise_of({'row_denoise': False}, None) is None
    assert RN.row_denoise_of({'row_denoise': 'off'}, argparse.Namespace(row_denoise=None)) is None
    assert RN.row_denoise_of({'row_denoise': True}, None) == default and RN.row_denoise_of({'row_denoise': 'on'}, None) == default
    assert RN.row_denoise_of({'row_denoise': 'sc=5,per=plane'}, None) == dict(default, sc=5.0, per='plane')
    flag = RN.row_denoise_arg('d=31')
    assert RN.row_denoise_of({'row_denoise': 'sc=5,per=plane'}, argparse.Namespace(row_denoise=flag)) == flag
    with pytest.raises(YondHipError):
        RN.row_denoise_of({'row_denoise': 'd=24'}, None)


def test_the_drivers_parser_takes_the_flag_with_and_without_a_spec():
    from yond_public_amd.YOND_SIDD import YONDParser
    from yond_public_amd import rownoise as RN
    assert YONDParser().parse([]).row_denoise is None
    assert YONDParser().parse(['--row-denoise']).row_denoise == RN.row_denoise_arg('on')
    assert YONDParser().parse(['--row-denoise', '--synthetic', '1']).row_denoise == RN.row_denoise_arg('on')
    assert YONDParser().parse(['--row-denoise', 'sc=10,ss=9,d=25']).row_denoise == {'sc': 10.0, 'ss': 9.0, 'd': 25, 'per': 'row'}
    with pytest.raises(SystemExit):
        YONDParser().parse(['--row-denoise', 'd=24'])


def test_frame_units():
    """sc DN at capture are sc * ratio / (wp - bl) of the frame (DN - bl) / (wp - bl) * ratio; ss=auto is 1 + ISO / 200."""
    from yond_public_amd import rownoise as RN
    spec = RN.row_denoise_arg('on')
    sc, ss, dn = RN.frame_units(spec, 2, 1023, 64, 800)
    assert sc == 10.0 * 2 / 959 and ss == 5.0 and np.isclose(dn, 959 / 2, rtol=1e-15)
    sc, ss, _ = RN.frame_units(spec, 100, 16383, 512, None)
    assert sc == 10.0 * 100 / 15871 and ss == 1 + RN.DEFAULT_ISO / 200 == 9.0
    sc, ss, _ = RN.frame_units(RN.row_denoise_arg('sc=4,ss=3.5'), 1, 1023, 64, 6400)
    assert sc == 4.0 / 959 and ss == 3.5                     # a given ss is taken as it is
    # a frame in those units, denoised with the converted sc, is the DN frame denoised with sc (the filter is scale-equivariant)
    import rownoise_model as M
    x = M.frame(3, 20, 16)
    _, off_dn, _ = M.row_denoise(x.astype(np.float32), M.ROW, 25, 10.0, 9.0)
    scale = 2 / 959
    _, off_u, _ = M.row_denoise(((x - 64) * scale).astype(np.float32), M.ROW, 25, 10.0 * scale, 9.0)
    assert np.abs(off_u / scale - off_dn).max() < 1e-3


def test_library_argument_errors_need_no_gpu():
    import torch
    from yond_public_amd import rownoise as RN
    from yond_public_amd._lib import YondHipError
    with pytest.raises(YondHipError):
        RN.row_denoise(torch.zeros(4, 4), 1600)              # a host tensor: no CPU fallback
    with pytest.raises(YondHipError):
        RN.row_sums(np.zeros((4, 4), np.float32))
    for kw in (dict(sigma_color=0.0), dict(sigma_space=-1.0), dict(d=24), dict(d=65), dict(per='col')):
        with pytest.raises(ValueError):
            RN.check_params(**dict(dict(sigma_color=10.0, sigma_space=9.0, d=25, per='row'), **kw))
