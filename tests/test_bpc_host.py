"""CPU: the host side of the defective-pixel feature -- the entry points' argument checks (they run before any launch, so a made-up
pointer is never dereferenced), the header / export / prototype wiring, the tile constants the GPU tests place defects by, and the
wrapper's host helpers (point lists, argument parsers, the keyed defect sites)."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
A, B, P = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)      # never read: every call below is refused


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from yond_public_amd import _lib
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from yond_public_amd import _lib
    header = open(os.path.join(ROOT, "include", "yond_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("yond_bpc_repair_list_f32", "yond_bpc_detect_repair_f32"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(raw, name) and name in _lib.PROTOTYPES
    assert lib.yond_abi_version() == 8                       # additive: the version stays


def test_tile_constants_match_the_header():
    from yond_public_amd import bpc as BP
    header = open(os.path.join(ROOT, "include", "yond_hip.h")).read()
    assert int(re.search(r"#define\s+YOND_BPC_TILE_W\s+(\d+)", header).group(1)) == BP.TILE_W
    assert int(re.search(r"#define\s+YOND_BPC_TILE_H\s+(\d+)", header).group(1)) == BP.TILE_H


def test_detect_entry_refuses_before_any_launch(lib):
    f = lib.yond_bpc_detect_repair_f32
    ok = (64, 64, 1e-3, 1e-6, 6.0)
    assert f(None, B, *ok, P, None, 0, None) == EINVAL
    assert f(A, None, *ok, P, None, 0, None) == EINVAL
    assert f(A, B, *ok, None, None, 0, None) == EINVAL       # the counts are not optional
    assert f(A, A, *ok, P, None, 0, None) == EINVAL          # one pass cannot repair in place
    for H, W in ((63, 64), (64, 63), (0, 64), (64, 0), (-2, 64), (64, -2), (65536, 65536)):
        assert f(A, B, H, W, 1e-3, 1e-6, 6.0, P, None, 0, None) == EINVAL, (H, W)
    assert f(A, B, *ok, P, None, -1, None) == EINVAL
    assert f(ctypes.c_void_p(0x10002), B, *ok, P, None, 0, None) == EINVAL       # a float pointer off its 4 bytes
    assert f(A, B, *ok, ctypes.c_void_p(0x30004), None, 0, None) == EINVAL       # the pair of counts is one 8-byte word


def test_list_entry_refuses_before_any_launch(lib):
    f = lib.yond_bpc_repair_list_f32
    assert f(None, B, 64, 64, P, 4, None) == EINVAL
    assert f(A, None, 64, 64, P, 4, None) == EINVAL
    assert f(A, B, 64, 64, None, 4, None) == EINVAL
    for H, W in ((63, 64), (64, 63), (0, 64), (64, -2)):
        assert f(A, B, H, W, P, 4, None) == EINVAL, (H, W)
    assert f(A, B, 64, 64, P, -1, None) == EINVAL
    assert f(A, A, 64, 64, P, 2, None) == EINVAL             # in place: one point at the most
    assert f(A, B, 64, 64, None, 0, None) == 0               # nothing listed: nothing launched, no pointer read
    assert f(A, A, 64, 64, None, 0, None) == 0


def test_point_lists():
    from yond_public_amd import bpc as BP
    pts = BP.check_points([[0, 0], [5, 7], [5, 7]], (6, 8))
    assert pts.dtype == np.int32 and pts.shape == (3, 2) and pts.flags['C_CONTIGUOUS']
    assert BP.check_points([], (6, 8)).shape == (0, 2)
    for bad in ([[6, 0]], [[0, 8]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(ValueError):
            BP.check_points(bad, (6, 8))
    with pytest.raises(ValueError):
        BP.check_points([[0.5, 1.0]], (6, 8))
    with pytest.raises(ValueError):
        BP.check_points([1, 2, 3], (6, 8))


def test_driver_argument_parsers():
    from yond_public_amd import bpc as BP
    assert BP.bad_pixels_arg('auto') == ('auto', 6.0) and BP.bad_pixels_arg('auto:4.5') == ('auto', 4.5)
    assert BP.bad_pixels_arg('cam/bad.npy') == ('list', 'cam/bad.npy')
    for bad in ('auto:', 'auto:0', 'auto:-1', 'auto:nan', 'median', 'list.txt'):
        with pytest.raises(argparse.ArgumentTypeError):
            BP.bad_pixels_arg(bad)
    assert BP.synth_defects_arg('40') == (40, None) and BP.synth_defects_arg('12,1.5') == (12, 1.5)
    for bad in ('-1', 'x', '3,', '3,1,2', '3,inf'):
        with pytest.raises(argparse.ArgumentTypeError):
            BP.synth_defects_arg(bad)
    assert BP.bad_pixels_of({}, None) is None and BP.bad_pixels_of({'bad_pixels': False}, None) is None
    assert BP.bad_pixels_of({'bad_pixels': 'auto:5'}, None) == ('auto', 5.0)
    assert BP.bad_pixels_of({'bad_pixels': 'auto:5'}, argparse.Namespace(bad_pixels=('list', 'a.npy'))) == ('list', 'a.npy')


def test_defect_sites_are_keyed_isolated_and_interior():
    from yond_public_amd import bpc as BP
    a, b, c = BP.defect_sites((64, 96), 80, 5), BP.defect_sites((64, 96), 80, 5), BP.defect_sites((64, 96), 80, 6)
    assert a.shape == (80, 2) and a.dtype == np.int32 and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, a[np.lexsort((a[:, 1], a[:, 0]))])
    assert a[:, 0].min() >= 2 and a[:, 0].max() <= 61 and a[:, 1].min() >= 2 and a[:, 1].max() <= 93
    d = np.abs(a[:, None, :] - a[None, :, :])
    close = (d[..., 0] <= 2) & (d[..., 1] <= 2)
    assert close.sum() == len(a)                             # each site is within the footprint of itself alone
    with pytest.raises(ValueError):
        BP.defect_sites((16, 16), 100, 0)


def test_inject_defects_on_a_host_tensor():
    from yond_public_amd import bpc as BP
    frame = torch.full((32, 48), 0.25)
    out, pts = BP.inject_defects(frame, 12, 9, cold_share=0.25, ratio=2.0)
    assert np.array_equal(pts, BP.defect_sites((32, 48), 12, 9))
    vals = out[pts[:, 0], pts[:, 1]].numpy()
    assert sorted(vals.tolist()) == [0.0] * 3 + [2.0] * 9    # default level: the white level, ratio * 1.0
    mask = np.ones((32, 48), bool)
    mask[pts[:, 0], pts[:, 1]] = False
    assert (out.numpy()[mask] == 0.25).all() and (frame == 0.25).all()
    out2, _ = BP.inject_defects(frame, 12, 9, level=0.9)
    assert (out2[pts[:, 0], pts[:, 1]] == 0.9).all()
