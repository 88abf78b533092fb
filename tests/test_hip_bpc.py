"""GPU: the defective-pixel kernels (csrc/bpc.hip, include/yond_hip.h M4) against the NumPy model tests/bpc_model.py -- exact: the
output frame `==` the model's, and the flagged coordinate sets and counts are equal.

Shapes: 2x2, 2x6, 6x2, 4x4 are all border; 34x258 and 66x130 cross the kernel's tile (bpc.TILE_H x bpc.TILE_W) in both directions;
70x134 and 18x1030 have W % 4 == 2 (rows are not 16-byte aligned: the 8-byte path); 256x512 is many workgroups.  Inputs are seeded
Poisson-Gaussian frames with hot and cold defects at the four corners, on every edge, on both sides of the tile seams, on neighbouring
mosaic positions of different colour, as a touching same-colour pair (unflagged in auto mode, repaired from the originals in list
mode), and four values that straddle the threshold by one float32 ulp, built from the model's own float64 comparison.  At t = 3 noise
pixels are flagged too; at t = 0.75 (two more cases) thousands are: the counters and the coordinate list at volume.
"""
import numpy as np
import pytest

import bpc_model as M

pytestmark = pytest.mark.gpu
SCALE, K, SIGMA = 959.0, 4.0, 6.0
BETA1, BETA2 = K / SCALE, (SIGMA / SCALE) ** 2
SHAPES = [(2, 2), (2, 6), (6, 2), (4, 4), (34, 258), (66, 130), (70, 134), (18, 1030), (256, 512)]
T_VOLUME = 0.75                      # the rule needs a pixel beyond ALL eight neighbours: at t = 3 a few noise pixels per 100,000 are flagged, here thousands
CASES = [(s, t) for s in SHAPES for t in (3.0, 6.0)] + [((70, 134), T_VOLUME), ((256, 512), T_VOLUME)]
HOT, COLD = np.float32(2.0), np.float32(0.0)


def _noisy(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    clean = 0.35 + 0.3 * x / max(W - 1, 1) + 0.1 * y / max(H - 1, 1)
    return ((rng.poisson(clean * SCALE / K) * K + rng.normal(0.0, SIGMA, (H, W))) / SCALE).astype(np.float32)


def _straddle(frame, y, x, t, hot):
    """The two float32 values one ulp apart between which the model's comparison at (y, x) turns, for the hot or the cold side."""
    nb = M.neighbourhood(frame)[[0, 1, 2, 3, 5, 6, 7, 8], y, x]
    ref = np.float64(nb.max() if hot else nb.min())
    t2 = np.float64(t) * np.float64(t)
    rhs = t2 * (np.float64(BETA1) * np.maximum(ref, 0.0) + np.float64(BETA2))

    def flagged(c):
        d = (np.float64(c) - ref) if hot else (ref - np.float64(c))
        return d * d > rhs
    step = np.float32(np.inf if hot else -np.inf)
    c = np.float32(ref + (1 if hot else -1) * np.sqrt(rhs))
    while flagged(c):                                        # walk to the last unflagged value, then one ulp on
        c = np.nextafter(c, -step)
    while not flagged(np.nextafter(c, step)):
        c = np.nextafter(c, step)
    return c, np.nextafter(c, step)                          # (unflagged, flagged)


def _case(H, W, t, seed=0):
    """(frame, {(row, col): tag} of the pixels it was disturbed at).  No two disturbed pixels are within each other's same-colour
    footprint, except the two pairs that are meant to be."""
    from yond_public_amd import bpc as BP
    frame = _noisy(H, W, 100 * H + W + seed)
    placed = {}

    def free(y, x, but=None):
        return 0 <= y < H and 0 <= x < W and all(abs(y - p) > 2 or abs(x - q) > 2 for p, q in placed if (p, q) != but)

    def put(y, x, v, tag, but=None):
        if free(y, x, but):
            frame[y, x] = v(y, x) if callable(v) else v
            placed[(y, x)] = tag
            return True
        return False
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        put(y, x, HOT, 'corner')
    for k, (y, x) in enumerate(((0, W // 2), (H - 1, W // 2 + 5), (H // 2, 0), (H // 2 + 5, W - 1), (1, W // 3), (H - 2, W // 3 + 7),
                                (H // 3, 1), (H // 3 + 7, W - 2))):                         # both rows / columns of the border ring
        put(y, x, COLD if k % 2 else HOT, 'edge')
    ym = H // 2 - 3
    if put(ym, 20, HOT, 'other colour'):
        put(ym, 21, HOT, 'other colour', but=(ym, 20))                                      # neighbours of different colour: both flagged
    if put(ym, 30, HOT, 'pair'):
        put(ym, 32, HOT, 'pair', but=(ym, 30))                                              # touching, same colour: they hide each other
    # one ulp on either side of the threshold (no later defect comes within the footprint of these four: their neighbours stay)
    for x, hot, pick in ((12, True, 0), (24, True, 1), (36, False, 0), (48, False, 1)):
        put(ym + 8, x, lambda yy, xx: _straddle(frame, yy, xx, t, hot)[pick], ('above' if pick else 'below') + (' hot' if hot else ' cold'))
    k = 0
    for ty in range(BP.TILE_H, H, BP.TILE_H):                                               # both sides of the horizontal seams
        for y in (ty - 1, ty, ty - 2, ty + 1):
            put(y, 7 + 11 * k, COLD if k % 3 == 0 else HOT, 'seam')
            k += 1
    for tx in range(BP.TILE_W, W, BP.TILE_W):                                               # ... and of the vertical ones
        for x in (tx - 1, tx, tx - 2, tx + 1):
            put(5 + 7 * (k % 3), x, COLD if k % 3 == 0 else HOT, 'seam')
            k += 1
    return frame, placed


@pytest.fixture(scope="module")
def cases():
    """(frame, disturbed sites, model output, model info) per (shape, t): computed once, shared, never modified."""
    out = {}
    for (H, W), t in CASES:
        frame, placed = _case(H, W, t)
        frame.setflags(write=False)
        out[(H, W, t)] = (frame, placed) + M.detect_and_repair(frame, BETA1, BETA2, t)
    return out


def _points(p):
    return {(int(r), int(c)) for r, c in p}


@pytest.mark.parametrize("shape,t", CASES)
def test_detect_and_repair_equals_the_model(cases, shape, t):
    import torch
    from yond_public_amd import bpc as BP
    frame, placed, want, winfo = cases[shape + (t,)]
    dev = torch.from_numpy(frame.copy()).cuda()
    out, info = BP.detect_and_repair(dev, BETA1, BETA2, t, coords=frame.size)
    torch.cuda.synchronize()
    n_model = winfo['hot'] + winfo['cold']
    print(f"[bpc] {shape} t={t}: model hot {winfo['hot']}, cold {winfo['cold']}; kernel hot {info['hot']}, cold {info['cold']}; {len(placed)} disturbed")
    assert (info['hot'], info['cold']) == (winfo['hot'], winfo['cold'])
    assert not info['overflow'] and info['points'].dtype == np.int32 and info['points'].shape == (n_model, 2)
    assert np.array_equal(info['points'], winfo['points'])               # both sorted by (row, col)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), frame)                      # the input is left alone
    if min(shape) <= 4:
        assert n_model == 0                                              # everything is border


def test_the_inputs_exercise_what_they_claim(cases):
    """The model on the inputs above: the border ring and the touching pair stay unflagged, the different-colour neighbours and the
    seam defects are flagged, and the straddling values fall one on each side."""
    seen = set()
    for (H, W, t), (frame, placed, want, winfo) in cases.items():
        flagged = _points(winfo['points'])
        for (y, x), tag in placed.items():
            ring = y < 2 or x < 2 or y >= H - 2 or x >= W - 2
            seen.add('ring' if ring else tag)
            if ring or tag == 'pair' or tag.startswith('below'):
                assert (y, x) not in flagged, (H, W, t, y, x, tag)
            else:
                assert (y, x) in flagged, (H, W, t, y, x, tag)
        if t == 3.0 and H * W >= 256 * 512:
            assert winfo['hot'] + winfo['cold'] > len(placed)            # noise pixels too
        if t == T_VOLUME and H * W >= 256 * 512:
            assert winfo['hot'] > 1000 and winfo['cold'] > 1000          # the counters and the coordinate list at volume
        if (H, W) in ((34, 258), (66, 130), (256, 512)):
            assert {tag for tag in placed.values()} >= {'corner', 'edge', 'seam', 'other colour', 'pair', 'above hot', 'below hot', 'above cold', 'below cold'}
    assert seen >= {'ring', 'seam', 'other colour', 'pair', 'above hot', 'below hot', 'above cold', 'below cold'}


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("shape", [(66, 130), (34, 256)])
def test_misaligned_frames_take_the_narrow_paths(shape, offset):
    """A frame that starts 4 or 8 bytes into its allocation: 4-byte and 8-byte global accesses, same values."""
    import torch
    from yond_public_amd import bpc as BP
    H, W = shape
    frame, _ = _case(H, W, 3.0, seed=1)
    want, winfo = M.detect_and_repair(frame, BETA1, BETA2, 3.0)
    buf = torch.zeros(H * W + 4, dtype=torch.float32, device='cuda')
    dev = buf[offset:offset + H * W].view(H, W)
    dev.copy_(torch.from_numpy(frame))
    assert dev.data_ptr() % 16 == 4 * offset and dev.is_contiguous()
    out, info = BP.detect_and_repair(dev, BETA1, BETA2, 3.0, coords=H * W)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(info['points'], winfo['points'])
    assert (info['hot'], info['cold']) == (winfo['hot'], winfo['cold'])
    assert float(buf[:offset].abs().sum()) == 0 and float(buf[offset + H * W:].abs().sum()) == 0


@pytest.mark.parametrize("shape,t", [((34, 258), 3.0), ((256, 512), T_VOLUME)])
def test_coordinate_capacity(cases, shape, t):
    import torch
    from yond_public_amd import bpc as BP
    frame, _, want, winfo = cases[shape + (t,)]
    n = winfo['hot'] + winfo['cold']
    assert n > 8
    dev = torch.from_numpy(frame.copy()).cuda()
    out, info = BP.detect_and_repair(dev, BETA1, BETA2, t)             # no buffer: counts only
    assert info['points'] is None and not info['overflow'] and (info['hot'], info['cold']) == (winfo['hot'], winfo['cold'])
    assert np.array_equal(out.cpu().numpy(), want)
    for cap in (1, n // 2, n - 1):
        out, info = BP.detect_and_repair(dev, BETA1, BETA2, t, coords=cap)
        assert info['overflow'] and (info['hot'], info['cold']) == (winfo['hot'], winfo['cold'])
        got = _points(info['points'])
        assert info['points'].shape == (cap, 2) and len(got) == cap and got <= _points(winfo['points'])
        assert np.array_equal(out.cpu().numpy(), want)
    out, info = BP.detect_and_repair(dev, BETA1, BETA2, t, coords=n)   # exactly enough
    assert not info['overflow'] and np.array_equal(info['points'], winfo['points'])


def test_coordinate_buffer_is_not_overrun():
    """The C entry with a buffer of cap rows inside a larger, poisoned allocation: nothing behind row cap is written."""
    import torch
    from yond_public_amd import _lib as L
    frame, _ = _case(66, 130, 3.0)
    want, winfo = M.detect_and_repair(frame, BETA1, BETA2, 3.0)
    cap = (winfo['hot'] + winfo['cold']) // 3
    dev = torch.from_numpy(frame).cuda()
    out = torch.empty_like(dev)
    counts = torch.zeros(2, dtype=torch.int32, device='cuda')
    buf = torch.full((cap + 64, 2), -7, dtype=torch.int32, device='cuda')
    L.check(L.load().yond_bpc_detect_repair_f32(L.ptr(dev), L.ptr(out), 66, 130, BETA1, BETA2, 3.0, L.ptr(counts), L.ptr(buf), cap, L.stream()), "detect")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[cap:] == -7).all() and (host[:cap] >= 0).all()
    assert counts.cpu().tolist() == [winfo['hot'], winfo['cold']]
    # a null buffer with a capacity: counts only
    counts.zero_()
    L.check(L.load().yond_bpc_detect_repair_f32(L.ptr(dev), L.ptr(out), 66, 130, BETA1, BETA2, 3.0, L.ptr(counts), None, 100, L.stream()), "detect")
    assert counts.cpu().tolist() == [winfo['hot'], winfo['cold']] and np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(2, 2), (4, 4), (66, 130), (70, 134)])
def test_list_mode_equals_the_model(cases, shape):
    import torch
    from yond_public_amd import bpc as BP
    from yond_public_amd.utils import isp_ops
    H, W = shape
    frame, placed, _, _ = cases[shape + (6.0,)]
    pts = np.array(list(placed) + list(placed)[:2] + [(H // 2, W // 2), (H // 2, (W // 2 + 2) % W), ((H // 2 + 1) % H, W // 2)], np.int64)   # duplicates, neighbours
    want = M.repair_list(frame, pts)
    dev = torch.from_numpy(frame.copy()).cuda()
    got = BP.repair_bad_pixels(dev, pts)
    assert got.data_ptr() != dev.data_ptr() and np.array_equal(got.cpu().numpy(), want) and np.array_equal(dev.cpu().numpy(), frame)
    assert np.array_equal(isp_ops.repair_bad_pixels(dev, pts).cpu().numpy(), want)      # the reference's seam, device in -> device out
    assert np.array_equal(isp_ops.repair_bad_pixels(frame.copy(), pts), want)           # ... NumPy in -> NumPy out
    if H >= 16 and W >= 40:
        y = H // 2 - 3
        assert want[y, 30] < 1 and want[y, 32] < 1                        # the touching pair, each repaired from the originals
    # n = 0, as a host list and as a device tensor
    assert np.array_equal(BP.repair_bad_pixels(dev, []).cpu().numpy(), frame)
    assert np.array_equal(BP.repair_bad_pixels(dev, torch.zeros((0, 2), dtype=torch.int32, device='cuda')).cpu().numpy(), frame)
    # a host list with a point outside the frame is the caller's mistake ...
    with pytest.raises(ValueError):
        BP.repair_bad_pixels(dev, np.concatenate([pts, [[H, 0]]]))
    with pytest.raises(ValueError):
        BP.repair_bad_pixels(dev, pts, method='mean')
    # ... a device list is not read on the host: the kernel drops such points, and nothing else in out changes
    wild = np.concatenate([pts, [[-1, 0], [0, -1], [H, 0], [0, W], [2 ** 30, 2 ** 30], [-2 ** 31, 5]]])
    for dtype in (torch.int32, torch.int64):
        got = BP.repair_bad_pixels(dev, torch.from_numpy(wild).to('cuda', dtype))
        assert np.array_equal(got.cpu().numpy(), want)


def test_non_finite_pixels_do_not_fault():
    import torch
    from yond_public_amd import bpc as BP
    frame = _noisy(66, 130, 5)
    frame[10, 10], frame[31, 127], frame[33, 2], frame[0, 0] = np.nan, np.inf, -np.inf, np.nan
    dev = torch.from_numpy(frame).cuda()
    out, info = BP.detect_and_repair(dev, BETA1, BETA2, 6.0, coords=64)
    fixed = BP.repair_bad_pixels(dev, [[10, 10], [31, 127], [33, 2], [0, 0]])
    torch.cuda.synchronize()
    far = np.ones(frame.shape, bool)
    for y, x in ((10, 10), (31, 127), (33, 2), (0, 0)):
        far[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = False
    want, _ = M.detect_and_repair(np.where(np.isfinite(frame), frame, np.float32(0.3)), BETA1, BETA2, 6.0)
    assert np.array_equal(out.cpu().numpy()[far], want[far])             # away from them the frame is the model's
    assert fixed.shape == dev.shape
