"""GPU: the raw DN <-> [0, 1] kernels (csrc/rawio.hip) against tests/rawio_model.py, element for element and bit for bit -- edge shapes,
misaligned bases, every uint16 level, near-ties of the rounding, NaN / inf, the saturation counter -- and the layers above them: the
loader's device ingest, the full-frame driver's --save / --host-ingest, YOND_SIDD's --save f32."""
import json
import os

import numpy as np
import pytest
import torch

from rawio_model import GRID, LEVELS, emit_model, ingest_model, saturated_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# n % 8 in {4, 0, 2}; (34, 1030) and the stack take more than one workgroup
SHAPES = [(2, 2), (2, 6), (4, 10), (6, 14), (34, 1030), (3, 256, 320)]
# (elements the input view starts into its buffer, elements the output view does): a frame sliced out of a stack is 2 bytes off
OFFSETS = [(0, 0), (1, 0), (3, 1), (7, 2), (0, 3)]


@pytest.fixture(autouse=True)
def _device_present():
    """Without a device these tests fail at once (a loader thread that cannot make its stream used to leave its consumer waiting)."""
    assert torch.cuda.is_available(), "tests/test_hip_rawio.py needs an MI355X"


def _view(arr, off):
    """`arr` on the device as a contiguous view that starts `off` elements into a larger allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1))
    buf = torch.empty(flat.numel() + 16, dtype=flat.dtype, device=DEV)
    v = buf[off:off + flat.numel()]
    v.copy_(flat)
    v = v.view(arr.shape)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * flat.element_size()
    return v


def _out_view(shape, dtype, off):
    n = int(np.prod(shape))
    buf = torch.from_numpy(np.full(n + 16, 7, np.uint16 if dtype == torch.uint16 else np.float32)).to(DEV)
    return buf, buf[off:off + n].view(shape)


def _dn_values(shape, bl, wp, dtype, seed):
    """Every uint16 level in a fixed shuffle (the stack holds each at least once), with bl, bl +- 1 and wp in front; float32 frames also
    carry a fraction, negative DN, one inf and one NaN."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    v = np.resize(rng.permutation(65536), n).astype(np.float64)
    front = [int(bl), max(int(bl) - 1, 0), int(bl) + 1, int(wp)]
    v[:min(n, 4)] = front[:min(n, 4)]
    if dtype == np.uint16:
        return v.astype(np.uint16).reshape(shape)
    v = v.astype(np.float32)
    if n > 16:
        v[5::7] += np.float32(0.25)
        v[9], v[10], v[11], v[12] = -5.0, np.inf, np.nan, -70000.0
    else:
        v[n - 1] = [np.nan, np.inf, -5.0][seed % 3]
    return v.reshape(shape)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_ingest_is_the_host_expression_bit_for_bit(dtype):
    """yond_raw_ingest_u16 / _f32 == ingest_model for every element: the edge shapes, misaligned input and output bases, the level grid,
    clip both ways.  The untouched elements around a misaligned output stay untouched."""
    from yond_public_amd import rawio
    checked = 0
    for si, shape in enumerate(SHAPES):
        for gi, (bl, wp, ratio) in enumerate(GRID):
            raw = _dn_values(shape, bl, wp, dtype, si)
            for oi, (off_in, off_out) in enumerate(OFFSETS):
                if shape == SHAPES[-1] and (gi + oi) % 5:               # (the stack: every offset and grid entry, not every pair)
                    continue
                d_raw = _view(raw, off_in)
                for clip in (False, True):
                    want = ingest_model(raw, bl, wp, ratio, clip)
                    buf, out = _out_view(shape, torch.float32, off_out)
                    got = rawio.ingest(d_raw, bl, wp, ratio, clip, out=out)
                    assert got is out and got.dtype == torch.float32
                    assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (shape, bl, wp, ratio, off_in, off_out, clip)
                    n = want.size
                    assert bool((buf[:off_out] == 7).all()) and bool((buf[off_out + n:] == 7).all())
                    checked += 1
    assert checked > 1000
    # every level exactly once, without `out`
    for bl, wp, ratio in GRID[::7]:
        raw = np.arange(65536).astype(dtype).reshape(256, 256)
        got = rawio.ingest(torch.from_numpy(raw).to(DEV), bl, wp, ratio)
        assert got.shape == (256, 256) and np.array_equal(got.cpu().numpy(), ingest_model(raw, bl, wp, ratio))


def test_ingest_and_emit_refuse_what_they_do_not_cover():
    from yond_public_amd import _lib, rawio
    lib = _lib.load()
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(TypeError, match="int16"):
        rawio.ingest(x.to(torch.int16), 64, 1023)
    with pytest.raises(TypeError, match="float64"):
        rawio.ingest(x.double(), 64, 1023)
    with pytest.raises(TypeError, match="float16"):
        rawio.emit(x.half(), 64, 1023)
    with pytest.raises(_lib.YondHipError):
        rawio.ingest(torch.zeros(4, 8), 64, 1023)
    with pytest.raises(ValueError):
        rawio.ingest(x, 64, 1023, out=torch.empty(4, 4, device=DEV))
    p = x.data_ptr()
    assert lib.yond_raw_ingest_u16(p, 0, 64.0, 1.0, 959.0, 0, p, None) == -1
    assert lib.yond_raw_ingest_u16(None, 8, 64.0, 1.0, 959.0, 0, p, None) == -1
    assert lib.yond_raw_ingest_f32(p, 8, 64.0, 1.0, 959.0, 0, None, None) == -1
    assert lib.yond_raw_ingest_f32(p, 0, 64.0, 1.0, 959.0, 0, p, None) == -1
    assert lib.yond_raw_emit_u16(None, 8, 64.0, 959.0, 1.0, 0, p, None, None) == -1
    assert lib.yond_raw_emit_u16(p, 0, 64.0, 959.0, 1.0, 0, p, None, None) == -1
    assert lib.yond_raw_emit_u16(p, 8, 64.0, 959.0, 1.0, 0, None, None, None) == -1
    torch.cuda.synchronize()


def _emit_checked(x, bl, wp, ratio, undo, off_in=0, off_out=0):
    from yond_public_amd import rawio
    d_x = _view(x, off_in)
    buf, out = _out_view(x.shape, torch.uint16, off_out)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    got = rawio.emit(d_x, bl, wp, ratio, undo, out=out, count=count)
    assert got is out and got.dtype == torch.uint16
    want = emit_model(x, bl, wp, ratio, undo)
    g = got.cpu().numpy()
    assert np.array_equal(g, want), (x.shape, bl, wp, ratio, undo, off_in, off_out, int(np.count_nonzero(g != want)))
    assert int(count[0]) == saturated_model(x, bl, wp, ratio, undo), (x.shape, bl, wp, ratio, undo)
    h = buf.cpu().numpy()
    assert (h[:off_out] == 7).all() and (h[off_out + x.size:] == 7).all()


def test_emit_on_uniform_samples():
    """2^22 uniform samples in [-0.1, 1.2] (a fused x * s + bl differs from the two roundings in a handful of them) per black / white level."""
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.1, 1.2, (1 << 11, 1 << 11)).astype(np.float32)
    for bl, wp in LEVELS:
        _emit_checked(x, bl, wp, 3, False)
        _emit_checked(x, bl, wp, 3, True)


def test_emit_near_ties_round_to_even_after_two_roundings():
    """For d + 0.5 at the ends and the middle of the range: the float32 x0 that lands there and its 8 neighbours on each side, every grid
    entry, undo_gain both ways.  A contracted x * s + bl (one rounding) or a round-half-away puts some of these one DN off."""
    ds = [0, 1, 63, 64, 1022, 1023, 16383, 65534, 65535]
    for bl, wp, ratio in GRID:
        for undo in (False, True):
            r = ratio if undo else 1
            x0 = np.array([(d + 0.5 - bl) * r / (wp - bl) for d in ds], np.float64).astype(np.float32)
            cols = [x0]
            lo, hi = x0.copy(), x0.copy()
            for _ in range(8):
                lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
                cols += [lo.copy(), hi.copy()]
            x = np.stack(cols, axis=1).astype(np.float32)                  # [9][17]
            assert x.shape == (9, 17)
            _emit_checked(x, bl, wp, ratio, undo)


def test_emit_specials_and_the_accumulating_counter():
    """Below 0, above 65535, +-inf and NaN: 0 / 65535 / 0, counted; the counter ADDS across launches until the caller resets it; without
    a counter nothing is counted and the values are the same."""
    from yond_public_amd import rawio
    x = np.linspace(-0.5, 1.5, 24 * 40, dtype=np.float32).reshape(24, 40)
    x[0, :8] = [np.nan, np.inf, -np.inf, -1e30, 1e30, 80.0, -3.0, np.nan]
    bl, wp, ratio = 512, 16383, 2
    for undo in (False, True):
        _emit_checked(x, bl, wp, ratio, undo)
    n1, n2 = saturated_model(x, bl, wp, ratio, False), saturated_model(x, bl, wp, ratio, True)
    assert n1 > 8 and n2 > 8 and n1 != n2
    d_x = torch.from_numpy(x).to(DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    a = rawio.emit(d_x, bl, wp, ratio, False, count=count)
    b = rawio.emit(d_x, bl, wp, ratio, True, count=count)
    assert int(count[0]) == n1 + n2
    c = rawio.emit(d_x, bl, wp, ratio, False)
    g = a.cpu().numpy()
    assert np.array_equal(g, c.cpu().numpy()) and not np.array_equal(g, b.cpu().numpy())
    assert g[0, 0] == 0 and g[0, 1] == 65535 and g[0, 2] == 0 and g[0, 3] == 0 and g[0, 4] == 65535 and g[0, 7] == 0
    # every element saturated, over many workgroups: the per-workgroup sums add up to the element count
    big = torch.full((1024, 1030), 100.0, device=DEV)
    count.zero_()
    rawio.emit(big, 0, 65535, 1, count=count)
    assert int(count[0]) == big.numel()


def test_emit_edge_shapes_and_misaligned_views():
    rng = np.random.default_rng(22)
    for si, shape in enumerate(SHAPES):
        x = rng.uniform(-0.2, 1.3, shape).astype(np.float32)
        x.reshape(-1)[si % x.size] = np.nan
        x.reshape(-1)[-1] = np.inf
        for gi, (bl, wp, ratio) in enumerate(GRID):
            for oi, (off_out, off_in) in enumerate(OFFSETS):              # (the uint16 side gets the offsets up to 7)
                if shape == SHAPES[-1] and (gi + oi) % 5:
                    continue
                _emit_checked(x, bl, wp, ratio, bool((gi + oi) & 1), off_in, off_out)
                if shape != SHAPES[-1]:
                    _emit_checked(x, bl, wp, ratio, not ((gi + oi) & 1), off_in, off_out)


def test_round_trip_every_level_on_the_device():
    """emit(ingest(v), undo_gain=True) == v for all uint16 v <= wp, over the grid."""
    from yond_public_amd import rawio
    for bl, wp, ratio in GRID:
        v = np.arange(0, int(wp) + 1, dtype=np.uint16).reshape(1, -1)
        count = torch.zeros(1, dtype=torch.int64, device=DEV)
        back = rawio.emit(rawio.ingest(torch.from_numpy(v).to(DEV), bl, wp, ratio), bl, wp, ratio, undo_gain=True, count=count)
        assert np.array_equal(back.cpu().numpy(), v), (bl, wp, ratio)
        assert int(count[0]) == 0


def _write_frames(root, n, H, W, bl, wp, dtype=np.uint16, seed0=60):
    import yond_oracle as O
    os.makedirs(root / "gt")
    for k in range(n):
        noisy, clean = O.synth_noisy(H, W, 2.0, 12.0, seed0 + k, clip=False)
        np.save(root / f"f{k}.npy", np.clip(np.round(noisy * (wp - bl) * 0.5 + bl), 0, 65535).astype(dtype))        # half exposure: ratio 2 restores it
        np.save(root / "gt" / f"f{k}.npy", np.clip(np.round(clean * (wp - bl) + bl), 0, 65535).astype(dtype))


def test_prefetcher_device_ingest_equals_the_host_upload(tmp_path):
    """Prefetcher(ingest=True), two workers, four uint16 frames: 'lr' / 'hr' are float32 device tensors, bit-equal to the default mode's
    upload (NumPy on the host, float32 over the bus), in order; the raw arrays do not travel on in the item."""
    from yond_public_amd.data import Any_Dataset, Prefetcher
    _write_frames(tmp_path, 4, 64, 96, 63, 1023)
    ds = Any_Dataset({'root_dir': str(tmp_path), 'bl': 63, 'wp': 1023, 'clip': False})
    ds.change_eval_ratio(2)
    want = [(k, d) for k, d in Prefetcher(ds, range(4), DEV, upload=('lr', 'hr'), workers=2)]
    ds.raw_items = True
    assert ds[0]['lr_raw'].dtype == np.uint16
    busy = torch.zeros(1 << 22, device=DEV)
    seen = []
    for (k, d), (kw, w) in zip(Prefetcher(ds, range(4), DEV, upload=('lr', 'hr'), workers=2, ingest=True), want):
        busy.add_(1.0)
        seen.append(k)
        assert k == kw and d['name'] == w['name'] and 'lr_raw' not in d and 'hr_raw' not in d
        for key in ('lr', 'hr'):
            assert d[key].is_cuda and d[key].dtype == torch.float32 and d[key].shape == (64, 96)
            assert torch.equal(d[key], w[key]), (k, key)
    assert seen == [0, 1, 2, 3]
    ds.raw_items = False
    assert float(want[0][1]['lr'].max()) > 0.3                       # (real frames, not zeros)


def test_frame_writer_on_device_tensors(tmp_path):
    """put queues emit + copy on the current stream: the caller overwrites its buffer right behind put, the files hold the frame as it was."""
    from yond_public_amd.rawio import FrameWriter
    rng = np.random.default_rng(8)
    frames = [rng.uniform(-0.2, 1.2, (70, 90)).astype(np.float32) for _ in range(6)]
    for mode in ('dn16', 'f32'):
        buf = torch.empty(70, 90, device=DEV)
        with FrameWriter(tmp_path / mode, mode, workers=2, depth=3) as w:
            for k, f in enumerate(frames):
                buf.copy_(torch.from_numpy(f))
                w.put(f"f{k}", buf, (64, 1023, 2), {'rounds': [(2.0, 12.0)]})
                buf.fill_(float('nan'))
        for k, f in enumerate(frames):
            arr, side = np.load(tmp_path / mode / f"f{k}.npy"), json.load(open(tmp_path / mode / f"f{k}.json"))
            if mode == 'dn16':
                assert arr.dtype == np.uint16 and np.array_equal(arr, emit_model(f, 64, 1023, 2)) and side['saturated'] == saturated_model(f, 64, 1023, 2)
            else:
                assert arr.dtype == np.float32 and np.array_equal(arr, f) and side['saturated'] is None
            assert side['gain_kept'] is True and side['rounds'] == [[2.0, 12.0]]


def test_full_frame_driver_device_ingest_and_save(tmp_path, monkeypatch):
    """YOND_Full on two 192 x 320 uint16 frames (+ gt/), ratio 2: device ingest (the default) against --host-ingest -- the same count, round-1
    estimates to rtol 1e-9 and PSNR within 2e-3 dB, the bounds test_yond_any_full_frame_driver holds between its own two runs (the
    estimator's atomics are not bit-reproducible) -- and --save dn16 / f32: one .npy + .json per frame, equal to emit_model of / to the very
    tensor the writer was given (captured by on_result)."""
    from test_hip_eval import _small_full_runfile
    from yond_public_amd import YOND_full as Y
    monkeypatch.chdir(tmp_path)
    frames = tmp_path / "frames"
    H, W, bl, wp = 192, 320, 63, 1023
    _write_frames(frames, 2, H, W, bl, wp)
    rf = _small_full_runfile(tmp_path, "ANY_simple+full_pre_grumix.yml", frames, nf=8, H=H, W=W, ratio_list=[2])
    drv = Y.YOND_Full(['-f', rf, '-m', 'eval', '--save', 'dn16'])
    assert type(drv.dst_eval).__name__ == 'Any_Dataset' and len(drv.dst_eval) == 2
    captured = {}
    drv.on_result = lambda name, res: captured.__setitem__(name, res['raw_dns'][-1].clone())
    red = drv.eval(-1)['x2']
    assert red['count'] == 2 and drv.dst_eval.raw_items is True
    dev_metrics = {k: dict(v) for k, v in drv.metrics.items()}
    out_dir = tmp_path / "images" / drv.method_name
    assert sorted(os.listdir(out_dir)) == ['f0_x02.json', 'f0_x02.npy', 'f1_x02.json', 'f1_x02.npy']
    for name in ('f0_x02', 'f1_x02'):
        arr, side = np.load(out_dir / f"{name}.npy"), json.load(open(out_dir / f"{name}.json"))
        x = captured[name].cpu().numpy()
        assert arr.dtype == np.uint16 and arr.shape == (H, W)
        assert np.array_equal(arr, emit_model(x, bl, wp, 2))
        assert side['saturated'] == saturated_model(x, bl, wp, 2)
        assert (side['bl'], side['wp'], side['ratio'], side['gain_kept']) == (63.0, 1023.0, 2.0, True)
        assert len(side['rounds']) == 2 and all(len(r) == 2 for r in side['rounds'])
        assert all(np.isfinite(r).all() for r in side['rounds'])
    # --save f32: the file is the captured tensor
    drv.parser.save = 'f32'
    captured.clear()
    drv.eval(-1)
    for name in ('f0_x02', 'f1_x02'):
        arr = np.load(out_dir / f"{name}.npy")
        assert arr.dtype == np.float32 and np.array_equal(arr, captured[name].cpu().numpy())
        assert json.load(open(out_dir / f"{name}.json"))['saturated'] is None
    # the host path, as before this change
    host = Y.YOND_Full(['-f', rf, '-m', 'eval', '--host-ingest'])
    red_h = host.eval(-1)['x2']
    assert host.dst_eval.raw_items is False and red_h['count'] == red['count'] == 2
    assert abs(red_h['psnr_last'] - red['psnr_last']) < 2e-3
    for k, mh in host.metrics.items():
        md = dev_metrics[k]
        assert len(mh['reg']) == len(md['reg'])
        np.testing.assert_allclose(np.asarray(mh['reg'][0], np.float64), np.asarray(md['reg'][0], np.float64), rtol=1e-9)
        assert abs(mh['psnr'][-1] - md['psnr'][-1]) < 2e-3
    assert sorted(os.listdir(out_dir)) == ['f0_x02.json', 'f0_x02.npy', 'f1_x02.json', 'f1_x02.npy']      # --save none wrote nothing new


def test_yond_sidd_save_f32_writes_the_reference_cache(tmp_path, monkeypatch):
    """YOND_SIDD --synthetic 1 --save f32: npy/<method>/000.npy, float32 [max_iter + 1][256][8192] (YOND_SIDD.py:512-536), equal to the rounds
    the driver produced."""
    from yond_public_amd import YOND_SIDD as Y
    monkeypatch.chdir(tmp_path)
    rf = os.path.join(ROOT, "runfiles", "YOND", "SIDD_simple+full_pre_grumix.yml")
    trainer = Y.YOND_SIDD(['-f', rf, '-m', 'eval', '--synthetic', '1', '--save', 'f32'])
    rounds = {}
    trainer.on_result = lambda name, res: rounds.__setitem__(name, [dn.clone() for dn in res['raw_dns']])
    red = trainer.eval(-1)
    assert red['count'] == 1 and len(rounds) == 1
    out = np.load(tmp_path / "npy" / trainer.method_name / "000.npy")
    n_it = trainer.pipe['max_iter'] + 1
    assert out.dtype == np.float32 and out.shape == (n_it, 256, 8192)
    dns = next(iter(rounds.values()))
    assert 1 <= len(dns) <= n_it
    for it in range(n_it):
        want = dns[it].cpu().numpy() if it < len(dns) else np.zeros((256, 8192), np.float32)
        assert np.array_equal(out[it], want), it
    assert float(np.abs(out[0]).max()) > 0
