"""CPU: the host side of the raw DN <-> [0, 1] ends (yond_public_amd/rawio.py, the datasets' raw_items mode, _PinnedPool by dtype):
the NumPy model's round trip, raw items + the model against today's items, the FrameWriter on host tensors, the pinned pool's eviction."""
import json
import os
import threading

import numpy as np
import pytest
import torch

from rawio_model import GRID, emit_model, ingest_model, saturated_model


def test_model_round_trip_over_the_level_grid():
    """emit(ingest(v), undo_gain) == v for every uint16 v <= wp, for every (bl, wp) x ratio of the grid; and rawio's host forms are
    the model."""
    from yond_public_amd import rawio
    for bl, wp, ratio in GRID:
        v = np.arange(0, int(wp) + 1, dtype=np.uint16)
        x = ingest_model(v, bl, wp, ratio)
        back = emit_model(x, bl, wp, ratio, undo_gain=True)
        assert np.array_equal(back, v), (bl, wp, ratio, int(np.count_nonzero(back != v)))
        assert np.array_equal(rawio.ingest_host(v, bl, wp, ratio), x)
        got, bad = rawio.emit_host(x, bl, wp, ratio, undo_gain=True)
        assert np.array_equal(got, v) and bad == saturated_model(x, bl, wp, ratio, True)


def test_host_forms_on_special_values():
    from yond_public_amd import rawio
    x = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 0.5, 1.0, 80.0, -1e30, 1e30], np.float32)
    for undo in (False, True):
        got, bad = rawio.emit_host(x, 64, 1023, 3, undo)
        assert np.array_equal(got, emit_model(x, 64, 1023, 3, undo)) and bad == saturated_model(x, 64, 1023, 3, undo)
    assert got[0] == 0 and got[1] == 65535 and got[2] == 0
    raw = np.array([np.nan, np.inf, -5.0, 64.0, 1023.0, 2000.0], np.float32)
    for clip in (False, True):
        assert np.array_equal(rawio.ingest_host(raw, 64, 1023, 2, clip), ingest_model(raw, 64, 1023, 2, clip), equal_nan=True)
    assert np.isnan(rawio.ingest_host(raw, 64, 1023, 2, True)[0])               # np.clip hands a NaN on


def _check_raw_items(ds, keys):
    """Every item of `ds`: raw_items mode + the model == the default mode, bit for bit; everything else in the item unchanged."""
    for k in range(len(ds)):
        ds.raw_items = False
        want = ds[k]
        ds.raw_items = True
        item = ds[k]
        ds.raw_items = False
        for key in keys:
            if key not in want:
                assert key + '_raw' not in item
                continue
            assert key not in item
            raw = item[key + '_raw']
            bl, wp, ratio, clip = item[key + '_levels']
            assert np.array_equal(ingest_model(raw, bl, wp, ratio, clip), want[key]), (k, key)
            assert want[key].dtype == np.float32
        for key in set(want) - set(keys):
            a, b = want[key], item[key]
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, key
    return item


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.int32])
@pytest.mark.parametrize("clip", [False, True])
def test_raw_items_plus_model_equal_the_default_items(tmp_path, monkeypatch, dtype, clip):
    """ELD, LRID and ANY on miniature trees of uint16 / float32 files (int32: converted to float32): 'lr_raw' / 'hr_raw' are the files as
    np.load returns them, and ingest_model of them with the item's levels is the default mode's 'lr' / 'hr'."""
    from yond_public_amd.data import Any_Dataset, ELD_Full_Dataset, LRID_Dataset
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(11)
    keep = np.float32 if dtype == np.int32 else dtype

    def frame(lo, hi, shape):
        return rng.integers(lo, hi, shape).astype(dtype)
    # ELD
    root = tmp_path / "ELD"
    d = root / "SonyA7S2" / "scene-1"
    os.makedirs(d)
    json.dump({"bl": 512, "wp": 16383}, open(root / "SonyA7S2" / "meta.json", "w"))
    for img in range(1, 17):
        np.save(d / f"IMG_{img:04d}.npy", frame(480, 17000, (12, 20)))
    ds = ELD_Full_Dataset({'root_dir': str(root), 'clip': clip})
    for ratio in (1, 100, 200):
        ds.change_eval_ratio('SonyA7S2', ratio=ratio)
        assert len(ds) == 3
        item = _check_raw_items(ds, ('lr', 'hr'))
        assert item['lr_raw'].dtype == keep and item['lr_levels'] == (512.0, 16383.0, ratio, clip) and item['hr_levels'][2] == 1
    # LRID
    root = tmp_path / "LRID"
    for i in LRID_Dataset.get_eval_id('indoor_x5')[:2]:
        d = root / "indoor_x5" / f"{i:03d}"
        os.makedirs(d)
        np.save(d / "gt.npy", frame(50, 1100, (10, 14)))
        for r in (1, 3):
            np.save(d / f"x{r:02d}.npy", frame(50, 600, (10, 14)))
    ds = LRID_Dataset({'root_dir': str(root), 'dstname': ['indoor_x5'], 'bl': 63.5, 'wp': 1023, 'clip': clip})
    for ratio in (1, 3):
        ds.change_eval_ratio(ratio)
        assert len(ds) == 2
        item = _check_raw_items(ds, ('lr', 'hr'))
        assert item['hr_raw'].dtype == keep
    # ANY (one frame without a reference)
    frames = tmp_path / "frames"
    os.makedirs(frames / "gt")
    for k in range(2):
        np.save(frames / f"f{k}.npy", frame(40, 1100, (6, 10)))
    np.save(frames / "gt" / "f1.npy", frame(40, 1100, (6, 10)))
    ds = Any_Dataset({'root_dir': str(frames), 'bl': 64, 'wp': 1023, 'clip': clip})
    ds.change_eval_ratio(10)
    item = _check_raw_items(ds, ('lr', 'hr'))
    assert item['lr_raw'].dtype == keep and 'hr_raw' in item
    ds.raw_items = True
    assert 'hr_raw' not in ds[0] and 'lr' not in ds[0]


def test_prefetcher_ingest_on_the_host(tmp_path):
    """Prefetcher(ingest=True) without a GPU: the raw items through rawio.ingest_host, equal to the default mode, in order."""
    from yond_public_amd.data import Any_Dataset, Prefetcher
    rng = np.random.default_rng(5)
    os.makedirs(tmp_path / "gt")
    for k in range(4):
        np.save(tmp_path / f"f{k}.npy", rng.integers(0, 1200, (8, 12)).astype(np.uint16))
        np.save(tmp_path / "gt" / f"f{k}.npy", rng.integers(0, 1200, (8, 12)).astype(np.uint16))
    ds = Any_Dataset({'root_dir': str(tmp_path), 'bl': 64, 'wp': 1023, 'clip': False})
    ds.change_eval_ratio(3)
    want = [d for _, d in Prefetcher(ds, range(4), 'cpu', upload=('lr', 'hr'), workers=2)]
    ds.raw_items = True
    got = list(Prefetcher(ds, range(4), 'cpu', upload=('lr', 'hr'), workers=2, ingest=True))
    assert [k for k, _ in got] == [0, 1, 2, 3]
    for (k, d), w in zip(got, want):
        assert d['name'] == w['name'] and 'lr_raw' not in d
        for key in ('lr', 'hr'):
            assert d[key].dtype == torch.float32 and torch.equal(d[key], w[key])


def test_prefetcher_relays_a_worker_that_cannot_make_its_stream(monkeypatch):
    """A loader thread whose copy stream cannot be created (no usable device) hands the error to the consumer at its first item instead of
    dying and leaving the consumer waiting."""
    from yond_public_amd.data import Prefetcher

    def no_stream(*a, **k):
        raise RuntimeError("no device for this stream")
    monkeypatch.setattr(torch.cuda, 'Stream', no_stream)
    items = [{'lr': np.zeros((2, 2), np.float32), 'name': f'i{k}'} for k in range(3)]
    got = []

    def consume():
        try:
            got.append(list(Prefetcher(items, range(3), 'cuda:0', workers=2)))
        except BaseException as e:                                  # noqa: BLE001
            got.append(e)
    t = threading.Thread(target=consume, daemon=True)
    t.start()
    t.join(10)                                                      # (returns at once when the error is relayed)
    assert not t.is_alive(), "the consumer is still waiting for a worker that died"
    assert isinstance(got[0], RuntimeError) and "no device for this stream" in str(got[0])


@pytest.mark.parametrize("mode", ["dn16", "f32"])
def test_frame_writer_on_host_tensors(tmp_path, mode):
    from yond_public_amd.rawio import FrameWriter
    rng = np.random.default_rng(2)
    frames = [torch.from_numpy(rng.uniform(-0.4, 1.2, (10, 14)).astype(np.float32)) for _ in range(5)]
    frames[1][0, 0], frames[1][0, 1] = float('nan'), float('inf')
    kept = [f.clone() for f in frames]
    w = FrameWriter(tmp_path / "out", mode, workers=2, depth=2)
    for k, f in enumerate(frames):
        w.put(f"f{k}", f, (64, 1023, 2), {'rounds': [(2.0, 12.0), (2.1, 11.5)]})
        f.zero_()                                                   # the caller reuses its buffer: the writer kept no reference
    w.close()
    assert w.written == 5
    for k, f in enumerate(kept):
        arr = np.load(tmp_path / "out" / f"f{k}.npy")
        side = json.load(open(tmp_path / "out" / f"f{k}.json"))
        if mode == 'dn16':
            assert arr.dtype == np.uint16 and np.array_equal(arr, emit_model(f.numpy(), 64, 1023, 2))
            assert side['saturated'] == saturated_model(f.numpy(), 64, 1023, 2) and side['saturated'] > 0
        else:
            assert arr.dtype == np.float32 and np.array_equal(arr, f.numpy(), equal_nan=True) and side['saturated'] is None
        assert (side['bl'], side['wp'], side['ratio'], side['gain_kept']) == (64.0, 1023.0, 2.0, True)
        assert side['rounds'] == [[2.0, 12.0], [2.1, 11.5]] and side['shape'] == [10, 14]
    with pytest.raises(RuntimeError):
        w.put("late", kept[0], (64, 1023, 2))
    with pytest.raises(ValueError):
        FrameWriter(tmp_path / "out", "png")


def test_frame_writer_undo_gain_round_trip(tmp_path):
    from yond_public_amd.rawio import FrameWriter
    v = np.arange(0, 1024, dtype=np.uint16).reshape(16, 64)
    with FrameWriter(tmp_path, 'dn16', undo_gain=True) as w:
        w.put("v", torch.from_numpy(ingest_model(v, 64, 1023, 200)), (64, 1023, 200))
    assert np.array_equal(np.load(tmp_path / "v.npy"), v)
    assert json.load(open(tmp_path / "v.json"))['gain_kept'] is False


def test_frame_writer_blocks_at_depth(tmp_path):
    """`depth` frames in flight: the next put has no slot until a write has finished (timeout=0: it says so at once instead of waiting)."""
    from yond_public_amd.rawio import FrameWriter
    gate, entered = threading.Event(), threading.Semaphore(0)
    w = FrameWriter(tmp_path, 'f32', workers=2, depth=3)
    write = w._write

    def held(name, arr, side):
        entered.release()
        gate.wait()
        write(name, arr, side)
    w._write = held
    x = torch.zeros(4, 6)
    for k in range(3):
        w.put(f"a{k}", x, (0, 1, 1), timeout=0)
    entered.acquire()
    entered.acquire()                                               # both workers sit in their writes; the third frame waits in the queue
    with pytest.raises(TimeoutError):
        w.put("a3", x, (0, 1, 1), timeout=0)
    gate.set()
    w.put("a3", x, (0, 1, 1))                                       # blocks until a slot is free
    w.close()
    assert sorted(os.listdir(tmp_path)) == sorted([f"a{k}.{e}" for k in range(4) for e in ("npy", "json")])


def test_frame_writer_surfaces_a_failed_write(tmp_path):
    """A writer thread's exception (the directory became a file's child: not writable for any user) is re-raised by close(), and by the
    next put."""
    from yond_public_amd.rawio import FrameWriter
    w = FrameWriter(tmp_path / "out", 'dn16')
    w.out_dir = str(tmp_path / "out" / "missing" / "dir")           # np.save cannot create it
    w.put("f0", torch.zeros(4, 4), (64, 1023, 1))
    with pytest.raises(OSError):
        w.close()
    w2 = FrameWriter(tmp_path / "out2", 'f32', workers=1, depth=1)
    w2.out_dir = str(tmp_path / "out2" / "missing")
    w2.put("f0", torch.zeros(4, 4), (64, 1023, 1))
    w2._free.put(w2._free.get())                                    # (the slot is back: the failed write has been handled)
    with pytest.raises(OSError):
        w2.put("f1", torch.zeros(4, 4), (64, 1023, 1))
    w2.close()


def test_pinned_pool_counts_bytes_by_dtype_and_evicts_by_identity(monkeypatch):
    """Three shapes, two buffers each, uint16 and float32 keys, a budget that holds four of the six and one small one: eviction drops the least recently used
    idle buffer (list.remove on dicts of tensors used to compare tensors and raise), `bytes` stays the sum over the live buffers."""
    from yond_public_amd.data import _PinnedPool
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, *a, **k: self)
    shapes = [('lr_raw', (8, 16), torch.uint16), ('lr', (8, 16), torch.float32), ('hr_raw', (4, 16), torch.uint16)]     # 256, 512, 128 bytes
    pool = _PinnedPool(budget=2 * 256 + 2 * 512 + 128)

    def live_bytes():
        return sum(b['t'].numel() * b['t'].element_size() for lst in pool.bufs.values() for b in lst)
    held = []
    for key, shape, dt in shapes[:2]:
        a, b = pool.take(key, shape, dt), pool.take(key, shape, dt)
        assert a is not b and a['t'].dtype == dt and tuple(a['t'].shape) == shape
        held += [a, b]
    assert pool.bytes == live_bytes() == 1536
    assert pool.take('lr', (8, 16))['t'].dtype == torch.float32     # (the default dtype; all 'lr' buffers busy: a third one, over budget, nothing idle)
    third = pool.bufs[('lr', (8, 16), torch.float32)][2]
    assert pool.bytes == live_bytes() == 2048
    for b in held + [third]:
        pool.give(b, None)
    # everything idle, 2048 bytes held; two 128-byte buffers of a new shape: the least recently used idle ones go, oldest first
    c = pool.take('hr_raw', (4, 16), torch.uint16)
    assert pool.bytes == live_bytes() and pool.bytes <= pool.budget
    assert all(q is not held[0] and q is not held[1] for lst in pool.bufs.values() for q in lst)     # the two uint16 'lr_raw' buffers were the oldest
    assert any(q is held[2] for q in pool.bufs[('lr', (8, 16), torch.float32)])
    d = pool.take('hr_raw', (4, 16), torch.uint16)
    assert c is not d and pool.bytes == live_bytes() and pool.bytes <= pool.budget
    pool.give(c, None)
    assert pool.take('hr_raw', (4, 16), torch.uint16) is c          # an idle buffer of the shape is handed out again
    assert pool.bytes == live_bytes()
