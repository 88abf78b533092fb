"""The two ends of a full-frame run on the device (csrc/rawio.hip, include/yond_hip.h R2 / R3):

    ingest   raw DN (uint16 or float32, as the camera / np.load gave them) -> the [0, 1] scale the pipeline works on,
             out = ((float32)raw - bl) * ratio / (wp - bl), bit-equal to the host expression of data.py's full-frame datasets
    emit     the inverse, back to uint16 DN: rint(clip(x * (wp - bl) [/ ratio] + bl, 0, 65535)), with a saturation count
    FrameWriter   results to disk behind the GPU: emit + device-to-host copy into a pinned ring on the caller's stream, the files
             written by background threads

`ingest_host` / `emit_host` state the same arithmetic in NumPy (what the kernels are tested against, and what the writer and
the loader use for HOST tensors: a CPU box has no kernel to call).  Device tensors always go through the kernels.
"""
import json
import os
import queue
import threading

import numpy as np
import torch

from . import _lib


def _scalars(bl, wp, ratio):
    """The three float32 constants as NumPy forms them from the Python scalars of data.py: wp - bl in double first."""
    return np.float32(bl), np.float32(ratio), np.float32(float(wp) - float(bl))


def ingest_host(raw, bl, wp, ratio=1, clip=False):
    """NumPy statement of ingest (three float32 roundings: subtract, multiply, divide)."""
    b, r, s = _scalars(bl, wp, ratio)
    x = (np.asarray(raw).astype(np.float32) - b) * r / s
    return x.clip(0, 1) if clip else x


def emit_host(x, bl, wp, ratio=1, undo_gain=False):
    """NumPy statement of emit -> (uint16 DN, number of elements that were NaN or clamped at either end)."""
    b, r, s = _scalars(bl, wp, ratio)
    with np.errstate(invalid='ignore', over='ignore'):
        y = np.asarray(x).astype(np.float32) * s
        if undo_gain:
            y = y / r
        y = y + b
        bad = int(np.count_nonzero(np.isnan(y) | (y < 0) | (y > 65535)))
        y = np.where(np.isnan(y), np.float32(0), y)
        return np.rint(np.clip(y, np.float32(0), np.float32(65535))).astype(np.uint16), bad


def _flat_device(t, name, dtypes):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.YondHipError(f"{name} must be a tensor on a ROCm device (the HIP path has no CPU fallback; ingest_host / emit_host are the NumPy forms)")
    if t.dtype not in dtypes:
        raise TypeError(f"{name}: dtype {t.dtype} is not supported (expected {' or '.join(str(d) for d in dtypes)})")
    if t.dim() not in (2, 3):
        raise ValueError(f"{name} must be [H][W] or [B][H][W], got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise _lib.YondHipError(f"{name} must be contiguous")
    return t


def ingest(raw, bl, wp, ratio=1, clip=False, out=None):
    """Device uint16 / float32 DN [H][W] or [B][H][W] -> device float32 of the same shape, on the current stream."""
    _flat_device(raw, 'raw', (torch.uint16, torch.float32))
    if out is None:
        out = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    else:
        _flat_device(out, 'out', (torch.float32,))
        if out.shape != raw.shape or out.device != raw.device:
            raise ValueError(f"out {tuple(out.shape)} on {out.device} does not match raw {tuple(raw.shape)} on {raw.device}")
    b, r, s = _scalars(bl, wp, ratio)
    lib = _lib.load()
    fn = lib.yond_raw_ingest_u16 if raw.dtype == torch.uint16 else lib.yond_raw_ingest_f32
    with torch.cuda.device(raw.device):
        _lib.check(fn(_lib.ptr(raw), raw.numel(), float(b), float(r), float(s), int(bool(clip)), _lib.ptr(out), _lib.stream()), fn.__name__)
    return out


def emit(x, bl, wp, ratio=1, undo_gain=False, out=None, count=None):
    """Device float32 [H][W] or [B][H][W] -> device uint16 DN of the same shape, on the current stream.  `count`: an optional device
    int64 tensor of one element to which the launch ADDS the number of elements that were NaN or clamped (zero it for a per-call count)."""
    _flat_device(x, 'x', (torch.float32,))
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint16, device=x.device)
    else:
        _flat_device(out, 'out', (torch.uint16,))
        if out.shape != x.shape or out.device != x.device:
            raise ValueError(f"out {tuple(out.shape)} on {out.device} does not match x {tuple(x.shape)} on {x.device}")
    if count is not None and not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int64 and count.numel() == 1
                                  and count.device == x.device):
        raise ValueError("count must be a device int64 tensor of one element on x's device")
    b, r, s = _scalars(bl, wp, ratio)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.yond_raw_emit_u16(_lib.ptr(x), x.numel(), float(b), float(s), float(r), int(bool(undo_gain)), _lib.ptr(out),
                                         _lib.ptr(count), _lib.stream()), 'yond_raw_emit_u16')
    return out


class FrameWriter:
    """Results to `<out_dir>/<name>.npy` (+ `<name>.json`) without stalling the GPU loop.

    put(name, frame, levels, info) queues, on the CURRENT stream and before it returns, everything that reads `frame`: for
    mode 'dn16' the emit launch (uint16 DN, the digital gain kept unless undo_gain), for both modes the device-to-host copy into a
    pinned buffer of a ring of `depth` slots, then an event.  The stream drivers reuse their output buffers, so the writer keeps no
    reference to `frame`.  One of `workers` background threads waits for the event and writes the files.  put blocks while `depth`
    frames are in flight (timeout: seconds to wait for a free slot, then TimeoutError); an exception of a writer thread is re-raised
    by the next put or by close(), which drains the queue.
      levels  (bl, wp, ratio[, ...]);  info  {'rounds': [(K, sigma), ...], ...}: JSON-able extras kept in the sidecar
      sidecar bl, wp, ratio, gain_kept, rounds, saturated (NaN or clamped elements; None for 'f32'), mode, shape
    Host tensors take the NumPy forms (emit_host) inside put."""

    def __init__(self, out_dir, mode, workers=2, depth=4, undo_gain=False):
        if mode not in ('dn16', 'f32'):
            raise ValueError(f"FrameWriter mode {mode!r}: expected 'dn16' or 'f32'")
        self.out_dir, self.mode, self.undo_gain, self.depth = str(out_dir), mode, bool(undo_gain), max(1, int(depth))
        os.makedirs(self.out_dir, exist_ok=True)
        self._slots = [{'host': None, 'dev': None, 'count': None, 'count_host': None} for _ in range(self.depth)]
        self._free = queue.Queue()
        for i in range(self.depth):
            self._free.put(i)
        self._jobs = queue.Queue()
        self._err, self._closed, self.written = None, False, 0
        self._threads = [threading.Thread(target=self._work, daemon=True) for _ in range(max(1, int(workers)))]
        for t in self._threads:
            t.start()

    # -- the caller's side ------------------------------------------------------------------------
    def _raise(self):
        if self._err is not None:
            err, self._err = self._err, None
            raise err

    def put(self, name, frame, levels, info=None, timeout=None):
        if self._closed:
            raise RuntimeError("FrameWriter.put after close()")
        self._raise()
        bl, wp, ratio = float(levels[0]), float(levels[1]), float(levels[2])
        if not isinstance(frame, torch.Tensor):
            frame = torch.from_numpy(np.ascontiguousarray(frame, np.float32))
        if frame.dtype != torch.float32:
            raise TypeError(f"FrameWriter.put: dtype {frame.dtype} is not supported (expected torch.float32)")
        try:
            i = self._free.get(timeout=timeout)
        except queue.Empty:
            raise TimeoutError(f"FrameWriter: {self.depth} frames in flight") from None
        slot = self._slots[i]
        try:
            side = {'bl': bl, 'wp': wp, 'ratio': ratio, 'gain_kept': not self.undo_gain, 'mode': self.mode, 'shape': list(frame.shape),
                    'saturated': None}
            for k, v in (info or {}).items():
                side[k] = [[float(a) for a in r] for r in v] if k == 'rounds' else v
            side.setdefault('rounds', [])
            if not frame.is_cuda:                                   # host tensor: the NumPy forms, nothing kept of `frame`
                if self.mode == 'dn16':
                    arr, side['saturated'] = emit_host(frame.numpy(), bl, wp, ratio, self.undo_gain)
                else:
                    arr = frame.numpy().copy()
                job = (i, name, arr, None, side)
            else:
                frame = frame.contiguous()
                want = torch.uint16 if self.mode == 'dn16' else torch.float32
                if slot['host'] is None or slot['host'].shape != frame.shape or slot['host'].dtype != want:
                    slot['host'] = torch.empty(frame.shape, dtype=want).pin_memory()
                    slot['dev'] = torch.empty(frame.shape, dtype=want, device=frame.device) if self.mode == 'dn16' else None
                if self.mode == 'dn16':
                    if slot['count'] is None or slot['count'].device != frame.device:
                        slot['count'] = torch.zeros(1, dtype=torch.int64, device=frame.device)
                        slot['count_host'] = torch.zeros(1, dtype=torch.int64).pin_memory()
                    slot['count'].zero_()
                    x = frame if frame.dim() in (2, 3) else frame.reshape(-1, frame.shape[-1])
                    emit(x, bl, wp, ratio, self.undo_gain, out=slot['dev'].view(x.shape), count=slot['count'])
                    slot['host'].copy_(slot['dev'], non_blocking=True)
                    slot['count_host'].copy_(slot['count'], non_blocking=True)
                else:
                    slot['host'].copy_(frame, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(frame.device))
                job = (i, name, None, ev, side)
        except BaseException:
            self._free.put(i)
            raise
        self._jobs.put(job)

    def close(self):
        """Wait for every queued frame to be on disk, stop the threads, re-raise a writer thread's exception."""
        if not self._closed:
            self._closed = True
            for _ in self._threads:
                self._jobs.put(None)
            for t in self._threads:
                t.join()
        self._raise()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.close()
        else:                                                      # (keep the caller's exception)
            try:
                self.close()
            except BaseException:                                  # noqa: BLE001
                pass

    # -- the writer threads -----------------------------------------------------------------------
    def _write(self, name, arr, side):
        np.save(os.path.join(self.out_dir, f'{name}.npy'), arr)
        with open(os.path.join(self.out_dir, f'{name}.json'), 'w') as f:
            json.dump(side, f)

    def _work(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            i, name, arr, ev, side = job
            try:
                if ev is not None:
                    ev.synchronize()
                    slot = self._slots[i]
                    arr = slot['host'].numpy()
                    if self.mode == 'dn16':
                        side['saturated'] = int(slot['count_host'][0])
                self._write(name, arr, side)
                self.written += 1
            except BaseException as e:                             # noqa: BLE001 -- handed to the caller
                if self._err is None:
                    self._err = e
            finally:
                self._free.put(i)
