"""I4 measurement: raw training batches cut from resident frames (yond_rawcrop_f32, csrc/rawcrop.hip) at the SID runfile's shape --
one batch of 64 patches of 4 x 128 x 128 from 8 resident 2848 x 4256 uint16 frames, 8 crops each.
    python tools/rawcrop_bench.py [--iters 100] [--out profiles/rawcrop_bench.json]
Prints one JSON line:
  - pattern0..3, mixed: median of event-timed launches (after warm-up) with every frame under that Bayer rotation (mixed: the
    planner's own draws), and the 10 B per element the launch moves (2 in, 8 out) over that time as GB/s and a share of 6.3 TB/s;
  - img2raw_uint8: yond_img2raw_f32 on the same box at the same output shape (tools/img2raw_bench.py's kernel_time), the yardstick;
  - host_numpy_ms: the same items through the NumPy expression of tests/rawcrop_model.py plus standard_normal noise, one thread;
  - host_plan_ms: the host's per-batch work (the draws of 8 frames + the patch array), median;
  - clock_mhz: the shader clock the chip held (yond_clock_probe)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np
import torch

import __graft_entry__ as G
import img2raw_bench as IB
import rawcrop_model as M
from yond_public_amd import _lib
from yond_public_amd import img2raw as I
from yond_public_amd import rawcrop as R

DEV = "cuda:0"
HBM_TBS = 6.3
H, W, PS, CPI, NF = 2848, 4256, 128, 8, 8
BL, WP = 512., 16383.


def items_of(gen, pattern=None):
    out = []
    while len(out) < NF:
        it = R.sample_item(gen, H // 2, W // 2, PS, CPI, "random", 5, 50, wb=(2.0, 1.0, 1.6))
        if pattern is None or it["pattern"] == pattern:
            out.append(it)
    return out


def kernel_time(cache, items, key, iters):
    p = R.plan(cache.offsets(np.arange(NF)), items, H, W, PS, key, np.arange(NF * CPI))
    B = len(p)
    hr = torch.empty((B, 4, PS, PS), device=DEV)
    lr, sig = torch.empty_like(hr), torch.empty(B, device=DEV)
    lib = _lib.load()
    args = (C.c_void_p(cache.buf.data_ptr()), cache.buf.numel(), 0, H, W, BL, WP, C.c_void_p(p.ctypes.data), B, PS, 1, _lib.ptr(hr),
            _lib.ptr(lr), _lib.ptr(sig), _lib.stream())
    for _ in range(20):
        _lib.check(lib.yond_rawcrop_f32(*args), "yond_rawcrop_f32")
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        lib.yond_rawcrop_f32(*args)
        b.record()
    torch.cuda.synchronize()
    us = float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))
    nbytes = hr.numel() * 10
    return {"us": round(us, 2), "bytes": int(nbytes), "GBs": round(nbytes / us * 1e-3, 1), "hbm_share": round(nbytes / us * 1e-6 / HBM_TBS, 3)}


def host_numpy(frames, items, reps=2):
    rng = np.random.default_rng(0)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for f, it in zip(frames, items):
            hr = M.patches_hr(f, BL, WP, it["pattern"], it["vst_aug"], it["y0"], it["x0"], PS, it["rgb_gain"], it["gain0"], it["gain2"])
            lr = hr + rng.standard_normal(hr.shape) * it["sigma"]
            lr, hr = lr.clip(0, 1), hr.clip(0, 1)
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rawcrop_bench needs an MI355X"
    G.build()
    res = {"clock_mhz_before": round(IB.clock_mhz()), "shape": [NF * CPI, 4, PS, PS], "frames": [NF, H, W]}
    rng = np.random.default_rng(0)
    frames = [rng.integers(300, 16600, (H, W)).astype(np.uint16) for _ in range(NF)]
    cache = R.FrameCache([f"frame{i}" for i in range(NF)], DEV, frames=frames)
    gen, key = I.train_streams(1, 0)
    for k in range(4):
        res[f"pattern{k}"] = kernel_time(cache, items_of(gen, k), key, a.iters)
    mixed = items_of(gen)
    res["mixed"] = dict(kernel_time(cache, mixed, key, a.iters), patterns=[it["pattern"] for it in mixed])
    host = []
    for _ in range(20):
        t0 = time.perf_counter()
        R.plan(cache.offsets(np.arange(NF)), items_of(gen), H, W, PS, key, np.arange(NF * CPI))
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_plan_ms"] = round(float(np.median(host)), 3)
    with tempfile.TemporaryDirectory() as tmp:
        res["img2raw_uint8"] = IB.kernel_time(tmp, np.uint8, a.iters)
    res["host_numpy_ms"] = host_numpy(frames, mixed)
    res["clock_mhz_after"] = round(IB.clock_mhz())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
