"""R1 measurement: the raw -> sRGB render (yond_render_srgb, csrc/isp.hip) in codes form next to a device-to-device copy of the
same traffic in the same process, and what --fig costs the SIDD evaluation driver per image.
    python tools/isp_bench.py [--iters 200] [--driver 8] [--out profiles/isp_bench.json]
Prints one JSON line:
  - per frame size (3000 x 4000, 256 x 8192): render_us = median of event-timed launches after warm-up; bytes = 4 B in + 3 B out per
    pixel; copy_us = a copy of bytes / 2 (reads and writes that many: the same traffic) timed the same way, interleaved with the
    render launches; ratio = copy_us / render_us (1 = the copy's rate; the yardstick is this copy, tools/probe/hbm_ceiling.py reports
    the box's rate);
  - driver (with --driver N): wall and path ms per image of `YOND_SIDD.py --synthetic N --group 1 --no-stream` with --fig and without
    (both on the one-group-at-a-time path, so the difference is the figures: renders, metrics, PNG encoding on host threads);
  - clock_mhz: the shader clock the chip held (yond_clock_probe)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib
from yond_public_amd import isp

DEV = "cuda:0"


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def frame_time(H, W, iters):
    g = torch.Generator(device=DEV).manual_seed(H + W)
    frame = torch.rand((H, W), device=DEV, generator=g) * 1.2 - 0.1
    nbytes = H * W * 7
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    wb = [[0.52, 1.0, 0.62]]
    cst = np.array([[0.9142, -0.3268, -0.0871], [-0.4537, 1.3009, 0.1652], [-0.0913, 0.2446, 0.6104]])
    render = lambda: isp.render_sidd(frame, [[3, 2], [2, 1]], wb, cst, order='rgb')
    for _ in range(10):
        render()
        dst.copy_(src)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in ev:
        a.record()
        render()
        b.record()
        dst.copy_(src)
        c.record()
    torch.cuda.synchronize()
    r_us = float(np.median([a.elapsed_time(b) * 1e3 for a, b, _ in ev]))
    c_us = float(np.median([b.elapsed_time(c) * 1e3 for _, b, c in ev]))
    return {"render_us": round(r_us, 2), "copy_us": round(c_us, 2), "bytes": nbytes, "render_GBs": round(nbytes / r_us * 1e-3, 1),
            "copy_GBs": round(nbytes / c_us * 1e-3, 1), "ratio": round(c_us / r_us, 3)}


def driver_time(n):
    from yond_public_amd import YOND_SIDD as Y
    runfile = os.path.join(ROOT, "runfiles", "YOND", "SIDD_simple+full_pre_grumix.yml")
    out = {}
    cwd = os.getcwd()
    for key, extra in (("plain", []), ("fig", ["--fig"]), ("plain_again", [])):
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                Y.main(['-f', runfile, '-m', 'eval', '--synthetic', str(n), '--group', '1', '--no-stream'] + extra)
                out[key] = {k: round(v, 2) for k, v in Y.main.trainer.last_timing.items()}
            finally:
                os.chdir(cwd)
    out["fig_ms_per_image"] = round(out["fig"]["wall_ms_per_image"] - 0.5 * (out["plain"]["wall_ms_per_image"] + out["plain_again"]["wall_ms_per_image"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--driver", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "isp_bench needs an MI355X"
    G.build()
    res = {"clock_mhz_before": round(clock_mhz())}
    res["3000x4000"] = frame_time(3000, 4000, a.iters)
    res["256x8192"] = frame_time(256, 8192, a.iters)
    res["clock_mhz_after"] = round(clock_mhz())
    if a.driver:
        res["driver"] = driver_time(a.driver)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
