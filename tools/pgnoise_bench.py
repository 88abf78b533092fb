"""I2 measurement: Poisson-Gaussian noise synthesis (yond_pg_noise_f32, csrc/pgnoise.hip) next to the same expression in NumPy.
    python tools/pgnoise_bench.py [--iters 50] [--out profiles/pgnoise_bench.json]
Two shapes: a training batch, 64 x 4 x 128 x 128 with (K, sigma) per item from the camera-noise prior (pgnoise.sample_pg_params) on
synthetic clean patches, and one 3472 x 4624 frame at K = 2, sigma = 8 (the full-frame drivers' stand-in).  Prints one JSON line:
  - us: median of event-timed launches after warm-up (at least 20), GBs: the 8 bytes per element the kernel must move (4 in, 4 out)
    over that time, hbm_share of 6.3 TB/s;
  - numpy_ms: noisy = rng.poisson(x / beta1) * beta1 + rng.normal(0, sigma_n, shape) on ONE host thread of the same box (median of
    --host-iters runs), and speedup = numpy_ms / us;
  - lambda_max: the largest Poisson mean of the shape (which of the sampler's regimes the launch exercises);
  - clock_mhz: the shader clock the chip held before and after (yond_clock_probe)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib
from yond_public_amd import pgnoise as PG
from yond_public_amd import synthetic as S

DEV = "cuda:0"
HBM_TBS = 6.3


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def measure(clean, K, sigma, scale, iters, host_iters):
    """clean: host float32 [B][...]; K, sigma: per item."""
    B = clean.shape[0]
    items = PG.plan(B, K, sigma, scale, 1997, np.arange(B))
    x = torch.from_numpy(clean).to(DEV)
    y = torch.empty_like(x)
    d_items = torch.from_numpy(items.view(np.uint8)).to(DEV)
    lib = _lib.load()
    args = (_lib.ptr(x), _lib.ptr(y), x.numel() // B, B, C.c_void_p(d_items.data_ptr()), 0, _lib.stream())
    for _ in range(20):
        _lib.check(lib.yond_pg_noise_f32(*args), "yond_pg_noise_f32")
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(20, iters))]
    for a, b in ev:
        a.record()
        lib.yond_pg_noise_f32(*args)
        b.record()
    torch.cuda.synchronize()
    us = float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))
    nbytes = 8 * x.numel()
    shape = (B,) + (1,) * (clean.ndim - 1)
    b1 = items['beta1'].astype(np.float64).reshape(shape)
    sn = items['sigma_n'].astype(np.float64).reshape(shape)
    rng = np.random.default_rng(0)
    host = []
    for _ in range(host_iters):
        t0 = time.perf_counter()
        noisy = rng.poisson(clean / b1) * b1 + rng.normal(0.0, 1.0, clean.shape) * sn
        host.append((time.perf_counter() - t0) * 1e3)
    # the launch and the host draw describe the same thing: equal mean and variance of the residual to the draws' own spread
    r_dev, r_host = (y.double().cpu().numpy() - clean), (noisy - clean)
    ms = float(np.median(host))
    return {"shape": list(clean.shape), "us": round(us, 2), "bytes": int(nbytes), "GBs": round(nbytes / us * 1e-3, 1),
            "hbm_share": round(nbytes / us * 1e-6 / HBM_TBS, 3), "numpy_ms": round(ms, 2), "speedup": round(ms * 1e3 / us, 1),
            "lambda_max": float((clean / b1).max()), "residual_var_device": float(r_dev.var()), "residual_var_numpy": float(r_host.var())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgnoise_bench.json"))
    a = ap.parse_args()
    G.build()
    torch.set_num_threads(1)
    res = {"clock_mhz_before": round(clock_mhz())}
    rs = np.random.RandomState(0)
    prm = [PG.sample_pg_params(rs) for _ in range(64)]
    big = S.synth_clean(1024, 2048).astype(np.float32)
    batch = np.stack([np.stack([big[(37 * i) % 768:, (101 * i) % 1792:][c // 2:256 + c // 2:2, c % 2:256 + c % 2:2] for c in range(4)])
                      for i in range(64)])
    assert batch.shape == (64, 4, 128, 128)
    res["train_batch"] = measure(batch, [q['K'] for q in prm], [q['sigma'] for q in prm], 959.0, a.iters, a.host_iters)
    frame = (S.synth_clean(3472, 4624) * 0.6).astype(np.float32)[None]
    res["frame_16mp"] = measure(frame, 2.0, 8.0, 959.0, a.iters, a.host_iters)
    res["clock_mhz_after"] = round(clock_mhz())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
