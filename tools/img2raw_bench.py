"""I1 measurement: the sRGB -> raw synthesis (yond_img2raw_f32, csrc/img2raw.hip) at the reference's training shape (64 crops of
256 x 256) and an epoch of trainer_AWGN on sRGB crops next to the same epoch on --synthetic patches.
    python tools/img2raw_bench.py [--iters 100] [--out profiles/img2raw_bench.json]
Prints one JSON line:
  - kernel_us: median of event-timed launches (after warm-up) for uint8 and uint16 crops, with the algorithmic bytes (crops in,
    hr + lr + sigma out, the patch array, the uint16 curve) over that time as GB/s and as a share of 6.3 TB/s;
  - host_plan_ms: the host's per-batch work (64 metadata / pattern / sigma draws + the patch array), median;
  - epoch_s: one epoch (after a warm-up epoch) of the GRU runfile at batch 64 on N sRGB crops and on --synthetic N;
  - clock_mhz: the shader clock the chip held (yond_clock_probe)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib
from yond_public_amd import img2raw as I

DEV = "cuda:0"
HBM_TBS = 6.3


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def crops(n, H, W, dtype, seed=0):
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    return [rng.integers(0, top + 1, (H, W, 3), dtype=dtype) for _ in range(n)]


def kernel_time(tmp, dtype, iters, B=64, S=256):
    d = os.path.join(tmp, f"k_{np.dtype(dtype).name}")
    os.makedirs(d)
    for i, c in enumerate(crops(B, S, S, dtype)):
        np.save(os.path.join(d, f"{i:03d}.npy"), c)
    cache = I.CropCache(sorted(os.path.join(d, f) for f in os.listdir(d)), DEV)
    table = I.curve(dtype, 255. if dtype == np.uint8 else 65535., DEV)
    gen, key = I.train_streams(1, 0)
    metas, pats, sigs = zip(*[I.sample_item(gen, 5, 50) for _ in range(B)])
    p = I.plan(cache.offsets(np.arange(B)), metas, pats, sigs, key, np.arange(B))
    pd = torch.from_numpy(p.view(np.uint8)).to(DEV)
    hr = torch.empty((B, 4, S // 2, S // 2), device=DEV)
    lr, sig = torch.empty_like(hr), torch.empty(B, device=DEV)
    lib = _lib.load()
    args = (C.c_void_p(cache.buf.data_ptr()), cache.buf.numel(), 0 if dtype == np.uint8 else 1, S, S, _lib.ptr(table),
            C.c_void_p(pd.data_ptr()), B, -1, 1, _lib.ptr(hr), _lib.ptr(lr), _lib.ptr(sig), _lib.stream())
    for _ in range(20):
        _lib.check(lib.yond_img2raw_f32(*args), "yond_img2raw_f32")
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        lib.yond_img2raw_f32(*args)
        b.record()
    torch.cuda.synchronize()
    us = float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))
    esz = np.dtype(dtype).itemsize
    nbytes = B * S * S * 3 * esz + 2 * hr.numel() * 4 + B * 4 + p.nbytes + (table.numel() * 4 if esz == 2 else 0)
    t0 = time.perf_counter()
    host = []
    for _ in range(20):
        t0 = time.perf_counter()
        m2, p2, s2 = zip(*[I.sample_item(gen, 5, 50) for _ in range(B)])
        I.plan(cache.offsets(np.arange(B)), m2, p2, s2, key, np.arange(B))
        host.append((time.perf_counter() - t0) * 1e3)
    return {"us": round(us, 2), "bytes": int(nbytes), "GBs": round(nbytes / us * 1e-3, 1), "hbm_share": round(nbytes / us * 1e-6 / HBM_TBS, 3),
            "host_plan_ms": round(float(np.median(host)), 3)}


def epoch_time(tmp, n, synthetic):
    """Seconds of epoch 2 (epoch 1 fills the crop cache and captures the step) of the GRU runfile, batch 64, 256 x 256 crops."""
    import yaml
    from yond_public_amd import trainer_AWGN as TA
    sub = os.path.join(tmp, "syn" if synthetic else "srgb")
    os.makedirs(sub)
    if not synthetic:
        for d in ("train_mix", "eval"):
            os.makedirs(os.path.join(sub, "data", d))
            for i, c in enumerate(crops(n if d == "train_mix" else 1, 256, 256, np.uint8, seed=1)):
                np.save(os.path.join(sub, "data", d, f"{i:04d}.npy"), c)
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "GRU_5to50_norm_mix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ("dst", "dst_train", "dst_eval", "dst_test"):
        cfg[sec].update(root_dir=os.path.join(sub, "data"))
    cfg["hyper"].update(last_epoch=0, stop_epoch=10, save_freq=1000, plot_freq=1000)
    rf = os.path.join(sub, "run.yml")
    with open(rf, "w") as f:
        yaml.dump(cfg, f)
    cwd = os.getcwd()
    os.chdir(sub)
    try:
        tr = TA.AWGN_Trainer(['-f', rf, '-m', 'train'] + (['--synthetic', str(n)] if synthetic else []))
        times = []
        for epoch in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nb = 0
            for data in tr._epoch_batches(epoch):
                lr, hr, sigma = tr.preprocess(data)
                tr.ts.step(lr, hr, sigma)
                nb += 1
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return {"s": round(times[1], 4), "first_epoch_s": round(times[0], 4), "batches": nb, "ms_per_batch": round(times[1] / nb * 1e3, 2)}
    finally:
        os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--crops", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "img2raw_bench needs an MI355X"
    G.build()
    res = {"clock_mhz_before": round(clock_mhz())}
    with tempfile.TemporaryDirectory() as tmp:
        res["uint8"] = kernel_time(tmp, np.uint8, a.iters)
        res["uint16"] = kernel_time(tmp, np.uint16, a.iters)
        res["epoch_srgb"] = epoch_time(tmp, a.crops, False)
        res["epoch_synthetic"] = epoch_time(tmp, a.crops, True)
    res["clock_mhz_after"] = round(clock_mhz())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
