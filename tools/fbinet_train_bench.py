"""Measure FBI_Net training on the HIP kernels: every entry of csrc/fbinet_train.hip at the training shape of
runfiles/Gaussian/FBI_5to50_norm.yml, the forward tap kernel on the same tensor, and the whole training step.

    python tools/fbinet_train_bench.py [--out profiles/fbinet_train_bench.json] [--iters 10] [--steps 5] [--batch 16]

  * kernels: each entry on [batch][256][256][64] float32 tensors (batch 16: 268 MB each, more than the 256 MB Infinity Cache; the
    launches walk a ring of three tensor sets, so none is resident), HIP events around single calls, the median of --iters, beside a
    device copy of the same tensor in the same loop (`x_copy` = time / copy time).  `tapconv_fwd<set>` is yond_fbi_tapconv_f32, the
    inference kernel the training forward and the data gradient also run on; `per_live_tap` puts the weight gradient's time per
    live tap beside the forward's.
  * step: TrainStep on FBI_Net nf 64, 17 layers, [batch][4][128][128] packed batches (mosaics of 256 x 256), host clock around steps
    (each ends in a synchronise), captured (graph=True, from the third step on) and eager; peak device memory of the eager run.
  * clock_mhz: the shader clock before and after (yond_clock_probe).
These are measurements to write down, not pass marks."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yond_public_amd import _lib as L  # noqa: E402

NF, HW = 64, 256
TAPS = {0: 9, 1: 5, 2: 1}


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device='cuda')
    L.check(L.load().yond_clock_probe(2000.0, L.ptr(out), L.stream()), "yond_clock_probe")
    torch.cuda.synchronize()
    c, r = (int(v) for v in out.cpu())
    return c / max(r, 1) * 100.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench_kernels(batch, iters):
    lib = L.load()
    N, H, W, R = batch, HW, HW, 3
    npix = N * H * W
    g = torch.Generator(device='cuda').manual_seed(1)
    ring = [tuple(torch.randn((N, H, W, NF), device='cuda', generator=g) for _ in range(2)) + tuple(torch.empty((N, H, W, NF), device='cuda') for _ in range(2))
            for _ in range(R)]
    x4, dp4 = torch.rand((N, H // 2, W // 2, 4), device='cuda', generator=g), torch.randn((N, H // 2, W // 2, 4), device='cuda', generator=g)
    slope, one, bias = torch.rand(NF, device='cuda') - 0.3, torch.ones(NF, device='cuda'), torch.zeros(NF, device='cuda')
    wout = torch.randn((2, NF), device='cuda') * 0.1
    wpk = {}
    for tset, k in ((0, 5), (1, 3)):
        w = (torch.randn((NF, NF, k, k)) * 0.05).numpy()
        out = np.empty(TAPS[tset] * NF * NF, np.float32)
        L.check(lib.yond_pack_fbi_tap_weight_f32(C.c_void_p(w.ctypes.data), NF, tset, C.c_void_p(out.ctypes.data)), "pack")
        wpk[tset] = torch.from_numpy(out).cuda()
    need = int(lib.yond_fbi_train_ws_bytes(NF, N, H, W))
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device='cuda')
    small = torch.empty(9 * NF * NF + NF, device='cuda')
    st = L.stream

    def call(name, k):
        a, b, o1, o2 = ring[k % R]
        if name.startswith('wgrad'):
            L.check(lib.yond_fbi_wgrad_f32(L.ptr(a), L.ptr(b), int(name[-1]), NF, N, H, W, L.ptr(small), L.ptr(ws), need, st()), name)
        elif name.startswith('tapconv_fwd'):
            t = int(name[-1])
            L.check(lib.yond_fbi_tapconv_f32(L.ptr(a), L.ptr(b), t, NF, L.ptr(wpk[t]), L.ptr(bias), L.ptr(slope), L.ptr(slope), N, H, W, L.ptr(o1), L.ptr(o2),
                                             st()), name)
        elif name == 'prelu':
            L.check(lib.yond_fbi_prelu_f32(L.ptr(a), L.ptr(b), 2.0, L.ptr(slope), NF, NF, npix, L.ptr(o1), L.ptr(o2), st()), name)
        elif name == 'prelu_bwd':
            L.check(lib.yond_fbi_prelu_bwd_f32(L.ptr(a), L.ptr(b), 2.0, L.ptr(slope), NF, NF, npix, L.ptr(o1), L.ptr(small), L.ptr(ws), need, st()), name)
        elif name == 'first_bwd':
            L.check(lib.yond_fbi_first_bwd_f32(L.ptr(x4), L.ptr(a), N, H // 2, W // 2, NF, L.ptr(small), L.ptr(ws), need, st()), name)
        elif name == 'out_bwd':
            L.check(lib.yond_fbi_out_bwd_f32(L.ptr(a), NF, L.ptr(wout), L.ptr(bias), 2, 0, 0.1, L.ptr(x4), L.ptr(dp4), N, H // 2, W // 2, L.ptr(o1), L.ptr(small),
                                             L.ptr(ws), need, st()), name)
        else:
            o1.copy_(a)
    # tensors read + written, in units of one [N][H][W][nf] tensor (the algorithmic traffic; halos and partial sums not counted)
    units = {'wgrad0': 2, 'wgrad1': 2, 'wgrad2': 2, 'tapconv_fwd0': 4, 'tapconv_fwd1': 4, 'prelu': 4, 'prelu_bwd': 3, 'first_bwd': 1, 'out_bwd': 2, 'copy': 2}
    times = {n: [] for n in units}
    for k in range(iters + 2):
        for n in units:                                      # interleaved: the same clock and neighbours for every entry
            t = timed(lambda: call(n, k))
            if k >= 2:
                times[n].append(t)
    tensor_bytes = npix * NF * 4
    res = {'tensor': [N, H, W, NF], 'tensor_mb': tensor_bytes / 1e6, 'iters': iters, 'ws_mb': need / 1e6}
    copy_med = float(np.median(times['copy']))
    for n, ts in times.items():
        med = float(np.median(ts))
        res[n] = {'ms_median': med, 'ms_min': float(np.min(ts)), 'ms_max': float(np.max(ts)), 'units': units[n], 'x_copy': med / copy_med}
        if n.startswith('wgrad') or n.startswith('tapconv_fwd'):
            res[n]['tflops'] = 2.0 * TAPS[int(n[-1])] * NF * NF * npix / (med / 1e3) / 1e12
    res['per_live_tap'] = {f'set{t}': {'wgrad_ms': res[f'wgrad{t}']['ms_median'] / TAPS[t], 'forward_ms': res[f'tapconv_fwd{t}']['ms_median'] / TAPS[t]}
                           for t in (0, 1)}
    del ring
    torch.cuda.empty_cache()
    return res


def bench_step(batch, steps, graph):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fbinet_common as D
    from yond_public_amd import archs as A
    from yond_public_amd.train import TrainStep
    torch.manual_seed(0)
    net = A.FBI_Net(D.fbi_args())
    A.initialize_weights(net)
    net = net.to('cuda').train()
    ts = TrainStep(net, lr=1e-4, ddp=False, graph=graph)
    g = torch.Generator().manual_seed(1)
    hr = torch.rand(batch, 4, HW // 2, HW // 2, generator=g).cuda()
    lr = (hr + torch.randn(hr.shape, generator=g).cuda() * 0.1).clamp(0, 1)
    torch.cuda.reset_peak_memory_stats()
    for _ in range(4):
        loss, _ = ts.step(lr, hr)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        loss, _ = ts.step(lr, hr)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert bool(ts._graphs) == graph
    peak = torch.cuda.max_memory_allocated()
    del ts, net
    torch.cuda.empty_cache()
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'steps': steps, 'last_loss': loss,
            'patches_per_s': batch / (float(np.median(ms)) / 1e3), 'peak_device_memory_gb': peak / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fbinet_train_bench.json'))
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fbinet_train_bench.py needs an MI355X: there is nothing to measure without one")
    res = {'device': torch.cuda.get_device_name(0), 'clock_mhz_before': round(clock_mhz())}
    res['kernels'] = k = bench_kernels(a.batch, a.iters)
    for n, v in k.items():
        if isinstance(v, dict) and 'ms_median' in v:
            print(f"{n:13s} {v['ms_median']:8.3f} ms  x{v['x_copy']:.2f} of a copy" + (f"  {v['tflops']:.1f} TFLOP/s" if 'tflops' in v else ""), flush=True)
    print(f"per live tap: {k['per_live_tap']}", flush=True)
    res['step'] = {'shape': [a.batch, 4, HW // 2, HW // 2], 'arch': 'FBI_Net nf 64, 17 layers, res, linear'}
    for graph in (False, True):
        r = bench_step(a.batch, a.steps, graph)
        res['step']['captured' if graph else 'eager'] = r
        print(f"step ({'captured' if graph else 'eager'}): {r['ms_median']:.2f} ms, {r['patches_per_s']:.1f} patches/s, peak {r['peak_device_memory_gb']:.1f} GB",
              flush=True)
    res['clock_mhz_after'] = round(clock_mhz())
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
