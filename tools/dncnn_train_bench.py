"""Measure DnCNN training on the HIP kernels: the four BatchNorm launches of csrc/bn_train.hip, torch's own BatchNorm + ReLU on the same
tensor, and the whole training step at the reference's training shape.

    python tools/dncnn_train_bench.py [--out profiles/dncnn_train_bench.json] [--iters 20] [--steps 10] [--batch 64]

  * kernels: each entry on a [batch][128][128][64] float32 tensor (batch 64: 268 MB, more than the 256 MB Infinity Cache, and the
    launches walk a ring of three such tensor sets, so none is resident), HIP events around single calls, the median of --iters;
    beside a device copy of the same tensor in the same loop.  Algorithmic bytes in units of the tensor: statistics 1, apply 2,
    backward reduction 2, backward apply 3, copy 2; `x_copy_per_2_units` = (time / units) / (copy time / 2).
  * torch: F.relu(F.batch_norm(x, training=True)) forward and autograd backward on the same memory (channels-last), the baseline the
    kernels are measured against -- not the code under test.
  * step: TrainStep on DnCNN nf 64, depth 17, use_bn, [batch][4][128][128], host clock around steps (each ends in a synchronise),
    captured (graph=True, from the third step on) and eager; `bn_share` = 15 layers x the four entries' medians over the step time
    (computed from the two measurements above, not traced).
  * clock_mhz: the shader clock before and after (yond_clock_probe)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yond_public_amd import _lib as L  # noqa: E402

UNITS = {'stats': 1, 'apply': 2, 'bwd_reduce': 2, 'bwd_apply': 3, 'copy': 2}


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
    M, C, R = batch * 128 * 128, 64, 3
    g = torch.Generator(device='cuda').manual_seed(1)
    ring = [tuple(torch.randn((M, C), device='cuda', generator=g) for _ in range(2)) + tuple(torch.empty((M, C), device='cuda') for _ in range(2))
            for _ in range(R)]
    gamma, beta = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda') * 0.1
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    stat, pend, dgb = torch.zeros((4, C), device='cuda'), torch.zeros((2, C), device='cuda'), torch.zeros((2, C), device='cuda')
    need = int(lib.yond_bn_train_ws_bytes(M, C))
    ws = torch.empty(need // 8, dtype=torch.float64, device='cuda')
    st = L.stream

    def call(name, k):
        y, dout, out, dy = ring[k % R]
        if name == 'stats':
            L.check(lib.yond_bn_stats_f32(L.ptr(y), M, C, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), 1e-4, 0.95, L.ptr(stat), L.ptr(pend),
                                          L.ptr(ws), need, st()), name)
        elif name == 'apply':
            L.check(lib.yond_bn_apply_relu_f32(L.ptr(y), L.ptr(stat), M, C, L.ptr(out), st()), name)
        elif name == 'bwd_reduce':
            L.check(lib.yond_bn_bwd_reduce_f32(L.ptr(y), L.ptr(dout), L.ptr(stat), M, C, L.ptr(dgb[0]), L.ptr(dgb[1]), L.ptr(ws), need, st()), name)
        elif name == 'bwd_apply':
            L.check(lib.yond_bn_bwd_apply_f32(L.ptr(y), L.ptr(dout), L.ptr(stat), L.ptr(dgb[0]), L.ptr(dgb[1]), M, C, L.ptr(dy), st()), name)
        else:
            out.copy_(y)
    times = {n: [] for n in UNITS}
    for k in range(iters + 2):
        for n in UNITS:                                      # interleaved: the same clock and neighbours for every entry
            t = timed(lambda: call(n, k))
            if k >= 2:
                times[n].append(t)
    tensor_bytes = M * C * 4
    res = {'tensor': [batch, 128, 128, C], 'tensor_mb': tensor_bytes / 1e6, 'iters': iters}
    copy_med = float(np.median(times['copy']))
    for n, ts in times.items():
        med = float(np.median(ts))
        res[n] = {'ms_median': med, 'ms_min': float(np.min(ts)), 'ms_max': float(np.max(ts)), 'units': UNITS[n],
                  'tb_per_s': UNITS[n] * tensor_bytes / (med / 1e3) / 1e12, 'x_copy_per_2_units': (med / UNITS[n]) / (copy_med / 2)}
    # torch on the same memory: logical NCHW, channels-last strides = [N][H][W][C]
    tf, tfb = [], []
    for k in range(iters + 2):
        y, dout, _, _ = ring[k % R]
        x = y.view(batch, 128, 128, C).permute(0, 3, 1, 2).detach().requires_grad_(True)
        d = dout.view(batch, 128, 128, C).permute(0, 3, 1, 2)
        w, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        box = {}
        t1 = timed(lambda: box.__setitem__('o', F.relu(F.batch_norm(x, rm.clone(), rv.clone(), w, b, True, 0.95, 1e-4))))
        t2 = timed(lambda: box['o'].backward(d))
        if k >= 2:
            tf.append(t1)
            tfb.append(t2)
        del box, x
    res['torch'] = {'forward_ms_median': float(np.median(tf)), 'backward_ms_median': float(np.median(tfb)),
                    'hip_forward_ms_median': res['stats']['ms_median'] + res['apply']['ms_median'],
                    'hip_backward_ms_median': res['bwd_reduce']['ms_median'] + res['bwd_apply']['ms_median']}
    del ring
    torch.cuda.empty_cache()
    return res


def bench_step(batch, steps, graph):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dncnn_common as D
    from yond_public_amd import archs as A
    from yond_public_amd.train import TrainStep
    torch.manual_seed(0)
    net = A.DnCNN(D.dn_args())
    A.initialize_weights(net)
    net = net.to('cuda').train()
    ts = TrainStep(net, lr=1e-4, ddp=False, graph=graph)
    g = torch.Generator().manual_seed(1)
    hr = torch.rand(batch, 4, 128, 128, generator=g).cuda()
    lr = (hr + torch.randn(hr.shape, generator=g).cuda() * 0.1).clamp(0, 1)
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
    del ts, net
    torch.cuda.empty_cache()
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'steps': steps, 'last_loss': loss,
            'patches_per_s': batch / (float(np.median(ms)) / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dncnn_train_bench.json'))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dncnn_train_bench.py needs an MI355X: there is nothing to measure without one")
    res = {'device': torch.cuda.get_device_name(0), 'clock_mhz_before': round(clock_mhz())}
    res['kernels'] = k = bench_kernels(a.batch, a.iters)
    for n in UNITS:
        print(f"{n:11s} {k[n]['ms_median']:.3f} ms  {k[n]['tb_per_s']:.2f} TB/s  x{k[n]['x_copy_per_2_units']:.2f} of a copy per 2 units", flush=True)
    print(f"torch batch_norm + relu: forward {k['torch']['forward_ms_median']:.3f} ms (HIP {k['torch']['hip_forward_ms_median']:.3f}), backward "
          f"{k['torch']['backward_ms_median']:.3f} ms (HIP {k['torch']['hip_backward_ms_median']:.3f})", flush=True)
    bn_ms = 15 * sum(k[n]['ms_median'] for n in ('stats', 'apply', 'bwd_reduce', 'bwd_apply'))
    res['step'] = {'shape': [a.batch, 4, 128, 128], 'arch': 'DnCNN nf 64 depth 17 use_bn', 'bn_ms_15_layers': bn_ms}
    for graph in (True, False):
        r = bench_step(a.batch, a.steps, graph)
        r['bn_share'] = bn_ms / r['ms_median']
        res['step']['captured' if graph else 'eager'] = r
        print(f"step ({'captured' if graph else 'eager'}): {r['ms_median']:.2f} ms, {r['patches_per_s']:.0f} patches/s, BatchNorm share {100 * r['bn_share']:.1f} %",
              flush=True)
    res['clock_mhz_after'] = round(clock_mhz())
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
