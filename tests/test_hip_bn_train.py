"""GPU: the training-mode BatchNorm + ReLU kernels (csrc/bn_train.hip: yond_bn_stats_f32, yond_bn_apply_relu_f32, yond_bn_bwd_reduce_f32,
yond_bn_bwd_apply_f32) against the float64 model of tests/bn_model.py, element by element within the bounds derived there from the
kernels' arithmetic (checked on the CPU by tests/test_bn_model.py).  The backward's model takes its ReLU mask from the kernel's own
forward output.  Shapes are the smallest at which the kernels can go wrong: two values per channel, every supported channel count, a
ragged pixel count at C = 96 (240 of a workgroup's 256 threads), more than one workgroup's partial sums.

The [parity] lines (worst |kernel - model| / bound per output and case; at most 1) are what profiles/bn_train_report.txt records: with
YOND_BN_REPORT=<file> in the environment the lines are appended to that file as well."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bn_model as B

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS, MOM = 1e-4, 0.95


def note(line):
    print(line)
    path = os.environ.get("YOND_BN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def lib():
    from yond_public_amd import _lib as L
    return L, L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_forward(y, gamma, beta, rm, rv, ws_extra=0):
    """The stats and apply entries on [M][C] arrays.  Returns (stat [4][C], pending [2][C], out [M][C], the workspace tensor)."""
    L, lb = lib()
    M, Cn = y.shape
    need = int(lb.yond_bn_train_ws_bytes(M, Cn))
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8 + ws_extra,), -7.0, dtype=torch.float64, device=DEV)
    yd, gd, bd, rmd, rvd = (dev(t) for t in (y, gamma, beta, rm, rv))
    stat = torch.full((4, Cn), float('nan'), dtype=torch.float32, device=DEV)
    pend = torch.full((2, Cn), float('nan'), dtype=torch.float32, device=DEV)
    out = torch.full((M, Cn), float('nan'), dtype=torch.float32, device=DEV)
    L.check(lb.yond_bn_stats_f32(L.ptr(yd), M, Cn, L.ptr(gd), L.ptr(bd), L.ptr(rmd), L.ptr(rvd), EPS, MOM, L.ptr(stat), L.ptr(pend), L.ptr(ws),
                                 need, L.stream()), "yond_bn_stats_f32")
    L.check(lb.yond_bn_apply_relu_f32(L.ptr(yd), L.ptr(stat), M, Cn, L.ptr(out), L.stream()), "yond_bn_apply_relu_f32")
    torch.cuda.synchronize()
    assert torch.equal(rmd.cpu(), torch.from_numpy(rm)) and torch.equal(rvd.cpu(), torch.from_numpy(rv))     # the running statistics are only read
    return stat, pend, out, ws


def run_backward(y, dout, stat, ws_extra=0):
    L, lb = lib()
    M, Cn = y.shape
    need = int(lb.yond_bn_train_ws_bytes(M, Cn))
    ws = torch.full((need // 8 + ws_extra,), -7.0, dtype=torch.float64, device=DEV)
    yd, dd = dev(y), dev(dout)
    dg = torch.full((Cn,), float('nan'), dtype=torch.float32, device=DEV)
    db = torch.full((Cn,), float('nan'), dtype=torch.float32, device=DEV)
    dy = torch.full((M, Cn), float('nan'), dtype=torch.float32, device=DEV)
    L.check(lb.yond_bn_bwd_reduce_f32(L.ptr(yd), L.ptr(dd), L.ptr(stat), M, Cn, L.ptr(dg), L.ptr(db), L.ptr(ws), need, L.stream()),
            "yond_bn_bwd_reduce_f32")
    L.check(lb.yond_bn_bwd_apply_f32(L.ptr(yd), L.ptr(dd), L.ptr(stat), L.ptr(dg), L.ptr(db), M, Cn, L.ptr(dy), L.stream()), "yond_bn_bwd_apply_f32")
    torch.cuda.synchronize()
    return dg, db, dy, ws


def check_case(tag, case):
    """All four kernels of one case against the model within the bounds.  Returns what the special cases look at."""
    y, dout, gamma, beta, rm, rv = case
    stat, pend, out, _ = run_forward(y, gamma, beta, rm, rv)
    stat_h, pend_h, out_h = stat.cpu().numpy(), pend.cpu().numpy(), out.cpu().numpy()
    fwd = B.exact(y, gamma, beta, rm, rv)
    bd = B.bounds(y, gamma, beta, rm, rv, fwd)
    ratios = {n: B.worst_ratio(stat_h[i], fwd[n], bd[n]) for i, n in enumerate(('mean', 'rstd', 'scale', 'shift'))}
    ratios['out'] = B.worst_ratio(out_h, fwd['out'], bd['out'])
    ratios['rm_new'] = B.worst_ratio(pend_h[0], fwd['rm_new'], bd['rm_new'])
    ratios['rv_new'] = B.worst_ratio(pend_h[1], fwd['rv_new'], bd['rv_new'])
    with np.errstate(invalid='ignore'):
        mask = out_h > 0                                      # the kernel's own forward decides the backward's mask
    dg, db, dy, _ = run_backward(y, dout, stat)
    dg_h, db_h, dy_h = dg.cpu().numpy(), db.cpu().numpy(), dy.cpu().numpy()
    bwd = B.exact_backward(y, dout, mask, fwd)
    bb = B.bounds_backward(y, fwd, bwd)
    ratios['dbeta'] = B.worst_ratio(db_h, bwd['dbeta'], bb['dbeta'])
    ratios['dgamma'] = B.worst_ratio(dg_h, bwd['dgamma'], bb['dgamma'])
    ratios['dy'] = B.worst_ratio(dy_h, bwd['dy'], bb['dy'])
    note(f"[parity] bn_train {tag} M={y.shape[0]} C={y.shape[1]}: worst |kernel - model| / bound  "
         + "  ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    return dict(stat=stat_h, pend=pend_h, out=out_h, dg=dg_h, db=db_h, dy=dy_h, fwd=fwd, bwd=bwd)


@pytest.mark.parametrize("Cn", [32, 64, 96, 128])
def test_two_values_per_channel_every_channel_count(Cn):
    """M = 2: the unbiased variance's M / (M - 1) = 2."""
    r = check_case("m2", B.make_case('m2', Cn))
    y = B.make_case('m2', Cn)[0].astype(np.float64)
    assert np.allclose(r['fwd']['var'] * 2, y.var(0, ddof=1), rtol=1e-12, atol=0)


def test_one_value_per_channel_and_bad_arguments_are_refused():
    L, lb = lib()
    t = torch.zeros(4 * 128 + 64, dtype=torch.float32, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p, w = L.ptr(t), L.ptr(ws)
    ok = lambda M, Cn: (lb.yond_bn_stats_f32(p, M, Cn, p, p, p, p, EPS, MOM, p, p, w, ws.numel() * 8, L.stream()),
                        lb.yond_bn_apply_relu_f32(p, p, M, Cn, p, L.stream()),
                        lb.yond_bn_bwd_reduce_f32(p, p, p, M, Cn, p, p, w, ws.numel() * 8, L.stream()),
                        lb.yond_bn_bwd_apply_f32(p, p, p, p, p, M, Cn, p, L.stream()))
    assert ok(1, 32) == (-1, -1, -1, -1)                      # (1, 1, 1, C): M = 1
    assert ok(0, 32) == (-1, -1, -1, -1)
    for Cn in (0, 16, 48, 160, 256):
        assert ok(2, Cn) == (-1, -1, -1, -1), Cn
        assert lb.yond_bn_train_ws_bytes(2, Cn) == 0
    assert lb.yond_bn_train_ws_bytes(1, 32) == 0
    assert lb.yond_bn_stats_f32(None, 2, 32, p, p, p, p, EPS, MOM, p, p, w, ws.numel() * 8, L.stream()) == -1
    assert lb.yond_bn_stats_f32(p, 2, 32, p, p, p, p, EPS, MOM, p, p, None, ws.numel() * 8, L.stream()) == -1
    assert lb.yond_bn_stats_f32(p, 2, 32, p, p, p, p, EPS, MOM, p, p, w, lb.yond_bn_train_ws_bytes(2, 32) - 8, L.stream()) == -1
    assert lb.yond_bn_stats_f32(p, 2, 32, p, p, p, p, -1.0, MOM, p, p, w, ws.numel() * 8, L.stream()) == -1
    assert lb.yond_bn_stats_f32(p, 2, 32, p, p, p, p, EPS, 1.5, p, p, w, ws.numel() * 8, L.stream()) == -1
    off = C.c_void_p(t.data_ptr() + 4)                        # a tensor pointer off the 16-byte grid
    assert lb.yond_bn_apply_relu_f32(off, p, 2, 32, p, L.stream()) == -1
    assert lb.yond_bn_bwd_apply_f32(p, p, p, p, p, 2, 32, off, L.stream()) == -1
    assert lb.yond_bn_apply_relu_f32(p, None, 2, 32, p, L.stream()) == -1
    assert lb.yond_bn_bwd_reduce_f32(p, p, p, 2, 32, None, p, w, ws.numel() * 8, L.stream()) == -1
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0                        # nothing was launched


def test_ragged_pixel_count_at_96_channels():
    check_case("ragged", B.make_case('ragged', 96))


@pytest.fixture(scope="module")
def multi():
    return B.make_case('multi', 32)


def test_more_than_one_workgroup(multi):
    """(2, 64, 64, 32): 8192 pixels = 32 workgroups' partial sums for the finish launch."""
    _, lb = lib()
    assert lb.yond_bn_train_ws_bytes(8192, 32) == 32 * 2 * 32 * 8
    check_case("multi", multi)


def test_constant_channel():
    r = check_case("constant", B.make_case('constant', 32))
    assert r['stat'][0][3] == np.float32(0.7) and r['stat'][1][3] == np.float32(100.0)        # var = 0, rstd = 1 / sqrt(eps)


def test_cancellation_in_the_variance():
    """Mean 1e3, deviation 1e-2: Syy / M - mean^2 loses ten digits; float64 sums keep the rest."""
    r = check_case("cancel", B.make_case('cancel', 64))
    var = r['fwd']['var'][5]
    assert 2e-5 < var < 5e-4                                  # (the case is what it says; the bounds above are the check)


def test_dead_channels_get_exactly_zero_gradients():
    r = check_case("dead", B.make_case('dead', 32))
    assert (r['out'][:, 1:3] == 0).all()
    assert (r['dg'][1:3] == 0).all() and (r['db'][1:3] == 0).all() and (r['dy'][:, 1:3] == 0).all()


def test_an_output_of_exactly_zero_passes_no_gradient():
    case = B.make_case('boundary', 32)
    r = check_case("boundary", case)
    assert (r['out'][2:, 0] == 0).all() and r['out'][0, 0] > 0
    # the model ran with the kernel's mask (out > 0: false at the zeros); had the kernel let dout through there, dbeta would differ
    dout = case[1].astype(np.float64)
    assert abs(float(r['db'][0]) - dout[0, 0]) <= 1e-6 * abs(dout[0, 0])


def test_a_nan_stays_in_its_channel():
    Cn = 32
    r = check_case("nan", B.make_case('nan', Cn))
    good = np.ones(Cn, bool)
    good[7] = False
    assert np.isnan(r['out'][:, 7]).all() and np.isnan(r['dy'][:, 7]).all() and np.isnan(r['dg'][7])
    assert np.isnan(r['stat'][:, 7]).all() and np.isnan(r['pend'][:, 7]).all()
    for k in ('out', 'dy'):
        assert np.isfinite(r[k][:, good]).all()
    for k in ('stat', 'pend'):
        assert np.isfinite(r[k][:, good]).all()
    assert np.isfinite(r['dg'][good]).all() and np.isfinite(r['db'][good]).all()


def test_two_runs_are_bitwise_equal(multi):
    y, dout, gamma, beta, rm, rv = multi
    runs = []
    for _ in range(2):
        stat, pend, out, _ = run_forward(y, gamma, beta, rm, rv)
        dg, db, dy, _ = run_backward(y, dout, stat)
        runs.append([t.cpu() for t in (stat, pend, out, dg, db, dy)])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("M,Cn", [(2, 32), (105, 96), (8192, 32), (257, 128), (70000, 64), (70000, 128)])
def test_workspace_query_covers_what_the_launches_touch(M, Cn):
    """Poisoned doubles behind the queried size stay as they were; every double inside it is overwritten."""
    rng = np.random.default_rng(M + Cn)
    y = rng.standard_normal((M, Cn)).astype(np.float32)
    dout = rng.standard_normal((M, Cn)).astype(np.float32)
    one, zero = np.ones(Cn, np.float32), np.zeros(Cn, np.float32)
    stat, _, _, ws = run_forward(y, one, zero, zero, one, ws_extra=1024)
    _, _, _, ws2 = run_backward(y, dout, stat, ws_extra=1024)
    _, lb = lib()
    n = int(lb.yond_bn_train_ws_bytes(M, Cn)) // 8
    for w in (ws, ws2):
        assert bool((w[n:] == -7.0).all()) and w[n:].numel() == 1024
    assert not bool((ws[:n] == -7.0).any())                  # (sums of y and y y: none of them is the poison value)
