"""CPU: the float64 models of tests/train_model.py (the training step's small kernels) against torch's float64 autograd, their bounds
against structure-faithful float32 simulations of the kernels (worst ratio printed, at most 1), and single defects against the bounds (each
must exceed its bound on a named case).  The GPU counterpart is tests/test_hip_train_edges.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_model as M

HYP = dict(lr=3e-4, b1=0.9, b2=0.999, eps=1e-8)


def show(name, r):
    print(f"[bound] {name}: worst |sim - model| / bound = {r:.3f}")
    return r


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------
# the models are the operations: torch float64 autograd of the reference's formulation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,C", [(1, 1, 32), (3, 9, 32), (1, 97, 256), (3, 2, 1024)])
def test_film_silu_models_equal_float64_autograd(N, P, C):
    z, tk, tb, dout = M.film_silu_operands(N, P, C)
    tz, tK, tB = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (z, tk, tb))
    out = F.silu(tz * tK[:, None, :] + tB[:, None, :])
    out.backward(torch.from_numpy(dout.astype(np.float64)))
    assert rel(M.film_silu_fwd_model(z, tk, tb)[0], out.detach().numpy()) < 1e-13
    bw = M.film_silu_bwd_model(z, tk, tb, dout)
    for name, t in (('dz', tz), ('dtk', tK), ('dtb', tB)):
        assert rel(bw[name][0], t.grad.numpy()) < 1e-12, name


def test_silu_pair_and_losses_equal_float64_autograd():
    x = M.silu_operands(1000)
    dz, dres = np.random.default_rng(1).standard_normal((2, 1000)).astype(np.float32)
    tx = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    y = F.silu(tx)
    (y * torch.from_numpy(dz.astype(np.float64))).sum().backward()
    assert np.abs(M.silu_model(x)[0] - y.detach().numpy()).max() < 1e-13
    assert np.abs(M.silu_bwd_add_model(x, dz, dres)[0] - (tx.grad.numpy() + dres)).max() < 1e-13
    p, t = M.loss_operands(1001)
    d = (p - t).astype(np.float64)                                # the losses' input is the float32 difference
    td = torch.from_numpy(d).requires_grad_()
    F.l1_loss(td, torch.zeros_like(td)).backward()
    (s, _), grad = M.l1_model(p, t)
    assert abs(s / 1001 - float(np.abs(d).mean())) < 1e-15
    assert np.abs(grad - td.grad.numpy()).max() <= 2.0 ** -24 / 1001          # sign(d) / n, the float32 1 / n
    assert np.all(grad[d == 0] == 0) and np.any(d == 0)
    td.grad = None
    torch.sqrt(td * td + 1e-6).mean().backward()
    (_, _), (g64, band) = M.charbonnier_model(p, t, 1e-6)
    assert np.abs(g64 - td.grad.numpy()).max() < 1e-18
    _, g32 = M.charbonnier_f32(p, t, 1e-6)
    assert M.ratio(g32, g64, band) <= 1.0                          # the float32 steps lie within the stated band of the formula


@pytest.mark.parametrize("B,C", [(1, 8), (17, 24), (5, 96)])
def test_film_mlp_models_equal_float64_autograd(B, C):
    o = M.film_mlp_operands(B, C)
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    w1, b1, W2, b2, W3, b3 = (T(o[k]).requires_grad_() for k in ('w1', 'b1', 'W2', 'b2', 'W3', 'b3'))
    tt = T(o['t']).view(B, 1, 1, 1)
    tk = F.conv2d(F.silu(F.conv2d(tt, w1.view(C, 1, 1, 1), b1)), W2.view(C, C, 1, 1), b2)
    tb = F.conv2d(F.silu(tk), W3.view(C, C, 1, 1), b3)
    ((tk[:, :, 0, 0] * T(o['dtk'])).sum() + (tb[:, :, 0, 0] * T(o['dtb'])).sum()).backward()
    # the stages chained on the model's own float64 intermediates (rounded to float32 where a kernel would read them: 6e-8 apart)
    m = M.film_mlp_models(**{k: o[k] for k in ('t', 'w1', 'b1', 'W2', 'b2', 'W3', 'b3')})
    tk64 = m['tk'][0]
    m = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=tk64.astype(np.float32), dtk=o['dtk'], dtb=o['dtb'])
    m = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=tk64.astype(np.float32), dtk=o['dtk'], dtb=o['dtb'],
                          dtk_tot_dev=m['dtk_tot'][0].astype(np.float32))
    m = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=tk64.astype(np.float32), dtk=o['dtk'], dtb=o['dtb'],
                          dtk_tot_dev=m['dtk_tot'][0].astype(np.float32), da_dev=m['da'][0].astype(np.float32))
    assert rel(m['tk'][0], tk[:, :, 0, 0].detach().numpy()) < 1e-13
    assert rel(m['tb'][0], tb[:, :, 0, 0].detach().numpy()) < 1e-6
    for name, ref in (('dW3', W3.grad), ('dW2', W2.grad), ('db3', b3.grad), ('db2', b2.grad), ('dw1', w1.grad), ('db1', b1.grad)):
        assert rel(m[name][0], ref.numpy()) < 1e-5, name           # (float32-rounded intermediates between the stages)


def test_colsum_and_zero_interleave_models():
    dy = M.colsum_operands(515, 96)
    ref, bound = M.colsum_model(dy)
    assert np.array_equal(ref, torch.from_numpy(dy).double().sum(0).numpy()) or rel(ref, torch.from_numpy(dy).double().sum(0).numpy()) < 1e-15
    assert ref[5] == 0 and bound[5] == 0
    assert np.abs(ref).max() < 200.0                               # the +-1e4 offsets cancel
    for (N, H, W, C) in M.ZI_CASES:
        d = np.random.default_rng(N).standard_normal((N, (H + 1) // 2, (W + 1) // 2, C)).astype(np.float32)
        g = torch.zeros(N, H, W, C)
        g[:, ::2, ::2] = torch.from_numpy(d)
        assert np.array_equal(M.zero_interleave_model(d, H, W), g.numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# Adam: the float32 restatement is torch's CPU Adam; the kernel's old constants are not
# ---------------------------------------------------------------------------------------------------------------------------
def ulps(a, b, scale):
    """|a - b| in float32 ulps at the magnitude `scale`."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.asarray(scale, np.float32)).astype(np.float64)))


def _torch_adam_three_steps(defect, order, chained=True):
    """Three chained steps of torch's CPU Adam beside the restatement: worst distance of (exp_avg, exp_avg_sq) in ulps of the line's sum of
    absolute terms |m| + |w (g - m)| resp. of v' (all its terms are non-negative).  chained: the restatement runs its own three steps;
    otherwise it takes each step from torch's state before it, so that one step's arithmetic is what is measured."""
    n = 1001
    r = np.random.default_rng(7)
    p = r.standard_normal(n).astype(np.float32)
    grads = [(r.standard_normal(n) * 10.0 ** r.uniform(-4, 0, n)).astype(np.float32) for _ in range(3)]
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=HYP['lr'], betas=(HYP['b1'], HYP['b2']), eps=HYP['eps'], foreach=False)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = [0.0, 0.0]
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        scale = np.abs(m) + np.abs(g - m) * np.float32(0.1)
        p, m, v = M.adam_f32(p, g, m, v, t=t, defect=defect, order=order, **HYP)
        st = opt.state[tp]
        tm, tv = st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()
        worst[0] = max(worst[0], ulps(m, tm, scale))
        worst[1] = max(worst[1], ulps(v, tv, tv))
        if not chained:
            p, m, v = tp.detach().numpy().copy(), tm, tv
    return worst


def test_adam_restatement_is_torch_cpu_adam_and_the_old_constants_are_not():
    """With float32(1 - beta) the restatement in torch's order of roundings (one FMA per state line) IS torch's CPU Adam over three chained
    steps, well within the one ulp asked for; with 1.0f - float32(beta) it is not.  The kernels' own order (no FMA, (g g) w) is a rounding
    of each product away from it: per step, from the same state, w (g - m) rounded or not is half an ulp of the line and the final rounding
    one more (m': 1.5 ulp); (g g) w against (w g) g is two roundings each = 2 ulp of the term, the final rounding one more (v': 3 ulp)."""
    good, bad = _torch_adam_three_steps(None, 'torch'), _torch_adam_three_steps('omb_f32', 'torch')
    kern = _torch_adam_three_steps(None, 'kernel', chained=False)
    print(f"[bound] adam vs torch.optim.Adam(foreach=False), 3 steps, ulps (exp_avg, exp_avg_sq): float32(1 - beta) {good}, "
          f"1.0f - beta {bad}; float32(1 - beta) in the kernels' unfused order, each step from torch's state {kern}")
    assert max(good) <= 1.0
    assert bad[0] > 1.0 and bad[1] > 100.0                          # 2.2e-7 of (1 - b1) (g - m); 1.29e-5 of (1 - b2) g^2 = 200 ulp
    assert kern[0] <= 1.5 and kern[1] <= 3.0


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds hold for faithful simulations ...
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,t", [('heavy', 1), ('heavy', 100000), ('first', 1)])
def test_adam_bound_holds_for_the_restatement(kind, t):
    worst = 0.0
    for n in M.FLAT_SIZES + (M.ADAM_CAP,):
        ops = M.adam_operands(n, kind)
        val, bnd = M.adam_model(*ops, t=t, **HYP)
        sim = M.adam_f32(*ops, t=t, **HYP)
        worst = max([worst] + [M.ratio(s, v, b) for s, v, b in zip(sim, val, bnd)])
    assert show(f"adam {kind} step {t}", worst) <= 1.0


def test_loss_bounds_hold():
    for n in M.FLAT_SIZES + (M.ADAM_CAP,):
        p, t = M.loss_operands(n)
        (s, b), grad = M.l1_model(p, t)
        d = (p - t).astype(np.float64)
        r = np.random.default_rng(n).permutation(n)
        assert abs(float(np.abs(d)[r].sum()) - s) <= b                 # another order of the float64 sum
        (s, b), (g64, band) = M.charbonnier_model(p, t, 1e-6)
        e, g32 = M.charbonnier_f32(p, t, 1e-6)
        assert abs(float(e.astype(np.float64)[r].sum()) - s) <= b
        assert show(f"charbonnier grad n {n}", M.ratio(g32, g64, band)) <= 1.0


@pytest.mark.parametrize("C", M.COLSUM_C)
def test_colsum_bound_holds_for_the_simulation(C):
    worst = 0.0
    for npix in M.colsum_npix(C):
        dy = M.colsum_operands(npix, C)
        ref, bound = M.colsum_model(dy)
        worst = max(worst, M.ratio(M.colsum_sim(dy, seed=npix), ref, bound))
    assert show(f"colsum C {C}", worst) <= 1.0


def test_silu_pair_bounds_hold():
    for n in (4, 256, 260, 65536):
        x = M.silu_operands(n)
        assert M.floor_share(x) <= 0.01 + (4 if n > 64 else 2) / n          # (1 % of the drawn values + the listed neighbours: see floor_share)
        val, bnd = M.silu_model(x)
        r1 = M.ratio(M.silu_f32(x), val, bnd)
        dz, dres = np.random.default_rng(n).standard_normal((2, n)).astype(np.float32)
        val, bnd = M.silu_bwd_add_model(x, dz, dres)
        r2 = M.ratio(dres + dz * M.dsilu_f32(x), val, bnd)
        assert max(show(f"silu n {n}", r1), show(f"silu_bwd_add n {n}", r2)) <= 1.0


@pytest.mark.parametrize("C", M.FILM_C)
def test_film_silu_bounds_hold_for_the_simulation(C):
    worst = {}
    for N in (1, 3):
        for P in M.film_P(C):
            z, tk, tb, dout = M.film_silu_operands(N, P, C)
            u = z.astype(np.float64) * tk[:, None, :] + tb[:, None, :]
            assert np.abs(u).max() <= 100.0 + 1e-3 and (P * N * C < 20000 or M.floor_share(u) <= 0.01)
            out, dz, dtk, dtb = M.film_silu_sim(z, tk, tb, dout, seed=P)
            fw, bw = M.film_silu_fwd_model(z, tk, tb), M.film_silu_bwd_model(z, tk, tb, dout)
            for name, got, (val, bnd) in (('out', out, fw), ('dz', dz, bw['dz']), ('dtk', dtk, bw['dtk']), ('dtb', dtb, bw['dtb'])):
                worst[name] = max(worst.get(name, 0.0), M.ratio(got, val, bnd))
            assert np.all(dz[:, :, [3, 17]] == 0)
    for name, r in worst.items():
        assert show(f"film_silu C {C} {name}", r) <= 1.0


@pytest.mark.parametrize("B", M.MLP_B)
@pytest.mark.parametrize("C", [c for c, _ in M.MLP_C])
def test_film_mlp_bounds_hold_for_the_simulation(B, C):
    o = M.film_mlp_operands(B, C)
    sim = M.film_mlp_sim(**o)
    m = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=sim['tk'], dtk=o['dtk'], dtb=o['dtb'],
                          dtk_tot_dev=sim['dtk_tot'], da_dev=sim['da'])
    worst = max(M.ratio(sim[k], *m[k]) for k in m)
    assert show(f"film_mlp B {B} C {C}", worst) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# ... and single defects exceed them
# ---------------------------------------------------------------------------------------------------------------------------
def defect(name, r):
    print(f"[defect] {name}: worst ratio {r:.3g}")
    assert r > 1.0, name


def test_adam_defects_exceed_the_bounds():
    ops = M.adam_operands(257, 'first')
    val, bnd = M.adam_model(*ops, t=1, **HYP)
    sim = M.adam_f32(*ops, t=1, defect='omb_f32', **HYP)
    defect("adam 1.0f - b2 on v' (first step, v = 0)", M.ratio(sim[2], val[2], bnd[2]))
    ops = M.adam_operands(257, 'heavy')
    val, bnd = M.adam_model(*ops, t=1, **HYP)
    sim = M.adam_f32(*ops, t=1, defect='no_bc1', **HYP)
    defect("adam lr in place of lr / (1 - b1^t) on p' (step 1)", M.ratio(sim[0], val[0], bnd[0]))


def test_colsum_defects_exceed_the_bounds():
    dy = M.colsum_operands(8 * 32 + 1, 32)                     # the cancellation case: +-1e4 per thread, O(1) per workgroup
    ref, bound = M.colsum_model(dy)
    defect("colsum float32 thread accumulators", M.ratio(M.colsum_sim(dy, defect='f32_threads'), ref, bound))
    for npix, C in ((7, 64), (1024 * 8 * 4 + 3 * 4 + 1, 256)):
        dy = M.colsum_operands(npix, C)
        ref, bound = M.colsum_model(dy)
        defect(f"colsum without the two-in-flight loop's tail pixel, npix {npix}", M.ratio(M.colsum_sim(dy, defect='drop_tail'), ref, bound))


def test_loss_defects_are_caught():
    p, t = M.loss_operands(257)
    (_, _), grad = M.l1_model(p, t)
    d = p - t
    wrong = np.where(d >= 0, 1.0, -1.0).astype(np.float32) / np.float32(257)     # sign(0) = 1
    assert not np.array_equal(wrong, grad) and np.array_equal(wrong[d != 0], grad[d != 0])
    print(f"[defect] l1 gradient nonzero at d == 0: {int((wrong != grad).sum())} elements differ")
    _, good = M.charbonnier_f32(p, t, 1e-6)
    _, fused = M.charbonnier_f32(p, t, 1e-6, fused=True)
    sub = np.abs(d) < 2.0 ** -126
    assert not np.array_equal(good, fused) and np.array_equal(good[~sub], fused[~sub])
    print(f"[defect] charbonnier 2 gu d: {int((good != fused).sum())} elements (subnormal gu d) differ bit for bit")


def test_film_silu_and_silu_defects_exceed_the_bounds():
    z, tk, tb, dout = M.film_silu_operands(3, 97, 32)
    bw = M.film_silu_bwd_model(z, tk, tb, dout)
    _, _, dtk, _ = M.film_silu_sim(z, tk, tb, dout, defect='dtk_sum_g')
    defect("film_silu_bwd dtk summed over g", M.ratio(dtk, *bw['dtk']))
    x = M.silu_operands(260)
    dz, dres = np.random.default_rng(0).standard_normal((2, 260)).astype(np.float32)
    val, bnd = M.silu_bwd_add_model(x, dz, dres)
    defect("SiLU' without u (1 - s)", M.ratio(dres + dz * M.dsilu_f32(x, defect='no_u_term'), val, bnd))


def test_zero_interleave_and_film_mlp_defects():
    N, H, W, C = 3, 5, 7, 36
    d = np.random.default_rng(0).standard_normal((N, 3, 4, C)).astype(np.float32)
    assert not np.array_equal(M.zero_interleave_model(d, H, W, defect='floor_ho'), M.zero_interleave_model(d, H, W))
    print("[defect] zero_interleave with Ho = H / 2 on odd H: differs")
    o = M.film_mlp_operands(17, 24)
    sim = M.film_mlp_sim(**o)
    m = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=sim['tk'], dtk=o['dtk'], dtb=o['dtb'])
    bad = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=sim['tk'], dtk=o['dtk'], dtb=o['dtb'],
                            defect='mode2_no_dtk')
    defect("film_mlp mode 2 without dtk", M.ratio(bad['dtk_tot'][0], *m['dtk_tot']))
