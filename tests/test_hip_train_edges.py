"""GPU: the training step's small kernels (csrc/train.hip: Adam x2, the two losses, colsum x2, FiLM+SiLU forward / backward, SiLU and its
backward-add, zero_interleave, the sigma MLPs, weight-gradient impulses, the batch weight packer) at their edges, each against its float64
model and derived per-element bound of tests/train_model.py -- never against another kernel.

Rules of every case: each output lives inside a NaN-filled allocation with MARGIN elements in front and behind; the margins must stay NaN
and the interior must be fully overwritten; pure outputs (loss_sum, db, dtk, dtb, dw included: the launchers zero them) start as NaN.
The [parity] lines (worst |kernel - model| / bound per kernel and case; at most 1) are what profiles/train_edges_report.txt records.

Alignment: Adam and the losses take any element-aligned pointer (run here on views one element into their allocation).  The float4
kernels (yond_silu_f32, yond_silu_bwd_add_f32; colsum, film_silu and zero_interleave alike) need 16-byte aligned pointers; the two SiLU
entries refuse others (include/yond_hip.h)."""
import ctypes

import numpy as np
import pytest
import torch

import train_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 1024
HYP = dict(lr=3e-4, b1=0.9, b2=0.999, eps=1e-8)
EINVAL = -1


def lib_():
    from yond_public_amd import _lib as L
    return L, L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guard:
    """n elements inside a NaN-filled allocation (margins of MARGIN elements; shift: the view starts that many elements later).  init None:
    a pure output, NaN until the kernel writes it."""

    def __init__(self, n, init=None, dtype=torch.float32, shift=0):
        self.n, self.lo = int(n), MARGIN + shift
        self.buf = torch.full((self.lo + self.n + MARGIN,), float('nan'), dtype=dtype, device=DEV)
        self.view = self.buf[self.lo:self.lo + self.n]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def get(self, shape=None, allow_nan=False):
        """The interior as numpy, after checking that the margins are untouched and (unless allow_nan) that nothing inside is still NaN."""
        assert bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all()), "a margin was written"
        out = self.view.cpu().numpy()
        assert allow_nan or not np.isnan(out).any(), "the interior was not fully overwritten"
        return out if shape is None else out.reshape(shape)


def parity(name, r):
    print(f"[parity] {name}: worst |kernel - model| / bound = {r:.3f}")
    return r


def pmap(fn, n):
    """[fn(i) for i < n] on a thread pool (NumPy releases the GIL: the float64 models of the largest cases run on several cores)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, min(n, 16))) as ex:
        return list(ex.map(fn, range(n)))


def chunked_ratio(model, got, *ops):
    """M.ratio(got, *model(*ops)) for an elementwise model, in 16 chunks when the arrays are large."""
    k = 16 if got.size >= (1 << 20) else 1
    cut = [np.array_split(a.reshape(-1), k) for a in (got,) + ops]
    return max(pmap(lambda i: M.ratio(cut[0][i], *model(*(c[i] for c in cut[1:]))), k))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------
def run_adam(entry, ops, t, shift=0):
    L, lib = lib_()
    n = ops[0].size
    gp, gg, gm, gv = (Guard(n, a, shift=shift) for a in ops)
    if entry == 'host':
        rc = lib.yond_adam_step_f32(gp.ptr(), gg.ptr(), gm.ptr(), gv.ptr(), n, HYP['lr'], HYP['b1'], HYP['b2'], HYP['eps'], t, L.stream())
    else:
        hyp = torch.tensor(list(M.adam_hyp(HYP['lr'], HYP['b1'], t, HYP['b2'])), dtype=torch.float64).to(torch.float32).to(DEV)
        rc = lib.yond_adam_step_dev_f32(gp.ptr(), gg.ptr(), gm.ptr(), gv.ptr(), n, HYP['b1'], HYP['b2'], HYP['eps'], L.ptr(hyp), None, L.stream())
    L.check(rc, f"adam {entry}")
    torch.cuda.synchronize()
    assert np.array_equal(bits(gg.get()), bits(ops[1]))                     # the gradient is read only
    return gp.get(), gm.get(), gv.get()


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("n,shift", [(n, 0) for n in M.FLAT_SIZES + (M.ADAM_CAP,)] + [(256, 1), (M.ADAM_CAP - 1, 1)])
def test_adam_kernels_vs_model(entry, n, shift):
    """yond_adam_step_f32 / yond_adam_step_dev_f32: p', m', v' each within its bound, at step 1 and step 100,000, on heavy-tailed gradients
    (1e-12 .. 1e3, exact zeros with v = 0, subnormal v) and on the first step's state (m = v = 0: v' = (1 - b2) g^2 is where a complement
    formed as 1.0f - float32(b2) shows, 1.29e-5 against a bound of 2.4e-7)."""
    for kind, t in (('first', 1), ('heavy', 1), ('heavy', 100000)):
        ops = M.adam_operands(n, kind)
        val, bnd = M.adam_model(*ops, t=t, **HYP)
        got = run_adam(entry, ops, t, shift)
        rs = [M.ratio(g_, v_, b_) for g_, v_, b_ in zip(got, val, bnd)]
        parity(f"adam {entry} n {n} shift {shift} {kind} step {t} (p', m', v')", max(rs))
        print(f"         p' {rs[0]:.3f} m' {rs[1]:.3f} v' {rs[2]:.3f}")
        assert rs[2] <= 1.0, f"v' {kind} step {t}"
        assert rs[1] <= 1.0, f"m' {kind} step {t}"
        assert rs[0] <= 1.0, f"p' {kind} step {t}"
        z = ops[1] == 0
        assert np.all(got[1][z] == 0) and np.all(got[2][z] == 0) and np.array_equal(bits(got[0][z]), bits(ops[0][z]))   # g = m = v = 0: nothing moves


def test_adam_entries_refuse_bad_arguments():
    L, lib = lib_()
    q = torch.zeros(8, device=DEV)
    assert lib.yond_adam_step_f32(L.ptr(q), L.ptr(q), L.ptr(q), L.ptr(q), 0, 1e-3, 0.9, 0.999, 1e-8, 1, L.stream()) == EINVAL
    assert lib.yond_adam_step_f32(L.ptr(q), L.ptr(q), L.ptr(q), L.ptr(q), 8, 1e-3, 0.9, 0.999, 1e-8, 0, L.stream()) == EINVAL
    assert lib.yond_adam_step_dev_f32(L.ptr(q), L.ptr(q), L.ptr(q), L.ptr(q), 8, 0.9, 0.999, 1e-8, None, None, L.stream()) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------------------------
def run_loss(kind, p, t, shift=0, with_grad=True):
    L, lib = lib_()
    n = p.size
    gp, gt = Guard(n, p, shift=shift), Guard(n, t, shift=shift)
    gl = Guard(1, dtype=torch.float64)
    gg = Guard(n, shift=shift)
    gptr = gg.ptr() if with_grad else None
    if kind == 'l1':
        rc = lib.yond_l1_loss_f32(gp.ptr(), gt.ptr(), n, gl.ptr(), gptr, L.stream())
    else:
        rc = lib.yond_charbonnier_loss_f32(gp.ptr(), gt.ptr(), n, 1e-6, gl.ptr(), gptr, L.stream())
    L.check(rc, kind)
    torch.cuda.synchronize()
    return gl, gg


@pytest.mark.parametrize("n,shift", [(n, 0) for n in M.FLAT_SIZES + (M.ADAM_CAP,)] + [(257, 1), (M.ADAM_CAP - 1, 1)])
def test_losses_vs_model(n, shift):
    """yond_l1_loss_f32 / yond_charbonnier_loss_f32 on runs of pred == target, -0.0 and subnormal differences: loss_sum within the reordering
    bound of the float64 sum, the L1 gradient bit-equal to sign(d) float32(1 / n) (+0.0 at d == +-0), Charbonnier's bit-equal to the float32
    steps the kernel names and within 6 E of the float64 formula; the same sums with grad = NULL."""
    p, t = M.loss_operands(n)
    (s, b), grad = M.l1_model(p, t)
    gl, gg = run_loss('l1', p, t, shift)
    got = float(gl.get()[0])
    parity(f"l1 loss_sum n {n} shift {shift}", abs(got - s) / b if b else float(got != s))
    assert abs(got - s) <= b
    assert np.array_equal(bits(gg.get()), bits(grad))
    gl2, gg2 = run_loss('l1', p, t, shift, with_grad=False)
    assert abs(float(gl2.get()[0]) - s) <= b and bool(torch.isnan(gg2.buf).all())
    (s, b), (g64, band) = M.charbonnier_model(p, t, 1e-6)
    _, g32 = M.charbonnier_f32(p, t, 1e-6)
    gl, gg = run_loss('charbonnier', p, t, shift)
    got = float(gl.get()[0])
    parity(f"charbonnier loss_sum n {n} shift {shift}", abs(got - s) / b)
    assert abs(got - s) <= b
    gk = gg.get()
    assert np.array_equal(bits(gk), bits(g32))
    assert parity(f"charbonnier grad vs float64 n {n} shift {shift}", M.ratio(gk, g64, band)) <= 1.0
    gl2, gg2 = run_loss('charbonnier', p, t, shift, with_grad=False)
    assert abs(float(gl2.get()[0]) - s) <= b and bool(torch.isnan(gg2.buf).all())


def test_losses_with_a_nan_in_pred():
    """Decided in include/yond_hip.h: a NaN difference makes loss_sum NaN (the signal TrainStep's status word acts on); the gradient at that
    element is 0 for L1 (neither comparison holds) and NaN for Charbonnier; every other element is what it would be without it."""
    n, k = 1000, 613
    p, t = M.loss_operands(n)
    p[k] = np.nan
    for kind in ('l1', 'charbonnier'):
        gl, gg = run_loss(kind, p, t)
        assert np.isnan(gl.get(allow_nan=True)[0])
        g = gg.get(allow_nan=True)
        ref = M.l1_model(p, t)[1] if kind == 'l1' else M.charbonnier_f32(p, t, 1e-6)[1]
        keep = np.arange(n) != k
        assert np.array_equal(bits(g[keep]), bits(ref[keep]))
        assert (g[k] == 0) if kind == 'l1' else np.isnan(g[k])


# ---------------------------------------------------------------------------------------------------------------------------
# SiLU, SiLU backward + add
# ---------------------------------------------------------------------------------------------------------------------------
SILU_REAL_CAP = 4 * (4096 * 1024) + 4        # the grid's cap itself (4096 workgroups x 256 threads x 4 groups of four) and one group more


@pytest.mark.parametrize("n", [4, 252, 256, 260, M.SILU_CAP, SILU_REAL_CAP])
def test_silu_pair_vs_model(n):
    """yond_silu_f32 and yond_silu_bwd_add_f32 over u in [-120, 120] with both float32 neighbours of +-88.72 and of expf's overflow point,
    +-0 and subnormals, per element.  No element is excluded: below the overflow point the bound is SILU_FLOOR (printed share)."""
    L, lib = lib_()
    x = M.silu_operands(n)
    r = np.random.default_rng(n)
    dz, dres = (r.standard_normal(n).astype(np.float32) for _ in range(2))
    xd, dzd, drd = dev(x), dev(dz), dev(dres)
    gy, gx = Guard(n), Guard(n)
    L.check(lib.yond_silu_f32(L.ptr(xd), gy.ptr(), n, L.stream()), "silu")
    L.check(lib.yond_silu_bwd_add_f32(L.ptr(xd), L.ptr(dzd), L.ptr(drd), gx.ptr(), n, L.stream()), "silu_bwd_add")
    torch.cuda.synchronize()
    print(f"[parity] silu pair n {n}: {100 * M.floor_share(x):.2f} % of the elements lie below expf's overflow point (held by the floor)")
    r1 = parity(f"silu n {n}", chunked_ratio(M.silu_model, gy.get(), x))
    r2 = parity(f"silu_bwd_add n {n}", chunked_ratio(M.silu_bwd_add_model, gx.get(), x, dz, dres))
    assert r1 <= 1.0 and r2 <= 1.0


def test_silu_pair_refuses_ragged_sizes_and_misaligned_pointers():
    """n % 4 != 0 and a pointer that is not 16-byte aligned (a view one element into its allocation) are refused, nothing is written."""
    L, lib = lib_()
    x = dev(M.silu_operands(264))
    for n in (1, 255, 257):
        g = Guard(n)
        assert lib.yond_silu_f32(L.ptr(x), g.ptr(), n, L.stream()) == EINVAL
        assert lib.yond_silu_bwd_add_f32(L.ptr(x), L.ptr(x), L.ptr(x), g.ptr(), n, L.stream()) == EINVAL
        torch.cuda.synchronize()
        assert bool(torch.isnan(g.buf).all())
    g = Guard(256, shift=1)
    x1 = ctypes.c_void_p(x.data_ptr() + 4)
    assert lib.yond_silu_f32(L.ptr(x), g.ptr(), 256, L.stream()) == EINVAL
    assert lib.yond_silu_f32(x1, Guard(256).ptr(), 256, L.stream()) == EINVAL
    assert lib.yond_silu_bwd_add_f32(L.ptr(x), L.ptr(x), L.ptr(x), g.ptr(), 256, L.stream()) == EINVAL
    assert lib.yond_silu_bwd_add_f32(L.ptr(x), x1, L.ptr(x), Guard(256).ptr(), 256, L.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.buf).all())


# ---------------------------------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", M.COLSUM_C)
def test_colsum_vs_model(C):
    """yond_colsum_f32, both kernels (C = 96, 512, 1024 take colsum_wide_kernel), at one pixel, seven, either side of eight passes of one
    workgroup and the capped grid with both arms of the two-in-flight loop and its tail: per channel within the bound built from the
    workgroups' partial sums; offsets of +-1e4 that cancel; an all-zero channel exactly 0."""
    L, lib = lib_()
    for npix in M.colsum_npix(C):
        kind, nb, ppw = M.colsum_geometry(npix, C)
        dy = M.colsum_operands(npix, C)
        ref, bound = M.colsum_model(dy)
        g = Guard(C)
        dyd = dev(dy)
        L.check(lib.yond_colsum_f32(L.ptr(dyd), npix, C, g.ptr(), L.stream()), "colsum")
        torch.cuda.synchronize()
        got = g.get()
        r = parity(f"colsum {kind} C {C} npix {npix} ({nb} workgroups)", M.ratio(got, ref, bound))
        assert r <= 1.0
        assert got[5] == 0.0 and bits(got[5:6])[0] == 0
    assert lib.yond_colsum_f32(L.ptr(dyd), 0, C, g.ptr(), L.stream()) == EINVAL
    assert lib.yond_colsum_f32(L.ptr(dyd), 4, C + 8, g.ptr(), L.stream()) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# FiLM + SiLU
# ---------------------------------------------------------------------------------------------------------------------------
def run_film_silu(z, tk, tb, dout):
    L, lib = lib_()
    N, P, C = z.shape
    zd, kd, bd, dd = dev(z), dev(tk), dev(tb), dev(dout)
    go, gz, gk, gb = Guard(z.size), Guard(z.size), Guard(N * C), Guard(N * C)
    L.check(lib.yond_film_silu_f32(L.ptr(zd), L.ptr(kd), L.ptr(bd), go.ptr(), N, P, C, L.stream()), "film_silu")
    L.check(lib.yond_film_silu_bwd_f32(L.ptr(zd), L.ptr(kd), L.ptr(bd), L.ptr(dd), gz.ptr(), gk.ptr(), gb.ptr(), N, P, C, L.stream()), "film_silu_bwd")
    torch.cuda.synchronize()
    return go.get(z.shape), gz.get(z.shape), gk.get((N, C)), gb.get((N, C))


def check_film_silu(N, P, C):
    z, tk, tb, dout = M.film_silu_operands(N, P, C)
    out, dz, dtk, dtb = run_film_silu(z, tk, tb, dout)

    def image(n):                                                  # (the images are independent: one model call each, on a thread pool)
        q = slice(n, n + 1)
        fw, bw = M.film_silu_fwd_model(z[q], tk[q], tb[q]), M.film_silu_bwd_model(z[q], tk[q], tb[q], dout[q], launch_N=N)
        share = M.floor_share(z[q].astype(np.float64) * tk[q, None, :] + tb[q, None, :])
        return (M.ratio(out[q], *fw), M.ratio(dz[q], *bw['dz']), M.ratio(dtk[q], *bw['dtk']), M.ratio(dtb[q], *bw['dtb']), share)
    per = pmap(image, N)
    rs = dict(zip(('out', 'dz', 'dtk', 'dtb'), (max(c) for c in list(zip(*per))[:4])))
    print(f"[parity] film_silu N {N} P {P} C {C}: " + " ".join(f"{k} {v:.3f}" for k, v in rs.items())
          + f"  ({100 * np.mean([q[4] for q in per]):.2f} % of u below expf's overflow point)")
    assert np.all(dz[:, :, [3, 17]] == 0)                          # tk = 0: no gradient reaches z
    for k, v in rs.items():
        assert v <= 1.0, k


@pytest.mark.parametrize("C", M.FILM_C)
def test_film_silu_kernels_vs_model(C):
    """yond_film_silu_f32 / yond_film_silu_bwd_f32 called directly: out and dz per element, dtk / dtb per (n, c) within bounds proportional
    to sum_p |g z| and sum_p |g| (a quiet channel is held at its own scale); u over [-100, 100], tk = 0 channels, dout scaled 1e-4 .. 1e2 per
    channel; P = 1, either side of one workgroup pass, and 97; N = 1 and 3."""
    for N in (1, 3):
        for P in M.film_P(C):
            check_film_silu(N, P, C)


def test_film_silu_kernels_on_a_capped_grid():
    """N = 8, C = 1024, P = 2060: both launchers cap their grids at 2048 / N + 1 workgroups per image, every workgroup loops twice."""
    N, P, C = 8, 2060, 1024
    assert M.film_silu_geometry(N, P, C, True)[0] == 2048 // N + 1 < -(-P // 8)
    assert M.film_silu_geometry(N, P, C, False)[0] == 2048 // N + 1 < -(-(P * C // 4) // 2048)
    check_film_silu(N, P, C)


def test_film_silu_refuses_unsupported_widths():
    L, lib = lib_()
    q = torch.zeros(4096, device=DEV)
    g = Guard(4096)
    for C in (48, 96, 2048, 0):
        assert lib.yond_film_silu_supported(C) == 0
        assert lib.yond_film_silu_f32(L.ptr(q), L.ptr(q), L.ptr(q), g.ptr(), 1, 1, C, L.stream()) == EINVAL
        assert lib.yond_film_silu_bwd_f32(L.ptr(q), L.ptr(q), L.ptr(q), L.ptr(q), g.ptr(), g.ptr(), g.ptr(), 1, 1, C, L.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.buf).all())


# ---------------------------------------------------------------------------------------------------------------------------
# zero_interleave
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C", list(M.ZI_CASES) + [(1, 129, 128, 512),      # N H W C / 4 just beyond 8192 * 256
                                                        (2, 257, 256, 256)])     # ... and beyond 8192 * 1024: the grid is capped
def test_zero_interleave_is_exact(N, H, W, C):
    L, lib = lib_()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dy = np.random.default_rng(H * W).standard_normal((N, Ho, Wo, C)).astype(np.float32)
    dy.reshape(-1)[::97] = -0.0
    g, dyd = Guard(N * H * W * C), dev(dy)
    L.check(lib.yond_zero_interleave_f32(L.ptr(dyd), N, Ho, Wo, C, H, W, g.ptr(), L.stream()), "zero_interleave")
    torch.cuda.synchronize()
    assert np.array_equal(bits(g.get((N, H, W, C))), bits(M.zero_interleave_model(dy, H, W)))
    print(f"[parity] zero_interleave {N}x{H}x{W}x{C}: bit-equal")
    if H % 2:
        assert lib.yond_zero_interleave_f32(L.ptr(dyd), N, H // 2, Wo, C, H, W, g.ptr(), L.stream()) == EINVAL
    assert lib.yond_zero_interleave_f32(L.ptr(dyd), N, Ho, Wo, C + 2, H, W, g.ptr(), L.stream()) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# the sigma MLPs
# ---------------------------------------------------------------------------------------------------------------------------
MLP_KEYS = ('tk', 'tb', 'dtk_tot', 'da', 'dW3', 'dW2', 'db3', 'db2', 'dw1', 'db1')


def mlp_buffers(B, C, cp, o):
    """Device operands and guarded outputs of one block.  tk / tb rows have stride cp; dtk / dtb are padded with zeros to it."""
    d = {k: dev(o[k]) for k in ('t', 'w1', 'b1', 'W2', 'b2', 'W3', 'b3')}
    for k in ('dtk', 'dtb'):
        pad = np.zeros((B, cp), np.float32)
        pad[:, :C] = o[k]
        d[k] = dev(pad)
    g = dict(tk=Guard(B * cp), tb=Guard(B * cp), scratch=Guard(2 * B * C), dw1=Guard(C), db1=Guard(C), dW2=Guard(C * C), db2=Guard(C), dW3=Guard(C * C),
             db3=Guard(C))
    return d, g


def mlp_check(tag, B, C, cp, o, g):
    tk, tb = g['tk'].get((B, cp)), g['tb'].get((B, cp))
    assert np.all(bits(tk[:, C:]) == 0) and np.all(bits(tb[:, C:]) == 0)      # the channel padding is +0
    sc = g['scratch'].get()
    got = dict(tk=tk[:, :C], tb=tb[:, :C], dtk_tot=sc[:B * C].reshape(B, C), da=sc[B * C:].reshape(B, C), dW3=g['dW3'].get((C, C)),
               dW2=g['dW2'].get((C, C)), db3=g['db3'].get(), db2=g['db2'].get(), dw1=g['dw1'].get(), db1=g['db1'].get())
    m = M.film_mlp_models(o['t'], o['w1'], o['b1'], o['W2'], o['b2'], o['W3'], o['b3'], tk_dev=got['tk'], dtk=o['dtk'], dtb=o['dtb'],
                          dtk_tot_dev=got['dtk_tot'], da_dev=got['da'])
    rs = {k: M.ratio(got[k], *m[k]) for k in MLP_KEYS}
    worst = max(rs, key=rs.get)
    parity(f"film_mlp {tag} B {B} C {C} (ld {cp}), worst stage {worst}", rs[worst])
    for k in MLP_KEYS:
        assert rs[k] <= 1.0, k


@pytest.mark.parametrize("B", M.MLP_B)
def test_film_mlp_kernels_vs_model(B):
    """yond_film_mlp_fwd_f32 / _bwd_f32 and the _multi entries (all four widths in one call), every stage -- tk, tb, dtk_tot, da, dW3, dW2
    and the four vector sums -- against its model on heavy-tailed operands; a later stage is modelled on what the earlier one wrote, so each
    bound is one stage's.  C = 8 padded to 32, 24, 96, 512: ragged 16-wide tiles, a ragged 64-deep K chunk, and K = B = 1."""
    L, lib = lib_()
    blocks = []
    for C, cp in M.MLP_C:
        o = M.film_mlp_operands(B, C)
        d, g = mlp_buffers(B, C, cp, o)
        L.check(lib.yond_film_mlp_fwd_f32(L.ptr(d['t']), L.ptr(d['w1']), L.ptr(d['b1']), L.ptr(d['W2']), L.ptr(d['b2']), L.ptr(d['W3']), L.ptr(d['b3']),
                                          B, C, cp, g['tk'].ptr(), g['tb'].ptr(), L.stream()), "film_mlp_fwd")
        L.check(lib.yond_film_mlp_bwd_f32(L.ptr(d['t']), L.ptr(d['w1']), L.ptr(d['b1']), L.ptr(d['W2']), L.ptr(d['W3']), g['tk'].ptr(), L.ptr(d['dtk']),
                                          L.ptr(d['dtb']), B, C, cp, g['scratch'].ptr(), g['dw1'].ptr(), g['db1'].ptr(), g['dW2'].ptr(), g['db2'].ptr(),
                                          g['dW3'].ptr(), g['db3'].ptr(), L.stream()), "film_mlp_bwd")
        torch.cuda.synchronize()
        mlp_check("single", B, C, cp, o, g)
        blocks.append((C, cp, o, d))
    descs = (L.FilmMlpDesc * len(blocks))()
    guards = []
    for q, (C, cp, o, d) in zip(descs, blocks):
        _, g = mlp_buffers(B, C, cp, o)
        for k in ('tk', 'tb'):                                    # (the multi entries leave the padding to the caller: header)
            g[k].view.view(B, cp)[:, C:] = 0.0
        q.t, q.w1, q.b1, q.W2, q.b2, q.W3, q.b3 = (d[k].data_ptr() for k in ('t', 'w1', 'b1', 'W2', 'b2', 'W3', 'b3'))
        q.tk, q.tb, q.dtk, q.dtb, q.scratch = g['tk'].view.data_ptr(), g['tb'].view.data_ptr(), d['dtk'].data_ptr(), d['dtb'].data_ptr(), g['scratch'].view.data_ptr()
        q.dw1, q.db1, q.dW2, q.db2, q.dW3, q.db3 = (g[k].view.data_ptr() for k in ('dw1', 'db1', 'dW2', 'db2', 'dW3', 'db3'))
        q.B, q.C, q.ld = B, C, cp
        guards.append(g)
    L.check(lib.yond_film_mlp_fwd_multi_f32(ctypes.cast(descs, ctypes.c_void_p), len(blocks), L.stream()), "film_mlp_fwd_multi")
    L.check(lib.yond_film_mlp_bwd_multi_f32(ctypes.cast(descs, ctypes.c_void_p), len(blocks), L.stream()), "film_mlp_bwd_multi")
    torch.cuda.synchronize()
    for (C, cp, o, d), g in zip(blocks, guards):
        mlp_check("multi", B, C, cp, o, g)


# ---------------------------------------------------------------------------------------------------------------------------
# weight-gradient impulses: exact
# ---------------------------------------------------------------------------------------------------------------------------
def wgrad_chunk(mode, nco, N, Hk, Wk, cin, cout):
    """Rows of K space per wave, as wgrad_split of csrc/train.hip chooses them."""
    rows = N * Hk
    tiles = (cout // (32 * nco)) * (cin // 32) * (3 if (mode == 0 and nco == 2) else 1)
    target = 1024 * ((3 if nco == 2 else 2) if mode == 0 else 4)
    chunks = -(-target // tiles)
    return max(-(-rows // chunks), -(-128 // Wk))


def impulse_rows(N, Hk, chunk):
    """K-space rows to hit, {row: is it the LAST row of its image or chunk}: first and last row of the first and the last image, and the
    first and last row of every wave chunk that straddles two images."""
    rows = {0: False, (N - 1) * Hk: False, Hk - 1: True, N * Hk - 1: True}
    for r0 in range(0, N * Hk, chunk):
        r1 = min(r0 + chunk, N * Hk) - 1
        if r0 // Hk != r1 // Hk:
            rows.setdefault(r0, False)
            rows.setdefault(r1, True)
    return sorted(rows.items())


def impulse_case(mode, stride, N, H, W, cin, cout):
    """x of small integers, dy with ONE 1.0 per output channel (at most cout impulses, each in a channel of its own, so one launch carries
    them all and every dw row has one nonzero product), and the expected dw [taps][cout][cin]: the input patch under each impulse."""
    Ho, Wo = ((H + stride - 1) // stride, (W + stride - 1) // stride) if mode == 0 else ((2 * H, 2 * W) if mode == 1 else (H, W))
    r = np.random.default_rng(mode * 7 + stride + cout)
    x = r.integers(-8, 9, (N, H, W, cin)).astype(np.float32)
    Hk, Wk = (H, W) if mode == 1 else (Ho, Wo)
    nco = 2 if (cout % 64 == 0 and mode != 1) else 1
    chunk = wgrad_chunk(mode, nco, N, Hk, Wk, cin, cout)
    pos = []
    for row, last in impulse_rows(N, Hk, chunk):
        n, yk = divmod(row, Hk)
        for xk in (0, Wk - 1):
            # (transposed layer: K space is the INPUT; a first row / column takes its upper / left output pixel, a last one the lower / right,
            #  so that the output's true corners (0, 0), (0, 2W-1), (2H-1, 0), (2H-1, 2W-1) are hit)
            pos.append((n, 2 * yk + int(last), 2 * xk + (xk > 0)) if mode == 1 else (n, yk, xk))
    assert any(r0 // Hk != (min(r0 + chunk, N * Hk) - 1) // Hk for r0 in range(0, N * Hk, chunk)), "no chunk straddles two images"
    pos = pos[:cout]
    taps = {0: 9, 1: 4, 2: 1}[mode]
    dy = np.zeros((N, Ho, Wo, cout), np.float32)
    dw = np.zeros((taps, cout, cin), np.float32)
    for co, (n, y, xx) in enumerate(pos):
        dy[n, y, xx, co] = 1.0
        if mode == 0:
            for ky in range(3):
                for kx in range(3):
                    yi, xi = y * stride + ky - 1, xx * stride + kx - 1
                    if 0 <= yi < H and 0 <= xi < W:
                        dw[ky * 3 + kx, co] = x[n, yi, xi]
        elif mode == 1:
            dw[(y % 2) * 2 + (xx % 2), co] = x[n, y // 2, xx // 2]
        else:
            dw[0, co] = x[n, y, xx]
    return x, dy, dw, (Ho, Wo), len(pos)


@pytest.mark.parametrize("mode,stride", [(0, 1), (0, 2), (1, 2), (2, 1)])
@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 64)])
def test_wgrad_impulses_are_exact(mode, stride, cin, cout):
    """yond_conv_wgrad_ws_f32 (workspace and atomics) on dy = single ones: dw must equal the input patch under each impulse bit for bit, zeros
    where the patch leaves the image -- at the four corners of the first and last image and at the first / last row of a wave's row chunk
    that straddles two images (N = 3, H = 7, W = 33): halo rows may not leak across an image boundary."""
    L, lib = lib_()
    N, H, W = 3, 7, 33
    x, dy, dw, (Ho, Wo), k = impulse_case(mode, stride, N, H, W, cin, cout)
    xd, dyd = dev(x), dev(dy)
    nws = int(lib.yond_conv_wgrad_ws_bytes(N, H, W, cin, Ho, Wo, cout, mode, stride))
    assert nws > 0
    for use_ws in (True, False):
        ws = torch.full((nws // 4,), float('nan'), device=DEV)
        g = Guard(dw.size)
        L.check(lib.yond_conv_wgrad_ws_f32(L.ptr(xd), L.ptr(dyd), N, H, W, cin, Ho, Wo, cout, mode, stride, g.ptr(), L.ptr(ws) if use_ws else None,
                                           nws if use_ws else 0, L.stream()), "wgrad_ws")
        torch.cuda.synchronize()
        got = g.get(dw.shape)
        assert np.array_equal(got, dw), f"ws {use_ws}: {int((got != dw).sum())} of {dw.size} elements differ"
    print(f"[parity] wgrad impulses mode {mode} stride {stride} {cin}->{cout}: {k} impulses, workspace and atomics bit-equal to the patches")


@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 64)])
def test_wgrad_split_impulses_are_exact(cin, cout):
    """The same on yond_conv_wgrad_split_f32 (3x3 stride 1 on the fp16 MFMA: small integers and 1.0 are exact halves), with the bias
    gradient riding along: db[co] = 1 for each channel that carries an impulse.  The impulses stand where the fp32 kernel's are (the image
    corners and ITS row chunks' edges); this kernel slices the padded pixel space by steps_per_slice, and its own slice edges are not
    targeted here -- the corners and the rows beside every image boundary are."""
    L, lib = lib_()
    N, H, W = 3, 7, 33
    x, dy, dw, _, k = impulse_case(0, 1, N, H, W, cin, cout)
    need = int(lib.yond_conv_wgrad_split_ws_bytes(N, H, W, cin, cout))
    assert need > 0
    ws = torch.full((need // 4,), float('nan'), device=DEV)
    g = Guard(dw.size + cout)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    xd, dyd = dev(x), dev(dy)                                     # (both held until the call has run: a temporary's block is free for the next allocation)
    L.check(lib.yond_conv_wgrad_split_f32(L.ptr(xd), L.ptr(dyd), N, H, W, cin, cout, g.ptr(), 1, L.ptr(ws), need, L.ptr(status), L.stream()),
            "wgrad_split")
    torch.cuda.synchronize()
    got = g.get()
    assert int(status.item()) == 0
    assert np.array_equal(got[:dw.size].reshape(dw.shape), dw), f"{int((got[:dw.size] != dw.reshape(-1)).sum())} elements differ"
    assert np.array_equal(got[dw.size:], (np.arange(cout) < k).astype(np.float32))
    print(f"[parity] wgrad_split impulses {cin}->{cout}: {k} impulses bit-equal to the patches")


# ---------------------------------------------------------------------------------------------------------------------------
# the batch weight packer
# ---------------------------------------------------------------------------------------------------------------------------
def test_batch_weight_packer_equals_the_per_layer_packer():
    """yond_pack_conv_split_weights_batch_dev_f32 (always both halves: parts = 2) against yond_pack_conv_split_weight_dev_f32 layer by layer,
    bit for bit: the whole image against parts = 2, its h halves against parts = 1 (the layout is [...][half of 16 channels][part][tn][8]);
    the per-layer device packer against the host packer on the way.  In-range weights leave the status word alone."""
    L, lib = lib_()
    layers = [(64, 32, 3, 64), (32, 96, 1, 32), (128, 128, 3, 64)]            # cout, cin, ksize, tn
    r = np.random.default_rng(5)
    ws = [(r.standard_t(3, (co, ci, k, k)) * 0.1).astype(np.float32) for co, ci, k, _ in layers]
    ws[0].reshape(-1)[:4] = [65504.0, -65504.0, 2.0 ** -20, 0.0]              # fp16's largest value is in range
    src = Guard(sum(w.size for w in ws) + 8, np.concatenate([np.zeros(8, np.float32)] + [w.reshape(-1) for w in ws]))
    desc, so, off_d, off_g = [], 8, 0, 0
    for (co, ci, k, tn), w in zip(layers, ws):
        desc.append([so, co, ci, k * k, tn, off_d, off_g])
        so, off_d, off_g = so + w.size, off_d + w.size, off_g + w.size // 4
    dst = Guard(off_d)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    dd = torch.tensor(desc, dtype=torch.int64, device=DEV)
    L.check(lib.yond_pack_conv_split_weights_batch_dev_f32(src.ptr(), L.ptr(dd), len(layers), dst.ptr(), off_g, L.ptr(status), L.stream()), "pack batch")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    batch = dst.get().view(np.uint32)
    for (co, ci, k, tn), w, d in zip(layers, ws, desc):
        mine = batch[d[5]:d[5] + w.size]
        for parts in (2, 1):
            one = Guard(w.size * parts // 2)
            wd = dev(w)
            L.check(lib.yond_pack_conv_split_weight_dev_f32(L.ptr(wd), co, ci, k, tn, parts, one.ptr(), L.ptr(status), L.stream()), "pack layer")
            torch.cuda.synchronize()
            got = one.get().view(np.uint32)
            host = np.full(w.size * parts // 2, np.nan, np.float32)
            L.check(lib.yond_pack_conv_split_weight_f32(ctypes.c_void_p(w.ctypes.data), co, ci, k, tn, parts, ctypes.c_void_p(host.ctypes.data)), "pack host")
            assert np.array_equal(got, host.view(np.uint32))
            # [cout tile][chunk][tap][half][part][tn][8 halves] = ... [part][tn * 4 words]
            want = mine if parts == 2 else mine.reshape(-1, 2, tn * 4)[:, 0].reshape(-1)
            assert np.array_equal(got, want), f"layer {co}x{ci}x{k} parts {parts}"
        assert int(status.item()) == 0
    print("[parity] batch weight packer: three layers bit-equal to the per-layer packer (parts 2; h halves = parts 1), status silent")
    over = ws[1].copy()
    over[3, 5] = 7e4                                                          # ... and a weight beyond fp16's range is reported
    src.view[8 + ws[0].size:8 + ws[0].size + over.size].copy_(torch.from_numpy(over.reshape(-1)))
    dd = torch.tensor(desc, dtype=torch.int64, device=DEV)
    L.check(lib.yond_pack_conv_split_weights_batch_dev_f32(src.ptr(), L.ptr(dd), len(layers), dst.ptr(), off_g, L.ptr(status), L.stream()), "pack batch")
    torch.cuda.synchronize()
    assert int(status.item()) & 1
