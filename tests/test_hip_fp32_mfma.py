"""GPU: the fp32-input MFMA convolution kernels the project falls back on -- the Winograd kernel (csrc/conv_wino.hip, descriptor algo 1) and the
direct kernel conv_mfma_kernel MODE 0 (csrc/conv.hip, algo 0) -- element by element against the float64 models of tests/fp32_model.py, where their
persistent workgroups walk from tile to tile: every walk case of fp32_model.CASES (tests/test_fp32_model.py pins the regime and the launch form each
one claims) on every operand kind, 'beyond fp16' included.  Per case: dst starts as NaN and must be fully overwritten, a NaN margin behind it must stay
NaN, every element must lie within FACTOR x its own T, two runs of the launch must agree bit for bit, the launch must carry the plan.prof tag of its form,
and at most 1 % of the outputs may be ill-conditioned.  The model is evaluated in float64 on the device (torch's own kernels; the same functions are
checked on the CPU against torch's conv2d).  The [parity] lines are what profiles/fp32_fallback_report.txt records: the worst err / T per case, and for
Winograd the maximum and median of T / D and err / D, D the direct-form bound of the same output (not asserted: the measured answer to how much wider
than a direct convolution the fallback is on guard-tripping operands).
Also: the walk cases of the two 1 x 1 forms with fp16 fragments (algo 2) and with split operands (algo 5) in the same kernel; non-finite containment of
both kernels; the 3000 x 4000 frame on the fp32-mfma plan against the reference's own output."""
import numpy as np
import pytest
import torch

import fp32_model as M
import split_model as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 4096
CASE = {c['name']: c for c in M.CASES}


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """A fault of the device ends the session: every later test would only fail on the dead context."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001
        pytest.exit(f"the device faulted: {e}", returncode=3)


def bits(t):
    return t.contiguous().view(torch.int32)


def make_pc(c, o):
    """The case's layer packed at its REAL channel widths (the engine pads every input to a multiple of 32 with zero weights; the library takes
    multiples of 8 / 16), with the descriptor's (tn, kc) forced where the case says so."""
    from yond_public_amd import _lib as L
    from yond_public_amd.engine import _PackedConv, _np_ptr
    bias = None if o['bias'] is None else o['bias'].float().cpu()
    pc = _PackedConv(torch.device(DEV), o['w'].float().cpu(), bias, c['ks'], c['st'], list(c['splits']), shuffle=c['sh'])
    assert pc.coutp == c['cout']
    if list(pc.psplits) != list(c['splits']):
        cols, off = [], 0
        for s, ps in zip(c['splits'], pc.psplits):
            cols.append(pc._wp[:, off:off + s])
            off += ps
        pc._wp = np.ascontiguousarray(np.concatenate(cols, 1))
        pc.psplits, pc.cinp, pc._packed = list(c['splits']), sum(c['splits']), {}
    if c['force'] is not None:
        tn, kc = c['force']
        packed = np.empty(pc._wp.size, np.float32)
        L.check(L.load().yond_pack_conv_weight_f32(_np_ptr(pc._wp), pc.gemm_n, pc.cinp, pc.ksize, tn, kc, _np_ptr(packed)), "yond_pack_conv_weight_f32")
        wd = torch.from_numpy(packed).to(DEV)
        pc.config = lambda N, Ho, Wo, split=False: (tn, kc, wd)
    return pc


def new_plan():
    from test_hip_conv import bare_plan
    plan = bare_plan()
    plan.status = torch.zeros(4, dtype=torch.int32, device=DEV)
    plan.status_slot = 0
    plan.prof = []
    return plan


def launch(plan, pc, c, o, algo):
    """One launch into a NaN-filled allocation with a NaN margin behind it: (dst, margin, prof tag)."""
    g, gemm_n, Ho, Wo = M.case_geometry(c)
    f = 2 if c['sh'] else 1
    shape = (c['N'], f * Ho, f * Wo, c['cout'])
    n = int(np.prod(shape))
    buf = torch.full((n + MARGIN,), float('nan'), device=DEV)
    dst = buf[:n].view(shape)
    xs = [x.float().contiguous() for x in o['xs']]
    kw = {}
    if o['es'] is not None:
        kw.update(escale=o['es'].float().contiguous(), eshift=o['et'].float().contiguous(), ebatch=1)
    if o['res'] is not None:
        kw['res'] = o['res'].float().contiguous()
    if c['slope'] is not None:
        kw.update(post_act=2, slope=c['slope'])
    plan._conv(pc, xs[0], xs[1] if len(xs) > 1 else None, c['N'], c['H'], c['W'], dst, pre_act=int(c['pre']), algo=algo, **kw)
    torch.cuda.synchronize()
    return dst, buf[n:], plan.prof[-1][0]


def check(name, got, margin, m, factor=M.FACTOR):
    assert bool(torch.isnan(margin).all()), name
    assert bool(torch.isfinite(got).all()), name
    err = (got.double() - m['y']).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / m['T'])
    line = f"[parity] {name}: worst err / T = {float(r.max()):.3f}"
    if m.get('D') is not None:
        td, ed = m['T'] / m['D'], err / m['D']
        line += f"; T / D max {float(td.max()):.2f} median {float(td.median()):.2f}; err / D max {float(ed.max()):.3f} median {float(ed.median()):.3f}"
    print(line)
    bad = int((r > factor).sum())
    assert bad == 0, (name, bad, float(r.max()))


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("name", list(CASE))
def test_walk_case(name, kind):
    c = CASE[name]
    o = M.case_operands(c, kind, DEV)
    m = M.case_model(c, o)
    assert M.ill_conditioned(m) <= 0.01
    plan = new_plan()
    pc = make_pc(c, o)
    algo = 2 if c['form'].startswith('wino') else 0
    got, margin, tag = launch(plan, pc, c, o, algo)
    assert tag == M.expected_tag(c), tag
    check(f"{name} {kind}", got, margin, m)
    again, margin2, _ = launch(plan, pc, c, o, algo)
    assert torch.equal(bits(got), bits(again)), (name, int((bits(got) != bits(again)).sum()))
    assert bool(torch.isnan(margin2).all())
    assert int(plan.status.abs().sum()) == 0


K1_CASES = [n for n, c in CASE.items() if c['form'] in ('k1_64', 'k1_32')]
IN_RANGE = ('tame', 'pos', 'signed', 'big')        # operands the half-precision fragments accept: |.| <= 65504 ('beyond' is what the guard exists for)


@pytest.mark.parametrize("kind", IN_RANGE)
@pytest.mark.parametrize("name", K1_CASES)
def test_walk_case_fp16_fragments(name, kind):
    """Descriptor algo 2: the same walk with the fragments rounded to half on their way into the matrix core -- against float64 on the half-rounded
    operands, with the direct bound; the status word stays 0."""
    c = CASE[name]
    o = M.case_operands(c, kind, DEV)
    oh = dict(o, xs=[x.half().double() for x in o['xs']], w=o['w'].half().double())
    m = M.case_model(c, oh)
    plan = new_plan()
    got, margin, tag = launch(plan, make_pc(c, o), c, o, 'fp16')
    assert tag == M.expected_tag(c) + "/f16", tag
    check(f"{name} {kind} fp16 fragments", got, margin, m)
    assert int(plan.status.abs().sum()) == 0


@pytest.mark.parametrize("kind", IN_RANGE)
@pytest.mark.parametrize("name", K1_CASES)
def test_walk_case_split_operands(name, kind):
    """Descriptor algo 5: the same walk with split operands in the generic kernel -- against tests/split_model.py's bound; the status word stays 0."""
    c = CASE[name]
    o = M.case_operands(c, kind, DEV)
    x = torch.cat(o['xs'], 3)
    w = o['w']
    z = M.linear_op(x, w, 1, 1, c['sh'])
    K = sum(c['splits'])
    Q = M.linear_op(x * x, w * w, 1, 1, c['sh']).sqrt()
    sa = ((x.abs() > 0) & (x.abs() < S.SUB)).double()
    sw = ((w.abs() > 0) & (w.abs() < S.SUB)).double()
    e, _ = S.rel_eps(K, 2)
    Tz = e * (Q + z.abs()) + S.floor_unit(2) * (M.linear_op(sa, w.abs(), 1, 1, c['sh']) + M.linear_op(x.abs(), sw, 1, 1, c['sh']))
    es, et = M.film_vec(o['es'], c['N']), M.film_vec(M.case_et(o), c['N'])
    y, T = S.through_epilogue(Tz, z, es, et, post=2 if c['slope'] is not None else 0, slope=c['slope'] or 0.0, res=o['res'])
    plan = new_plan()
    pc = make_pc(c, o)
    pc.split = lambda *a, **k: None                   # (the transposed layer: not the split-operand GEMM of conv_split.hip, the generic kernel)
    got, margin, tag = launch(plan, pc, c, o, 'split')
    assert tag == M.expected_tag(c) + "/split", tag
    check(f"{name} {kind} split operands", got, margin, dict(y=y, T=T))
    assert int(plan.status.abs().sum()) == 0


# ---- non-finite containment ---------------------------------------------------------------------------------------------------------------
CONTAIN = {
    'wino': M.case('contain_wino', 'wino64', (8, 8), 64, 2, 20, 40, (), pre=True, **M.FR),
    'direct': M.case('contain_direct', 's1_64_8', (16, 16), 64, 2, 20, 40, (), pre=True, **M.FR),
}


@pytest.mark.parametrize("kernel", list(CONTAIN))
def test_non_finite_values_stay_inside_their_footprint(kernel):
    """NaN at pixel 0 of src0 and of src1 and at element 0 of res -- both kernels read offset 0 for masked lanes (issue_loads, the residual
    prefetch) -- and one +inf at an interior pixel of image 0: every output whose input footprint (3 x 3 for the direct kernel, the 4 x 4 tile of
    its 2 x 2 patch for Winograd: include/yond_hip.h) holds no non-finite value is finite and within its bound -- the far borders of image 0 and
    all of image 1 among them."""
    c = CONTAIN[kernel]
    o = M.case_operands(c, 'signed', DEV)
    clean = dict(o, xs=[x.clone() for x in o['xs']], res=o['res'].clone())
    o['xs'][0][0, 0, 0, :] = float('nan')
    o['xs'][1][0, 0, 0, :] = float('nan')
    o['res'][0, 0, 0, 0] = float('nan')
    o['xs'][0][0, 9, 21, 3] = float('inf')
    for x in clean['xs']:
        x[0, 0, 0, :] = 0.0
    clean['xs'][0][0, 9, 21, 3] = 0.0
    clean['res'][0, 0, 0, 0] = 0.0
    bad = torch.zeros(c['N'], c['H'], c['W'], 1, dtype=torch.float64, device=DEV)
    bad[0, 0, 0] = 1.0
    bad[0, 9, 21] = 1.0
    if kernel == 'wino':
        hit = M.wino_patches(bad).sum((0, 1)) > 0                                   # [N][PH][PW][1]
        hit = M.wino_unpatch([[hit, hit], [hit, hit]], c['H'], c['W'])
        assert int(hit.sum()) == 4 + 16                                             # one patch at the corner, four around the interior pixel
    else:
        hit = M.conv_nhwc(bad, torch.ones(1, 1, 3, 3, dtype=torch.float64, device=DEV)) > 0
        assert int(hit.sum()) == 4 + 9
    free = ~hit.expand(-1, -1, -1, c['cout'])
    m = M.case_model(c, clean)
    plan = new_plan()
    got, margin, tag = launch(plan, make_pc(c, o), c, o, 2 if kernel == 'wino' else 0)
    assert tag.startswith("conv_wino_kernel" if kernel == 'wino' else "conv_mfma_kernel<3,1,"), tag
    assert bool(torch.isnan(margin).all())
    assert bool(torch.isfinite(got[free]).all()), int((~torch.isfinite(got[free])).sum())
    assert bool(free[1].all()) and bool(free[0, -1].all()) and bool(free[0, :, -1].all())
    r = (got.double() - m['y']).abs()[free] / m['T'][free]
    print(f"[parity] non-finite containment, {kernel}: worst err / T outside the footprints = {float(r.max()):.3f}; "
          f"non-finite outputs {int((~torch.isfinite(got)).sum())} of {got.numel()}")
    assert float(r.max()) <= M.FACTOR


# ---- the frame size ---------------------------------------------------------------------------------------------------------------------
def test_full_cfg2_3000x4000_on_the_fp32_mfma_plan(golden):
    """The fallback's plan (every 3 x 3 layer on the Winograd kernel, 1,500 and more tiles per launch) on the 3000 x 4000 frame against THE REFERENCE's
    output (tests/golden/full_cfg2.npz), at the tolerances of the default path: 1e-4, 2e-5, PSNR within 0.01 dB."""
    from hip_common import sha
    from test_hip_pipeline import _check_full, _check_regs, _full_net
    from test_oracle_golden import FULL_PIPE, full_case
    from yond_public_amd import pipeline as P
    g = golden("full_cfg2")
    noisy, clean, arch, sd = full_case("cfg2")
    assert np.array_equal(sha(noisy), g["a_sha"])
    net = _full_net(dict(arch, precision='fp32-mfma'), sd)
    once = P.IterDenoise(noisy, net, arch, dict(FULL_PIPE, iter='once'), device=DEV)
    assert len(once['raw_dns']) == 1
    _check_regs("cfg2 3000x4000 fp32-mfma", once['regs'][0], g["a_reg0"])
    dn = _check_full("cfg2 3000x4000 fp32-mfma once vs reference", once['raw_dns'][0], g, "a_dn0")
    psnr = 10 * np.log10(1.0 / ((np.asarray(dn, np.float64) - clean) ** 2).mean())
    print(f"[parity] cfg2 3000x4000 fp32-mfma: PSNR vs clean {psnr:.5f} dB, reference {g['a_psnr'][1]:.5f} dB")
    assert abs(psnr - g["a_psnr"][1]) <= 0.01
