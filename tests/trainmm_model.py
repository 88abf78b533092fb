"""Float64 references, float32 restatements, per-element bounds, single-defect variants and operand generators of the training step's three
matrix-core kernels: csrc/wgrad_split.hip (3x3 stride-1 weight gradient, split operands on the fp16 MFMA), csrc/train.hip's wgrad_rows_kernel /
wgrad_reduce64_kernel (fp32-MFMA weight gradient) and csrc/gemm_split.hip (1x1 convolutions, transposed 2x2 layers, their data gradients).
Plain NumPy, independent of the library: whatever geometry the library decides (yond_conv_wgrad_split_plan, the fp32 kernel's row chunks) is
handed in by the caller.  tests/test_trainmm_model.py (CPU) shows that the restatements stay below 1 T and that the defects exceed FACTOR T or
break bit-equality; tests/test_hip_trainmm.py (GPU) holds the kernels to the same references and bounds.

Arithmetic restated
  wgrad_split   x -> (h, l), dy -> (P = 2^11 h exactly, h, l); the image stream is padded to (H + 2)(W + 2) per image (zero halo), tap (ky, kx)
                of stream pixel g reads X at g + (ky - 1)(W + 2) + (kx - 1).  Per 16-pixel K step and tap three MFMAs P h_x, h l_x, l h_x into
                ONE fp32 accumulator.  A step is SK = 16 KS KPW pixels, wave ks takes K steps ks KPW .. ks KPW + KPW - 1 of it; a slice is
                steps_per_slice steps.  The KS waves are added in order, the sum is multiplied by 2^-11 once, the slices are added by
                wgrad_reduce64_kernel (four waves take every fourth slice with two accumulators, then (p0 + p1) + (p2 + p3)).  The bias
                gradient: a thread adds what it stages per step (fp32), one thread per channel adds the SK pixel offsets, then the slices.
  gemm_split    the same three-part form on the WEIGHTS (P_w x_h, h_w x_l, l_w x_h), 32-channel K steps = two 16-wide MFMA steps, source after
                source; x 2^-11, + bias (one rounding), plain or pixel-shuffle store.
  fp32 kernel   v_mfma_f32_32x32x2_f32 per pixel pair: fp32 products, fp32 accumulation per wave over its chunk of K-space rows; workspace
                path: (w0 + w1) + (w2 + w3) per workgroup, then wgrad_reduce64_kernel; atomics path: the waves' tiles meet in any order.

Bounds (all per output element; E = 2^-24, TINY = 2^-149, gamma(k) = k E / (1 - k E) of tests/train_model.py)
  split kernels T = split_model.threshold_gemm(A, Wt, ref, parts=2) + walk + sub (+ epilogue), with per tap A = dY^T [Co][K], Wt = the shifted X
                [K][Ci], K = the stream length N (H + 2)(W + 2) (gemm_split: A = x [P][K], Wt = B [K][n], K = all sources' channels).
                threshold_gemm has (2^-22 + sqrt(K / 16) 2^-24)(Q + |ref|) + 2^-36 floor: ONE fp32 rounding per 16-wide K step.  These kernels
                round THREE times per K step (three MFMAs into one accumulator), wgrad_split then adds KS waves per slice and the slices:
                R = 3 K / 16 + (KS + 1) nslices roundings of values no larger than the partial sums (Q + |ref| as in threshold_gemm),
                independent, so  walk = (sqrt(R) - sqrt(K / 16)) 2^-24 (Q + |ref|).  The multiply by 2^-11 is exact unless the result is
                subnormal: sub = TINY per slice, only where any product is nonzero (an exactly-zero channel keeps T = 0).
                gemm_split's epilogue adds the bias with one rounding: E |y|.
  riding bias gradient   a term passes at most L = steps_per_slice + SK + ceil(nslices / 8) + 3 fp32 additions (its thread's steps, the column
                of SK pixel offsets, a reducing wave's share of the slices, the join): gamma(L) sum_p |dy|.
  fp32 kernel   every product rounds once (E) and passes the additions of its wave -- two per MFMA, chunk * ceil(Wk / 2) MFMAs -- then
                workspace: 2 (the workgroup's four waves) + ceil(wgchunks / 8) + 3 (the reduction); atomics: one per live wave but the first.
                T = (gamma(L) + E)(1 + E) sum_p |dy x| + TINY where that sum is nonzero.
The GPU tests allow FACTOR * T with split_model.FACTOR; no other constant is fixed in advance."""
import numpy as np

import split_model as S
import train_model as TM

E, TINY, gamma = TM.E, TM.TINY, TM.gamma
FACTOR = S.FACTOR
f32, f64 = np.float32, np.float64

# cfg -> (PA, PB, KS, KPW): tile pairs per workgroup, waves per tile along K, K steps per wave and step (wgrad_split.hip's five instantiations)
WGS_CFG = {1: (1, 1, 8, 1), 2: (2, 2, 2, 1), 3: (2, 4, 1, 2), 4: (2, 1, 4, 1), 5: (1, 2, 4, 1)}

WGS_DEFECTS = ('drop_l_dy_step', 'drop_l_x_step', 'P_from_v', 'scale_2e-10', 'halo_leak', 'skip_partial_step', 'bias_double_count', 'oihw_swap')
GEMM_DEFECTS = ('k_mask_block', 'n_mask_block', 'shuffle_swap')


def wgs_sk(cfg):
    _, _, ks, kpw = WGS_CFG[cfg]
    return 16 * ks * kpw


def wgs_lead(W):
    return W + 3


# ---------------------------------------------------------------------------------------------------------------------------
# shared: the taps' operand pairs, the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def tap_operands(x, dy, mode=0, stride=1):
    """[(D [R][Wk][Co], X [R][Wk][Ci])] per tap, R = N Hk rows of K space: dw[tap] = sum over (row, column) of D^T X.
    mode 0: 3x3 pad 1 (tap = ky 3 + kx, K space = the output), 1: transposed 2x2 stride 2 (tap = ty 2 + tx, K space = the input), 2: 1x1."""
    N, H, W, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    out = []
    if mode == 0:
        s = stride
        assert (Ho, Wo) == ((H + s - 1) // s, (W + s - 1) // s)
        xp = np.zeros((N, H + 2, W + 2, Ci), x.dtype)
        xp[:, 1:-1, 1:-1] = x
        for ky in range(3):
            for kx in range(3):
                out.append((dy.reshape(N * Ho, Wo, Co), xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s].reshape(N * Ho, Wo, Ci)))
    elif mode == 1:
        assert (Ho, Wo) == (2 * H, 2 * W)
        for ty in range(2):
            for tx in range(2):
                out.append((dy[:, ty::2, tx::2].reshape(N * H, W, Co), x.reshape(N * H, W, Ci)))
    else:
        assert (Ho, Wo) == (H, W)
        out.append((dy.reshape(N * H, W, Co), x.reshape(N * H, W, Ci)))
    return out


def wgrad_ref(x, dy, mode=0, stride=1, absolute=False):
    """float64 dw [taps][Co][Ci] (absolute: of |dy| and |x| -- the sum of the products' magnitudes)."""
    g = (lambda a: np.abs(a.astype(f64))) if absolute else (lambda a: a.astype(f64))
    return np.stack([g(D).reshape(-1, D.shape[-1]).T @ g(X).reshape(-1, X.shape[-1]) for D, X in tap_operands(x, dy, mode, stride)])


def to_oihw(dw):
    """[9][Co][Ci] -> [Co][Ci][9] (an nn.Conv2d weight's order, what with_bias & 2 stores)."""
    return np.ascontiguousarray(dw.transpose(1, 2, 0))


def reduce64(ws):
    """wgrad_reduce64_kernel on ws [nchunk][...] float32: wave q adds chunks q, q + 8, .. into a0 and q + 4, q + 12, .. into a1 (the tail into
    a0), then (p0 + p1) + (p2 + p3)."""
    ws = np.asarray(ws, f32)
    n = ws.shape[0]
    part = []
    for q in range(4):
        a0, a1 = np.zeros(ws.shape[1:], f32), np.zeros(ws.shape[1:], f32)
        j = q
        while j + 4 < n:
            a0, a1 = a0 + ws[j], a1 + ws[j + 4]
            j += 8
        while j < n:
            a0 = a0 + ws[j]
            j += 4
        part.append(a0 + a1)
    return (part[0] + part[1]) + (part[2] + part[3])


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad_split
# ---------------------------------------------------------------------------------------------------------------------------
def stream(t):
    """[N][H][W][C] -> the padded pixel stream [N (H + 2)(W + 2)][C]."""
    N, H, W, C = t.shape
    p = np.zeros((N, H + 2, W + 2, C), t.dtype)
    p[:, 1:-1, 1:-1] = t
    return p.reshape(-1, C)


def wgs_slices(total, plan):
    """[(G0, nsteps)] of the plan's slices over a stream of `total` pixels."""
    cfg, nsl, sps = plan[:3]
    SK = wgs_sk(cfg)
    return [(sl * sps * SK, min(sps, -(-(total - sl * sps * SK) // SK))) for sl in range(nsl)]


def wgs_model(x, dy, plan, with_bias=1, defect=None):
    """yond_conv_wgrad_split_f32 restated: (dw float32 -- [9][Co][Ci], or [Co][Ci][9] with with_bias & 2 --, db float32 [Co]).
    plan: (cfg, nslices, steps_per_slice, ...) of yond_conv_wgrad_split_plan.  defect: None or one of WGS_DEFECTS
      drop_l_dy_step     the l half of dy is zero in the 16-pixel K step at the middle of the stream
      drop_l_x_step      the l half of x is zero in that step
      P_from_v           P = fp16(2^11 v) instead of 2^11 fp16(v)
      scale_2e-10        the tiles are stored times 2^-10
      halo_leak          X's right halo column holds the next row's (the next image's) first pixel: rows of W + 1 pixels instead of W + 2 zeros
      skip_partial_step  a slice's step count rounds the pixels left DOWN to whole steps
      bias_double_count  the batch staged during a slice's last step (the next slice's first) is counted in this slice's column sums too
      oihw_swap          the OIHW store writes [ci][co][tap]"""
    cfg, nsl, sps = (int(v) for v in plan[:3])
    _, _, KS, KPW = WGS_CFG[cfg]
    SK = 16 * KS * KPW
    x, dy = np.asarray(x, f32), np.asarray(dy, f32)
    N, H, W, Ci = x.shape
    Co = dy.shape[-1]
    W2 = W + 2
    Xs, Ds = stream(x), stream(dy)
    total = Xs.shape[0]
    if defect == 'halo_leak':
        xp = Xs.reshape(N, H + 2, W2, Ci).copy()
        flat = x.reshape(N * H, W, Ci)
        nxt = np.concatenate([flat[1:, 0], np.zeros((1, Ci), f32)]).reshape(N, H, Ci)
        xp[:, 1:H + 1, W + 1] = nxt
        Xs = xp.reshape(-1, Ci)
    hx, lx = S.split(Xs)
    h, l = S.split(Ds)
    P = ((Ds if defect == 'P_from_v' else h.astype(f32)) * f32(2048.0)).astype(np.float16)
    front, back = W2 + 1, W2 + 1 + 2 * SK
    pad = lambda a: np.concatenate([np.zeros((front, a.shape[1]), f64), a.astype(f64), np.zeros((back, a.shape[1]), f64)])
    hx, lx, P, h, l = (pad(a) for a in (hx, lx, P, h, l))
    offs = [(ky - 1) * W2 + (kx - 1) for ky in range(3) for kx in range(3)]
    hit = (total // 32) * 16                                            # first pixel of the K step the 'one step' defects hit
    ws = np.zeros((nsl, 9, Co, Ci), f32)
    for sl, (G0, nsteps) in enumerate(wgs_slices(total, plan)):
        if defect == 'skip_partial_step':
            nsteps = min(sps, (total - G0) // SK)
        acc = np.zeros((KS, 9, Co, Ci), f32)
        for s in range(nsteps):
            for ks in range(KS):
                for kp in range(KPW):
                    g0 = G0 + s * SK + 16 * (ks * KPW + kp)
                    if g0 >= total:
                        continue                                       # (past the stream: every operand is masked to zero)
                    a = slice(front + g0, front + g0 + 16)
                    AP, Ah, Al = P[a].T, h[a].T, l[a].T                 # [Co][16]
                    Bh = np.stack([hx[front + g0 + o:front + g0 + o + 16] for o in offs])     # [9][16][Ci]
                    Bl = np.stack([lx[front + g0 + o:front + g0 + o + 16] for o in offs])
                    c = acc[ks].astype(f64)
                    c = (c + AP @ Bh).astype(f32).astype(f64)
                    if not (defect == 'drop_l_x_step' and g0 == hit):
                        c = (c + Ah @ Bl).astype(f32).astype(f64)
                    if not (defect == 'drop_l_dy_step' and g0 == hit):
                        c = (c + Al @ Bh).astype(f32).astype(f64)
                    acc[ks] = c.astype(f32)
        v = acc[0]
        for ks in range(1, KS):
            v = v + acc[ks]
        ws[sl] = v * f32(2.0 ** -10 if defect == 'scale_2e-10' else 2.0 ** -11)
    dw = reduce64(ws)
    if with_bias & 2:
        dw = np.ascontiguousarray(dw.transpose(2, 1, 0)).reshape(Co, Ci, 9) if defect == 'oihw_swap' else to_oihw(dw)
    db = None
    if with_bias & 1:
        Dz = np.concatenate([Ds, np.zeros((2 * SK, Co), f32)])
        col = np.zeros((nsl, Co), f32)
        for sl, (G0, nsteps) in enumerate(wgs_slices(total, plan)):
            n = nsteps + (1 if defect == 'bias_double_count' else 0)
            batches = Dz[G0:G0 + n * SK].reshape(n, SK, Co)
            thr = np.zeros((SK, Co), f32)
            for s in range(n):
                thr = thr + batches[s]                                  # a thread: its pixel offset's value of every step
            a = np.zeros(Co, f32)
            for po in range(SK):
                a = a + thr[po]                                         # the channel's thread: the column of SK pixel offsets
            col[sl] = a
        db = reduce64(col)
    return dw, db


def wgs_threshold(x, dy, plan):
    """(ref [9][Co][Ci], T, dbref [Co], Tdb) of a 3x3 stride-1 layer under the plan (module docstring)."""
    cfg, nsl, sps = (int(v) for v in plan[:3])
    KS = WGS_CFG[cfg][2]
    SK = wgs_sk(cfg)
    x, dy = np.asarray(x, f32), np.asarray(dy, f32)
    N, H, W, Ci = x.shape
    K = N * (H + 2) * (W + 2)
    R = 3.0 * K / 16.0 + (KS + 1) * nsl
    ref, T = [], []
    for D, X in tap_operands(x, dy):
        A = np.zeros((D.shape[-1], K), f64)                             # the real pixels in front, the halo's zeros behind: a sum does not mind
        A[:, :D.shape[0] * D.shape[1]] = D.reshape(-1, D.shape[-1]).T
        Wt = np.zeros((K, Ci), f64)
        Wt[:X.shape[0] * X.shape[1]] = X.reshape(-1, Ci)
        r = A @ Wt
        Q = np.sqrt((A * A) @ (Wt * Wt))
        t = S.threshold_gemm(A, Wt, r, parts=2) + (np.sqrt(R) - np.sqrt(K / 16.0)) * E * (Q + np.abs(r)) + np.where(Q > 0, nsl * TINY, 0.0)
        ref.append(r)
        T.append(t)
    d64 = dy.astype(f64).reshape(-1, dy.shape[-1])
    L = sps + SK + -(-nsl // 8) + 3
    return np.stack(ref), np.stack(T), d64.sum(0), gamma(L) * np.abs(d64).sum(0)


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32-MFMA weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def wg32_geometry(N, Hk, Wk, chunk):
    """(live waves, workgroup chunks, MFMAs per wave) for `chunk` K-space rows per wave."""
    waves = -(-(N * Hk) // chunk)
    return waves, -(-waves // 4), chunk * ((Wk + 1) // 2)


def wg32_threshold(x, dy, mode, stride, chunk, use_ws):
    """(ref [taps][Co][Ci], T) -- module docstring."""
    D, _ = tap_operands(x, dy, mode, stride)[0]
    waves, wgchunks, mfmas = wg32_geometry(1, D.shape[0], D.shape[1], chunk)
    L = 2 * mfmas + ((2 + -(-wgchunks // 8) + 3) if use_ws else (waves - 1))
    ab = wgrad_ref(x, dy, mode, stride, absolute=True)
    return wgrad_ref(x, dy, mode, stride), (gamma(L) + E) * (1 + E) * ab + np.where(ab > 0, TINY, 0.0)


def wg32_sim(x, dy, mode, stride, chunk, use_ws, seed=0, defect=None):
    """wgrad_rows_kernel + its two ways to join the waves, in float32 NumPy: a wave adds its rows' pixels in order (product rounded, then the
    sum), the workspace path joins four waves as (w0 + w1) + (w2 + w3) and reduce64 the workgroups; the atomics path adds the waves' tiles in
    a random order.  defect 'drop_odd_tail': the last pixel of an odd-width row (the half-empty pair) is not multiplied."""
    x, dy = np.asarray(x, f32), np.asarray(dy, f32)
    ops = tap_operands(x, dy, mode, stride)
    if defect == 'drop_odd_tail':
        assert ops[0][0].shape[1] % 2 == 1
        ops = [(np.concatenate([D[:, :-1], np.zeros_like(D[:, -1:])], 1), X) for D, X in ops]
    R, Wk = ops[0][0].shape[:2]
    waves = -(-R // chunk)
    tiles = []
    for D, X in ops:
        Dp = np.zeros((waves * chunk, Wk, D.shape[-1]), f32)
        Dp[:R] = D
        Xp = np.zeros((waves * chunk, Wk, X.shape[-1]), f32)
        Xp[:R] = X
        Dp, Xp = Dp.reshape(waves, chunk * Wk, -1), Xp.reshape(waves, chunk * Wk, -1)
        acc = np.zeros((waves, D.shape[-1], X.shape[-1]), f32)
        for i in range(chunk * Wk):
            acc = acc + Dp[:, i, :, None] * Xp[:, i, None, :]
        tiles.append(acc)
    t = np.stack(tiles, 1)                                              # [waves][taps][Co][Ci]
    if use_ws:
        wg = -(-waves // 4)
        tp = np.zeros((wg * 4,) + t.shape[1:], f32)
        tp[:waves] = t
        tp = tp.reshape(wg, 4, *t.shape[1:])
        return reduce64((tp[:, 0] + tp[:, 1]) + (tp[:, 2] + tp[:, 3]))
    out = np.zeros(t.shape[1:], f32)
    for w in np.random.default_rng(seed).permutation(waves):
        out = out + t[w]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_split
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_B(w, sk_lo, sk_hi, kblk, k, k_real, sn_lo, sn_hi, nblk, n_p, n_real, defect=None):
    """The dense weight matrix [k][n_p] the kernel reads from the flat float32 array w (element 0 = the source's w pointer):
    B(k, n) = w[(k % kblk) sk_lo + (k / kblk) sk_hi + (n % nblk) sn_lo + (n / nblk) sn_hi], zero where k % kblk >= k_real or n % nblk >= n_real.
    defect 'k_mask_block' / 'n_mask_block': the mask lets one more block of 32 through (what lies behind the real extent is read)."""
    w = np.asarray(w, f32).reshape(-1)
    kk, nn = np.arange(k), np.arange(n_p)
    klo, khi, nlo, nhi = kk % kblk, kk // kblk, nn % nblk, nn // nblk
    kr = k_real + (32 if defect == 'k_mask_block' else 0)
    nr = n_real + (32 if defect == 'n_mask_block' else 0)
    ok = (klo < kr)[:, None] & (nlo < nr)[None, :]
    idx = (klo * sk_lo + khi * sk_hi)[:, None] + (nlo * sn_lo + nhi * sn_hi)[None, :]
    return np.where(ok, np.take(w, np.where(ok, idx, 0), mode='wrap'), f32(0.0)).astype(f32)


def gemm_bias(bias, nblk, n_p, n_real):
    """bias[n % nblk] where n % nblk < n_real, else 0: float32 [n_p]."""
    nlo = np.arange(n_p) % nblk
    b = np.asarray(bias, f32)
    return np.where(nlo < n_real, b[np.minimum(nlo, b.size - 1)], f32(0.0)).astype(f32)


def shuffle_store(y, N, H, W, defect=None):
    """[N H W][4 cop] -> [N][2H][2W][cop]: n = j cop + co goes to pixel (2 yy + j / 2, 2 xx + j % 2).  defect 'shuffle_swap': (j % 2, j / 2)."""
    cop = y.shape[1] // 4
    t = y.reshape(N, H, W, 2, 2, cop)                                   # [..][j / 2][j % 2][co]
    t = t.transpose(0, 1, 4, 2, 3, 5) if defect == 'shuffle_swap' else t.transpose(0, 1, 3, 2, 4, 5)
    return np.ascontiguousarray(t).reshape(N, 2 * H, 2 * W, cop)


def gemm_model(xs, Bs, bias_np=None, shuffle=None, defect=None):
    """yond_gemm_split_f32 restated: xs [P][k] float32 per source, Bs the dense [k][n_p] of gemm_B, bias_np the [n_p] of gemm_bias;
    shuffle: (N, H, W) or None.  Returns float32 [P][n_p] or [N][2H][2W][n_p / 4]."""
    acc = np.zeros((xs[0].shape[0], Bs[0].shape[1]), f64)
    for x, B in zip(xs, Bs):
        xh, xl = (a.astype(f64) for a in S.split(x))
        h, l = S.split(B)
        P = (h.astype(f32) * f32(2048.0)).astype(np.float16).astype(f64)
        h, l = h.astype(f64), l.astype(f64)
        for k0 in range(0, x.shape[1], 16):
            s = slice(k0, k0 + 16)
            acc = (acc + xh[:, s] @ P[s]).astype(f32).astype(f64)
            acc = (acc + xl[:, s] @ h[s]).astype(f32).astype(f64)
            acc = (acc + xh[:, s] @ l[s]).astype(f32).astype(f64)
    y = acc.astype(f32) * f32(2.0 ** -11)
    if bias_np is not None:
        y = y + bias_np[None, :]
    return y if shuffle is None else shuffle_store(y, *shuffle, defect=defect)


def gemm_threshold(xs, Bs, bias_np=None):
    """(y64 [P][n_p], T): threshold_gemm on the concatenated sources + the three-MFMA walk + the bias addition's rounding (module docstring)."""
    A = np.concatenate([np.asarray(x, f64) for x in xs], 1)
    Wt = np.concatenate([np.asarray(B, f64) for B in Bs], 0)
    K = A.shape[1]
    ref = A @ Wt
    Q = np.sqrt((A * A) @ (Wt * Wt))
    T = S.threshold_gemm(A, Wt, ref, parts=2) + (np.sqrt(3.0 * K / 16.0) - np.sqrt(K / 16.0)) * E * (Q + np.abs(ref)) + np.where(Q > 0, TINY, 0.0)
    if bias_np is not None:
        ref = ref + bias_np.astype(f64)[None, :]
        T = T + E * np.abs(ref)
    return ref, T


# ---------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------
def dense_wgrad(rng, N, H, W, Ci, Co, kind='plain'):
    """(x, dy) float32 on which every product, every partial sum in any order and the 2^11-scaled accumulator are exact, so that a kernel
    must equal the float64 reference bit for bit.  Values are integers times a power of two:
      plain  x, dy in -4 .. 4 (every l half is zero)
      lx     x in {-3 .. 3, +-4097, +-4099} (4097 = 4096 + 1: h = 4096, l = 2^11; 4099: h = 4100, l = -2^11), dy in -1 .. 1: the l half of X counts
      ldy    dy in {0, +-1, +-(1 + 2^-11)} (h = 1, l = 1), x in -2 .. 2: the l half of dY counts
    (never both l halves in one product: the kernels drop l l, 2^-22 relative.)  With mx, md the largest integer mantissas and K = N H W
    products per output, K mx md < 2^24 is asserted: sums of K such products have at most 24 significant bits."""
    K = N * H * W
    if kind == 'plain':
        x, dy, mx, md = rng.integers(-4, 5, (N, H, W, Ci)), rng.integers(-4, 5, (N, H, W, Co)), 4, 4
    elif kind == 'lx':
        x = rng.choice(np.array([-4099, -4097, -3, -2, -1, 0, 1, 2, 3, 4097, 4099]), (N, H, W, Ci))
        dy, mx, md = rng.integers(-1, 2, (N, H, W, Co)), 4099, 1
    elif kind == 'ldy':
        dy = rng.choice(np.array([0.0, 1.0, -1.0, 1.0 + 2.0 ** -11, -1.0 - 2.0 ** -11]), (N, H, W, Co))
        x, mx, md = rng.integers(-2, 3, (N, H, W, Ci)), 2, 2049
    else:
        raise ValueError(kind)
    assert K * mx * md < 2 ** 24, (K, mx, md)
    return x.astype(f32), dy.astype(f32)


def dense_int(rng, shape, amax, k, other):
    """Integers in -amax .. amax as float32 that enter sums of k products with a factor of magnitude <= other: k amax other < 2^24 is asserted."""
    assert k * amax * other < 2 ** 24, (k, amax, other)
    return rng.integers(-amax, amax + 1, shape).astype(f32)


def wgs_facts(case, plan):
    """What a (N, H, W, Ci, Co) case reaches under its plan (cfg, nslices, steps_per_slice, ring, lds): the facts the tests assert.
    boundaries: where the slices' first stream pixels fall -- 'image' (a multiple of the image's stream length), 'halo_col' (padded column 0 or
    W + 1), 'in_row' (a real pixel that is not its row's first); wraps: how often a slice's staging passes the end of the X ring (the last ring-
    relative position a full slice writes, 2 lead + steps SK - 1, over the ring size); tail: the pixels of the stream's last, partial step."""
    N, H, W = case[:3]
    cfg, nsl, sps, ring = (int(v) for v in plan[:4])
    SK, W2 = wgs_sk(cfg), W + 2
    Ls = (H + 2) * W2
    steps = -(-(N * Ls) // SK)
    kinds = set()
    for sl in range(1, nsl):
        n, i = divmod(sl * sps * SK, Ls)
        r, c = divmod(i, W2)
        if i == 0:
            kinds.add('image')
        elif c in (0, W + 1):
            kinds.add('halo_col')
        elif 1 <= r <= H and 1 < c <= W:
            kinds.add('in_row')
    return dict(cfg=cfg, nslices=nsl, steps=steps, partial_last=nsl > 1 and steps - (nsl - 1) * sps < sps, boundaries=kinds,
                single=nsl == 1 and steps < 8, wraps=(2 * wgs_lead(W) + sps * SK - 1) // ring, ring_mod=ring % SK, lead_gt_sk=wgs_lead(W) > SK,
                tail=N * Ls - (steps - 1) * SK)


def hard_wgrad(rng, N, H, W, Ci, Co, zero_ci=3, zero_co=5, quiet_co=7):
    """(x [N][H][W][Ci], dy [N][H][W][Co]) float32 with split_model's stress statistics: x = rand 10^U(-4, 0) with random signs, rescaled to
    max|x| = 6e4; dy = rand 10^U(-8, 0) with random signs, rescaled to max|dy| = 31.89 -- about three values in ten lie below fp16's normal
    range (2^-14), the loss-scaled gradients of deep layers.  Input channel zero_ci and output channel zero_co are exactly zero; output
    channel quiet_co is scaled to max|dy| = 2^-15: every one of its values is a subnormal half (what a bound tied to the loudest channel
    never sees)."""
    x = S.stress_acts(rng, (N, H, W, Ci), 'signed').astype(f64)
    x *= 6.0e4 / np.abs(x).max()
    dy = rng.random((N, H, W, Co)) * 10.0 ** rng.uniform(-8, 0, (N, H, W, Co)) * rng.choice([-1.0, 1.0], (N, H, W, Co))
    dy *= 31.89 / np.abs(dy).max()
    dy[..., quiet_co] *= 2.0 ** -15 / np.abs(dy[..., quiet_co]).max()
    x, dy = x.astype(f32), dy.astype(f32)
    x[..., zero_ci] = 0.0
    dy[..., zero_co] = 0.0
    assert np.abs(dy).max() <= f32(31.89) and np.abs(x).max() <= 6.0e4
    return x, dy


def hard_gemm(rng, P, k, n, zero_k=3, zero_n=5):
    """(x [P][k], w [n][k]): x as hard_wgrad's, w = split_model.stress_weights rescaled to max|w| = 30 (the kernel needs |w| < 32); input
    channel zero_k and output channel zero_n exactly zero."""
    x = S.stress_acts(rng, (P, k), 'signed').astype(f64)
    x = (x * (6.0e4 / np.abs(x).max())).astype(f32)
    w = S.stress_weights(rng, n, k, 1)[:, :, 0, 0].astype(f64)
    w = (w * (30.0 / np.abs(w).max())).astype(f32)
    x[:, zero_k] = 0.0
    w[zero_n] = 0.0
    return x, w


def ratio(got, ref, T):
    """Worst |got - ref| / T (train_model.ratio: T = 0 asks for the exact value, NaN counts as inf)."""
    return TM.ratio(got, ref, T)


def zero_share(T):
    return float(np.mean(np.asarray(T) == 0.0))


# ---------------------------------------------------------------------------------------------------------------------------
# the wgrad_split cases shared by the CPU and the GPU module: ((N, H, W, Ci, Co), the facts of wgs_facts the case is there for)
# ---------------------------------------------------------------------------------------------------------------------------
WGS_CASES = (
    ((3, 7, 33, 32, 32), dict(cfg=1, nslices=2, ring_ragged=True)),
    ((3, 7, 33, 64, 64), dict(cfg=2, boundary='in_row', lead_gt_sk=True, ring_ragged=True)),
    ((3, 7, 33, 32, 64), dict(cfg=4, nslices=3, ring_ragged=True)),
    ((3, 7, 33, 64, 32), dict(cfg=5, nslices=3, ring_ragged=True)),
    ((1, 5, 6, 384, 192), dict(cfg=3, single=True)),
    ((1, 3, 30, 384, 192), dict(cfg=3, lead_gt_sk=True, ring_ragged=True)),
    ((5, 16, 16, 32, 32), dict(cfg=1, partial_last=True)),
    ((5, 16, 16, 64, 64), dict(cfg=2, nslices=11)),
    ((2, 9, 40, 64, 64), dict(cfg=2, partial_last=True, lead_gt_sk=True)),
    ((1, 5, 38, 64, 64), dict(cfg=2, boundary='halo_col', partial_last=True)),
    ((2, 6, 30, 64, 64), dict(cfg=2, boundary='image')),
    ((1, 1, 1, 32, 32), dict(cfg=1, single=True)),
    ((1, 1, 1, 64, 64), dict(cfg=2, single=True)),
    ((2, 3, 2, 64, 32), dict(cfg=5, single=True)),
    ((2, 3, 2, 32, 64), dict(cfg=4, single=True)),
    ((1, 7, 1, 32, 32), dict(cfg=1, single=True)),
    ((1, 1, 9, 64, 64), dict(cfg=2, single=True)),
    ((1, 70, 1, 64, 64), dict(cfg=2, single=True, wraps=3, ring_ragged=True)),
    ((1, 280, 1, 32, 32), dict(cfg=1, single=True, wraps=3, ring_ragged=True)),
    # the widest row each configuration still takes, and the first width at which the plan leaves it (N = 1, H = 2)
    ((1, 2, 317, 32, 32), dict(cfg=1, ring_ragged=False)),
    ((1, 2, 237, 64, 64), dict(cfg=2)), ((1, 2, 238, 64, 64), dict(cfg=4)),
    ((1, 2, 101, 384, 192), dict(cfg=3)), ((1, 2, 102, 384, 192), dict(cfg=2)),
    ((1, 2, 381, 32, 64), dict(cfg=4)),
    ((1, 2, 205, 64, 32), dict(cfg=5)), ((1, 2, 206, 64, 32), dict(cfg=1)),
)
# the first width at which yond_conv_wgrad_split_ws_bytes is 0 (the layer stays with the fp32 kernel)
WGS_UNSUPPORTED = ((1, 2, 318, 32, 32), (1, 2, 382, 64, 64), (1, 2, 382, 32, 64), (1, 2, 318, 64, 32), (1, 2, 382, 384, 192))
# one shape per configuration for the hard operands, and the CPU module's defect cases
WGS_HARD = ((3, 7, 33, 32, 32), (2, 9, 40, 64, 64), (1, 3, 30, 384, 192), (3, 7, 33, 32, 64), (3, 7, 33, 64, 32), (5, 16, 16, 64, 64))


def check_facts(case, plan, want):
    """Assert that the plan of `case` reaches what the case is there for; returns the facts."""
    f = wgs_facts(case, plan)
    for k, v in want.items():
        if k == 'boundary':
            assert v in f['boundaries'], (case, k, v, f)
        elif k == 'wraps':
            assert f['wraps'] >= v, (case, k, v, f)
        elif k == 'ring_ragged':                                       # the ring is no multiple of the step: the wrap falls inside a batch
            assert (f['ring_mod'] != 0) == v, (case, k, v, f)
        else:
            assert f[k] == v, (case, k, v, f)
    return f
