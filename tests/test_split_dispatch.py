"""CPU: which instantiation of the split-operand kernel a descriptor gets -- yond_conv_split_variant (csrc/conv_split.hip: the chooser of the
dispatcher behind yond_conv2d_f32 algo 3 / 4) and the table of variants (csrc/conv_split_kernel.h).  The chooser dereferences no pointer, the
library loads without a GPU: dummy non-null integers stand for the tensors.  One accepted base descriptor per family, the fields a case names
changed.  The expectations are derived by hand from the kernels' tiling, not read off the chooser:
  * a launch walks tiles of TH rows x 32 pixels x TN channels with 256 persistent workgroups, in rounds of 256 tiles;
  * 12-row tiles (64- / 128-channel kernels) need 256 tiles and lose to 8-row tiles that are >= 7 % cheaper by rounds x rows (8 r8 < 0.93 x 10.8 r12);
  * 16-row x 64 and 32-row x 32 tiles of the h-only flow, its 8-row stride-2 tiles and its 16-row decoder GEMM need 256 tiles;
  * images at most 16 / 8 pixels wide fold 2 / 4 sub-tiles into an MFMA row where the rounds say so, while a sub-tile of another image stays addressable in 32 bits;
  * 32-bit offsets: elements of a planes-of-4 tensor, elements of a whole split-plane tensor staged through registers, bytes inside a chunk's planes.
A name is <s1 | s2 | k1>_<TH>x<TN>_<split | h>_<f32 | dma | reg: input staging>_<f32 | sp: output>[_o4][_sub2][_d2][_f2 | _f4][_wres][_pre]."""
import ctypes as C

import pytest

P = 0x10000                      # a non-null pointer nobody reads
EINVAL, EUNSUPPORTED = -1, -2


def units(H, W):
    """YOND_SP_PLANE_UNITS: 16-byte units per plane, the pixels and at least one zero unit, a multiple of 8."""
    return (H * W + 8) // 8 * 8


def variant(base, **kw):
    """The variant's name, or the negative error code.  Ho / Wo follow H / W unless a case sets them.  Every name is held against the
    (stride | k1, tn, parts) of the tag engine._conv records for the same descriptor: conv_split_kernel<{stride or 'k1'},{tn},{1 if algo 4 else 2}>."""
    from yond_public_amd import _lib as L
    f = dict(base)
    f.update(kw)
    s2 = f['ksize'] == 3 and f['stride'] == 2
    f.setdefault('Ho', (f['H'] + 1) // 2 if s2 else f['H'])
    f.setdefault('Wo', (f['W'] + 1) // 2 if s2 else f['W'])
    d = L.YondConvDesc()
    for k, v in f.items():
        setattr(d, k, v)
    lib = L.load()
    v = int(lib.yond_conv_split_variant(C.byref(d)))
    if v < 0:
        return v
    name = lib.yond_conv_split_variant_name(v).decode()
    kind, tile, operands = name.split('_')[:3]
    tag = (f['stride'] if f['ksize'] == 3 else 'k1', f['tn'], 1 if f['algo'] == 4 else 2)
    assert (int(kind[1]) if kind[0] == 's' else kind, int(tile.split('x')[1]), {'split': 2, 'h': 1}[operands]) == tag, (name, tag)
    return name


def all_names():
    from yond_public_amd import _lib as L
    lib, out = L.load(), []
    while lib.yond_conv_split_variant_name(len(out)) is not None:
        out.append(lib.yond_conv_split_variant_name(len(out)).decode())
    return out


COMMON = dict(src0=P, src1=None, C1=0, N=1, H=96, W=64, shuffle=0, pre_act=0, post_act=0, slope=0.0, wpk=P, escale=None, eshift=P, ebatch=0, res=None,
              dst=P, kc=16, algo=3, in_fmt=0, out_fmt=0, res_fmt=0, dst2=None, out4_dst=None)
# a 3x3 layer on [N][H][W][C] tensors, 64 -> 64 channels at 96 x 64: 2 x 12 tiles of 8 rows
PLAIN = dict(COMMON, C0=64, Cout=64, ksize=3, stride=1, tn=64)
# the split-plane flow's block: conv1 (float32 planes of 4 in, SiLU staged, split planes out), conv2 (split planes in by LDS-DMA, residual in
# planes of 4, split planes out), a consumer that stores a float32 tensor
CONV1 = dict(PLAIN, in_fmt=2, out_fmt=1, pre_act=1)
CONV2 = dict(PLAIN, in_fmt=1, out_fmt=1, res=P, res_fmt=2)
SP_IN = dict(PLAIN, in_fmt=1)
C32 = dict(C0=32, Cout=32, tn=32)                 # the 32 -> 32 layers of level 0
C64_32 = dict(C0=64, Cout=32, tn=32)              # 32-channel tiles without the 32 -> 32 layers' resident weights
O4 = dict(out4_dst=P, out4_w=P)                   # the fused 32 -> 4 output projection
# stride 2, 32 -> 64 channels: [N][H][W][C] tensors, and the flow's form (split planes in, planes of 4 out)
S2 = dict(COMMON, C0=32, Cout=64, ksize=3, stride=2, tn=64)
S2F = dict(S2, in_fmt=1, out_fmt=2)
# the decoder GEMM 2 -> 1: 128 low-resolution + 64 skip channels, 64-channel output pixels (GEMM N = 4 x 64); its flow form; 32-channel output pixels
K1 = dict(COMMON, src1=P, C0=128, C1=64, Cout=256, ksize=1, stride=1, shuffle=1, tn=64)
K1F = dict(K1, in_fmt=1, out_fmt=2)
CR32 = dict(C0=64, C1=32, Cout=128, tn=32)
SUB2 = dict(K1F, shuffle=2, C0=64, C1=80, Cout=128, out_fmt=0)         # level 1 -> 0 in the two-sub-positions form, [N][H][W][C] out
HALF = dict(algo=4)                                  # h-only operands
# ... packed for 128-channel tiles
H128 = dict(algo=4, tn=128, C0=128, Cout=128)
# the levels of the 3000 x 4000 frame (packed 1504 x 2016): rows x columns at channels
LEVELS = [(1504, 2016, 32), (752, 1008, 64), (376, 504, 128), (188, 252, 256), (94, 126, 512)]
L1 = dict(H=752, W=1008)                          # 32 x 63 = 2016 tiles of 12 rows (8 rounds) against 32 x 94 = 3008 of 8 rows (12 rounds): 12-row tiles
BATCH16 = dict(N=64, H=16, W=16)                  # a batch of small blocks' deep level: 128 tiles of 8 rows; folded by 2: 64 x 4 sub-tiles / 2 = 128 tiles of 4 rows
BATCH8 = dict(N=64, H=8, W=8)                     # ... 64 tiles of 8 rows; folded by 4: 64 x 2 sub-tiles / 4 = 32 tiles

# every variant of the table, each with a descriptor that must get it
EXPECT = [
    # [N][H][W][C] tensors, split operands
    ("s1_8x64_split_f32_f32", PLAIN, {}), ("s1_8x64_split_f32_f32_pre", PLAIN, dict(pre_act=1)),
    ("s1_12x64_split_f32_f32", PLAIN, L1), ("s1_12x64_split_f32_f32_pre", PLAIN, dict(L1, pre_act=1)),
    ("s1_16x32_split_f32_f32", PLAIN, C32), ("s1_16x32_split_f32_f32_pre", PLAIN, dict(C32, pre_act=1)),
    ("s1_16x32_split_f32_f32_o4", PLAIN, dict(C32, **O4)), ("s1_16x32_split_f32_f32_o4_pre", PLAIN, dict(C32, pre_act=1, **O4)),
    ("s1_4x64_split_f32_f32_f2", PLAIN, BATCH16), ("s1_4x64_split_f32_f32_f4", PLAIN, BATCH8),
    ("s2_4x64_split_f32_f32", S2, {}), ("s2_4x64_h_f32_f32", S2, HALF),
    # (stride 2, 65 images of 32 x 32 -> 16 x 16: 260 tiles of 4 rows are two rounds, 130 folded ones are one; 129 of 16 x 16 -> 8 x 8: 258 against 65)
    ("s2_4x64_split_f32_f32_f2", S2, dict(N=65, H=32, W=32)), ("s2_4x64_split_f32_f32_f4", S2, dict(N=129, H=16, W=16)),
    ("k1_8x64_split_f32_f32", K1, {}), ("k1_8x32_split_f32_f32", K1, CR32),
    # ... h-only operands: 12 rows x 64, 32 rows x 32 (256 tiles: one column of 8192 rows), 128-channel tiles (level 2: 16 x 32 = 512 tiles of 12 rows,
    # 2 rounds, against 752 of 8 rows, 3 rounds)
    ("s1_8x64_h_f32_f32", PLAIN, HALF), ("s1_8x64_h_f32_f32_pre", PLAIN, dict(HALF, pre_act=1)),
    ("s1_12x64_h_f32_f32", PLAIN, dict(HALF, **L1)), ("s1_12x64_h_f32_f32_pre", PLAIN, dict(HALF, pre_act=1, **L1)),
    ("s1_16x32_h_f32_f32", PLAIN, dict(HALF, **C32)), ("s1_16x32_h_f32_f32_pre", PLAIN, dict(HALF, pre_act=1, **C32)),
    ("s1_32x32_h_f32_f32", PLAIN, dict(HALF, H=8192, W=32, **C32)), ("s1_32x32_h_f32_f32_pre", PLAIN, dict(HALF, H=8192, W=32, pre_act=1, **C32)),
    ("s1_8x128_h_f32_f32", PLAIN, H128), ("s1_8x128_h_f32_f32_pre", PLAIN, dict(H128, pre_act=1)),
    ("s1_12x128_h_f32_f32", PLAIN, dict(H128, H=376, W=504)), ("s1_12x128_h_f32_f32_pre", PLAIN, dict(H128, H=376, W=504, pre_act=1)),
    # the split-plane flow, split operands
    ("s1_8x64_split_f32_sp_pre", CONV1, {}), ("s1_8x64_split_f32_sp", CONV1, dict(pre_act=0, in_fmt=0)),
    ("s1_12x64_split_f32_sp_pre", CONV1, L1), ("s1_12x64_split_f32_sp", CONV1, dict(L1, pre_act=0, in_fmt=0)),
    ("s1_16x32_split_f32_sp_pre", CONV1, C64_32), ("s1_16x32_split_f32_sp", CONV1, dict(C64_32, pre_act=0, in_fmt=0)),
    ("s1_8x64_split_dma_sp", CONV2, {}), ("s1_12x64_split_dma_sp", CONV2, L1), ("s1_16x32_split_dma_sp", CONV2, C64_32),
    ("s1_8x64_split_dma_f32", SP_IN, {}), ("s1_12x64_split_dma_f32", SP_IN, L1), ("s1_16x32_split_dma_f32", SP_IN, C64_32),
    ("s1_16x32_split_dma_f32_o4", SP_IN, dict(C64_32, **O4)),
    ("s1_16x32_split_f32_sp_wres_pre", CONV1, C32), ("s1_16x32_split_dma_sp_wres", CONV2, C32), ("s1_16x32_split_dma_f32_o4_wres", SP_IN, dict(C32, **O4)),
    ("s1_4x64_split_dma_sp_f2", CONV2, BATCH16), ("s1_4x64_split_dma_sp_f4", CONV2, BATCH8),
    ("s1_4x64_split_f32_sp_f2_pre", CONV1, BATCH16), ("s1_4x64_split_f32_sp_f4_pre", CONV1, BATCH8),
    ("s2_4x64_split_reg_f32", S2F, {}), ("s2_4x64_split_reg_f32_d2", S2F, dict(dst2=P)),
    ("s2_4x64_split_reg_f32_f2", S2F, dict(N=65, H=32, W=32)), ("s2_4x64_split_reg_f32_d2_f2", S2F, dict(N=65, H=32, W=32, dst2=P)),
    ("s2_4x64_split_reg_f32_f4", S2F, dict(N=129, H=16, W=16)), ("s2_4x64_split_reg_f32_d2_f4", S2F, dict(N=129, H=16, W=16, dst2=P)),
    ("k1_8x64_split_reg_f32", K1F, {}), ("k1_8x32_split_reg_f32", K1F, CR32), ("k1_8x64_split_reg_f32_d2", K1F, dict(dst2=P)),
    # (the decoder GEMM, 65 images of 8 x 16: 4 channel tiles x 65 = 260 tiles, two rounds; folded by 2: 4 x 33 = 132; 8 x 8 folded by 4: 4 x 17 = 68)
    ("k1_8x64_split_reg_f32_f2", K1F, dict(N=65, H=8, W=16)), ("k1_8x64_split_reg_f32_f4", K1F, dict(N=65, H=8, W=8)),
    ("k1_8x64_split_reg_f32_sub2", SUB2, {}),
    # the flow on h-only planes.  12 rows: 3072 rows of one tile column are 256 tiles of 12 rows, 192 of 16; 16 rows: 4096 rows are 256 tiles;
    # 32 rows x 32 channels: 8192 rows
    ("s1_8x64_h_f32_sp_pre", CONV1, HALF), ("s1_12x64_h_f32_sp_pre", CONV1, dict(HALF, H=3072, W=32)), ("s1_16x64_h_f32_sp_pre", CONV1, dict(HALF, H=4096, W=32)),
    ("s1_16x32_h_f32_sp_pre", CONV1, dict(HALF, **C32)),
    ("s1_8x64_h_dma_sp", CONV2, HALF), ("s1_12x64_h_dma_sp", CONV2, dict(HALF, H=3072, W=32)), ("s1_16x64_h_dma_sp", CONV2, dict(HALF, H=4096, W=32)),
    ("s1_16x32_h_dma_sp", CONV2, dict(HALF, **C32)), ("s1_32x32_h_dma_sp", CONV2, dict(HALF, H=8192, W=32, **C32)),
    ("s1_16x32_h_dma_f32_o4", SP_IN, dict(HALF, **C32, **O4)),
    ("s1_8x128_h_f32_sp_pre", CONV1, H128), ("s1_8x128_h_dma_sp", CONV2, H128),
    # (stride 2 at 64 x 64 -> 32 x 32: four 8-row tiles an image)
    ("s2_4x64_h_reg_f32", S2F, HALF), ("s2_4x64_h_reg_f32_d2", S2F, dict(HALF, dst2=P)),
    ("s2_8x64_h_reg_f32", S2F, dict(HALF, N=64, H=64, W=64)), ("s2_8x64_h_reg_f32_d2", S2F, dict(HALF, N=64, H=64, W=64, dst2=P)),
    ("s2_8x128_h_reg_f32", S2F, dict(HALF, N=64, H=64, W=64, tn=128, C0=64, Cout=128)),
    # (the decoder GEMM at 16 x 32: four channel tiles of one 16-row tile an image)
    ("k1_8x64_h_reg_f32", K1F, HALF), ("k1_8x32_h_reg_f32", K1F, dict(HALF, **CR32)), ("k1_8x64_h_reg_f32_d2", K1F, dict(HALF, dst2=P)),
    ("k1_16x64_h_reg_f32", K1F, dict(HALF, N=64, H=16, W=32)), ("k1_8x128_h_reg_f32", K1F, dict(HALF, tn=128, C0=256, C1=128, Cout=512)),
    ("k1_8x64_h_reg_f32_sub2", SUB2, HALF),
]


@pytest.mark.parametrize("name,base,kw", EXPECT, ids=[e[0] for e in EXPECT])
def test_variant_of(name, base, kw):
    assert variant(base, **kw) == name


def test_every_variant_of_the_table_is_reached():
    names = all_names()
    assert len(names) == len(set(names)) == 83
    assert sorted(e[0] for e in EXPECT) == sorted(names)
    from yond_public_amd import _lib as L
    lib = L.load()
    assert lib.yond_conv_split_variant_name(-1) is None and lib.yond_conv_split_variant_name(len(names)) is None
    assert int(lib.yond_conv_split_variant(None)) == EINVAL
    assert variant(PLAIN, algo=0) == EINVAL and variant(PLAIN, algo=6) == EINVAL and variant(PLAIN, N=0) == EINVAL


def test_the_two_pre_forms_of_a_layer_share_a_stem():
    names = set(all_names())
    pre = [n for n in names if n.endswith('_pre')]
    assert len(pre) == 21
    # (the forms that stage a float32 tensor for a split-plane store at 16 x 64 / 8 x 128 / h-only / folded / with resident weights exist with SiLU only)
    assert sum(n[:-4] in names for n in pre) == 13


def test_frame_levels_take_12_row_tiles():
    """3000 x 4000 (packed 1504 x 2016): tiles of 12 / 8 rows and their rounds of 256 per level -- 752 x 1008 x 64: 2016 / 3008, 8 / 12 rounds;
    376 x 504 x 128: 1024 / 1504, 4 / 6; 188 x 252 x 256: 512 / 768, 2 / 3; 94 x 126 x 512: 256 / 384, 1 / 2: 8 r8 is never below 0.93 x 10.8 r12.
    Level 0 has 32 channels: the family's only 32-channel tile of the split form is 16 rows high (the 32 -> 32 layers with resident weights)."""
    for (h, w, c) in LEVELS[1:]:
        t12, t8 = (c // 64) * ((w + 31) // 32) * ((h + 11) // 12), (c // 64) * ((w + 31) // 32) * ((h + 7) // 8)
        assert t12 >= 256 and not 8000 * ((t8 + 255) // 256) < 10044 * ((t12 + 255) // 256)
        g = dict(H=h, W=w, C0=c, Cout=c)
        assert variant(PLAIN, **g) == "s1_12x64_split_f32_f32"
        assert variant(CONV1, **g) == "s1_12x64_split_f32_sp_pre" and variant(CONV2, **g) == "s1_12x64_split_dma_sp"
        assert variant(SP_IN, **g) == "s1_12x64_split_dma_f32"
        assert variant(PLAIN, algo=4, **g) == "s1_12x64_h_f32_f32"
    h, w, c = LEVELS[0]
    g = dict(H=h, W=w, **C32)
    assert variant(PLAIN, **g) == "s1_16x32_split_f32_f32"
    assert variant(CONV1, **g) == "s1_16x32_split_f32_sp_wres_pre" and variant(CONV2, **g) == "s1_16x32_split_dma_sp_wres"


def test_12_row_tiles_start_at_256_tiles():
    # one tile column, one channel tile: 3060 rows are 255 tiles of 12 rows, 3072 rows 256 (one round; 384 tiles of 8 rows are two)
    assert variant(PLAIN, H=3060, W=32) == "s1_8x64_split_f32_f32" and variant(PLAIN, H=3072, W=32) == "s1_12x64_split_f32_f32"
    assert variant(CONV2, H=3060, W=32) == "s1_8x64_split_dma_sp" and variant(CONV2, H=3072, W=32) == "s1_12x64_split_dma_sp"
    assert variant(PLAIN, H=3060, W=32, **H128) == "s1_8x128_h_f32_f32" and variant(PLAIN, H=3072, W=32, **H128) == "s1_12x128_h_f32_f32"
    # enough tiles, but 8-row tiles cheaper: 64 images of 32 x 64 are 384 tiles of 12 rows and 512 of 8 rows, two rounds each: 16 against 0.93 x 21.6
    assert variant(PLAIN, N=64, H=32, W=64) == "s1_8x64_split_f32_f32"


def test_folding_by_width():
    """8 and 16 pixels wide: folded by 4 and by 2 (EXPECT holds every folded form where it wins); 17 pixels are a plain tile; and where the
    rounds say nothing is saved, the plain tile stays."""
    assert variant(PLAIN, N=64, H=16, W=17) == "s1_8x64_split_f32_f32"
    assert variant(CONV1, N=64, H=16, W=17) == "s1_8x64_split_f32_sp_pre" and variant(CONV2, N=64, H=16, W=17) == "s1_8x64_split_dma_sp"
    assert variant(CONV2, N=64, H=16, W=9) == "s1_4x64_split_dma_sp_f2" and variant(CONV2, N=64, H=16, W=8) == "s1_4x64_split_dma_sp_f4"
    # stride 2, 32 x 32 -> 16 x 16: 64 images are 256 tiles of 4 rows, one round either way -- not folded; 65 images fold (EXPECT); 33 columns out: 17
    for base, plain in ((S2, "s2_4x64_split_f32_f32"), (S2F, "s2_4x64_split_reg_f32")):
        assert variant(base, N=64, H=32, W=32) == plain
        assert variant(base, N=65, H=32, W=33) == plain
        assert variant(base, N=128, H=16, W=16) == plain          # 8 x 8 out: 2 x 128 = 256 tiles
    # the decoder GEMM: 64 images of 8 x 16 are 4 x 64 = 256 tiles; 65 fold (EXPECT); 17 columns do not
    assert variant(K1F, N=64, H=8, W=16) == "k1_8x64_split_reg_f32" and variant(K1F, N=65, H=8, W=17) == "k1_8x64_split_reg_f32"
    # folded tiles are split operands' only
    assert variant(CONV2, algo=4, **BATCH16) == "s1_8x64_h_dma_sp" and variant(PLAIN, algo=4, **BATCH16) == "s1_8x64_h_f32_f32"


def test_folding_stops_where_another_image_leaves_32_bits():
    """A sub-tile of another image is addressed from sub-tile 0's base, at most f - 1 images further: H W C 4 f bytes below 2^31 (the plain layer:
    N H W C elements)."""
    # the flow's 3x3 layer, 16 columns, f = 2, 2048 channels: H 16 2048 8 < 2^31 <=> H < 8192.  8191 rows: 2048 sub-tile rows fold into 32 x 1024 tiles,
    # 128 rounds, against 128 rounds of 8-row tiles: 2 x 128 < 3 x 128.  8192 rows: 32 x 683 = 21856 tiles of 12 rows, 86 rounds, against 128 of 8 rows
    big = dict(W=16, C0=2048, Cout=2048)
    assert 8191 * 16 * 2048 * 4 * 2 < 2 ** 31 <= 8192 * 16 * 2048 * 4 * 2
    assert variant(CONV2, H=8191, **big) == "s1_4x64_split_dma_sp_f2" and variant(CONV2, H=8192, **big) == "s1_12x64_split_dma_sp"
    # stride 2 on planes, 32 -> 16 columns, 2048 input channels: H 32 2048 8 < 2^31 <=> H < 4096; 2048 output rows are 512 tiles of 4 rows, 256 folded
    assert variant(S2F, H=4095, W=32, C0=2048) == "s2_4x64_split_reg_f32_f2" and variant(S2F, H=4096, W=32, C0=2048) == "s2_4x64_split_reg_f32"
    # the decoder GEMM: the skip tensor has 4 C1 = 256 channels per low-resolution pixel: H 16 256 8 < 2^31 <=> H < 65536
    assert variant(K1F, H=65535, W=16) == "k1_8x64_split_reg_f32_f2" and variant(K1F, H=65536, W=16) == "k1_8x64_split_reg_f32"
    # the plain layer: H 16 2048 elements < 2^31 <=> H < 65536.  65536 rows: 32 x 5462 tiles of 12 rows, 683 rounds, against 1024 of 8 rows
    assert variant(PLAIN, H=65535, **big) == "s1_4x64_split_f32_f32_f2" and variant(PLAIN, H=65536, **big) == "s1_12x64_split_f32_f32"


def test_h_only_flow_tiles():
    # 128-channel tiles: the output channels divide by 128, or the packing is refused
    assert variant(CONV2, **H128) == "s1_8x128_h_dma_sp" and variant(CONV2, **dict(H128, C0=256, Cout=256)) == "s1_8x128_h_dma_sp"
    assert variant(CONV2, **dict(H128, Cout=192)) == EINVAL and variant(CONV1, **dict(H128, Cout=64)) == EINVAL
    assert variant(CONV2, **dict(H128, algo=3)) == EINVAL                      # split operands have no 128-channel tile
    # stride 2 on 128-channel tiles: the 8-row form alone -- 64 x 64 -> 32 x 32 is four tiles an image: 64 images are 256, 63 are 252
    s2w = dict(algo=4, tn=128, C0=64, Cout=128, H=64, W=64)
    assert variant(S2F, N=64, **s2w) == "s2_8x128_h_reg_f32" and variant(S2F, N=63, **s2w) == EUNSUPPORTED
    assert variant(S2F, N=64, dst2=P, **s2w) == EUNSUPPORTED                    # (with the second output it spills: not built)
    # ... on 64-channel tiles the 4-row form takes over below 256
    assert variant(S2F, algo=4, N=64, H=64, W=64) == "s2_8x64_h_reg_f32" and variant(S2F, algo=4, N=63, H=64, W=64) == "s2_4x64_h_reg_f32"
    assert variant(S2F, algo=4, N=63, H=64, W=64, dst2=P) == "s2_4x64_h_reg_f32_d2"
    # 16 rows x 64 channels from 256 tiles: 4096 rows of one tile column; 4080 rows are 255 (and 340 tiles of 12 rows, 2 rounds, lose to 510 of 8 rows, 2 rounds)
    for base, stem in ((CONV1, "h_f32_sp_pre"), (CONV2, "h_dma_sp")):
        assert variant(base, algo=4, H=4096, W=32) == "s1_16x64_" + stem and variant(base, algo=4, H=4080, W=32) == "s1_8x64_" + stem
        assert variant(base, algo=4, N=64, H=64, W=32) == "s1_16x64_" + stem and variant(base, algo=4, N=63, H=64, W=32) == "s1_8x64_" + stem
    # 32 rows x 32 channels likewise: 8192 rows; split-plane input only
    assert variant(CONV2, algo=4, H=8192, W=32, **C32) == "s1_32x32_h_dma_sp" and variant(CONV2, algo=4, H=8160, W=32, **C32) == "s1_16x32_h_dma_sp"
    assert variant(CONV1, algo=4, H=8192, W=32, **C32) == "s1_16x32_h_f32_sp_pre"
    assert variant(PLAIN, algo=4, H=8192, W=32, **C32) == "s1_32x32_h_f32_f32" and variant(PLAIN, algo=4, H=8160, W=32, **C32) == "s1_16x32_h_f32_f32"
    # the decoder GEMM on 16 rows: 4 channel tiles x 64 images of one tile; 63 images are 252
    assert variant(K1F, algo=4, N=64, H=16, W=32) == "k1_16x64_h_reg_f32" and variant(K1F, algo=4, N=63, H=16, W=32) == "k1_8x64_h_reg_f32"
    # h-only operands serve the flow's formats and plain 3x3 layers, nothing in between
    assert variant(K1, algo=4) == EUNSUPPORTED and variant(CONV1, algo=4, pre_act=0, in_fmt=0) == EUNSUPPORTED
    assert variant(SP_IN, algo=4) == EUNSUPPORTED and variant(S2F, algo=4, out_fmt=0) == EUNSUPPORTED


def test_resident_weights_are_the_32_to_32_layers():
    assert variant(CONV1, **C32) == "s1_16x32_split_f32_sp_wres_pre" and variant(CONV1, **C64_32) == "s1_16x32_split_f32_sp_pre"
    assert variant(CONV2, **C32) == "s1_16x32_split_dma_sp_wres" and variant(CONV2, **C64_32) == "s1_16x32_split_dma_sp"
    assert variant(CONV2, **dict(C32, src1=P, C0=16, C1=16)) == "s1_16x32_split_dma_sp_wres"       # two sources, 32 channels in all
    assert variant(SP_IN, **C32, **O4) == "s1_16x32_split_dma_f32_o4_wres"
    assert variant(CONV2, algo=4, **C32) == "s1_16x32_h_dma_sp"                                    # (measured without gain on h-only planes: not built)
    assert variant(PLAIN, **C32) == "s1_16x32_split_f32_f32"                                       # float32 tensors in and out: the three-buffer form


REFUSED = [
    # the fused projection: 32 output channels, never behind a split-plane store, split operands or the h-only flow's last convolution
    ("projection at 64 channels", PLAIN, O4, EUNSUPPORTED), ("projection at 64 channels, split planes in", SP_IN, O4, EUNSUPPORTED),
    ("projection behind a split-plane store", CONV2, dict(C32, **O4), EUNSUPPORTED), ("projection, h only, tensor in", PLAIN, dict(C32, algo=4, **O4), EUNSUPPORTED),
    ("projection on the decoder GEMM", K1, O4, EUNSUPPORTED),
    # the second output: the flow's stride-2 layers and its 64-column decoder GEMM, nothing else
    ("dst2 on a plain 3x3 layer", PLAIN, dict(dst2=P), EUNSUPPORTED), ("dst2 on conv1", CONV1, dict(dst2=P), EUNSUPPORTED), ("dst2 on conv2", CONV2, dict(dst2=P), EUNSUPPORTED),
    ("dst2 on stride 2 from a tensor", S2, dict(dst2=P), EUNSUPPORTED), ("dst2 on stride 2 to a tensor", S2F, dict(dst2=P, out_fmt=0), EUNSUPPORTED),
    ("dst2 on the plain decoder GEMM", K1, dict(dst2=P), EUNSUPPORTED), ("dst2 on 32-channel output pixels", K1F, dict(CR32, dst2=P), EUNSUPPORTED),
    # formats
    ("SiLU on split-plane input", CONV2, dict(pre_act=1), EUNSUPPORTED), ("planes of 4 out of a 3x3 layer", PLAIN, dict(out_fmt=2), EUNSUPPORTED),
    ("split planes out of stride 2", S2F, dict(out_fmt=1), EUNSUPPORTED), ("planes of 4 into stride 2", S2, dict(in_fmt=2), EUNSUPPORTED),
    ("split planes out of the decoder GEMM", K1F, dict(out_fmt=1), EUNSUPPORTED), ("planes of 4 into the decoder GEMM", K1, dict(in_fmt=2), EUNSUPPORTED),
    ("residual in planes of 4 without a split-plane store", SP_IN, dict(res=P, res_fmt=2), EUNSUPPORTED), ("residual tensor behind a split-plane store", CONV2, dict(res_fmt=0), EUNSUPPORTED),
    ("residual on conv1", CONV1, dict(res=P, res_fmt=2), EUNSUPPORTED), ("res_fmt 1", PLAIN, dict(res_fmt=1), EINVAL),
    ("residual into planes of 4, stride 2", S2F, dict(res=P), EUNSUPPORTED), ("residual on the decoder GEMM", K1, dict(res=P), EUNSUPPORTED),
    # shapes
    ("tn of another packing", PLAIN, dict(tn=32), EINVAL), ("tn 128, split operands", PLAIN, dict(tn=128, C0=128, Cout=128), EINVAL),
    ("C0 24", PLAIN, dict(C0=24), EUNSUPPORTED), ("Cout 48", PLAIN, dict(Cout=48), EUNSUPPORTED), ("stride 2 at 32 output channels", S2, dict(Cout=32, tn=32), EUNSUPPORTED),
    ("decoder GEMM, 64 input channels", K1, dict(C0=32, C1=32), EUNSUPPORTED), ("shuffle without ksize 1", PLAIN, dict(shuffle=1), EUNSUPPORTED),
    ("ksize 1 without shuffle", K1, dict(shuffle=0), EUNSUPPORTED), ("post_act 3", PLAIN, dict(post_act=3), EUNSUPPORTED), ("SiLU behind the decoder GEMM", K1, dict(post_act=1), EUNSUPPORTED),
    ("SiLU into stride 2", S2, dict(pre_act=1), EINVAL), ("SiLU into the decoder GEMM", K1, dict(pre_act=1), EUNSUPPORTED),
    ("Ho one off", PLAIN, dict(Ho=97), EINVAL), ("Wo one off", PLAIN, dict(Wo=63), EINVAL), ("stride 2, Ho of an even input one too many", S2, dict(Ho=49), EINVAL),
    ("stride 2, Wo one too few", S2, dict(Wo=31), EINVAL), ("decoder GEMM, Ho of the output", K1, dict(Ho=192, Wo=128), EUNSUPPORTED),
    ("h-only decoder GEMM without its skip tensor", K1F, dict(algo=4, src1=None), EUNSUPPORTED),
]


@pytest.mark.parametrize("name,base,kw,err", REFUSED, ids=[c[0].replace(' ', '_').replace(',', '') for c in REFUSED])
def test_refuses(name, base, kw, err):
    assert isinstance(variant(base), str)
    assert variant(base, **kw) == err, name


def test_two_sub_positions_padding_rule():
    """K = [C0 | Cr skip channels at dx = 0 | the same at dx = 1 | pad], Cr = Cout / 4 = 32: 0 <= pad < 48, pad % 16 == 0, K % 48 == 0."""
    assert variant(SUB2) == "k1_8x64_split_reg_f32_sub2"                      # C0 64, C1 80: pad 16, K 144
    assert variant(SUB2, C0=80, C1=64) == "k1_8x64_split_reg_f32_sub2"        # pad 0, K 144
    assert variant(SUB2, C0=48, C1=96) == "k1_8x64_split_reg_f32_sub2"        # pad 32, K 144
    assert variant(SUB2, C0=80, C1=112) == EUNSUPPORTED                       # pad 48, K 192: a whole step of zero weights
    assert variant(SUB2, C0=96, C1=48) == EUNSUPPORTED                        # pad -16, K 144: the dx = 1 range is short
    assert variant(SUB2, C0=72, C1=72) == EUNSUPPORTED                        # pad 8, K 144
    assert variant(SUB2, C0=64, C1=96) == EUNSUPPORTED                        # pad 32, K 160
    for kw in (dict(tn=32), dict(Cout=192, C1=112), dict(in_fmt=0), dict(out_fmt=1), dict(src1=None), dict(res=P), dict(post_act=1), dict(pre_act=1), dict(Ho=97),
               dict(ksize=3), dict(stride=2), dict(res_fmt=2)):
        assert variant(SUB2, **kw) == EUNSUPPORTED, kw
    assert variant(SUB2, out_fmt=2) == "k1_8x64_split_reg_f32_sub2" and variant(SUB2, post_act=2) == "k1_8x64_split_reg_f32_sub2"


def test_offset_limits():
    """Every 32-bit limit one step either side; a limit is `>= 2^31 - 1` refused."""
    lim = 2 ** 31 - 1
    ok = lambda v: isinstance(v, str)
    # elements of a planes-of-4 input, N max(C0, C1) H W: 2048 channels, one row
    for W, want in ((1048575, True), (1048576, False)):
        assert (2048 * W < lim) == want
        assert ok(variant(CONV1, H=1, W=W, C0=2048)) == want, W
    # elements of the whole split-plane input where it is staged through registers, N (C0 / 16) 4 units 4: 256 channels, one row: 256 units
    for W, want in ((8388599, True), (8388600, False)):
        assert (256 * units(1, W) < lim) == want
        assert ok(variant(S2F, H=1, W=W, C0=256)) == want, W
        assert ok(variant(CONV2, H=1, W=W, C0=256)) and ok(variant(SP_IN, H=1, W=W, C0=256))        # (LDS-DMA staging has no such limit)
    # ... over images: 8 of an eighth
    for W, want in ((1048567, True), (1048568, False)):
        assert (8 * 256 * units(1, W) < lim) == want
        assert ok(variant(S2F, N=8, H=1, W=W, C0=256)) == want, W
    # ... the decoder GEMM's skip tensor at twice the resolution, N (C1 / 16) 4 units(2H, 2W) 4: 128 skip channels beside 16: 128 units(2, 2W)
    for W, want in ((4194301, True), (4194302, False)):
        assert (128 * units(2, 2 * W) < lim) == want
        assert ok(variant(K1F, H=1, W=W, C0=16, C1=128)) == want, W
    # bytes inside a chunk's four planes, 4 x 16 units (the decoder GEMM: of four planes' worth, 256 units); 16 input channels keep the whole tensor below its limit
    for W, want in ((33554423, True), (33554424, False)):
        assert (64 * units(1, W) < lim) == want
        assert ok(variant(SP_IN, H=1, W=W, C0=16)) == want, W
        assert ok(variant(S2F, H=1, W=W, C0=16)) == want, W
    for W, want in ((8388599, True), (8388600, False)):
        assert (256 * units(1, W) < lim) == want
        assert ok(variant(K1F, H=1, W=W, C0=16, C1=32, Cout=128, tn=32)) == want, W
    # two sub-positions: the skip tensor has Cr = 32 channels at twice the resolution: 32 units(2, 2W); the input with 2080 channels: 2080 units(1, W)
    for W, want in ((16777213, True), (16777214, False)):
        assert (32 * units(2, 2 * W) < lim) == want
        assert ok(variant(SUB2, H=1, W=W)) == want, W
    for W, want in ((1032439, True), (1032440, False)):
        assert (2080 * units(1, W) < lim) == want and 32 * units(2, 2 * W) < lim
        assert ok(variant(SUB2, H=1, W=W, C0=2080)) == want, W
