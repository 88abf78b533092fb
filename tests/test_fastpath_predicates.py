"""CPU: the two predicates that decide which kernel a layer of the forward gets -- yond_conv_s2_tall_supported (csrc/conv_s2_tall.hip,
descriptor algo 7) and yond_gemm_k1_stationary_supported (csrc/gemm_k1_stationary.hip, algo 6).  Neither dereferences a pointer, the library
loads without a GPU: dummy non-null integers stand for the tensors.  One accepted base descriptor per predicate, ONE field changed per case.
The limits are pinned at the boundary with facts derived by hand from the kernels' layouts, not read off the predicates:
  * the per-image scale / shift vectors stay in LDS -- algo 7 has room for 1536 floats each, algo 6 for 16 images;
  * a level the template serves with folded tiles in fewer rounds of the 256 workgroups stays there;
  * 32-bit offsets: elements over the whole split-plane input (algo 7), bytes inside a chunk's four planes (both), bytes over dst (algo 6)."""
import ctypes as C

import pytest

P = 0x10000                      # a non-null pointer nobody reads


def units(H, W):
    """YOND_SP_PLANE_UNITS: 16-byte units per plane, the pixels and at least one zero unit, a multiple of 8."""
    return (H * W + 8) // 8 * 8


def desc(base, **kw):
    from yond_public_amd import _lib as L
    d = L.YondConvDesc()
    f = dict(base)
    f.update(kw)
    for k, v in f.items():
        setattr(d, k, v)
    return d


def tall(**kw):
    from yond_public_amd import _lib as L
    return int(L.load().yond_conv_s2_tall_supported(C.byref(desc(TALL, **kw))))


def stat(**kw):
    from yond_public_amd import _lib as L
    return int(L.load().yond_gemm_k1_stationary_supported(C.byref(desc(STAT, **kw))))


# the layer 0 -> 1 of the data flow at an 18 x 66 input: split planes in, planes of 4 out, the bias alone
TALL = dict(src0=P, src1=None, C0=32, C1=0, N=1, H=18, W=66, Ho=9, Wo=33, Cout=64, ksize=3, stride=2, shuffle=0, pre_act=0, post_act=0, slope=0.0,
            wpk=P, escale=None, eshift=P, ebatch=0, res=None, dst=P, tn=64, kc=16, algo=3, in_fmt=1, out_fmt=2, res_fmt=0, dst2=None)
# the decoder GEMM 2 -> 1 at 9 x 31: 128 low-resolution + 64 skip channels, 64-channel output pixels (GEMM N = 4 x 64)
STAT = dict(src0=P, src1=P, C0=128, C1=64, N=1, H=9, W=31, Ho=9, Wo=31, Cout=256, ksize=1, stride=1, shuffle=1, pre_act=0, post_act=0, slope=0.0,
            wpk=P, escale=None, eshift=P, ebatch=0, res=None, dst=P, tn=64, kc=16, algo=3, in_fmt=1, out_fmt=2, res_fmt=0, dst2=None)
SUB2 = dict(shuffle=2, C0=64, C1=80, Cout=128, out_fmt=0)         # level 1 -> 0 in the two-sub-positions form, [N][H][W][C] out

TALL_REFUSED = [
    ("algo 4", dict(algo=4)), ("algo 0", dict(algo=0)), ("stride 1", dict(stride=1, Ho=18, Wo=66)), ("stride 1, stride-2 extent", dict(stride=1)),
    ("ksize 1", dict(ksize=1)), ("shuffle 1", dict(shuffle=1)), ("tn 32", dict(tn=32)), ("tn 128", dict(tn=128)), ("src1 set", dict(src1=P)),
    ("C1 16", dict(C1=16)), ("in_fmt 0", dict(in_fmt=0)), ("out_fmt 0", dict(out_fmt=0)), ("out_fmt 1", dict(out_fmt=1)), ("res", dict(res=P)),
    ("res_fmt", dict(res_fmt=2)), ("out4_dst", dict(out4_dst=P)), ("pre_act 1", dict(pre_act=1)), ("post_act 1", dict(post_act=1)),
    ("Ho of an even input one too many", dict(Ho=10)), ("Ho one too few", dict(Ho=8)), ("Wo one too many", dict(Wo=34)), ("C0 24", dict(C0=24)),
    ("Cout 96", dict(Cout=96)), ("no input", dict(src0=None)), ("no output", dict(dst=None)), ("no weights", dict(wpk=None)), ("N 0", dict(N=0)),
]


@pytest.mark.parametrize("name,kw", TALL_REFUSED, ids=[c[0].replace(' ', '_') for c in TALL_REFUSED])
def test_s2_tall_refuses(name, kw):
    assert tall() == 1
    assert tall(**kw) == 0, name


def test_s2_tall_accepts():
    assert tall() == 1
    assert tall(algo=7) == 1
    assert tall(post_act=2, slope=0.2) == 1
    assert tall(dst2=P) == 1                                       # the second output
    assert tall(H=17, W=65) == 1                                   # odd input sizes: Ho = (H + 1) / 2
    assert tall(escale=P, ebatch=1, N=2) == 1
    assert tall(C0=16) == 1 and tall(C0=256, Cout=512) == 1        # one chunk per tile; the layer 3 -> 4
    from yond_public_amd import _lib as L
    assert int(L.load().yond_conv_s2_tall_supported(None)) == 0


def test_s2_tall_vector_room():
    """Scale and shift of every image and channel are copied into LDS once: 1536 floats each (six images of the 256-channel level)."""
    assert tall(Cout=1536) == 1 and tall(Cout=1600) == 0           # one vector for all images
    assert tall(Cout=1536, N=40) == 1                              # ... however many
    assert tall(Cout=256, C0=64, ebatch=1, escale=P, N=6) == 1     # 6 x 256 = 1536
    assert tall(Cout=256, C0=64, ebatch=1, escale=P, N=7) == 0
    assert tall(Cout=256, C0=64, ebatch=0, escale=P, N=7) == 1


def test_s2_tall_leaves_folded_levels_to_the_template_where_they_take_fewer_rounds():
    # 8 x 12 input, 256 -> 512, one image (the deepest level of the whole-forward test at 64 x 96): output 4 x 6.  Eight channel tiles of one
    # 8-row tile each; folded, the one 4-row x 8-column sub-tile is a tile per channel tile as well: 8 against 8, one round either way -- taken
    assert tall(C0=256, Cout=512, H=8, W=12, Ho=4, Wo=6) == 1
    # 11 x 13 input, 64 -> 128, 70 images: output 6 x 7 = two 4-row sub-tiles of 8 columns per image, four of them fold into a tile:
    # 140 / 4 = 35 tiles x 2 channel tiles = 70, ONE round of 256 workgroups; 4-row tiles unfolded: 2 x 70 x 2 = 280, TWO rounds -- refused
    assert tall(C0=64, Cout=128, N=70, H=11, W=13, Ho=6, Wo=7) == 0
    # ... the same level with 64 images: 256 unfolded tiles are one round as well -- taken
    assert tall(C0=64, Cout=128, N=64, H=11, W=13, Ho=6, Wo=7) == 1
    # ... and one column more than the folded forms serve (Wo = 17) is not theirs
    assert tall(C0=64, Cout=128, N=70, H=11, W=33, Ho=6, Wo=17) == 1


def test_s2_tall_offset_limits():
    # elements of the whole split-plane input, N (C0 / 16) 4 units(H, W) 4 floats, below 2^31 - 1.  256 channels, one image, one row:
    # 256 units(1, W) floats; units = 8388600 -> 2^31 - 2048 (taken), units = 8388608 -> 2^31 (refused)
    for W, want in ((8388592, 1), (8388599, 1), (8388600, 0), (8388608, 0)):
        n = 1 * (256 // 16) * 4 * units(1, W) * 4
        assert (n < 2 ** 31 - 1) == bool(want), W
        assert tall(C0=256, Cout=512, H=1, W=W, Ho=1, Wo=(W + 1) // 2) == want, (W, n)
    # ... the same count spread over images: 8 images of an eighth
    for W, want in ((1048567, 1), (1048568, 0)):
        n = 8 * (256 // 16) * 4 * units(1, W) * 4
        assert (n < 2 ** 31 - 1) == bool(want), W
        assert tall(C0=256, Cout=512, N=8, H=1, W=W, Ho=1, Wo=(W + 1) // 2) == want, (W, n)
    # bytes inside a chunk's four planes (the per-lane source offsets of the LDS-DMA): 4 x 16 units(H, W) below 2^31 - 1.  16 channels keep the
    # element count of the whole input (16 units) below its own limit
    for W, want in ((33554423, 1), (33554424, 0)):
        b = 4 * 16 * units(1, W)
        assert (b < 2 ** 31 - 1) == bool(want), W
        assert tall(C0=16, H=1, W=W, Ho=1, Wo=(W + 1) // 2) == want, (W, b)


STAT_REFUSED = [
    ("algo 4", dict(algo=4)), ("algo 0", dict(algo=0)), ("algo 7", dict(algo=7)), ("stride 2", dict(stride=2)), ("ksize 3", dict(ksize=3)),
    ("shuffle 0", dict(shuffle=0)), ("tn 32", dict(tn=32)), ("tn 128", dict(tn=128)), ("no skip tensor", dict(src1=None)), ("C1 16", dict(C1=16)),
    ("in_fmt 0", dict(in_fmt=0)), ("out_fmt 0", dict(out_fmt=0)), ("out_fmt 1", dict(out_fmt=1)), ("res", dict(res=P)), ("res_fmt", dict(res_fmt=2)),
    ("out4_dst", dict(out4_dst=P)), ("pre_act 1", dict(pre_act=1)), ("post_act 1", dict(post_act=1)), ("dst2", dict(dst2=P)),
    ("Ho of the output", dict(Ho=18, Wo=62)), ("Ho one off", dict(Ho=10)), ("Wo one off", dict(Wo=30)), ("C0 24", dict(C0=24)), ("Cout 96", dict(Cout=96)),
    ("no input", dict(src0=None)), ("no output", dict(dst=None)), ("no weights", dict(wpk=None)), ("N 0", dict(N=0)),
    # the channel patterns: 64- or 128-channel output pixels, C0 = 2 Cr low-resolution and C1 = Cr skip channels
    ("Cr 32, shuffle 1", dict(Cout=128, C0=64, C1=32)), ("Cr 256", dict(Cout=1024, C0=512, C1=256)), ("Cr 96", dict(Cout=384, C0=192, C1=96)),
    ("C0 = Cr", dict(C0=64)), ("C1 = 2 Cr", dict(C1=128)), ("C0 of the level below", dict(C0=256)), ("Cr 128 on this level's inputs", dict(Cout=512)),
    ("two sub-positions at Cr 64", dict(shuffle=2)), ("two sub-positions, planes of 4 out", dict(SUB2, out_fmt=2)),
    ("two sub-positions, C1 64", dict(SUB2, C1=64)), ("two sub-positions, C1 96", dict(SUB2, C1=96)), ("two sub-positions, C0 128", dict(SUB2, C0=128)),
    ("two sub-positions, Cout 256", dict(SUB2, Cout=256)),
]


@pytest.mark.parametrize("name,kw", STAT_REFUSED, ids=[c[0].replace(' ', '_').replace(',', '') for c in STAT_REFUSED])
def test_k1_stationary_refuses(name, kw):
    assert stat() == 1
    assert stat(**kw) == 0, name


def test_k1_stationary_accepts():
    assert stat() == 1
    assert stat(algo=6) == 1
    assert stat(post_act=2, slope=0.2) == 1
    assert stat(Cout=512, C0=256, C1=128) == 1                     # level 3 -> 2
    assert stat(**SUB2) == 1                                       # level 1 -> 0
    assert stat(**dict(SUB2, algo=6, post_act=2)) == 1
    assert stat(H=1, W=1, Ho=1, Wo=1) == 1
    from yond_public_amd import _lib as L
    assert int(L.load().yond_gemm_k1_stationary_supported(None)) == 0


def test_k1_stationary_vector_room():
    """A scale / shift pair of the tile's 64 channels per image: LDS room for 16 images."""
    assert stat(ebatch=1, escale=P, N=16) == 1 and stat(ebatch=1, escale=P, N=17) == 0
    assert stat(ebatch=0, escale=P, N=17) == 1
    assert stat(**dict(SUB2, ebatch=1, escale=P, N=16)) == 1 and stat(**dict(SUB2, ebatch=1, escale=P, N=17)) == 0


def test_k1_stationary_offset_limits():
    # dst is stored through a buffer resource with 32-bit byte offsets: N Cr (2 H) (2 W) 4 bytes below 2^31 - 1.  Cr = 64, one row:
    # 1024 W bytes; W = 2097151 -> 2^31 - 1024 (taken), W = 2097152 -> 2^31 (refused)
    for W, want in ((2097151, 1), (2097152, 0)):
        b = 1 * 64 * 2 * 2 * W * 4
        assert (b < 2 ** 31 - 1) == bool(want)
        assert stat(H=1, W=W, Ho=1, Wo=W) == want, (W, b)
    # ... over images: 3 x 699050 = 2097150 pixels (taken), 3 x 699051 = 2097153 (refused)
    for W, want in ((699050, 1), (699051, 0)):
        assert stat(N=3, H=1, W=W, Ho=1, Wo=W) == want, W
    # the two-sub-positions form: Cr = 32, 512 bytes per low-resolution pixel
    for W, want in ((4194303, 1), (4194304, 0)):
        assert stat(**dict(SUB2, H=1, W=W, Ho=1, Wo=W)) == want, W
