"""not gpu: the domain of the fp32 convolution kernels (csrc/conv_igemm.hip, csrc/conv_small.hip: routes IGEMM, N16, NARROW, PHASES, RING,
N16_WGRAD, WGD) as tests/test_gpu_igemm_domain.py walks it.

This file holds the case tables of the GPU file and `fp32_expected(case, kind)`: a Python restatement of the family's host-side predicates
with the Winograd and split-bf16 switches at 0 — choose_tile, choose_split, fwd_split, the `taps` condition of launch_fwd_tile with
taps_shape and the pair rule of launch_taps, the kmode choice, n16_geom_ok / n16_wgrad_ok / n16_wgrad_blocks, narrow_fwd_ok and the
instance choice of launch_narrow, plan_phases / phases_in_one_launch / phase_group_tiles, wgd_plan and the variant choice of launch_wgd,
wgrad_plan_split, and rows_ok / lin_any / uni of launch_wgrad_tile.  It returns (route, symbols the profiler records, reduction-split
count of the workspace query); `plan(case, kind)` gives the details (the splits each launch really takes, the summing kernel, variant tags
for what the profiler does not name).  Here it is held to pnp_conv2d_route and the three workspace queries of the built library for every
row and every pass; the GPU file holds the symbols that RAN to it.

wgrad_direct4_kernel<KK, 2, ...> (two quads per thread: nquads > 256) would need more than 1024 (tap, channel) pairs, which wgd_plan refuses
(npairs > 1024 -> use = 0): no entry point could reach it and the instance is gone, see test_direct4_two_quads_per_thread_is_unreachable.
The vector-ALU family (NARROW, WGD) lives in csrc/conv_valu.hip, the summing kernels in csrc/split_sum.h."""
import ctypes
import math

import pytest

from conftest import pkg

BK = 32
(IGEMM, N16, NARROW, WINO, X3D, X3S, PHASES, WINO_WGRAD, X3W, N16_WGRAD, WGD, RING) = range(12)     # PNP_ROUTE_* of include/pnp_hip.h

# ---- case tables: (N, H, W, C, K, R, S, stride, dil, padding) --------------------------------------------------------------------------
# forward and stride-1 data gradient (every case runs all three passes; the comment names what the row is in the table for)
FWD = [
    (2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"),         # N16 / N16 / N16_WGRAD with 32 blocks: conv_n16_kernel<16, 0|1>, wgrad_n16_kernel<16>
    (1, 92, 93, 32, 16, 3, 3, 1, 1, "VALID"),        # M = 8190: one pixel pair under the 8192 bar of N16 / NARROW / WGD -> IGEMM / IGEMM / RING
    (2, 64, 64, 16, 3, 3, 3, 1, 1, "SAME"),          # NARROW (<8, false>) / N16 on conv_c3n16_kernel<3, 1> / WGD
    (2, 64, 64, 3, 16, 3, 3, 1, 1, "SAME"),          # conv_c3n16_kernel<3, 0> / NARROW <8, false> over 16 channels of dy / wgrad_c3n16_kernel
    (65535, 1, 1, 16, 16, 3, 3, 1, 1, "SAME"),       # N16 on 1x1 maps: the largest grid z extent
    (65536, 1, 1, 16, 16, 3, 3, 1, 1, "SAME"),       # one image more: NARROW <16, true> / NARROW / WGD
    (2, 70, 66, 32, 16, 3, 3, 1, 1, "VALID"),        # conv_n16_kernel<32, 0>, ragged 8x32 tiles, VALID; data gradient: 16 -> 32 on the MFMA tiles
    (2, 70, 66, 16, 32, 3, 3, 1, 1, "SAME"),         # data gradient conv_n16_kernel<32, 1>, ragged tiles; wgrad_n16_kernel<16> with 2 filter groups
    (2049, 1, 33, 16, 16, 3, 3, 1, 1, "SAME"),       # 4098 tiles of the N16 kernels: two column tiles per workgroup (tpw = 2)
    (1, 8, 8, 160, 64, 3, 3, 1, 1, "SAME"),          # forward split 5: one channel group per split (conv_taps_kernel, odd count), summing kernel
    (1, 8, 8, 224, 32, 3, 3, 1, 1, "SAME"),          # forward split 7
    (2, 4, 4, 512, 128, 3, 3, 1, 1, "SAME"),         # planned split 18, 16 channel groups: 16 splits launch; 128x64 tile (K > 64)
    (1, 110, 128, 160, 32, 3, 3, 1, 1, "SAME"),      # 110 tiles: 4 splits planned, 5 channel groups -> 3 splits of 2, 2, 1: ragged taps split
    (1, 171, 128, 32, 128, 3, 3, 1, 1, "SAME"),      # data gradient: 171 tiles, 2 splits of 2 channel groups: conv_taps3_kernel split
    (2, 64, 64, 112, 7, 3, 3, 1, 1, "SAME"),         # K % 4 != 0: the scalar-B tile, forward split 4 of 32 chunks: 8, 8, 8, 8 (C = 112: mode 4)
    (1, 40, 40, 104, 5, 3, 3, 1, 1, "SAME"),         # scalar-B tile, 30 chunks in 3 planned splits of 10; K = 5
    (1, 30, 30, 100, 36, 3, 3, 1, 1, "SAME"),        # non-taps split with a ragged last split: 29 chunks, 3 splits of 10, 10, 9; K = 36, mode 4
    (2, 112, 112, 32, 256, 3, 3, 1, 1, "SAME"),      # 392 tiles of 128x128: conv_taps_kernel<128, 128, ...>; one channel group
    (2, 12, 12, 96, 96, 3, 3, 1, 1, "SAME"),         # C = 96, K = 96: 128x64 tile, 3 channel groups in 3 splits (odd: two-stage kernel)
    (2, 48, 48, 64, 48, 3, 3, 1, 1, "VALID"),        # K = 48: ragged second column block of the 128x32 tile; VALID; M = 4232; 2 splits of 1 group
    (2, 68, 68, 64, 96, 3, 3, 1, 1, "VALID"),        # conv_taps3_kernel<128, 64, ...> forward, un-split (138 tiles), K = 96 = 64 + 32
    (1, 116, 116, 96, 64, 3, 3, 1, 1, "SAME"),       # data gradient conv_taps3_kernel<128, 64, ..., 1, 3, 3> un-split (212 tiles); forward: 3 groups
    (3, 31, 29, 64, 100, 3, 3, 1, 1, "SAME"),        # K = 100: ragged second column block of the 128x64 tile, odd map, tiles straddle images; 2 splits
    (3, 43, 1, 32, 32, 3, 3, 1, 1, "SAME"),          # M = 129, C = 32 (one group: two-stage kernel), one-pixel-wide map; a tile straddles 3 images
    (1, 127, 1, 64, 132, 3, 3, 1, 1, "SAME"),        # M = 127; K = 132: the third column block of the 128x64 tile is 4 wide
    (2, 8, 8, 64, 32, 3, 3, 1, 1, "SAME"),           # M = 128 exactly
    (1, 3, 3, 64, 32, 3, 3, 1, 1, "VALID"),          # M = 1: one output pixel
    (2, 20, 24, 64, 96, 5, 5, 1, 1, "SAME"),         # conv_taps_kernel 5x5 (forward); data gradient 5x5: conv_fwd_kernel mode 0
    (2, 20, 24, 64, 32, 3, 3, 1, 2, "SAME"),         # dilation 2 on the taps kernels
    (1, 24, 20, 32, 64, 3, 3, 1, 3, "VALID"),        # dilation 3, VALID
    (2, 16, 16, 64, 96, 3, 3, 1, 1, "SYMMETRIC"),    # SYMMETRIC: conv_fwd_kernel mode 0 on 128x64; data gradient + sympad_bwd; conv_wgrad_kernel mode 1
    (2, 16, 18, 64, 64, 1, 1, 1, 1, "SAME"),         # 1x1: forward mode 0; data gradient conv_taps3 1x1 (two channel groups)
    (1, 20, 20, 32, 40, 7, 7, 1, 1, "SAME"),         # 7x7: mode 0 both ways
    (2, 16, 16, 32, 32, 3, 5, 1, 1, "SAME"),         # 3x5: mode 0 both ways; asymmetric filter extents
    (2, 16, 16, 16, 24, 3, 3, 1, 1, "SAME"),         # mode 4 (C = 16, incremental loaders); data gradient: mode 4 too (24 channels of dy)
    (3, 9, 7, 20, 24, 3, 3, 1, 1, "SAME"),           # mode 4, C = 20, ragged everything
    (2, 16, 16, 40, 32, 3, 3, 1, 2, "SAME"),         # mode 4, C = 40, dilation 2
    (2, 12, 12, 4, 32, 3, 3, 1, 1, "SAME"),          # mode 1: C = 4
    (2, 12, 12, 8, 36, 3, 3, 1, 1, "VALID"),         # mode 1: C = 8; K = 36
    (2, 12, 12, 12, 5, 3, 3, 1, 1, "SAME"),          # mode 1: C = 12, on the scalar-B tile (K = 5)
    (2, 12, 12, 20, 32, 3, 3, 1, 1, "SYMMETRIC"),    # mode 1 through SYMMETRIC (C % 4 == 0, C >= 16)
    (2, 12, 12, 3, 32, 3, 3, 1, 1, "SAME"),          # mode 2: C = 3 with K != 16
    (2, 12, 12, 5, 32, 3, 3, 1, 1, "SAME"),          # mode 2: C = 5
    (2, 12, 12, 6, 1, 3, 3, 1, 1, "SAME"),           # mode 2: C = 6; K = 1 on the scalar-B tile
    (2, 12, 12, 32, 5, 3, 3, 1, 1, "SAME"),          # scalar-B tile, K = 5, mode 0
    (2, 14, 14, 16, 7, 3, 3, 1, 1, "SAME"),          # scalar-B tile, K = 7, mode 4
    (2, 68, 68, 40, 5, 5, 5, 1, 1, "VALID"),         # NARROW <5, true>, 5x5, C / 4 even (LDS pitch C + 4); WGD: 1000 pairs in 250 quads
    (2, 66, 70, 12, 8, 3, 3, 1, 2, "SAME"),          # NARROW <8, false> K = 8, C / 4 odd (pitch C), dilation 2, ragged 8x32 patches
    (2, 64, 64, 8, 16, 3, 3, 1, 3, "SAME"),          # NARROW <16, true>, dilation 3
    (2, 64, 64, 16, 9, 3, 3, 1, 1, "SAME"),          # NARROW <16, false> K = 9: R S C K = 1296
    (2, 64, 64, 16, 16, 3, 3, 1, 2, "SAME"),         # R S C K = 2304 exactly, dilation 2 (so not N16): NARROW <16, true>
    (2, 64, 64, 20, 13, 3, 3, 1, 1, "SAME"),         # R S C K = 2340: one step over -> IGEMM (scalar-B tile, K = 13)
    (1, 136, 136, 512, 64, 3, 3, 1, 1, "SAME"),      # data gradient: 580 tiles of 128x128, split 2 (the nearly empty last round of choose_split)
]

# strided layers: the data gradient by stride phases, and the zero-upsampled fallback
STRIDED = [
    (2, 16, 16, 64, 64, 3, 3, 2, 1, "SAME"),         # phases in one launch, 32 tiles: conv_dgrad_phases_kernel<128, 32, 4, 1>
    (4, 96, 96, 64, 64, 3, 3, 2, 1, "SAME"),         # 288 phase tiles: conv_dgrad_phases_kernel<128, 64, 2, 2>
    (2, 15, 13, 32, 32, 3, 3, 2, 1, "SAME"),         # odd extents: the four phase grids differ in size
    (2, 16, 1, 32, 32, 3, 3, 2, 1, "SAME"),          # a one-pixel-wide map: the phases of odd columns are empty
    (2, 9, 9, 32, 64, 3, 3, 2, 1, "VALID"),          # VALID, 4x4 outputs (every input row is read: (OH - 1) 2 + 3 = 9); 64 filters: 2 channel groups of dy
    (1, 14, 14, 32, 64, 5, 5, 3, 1, "SAME"),         # stride 3, 5x5: sub-filters 2x2, 2x1, 1x2, 1x1
    (2, 16, 16, 64, 64, 5, 5, 4, 1, "SAME"),         # stride 4, 16 phases, sub-filters 2x2 .. 1x1
    (2, 17, 19, 32, 32, 5, 5, 2, 1, "SAME"),         # stride 2, 5x5: sub-filters 3x3, 3x2, 2x3, 2x2 in one launch
    (2, 10, 10, 20, 24, 3, 3, 2, 1, "SAME"),         # K % 32 != 0: one phase at a time on conv_fwd_kernel (mode 1: 24 channels of dy), no split
    (2, 12, 14, 16, 64, 5, 5, 2, 1, "SAME"),         # C < 32: one phase at a time on the taps kernels 3x3 (2 splits + scatter), 3x2, 2x3, 2x2
    (2, 16, 16, 16, 272, 5, 5, 2, 1, "SAME"),        # one phase at a time, split 9 + split_sum::serial_kernel<Scatter> (split phases are its only reach)
    (2, 12, 12, 16, 64, 6, 6, 3, 1, "SAME"),         # stride 3, 6x6: every sub-filter 2x2; one at a time
    (8, 130, 130, 32, 32, 3, 3, 2, 1, "SAME"),       # more than 512 phase tiles: one at a time, taps 2x2, 2x1, 1x2, 1x1 un-split
    (2, 16, 16, 64, 32, 3, 3, 2, 1, "SYMMETRIC"),    # SYMMETRIC strided: phases over the mirror-padded image, then sympad_bwd
    (2, 8, 8, 32, 32, 1, 1, 2, 1, "SAME"),           # filter smaller than the stride: zero-upsampled fallback (KIND 2)
    (2, 16, 16, 32, 32, 3, 3, 2, 2, "SAME"),         # stride 2 with dilation 2: fallback
    (2, 20, 20, 20, 32, 5, 5, 5, 1, "SAME"),         # stride 5: fallback over 32 channels of dy (mode 0), 20 outputs, 3 splits
    (2, 20, 20, 32, 20, 5, 5, 5, 1, "VALID"),        # stride 5: fallback with 20 channels of dy: KIND 2 never takes mode 4 -> mode 1
]

# filter gradients
WGRAD = [
    (2, 33, 45, 64, 96, 3, 3, 1, 1, "SAME"),         # ring kernel <128, 128, ..., 2>, ragged rows and tiles, K not a tile multiple
    (1, 40, 36, 32, 64, 3, 3, 1, 1, "SAME"),         # ring <128, 64, ..., 2> (fewer than 8192 pixels: not the N16 kernel)
    (1, 36, 40, 64, 32, 3, 3, 1, 1, "VALID"),        # ring <128, 32, ..., 2>, VALID
    (1, 32, 32, 128, 32, 3, 3, 1, 1, "SAME"),        # C % 128 == 0: the uniform-row variant <..., 12>
    (2, 20, 32, 128, 96, 3, 3, 1, 1, "SAME"),        # uniform rows on the 128x128 tile
    (1, 32, 16, 64, 32, 3, 3, 1, 1, "SAME"),         # short rows, OW = 16
    (1, 64, 8, 64, 32, 3, 3, 1, 1, "SAME"),          # OW = 8, 2 splits
    (1, 64, 4, 64, 32, 3, 3, 1, 1, "SAME"),          # OW = 4
    (2, 67, 65, 32, 48, 3, 3, 2, 1, "SAME"),         # strided output with odd OW = 33
    (1, 70, 70, 32, 64, 3, 3, 2, 1, "VALID"),        # strided, VALID, OW = 34; input row / column 69 is read by no output: bit-zero dx there
    (2, 40, 72, 64, 64, 5, 5, 2, 1, "SAME"),         # 5x5 stride 2, OW = 36
    (2, 33, 35, 32, 32, 5, 5, 1, 1, "SAME"),         # 5x5 stride 1
    (3, 37, 41, 64, 64, 3, 3, 1, 1, "SAME"),         # reduction splits with a ragged last split: 143 chunks
    (2, 64, 64, 116, 8, 3, 3, 1, 1, "SAME"),         # 1044 pairs: WGD refused, ring with 32 splits
    (1, 30, 12, 64, 32, 3, 3, 1, 1, "SAME"),         # OW = 12: rows_ok false -> conv_wgrad_kernel mode 1
    (2, 20, 24, 32, 7, 3, 3, 2, 1, "SAME"),          # K % 4 != 0, fewer than 8192 pixels, strided: conv_wgrad_kernel mode 1 on the scalar-B tile
    (2, 40, 36, 32, 6, 3, 3, 1, 1, "SAME"),          # K % 4 != 0, stride 1, OW >= 32: conv_wgrad_kernel mode 3 (the linear walk, one stage in flight)
    (2, 20, 20, 6, 32, 3, 3, 1, 1, "SAME"),          # C % 4 != 0: conv_wgrad_kernel mode 2
    (2, 64, 64, 32, 32, 3, 3, 1, 1, "SAME"),         # wgrad_n16_kernel<32>, K = 32
    (2, 64, 64, 16, 64, 3, 3, 1, 1, "SAME"),         # wgrad_n16_kernel<16>, K = 64: four filter groups
    (460, 1, 32, 32, 64, 3, 3, 1, 1, "SAME"),        # 460 tiles, 455 blocks: the 32 MB cap in force (some blocks walk two tiles)
    (1300, 1, 32, 16, 16, 3, 3, 1, 1, "SAME"),       # 1300 tiles on 1024 blocks
    (1100, 1, 32, 3, 16, 3, 3, 1, 1, "SAME"),        # wgrad_c3n16_kernel with 1100 tiles on 1024 blocks
    (2, 64, 64, 128, 8, 2, 2, 1, 1, "SAME"),         # WGD: 512 pairs, C % 4 == 0, K = 8: wgrad_direct4_kernel<8, 1>
    (2, 64, 64, 84, 5, 3, 3, 1, 1, "SAME"),          # 756 pairs, K = 5: wgrad_direct4_kernel<5, 1>
    (2, 64, 64, 3, 16, 3, 3, 1, 2, "SAME"),          # 27 pairs, 9 pixel groups: wgrad_direct_kernel<16, 1, true, false>, dilation 2
    (2, 64, 64, 12, 12, 3, 3, 1, 1, "SAME"),         # 108 pairs, 2 groups, K = 12: <16, 1, false, false>
    (2, 64, 64, 20, 12, 3, 3, 1, 1, "SAME"),         # 180 pairs: one group <16, 1, false, true>
    (2, 128, 128, 40, 16, 3, 3, 2, 1, "SAME"),       # 360 pairs, K = 16 > 8: ppt = 2, stride 2
    (2, 64, 64, 72, 16, 3, 3, 1, 2, "SAME"),         # 648 pairs: ppt = 3, dilation 2
    (2, 64, 64, 100, 12, 3, 3, 1, 1, "SAME"),        # 900 pairs, K = 12 > 8: ppt = 4 <16, 4, false, true>
    (2, 64, 64, 5, 7, 3, 3, 1, 1, "SAME"),           # 45 pairs, 5 groups, K = 7: <8, 1, false, false>, C % 4 != 0
    (2, 128, 128, 5, 16, 3, 3, 2, 1, "SAME"),        # stride 2 (the mask critic's first layer): <16, 1, true, false>
    (1, 80, 104, 8, 5, 3, 3, 1, 1, "SAME"),          # WGD, 65 = 4 x 16 + 1 partials of 360 = 5 x 64 + 40 values: sliced_kernel<1> with ragged slices AND a ragged last workgroup
]

# anchors too large for the GPU file's float64 oracle: routes and counts only
HOST_ONLY = [
    (4, 176, 176, 32, 64, 3, 3, 1, 1, "SAME"),       # N16_WGRAD, 455 blocks for 528 tiles of 8x32: the 32 MB cap
    (5, 256, 256, 16, 16, 3, 3, 1, 1, "SAME"),       # 1024 blocks for 1280 tiles
    (2, 16, 16, 512, 64, 5, 5, 4, 1, "SAME"),        # forward split 32 (the cap of a handful of tiles)
]
# one layer per forward tile class with an un-split reduction, for the statistics / fused-BN epilogues: (case, symbol of its forward under the
# fused BN — a NARROW layer takes the implicit GEMM there)
EPILOGUE = [
    ((2, 112, 112, 32, 256, 1, 1, 1, 1, "SAME"), "conv_fwd_kernel<128, 128, 2, 2, 0, 0, true>"),      # 128x128, 392 tiles
    ((2, 68, 68, 64, 96, 3, 3, 1, 1, "VALID"), "conv_taps3_kernel<128, 64, 2, 2, 0, 3, 3>"),          # 128x64
    ((2, 20, 24, 32, 32, 3, 3, 1, 1, "SAME"), "conv_taps_kernel<128, 32, 4, 1, 0, 3, 3>"),            # 128x32, ragged last tile (M = 960)
    ((2, 14, 14, 16, 7, 3, 3, 1, 1, "SAME"), "conv_fwd_kernel<128, 32, 4, 1, 4, 0, false>"),          # scalar-B
    ((2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"), "conv_n16_kernel<16, 0>"),                              # N16 (fused BN only: no statistics)
    ((2, 66, 70, 12, 8, 3, 3, 1, 2, "SAME"), "conv_fwd_kernel<128, 32, 4, 1, 1, 0, true>"),           # a NARROW layer: the fused BN takes IGEMM
]
ALL = FWD + STRIDED + WGRAD + HOST_ONLY + [c for c, _ in EPILOGUE if c not in FWD]


def case_id(c):
    return "x".join(str(v) for v in c)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
class Geom(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def cdiv(a, b):
    return -(-a // b)


def al256(b):
    return (b + 255) & ~255


def geom_of(case):
    """kernels.conv_geom restated"""
    N, H, W, C, K, R, S, st, dil, padding = case

    def axis(n, k):
        eff = (k - 1) * dil + 1
        if padding == "SAME":
            o = cdiv(n, st)
            return o, max((o - 1) * st + eff - n, 0) // 2
        if padding == "SYMMETRIC":
            return (n + 2 * (k // 2) - eff) // st + 1, k // 2
        return (n - eff) // st + 1, 0
    (OH, pt), (OW, pl) = axis(H, R), axis(W, S)
    return Geom(N=N, H=H, W=W, C=C, K=K, R=R, S=S, stride=st, dil=dil, pad_t=pt, pad_l=pl, OH=OH, OW=OW, sym=padding == "SYMMETRIC")


def choose_tile(M, K):
    """0 / 1 / 2: 128 x {128, 64, 32}; 3: the scalar-B variant of the narrow tile"""
    if K & 3:
        return 3
    mt = cdiv(M, 128)
    if K > 64 and mt * cdiv(K, 128) >= 384:
        return 0
    if K > 32 and (mt * cdiv(K, 64) >= 384 or K > 64):
        return 1
    return 2


TILE_BN = {0: 128, 1: 64, 2: 32, 3: 32}
TILE_ARGS = {0: "128, 128, 2, 2", 1: "128, 64, 2, 2", 2: "128, 32, 4, 1", 3: "128, 32, 4, 1"}


def choose_split(M, K, Kred, tile):
    nblk = cdiv(M, 128) * cdiv(K, TILE_BN[tile])
    nch = cdiv(Kred, BK)
    rounds = nblk / 512.0
    ns = 1
    if rounds <= 0.4:
        ns = 512 // nblk
    elif 1.0 < rounds < 3.0 and math.ceil(rounds) - rounds > 0.3:
        best = 0.0
        for n in range(1, 9):
            r = rounds * n
            score = r / math.ceil(r) - 0.01 * n
            if score > best + 1e-9:
                best, ns = score, n
    ns = min(ns, 32 if nblk <= 64 else 8, nch // 8)
    return max(ns, 1)


def fwd_split(g):
    if g.sym:
        return 1
    M = g.N * g.OH * g.OW
    tile = choose_tile(M, g.K)
    if cdiv(M, 128) * cdiv(g.K, TILE_BN[tile]) > 128:
        return 1
    return choose_split(M, g.K, g.R * g.S * g.C, tile)


def taps_shape(kind, R, S):
    if R == 3 and S == 3:
        return True
    if kind == 0:
        return R == 5 and S == 5
    if kind == 1:
        return 1 <= R <= 3 and 1 <= S <= 3 and (R, S) not in ((3, 1), (1, 3))
    return False


def igemm_launch(M, K, C, R, S, zero, kind, split, drop=False, scatter=False):
    """launch_fwd + launch_fwd_tile for a convolution with M output pixels, K filters over C channels (kind 1 / 2: a convolution of dy, so
    C = the layer's filters and K = its channels), split: did the caller bring room for partials -> dict(sym, ns, per, total, reducer):
    ns splits of `per` units out of `total` (units: whole channel groups on the taps kernels, 32-deep chunks elsewhere)"""
    tile = choose_tile(M, K)
    ns = choose_split(M, K, R * S * C, tile) if split else 1
    bn, vecb = TILE_BN[tile], tile != 3
    taps = vecb and kind != 2 and zero and taps_shape(kind, R, S) and C % 32 == 0
    if taps:
        total = C // BK
        per = cdiv(total, ns)
        ns = cdiv(total, per)
        pairs_ok = (R * S) % 2 == 0 or all(min(total - z * per, per) % 2 == 0 for z in range(ns))
        t3 = bn <= 64 and R * S <= 9 and pairs_ok
        sym = "%s<%s, %d, %d, %d>" % ("conv_taps3_kernel" if t3 else "conv_taps_kernel", TILE_ARGS[tile], kind, R, S)
    else:
        total = cdiv(R * S * C, BK)
        per = cdiv(total, ns)
        ns = cdiv(total, per)
        mode = 0 if C % 32 == 0 else (1 if C % 4 == 0 else 2)
        kmode = mode if mode != 1 else (4 if kind != 2 and zero and C >= 16 else 1)
        sym = "conv_fwd_kernel<%s, %d, %d, %s>" % (TILE_ARGS[tile], kmode, kind, "true" if vecb else "false")
    reducer = None
    if ns > 1:
        reducer = "split_sum::serial_kernel<Drop>" if drop else ("split_sum::serial_kernel<Scatter>" if scatter else "split_sum::serial_kernel<Plain>")
    return dict(sym=sym, ns=ns, per=per, total=total, reducer=reducer, taps=taps, tile=tile)


def n16_geom_ok(g):
    if g.K != 16 or g.C not in (16, 32, 3) or (g.R, g.S) != (3, 3) or g.stride != 1 or g.dil != 1:
        return False
    if g.sym or g.pad_t > 1 or g.pad_l > 1:
        return False
    if g.OH != g.H + 2 * g.pad_t - 2 or g.OW != g.W + 2 * g.pad_l - 2:
        return False
    return g.N * g.OH * g.OW >= 8192 and g.N <= 65535


def n16_launch(g, kind):
    tiles_w, tiles_h = cdiv(g.OW, 32), cdiv(g.OH, 8)
    tpw = 1
    while tpw < tiles_w and cdiv(tiles_w, tpw) * tiles_h * g.N > 4096:
        tpw *= 2
    return dict(sym="%s<%d, %d>" % ("conv_c3n16_kernel" if g.C == 3 else "conv_n16_kernel", g.C, kind), tpw=tpw, tiles=tiles_w * tiles_h * g.N)


def n16_wgrad_ok(g):
    if n16_geom_ok(g):
        return True
    if g.K not in (32, 64) or g.C not in (16, 32) or (g.R, g.S) != (3, 3) or g.stride != 1 or g.dil != 1:
        return False
    if g.sym or g.pad_t > 1 or g.pad_l > 1:
        return False
    if g.OH != g.H + 2 * g.pad_t - 2 or g.OW != g.W + 2 * g.pad_l - 2:
        return False
    P = g.N * g.OH * g.OW
    if g.K == 64 and P >= 1 << 19:
        return False
    return P >= 8192


def n16_wgrad_blocks(g):
    ntiles = cdiv(g.OW, 32) * cdiv(g.OH, 8) * g.N
    return max(min(ntiles, 1024, (8 << 20) // (9 * g.C * g.K)), 1)


NARROW_MAX_N = 65536      # the images are the grid's z extent (see test_narrow_route_refuses_more_images_than_a_grid_holds)


def narrow_fwd_ok(g):
    """-> None or (PH, PW, CP): the LDS patch and its pixel pitch"""
    if g.K > 16 or g.stride != 1 or g.sym or g.C & 3 or g.C < 8:
        return None
    if g.N * g.OH * g.OW < 8192 or g.N > NARROW_MAX_N:
        return None
    if g.K > 8 and g.R * g.S * g.C * g.K > 2304:
        return None
    PH, PW = 8 + (g.R - 1) * g.dil, 32 + (g.S - 1) * g.dil
    CP = g.C if (g.C >> 2) & 1 else g.C + 4
    if PH * PW * CP * 4 > 150 * 1024:
        return None
    return PH, PW, CP


def narrow_symbol(K):
    """launch_narrow's instance"""
    kk, exact = (5, True) if K == 5 else ((16, True) if K == 16 else ((8, False) if K <= 8 else (16, False)))
    return "conv_fwd_narrow_kernel<%d, %s>" % (kk, "true" if exact else "false")


def wgd_plan(g):
    """-> None or dict(nblk, ppb, G, ppt, ws_bytes)"""
    P, npairs = g.N * g.OH * g.OW, g.R * g.S * g.C
    if g.K > 16 or g.sym or npairs > 1024 or P < 8192:
        return None
    ppt = 1 if npairs <= 256 else cdiv(npairs, 256)
    G = min(256 // npairs, 16) if ppt == 1 else 1
    ppb = cdiv(P, min(P // 128, 2048))
    nblk = cdiv(P, ppb)
    return dict(nblk=nblk, ppb=ppb, G=G, ppt=ppt, ws_bytes=nblk * npairs * g.K * 4)


def wgd_variant(g, pl):
    """launch_wgd's instance: the profiler names the whole family "wgrad_direct_kernel<KK> (all variants)\""""
    kk, exact = (16, True) if g.K == 16 else ((5, True) if g.K == 5 else ((8, False) if g.K <= 8 else (16, False)))
    ex = "true" if exact else "false"
    nquads = g.R * g.S * g.C // 4
    if g.C % 4 == 0 and 128 <= nquads <= 512 and kk <= 8:
        return kk, "wgrad_direct4_kernel<%d, %d, %s>" % (kk, 1 if nquads <= 256 else 2, ex)
    if pl["ppt"] == 1 and pl["G"] > 1:
        return kk, "wgrad_direct_kernel<%d, 1, %s, false>" % (kk, ex)
    return kk, "wgrad_direct_kernel<%d, %d, %s, true>" % (kk, min(pl["ppt"], 4), ex)


def plan_phases(g):
    """-> list of dict(T, U, h0, w0, pad_t, pad_l, I, J); empty: not applicable (the zero-upsampled kernel)"""
    st = g.stride
    if st < 2 or st > 4 or g.dil != 1 or g.R < st or g.S < st:
        return []
    Ho, Wo = (g.H + 2 * g.pad_t, g.W + 2 * g.pad_l) if g.sym else (g.H, g.W)
    fpt, fpl = (0, 0) if g.sym else (g.pad_t, g.pad_l)
    out = []
    for a in range(st):
        for b in range(st):
            T, U = cdiv(g.R - a, st), cdiv(g.S - b, st)
            h0, w0 = (a - fpt) % st, (b - fpl) % st
            pt, pl = T - 1 - (h0 + fpt - a) // st, U - 1 - (w0 + fpl - b) // st
            if pt < 0 or pl < 0:
                return []
            out.append(dict(T=T, U=U, h0=h0, w0=w0, pad_t=pt, pad_l=pl, I=(Ho - 1 - h0) // st + 1 if h0 < Ho else 0,
                            J=(Wo - 1 - w0) // st + 1 if w0 < Wo else 0))
    return out


def phase_group_tiles(g, ph, bn):
    return sum(cdiv(g.N * p["I"] * p["J"], 128) * cdiv(g.C, bn) for p in ph if p["I"] > 0 and p["J"] > 0)


def phases_in_one_launch(g, ph):
    if len(ph) < 2 or len(ph) > 16 or g.K % 32 or g.C % 4 or g.C < 32:
        return False
    return phase_group_tiles(g, ph, 64) <= 512


def dgrad_as_conv(g):
    OH, OW = (g.H + 2 * g.pad_t, g.W + 2 * g.pad_l) if g.sym else (g.H, g.W)
    return Geom(N=g.N, H=g.OH, W=g.OW, C=g.K, K=g.C, R=g.R, S=g.S, OH=OH, OW=OW, stride=1, dil=g.dil,
                pad_t=g.dil * (g.R - 1) - (0 if g.sym else g.pad_t), pad_l=g.dil * (g.S - 1) - (0 if g.sym else g.pad_l), sym=False)


def wgrad_plan_split(nblk, nchunks):
    max_split = max(nchunks // 8, 1)
    lo = cdiv(512, nblk)
    if lo >= max_split:
        return max_split
    hi = min(lo * 3 + 2, max_split)
    best, best_score = lo, -1.0
    for ns in range(lo, hi + 1):
        rounds = nblk * ns / 512.0
        score = rounds / math.ceil(rounds) - 0.02 * rounds
        if score > best_score:
            best_score, best = score, ns
    return best


def ring_tile(K):
    return 3 if K & 3 else (0 if K > 64 else (1 if K > 32 else 2))


def ring_launch(g, ws_bytes):
    """launch_wgrad_tile with a workspace of ws_bytes -> dict(sym, ns, per, total, planned): the ring kernel takes as many of the planned
    splits as fit, a single partial is no split"""
    tile = ring_tile(g.K)
    bn, vecb = TILE_BN[tile], tile != 3
    M, Kred = g.N * g.OH * g.OW, g.R * g.S * g.C
    nblk, total = cdiv(Kred, 128) * cdiv(g.K, bn), cdiv(M, BK)
    planned = ns = wgrad_plan_split(nblk, total)
    nout = Kred * g.K
    if ns > 1 and ws_bytes < ns * nout * 4:
        ns = ws_bytes // (nout * 4)
        if ns < 2:
            ns = 1
    per = cdiv(total, ns)
    ns = cdiv(total, per)
    OHW = g.OH * g.OW
    rows_ok = g.OW >= BK or (BK % g.OW == 0 and g.OH > BK // g.OW and OHW % BK == 0)
    lin_any = (not g.sym) and g.C % 4 == 0 and rows_ok
    lin = lin_any and g.stride == 1 and g.OW >= BK
    if lin_any and vecb:
        sym = "conv_wgrad_ring_kernel<%s, %d>" % (TILE_ARGS[tile], 12 if g.C % 128 == 0 else 2)
    else:
        sym = "conv_wgrad_kernel<%s, %d, %s>" % (TILE_ARGS[tile], 3 if lin else (1 if g.C % 4 == 0 else 2), "true" if vecb else "false")
    return dict(sym=sym, ns=ns, per=per, total=total, planned=planned, reducer="split_sum::serial_kernel<Plain>" if ns > 1 else None)


def plan(case, kind, drop=False):
    """the whole plan of one pass (0 forward, 1 data gradient, 2 filter gradient) with the full workspace of the query:
    dict(route, symbols [sorted, as the profiler records them], nsplit [the count the workspace query encodes], ws_bytes [the query],
    launches [igemm_launch / ring_launch dicts], tags [variant names: symbols + what the profiler does not tell apart])"""
    g = geom_of(case)
    M = g.N * g.OH * g.OW
    nout = g.R * g.S * g.C * g.K
    if kind == 0:
        ns = fwd_split(g)
        ws = ns * M * g.K * 4 if ns > 1 else 0
        if n16_geom_ok(g):
            L = n16_launch(g, 0)
            return dict(route=N16, symbols=[L["sym"]], nsplit=ns, ws_bytes=ws, launches=[L], tags={L["sym"]} | ({"n16 tpw>1"} if L["tpw"] > 1 else set()))
        if narrow_fwd_ok(g):
            s = narrow_symbol(g.K)
            return dict(route=NARROW, symbols=[s], nsplit=ns, ws_bytes=ws, launches=[], tags={s, "narrow pitch C%s" % ("" if (g.C >> 2) & 1 else "+4")})
        L = igemm_launch(M, g.K, g.C, g.R, g.S, not g.sym, 0, ns > 1, drop=drop)
        return dict(route=IGEMM, symbols=[L["sym"]], nsplit=ns, ws_bytes=ws, launches=[L], tags={L["sym"]} | ({L["reducer"]} if L["reducer"] else set()))
    if kind == 1:
        d = dgrad_as_conv(g)
        outb = d.N * d.OH * d.OW * d.K * 4
        b = al256(nout * 4) + (al256(outb) if g.sym else 0)
        ph = plan_phases(g)
        if ph:
            mx, ns_q = 0, 1
            for p in ph:
                Mp = g.N * p["I"] * p["J"]
                if Mp == 0:
                    continue
                ns = choose_split(Mp, g.C, p["T"] * p["U"] * g.K, choose_tile(Mp, g.C))
                if ns > 1 and ns * Mp * g.C * 4 > mx:
                    mx, ns_q = ns * Mp * g.C * 4, ns
            if phases_in_one_launch(g, ph):
                narrow = phase_group_tiles(g, ph, 64) < 256
                s = "conv_dgrad_phases_kernel<128, %d, %d, %d>" % ((32, 4, 1) if narrow else (64, 2, 2))
                return dict(route=PHASES, symbols=[s], nsplit=ns_q, ws_bytes=b + mx, launches=[], tags={s}, phases=ph, mx=mx)
            Ls = [igemm_launch(g.N * p["I"] * p["J"], g.C, g.K, p["T"], p["U"], True, 1, mx > 0, scatter=True) for p in ph if p["I"] * p["J"] > 0]
            tags = {L["sym"] for L in Ls} | {L["reducer"] for L in Ls if L["reducer"]} | {"phases one at a time"}
            return dict(route=PHASES, symbols=sorted({L["sym"] for L in Ls}), nsplit=ns_q, ws_bytes=b + mx, launches=Ls, tags=tags, phases=ph, mx=mx)
        Md = d.N * d.OH * d.OW
        ns = choose_split(Md, g.C, g.R * g.S * g.K, choose_tile(Md, g.C))
        ws = b + (ns * outb if ns > 1 else 0)
        if not g.sym and n16_geom_ok(d):
            L = n16_launch(d, 1)
            return dict(route=N16, symbols=[L["sym"]], nsplit=ns, ws_bytes=ws, launches=[L], tags={L["sym"]} | ({"n16 tpw>1"} if L["tpw"] > 1 else set()))
        if g.stride == 1 and narrow_fwd_ok(d):
            s = narrow_symbol(d.K)
            return dict(route=NARROW, symbols=[s], nsplit=ns, ws_bytes=ws, launches=[], tags={s, "narrow pitch C%s" % ("" if (d.C >> 2) & 1 else "+4")})
        L = igemm_launch(Md, g.C, g.K, g.R, g.S, True, 2 if g.stride > 1 else 1, ns > 1)
        return dict(route=IGEMM, symbols=[L["sym"]], nsplit=ns, ws_bytes=ws, launches=[L], tags={L["sym"]} | ({L["reducer"]} if L["reducer"] else set()))
    pl = wgd_plan(g)
    if n16_wgrad_ok(g):
        nb = n16_wgrad_blocks(g)
        s = "%s<%d>" % ("wgrad_c3n16_kernel" if g.C == 3 else "wgrad_n16_kernel", g.C)
        ntiles = cdiv(g.OW, 32) * cdiv(g.OH, 8) * g.N
        tags = {s, "%s K=%d" % (s, g.K)} | ({"n16 wgrad several tiles per block"} if ntiles > nb else set())
        return dict(route=N16_WGRAD, symbols=[s], nsplit=nb, ws_bytes=nb * nout * 4, launches=[], tags=tags)
    tile = ring_tile(g.K)
    ns_ring = wgrad_plan_split(cdiv(g.R * g.S * g.C, 128) * cdiv(g.K, TILE_BN[tile]), cdiv(M, BK))
    mfma_ws = ns_ring * nout * 4 if ns_ring > 1 else 0
    if pl:
        kk, var = wgd_variant(g, pl)
        tags = {var} | ({"wgd stride 2"} if g.stride == 2 else set()) | ({"wgd dilation 2"} if g.dil == 2 else set())
        return dict(route=WGD, symbols=["wgrad_direct_kernel<%d> (all variants)" % kk], nsplit=pl["nblk"], ws_bytes=max(pl["ws_bytes"], mfma_ws),
                    launches=[], tags=tags, wgd=pl)
    L = ring_launch(g, mfma_ws)
    return dict(route=RING, symbols=[L["sym"]], nsplit=ns_ring, ws_bytes=mfma_ws, launches=[L], tags={L["sym"]} | ({"ring split"} if L["ns"] > 1 else set()))


def fp32_expected(case, kind):
    """(route, symbols, nsplit) of the pass with the Winograd and split-bf16 switches at 0 and the query's workspace supplied"""
    p = plan(case, kind)
    return p["route"], p["symbols"], p["nsplit"]


# ---- against the library ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32_routes(built):
    """wino_mode(0), wino_wgrad_mode(0), x3_direct(0), x3_strided(0), x3_wgrad(0); restores what was in force"""
    K = pkg("kernels")
    prev = (K.wino_mode(0), K.wino_wgrad_mode(0), K.x3_direct(0), K.x3_strided(0), K.x3_wgrad(0))
    yield K
    K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.x3_direct(prev[2]); K.x3_strided(prev[3]); K.x3_wgrad(prev[4])


def lib_geom(K, case):
    N, H, W, C, Kf, R, S, st, dil, padding = case
    return K.conv_geom((N, H, W, C), (R, S, C, Kf), st, dil, padding)


def test_restated_geometry_is_conv_geom(fp32_routes):
    K = fp32_routes
    for case in ALL:
        g, r = lib_geom(K, case), geom_of(case)
        assert (g.OH, g.OW, g.pad_t, g.pad_l, g.pad_mode != 0) == (r.OH, r.OW, r.pad_t, r.pad_l, r.sym), case


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_restated_routes_against_the_library_for_every_row(fp32_routes, kind):
    K = fp32_routes
    for case in ALL:
        assert K.conv_route(lib_geom(K, case), kind) == fp32_expected(case, kind)[0], (case, kind)


def query_splits(lib, K, case, kind):
    """the reduction-split count (or per-workgroup partial count) read off the workspace query of the library, by its documented layout"""
    g, r = lib_geom(K, case), geom_of(case)
    M, nout = r.N * r.OH * r.OW, r.R * r.S * r.C * r.K
    if kind == 0:
        b, per = int(lib.pnp_conv2d_fwd_workspace_bytes(ctypes.byref(g))), M * r.K * 4
    elif kind == 2:
        b, per = int(lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g))), nout * 4
    else:
        d = dgrad_as_conv(r)
        outb = d.N * d.OH * d.OW * d.K * 4
        b = int(lib.pnp_conv2d_dgrad_workspace_bytes(ctypes.byref(g))) - al256(nout * 4) - (al256(outb) if r.sym else 0)
        p = plan(case, 1)
        per = outb
        if "phases" in p:          # the largest phase's ns * Mp * C * 4.  The query does not say WHICH phase: the divisor is picked with the
            # restated count, so for phase layers this is no independent reading — the independent check is the byte equality in the caller
            sizes = [r.N * q["I"] * q["J"] * r.C * 4 for q in p["phases"] if q["I"] * q["J"] > 0]
            per = max(s for s in sizes if b % s == 0 and b // s == p["nsplit"]) if b else max(sizes)
    assert b >= 0 and b % per == 0, (case, kind, b, per)
    return b // per if b else 1, b


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_split_counts_read_off_the_workspace_queries(fp32_routes, kind):
    K, lib = fp32_routes, pkg("_lib").load()
    for case in ALL:
        p = plan(case, kind)
        ns, b = query_splits(lib, K, case, kind)
        r = geom_of(case)
        full = b + (al256(r.R * r.S * r.C * r.K * 4) + (al256(r.N * (r.H + 2 * r.pad_t) * (r.W + 2 * r.pad_l) * r.C * 4) if r.sym else 0) if kind == 1 else 0)
        assert full == p["ws_bytes"], (case, kind, full, p["ws_bytes"])
        if kind == 2 and p["route"] == WGD and p["wgd"]["ws_bytes"] < p["ws_bytes"]:
            continue               # (the query is the ring fall-back's, larger than the vector-ALU kernel's slabs: no block count to read)
        assert ns == p["nsplit"], (case, kind, ns, p["nsplit"])


def _p(case, kind):
    assert case in ALL, case
    return plan(case, kind)


def test_restated_planner_anchors(fp32_routes):
    """what the tables' comments claim, spelled out, so that the restatement and the library cannot drift together unnoticed"""
    routes = lambda c: tuple(fp32_expected(c, k)[0] for k in (0, 1, 2))
    assert routes((2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME")) == (N16, N16, N16_WGRAD) and _p((2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"), 2)["nsplit"] == 32
    c = (1, 92, 93, 32, 16, 3, 3, 1, 1, "VALID")
    g = geom_of(c)
    assert g.N * g.OH * g.OW == 8190 and routes(c) == (IGEMM, IGEMM, RING)
    c = (2, 64, 64, 16, 3, 3, 3, 1, 1, "SAME")
    assert routes(c) == (NARROW, N16, WGD) and fp32_expected(c, 1)[1] == ["conv_c3n16_kernel<3, 1>"]
    assert routes((2, 64, 64, 3, 16, 3, 3, 1, 1, "SAME")) == (N16, NARROW, N16_WGRAD)
    assert routes((65535, 1, 1, 16, 16, 3, 3, 1, 1, "SAME")) == (N16, N16, N16_WGRAD)
    assert routes((65536, 1, 1, 16, 16, 3, 3, 1, 1, "SAME")) == (NARROW, NARROW, WGD)
    for c, ns in (((1, 8, 8, 160, 64, 3, 3, 1, 1, "SAME"), 5), ((1, 8, 8, 224, 32, 3, 3, 1, 1, "SAME"), 7), ((2, 4, 4, 512, 128, 3, 3, 1, 1, "SAME"), 18),
                  ((2, 16, 16, 512, 64, 5, 5, 4, 1, "SAME"), 32), ((2, 64, 64, 112, 7, 3, 3, 1, 1, "SAME"), 4)):
        assert fp32_expected(c, 0)[0] == IGEMM and fp32_expected(c, 0)[2] == ns, (c, fp32_expected(c, 0))
    assert "false>" in fp32_expected((2, 64, 64, 112, 7, 3, 3, 1, 1, "SAME"), 0)[1][0]                 # the scalar-B tile
    L = _p((2, 4, 4, 512, 128, 3, 3, 1, 1, "SAME"), 0)["launches"][0]
    assert (L["ns"], L["per"], L["total"]) == (16, 1, 16)                                             # 18 planned, 16 channel groups
    c = (1, 136, 136, 512, 64, 3, 3, 1, 1, "SAME")
    L = _p(c, 1)["launches"][0]
    assert cdiv(136 * 136, 128) * cdiv(512, 128) == 580 and L["tile"] == 0 and fp32_expected(c, 1)[2] == 2 and L["ns"] == 2
    c = (2, 16, 16, 16, 272, 5, 5, 2, 1, "SAME")
    p = _p(c, 1)
    assert p["route"] == PHASES and p["nsplit"] == 9 and "split_sum::serial_kernel<Scatter>" in p["tags"] and "phases one at a time" in p["tags"]
    scat = [s for s in (STRIDED + FWD + WGRAD) if "split_sum::serial_kernel<Scatter>" in plan(s, 1)["tags"]]      # only split phases reach it
    assert c in scat and all("phases one at a time" in plan(s, 1)["tags"] for s in scat)
    g = geom_of((4, 176, 176, 32, 64, 3, 3, 1, 1, "SAME"))
    assert cdiv(g.OW, 32) * cdiv(g.OH, 8) * g.N == 528 and fp32_expected((4, 176, 176, 32, 64, 3, 3, 1, 1, "SAME"), 2)[::2] == (N16_WGRAD, 455)
    assert fp32_expected((5, 256, 256, 16, 16, 3, 3, 1, 1, "SAME"), 2)[::2] == (N16_WGRAD, 1024)
    c = (2, 64, 64, 116, 8, 3, 3, 1, 1, "SAME")
    assert 9 * 116 == 1044 and fp32_expected(c, 2)[::2] == (RING, 32)
    c = (1, 80, 104, 8, 5, 3, 3, 1, 1, "SAME")          # sliced_kernel<1>: 65 partials = 4 per slice + 1, 360 values = 5 workgroups of 64 + 40
    assert fp32_expected(c, 2)[::2] == (WGD, 65) and 9 * 8 * 5 == 360 and _p(c, 2)["wgd"]["ws_bytes"] == _p(c, 2)["ws_bytes"] == 65 * 360 * 4
    assert fp32_expected((1, 64, 8, 64, 32, 3, 3, 1, 1, "SAME"), 2) == (RING, ["conv_wgrad_ring_kernel<128, 32, 4, 1, 2>"], 2)
    assert fp32_expected((1, 30, 12, 64, 32, 3, 3, 1, 1, "SAME"), 2)[:2] == (RING, ["conv_wgrad_kernel<128, 32, 4, 1, 1, true>"])
    # ragged last splits: ns * per != total
    for c, kind in (((1, 110, 128, 160, 32, 3, 3, 1, 1, "SAME"), 0), ((1, 30, 30, 100, 36, 3, 3, 1, 1, "SAME"), 0), ((3, 37, 41, 64, 64, 3, 3, 1, 1, "SAME"), 2)):
        L = _p(c, kind)["launches"][0]
        assert L["ns"] > 1 and L["ns"] * L["per"] != L["total"], (c, kind, L)
    assert _p((1, 110, 128, 160, 32, 3, 3, 1, 1, "SAME"), 0)["launches"][0]["taps"] and not _p((1, 30, 30, 100, 36, 3, 3, 1, 1, "SAME"), 0)["launches"][0]["taps"]
    L = _p((1, 171, 128, 32, 128, 3, 3, 1, 1, "SAME"), 1)["launches"][0]
    assert L["sym"].startswith("conv_taps3_kernel<") and (L["ns"], L["per"]) == (2, 2)
    assert _p((2049, 1, 33, 16, 16, 3, 3, 1, 1, "SAME"), 0)["launches"][0] == dict(sym="conv_n16_kernel<16, 0>", tpw=2, tiles=4098)
    # the R S C K <= 2304 boundary of the 9..16-filter narrow kernel
    assert fp32_expected((2, 64, 64, 16, 16, 3, 3, 1, 2, "SAME"), 0)[:2] == (NARROW, ["conv_fwd_narrow_kernel<16, true>"])
    assert fp32_expected((2, 64, 64, 20, 13, 3, 3, 1, 1, "SAME"), 0)[0] == IGEMM and 9 * 20 * 13 == 2340
    # the N16 filter-gradient block cap and the empty phases
    assert _p((460, 1, 32, 32, 64, 3, 3, 1, 1, "SAME"), 2)["nsplit"] == 455
    assert sum(1 for q in _p((2, 16, 1, 32, 32, 3, 3, 2, 1, "SAME"), 1)["phases"] if q["I"] * q["J"] == 0) == 2
    for c in ((2, 8, 8, 32, 32, 1, 1, 2, 1, "SAME"), (2, 16, 16, 32, 32, 3, 3, 2, 2, "SAME"), (2, 20, 20, 20, 32, 5, 5, 5, 1, "SAME")):
        assert fp32_expected(c, 1)[0] == IGEMM and ", 2, true>" in fp32_expected(c, 1)[1][0], c                   # KIND 2


# every variant the GPU file must see at least once (its last test checks the tags it asserted against this list)
REQUIRED = [
    "conv_taps3_kernel<128, 64, 2, 2, 0, 3, 3>", "conv_taps3_kernel<128, 32, 4, 1, 0, 3, 3>", "conv_taps3_kernel<128, 64, 2, 2, 1, 3, 3>",
    "conv_taps3_kernel<128, 32, 4, 1, 1, 3, 3>", "conv_taps_kernel<128, 128, 2, 2, 0, 3, 3>", "conv_taps_kernel<128, 128, 2, 2, 1, 3, 3>",
    "conv_taps_kernel<128, 32, 4, 1, 0, 3, 3>", "conv_taps_kernel<128, 64, 2, 2, 0, 3, 3>", "conv_taps_kernel<128, 64, 2, 2, 0, 5, 5>",
] + ["conv_taps%s_kernel<128, 32, 4, 1, 1, %d, %d>" % (t, r, s) for (t, r, s) in (("", 1, 1), ("3", 1, 2), ("3", 2, 1), ("3", 2, 2), ("3", 2, 3), ("3", 3, 2))] + [
    "conv_fwd_kernel<128, 64, 2, 2, 0, 0, true>", "conv_fwd_kernel<128, 32, 4, 1, 0, 0, true>", "conv_fwd_kernel<128, 32, 4, 1, 4, 0, true>",
    "conv_fwd_kernel<128, 32, 4, 1, 1, 0, true>", "conv_fwd_kernel<128, 32, 4, 1, 2, 0, true>", "conv_fwd_kernel<128, 32, 4, 1, 2, 0, false>",
    "conv_fwd_kernel<128, 32, 4, 1, 0, 0, false>", "conv_fwd_kernel<128, 32, 4, 1, 4, 0, false>", "conv_fwd_kernel<128, 32, 4, 1, 1, 0, false>",
    "conv_fwd_kernel<128, 32, 4, 1, 0, 2, true>", "conv_fwd_kernel<128, 32, 4, 1, 1, 2, true>",
    "split_sum::serial_kernel<Plain>", "split_sum::serial_kernel<Drop>", "split_sum::serial_kernel<Scatter>", "phases one at a time",
    "conv_n16_kernel<16, 0>", "conv_n16_kernel<16, 1>", "conv_n16_kernel<32, 0>", "conv_n16_kernel<32, 1>", "conv_c3n16_kernel<3, 0>",
    "conv_c3n16_kernel<3, 1>", "n16 tpw>1",
    "conv_fwd_narrow_kernel<5, true>", "conv_fwd_narrow_kernel<16, true>", "conv_fwd_narrow_kernel<8, false>", "conv_fwd_narrow_kernel<16, false>",
    "narrow pitch C", "narrow pitch C+4",
    "conv_dgrad_phases_kernel<128, 32, 4, 1>", "conv_dgrad_phases_kernel<128, 64, 2, 2>",
    "conv_wgrad_ring_kernel<128, 128, 2, 2, 2>", "conv_wgrad_ring_kernel<128, 64, 2, 2, 2>", "conv_wgrad_ring_kernel<128, 32, 4, 1, 2>",
    "conv_wgrad_ring_kernel<128, 32, 4, 1, 12>", "conv_wgrad_ring_kernel<128, 128, 2, 2, 12>", "ring split",
    "conv_wgrad_kernel<128, 32, 4, 1, 1, true>", "conv_wgrad_kernel<128, 128, 2, 2, 1, true>", "conv_wgrad_kernel<128, 32, 4, 1, 1, false>",
    "conv_wgrad_kernel<128, 32, 4, 1, 3, false>", "conv_wgrad_kernel<128, 32, 4, 1, 2, true>",
    "wgrad_n16_kernel<16> K=16", "wgrad_n16_kernel<16> K=32", "wgrad_n16_kernel<16> K=64", "wgrad_n16_kernel<32> K=16", "wgrad_n16_kernel<32> K=32",
    "wgrad_n16_kernel<32> K=64", "wgrad_c3n16_kernel<3>", "n16 wgrad several tiles per block",
    "wgrad_direct4_kernel<8, 1, false>", "wgrad_direct4_kernel<5, 1, true>", "wgrad_direct_kernel<16, 1, true, false>",
    "wgrad_direct_kernel<16, 1, false, false>", "wgrad_direct_kernel<8, 1, false, false>", "wgrad_direct_kernel<16, 1, false, true>",
    "wgrad_direct_kernel<16, 2, true, true>", "wgrad_direct_kernel<16, 3, true, true>", "wgrad_direct_kernel<16, 4, false, true>",
    "wgd stride 2", "wgd dilation 2",
]


def tags_of_tables(drop_cases=()):
    tags = set()
    for case in FWD + STRIDED + WGRAD:
        for kind in (0, 1, 2):
            tags |= plan(case, kind)["tags"]
    for case in drop_cases:
        tags |= plan(case, 0, drop=True)["tags"]
    return tags


# forward cases the GPU file also runs with dropout (keep_prob 0.5): split ones (dropout in the summing kernel) and un-split ones
DROPOUT = [(1, 8, 8, 160, 64, 3, 3, 1, 1, "SAME"), (1, 30, 30, 100, 36, 3, 3, 1, 1, "SAME"), (2, 68, 68, 64, 96, 3, 3, 1, 1, "VALID"),
           (2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"), (2, 66, 70, 12, 8, 3, 3, 1, 2, "SAME")]


def test_the_tables_reach_every_required_variant():
    tags = tags_of_tables(DROPOUT)
    missing = [t for t in REQUIRED if t not in tags]
    assert not missing, missing


def test_epilogue_rows_are_unsplit_and_on_their_tile_class(fp32_routes):
    K = fp32_routes
    for case, symbol in EPILOGUE:
        p, g = plan(case, 0), lib_geom(K, case)
        if p["route"] == NARROW:           # the fused BN is not in the vector-ALU kernel: plan_fwd skips it, and never splits under EP_BN
            r = geom_of(case)
            assert igemm_launch(r.N * r.OH * r.OW, r.K, r.C, r.R, r.S, True, 0, False)["sym"] == symbol and K.conv_stats_parts(g) == 0
        else:
            assert p["symbols"] == [symbol] and p["nsplit"] == 1, case
            assert (K.conv_stats_parts(g) > 0) == (p["route"] == IGEMM), case


def test_direct4_two_quads_per_thread_is_unreachable():
    """wgrad_direct4_kernel<KK, 2, ...> served nquads = R S C / 4 in 257..512, i.e. more than 1024 pairs, and wgd_plan returns use = 0 for
    npairs > 1024 — so the instance is gone from the library (csrc/conv_valu.hip keeps <KK, 1, ...> alone).  The largest quad count wgd_plan
    lets through is 256."""
    for C in range(4, 1200, 4):
        for (R, S) in ((1, 1), (2, 2), (3, 3), (5, 5)):
            g = geom_of((2, 64, 64, C, 8, R, S, 1, 1, "SAME"))
            pl = wgd_plan(g)
            if pl:
                assert ", 2, " not in wgd_variant(g, pl)[1] or "direct4" not in wgd_variant(g, pl)[1], (C, R, S)
            else:
                assert R * S * C > 1024


def test_narrow_route_refuses_more_images_than_a_grid_holds(fp32_routes):
    """launch_narrow puts the images on the grid's z extent, like the N16 kernels (n16_geom_ok: N <= 65535).  HIP reports
    hipDeviceProp_t::maxGridSize = (2^31 - 1, 65536, 65536) on the MI355X and may refuse a larger launch, so narrow_fwd_ok stops at 65536
    images: (65536, 1, 1, 8 -> 8) is the narrow kernel's, (65537 / 70000, 1, 1, 8 -> 8) the implicit GEMM's, forward and data gradient.
    Host only: these geometries are not launched."""
    K = fp32_routes
    for n, want in ((65536, NARROW), (65537, IGEMM), (70000, IGEMM)):
        case = (n, 1, 1, 8, 8, 3, 3, 1, 1, "SAME")
        for kind in (0, 1):
            assert fp32_expected(case, kind)[0] == want and K.conv_route(lib_geom(K, case), kind) == want, (case, kind)
