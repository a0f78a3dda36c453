"""The case list of tests/test_gpu_fda_domain.py (which runs it on the GPU) and tests/test_fda_domain_host.py (which checks without a GPU,
from a restatement of csrc/fda.hip's launch geometry, that the list reaches every edge below, and that every case meets the input
condition and has an fp32 route within FDA's kernel bar).  numpy and torch on the CPU only.

A case is (name, (B, Bt, H, W, C), band, pair, generator, seed): one call of pnp_fda_amplitude_swap.  Sources come from fda_ref.blobs
where they meet the input condition (band_ratio >= 1e-6) and from fda_ref.spectral (floor SPECTRAL_FLOOR) otherwise; targets are
1.5 x blobs + 0.4.  The edges: every C in 1 ... 4; 1 x 1 to 1024 x 1024 and thin images; the split sums of the two analyses on either
side of their switch (row analysis C (b + 1) = 128 / 132 outputs, column analysis 2b + 1 = 127 / 129, one output over 256 segments on
a 1000-wide row) with extents that end segments unevenly; more than 256 rows and more than 256 floats a row (the NT-strided loops);
the shared arrays of the synthesis kernels filled (b = 511, C = 4); B = Bt = 256 with pair 255, targets shared by unequal bands,
targets unused and targets paired only with band -1."""
import numpy as np

import fda_ref as R

NT = 256                   # csrc/fda.hip: threads a block
MAX_BATCH, MAX_EXTENT, MAX_CH = 256, 1024, 4
MAX_BAND = (MAX_EXTENT - 1) // 2
SPECTRAL_FLOOR = 1e-2


def _full_batch_shared():
    """pair = i // 2: samples 2j and 2j + 1 share target j; bands (j mod 5) - 1 and ((j + 2) mod 5) - 1 always differ, except that
    both are -1 where j is a multiple of 7; targets 128 ... 255 are unused"""
    band, pair = [], []
    for i in range(MAX_BATCH):
        j = i // 2
        band.append(-1 if j % 7 == 0 else (j + 2 * (i % 2)) % 5 - 1)
        pair.append(j)
    return band, pair


_SHARED = _full_batch_shared()

#        name                 (B, Bt, H, W, C)            band                             pair                      generator   seed
CASES = [("c1_16x16",         (2, 2, 16, 16, 1),          [0, 7],                          [1, 0],                   "blobs",    1),
         ("c2_16x16",         (2, 2, 16, 16, 2),          [0, 7],                          [1, 0],                   "blobs",    2),
         ("c3_16x16",         (2, 2, 16, 16, 3),          [0, 7],                          [1, 0],                   "blobs",    3),
         ("c4_16x16",         (2, 2, 16, 16, 4),          [0, 7],                          [1, 0],                   "blobs",    4),
         ("1x1",              (1, 1, 1, 1, 2),            [0],                             [0],                      "blobs",    5),
         ("2x2",              (1, 1, 2, 2, 4),            [0],                             [0],                      "blobs",    6),
         ("1x7",              (1, 1, 1, 7, 3),            [0],                             [0],                      "blobs",    7),
         ("7x1",              (1, 1, 7, 1, 3),            [0],                             [0],                      "blobs",    8),
         ("3x3",              (2, 1, 3, 3, 2),            [1, 1],                          [0, 0],                   "blobs",    9),
         ("1024x3",           (1, 1, 1024, 3, 1),         [1],                             [0],                      "blobs",    10),
         ("3x1024",           (1, 1, 3, 1024, 1),         [1],                             [0],                      "blobs",    11),
         ("row128",           (1, 1, 80, 81, 4),          [31],                            [0],                      "blobs",    12),
         ("row132",           (1, 1, 80, 81, 4),          [32],                            [0],                      "blobs",    13),
         ("col127",           (1, 1, 161, 160, 1),        [63],                            [0],                      "blobs",    14),
         ("col129",           (1, 1, 161, 160, 1),        [64],                            [0],                      "blobs",    15),
         ("one_output",       (1, 1, 1023, 1000, 1),      [0],                             [0],                      "blobs",    16),
         ("rows300",          (2, 2, 300, 64, 2),         [31, 20],                        [1, 0],                   "blobs",    17),
         ("max_b511",         (1, 1, 1024, 1024, 4),      [511],                           [0],                      "spectral", 18),
         ("max_b0",           (1, 1, 1024, 1024, 4),      [0],                             [0],                      "blobs",    19),
         ("max_1024x1023",    (1, 1, 1024, 1023, 4),      [511],                           [0],                      "spectral", 20),
         ("max_1023x1024",    (1, 1, 1023, 1024, 2),      [511],                           [0],                      "spectral", 21),
         ("batch256",         (256, 256, 8, 8, 1),        [i % 5 - 1 for i in range(256)], [255 - i for i in range(256)], "blobs", 22),
         ("batch256_shared",  (256, 256, 8, 8, 1),        _SHARED[0],                      _SHARED[1],               "blobs",    23),
         ("mixed",            (4, 2, 64, 48, 3),          [1, 23, -1, 5],                  [0, 0, 1, 1],             "blobs",    24)]

BY_NAME = {c[0]: c for c in CASES}
BIT_EQUAL_CASES = [c[0] for c in CASES if c[0].startswith("max_") or c[1][0] == MAX_BATCH]      # in place = out of place = a repeat
WRAPPER_CASE = "mixed"                                                                       # kernels.fda_amplitude_swap = the direct call


# ---- csrc/fda.hip's launch geometry, restated ----------------------------------------------------------------------------------------
def segments(nout):
    """threads that share one output's sum (fda.hip segments())"""
    nseg = 1
    while nseg * 2 * nout <= NT:
        nseg *= 2
    return nseg


def target_bands(band, pair, Bt):
    """tband: the largest band of the samples paired with each target, -1 for a target no sample uses"""
    tb = [-1] * Bt
    for b, p in zip(band, pair):
        tb[p] = max(tb[p], b)
    return tb


def analyses(case):
    """[(image band, row-analysis outputs, column-analysis outputs)] of every image the analyses run on (sources, then targets in use)"""
    _, (B, Bt, H, W, C), band, pair, _, _ = case
    return [(b, C * (b + 1), 2 * b + 1) for b in list(band) + target_bands(band, pair, Bt) if b >= 0]


# ---- inputs and references, built once (read-only) -----------------------------------------------------------------------------------
_cache = {}


def inputs(name):
    if ("in", name) not in _cache:
        _, (B, Bt, H, W, C), _, _, gen, seed = BY_NAME[name]
        rng = np.random.default_rng(seed)
        src = R.blobs(rng, B, H, W, C) if gen == "blobs" else R.spectral(rng, B, H, W, C, SPECTRAL_FLOOR)
        tgt = (1.5 * R.blobs(rng, Bt, H, W, C) + 0.4).astype(np.float32)
        for a in (src, tgt):
            a.setflags(write=False)
        _cache[("in", name)] = (src, tgt)
    return _cache[("in", name)]


def reference(name):
    """(float64 reference, fp32 route, route error / max|ref|, bar), once per case"""
    if ("ref", name) not in _cache:
        _, _, band, pair, _, _ = BY_NAME[name]
        src, tgt = inputs(name)
        ref = R.fda_ref(src, tgt, band, pair)
        route = R.fda_route32(src, tgt, band, pair)
        err = float(np.abs(route - ref).max() / np.abs(ref).max())
        for a in (ref, route):
            a.setflags(write=False)
        _cache[("ref", name)] = (ref, route, err, R.route_bar(ref, route))
    return _cache[("ref", name)]
