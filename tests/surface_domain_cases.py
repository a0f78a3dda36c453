"""The case lists of tests/test_gpu_surface_domain.py (which runs them on the GPU) and tests/test_surface_domain_host.py (which proves
without a GPU, from a restatement of csrc/surface.hip's launch geometry and from the reference, that every branch is reached).  numpy only."""
import math

import numpy as np

import surface_ref as R

# ---- the EDT (pnp_edt3d_sq) ----------------------------------------------------------------------------------------------------------
EDT_SHAPES = [(1, 1, 1), (5, 7, 1), (7, 6, 3), (2, 3, 1024), (3, 1024, 2), (2, 1024, 9), (1024, 2, 9), (3, 200, 70), (130, 9, 33), (9, 5, 257)]
EDT_SPACINGS = [None, (0.7, 1.3, 2.5), (0.05, 1.0, 20.0)]
EDT_FEATURES = ["corner%d" % i for i in range(8)] + ["all", "plane0", "plane1", "plane2", "random", "empty"]
CLOSED_FORM = tuple(f for f in EDT_FEATURES if f != "random")

TILE_FLOATS, EDT_THREADS, KR = 8192, 256, 8      # csrc/surface.hip: kTileFloats, kEdtThreads, kR


def pow2_floor(v):
    p = 1
    while p * 2 <= v:
        p *= 2
    return p


def edt_geometry(shape):
    """edt3d's launches restated: the z pass stages Tz whole lines per workgroup; the y and the x pass put T z columns on the lanes"""
    X, Y, Z = shape
    nlines = X * Y
    Tz = max(1, min(256, TILE_FLOATS // Z))
    g = {"Tz": Tz, "z_groups": -(-nlines // Tz), "z_ragged": nlines % Tz != 0, "z_tail": Z % KR != 0, "passes": []}
    assert Tz * Z <= TILE_FLOATS
    for n in (Y, X):
        T = min(64, pow2_floor(TILE_FLOATS // n))
        while T > 1 and T // 2 >= Z:
            T //= 2
        logT = T.bit_length() - 1
        assert 1 << logT == T and n * T <= TILE_FLOATS
        groups = -(-Z // T)
        g["passes"].append({"n": n, "T": T, "logT": logT, "groups": groups, "last_nz": Z - (groups - 1) * T, "tail": n % KR != 0})
    return g


def plane_index(shape, axis):
    return shape[axis] // 3


def edt_mask(shape, feat):
    m = np.zeros(shape, np.uint8)
    if feat.startswith("corner"):
        i = int(feat[6:])
        m[tuple((s - 1) * ((i >> (2 - a)) & 1) for a, s in enumerate(shape))] = 1
    elif feat == "all":
        m[:] = 1
    elif feat.startswith("plane"):
        a = int(feat[5:])
        sl = [slice(None)] * 3
        sl[a] = plane_index(shape, a)
        m[tuple(sl)] = 1
    elif feat == "random":
        rng = np.random.default_rng(sum(shape) + 5)
        m[rng.random(shape) < 0.01] = 1
        m.flat[rng.integers(0, m.size)] = 1
    else:
        assert feat == "empty"
    return m


_cache = {}


def edt_expected(shape, feat, spacing):
    """float64 squared distances.  `random` is surface_ref.edt_sq itself; the others are closed forms in the reference's own arithmetic
    (coordinates are index * spacing, the squares are summed x + y + z) — the host file pins them to surface_ref.edt_sq at small shapes."""
    key = (shape, feat, spacing)
    if key in _cache:
        return _cache[key]
    s = [1.0, 1.0, 1.0] if spacing is None else [float(v) for v in spacing]
    ax = [np.arange(n, dtype=np.float64) * s[a] for a, n in enumerate(shape)]
    if feat == "random":
        out = R.edt_sq(edt_mask(shape, feat), spacing)
    elif feat == "empty":
        out = np.full(shape, np.inf)
    elif feat == "all":
        out = np.zeros(shape)
    elif feat.startswith("corner"):
        c = np.argwhere(edt_mask(shape, feat))[0]
        d = [(ax[a] - c[a] * s[a]) ** 2 for a in range(3)]
        out = (d[0][:, None, None] + d[1][None, :, None]) + d[2][None, None, :]
    else:
        a = int(feat[5:])
        d = (ax[a] - plane_index(shape, a) * s[a]) ** 2
        out = np.broadcast_to(d.reshape([-1 if i == a else 1 for i in range(3)]), shape).copy()
    out.setflags(write=False)
    _cache[key] = out
    return out


# ---- the metrics (pnp_surface_distances) -----------------------------------------------------------------------------------------------
def _ell(shape, ncls, seeds):
    return R.ellipsoids(shape, ncls, seeds[0]), R.ellipsoids(shape, ncls, seeds[1])


def _ell5_oob():
    """labels -1, ncls and 255 on both sides: in no class, but a neighbour's sameness breaks on them"""
    p, g = _ell((24, 20, 16), 5, (3, 4))
    rng = np.random.default_rng(17)
    for v in (p, g):
        hit = rng.random(v.shape) < 0.03
        v[hit] = rng.choice(np.array([-1, 5, 255], np.int32), size=int(hit.sum()))
    return p, g


ABSENT32 = {"pred": 7, "gt": 9, "both": 11}


def _boxes32():
    """one small box per class 1 ... 31 (class 31 makes bit 31 of the border mask), the ground truth shifted; three classes absent"""
    p, g = np.zeros((66, 8, 9), np.int32), np.zeros((66, 8, 9), np.int32)
    for c in range(1, 32):
        if c not in (ABSENT32["pred"], ABSENT32["both"]):
            p[2 * c:2 * c + 2, 1:5, 2:6] = c
        if c not in (ABSENT32["gt"], ABSENT32["both"]):
            g[2 * c:2 * c + 2, 2:6, 3:6] = c
    return p, g


def _single():
    p, g = np.zeros((5, 6, 7), np.int32), np.zeros((5, 6, 7), np.int32)
    p[1, 1, 1] = 1
    g[3, 4, 5] = 1
    return p, g


LERP_BARS = {1: ((0, 10), (6, 17)), 2: ((0, 5), (3, 10)), 3: ((0, 3), (2, 7)), 4: ((4, 5), (9, 10))}      # class: z range of pred, of gt


def _lerp():
    """one-voxel-thick bars along z (every voxel is border): the pooled n per class is 21, 12, 8 and 2"""
    p, g = np.zeros((4, 4, 20), np.int32), np.zeros((4, 4, 20), np.int32)
    for c, ((p0, p1), (g0, g1)) in LERP_BARS.items():
        p[c - 1, 0, p0:p1] = c
        g[c - 1, 2, g0:g1] = c
    return p, g


def _faces():
    p = np.ones((12, 11, 10), np.int32)
    g = p.copy()
    g[3:9, 3:8, 3:7] = 2
    return p, g


def _tiny():
    rng = np.random.default_rng(23)
    return rng.integers(0, 3, (3, 4, 5)).astype(np.int32), rng.integers(0, 3, (3, 4, 5)).astype(np.int32)


def _shifted_box():
    """a box against itself shifted by one voxel in x, the axis of EXACT_SPACING's smallest step: every distance is 0 or one x step —
    long runs of equal values in the pooled list"""
    p, g = np.zeros((40, 36, 30), np.int32), np.zeros((40, 36, 30), np.int32)
    p[5:35, 4:30, 5:20] = 1
    g[6:36, 4:30, 5:20] = 1
    return p, g


_METRIC_BUILDERS = {
    "ell2": (lambda: _ell((20, 18, 12), 2, (1, 2)), 2), "ell5_oob": (_ell5_oob, 5), "boxes32": (_boxes32, 32), "single": (_single, 2),
    "lerp": (_lerp, 5), "x1": (lambda: _ell((1, 20, 17), 5, (5, 6)), 5), "z1": (lambda: _ell((15, 22, 1), 5, (7, 8)), 5), "faces": (_faces, 3),
    "tiny": (_tiny, 3), "zeros": (lambda: (np.zeros((7, 9, 11), np.int32), np.zeros((7, 9, 11), np.int32)), 5), "shifted_box": (_shifted_box, 2),
}
METRIC_CASES = ["ell2", "ell5_oob", "boxes32", "single", "lerp", "x1", "z1", "faces", "tiny", "zeros"]
EXACT_SPACING = (0.8, 1.1, 2.5)
EXACT_CASES = ["ell5_oob", "shifted_box", "lerp", "boxes32"]       # exact selection under EXACT_SPACING
PUBLIC_CASE = "ell5_oob"                                           # through surface.surface_metrics


def ncls_of(name):
    return _METRIC_BUILDERS[name][1]


def metric_volumes(name):
    key = ("vol", name)
    if key not in _cache:
        p, g = _METRIC_BUILDERS[name][0]()
        for v in (p, g):
            assert v.dtype == np.int32 and v.flags.c_contiguous
            v.setflags(write=False)
        _cache[key] = (p, g)
    return _cache[key]


def metric_reference(name, spacing=None):
    key = ("ref", name, spacing)
    if key not in _cache:
        p, g = metric_volumes(name)
        _cache[key] = R.metrics(p, g, ncls_of(name), spacing)
    return _cache[key]


# ---- numpy.percentile(x, 95), method 'linear', restated as csrc/surface.hip's final kernel computes it ---------------------------------
def lerp_parts(n):
    """-> (klo, khi, g): the two order statistics around the virtual index 0.95 (n - 1) and the weight of the upper one"""
    vi = (n - 1) * 0.95
    lo = math.floor(vi)
    klo = int(lo)
    return klo, min(klo + 1, n - 1), vi - lo


def lerp_branch(n):
    g = lerp_parts(n)[2]
    return "g==0" if g == 0.0 else "g<0.5" if g < 0.5 else "g>=0.5"


def hd95_of_squares(sq):
    """sq: the pooled squared distances (any float dtype; float32 for the kernel's own values).  Selection on the squares (sqrt is
    monotone), sqrt in float64, numpy's two-branch lerp."""
    sq = np.sort(np.asarray(sq).reshape(-1))
    klo, khi, g = lerp_parts(len(sq))
    a, b = math.sqrt(float(sq[klo])), math.sqrt(float(sq[khi]))
    diff = b - a
    return b - diff * (1.0 - g) if g >= 0.5 else a + diff * g
