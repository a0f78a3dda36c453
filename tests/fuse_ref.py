"""float64 numpy restatement of pnp_fuse_views (csrc/paste.hip) — the reference of tests/test_gpu_fuse.py and
tests/test_gpu_volume_axes.py, pinned to an independent formulation (np.average over the covering views, scipy.stats.entropy) in
tests/test_fuse_host.py.

  fuse(probs, weights)      probs: M arrays [ncls, ...] (float32 as the kernel gets them) -> Result(label uint8 [...] (first maximum of P;
                            0 where no view covers), prob float64 [ncls, ...], entropy float64 [...] normalised by log(ncls), covered bool
                            [...]).  The weights are rounded to float32 first: that is what the kernel receives.
  delta_p(M)                the rounding bound of P, derived at the function
  admissible / entropy_bound   ensemble_ref's, for the labels and the entropy
  make_case / SWEEP / BIG   the cases shared by the host and the GPU tests
"""
import collections

import numpy as np

import ensemble_ref as E

Result = collections.namedtuple("Result", ("label", "prob", "entropy", "covered"))

U = E.U                 # unit roundoff of float32, 2^-24
admissible = E.admissible
entropy_bound = E.entropy_bound


def fuse(probs, weights=None):
    p = np.stack([np.asarray(v, dtype=np.float64) for v in probs])                   # [M, ncls, ...]
    M, ncls = p.shape[:2]
    w = np.ones(M) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    assert w.shape == (M,) and np.all(w > 0) and np.all(np.isfinite(w))
    cover = p.sum(axis=1) > 0.5                                                      # [M, ...]
    wc = w.reshape((M,) + (1,) * (p.ndim - 2)) * cover                               # the weight of a view where it covers, else 0
    wsum = wc.sum(axis=0)
    covered = wsum > 0
    acc = (wc[:, None] * p).sum(axis=0)
    P = np.where(covered[None], acc / np.where(covered, wsum, 1.0)[None], 0.0)
    label = np.where(covered, np.argmax(P, axis=0), 0).astype(np.uint8)
    H = np.where(covered, E.entropy(np.moveaxis(P, 0, -1)), 0.0)
    return Result(label, P, H, covered)


def delta_p(M):
    """|P_c - P_c^ref| <= (2 M + 1) 2^-24 for the same float32 probabilities and weights, M <= 8.
    With u = 2^-24 and n <= M covering views: every product w_v p_v is rounded once and the sum of n products takes n - 1 rounded
    additions (the first lands on an exact 0), so acc = A (1 + theta_n) with A = sum w_v p_v, |theta_k| <= gamma_k = k u / (1 - k u)
    (Higham, Accuracy and Stability, Lemma 3.1); wsum = W (1 + theta_(n-1)) from its n - 1 additions; the division adds one rounding.
    (1 + theta_n) / (1 + theta_(n-1)) (1 + delta) = 1 + theta_(2 n) (Lemma 3.3, j <= k), so |P^ - P| <= gamma_(2 n) P <= gamma_(2 M)
    as P = A / W <= 1 (every p <= 1).  gamma_(2 M) = 2 M u / (1 - 2 M u) < (2 M + 1) u for M <= 8 (16 u * 16 u << u).  Underflow of a
    product (an absolute 2^-150) is far below it.  Coverage is not in doubt: a view's sum is 1 within ncls u, or exactly 0."""
    assert 1 <= M <= 8
    return (2 * M + 1) * U


assert delta_p(8) <= 32 * U

# ---- the cases of tests/test_gpu_fuse.py (shared with the CPU check that the label comparison is not vacuous on them) --------------------
SHAPE = (7, 9, 11)                       # 693 elements: odd, so every vector width has a tail
SWEEP = [(M, ncls) for M in (1, 2, 3, 8) for ncls in (1, 2, 5, 8)]
BIG = (3, 5, 2 ** 20 + 3)                # M, ncls, elements: more than one pass of the grid
# The top-2 gap of this construction has a density of about 3.3 per unit near 0 (some 330 of the 10^6 covered elements lie below 1e-4), so
# about 2.8 elements per million are expected below 2 delta_p(3) = 8.3e-7, and a seed's count scatters around that (seeds 0 .. 5, with and
# without weights: 6 2 4 4 0 7 0 1 2 2 4 4).  The large case uses a seed whose count, by this reference alone, is at most 2 in both runs.
BIG_SEED = 3
VACUITY_SEEDS = range(5)


def softmax32(logits):
    """float32 softmax over axis 0, every step in float32: sums to 1 within rounding"""
    z = logits.astype(np.float32)
    e = np.exp(z - z.max(axis=0, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=0, keepdims=True, dtype=np.float32)).astype(np.float32)


def make_case(M, ncls, n, seed=0, zero_share=0.25):
    """-> (probs: M float32 arrays [ncls, n], weights float32 [M] uniform in [0.5, 2]): the float32 softmax of 3 N(0, 1) logits per view,
    every view independently set to 0 on a random `zero_share` of the elements (mixed coverage; for small M some elements have no view)"""
    rng = np.random.default_rng([seed, M, ncls, n])
    probs = []
    for _ in range(M):
        p = softmax32(3.0 * rng.standard_normal((ncls, n)))
        p[:, rng.random(n) < zero_share] = 0.0
        probs.append(np.ascontiguousarray(p))
    return probs, rng.uniform(0.5, 2.0, M).astype(np.float32)


def ambiguous(ref, M):
    """covered elements that admit more than one class: the label comparison leaves them to the bound"""
    adm = admissible(np.moveaxis(ref.prob, 0, -1), delta_p(M))
    return int(((adm.sum(-1) > 1) & ref.covered).sum())
