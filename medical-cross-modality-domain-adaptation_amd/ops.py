"""Drop-in for the reference's ops.py: the sub-pixel phase-shift upsampling `PS` (ops.py:3-27).

The reference builds PS out of reshape/transpose/split/squeeze/concat per channel group; its net effect for
batch_size >= 2 is the closed form
    out[n, i*r+u, j*r+v, c] = X[n, i, j, c*r*r + v*r + u]
(tests/golden pins this against a numpy emulation of the reference op sequence).  Here it is one gather kernel
(pnp_ps_fwd) and its inverse scatter for the gradient.
"""
import torch

from . import functional as Fn
from . import kernels as K
from .functional import PSFn, PSPadFn
from .layers import conv2d


def PS(X, r, n_channel=8, batch_size=10):
    """ops.py:23.  `batch_size` is accepted for signature compatibility; the closed form holds for any batch
    (the reference's batch_size==1 branch yields a transposed image and is never used with B>=2)."""
    if X.shape[-1] != n_channel * r * r:
        raise ValueError("PS: input has %d channels, expected n_channel*r*r = %d" % (X.shape[-1], n_channel * r * r))
    if X.is_meta:   # symbolic build pass
        return torch.empty((X.shape[0], X.shape[1] * r, X.shape[2] * r, n_channel), device="meta")
    return PSFn.apply(X, r, n_channel)


def PS_conv2d(X, W, r, n_channel, keep_prob_, batch_size=10):
    """conv2d(PS(X, r, n_channel), W, keep_prob_, padding='SYMMETRIC') — the segmenter head (adversarial.py:312-316,
    source_segmenter.py:202-206).  The mirror pad of the convolution is written by the PS kernel (pnp_ps_pad_fwd), the convolution then
    runs VALID on that image exactly as it does behind layers._prepad; PNP_PS_FUSE=0: the two calls as written."""
    p = int(W.shape[0]) // 2
    if (Fn.PS_FUSE and not X.is_meta and W.shape[0] == W.shape[1] and X.shape[-1] == n_channel * r * r
            and K.ps_pad_served(r, n_channel, p)):
        return conv2d(PSPadFn.apply(X, r, n_channel, p), W, keep_prob_=keep_prob_, padding='VALID')
    return conv2d(PS(X, r, n_channel=n_channel, batch_size=batch_size), W, keep_prob_=keep_prob_, padding='SYMMETRIC')


def _phase_shift(I, r, batch_size=10):
    """ops.py:3-21, the per-channel-group helper of PS: [B,a,b,r*r] -> [B,a*r,b*r,1] (closed form with one output channel)"""
    return PS(I, r, n_channel=1, batch_size=batch_size)
