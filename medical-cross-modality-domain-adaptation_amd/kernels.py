"""Raw (non-autograd) Python entry points over the C-ABI: torch tensors in, torch tensors out.

torch is used here only as the device-memory container and for the current HIP stream; every
arithmetic result comes from libpnp_hip.so.  Tensors are NHWC float32, filters HWIO — the
reference's layouts (layers.py).  Each function names the reference op it stands for.
"""
import ctypes
import os

import torch

from . import _lib
from . import weight_cache as _wc
from ._lib import ConvGeom, PAD_SYMMETRIC, PAD_ZERO, check

_ws_cache = {}


# the current stream's raw handle straight from the C extension: torch.cuda.current_stream() walks is_available() -> os.environ.get on every
# call — 36 % of a joint step's host time at ~700 launches per step (cProfile, tools/experiments/r6_hostprof.py), and the bf16 step is
# host-bound
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_ptr():
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _stream():
    return ctypes.c_void_p(_stream_ptr())


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.PnpError("pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.PnpError("pnp kernels need contiguous float32 tensors, got %s contiguous=%s" % (t.dtype, t.is_contiguous()))
    return ctypes.c_void_p(t.data_ptr())


def _ph(t):
    """device pointer of a contiguous bfloat16 tensor (the bf16-resident convolutions' operands)"""
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous():
        raise _lib.PnpError("expected a contiguous CUDA bfloat16 tensor, got %s %s contiguous=%s" % (t.device, t.dtype, t.is_contiguous()))
    return ctypes.c_void_p(t.data_ptr())


_ws_retired = []     # buffers replaced by a larger one while a recorded step exists: its hipGraph holds their ADDRESSES


def workspace(nbytes, device, slot="main"):
    """Grow-only scratch buffer per (device, slot, stream). All kernels are stream-ordered on the current stream.
    A buffer that has to grow is normally dropped (the allocator recycles it in stream order).  Not while a CapturedStep is alive or a
    stream is recording: a hipGraph replays the ADDRESS it recorded, so the replaced buffer is kept (`_ws_retired`, emptied when the last
    recorded step dies).  Round 6: the generator step's warm-up grew the filter-gradient side stream's buffer AFTER the discriminator
    step had been recorded with the smaller one — the bf16 joint step at B = 16 faulted on replay ("write access to a read-only page")."""
    key = (device.index if isinstance(device, torch.device) else str(device), slot, _stream_ptr())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and (_wc.CACHE.pins > 0 or torch.cuda.is_current_stream_capturing()):
            _ws_retired.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def same_pad(in_size, k, stride, dil=1):
    """TF 'SAME': out = ceil(in/stride); pad_total = max((out-1)*stride + (k-1)*dil + 1 - in, 0); before = total//2."""
    out = -(-in_size // stride)
    eff = (k - 1) * dil + 1
    total = max((out - 1) * stride + eff - in_size, 0)
    return out, total // 2, total - total // 2


CONV_DTYPE = _lib.DTYPE_F32      # arithmetic type new geometries ask for (functional.set_conv_dtype)


def conv_geom(x_shape, w_shape, stride=1, dil=1, padding="SAME", dtype=None):
    """Geometry of layers.conv2d / dilate_conv2d (layers.py:64-74, 84-93)."""
    N, H, W, C = x_shape
    R, S, Cw, K = w_shape
    if Cw != C:
        raise ValueError("conv2d: input has %d channels, filter expects %d" % (C, Cw))
    g = ConvGeom()
    g.N, g.H, g.W, g.C, g.K, g.R, g.S = N, H, W, C, K, R, S
    g.stride, g.dil = stride, dil
    g.dtype = CONV_DTYPE if dtype is None else dtype
    if padding == "SAME":
        g.OH, g.pad_t, _ = same_pad(H, R, stride, dil)
        g.OW, g.pad_l, _ = same_pad(W, S, stride, dil)
        g.pad_mode = PAD_ZERO
    elif padding == "SYMMETRIC":
        # tf.pad(x, floor(k/2), 'SYMMETRIC') then VALID conv (layers.py:19-24)
        ph, pw = R // 2, S // 2
        g.pad_t, g.pad_l = ph, pw
        g.OH = (H + 2 * ph - ((R - 1) * dil + 1)) // stride + 1
        g.OW = (W + 2 * pw - ((S - 1) * dil + 1)) // stride + 1
        g.pad_mode = PAD_SYMMETRIC
    elif padding == "VALID":
        g.pad_t = g.pad_l = 0
        g.OH = (H - ((R - 1) * dil + 1)) // stride + 1
        g.OW = (W - ((S - 1) * dil + 1)) // stride + 1
        g.pad_mode = PAD_ZERO
    else:
        raise ValueError("unknown padding %r" % (padding,))
    return g


def conv2d_fwd(x, w, g, keep_prob=1.0, seed=0, stream_id=0, out=None, naive=False):
    lib = _lib.load()
    y = out if out is not None else torch.empty((g.N, g.OH, g.OW, g.K), dtype=torch.float32, device=x.device)
    if naive:
        check(lib.pnp_conv2d_fwd_naive(_p(x), _p(w), _p(y), ctypes.byref(g), _stream()), "pnp_conv2d_fwd_naive")
    else:
        nbytes = lib.pnp_conv2d_fwd_workspace_bytes(ctypes.byref(g))      # > 0 only for layers with too few output tiles
        ws = workspace(nbytes, x.device) if nbytes else None
        _wino_u(w, g, 0)
        check(lib.pnp_conv2d_fwd_ws(_p(x), _p(w), _p(y), ctypes.byref(g), float(keep_prob), int(seed), int(stream_id),
                                    ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, ws.numel() if ws is not None else 0,
                                    _stream()), "pnp_conv2d_fwd")
    return y


def conv_stats_parts(g):
    """number of BN-statistics partial rows the forward of `g` can leave behind (0: not available, use bn_stats)"""
    return int(_lib.load().pnp_conv2d_fwd_stats_ws_parts(ctypes.byref(g)))


def wino_mode(mode=-1):
    """route policy of the wide stride-1 3x3 convolutions (csrc/conv_wino.hip): 0 direct kernels only, 1 Winograd F(2x2, 3x3) where the
    cost model says it pays, 2 wherever the geometry allows; returns the previous mode (mode < 0: read only)"""
    return int(_lib.load().pnp_conv2d_wino_mode(int(mode)))


def wino_wgrad_mode(mode=-1):
    """the same switch for the filter gradient (pnp_conv2d_wgrad*); returns the previous mode"""
    return int(_lib.load().pnp_conv2d_wino_wgrad_mode(int(mode)))


def wino_tile(tile=-1):
    """largest output tile of the route: 2 = F(2x2, 3x3) only, 4 = F(4x4, 3x3) where its planner takes the layer (36 multiplications per
    4x4 outputs instead of 64; points (0, +-1, 1/2, -2)); returns the previous value (tile < 2: read only)"""
    return int(_lib.load().pnp_conv2d_wino_tile(int(tile)))


def wino_x3(mode=-1):
    """arithmetic of the route's forward / data-gradient GEMMs: 0 = fp32 matrix pipe, 1 = split-bf16 operands (three bf16 planes per value,
    six MFMA products, fp32 accumulation in 64-channel chunks: csrc/conv_wino_x3.hip) where it pays (reductions over >= 256 channels), 2 =
    wherever the shapes allow; returns the previous mode (mode < 0: read only)"""
    return int(_lib.load().pnp_conv2d_wino_x3(int(mode)))


def x3_direct(mode=-1):
    """the narrow 3x3 layers of the Winograd route (32 / 64 input channels, <= 128 filters) as direct split-bf16 convolutions
    (csrc/conv_x3_direct.hip): 0 off, 1 on; returns the previous mode (mode < 0: read only)"""
    return int(_lib.load().pnp_conv2d_x3_direct(int(mode)))


def x3_strided(mode=-1):
    """the strided layers (stride 2..4) on the same direct split-bf16 kernels, forward and stride-phase data gradient, under x3_direct's
    mode: 0 off, 1 on; returns the previous value (mode < 0: read only)"""
    return int(_lib.load().pnp_conv2d_x3_strided(int(mode)))


def x3_wgrad(mode=-1):
    """the filter gradient of the stride-1 3x3 layers with 32 / 64 input channels and 64 filters on the direct split-bf16 kernel
    (csrc/conv_x3_wgrad.hip), under x3_direct's mode: 0 off, 1 on; returns the previous value (mode < 0: read only)"""
    return int(_lib.load().pnp_conv2d_x3_wgrad(int(mode)))


def x3_narrow(mode=-1):
    """the 5x5, 40 -> 5 logits layer's forward and data gradient on the direct split-bf16 kernels (csrc/conv_x3_narrow.hip), under
    x3_direct's mode: 0 off, 1 where a launch fills the chip (>= 256 tiles), 2 wherever the shapes allow; returns the previous mode
    (mode < 0: read only)"""
    return int(_lib.load().pnp_conv2d_x3_narrow(int(mode)))


def wino_chosen(g, kind=0):
    """pnp_conv2d_fwd* (kind 0) / pnp_conv2d_dgrad* (kind 1) / pnp_conv2d_wgrad* (kind 2) of this layer (g = the forward geometry): 0 = the
    direct kernels, else the output tile edge of the Winograd route (2 or 4) — truthy exactly when the layer is on the route"""
    return int(_lib.load().pnp_conv2d_wino_chosen(ctypes.byref(g), int(kind)))


def conv_route(g, kind=0):
    """the kernel family (_lib.ROUTE_*) that serves this layer's forward with the plain epilogue (kind 0) / data gradient (1) / filter gradient
    (2) when the workspace of the query is supplied (g = the forward geometry): pnp_conv2d_route"""
    return int(_lib.load().pnp_conv2d_route(ctypes.byref(g), int(kind)))


# ---- what is kept per filter between launches (weight_cache.py) -------------------------------------------------------------------------
# U = G g G^T of the Winograd route changes only when the filter does.  Filters OWNED BY A VariableStore (variables.py marks their tensors
# `_pnp_var`) get one buffer per pass, lent to the library; the library skips wino_filter_kernel while the entry is valid.  Who a filter
# is and when what was derived from it is stale: weight_cache.py, once, for U and for the bf16 shadows below.  Ad-hoc filters (tests,
# tools) are never bound.  PNP_WINOGRAD_UCACHE=0: off.
U_CACHE = os.environ.get("PNP_WINOGRAD_UCACHE", "1") != "0"


def _wino_u(w, g, kind):
    if U_CACHE:
        _wc.CACHE.bind_u(w, g, kind, _lib.load())


def wino_u_cache_clear():
    """withdraw every transformed-filter buffer (tests; a store that goes away)"""
    _wc.CACHE.clear_u()


def weights_changed(ranges=None):
    """weights were (or are queued to be) written.  ranges: [(first byte address, end address), ...] of what changed — the library drops
    the transformed filters (Winograd route) of exactly those; None: everything.  The bf16 shadows follow the same ranges (round 6: one
    global epoch re-built the shadows of every FROZEN filter after every optimiser step — 102 filter_bf16_kernel launches per joint step)."""
    _wc.CACHE.report(ranges)


def weight_epoch():
    """count of weight-write reports so far (functional: nothing may write parameters between a forward pass and its backward pass)"""
    return _wc.CACHE.log.epoch


def memory_report():
    """bytes of device memory the host side of the library holds on to between steps (nothing reported it):
    grow-only workspaces per (slot, stream), workspaces retired under a recorded step, transformed filters of the Winograd route,
    bf16 filter shadows"""
    nb = lambda t: int(t.numel()) * int(t.element_size())
    rep = {"workspaces": sum(nb(b) for b in _ws_cache.values()), "workspace_buffers": len(_ws_cache),
           "workspaces_retired": sum(nb(b) for b in _ws_retired)}
    rep.update(_wc.CACHE.memory())
    rep["total"] = rep["workspaces"] + rep["workspaces_retired"] + rep["winograd_filters"] + rep["bf16_filter_shadows"]
    return rep


def wino_u_cache_stats(reset=False):
    """(filter transforms skipped, transforms run into a cache entry) since the last reset"""
    h, f = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.load().pnp_conv2d_wino_filter_stats(ctypes.byref(h), ctypes.byref(f), 1 if reset else 0)
    return int(h.value), int(f.value)


def _fwd_ws(g, device):
    nbytes = _lib.load().pnp_conv2d_fwd_workspace_bytes(ctypes.byref(g))
    if not nbytes:
        return None, 0
    ws = workspace(nbytes, device)
    return ctypes.c_void_p(ws.data_ptr()), ws.numel()


def conv2d_fwd_stats(x, w, g, shift, keep_prob=1.0, seed=0, stream_id=0):
    """forward conv (+dropout) that also writes the batch-norm statistics partials of its output -> (y, parts [nparts, 2, K])"""
    lib = _lib.load()
    nparts = conv_stats_parts(g)
    y = torch.empty((g.N, g.OH, g.OW, g.K), dtype=torch.float32, device=x.device)
    parts = workspace(nparts * 2 * g.K * 4, x.device, slot="stats")
    wsp, wsn = _fwd_ws(g, x.device)
    _wino_u(w, g, 0)
    check(lib.pnp_conv2d_fwd_stats_ws(_p(x), _p(w), _p(y), ctypes.byref(g), float(keep_prob), int(seed), int(stream_id), _p(shift),
                                      ctypes.c_void_p(parts.data_ptr()), parts.numel(), wsp, wsn, _stream()), "pnp_conv2d_fwd_stats_ws")
    return y, (parts, nparts)


def bn_stats_finish(parts_n, shift, P, mm=None, mv=None, decay=0.9):
    """(mean, biased var) from conv2d_fwd_stats' partials; with mm / mv also the moving-average update"""
    parts, nparts = parts_n
    C = shift.numel()
    mean = torch.empty(C, dtype=torch.float32, device=shift.device)
    var = torch.empty(C, dtype=torch.float32, device=shift.device)
    check(_lib.load().pnp_bn_stats_finish(ctypes.c_void_p(parts.data_ptr()), int(nparts), _p(shift), _p(mean), _p(var), _p(mm), _p(mv), int(P), C,
                                          float(decay), _stream()), "pnp_bn_stats_finish")
    return mean, var


def bn_fold(gamma, beta, mean, var, eps=1e-3):
    """inference-mode BN as per-channel (scale, shift)"""
    lib = _lib.load()
    C = gamma.numel()
    ss = torch.empty((2, C), dtype=torch.float32, device=gamma.device)
    check(lib.pnp_bn_fold(_p(gamma), _p(beta), _p(mean), _p(var), _p(ss[0]), _p(ss[1]), C, float(eps), _stream()), "pnp_bn_fold")
    return ss


def conv2d_fwd_bn(x, w, g, scale_shift, shortcut=None, alpha=0.2, keep_prob=1.0, seed=0, stream_id=0):
    """conv -> dropout -> inference BN -> (+ shortcut) -> leaky-ReLU in one launch (pnp_conv2d_fwd_bn)"""
    lib = _lib.load()
    y = torch.empty((g.N, g.OH, g.OW, g.K), dtype=torch.float32, device=x.device)
    cs = shortcut.shape[-1] if shortcut is not None else 0
    wsp, wsn = _fwd_ws(g, x.device)
    _wino_u(w, g, 0)
    check(lib.pnp_conv2d_fwd_bn_ws(_p(x), _p(w), _p(y), ctypes.byref(g), float(keep_prob), int(seed), int(stream_id), _p(scale_shift[0]),
                                   _p(scale_shift[1]), _p(shortcut), cs, float(alpha), wsp, wsn, _stream()), "pnp_conv2d_fwd_bn_ws")
    return y


# ---- bf16-resident convolutions (BASELINE configs[4]; csrc/conv_bf16r.hip) ------------------------------------------------------------
def cast_bf16(x):
    """bf16 copy (round-to-nearest-even) of a float32 tensor: pnp_cast_bf16 — for tensors whose producer has no bf16 output"""
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(_lib.load().pnp_cast_bf16(_p(x), _ph(y), x.numel(), _stream()), "pnp_cast_bf16")
    return y


def filter_bf16(w, want_io=True, want_oi=True):
    """bf16 shadows of the fp32 master filter [R,S,C,K]: (w_io [R*S,C,K], w_oi [R*S,K,C])"""
    R, S, C, Kc = w.shape
    w_io = torch.empty((R * S, C, Kc), dtype=torch.bfloat16, device=w.device) if want_io else None
    w_oi = torch.empty((R * S, Kc, C), dtype=torch.bfloat16, device=w.device) if want_oi else None
    check(_lib.load().pnp_filter_bf16(_p(w), _ph(w_io), _ph(w_oi), R, S, C, Kc, _stream()), "pnp_filter_bf16")
    return w_io, w_oi


# bf16 copies ("shadows") of tensors the resident convolutions read.  An activation's shadow is written by its producer (yh / dxh side
# outputs) and travels as an attribute of the tensor OBJECT; a tensor that arrives without one (re-wrapped by a view, produced by a
# kernel without a bf16 output) is cast on demand.  Filter shadows are kept per filter (weight_cache.py): every kernel that writes
# weights (optimisers, clip) and every host-side load reports what it wrote (weights_changed).
CAST_COUNT = [0]          # on-demand casts since the last reset (tests / profiling: how many producers still lack a bf16 output)


class HalfOnly(object):
    """A tensor that exists ONLY as its bf16 copy (the gradient w.r.t. a convolution's accumulator when both of its consumers — data
    and filter gradient — are resident kernels: the float32 copy would be written and never read)."""
    __slots__ = ("h",)

    def __init__(self, h):
        self.h = h

    @property
    def shape(self):
        return self.h.shape


def bf16_of(t):
    if isinstance(t, HalfOnly):
        return t.h
    h = getattr(t, "_pnp_h", None)
    # (while a hipGraph is being recorded a cached shadow would leave the cast OUT of the graph: a replay on new input data would then
    # read the warm-up's copy — cast inside the recording instead)
    if h is not None and h[1] == t._version and h[0].shape == t.shape and not torch.cuda.is_current_stream_capturing():
        return h[0]
    CAST_COUNT[0] += 1
    hh = cast_bf16(t)
    set_bf16(t, hh)
    return hh


def set_bf16(t, h):
    if h is not None:
        t._pnp_h = (h, t._version)
    return t


def _filter_cast(w, into=None):
    """the shadows of `w`: a new pair, or `into` = (w_io, w_oi) written again"""
    if into is None:
        return filter_bf16(w)
    R, S, C, Kc = w.shape
    check(_lib.load().pnp_filter_bf16(_p(w), _ph(into[0]), _ph(into[1]), R, S, C, Kc, _stream()), "pnp_filter_bf16")
    return into


def filter_shadows(w):
    """(w_io, w_oi) of an fp32 filter [R,S,C,K], refreshed when a reported weight write has touched the filter since they were made"""
    return _wc.CACHE.shadows(w, _filter_cast)


_served_cache = {}


def bf16r(g, kind):
    """does the bf16-RESIDENT kernel family serve (geometry, kind) — only asked for geometries whose dtype is PNP_DTYPE_BF16"""
    if g.dtype != _lib.DTYPE_BF16:
        return False
    key = (g.key(), kind)
    v = _served_cache.get(key)
    if v is None:
        v = _served_cache[key] = bf16r_served(g, kind)
    return v


def bf16r_served(g, kind):
    """kind 0 forward / 1 data gradient: do the resident kernels serve this geometry"""
    return bool(_lib.load().pnp_conv2d_bf16r_served(ctypes.byref(g), int(kind)))


def conv2d_fwd_bf16r(xh, w_oi, g, keep_prob=1.0, seed=0, stream_id=0, want_h=False, stat_shift=None, want_stats=False, bn=None):
    """resident forward.  Returns (y, yh or None, parts or None).  want_stats: BN statistics partials (-> bn_stats_finish);
    bn = (scale_shift [2,K], shortcut or None, alpha): fused inference-mode BN + shortcut + leaky-ReLU"""
    lib = _lib.load()
    y = torch.empty((g.N, g.OH, g.OW, g.K), dtype=torch.float32, device=xh.device)
    yh = torch.empty((g.N, g.OH, g.OW, g.K), dtype=torch.bfloat16, device=xh.device) if want_h else None
    parts, nparts, pbytes = None, 0, 0
    if want_stats:
        nparts = int(lib.pnp_conv2d_fwd_bf16r_stats_parts(ctypes.byref(g)))
        parts = workspace(nparts * 2 * g.K * 4, xh.device, slot="stats")
        pbytes = parts.numel()
    ss, sc, alpha = (bn[0], bn[1], bn[2]) if bn is not None else (None, None, -1.0)
    check(lib.pnp_conv2d_fwd_bf16r(_ph(xh), _ph(w_oi), _p(y), _ph(yh), ctypes.byref(g), float(keep_prob), int(seed), int(stream_id),
                                   _p(stat_shift), ctypes.c_void_p(parts.data_ptr()) if parts is not None else None, pbytes,
                                   _p(ss[0]) if ss is not None else None, _p(ss[1]) if ss is not None else None, _p(sc),
                                   sc.shape[-1] if sc is not None else 0, float(alpha), _stream()), "pnp_conv2d_fwd_bf16r")
    return y, yh, ((parts, nparts) if want_stats else None)


def conv2d_dgrad_bf16r(dyh, w_io, g, residual=None, want_h=False):
    lib = _lib.load()
    dx = torch.empty((g.N, g.H, g.W, g.C), dtype=torch.float32, device=dyh.device)
    dxh = torch.empty((g.N, g.H, g.W, g.C), dtype=torch.bfloat16, device=dyh.device) if want_h else None
    check(lib.pnp_conv2d_dgrad_bf16r(_ph(dyh), _ph(w_io), _p(residual), _p(dx), _ph(dxh), ctypes.byref(g), _stream()),
          "pnp_conv2d_dgrad_bf16r")
    return dx, dxh


def conv2d_wgrad_bf16r(xh, dyh, g, into=None):
    """filter gradient from the bf16 copies of x and dy; `into`: dw is ADDED to it (a slot of the gradient arena)"""
    lib = _lib.load()
    nbytes = lib.pnp_conv2d_wgrad_bf16r_workspace_bytes(ctypes.byref(g))
    ws = workspace(nbytes, xh.device)
    dw = into if into is not None else torch.empty((g.R, g.S, g.C, g.K), dtype=torch.float32, device=xh.device)
    if tuple(dw.shape) != (g.R, g.S, g.C, g.K):
        raise ValueError("conv2d_wgrad_bf16r: `into` %s is not the filter shape %s" % (tuple(dw.shape), (g.R, g.S, g.C, g.K)))
    check(lib.pnp_conv2d_wgrad_bf16r(_ph(xh), _ph(dyh), _p(dw), 1 if into is not None else 0, ctypes.byref(g),
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()), "pnp_conv2d_wgrad_bf16r")
    return dw


def conv2d_dgrad(dy, w, g, residual=None):
    """gradient w.r.t. the conv input; with `residual` ([N,H,W,C]) dx = gradient + residual in the same launch (pnp_conv2d_dgrad_add)"""
    lib = _lib.load()
    dx = torch.empty((g.N, g.H, g.W, g.C), dtype=torch.float32, device=dy.device)
    nbytes = lib.pnp_conv2d_dgrad_workspace_bytes(ctypes.byref(g))
    ws = workspace(nbytes, dy.device)
    _wino_u(w, g, 1)
    if residual is not None:
        if tuple(residual.shape) != tuple(dx.shape):
            raise ValueError("conv2d_dgrad: residual %s does not match dx %s" % (tuple(residual.shape), tuple(dx.shape)))
        check(lib.pnp_conv2d_dgrad_add(_p(dy), _p(w), _p(residual), _p(dx), ctypes.byref(g), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                       _stream()), "pnp_conv2d_dgrad_add")
        return dx
    check(lib.pnp_conv2d_dgrad(_p(dy), _p(w), _p(dx), ctypes.byref(g), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          "pnp_conv2d_dgrad")
    return dx


def conv2d_wgrad(x, dy, g, into=None):
    """filter gradient; `into` ([R,S,C,K], e.g. the variable's slot of the gradient arena): dw is ADDED to it (pnp_conv2d_wgrad_acc)
    and `into` is returned"""
    lib = _lib.load()
    nbytes = lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g))
    ws = workspace(nbytes, x.device)
    if into is not None:
        if tuple(into.shape) != (g.R, g.S, g.C, g.K):
            raise ValueError("conv2d_wgrad: `into` %s is not the filter shape %s" % (tuple(into.shape), (g.R, g.S, g.C, g.K)))
        check(lib.pnp_conv2d_wgrad_acc(_p(x), _p(dy), _p(into), ctypes.byref(g), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
              "pnp_conv2d_wgrad_acc")
        return into
    dw = torch.empty((g.R, g.S, g.C, g.K), dtype=torch.float32, device=x.device)
    check(lib.pnp_conv2d_wgrad(_p(x), _p(dy), _p(dw), ctypes.byref(g), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          "pnp_conv2d_wgrad")
    return dw


def dropout(x, keep_prob, seed, stream_id, want_h=False):
    """want_h: also the bf16 copy of the result (attached as its shadow)"""
    lib = _lib.load()
    y = torch.empty_like(x)
    yh = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_h else None
    check(lib.pnp_dropout_h(_p(x), _p(y), _ph(yh), x.numel(), float(keep_prob), int(seed), int(stream_id), _stream()), "pnp_dropout")
    return set_bf16(y, yh)


def bn_stats(x2d_like):
    """per-channel mean / biased variance over all leading dims (layers.py:100, training path)."""
    lib = _lib.load()
    C = x2d_like.shape[-1]
    P = x2d_like.numel() // C
    mean = torch.empty(C, dtype=torch.float32, device=x2d_like.device)
    var = torch.empty(C, dtype=torch.float32, device=x2d_like.device)
    ws = workspace(lib.pnp_bn_workspace_bytes(P, C), x2d_like.device)
    check(lib.pnp_bn_stats(_p(x2d_like), _p(mean), _p(var), P, C, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          "pnp_bn_stats")
    return mean, var


def bn_stats_update(x2d_like, mm, mv, decay=0.9):
    """bn_stats + bn_update_moving in one pass (per-replica statistics)"""
    lib = _lib.load()
    C = x2d_like.shape[-1]
    P = x2d_like.numel() // C
    mean = torch.empty(C, dtype=torch.float32, device=x2d_like.device)
    var = torch.empty(C, dtype=torch.float32, device=x2d_like.device)
    ws = workspace(lib.pnp_bn_workspace_bytes(P, C), x2d_like.device)
    check(lib.pnp_bn_stats_update(_p(x2d_like), _p(mean), _p(var), _p(mm), _p(mv), P, C, float(decay), ctypes.c_void_p(ws.data_ptr()),
                                  ws.numel(), _stream()), "pnp_bn_stats_update")
    return mean, var


def bn_update_moving(mm, mv, mean, var, P, decay=0.9):
    lib = _lib.load()
    check(lib.pnp_bn_update_moving(_p(mm), _p(mv), _p(mean), _p(var), P, mm.numel(), float(decay), _stream()),
          "pnp_bn_update_moving")


def bn_apply(x, mean, var, gamma, beta, shortcut=None, eps=1e-3, alpha=0.2, want_h=False):
    lib = _lib.load()
    C = x.shape[-1]
    P = x.numel() // C
    y = torch.empty_like(x)
    yh = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_h else None
    Cs = shortcut.shape[-1] if shortcut is not None else 0
    check(lib.pnp_bn_apply_h(_p(x), _p(mean), _p(var), _p(gamma), _p(beta), _p(shortcut), Cs, _p(y), _ph(yh), P, C, float(eps),
                             float(alpha), _stream()), "pnp_bn_apply")
    return set_bf16(y, yh)


def bn_bwd(dout, out, x, mean, var, gamma, shortcut_channels=0, eps=1e-3, alpha=0.2, training=True, keep_prob=1.0, seed=0,
           stream_id=0, into=None, beta=None, want_h=False, only_h=False):
    """`into` = (dgamma_slot, dbeta_slot): the parameter gradients are also ADDED to these [C] buffers (pnp_bn_bwd_acc).
    out=None (with `beta`, units without a shortcut): the kernels recompute the activation's sign from x instead of reading `out`"""
    lib = _lib.load()
    C = x.shape[-1]
    P = x.numel() // C
    dx = torch.empty_like(x) if not only_h else None
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    dsc = None
    if shortcut_channels:
        dsc = torch.empty(x.shape[:-1] + (shortcut_channels,), dtype=torch.float32, device=x.device)
    ws = workspace(lib.pnp_bn_workspace_bytes(P, C), x.device)
    dxh = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if (want_h or only_h) else None
    a0, a1 = (into[0], into[1]) if into is not None else (None, None)
    check(lib.pnp_bn_bwd_acc_h(_p(dout), _p(out), _p(x), _p(mean), _p(var), _p(gamma), _p(beta), _p(dx), _ph(dxh), _p(dgamma), _p(dbeta), _p(a0),
                               _p(a1), _p(dsc), shortcut_channels, P, C, float(eps), float(alpha), 1 if training else 0,
                               float(keep_prob), int(seed), int(stream_id), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          "pnp_bn_bwd_acc" if into is not None else "pnp_bn_bwd")
    return (HalfOnly(dxh) if only_h else set_bf16(dx, dxh)), dgamma, dbeta, dsc


def bn_bwd_reduce(dout, out, x, mean, var, eps=1e-3, alpha=0.2, gamma=None, beta=None):
    """local sums (dgamma = sum dz*xhat, dbeta = sum dz) — first half of bn_bwd, for SyncBN"""
    lib = _lib.load()
    C = x.shape[-1]
    P = x.numel() // C
    sums = torch.empty((2, C), dtype=torch.float32, device=x.device)      # [dgamma, dbeta]
    ws = workspace(lib.pnp_bn_workspace_bytes(P, C), x.device)
    check(lib.pnp_bn_bwd_reduce(_p(dout), _p(out), _p(x), _p(mean), _p(var), _p(gamma), _p(beta), _p(sums[0]), _p(sums[1]), P, C, float(eps), float(alpha),
                                ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()), "pnp_bn_bwd_reduce")
    return sums


def bn_bwd_apply(dout, out, x, mean, var, gamma, sums, P_norm, shortcut_channels=0, eps=1e-3, alpha=0.2, training=True, keep_prob=1.0,
                 seed=0, stream_id=0, beta=None, want_h=False, only_h=False):
    """second half of bn_bwd with the (possibly all-reduced) sums and the row count behind them"""
    lib = _lib.load()
    C = x.shape[-1]
    P = x.numel() // C
    dx = torch.empty_like(x) if not only_h else None
    dsc = None
    if shortcut_channels:
        dsc = torch.empty(x.shape[:-1] + (shortcut_channels,), dtype=torch.float32, device=x.device)
    dg, db = (sums[0], sums[1]) if sums is not None else (None, None)      # not read in inference mode
    dxh = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if (want_h or only_h) else None
    check(lib.pnp_bn_bwd_apply_h(_p(dout), _p(out), _p(x), _p(mean), _p(var), _p(gamma), _p(beta), _p(dg), _p(db), _p(dx), _ph(dxh), _p(dsc),
                                 shortcut_channels, P, int(P_norm), C, float(eps), float(alpha), 1 if training else 0, float(keep_prob),
                                 int(seed), int(stream_id), _stream()), "pnp_bn_bwd_apply")
    return (HalfOnly(dxh) if only_h else set_bf16(dx, dxh)), dsc


def maxpool2_fwd(x):
    lib = _lib.load()
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    check(lib.pnp_maxpool2_fwd(_p(x), _p(y), N, H, W, C, _stream()), "pnp_maxpool2_fwd")
    return y


def maxpool2_bwd(x, dy):
    lib = _lib.load()
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    check(lib.pnp_maxpool2_bwd(_p(x), _p(dy), _p(dx), N, H, W, C, _stream()), "pnp_maxpool2_bwd")
    return dx


def ps_fwd(x, r, nc):
    lib = _lib.load()
    N, A, B, Cin = x.shape
    if Cin != nc * r * r:
        raise ValueError("PS: %d channels != n_channel*r*r = %d" % (Cin, nc * r * r))
    y = torch.empty((N, A * r, B * r, nc), dtype=torch.float32, device=x.device)
    check(lib.pnp_ps_fwd(_p(x), _p(y), N, A, B, r, nc, _stream()), "pnp_ps_fwd")
    return y


def ps_bwd(dy, r, nc):
    lib = _lib.load()
    N, Ar, Br, _ = dy.shape
    A, B = Ar // r, Br // r
    dx = torch.empty((N, A, B, nc * r * r), dtype=torch.float32, device=dy.device)
    check(lib.pnp_ps_bwd(_p(dy), _p(dx), N, A, B, r, nc, _stream()), "pnp_ps_bwd")
    return dx


def sympad_fwd(x, p):
    """tf.pad(x, p, 'SYMMETRIC') in H and W (layers.py:23,72,91)"""
    lib = _lib.load()
    N, H, W, C = x.shape
    xp = torch.empty((N, H + 2 * p, W + 2 * p, C), dtype=torch.float32, device=x.device)
    check(lib.pnp_sympad_fwd(_p(x), _p(xp), N, H, W, C, p, _stream()), "pnp_sympad_fwd")
    return xp


def sympad_bwd(dxp, p):
    lib = _lib.load()
    N, Hp, Wp, C = dxp.shape
    dx = torch.empty((N, Hp - 2 * p, Wp - 2 * p, C), dtype=torch.float32, device=dxp.device)
    check(lib.pnp_sympad_bwd(_p(dxp), _p(dx), N, Hp - 2 * p, Wp - 2 * p, C, p, _stream()), "pnp_sympad_bwd")
    return dx


def ps_pad_served(r, nc, p):
    """the geometries pnp_ps_pad_fwd / _bwd take: a coarse pixel's nc*r*r channels fit the kernels' LDS tile, the mirror stays inside the
    first / last coarse pixel"""
    return nc * r * r <= 4096 and 0 <= p <= r


def ps_pad_fwd(x, r, nc, p):
    """sympad_fwd(ps_fwd(x, r, nc), p) in one pass (bit-identical)"""
    lib = _lib.load()
    N, A, B, Cin = x.shape
    if Cin != nc * r * r:
        raise ValueError("PS: %d channels != n_channel*r*r = %d" % (Cin, nc * r * r))
    xp = torch.empty((N, A * r + 2 * p, B * r + 2 * p, nc), dtype=torch.float32, device=x.device)
    check(lib.pnp_ps_pad_fwd(_p(x), _p(xp), N, A, B, r, nc, p, _stream()), "pnp_ps_pad_fwd")
    return xp


def ps_pad_bwd(dxp, r, nc, p):
    """ps_bwd(sympad_bwd(dxp, p), r, nc) in one pass (bit-identical: the mirrored positions are summed in sympad_bwd's order)"""
    lib = _lib.load()
    N, Hp, Wp, _ = dxp.shape
    A, B = (Hp - 2 * p) // r, (Wp - 2 * p) // r
    dx = torch.empty((N, A, B, nc * r * r), dtype=torch.float32, device=dxp.device)
    check(lib.pnp_ps_pad_bwd(_p(dxp), _p(dx), N, A, B, r, nc, p, _stream()), "pnp_ps_pad_bwd")
    return dx


def seg_loss_fwd(logits, y, miu_cross=1.0, miu_dice=1.0):
    """returns (out[3] = total, xent, dice ; workspace tensor to hand to seg_loss_bwd)"""
    lib = _lib.load()
    ncls = logits.shape[-1]
    P = logits.numel() // ncls
    out = torch.empty(3, dtype=torch.float32, device=logits.device)
    ws = torch.empty(lib.pnp_seg_loss_workspace_bytes(P, ncls), dtype=torch.uint8, device=logits.device)
    check(lib.pnp_seg_loss_fwd(_p(logits), _p(y), _p(out), P, ncls, float(miu_cross), float(miu_dice),
                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()), "pnp_seg_loss_fwd")
    return out, ws


def seg_loss_bwd(logits, y, ws, miu_cross=1.0, miu_dice=1.0, gscale=1.0, P_norm=None):
    """P_norm: pixel count behind the sums in `ws` when they were all-reduced over the replicas (default: this tensor's)"""
    lib = _lib.load()
    ncls = logits.shape[-1]
    P = logits.numel() // ncls
    dl = torch.empty_like(logits)
    check(lib.pnp_seg_loss_bwd_norm(_p(logits), _p(y), _p(dl), P, int(P_norm or P), ncls, float(miu_cross), float(miu_dice),
                                    float(gscale), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()), "pnp_seg_loss_bwd_norm")
    return dl


def seg_loss_sums(ws):
    """the 32 double sums at the head of a seg_loss workspace (per class: n_i, sum p*y, sum p*p, cross-entropy terms), as a view"""
    return ws[:256].view(torch.float64)


def softmax_argmax(logits, want_prob=True):
    """layers.pixel_wise_softmax_2 + tf.argmax(.,3) (layers.py:134-138; source_segmenter.py:80-81)"""
    lib = _lib.load()
    ncls = logits.shape[-1]
    P = logits.numel() // ncls
    prob = torch.empty_like(logits) if want_prob else None
    label = torch.empty(logits.shape[:-1], dtype=torch.int64, device=logits.device)
    check(lib.pnp_softmax_argmax(_p(logits), _p(prob), ctypes.c_void_p(label.data_ptr()), P, ncls, _stream()), "pnp_softmax_argmax")
    return prob, label


def dice_eval(label, y):
    """lib._dice_eval (lib.py:96-110): returns tensor [1+ncls] = (mean, per-class...)"""
    lib = _lib.load()
    ncls = y.shape[-1]
    P = y.numel() // ncls
    out = torch.empty(1 + ncls, dtype=torch.float32, device=y.device)
    ws = workspace(1024 * 24 * 4, y.device)
    check(lib.pnp_dice_eval(ctypes.c_void_p(label.data_ptr()), _p(y), _p(out), P, ncls, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                            _stream()), "pnp_dice_eval")
    return out


def label_decomp(label, ncls):
    """lib._label_decomp (lib.py:75-92) on the device: integer-valued float label map [...] -> one-hot float32 [..., ncls]"""
    lab = label if label.dtype == torch.float32 else label.to(torch.float32)
    lab = lab.contiguous()
    out = torch.empty(tuple(lab.shape) + (ncls,), dtype=torch.float32, device=lab.device)
    check(_lib.load().pnp_label_decomp(_p(lab), _p(out), lab.numel(), int(ncls), _stream()), "pnp_label_decomp")
    return out


def confusion_matrix(y, pred=None, want_compact=True):
    """(compact_y = argmax of the one-hot labels, confusion matrix [ncls, ncls] int64 rows = truth) — source_segmenter.py:83-85"""
    ncls = y.shape[-1]
    P = y.numel() // ncls
    cy = torch.empty(y.shape[:-1], dtype=torch.int64, device=y.device) if want_compact else None
    cm = torch.empty((ncls, ncls), dtype=torch.int64, device=y.device) if pred is not None else None
    if pred is not None and (pred.dtype != torch.int64 or not pred.is_contiguous()):
        raise _lib.PnpError("confusion_matrix: pred must be a contiguous int64 label map")
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    check(_lib.load().pnp_confusion_matrix(_p(y), vp(pred), vp(cy), vp(cm), P, ncls, _stream()), "pnp_confusion_matrix")
    return cy, cm


def _spacing3(spacing):
    s = (1.0, 1.0, 1.0) if spacing is None else tuple(float(v) for v in spacing)
    if len(s) != 3:
        raise ValueError("spacing: 3 values (one per array axis) expected, got %r" % (spacing,))
    return s


def _labels_i32(t, what):
    if not t.is_cuda:
        raise _lib.PnpError("%s: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback" % what)
    if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 3:
        raise _lib.PnpError("%s: a contiguous int32 [X, Y, Z] CUDA tensor expected, got %s %s contiguous=%s" % (what, t.dtype, tuple(t.shape),
                                                                                                              t.is_contiguous()))
    return ctypes.c_void_p(t.data_ptr())


def edt_sq(mask_u8, spacing=None):
    """exact squared Euclidean distance transform (physical units) of a uint8 [X, Y, Z] mask to its non-zero voxels (pnp_edt3d_sq);
    +inf everywhere when the mask is empty"""
    if not mask_u8.is_cuda:
        raise _lib.PnpError("edt_sq: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    if mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous() or mask_u8.dim() != 3:
        raise _lib.PnpError("edt_sq: a contiguous uint8 [X, Y, Z] CUDA tensor expected, got %s %s" % (mask_u8.dtype, tuple(mask_u8.shape)))
    sx, sy, sz = _spacing3(spacing)
    out = torch.empty(mask_u8.shape, dtype=torch.float32, device=mask_u8.device)
    X, Y, Z = mask_u8.shape
    check(_lib.load().pnp_edt3d_sq(ctypes.c_void_p(mask_u8.data_ptr()), _p(out), X, Y, Z, sx, sy, sz, _stream()), "pnp_edt3d_sq")
    return out


def surface_distances(pred_i32, gt_i32, ncls, spacing=None):
    """per-class surface-distance rows of two int32 [X, Y, Z] label volumes (pnp_surface_distances) -> float64 [ncls, 7] device tensor:
    n_border_pred, n_border_gt, sum pred->gt, sum gt->pred, max pred->gt, max gt->pred, hd95"""
    pp, gp = _labels_i32(pred_i32, "surface_distances"), _labels_i32(gt_i32, "surface_distances")
    if tuple(pred_i32.shape) != tuple(gt_i32.shape):
        raise _lib.PnpError("surface_distances: prediction %s and ground truth %s differ in shape" % (tuple(pred_i32.shape), tuple(gt_i32.shape)))
    sx, sy, sz = _spacing3(spacing)
    X, Y, Z = pred_i32.shape
    lib = _lib.load()
    need = lib.pnp_surface_workspace_bytes(X, Y, Z, int(ncls))
    if need == 0:
        raise _lib.PnpError("surface_distances: unsupported volume %s / ncls %d (extents <= 1024, 2 <= ncls <= 32)" % ((X, Y, Z), ncls))
    out = torch.empty((int(ncls), 7), dtype=torch.float64, device=pred_i32.device)
    ws = workspace(need, pred_i32.device, slot="surface")
    check(lib.pnp_surface_distances(pp, gp, X, Y, Z, int(ncls), sx, sy, sz, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                    ws.numel(), _stream()), "pnp_surface_distances")
    return out


def gp_interpolate(a, b, seed, stream_id):
    """WGAN-GP interpolation x_hat = eps_i * a + (1 - eps_i) * b per sample i of the leading dim (pnp_gp_interpolate) -> (x_hat, eps [B])"""
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("gp_interpolate: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    B = a.shape[0]
    out = torch.empty_like(a)
    eps = torch.empty(B, dtype=torch.float32, device=a.device)
    check(_lib.load().pnp_gp_interpolate(_p(a), _p(b), _p(out), _p(eps), B, a.numel() // B, int(seed), int(stream_id), _stream()),
          "pnp_gp_interpolate")
    return out, eps


def gp_penalty_(g, coef, gscale=1.0):
    """per-sample norms of g [B, ...], penalty coef * mean_i (|g_i| - 1)^2; g is overwritten by gscale * dP/dg (pnp_gp_penalty)
    -> (penalty [1], norms [B])"""
    lib = _lib.load()
    B = g.shape[0]
    n = g.numel() // B
    norms = torch.empty(B, dtype=torch.float32, device=g.device)
    pen = torch.empty(1, dtype=torch.float32, device=g.device)
    ws = workspace(lib.pnp_gp_workspace_bytes(B, n), g.device)
    check(lib.pnp_gp_penalty(_p(g), B, n, float(coef), float(gscale), _p(norms), _p(pen), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                             _stream()), "pnp_gp_penalty")
    return pen, norms


def bn_dbl_bwd(gc_bar, d, y, gy, mean, var, gamma, sc_bar=None, eps=1e-3, alpha=0.2, keep_prob=1.0, seed=0, stream_id=0, gamma_bar=None):
    """double backward of conv -> dropout -> BN(train) [-> + pad(shortcut)] -> leaky (pnp_bn_dbl_bwd) -> (gy_bar, xc_bar); gamma_bar
    ([C], e.g. the variable's gradient slot) is ADDED to"""
    lib = _lib.load()
    C = d.shape[-1]
    P = d.numel() // C
    gy_bar = torch.empty_like(d)
    xc_bar = torch.empty_like(d)
    Cs = sc_bar.shape[-1] if sc_bar is not None else 0
    ws = workspace(lib.pnp_bn_dbl_bwd_workspace_bytes(P, C), d.device)
    check(lib.pnp_bn_dbl_bwd(_p(gc_bar), _p(d), _p(y), _p(gy), _p(mean), _p(var), _p(gamma), _p(sc_bar), Cs, _p(gy_bar), _p(xc_bar),
                             _p(gamma_bar), P, C, float(eps), float(alpha), float(keep_prob), int(seed), int(stream_id),
                             ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()), "pnp_bn_dbl_bwd")
    return gy_bar, xc_bar


def bn_moments(mean, var):
    C = mean.numel()
    mom = torch.empty(2 * C, dtype=torch.float64, device=mean.device)
    check(_lib.load().pnp_bn_moments(_p(mean), _p(var), ctypes.c_void_p(mom.data_ptr()), C, _stream()), "pnp_bn_moments")
    return mom


def bn_from_moments(mom, world):
    C = mom.numel() // 2
    mean = torch.empty(C, dtype=torch.float32, device=mom.device)
    var = torch.empty(C, dtype=torch.float32, device=mom.device)
    check(_lib.load().pnp_bn_from_moments(ctypes.c_void_p(mom.data_ptr()), int(world), _p(mean), _p(var), C, _stream()), "pnp_bn_from_moments")
    return mean, var


def _bumps_weights(fn):
    """a kernel that writes the weight arena: the filters' bf16 shadows and transformed filters are stale afterwards.
    ranges=[(lo, hi), ...]: byte-address ranges of the weights this call writes (an optimiser over a var_list: the chunks its mask selects)"""
    def wrapped(*a, **k):
        weights_changed(k.pop("ranges", None))
        return fn(*a, **k)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def _u8p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@_bumps_weights
def adam_step(w, g, m, v, chunk_l2, chunk_mask, lr, beta1, beta2, eps, t):
    check(_lib.load().pnp_adam_step(_p(w), _p(g), _p(m), _p(v), w.numel(), _p(chunk_l2), _u8p(chunk_mask), float(lr), float(beta1),
                                    float(beta2), float(eps), int(t), _stream()), "pnp_adam_step")


@_bumps_weights
def rmsprop_step(w, g, ms, chunk_l2, chunk_mask, lr, decay=0.9, eps=1e-10):
    check(_lib.load().pnp_rmsprop_step(_p(w), _p(g), _p(ms), w.numel(), _p(chunk_l2), _u8p(chunk_mask), float(lr), float(decay),
                                       float(eps), _stream()), "pnp_rmsprop_step")


@_bumps_weights
def momentum_step(w, g, acc, chunk_l2, chunk_mask, lr, momentum):
    check(_lib.load().pnp_momentum_step(_p(w), _p(g), _p(acc), w.numel(), _p(chunk_l2), _u8p(chunk_mask), float(lr),
                                        float(momentum), _stream()), "pnp_momentum_step")


@_bumps_weights
def clip(w, chunk_mask, lo, hi):
    check(_lib.load().pnp_clip(_p(w), w.numel(), _u8p(chunk_mask), float(lo), float(hi), _stream()), "pnp_clip")


def l2_loss(w, chunk_l2):
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.float32, device=w.device)
    ws = workspace(lib.pnp_reduce_workspace_bytes(w.numel()), w.device)
    check(lib.pnp_l2_loss(_p(w), w.numel(), _p(chunk_l2), _p(out), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          "pnp_l2_loss")
    return out


def axpby(x, y, a, b):
    check(_lib.load().pnp_axpby(_p(x), _p(y), x.numel(), float(a), float(b), _stream()), "pnp_axpby")
    return y


def add(x, y):
    """x + y into a new tensor (pnp_add)"""
    out = torch.empty_like(x)
    check(_lib.load().pnp_add(_p(x), _p(y), _p(out), x.numel(), _stream()), "pnp_add")
    return out


def fill_(t, value):
    check(_lib.load().pnp_fill(_p(t), t.numel(), float(value), _stream()), "pnp_fill")
    return t


def critic_input_fwd(a, tile_a, b, c, d, logits):
    lib = _lib.load()
    P = logits.numel() // logits.shape[-1]
    Ca, Cb, Cc, Cd, ncls = a.shape[-1], b.shape[-1], c.shape[-1], d.shape[-1], logits.shape[-1]
    Ct = Ca * tile_a + Cb + Cc + Cd + ncls + 1
    out = torch.empty(logits.shape[:-1] + (Ct,), dtype=torch.float32, device=logits.device)
    check(lib.pnp_critic_input_fwd(_p(a), Ca, tile_a, _p(b), Cb, _p(c), Cc, _p(d), Cd, _p(logits), ncls, _p(out), P, _stream()),
          "pnp_critic_input_fwd")
    return out


def critic_input_bwd(dout, shapes, tile_a, need=(True,) * 5):
    lib = _lib.load()
    (sa, sb, sc, sd, sl) = shapes
    P = dout.numel() // dout.shape[-1]
    mk = lambda s, n: torch.empty(s, dtype=torch.float32, device=dout.device) if n else None
    da, db, dc, dd, dl = mk(sa, need[0]), mk(sb, need[1]), mk(sc, need[2]), mk(sd, need[3]), mk(sl, need[4])
    check(lib.pnp_critic_input_bwd(_p(dout), _p(da), sa[-1], tile_a, _p(db), sb[-1], _p(dc), sc[-1], _p(dd), sd[-1], _p(dl), sl[-1],
                                   P, _stream()), "pnp_critic_input_bwd")
    return da, db, dc, dd, dl


def critic_input_ps_served(channels, tile_a, ncls, r):
    """the sizes pnp_critic_input_ps_fwd / _bwd take (channels: of a, b, c, d AFTER PS): the four sources' coarse pixel fits the forward's
    LDS tile, one coarse pixel's r x r fine pixels of dout the backward's"""
    ctot = channels[0] * tile_a + sum(channels[1:]) + ncls + 1
    return sum(channels) * r * r <= 4096 and r * (r * (ctot + 8) + 1) <= 6144


def critic_input_ps_fwd(a, tile_a, b, c, d, logits, r):
    """critic_input_fwd(ps_fwd(a), tile_a, ps_fwd(b), ps_fwd(c), ps_fwd(d), logits) from the coarse a..d [N,A,B,C*r*r] (bit-identical)"""
    lib = _lib.load()
    N, A, B, _ = a.shape
    rr = r * r
    Ca, Cb, Cc, Cd, ncls = a.shape[-1] // rr, b.shape[-1] // rr, c.shape[-1] // rr, d.shape[-1] // rr, logits.shape[-1]
    for t, C in ((a, Ca), (b, Cb), (c, Cc), (d, Cd)):
        if tuple(t.shape) != (N, A, B, C * rr):
            raise ValueError("critic_input_ps_fwd: coarse tensor %r, expected [%d,%d,%d,C*%d]" % (tuple(t.shape), N, A, B, rr))
    if tuple(logits.shape[:3]) != (N, A * r, B * r):
        raise ValueError("critic_input_ps_fwd: logits %r on a grid other than [%d,%d,%d]" % (tuple(logits.shape), N, A * r, B * r))
    Ct = Ca * tile_a + Cb + Cc + Cd + ncls + 1
    out = torch.empty((N, A * r, B * r, Ct), dtype=torch.float32, device=logits.device)
    check(lib.pnp_critic_input_ps_fwd(_p(a), Ca, tile_a, _p(b), Cb, _p(c), Cc, _p(d), Cd, _p(logits), ncls, _p(out), N, A, B, r, _stream()),
          "pnp_critic_input_ps_fwd")
    return out


def critic_input_ps_bwd(dout, shapes, tile_a, r, need=(True,) * 5):
    """the coarse gradients of a..d and dlogits from dout [N,A*r,B*r,Ctot]; shapes: of the coarse a..d and of logits (bit-identical to
    critic_input_bwd + ps_bwd x4)"""
    lib = _lib.load()
    (sa, sb, sc, sd, sl) = shapes
    N, A, B, _ = sa
    rr = r * r
    mk = lambda s, n: torch.empty(s, dtype=torch.float32, device=dout.device) if n else None
    da, db, dc, dd, dl = mk(sa, need[0]), mk(sb, need[1]), mk(sc, need[2]), mk(sd, need[3]), mk(sl, need[4])
    check(lib.pnp_critic_input_ps_bwd(_p(dout), _p(da), sa[-1] // rr, tile_a, _p(db), sb[-1] // rr, _p(dc), sc[-1] // rr, _p(dd), sd[-1] // rr,
                                      _p(dl), sl[-1], N, A, B, r, _stream()), "pnp_critic_input_ps_bwd")
    return da, db, dc, dd, dl


def wgan_loss(ct_cls, mr_cls, ct_mask, mr_mask, coefs):
    """adversarial.py:455-459: sum_i coef_i * mean(logits_i) over the non-None critic outputs -> 1-element tensor"""
    ref = next(t for t in (ct_cls, mr_cls, ct_mask, mr_mask) if t is not None)
    out = torch.empty(1, dtype=torch.float32, device=ref.device)
    check(_lib.load().pnp_wgan_loss(_p(ct_cls), _p(mr_cls), _p(ct_mask), _p(mr_mask), ref.numel(), float(coefs[0]), float(coefs[1]),
                                    float(coefs[2]), float(coefs[3]), _p(out), _stream()), "pnp_wgan_loss")
    return out


def softmax_entropy(logits, coef=1.0, want_grad=False):
    """normalised mean entropy of softmax(logits [..., ncls]) (csrc/entropy.hip) -> (value [1], not scaled by coef;
    coef * d value / d logits, or None without want_grad).  One streaming pass, stream-ordered, bit-identical from run to run."""
    return _pixel_loss("pnp_softmax_entropy", logits, (_p(logits),), (), coef, want_grad)


def _pixel_loss(entry, logits, inputs, scalars, coef, want_grad):
    """the common part of the per-pixel loss terms (csrc/pixel_loss.h): lib.`entry`(*inputs, P, ncls, *scalars, coef, dlogits, out,
    workspace, bytes, stream), inputs = the pointers of the logits and of the term's extra inputs, with the workspace that
    lib.`entry`_workspace_bytes(P, ncls) asks for -> (value [1], dlogits | None)"""
    lib = _lib.load()
    ncls = logits.shape[-1]
    P = logits.numel() // max(ncls, 1)
    out = torch.empty(1, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    ws = workspace(getattr(lib, entry + "_workspace_bytes")(P, ncls), logits.device)      # per-block partials, read by the second launch
    check(getattr(lib, entry)(*inputs, P, ncls, *scalars, float(coef), _p(dl), _p(out), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          entry)
    return out, dl


def class_mask(classes, ncls):
    """bit mask of an iterable of class indices; None = every class but the background (1 ... ncls-1).  ValueError out of range."""
    if classes is None:
        classes = range(1, ncls)
    mask = 0
    for c in classes:
        if int(c) != c or not 0 <= int(c) < ncls:
            raise ValueError("class index %r is not one of 0 ... %d" % (c, ncls - 1))
        mask |= 1 << int(c)
    return mask


def signed_distance_2d(y, classes=None):
    """signed distance maps of one-hot labels y [B, H, W, ncls] (csrc/boundary.hip) -> phi [B, H, W, ncls]: per slice and
    selected class the Euclidean distance in pixels to the nearest pixel of the other membership, d outside the class and -(d - 1) inside
    it; 0 for a class that is absent from or fills the slice and for a class that is not selected.  classes: iterable of class indices,
    default every class but the background.  Exact, stream-ordered, bit-identical from run to run."""
    lib = _lib.load()
    py = _p(y)
    if y.dim() != 4:
        raise _lib.PnpError("signed_distance_2d: one-hot labels [B, H, W, ncls] expected, got shape %s" % (tuple(y.shape),))
    B, H, W, ncls = y.shape
    mask = class_mask(classes, ncls) if ncls <= 32 else 0          # (more than 8 classes: refused by the library, with its message)
    phi = torch.empty_like(y)
    ws = workspace(lib.pnp_signed_distance_2d_workspace_bytes(B, H, W, ncls, mask), y.device)      # row distances, read by the second launch
    check(lib.pnp_signed_distance_2d(py, B, H, W, ncls, mask, _p(phi), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
          "pnp_signed_distance_2d")
    return phi


def boundary_loss(logits, phi, nsel, coef=1.0, want_grad=False):
    """boundary loss (csrc/boundary.hip): mean over pixels and the nsel selected classes of softmax(logits) * phi ->
    (value [1], not scaled by coef; coef * d value / d logits, or None without want_grad).  One streaming pass, stream-ordered,
    bit-identical from run to run."""
    inputs = (_p(logits), _p(phi))
    if phi.shape != logits.shape:
        raise _lib.PnpError("boundary_loss: phi %s does not have the shape of the logits %s" % (tuple(phi.shape), tuple(logits.shape)))
    return _pixel_loss("pnp_boundary_loss", logits, inputs, (int(nsel),), coef, want_grad)


def pseudo_label_loss(logits, thresholds, classes=None, coef=1.0, want_grad=False):
    """class-balanced pseudo-label term of softmax(logits [..., ncls]) against its own arg-max where it is confident (csrc/pseudo_label.hip,
    DESIGN.md §29).  thresholds: float32 device tensor [ncls], read by the kernel.  classes: iterable of class indices the term is
    restricted to, default EVERY class, the background included.  -> (value [1] = sum over selected pixels of -log p_argmax / P, not
    scaled by coef; share [1] of the pixels selected; counts int32 [2, ncls]: pixels predicted as / selected as each class; labels uint8
    [...] = class | selected << 7; conf float32 [...] = softmax of the arg-max class; coef * d value / d logits, or None without
    want_grad).  value and share are views of one [2] tensor.  One streaming pass, stream-ordered, bit-identical from run to run."""
    lib = _lib.load()
    pl, pt = _p(logits), _p(thresholds)
    ncls = logits.shape[-1]
    P = logits.numel() // max(ncls, 1)
    if thresholds.numel() != ncls:
        raise _lib.PnpError("pseudo_label_loss: %d thresholds for %d classes" % (thresholds.numel(), ncls))
    mask = 0 if ncls > 32 else ((1 << ncls) - 1 if classes is None else class_mask(classes, ncls))      # (> 8 classes: the library refuses)
    dev = logits.device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    counts = torch.empty((2, ncls), dtype=torch.int32, device=dev)
    labels = torch.empty(logits.shape[:-1], dtype=torch.uint8, device=dev)
    conf = torch.empty(logits.shape[:-1], dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_grad else None
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = workspace(lib.pnp_pseudo_label_loss_workspace_bytes(P, ncls), dev)      # per-block partials, read by the second launch
    check(lib.pnp_pseudo_label_loss(pl, pt, P, ncls, mask, float(coef), _p(dl), vp(labels), _p(conf), _p(out), vp(counts), vp(ws), ws.numel(),
                                    _stream()), "pnp_pseudo_label_loss")
    return out[0:1], out[1:2], counts, labels, conf, dl


def pseudo_label_update(labels, conf, thresholds, portion, momentum):
    """thresholds[k] <- q_k + momentum * (thresholds[k] - q_k) IN PLACE on the device, q_k = the ceil(portion * n_k)-th largest conf among
    the n_k pixels whose class byte (labels & 0x7f) is k — exact, by radix selection (csrc/pseudo_label.hip).  A class
    without pixels keeps its threshold bit for bit.  -> q float32 [ncls], NaN for a class without pixels.  Stream-ordered, no host read."""
    lib = _lib.load()
    pc, pt = _p(conf), _p(thresholds)
    if not labels.is_cuda or labels.dtype != torch.uint8 or not labels.is_contiguous() or labels.numel() != conf.numel():
        raise _lib.PnpError("pseudo_label_update: labels must be a contiguous CUDA uint8 tensor with one byte per entry of conf")
    ncls, P = thresholds.numel(), conf.numel()
    q = torch.empty(ncls, dtype=torch.float32, device=conf.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = workspace(lib.pnp_pseudo_label_update_workspace_bytes(P, ncls), conf.device)      # histograms and selection state of the rounds
    check(lib.pnp_pseudo_label_update(vp(labels), pc, P, ncls, float(portion), float(momentum), pt, _p(q), vp(ws), ws.numel(), _stream()),
          "pnp_pseudo_label_update")
    return q


def fda_amplitude_swap(src, tgt, band, pair, out=None):
    """Fourier domain adaptation (csrc/fda.hip): src [B, H, W, C] keeps the phase of every channel's 2-D spectrum and takes
    the amplitude of tgt[pair[i]] ([Bt, H, W, C]) on the square |u|, |v| <= band[i] of low frequencies; band[i] = -1 leaves sample i as it
    is, bit for bit.  band, pair: B host integers each (sequences, numpy arrays or CPU tensors), checked by the library.  out: None (a new
    tensor), src itself (in place) or a tensor that overlaps neither input.  -> out.  Stream-ordered, bit-identical from run to run."""
    import numpy as np
    lib = _lib.load()
    ps, pt = _p(src), _p(tgt)
    if src.dim() != 4 or tgt.dim() != 4 or tuple(tgt.shape[1:]) != tuple(src.shape[1:]):
        raise _lib.PnpError("fda_amplitude_swap: src [B, H, W, C] and tgt [Bt, H, W, C] of one image size, got %s and %s"
                            % (tuple(src.shape), tuple(tgt.shape)))
    B, H, W, C = src.shape
    bd = np.ascontiguousarray(np.asarray(band, dtype=np.int64).reshape(-1))
    pr = np.ascontiguousarray(np.asarray(pair, dtype=np.int64).reshape(-1))
    if bd.shape != (B,) or pr.shape != (B,):
        raise _lib.PnpError("fda_amplitude_swap: %d bands and %d pairs for %d samples" % (bd.size, pr.size, B))
    if B and (np.abs(bd).max() >= 2 ** 31 or np.abs(pr).max() >= 2 ** 31):
        raise _lib.PnpError("fda_amplitude_swap: band or pair out of the int32 range")
    bd, pr = bd.astype(np.int32), pr.astype(np.int32)
    y = torch.empty_like(src) if out is None else out
    po = _p(y)
    if tuple(y.shape) != tuple(src.shape):
        raise _lib.PnpError("fda_amplitude_swap: out has shape %s, src %s" % (tuple(y.shape), tuple(src.shape)))
    need = lib.pnp_fda_workspace_bytes(B, tgt.shape[0], H, W, C, int(bd.max()) if B else -1)
    ws = workspace(need, src.device, slot="fda")
    check(lib.pnp_fda_amplitude_swap(ps, B, pt, tgt.shape[0], H, W, C, bd.ctypes.data_as(ctypes.c_void_p), pr.ctypes.data_as(ctypes.c_void_p),
                                     po, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()), "pnp_fda_amplitude_swap")
    return y


def filled(shape, value, device):
    t = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.load().pnp_fill(_p(t), t.numel(), float(value), _stream()), "pnp_fill")
    return t


# ---- training input from resident volumes (csrc/augment.hip, volume_source.py) -------------------------------------------------------
def volume_preprocess(v, percentile=98, out=None):
    """pnp_volume_preprocess of a float32 CUDA tensor (any shape, finite values): clip at the exact order statistic
    k = (percentile * (n - 1) + 99) // 100, z-score with the population std -> (normalised tensor, float64 [4] device tensor: clip, mean,
    std, normalised minimum).  out=v normalises in place.  Stream-ordered, no host synchronisation."""
    pv = _p(v)
    out = torch.empty_like(v) if out is None else out
    stats = torch.empty(4, dtype=torch.float64, device=v.device)
    lib = _lib.load()
    n = v.numel()
    need = lib.pnp_volume_preprocess_workspace_bytes(n)
    ws = workspace(need, v.device, slot="augment")
    check(lib.pnp_volume_preprocess(pv, _p(out), n, int(percentile), ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                    ws.numel(), _stream()), "pnp_volume_preprocess")
    return out, stats


def label_frame_stats(label, ncls):
    """pnp_label_frame_stats of a contiguous uint8 CUDA label volume [X, Y, Z] (any storage offset: a misaligned base is
    served) -> int32 [Z, ncls, 5] on the device: per frame z and class c in [0, ncls) the voxel count and the bounding box (xmin, xmax, ymin,
    ymax) of the voxels of frame z with label c; (0, X, -1, Y, -1) for a class absent from the frame.  Stream-ordered, no host
    synchronisation, no workspace."""
    if not label.is_cuda:
        raise _lib.PnpError("label_frame_stats: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    if label.dtype != torch.uint8 or label.dim() != 3 or not label.is_contiguous():
        raise _lib.PnpError("label_frame_stats: a contiguous uint8 volume [X, Y, Z] expected, got %s %s contiguous=%s"
                            % (label.dtype, tuple(label.shape), label.is_contiguous()))
    X, Y, Z = (int(d) for d in label.shape)
    ncls = int(ncls)
    if not 1 <= ncls <= 8 or Z < 1:              # before the table is sized from them
        raise _lib.PnpError("label_frame_stats: ncls = %d outside [1, 8] or an empty volume %s" % (ncls, (X, Y, Z)))
    stats = torch.empty((Z, ncls, 5), dtype=torch.int32, device=label.device)
    check(_lib.load().pnp_label_frame_stats(_u8p(label), X, Y, Z, ncls, ctypes.c_void_p(stats.data_ptr()), _stream()),
          "pnp_label_frame_stats")
    return stats


def _flat_f32_volume(v, what):
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise _lib.PnpError("%s: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback" % what)
    if v.dtype != torch.float32 or not v.is_contiguous() or v.numel() < 1:
        raise _lib.PnpError("%s: a non-empty contiguous float32 tensor expected, got %s %s contiguous=%s"
                            % (what, v.dtype, tuple(v.shape), v.is_contiguous()))
    return v


def _check_nbins(nbins, what):
    if isinstance(nbins, bool) or int(nbins) != nbins or not 2 <= int(nbins) <= 1024:
        raise _lib.PnpError("%s: nbins = %r outside [2, 1024]" % (what, nbins))
    return int(nbins)


def volume_histogram_packed(v, nbins=256):
    """pnp_volume_histogram into ONE int32 device buffer of 2 + nbins words, so that one copy brings both results to the
    host: words 0:2 are the bits of the float32 (lo, hi) = (min v, max v), words 2: the voxel count per bin (< 2^31 each)"""
    _flat_f32_volume(v, "volume_histogram")
    nbins = _check_nbins(nbins, "volume_histogram")
    buf = torch.empty(2 + nbins, dtype=torch.int32, device=v.device)
    check(_lib.load().pnp_volume_histogram(_p(v), v.numel(), nbins, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 8),
                                           _stream()), "pnp_volume_histogram")
    return buf


def volume_histogram(v, nbins=256):
    """pnp_volume_histogram of a contiguous float32 CUDA tensor of finite values (any shape, any storage offset) ->
    (range: float32 [2] = (min, max), bit-exact; hist: int32 [nbins], the voxel count of bin
    min(nbins - 1, int((v - lo) * (float32(nbins) / (hi - lo)))) in float32 round-to-nearest operations; a constant tensor counts in bin 0).
    Both are views of one device buffer.  Stream-ordered, no host synchronisation, no workspace; bit-identical from run to run."""
    buf = volume_histogram_packed(v, nbins)
    return buf[:2].view(torch.float32), buf[2:]


def volume_threshold_mask(v, range, k, nbins=256, out=None):
    """pnp_volume_threshold_mask: uint8 tensor of v's shape, 1 where the bin of v (volume_histogram's, with `range` = its
    float32 [2] device tensor, read on the device) is above k, 0 elsewhere; all zeros for a constant tensor.  out: a contiguous uint8 CUDA
    tensor of v's shape to write into.  Stream-ordered, no host synchronisation."""
    _flat_f32_volume(v, "volume_threshold_mask")
    nbins = _check_nbins(nbins, "volume_threshold_mask")
    if not isinstance(range, torch.Tensor) or not range.is_cuda or range.dtype != torch.float32 or range.numel() != 2 or not range.is_contiguous():
        raise _lib.PnpError("volume_threshold_mask: range must be volume_histogram's float32 [2] CUDA tensor")
    if isinstance(k, bool) or int(k) != k or not 0 <= int(k) <= nbins - 1:
        raise _lib.PnpError("volume_threshold_mask: k = %r outside [0, %d]" % (k, nbins - 1))
    if out is None:
        out = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
    elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != tuple(v.shape) or not out.is_contiguous():
        raise _lib.PnpError("volume_threshold_mask: out must be a contiguous uint8 CUDA tensor of shape %s" % (tuple(v.shape),))
    check(_lib.load().pnp_volume_threshold_mask(_p(v), v.numel(), _p(range), nbins, int(k), _u8p(out), _stream()), "pnp_volume_threshold_mask")
    return out


def volume_smooth(v, weights, out=None):
    """pnp_volume_smooth of a contiguous float32 CUDA volume [X, Y, Z]: weights = (wx, wy, wz), each None (the axis is not
    filtered) or 2 r + 1 float32-convertible taps, r <= 32 (volume_source.gaussian_weights); borders replicated.  out=None: a new tensor;
    out=v: in place.  Stream-ordered, no host synchronisation; the workspace (at most one volume, slot "smooth") stays cached until
    drop_workspace("smooth")."""
    import numpy as np
    if v.dim() != 3:
        raise _lib.PnpError("volume_smooth: a volume [X, Y, Z] expected, got %s" % (tuple(v.shape),))
    pv = _p(v)
    out = torch.empty_like(v) if out is None else out
    if tuple(out.shape) != tuple(v.shape):
        raise _lib.PnpError("volume_smooth: out is %s, the volume %s" % (tuple(out.shape), tuple(v.shape)))
    if len(weights) != 3:
        raise _lib.PnpError("volume_smooth: three weight vectors (or None) expected, got %d" % len(weights))
    taps, ptrs, radii = [], [], []
    for a, w in enumerate(weights):
        if w is None:
            ptrs.append(None)
            radii.append(0)
            continue
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.ndim != 1 or w.size % 2 != 1:
            raise _lib.PnpError("volume_smooth: axis %d: 2 r + 1 weights expected, got shape %s" % (a, w.shape))
        taps.append(w)                      # alive until the call returns
        ptrs.append(w.ctypes.data_as(ctypes.c_void_p))
        radii.append(w.size // 2)
    X, Y, Z = (int(d) for d in v.shape)
    lib = _lib.load()
    need = lib.pnp_volume_smooth_workspace_bytes(X, Y, Z, *radii)
    ws = workspace(need, v.device, slot="smooth") if need else None
    check(lib.pnp_volume_smooth(pv, _p(out), X, Y, Z, ptrs[0], radii[0], ptrs[1], radii[1], ptrs[2], radii[2],
                                None if ws is None else ctypes.c_void_p(ws.data_ptr()), 0 if ws is None else ws.numel(), _stream()),
          "pnp_volume_smooth")
    return out


def drop_workspace(slot):
    """forget the cached scratch buffers of `slot` (every device and stream): the allocator gets them back in stream order"""
    for key in [k for k in _ws_cache if k[1] == slot]:
        del _ws_cache[key]


def aug_slices(vols_host, vols_dev, nvol, samples_dev, B, H, W, errors, ncls=0, want_onehot=True, entry="pnp_aug_slices"):
    """pnp_aug_slices: vols_host (ctypes array of _lib.AugVolume) / vols_dev (its device copy, uint8 tensor), samples_dev (device copy of B
    _lib.AugSample records, uint8 tensor), errors (int32 [1] device counter) -> (x [B,H,W,3], label [B,H,W], one-hot [B,H,W,ncls] or None)"""
    dev = vols_dev.device
    if not (vols_dev.is_cuda and samples_dev.is_cuda and errors.is_cuda):
        raise _lib.PnpError("aug_slices: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    if samples_dev.numel() * samples_dev.element_size() != int(B) * ctypes.sizeof(_lib.AugSampleZ if entry == "pnp_aug_slices_z" else _lib.AugSample):
        raise _lib.PnpError("%s: the sample table holds %d bytes, not B = %d records" % (entry, samples_dev.numel() * samples_dev.element_size(), B))
    x = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    label = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    onehot = torch.empty((B, H, W, int(ncls)), dtype=torch.float32, device=dev) if want_onehot else None
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(getattr(_lib.load(), entry)(ctypes.cast(vols_host, ctypes.c_void_p), vp(vols_dev), int(nvol), vp(samples_dev), int(B), int(H), int(W),
                                      _p(x), _p(label), _p(onehot), int(ncls), vp(errors), _stream()), entry)
    return x, label, onehot


def aug_slices_z(vols_host, vols_dev, nvol, samples_dev, B, H, W, errors, ncls=0, want_onehot=True):
    """pnp_aug_slices_z: aug_slices with samples_dev holding B _lib.AugSampleZ records — any centre frame, the outer
    channels at frame -+ dz (fractional, clamped at the ends), volumes of one frame or more"""
    return aug_slices(vols_host, vols_dev, nvol, samples_dev, B, H, W, errors, ncls, want_onehot, entry="pnp_aug_slices_z")


def aug_slices_warp(vols_host, vols_dev, nvol, samples_dev, ctrl_dev, G, B, H, W, errors, ncls=0, want_onehot=True):
    """pnp_aug_slices_warp: aug_slices_z with samples_dev holding B _lib.AugSampleW records (gain, bias, noise, seed, warp
    after AugSampleZ's fields) and ctrl_dev the control points [B, G + 3, G + 3, 2] float32 of the samples' B-spline displacements in
    source voxels (None with G == 0: no sample may ask for a warp)"""
    dev = vols_dev.device
    if not (vols_dev.is_cuda and samples_dev.is_cuda and errors.is_cuda and (ctrl_dev is None or ctrl_dev.is_cuda)):
        raise _lib.PnpError("aug_slices_warp: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    if samples_dev.numel() * samples_dev.element_size() != int(B) * ctypes.sizeof(_lib.AugSampleW):
        raise _lib.PnpError("pnp_aug_slices_warp: the sample table holds %d bytes, not B = %d records"
                            % (samples_dev.numel() * samples_dev.element_size(), B))
    if ctrl_dev is not None:
        want = int(B) * (int(G) + 3) ** 2 * 2
        if ctrl_dev.dtype != torch.float32 or not ctrl_dev.is_contiguous() or ctrl_dev.numel() != want:
            raise _lib.PnpError("pnp_aug_slices_warp: the control table must be contiguous float32 [B, G + 3, G + 3, 2] = %d values for B = %d, "
                                "G = %d, got %s %s" % (want, B, G, ctrl_dev.dtype, tuple(ctrl_dev.shape)))
    x = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    label = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    onehot = torch.empty((B, H, W, int(ncls)), dtype=torch.float32, device=dev) if want_onehot else None
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(_lib.load().pnp_aug_slices_warp(ctypes.cast(vols_host, ctypes.c_void_p), vp(vols_dev), int(nvol), vp(samples_dev),
                                          None if ctrl_dev is None else vp(ctrl_dev), int(G), int(B), int(H), int(W), _p(x), _p(label),
                                          _p(onehot), int(ncls), vp(errors), _stream()), "pnp_aug_slices_warp")
    return x, label, onehot


# ---- volume inference (csrc/paste.hip, volume_predict.py) -------------------------------------------------------------------------------
def paste_labels(logits, nb, z0, inv, src_xy, vol, origin, strides, fov=False):
    """fov=True: pnp_paste_labels_fov — a voxel column whose plane coordinates leave [-0.5, H - 0.5] x [-0.5, W - 0.5] is
    not written; otherwise
    pnp_paste_labels: logits [B, H, W, ncls] -> one label byte per (x < X, y < Y, b < nb) at vol.view(-1)[origin + x sx + y sy + (z0 + b) sz].
    inv: the six float32 entries of the map from a source voxel to output-plane coordinates (host); vol: a contiguous uint8 CUDA tensor (the
    whole allocation the offsets are checked against); strides = (sx, sy, sz) in elements, any sign.  Stream-ordered, returns vol."""
    if logits.dim() != 4:
        raise _lib.PnpError("paste_labels: logits must be [B, H, W, ncls], got %s" % (tuple(logits.shape),))
    if not vol.is_cuda or vol.dtype != torch.uint8 or not vol.is_contiguous():
        raise _lib.PnpError("paste_labels: vol must be a contiguous uint8 CUDA tensor (got %s %s) — there is no CPU fallback" % (vol.device, vol.dtype))
    B, H, W, ncls = (int(d) for d in logits.shape)
    m = (ctypes.c_float * 6)(*[float(v) for v in inv])
    entry = "pnp_paste_labels_fov" if fov else "pnp_paste_labels"
    check(getattr(_lib.load(), entry)(_p(logits), B, H, W, ncls, int(nb), int(z0), m, int(src_xy[0]), int(src_xy[1]),
                                      ctypes.c_void_p(vol.data_ptr()), vol.numel(), int(origin), int(strides[0]), int(strides[1]),
                                      int(strides[2]), _stream()), entry)
    return vol


def _paste_soft_args(who, logits, invs, nb, z0, src_xy, vol, origin, strides, prob, entropy):
    """what paste_ensemble and paste_tiles share: the checks of the member and output tensors, in the order the calls are refused in, and
    the arguments of the entry points -> ((B, H, W, ncls), member pointers, maps, the arguments from nb on).  No member: the shape is
    (1, 1, 1, 1) and the outputs are not looked at — M = 0 is the caller's or the library's refusal, before anything is read."""
    shape = tuple(logits[0].shape) if logits else (1, 1, 1, 1)
    for t in logits:
        if t.dim() != 4 or tuple(t.shape) != shape:
            raise _lib.PnpError("%s: every member must be [B, H, W, ncls] of one shape, got %s and %s" % (who, shape, tuple(t.shape)))
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.PnpError("%s: logits must be contiguous float32 CUDA tensors (got %s %s) — there is no CPU fallback" % (who, t.device, t.dtype))
    if not vol.is_cuda or vol.dtype != torch.uint8 or not vol.is_contiguous():
        raise _lib.PnpError("%s: vol must be a contiguous uint8 CUDA tensor (got %s %s) — there is no CPU fallback" % (who, vol.device, vol.dtype))
    dims = tuple(int(d) for d in shape)
    for name, t, n in (("prob", prob, dims[3] * vol.numel()), ("entropy", entropy, vol.numel())) if logits else ():
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
            raise _lib.PnpError("%s: %s must be a contiguous float32 CUDA tensor of %d elements (got %s %s, %d) — there is no CPU fallback"
                                % (who, name, n, t.device, t.dtype, t.numel()))
    M = len(logits)
    ptrs = (ctypes.c_void_p * M)(*[t.data_ptr() for t in logits])
    m = (ctypes.c_float * (6 * M))(*[float(v) for inv in invs for v in inv])
    tail = (int(nb), int(z0), int(src_xy[0]), int(src_xy[1]), ctypes.c_void_p(vol.data_ptr()), vol.numel(), int(origin), int(strides[0]),
            int(strides[1]), int(strides[2]), _p(prob), _p(entropy), _stream())
    return dims, ptrs, m, tail


def paste_ensemble(logits, nb, z0, invs, src_xy, vol, origin, strides, prob=None, entropy=None, fov=False):
    """fov=True: pnp_paste_ensemble_fov — a voxel column that any member's map takes outside its plane is written in none
    of vol, prob, entropy; otherwise
    pnp_paste_ensemble: M = len(logits) members, each [B, H, W, ncls] float32 (a tensor may repeat), invs: one six-entry map per member
    (host) -> per (x < X, y < Y, b < nb) at e = origin + x sx + y sy + (z0 + b) sz: vol.view(-1)[e] = the first strict maximum of the
    members' summed softmax of the interpolated logits, prob.view(ncls, -1)[c, e] = the mean probability (prob: contiguous float32,
    ncls * vol.numel() elements, or None), entropy.view(-1)[e] = the entropy normalised by log(ncls) (contiguous float32 of vol.numel()
    elements, or None).  Stream-ordered, returns (vol, prob, entropy)."""
    logits = list(logits)
    if not logits or len(invs) != len(logits):
        raise _lib.PnpError("paste_ensemble: %d members with %d maps" % (len(logits), len(invs)))
    dims, ptrs, m, tail = _paste_soft_args("paste_ensemble", logits, invs, nb, z0, src_xy, vol, origin, strides, prob, entropy)
    if len(m) != 6 * len(logits):
        raise _lib.PnpError("paste_ensemble: every map has six entries")
    entry = "pnp_paste_ensemble_fov" if fov else "pnp_paste_ensemble"
    check(getattr(_lib.load(), entry)(len(logits), ptrs, m, *dims, *tail), entry)
    return vol, prob, entropy


def paste_tiles(logits, nb, z0, invs, ramp, src_xy, vol, origin, strides, prob=None, entropy=None):
    """pnp_paste_tiles: paste_ensemble's arguments for M = len(logits) <= 64 members that each cover a part of the box, and
    `ramp` >= 1, the width of the blending window's rise in plane pixels.  A voxel column is written iff at least one member's map keeps
    it inside its plane; over the covering members vol gets the first strict maximum of the window-weighted softmax sum, prob the weighted
    mean probabilities, entropy their normalised entropy.  Stream-ordered, returns (vol, prob, entropy)."""
    logits = list(logits)
    if len(invs) != len(logits):
        raise _lib.PnpError("paste_tiles: %d members with %d maps" % (len(logits), len(invs)))
    if any(len(inv) != 6 for inv in invs):
        raise _lib.PnpError("paste_tiles: every map has six entries")
    dims, ptrs, m, tail = _paste_soft_args("paste_tiles", logits, invs, nb, z0, src_xy, vol, origin, strides, prob, entropy)
    check(_lib.load().pnp_paste_tiles(len(logits), ptrs, m, float(ramp), *dims, *tail), "pnp_paste_tiles")
    return vol, prob, entropy


def fuse_views(probs, weights=None, label=None, prob=None, entropy=None):
    """pnp_fuse_views: probs = 1 .. 8 contiguous float32 CUDA tensors [ncls, ...] of one shape (the probability volumes
    of the views of one scan, class-major as paste_ensemble writes them), weights: None or one positive finite number per view (host).
    Per voxel, over the views whose probabilities sum to more than 0.5 there: label = the first strict maximum of the weighted mean
    probabilities, prob = that mean, entropy = its normalised entropy; a voxel no view covers gets 0 in all three.
    label: a contiguous uint8 CUDA tensor of the voxel count (None: a new one of the views' spatial shape); prob / entropy: True = a new
    tensor, a tensor = written in place (prob may be probs[0] itself; any other overlap is refused), None / False = not computed.  Every
    element of the outputs is written.  Stream-ordered, returns (label, prob, entropy)."""
    probs = list(probs)
    M = len(probs)
    if M == 0:                                                  # the library's refusal (as M > 8 is), before anything is read
        check(_lib.load().pnp_fuse_views(0, None, None, 1, 1, None, None, None, None), "pnp_fuse_views")
    shape = tuple(probs[0].shape)
    for t in probs:
        if not torch.is_tensor(t) or t.dim() < 2 or tuple(t.shape) != shape:
            raise _lib.PnpError("fuse_views: every view must be [ncls, ...] of one shape, got %s and %s" % (shape, tuple(getattr(t, "shape", ()))))
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.PnpError("fuse_views: views must be contiguous float32 CUDA tensors (got %s %s) — there is no CPU fallback" % (t.device, t.dtype))
    ncls = int(shape[0])
    elems = 1
    for d in shape[1:]:
        elems *= int(d)
    if weights is not None and len(weights) != M:
        raise _lib.PnpError("fuse_views: %d weights for %d views" % (len(weights), M))
    dev = probs[0].device
    if label is None:
        label = torch.empty(shape[1:], dtype=torch.uint8, device=dev)
    prob = torch.empty(shape, dtype=torch.float32, device=dev) if prob is True else None if prob is False else prob
    entropy = torch.empty(shape[1:], dtype=torch.float32, device=dev) if entropy is True else None if entropy is False else entropy
    if not torch.is_tensor(label) or not label.is_cuda or label.dtype != torch.uint8 or not label.is_contiguous() or label.numel() != elems:
        raise _lib.PnpError("fuse_views: label must be a contiguous uint8 CUDA tensor of %d elements (got %s %s, %d) — there is no CPU fallback"
                            % (elems, label.device, label.dtype, label.numel()))
    for name, t, n in (("prob", prob, ncls * elems), ("entropy", entropy, elems)):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
            raise _lib.PnpError("fuse_views: %s must be a contiguous float32 CUDA tensor of %d elements (got %s %s, %d) — there is no CPU fallback"
                                % (name, n, t.device, t.dtype, t.numel()))
    ptrs = (ctypes.c_void_p * M)(*[t.data_ptr() for t in probs])
    w = None if weights is None else (ctypes.c_float * M)(*[float(v) for v in weights])
    check(_lib.load().pnp_fuse_views(M, ptrs, w, ncls, elems, ctypes.c_void_p(label.data_ptr()), _p(prob), _p(entropy), _stream()),
          "pnp_fuse_views")
    return label, prob, entropy


# ---- connected components of label volumes (csrc/components.hip, components.py) ------------------------------------------------------------
def _components_ws(vol):
    D0, D1, D2 = (int(d) for d in vol.shape)
    lib = _lib.load()
    need = lib.pnp_components_workspace_bytes(D0, D1, D2)
    if need == 0:
        raise _lib.PnpError("components: unsupported volume %s (each extent in [1, 4096], fewer than 2^31 voxels)" % ((D0, D1, D2),))
    return lib, (D0, D1, D2), workspace(need, vol.device, slot="components")


def components_errors(ws):
    """the two device error counters at the head of a components workspace (label, filter): one host read"""
    e = ws[:8].view(torch.int32).cpu()
    return int(e[0]), int(e[1])


def label_components(vol, ncls, connectivity=1):
    """pnp_label_components of a contiguous uint8 [D0, D1, D2] CUDA tensor -> (roots int32 [D0, D1, D2], the workspace: its head holds the
    error counters, components_errors).  Stream-ordered."""
    lib, (D0, D1, D2), ws = _components_ws(vol)
    roots = torch.empty(tuple(vol.shape), dtype=torch.int32, device=vol.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.pnp_label_components(vp(vol), D0, D1, D2, int(ncls), int(connectivity), vp(roots), vp(ws), ws.numel(), _stream()),
          "pnp_label_components")
    return roots, ws


def filter_components(vol, roots, ncls, class_mask, keep, min_size, out):
    """pnp_filter_components: vol / roots as label_components takes / returns them, out a uint8 tensor of vol's shape (vol itself filters
    in place) -> (out, stats int64 [ncls, 4], the workspace).  Stream-ordered."""
    lib, (D0, D1, D2), ws = _components_ws(vol)
    stats = torch.empty((int(ncls), 4), dtype=torch.int64, device=vol.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.pnp_filter_components(vp(vol), vp(roots), D0, D1, D2, int(ncls), int(class_mask), int(keep), int(min_size), vp(out), vp(stats),
                                    vp(ws), ws.numel(), _stream()), "pnp_filter_components")
    return out, stats, ws


def fill_holes_errors(ws):
    """the three device error counters of a fill workspace (labelling, size count, fill): one host read"""
    e = ws[:1032].cpu()
    a, b = e[:8].view(torch.int32), e[1024:1032].view(torch.int32)
    return int(a[0]), int(a[1]), int(b[0])


def fill_holes(vol, ncls, class_mask, max_size, out):
    """pnp_fill_holes: vol a contiguous uint8 [D0, D1, D2] CUDA tensor, out a uint8 tensor of vol's shape (vol itself fills in place)
    -> (out, stats int64 [ncls, 4], the workspace: its head holds the error counters, fill_holes_errors).  Stream-ordered."""
    D0, D1, D2 = (int(d) for d in vol.shape)
    lib = _lib.load()
    need = lib.pnp_fill_holes_workspace_bytes(D0, D1, D2, int(ncls))
    if need == 0:
        raise _lib.PnpError("fill_holes: unsupported volume %s or ncls %d (each extent in [1, 4096], fewer than 2^31 voxels, ncls in [2, 8])"
                            % ((D0, D1, D2), int(ncls)))
    ws = workspace(need, vol.device, slot="components")
    stats = torch.empty((int(ncls), 4), dtype=torch.int64, device=vol.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.pnp_fill_holes(vp(vol), D0, D1, D2, int(ncls), int(class_mask), int(max_size), vp(out), vp(stats), vp(ws), ws.numel(), _stream()),
          "pnp_fill_holes")
    return out, stats, ws
