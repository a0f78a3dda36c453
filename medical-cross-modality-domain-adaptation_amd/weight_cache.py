"""What is derived from a convolution filter and kept between launches, and the one answer to "is it still true".

Two artefacts hang off one record per filter, keyed by (data_ptr, shape):
  "shadows"    the bf16 pair (w_io, w_oi) the bf16-resident kernels read, with the recording token it was last cast under;
  ("U", kind)  the buffer lent to the library for the Winograd transform U = G g G^T of pass `kind` (0 forward, 1 data gradient), or
               None where the route has not taken the layer yet.  Only filters a VariableStore owns (their tensors carry `_pnp_var`).

IDENTITY (`WeightCache.record`): a record stands for the filter it was made for while its owner object is the same and the torch version
counter has not moved; a new tensor on a recycled address is another filter.  When either fails, everything derived is invalidated in
that one place: the shadows are stamped NEVER, and the library is told the filter's byte range if it holds a lent buffer.
STALENESS (`WeightCache.stale`): after identity, the write log — has a reported write touched the filter's bytes since the artefact was
filled — and for shadows the recording token.  A "not touched" answer is remembered by stamping the artefact with the current epoch, so
a frozen filter is scanned once per report, not once per read.  The library keeps U's validity itself from the same reports
(pnp_weights_changed clears its `valid` flag), so the U binding needs the identity rule only.

The owner is `w._base or w`.  Measured on CPU tensors the way VariableStore.finalize builds them: a TRAINABLE filter is
`arena[a:b].view(shape).detach()`, and detach() cuts `_base` (None, `_is_view()` False) while still sharing the arena's version counter —
its owner is the tensor itself and both former rules name the same object.  A FROZEN filter stays a plain view, its `_base` is the state
arena: the arena outlives the view, so the two are not equivalent.  The same tensor object implies the same `_base`, never the reverse.
The record therefore carries both: `owner` decides identity (a re-wrapped view of the same memory must still hit its shadows), `tensor`
is the marked object the U buffers were lent for — the mark lives on the object, so the bindings go when it dies or when any other
object turns up on its address.

No library import and no torch.cuda call happens at import time; the library handle arrives as an argument (`bind_u`) and is remembered
while something is lent, so all of this runs on CPU tensors against a stand-in library.
"""
import contextlib
import ctypes
import weakref

import torch

SHADOW_RECORDS_MAX, U_BINDINGS_MAX = 1024, 4096     # eviction (WeightCache.report): leftovers of stores that no longer exist (test suites)
LOG_MAX = 64                                        # ranged reports kept before the floor moves
NEVER = -1                                          # an epoch older than every floor


class WriteLog(object):
    """reported weight writes: an epoch per report, the byte ranges [lo, hi) of the range-limited ones since `floor`, oldest first; a
    write of unknown extent (or a 65th pending record) moves the floor: everything filled before it is stale"""

    def __init__(self):
        self.epoch, self.floor, self.pending = 0, 0, []

    def report(self, ranges=None):
        self.epoch += 1
        if ranges is None or len(self.pending) >= LOG_MAX:
            del self.pending[:]
            self.floor = self.epoch
        else:
            self.pending.append((self.epoch, tuple((int(lo), int(hi)) for lo, hi in ranges)))

    def touched(self, since_epoch, lo, hi):
        """has a reported write touched [lo, hi) after `since_epoch`"""
        if since_epoch < self.floor:
            return True
        for ep, rs in reversed(self.pending):
            if ep <= since_epoch:
                break
            for a, b in rs:
                if a < hi and lo < b:
                    return True
        return False


class Record(object):
    """one filter: key (data_ptr, shape), weakrefs to its owner and to the marked tensor its U buffers were lent for (None: none), the
    torch version last seen, and arts: name -> [epoch filled at, recording token, *buffers]"""
    __slots__ = ("key", "nbytes", "owner", "tensor", "version", "arts")


class WeightCache(object):
    def __init__(self):
        self.log, self.records = WriteLog(), {}
        self.token, self.pins = None, 0        # the hipGraph recording in progress; live recorded steps (their graphs hold shadow ADDRESSES)
        self.lib = None                        # the library something was lent to
        self.n_shadows = self.n_u = 0          # records with shadows; ("U", kind) artefacts, lent or not
        self.casts = 0                         # pnp_filter_bf16 calls made for shadows (tests, profiling)

    # ---- the two rules -------------------------------------------------------------------------------------------------------------
    def record(self, w):
        """identity rule -> the record of `w`, made or re-owned as needed"""
        key = (w.data_ptr(), tuple(w.shape))
        owner = w._base if w._base is not None else w
        rec = self.records.get(key)
        if rec is None:
            rec = self.records[key] = Record()
            rec.key, rec.nbytes, rec.owner, rec.tensor, rec.version, rec.arts = key, 4 * w.numel(), weakref.ref(owner), None, w._version, {}
            return rec
        if rec.tensor is not None and rec.tensor() is not w:      # lent for another object: the library must not serve the old U
            self._withdraw(rec)
        same = rec.owner() is owner
        if not same or rec.version != w._version:
            if same and rec.tensor is not None and any(a[2] is not None for n, a in rec.arts.items() if n != "shadows"):
                # written by a torch op: exactly the filter's own bytes
                self.lib.pnp_weights_changed(ctypes.c_void_p(key[0]), ctypes.c_void_p(key[0] + rec.nbytes))
            rec.owner, rec.version = weakref.ref(owner), w._version
            if "shadows" in rec.arts:
                rec.arts["shadows"][0] = NEVER
        return rec

    def stale(self, rec, art, token=None):
        """staleness rule for an artefact of a record that record() has just returned"""
        if art[1] is not token:
            return True
        if art[0] != self.log.epoch:
            if self.log.touched(art[0], rec.key[0], rec.key[0] + rec.nbytes):
                return True
            art[0] = self.log.epoch            # not touched: do not scan again before the next report
        return False

    # ---- bf16 shadows --------------------------------------------------------------------------------------------------------------
    def shadows(self, w, cast):
        """(w_io, w_oi) of an fp32 filter [R,S,C,K]; cast(w, None) -> a new pair, cast(w, pair) refreshes in place (same buffers: no
        allocation in the steady state, and a recorded step keeps their addresses)"""
        rec = self.record(w)
        art = rec.arts.get("shadows")
        # While a hipGraph is being recorded the cast is ALWAYS taken once per recording: a shadow that happens to be fresh at capture
        # time would leave its cast out of the graph, and every replay would read the copy of whatever the filter held when it was
        # recorded.  (Once: the token names the recording; a second read in it follows the ordinary rule.  No token: every read casts.)
        # The other way round, a cast that was only RECORDED has not run: outside that recording it counts as stale.
        token = (self.token if self.token is not None else object()) if torch.cuda.is_current_stream_capturing() else None
        if art is None or self.stale(rec, art, token):
            pair = cast(w, None if art is None else (art[2], art[3]))
            self.casts += 1
            self.n_shadows += art is None
            rec.arts["shadows"] = art = [self.log.epoch, token, pair[0], pair[1]]
        return art[2], art[3]

    # ---- transformed filters of the Winograd route ----------------------------------------------------------------------------------
    def bind_u(self, w, g, kind, lib):
        """before a launch of pass `kind` with geometry `g`: a store-owned filter gets one buffer per pass, lent to `lib` the first time
        the route takes the 3x3 layer; ad-hoc filters are never bound"""
        if not getattr(w, "_pnp_var", False):
            rec = self.records.get((w.data_ptr(), tuple(w.shape)))
            if rec is not None and rec.tensor is not None:       # an ad-hoc filter on a bound address
                self._withdraw(rec, forget=True)
            return
        rec = self.record(w)
        art = rec.arts.get(("U", kind))
        if art is not None and art[2] is not None:
            return
        on_route = g.R == 3 and g.S == 3 and lib.pnp_conv2d_wino_chosen(ctypes.byref(g), int(kind))
        if art is not None and not on_route:
            return
        # (an artefact without a buffer: the planner declined the layer when the filter was first seen — a small-batch forward, a policy
        # change; the route takes it NOW, so bind instead of leaving the cache off for the lifetime of the tensor)
        U = None
        nbytes = int(lib.pnp_conv2d_wino_filter_bytes(int(w.shape[2]), int(w.shape[3]))) if on_route else 0
        if nbytes:
            from ._lib import check
            U = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            check(lib.pnp_conv2d_wino_filter_bind(ctypes.c_void_p(rec.key[0]), int(kind), ctypes.c_void_p(U.data_ptr()), nbytes),
                  "pnp_conv2d_wino_filter_bind")
        self.lib = lib
        if rec.tensor is None:
            # the bindings go when the tensor object does (CPython frees it, and with it the arena it may keep alive, deterministically):
            # nothing allocated later on the same address can meet a valid entry
            rec.tensor = weakref.ref(w, lambda r, k=rec.key: self._died(k, r))
        self.n_u += art is None
        rec.arts[("U", kind)] = [self.log.epoch, None, U]

    def _died(self, key, ref):
        try:
            rec = self.records.get(key)
            if rec is not None and rec.tensor is ref:
                self._withdraw(rec, forget=True)
        except Exception:          # interpreter shutdown: the library and this module's globals may be gone already
            pass

    def _withdraw(self, rec, forget=False):
        """take back every buffer lent for `rec`; forget: drop the record too if nothing else hangs off it"""
        rec.tensor = None
        for name in [n for n in rec.arts if n != "shadows"]:
            if rec.arts.pop(name)[2] is not None:
                self.lib.pnp_conv2d_wino_filter_bind(ctypes.c_void_p(rec.key[0]), int(name[1]), None, 0)
            self.n_u -= 1
        if forget and not rec.arts:
            del self.records[rec.key]

    def clear_u(self):
        """withdraw every transformed-filter buffer (tests; a store that goes away)"""
        if self.n_u:
            self.lib.pnp_conv2d_wino_filter_bind(None, 0, None, 0)
            for rec in list(self.records.values()):
                rec.tensor = None
                rec.arts = {n: a for n, a in rec.arts.items() if n == "shadows"}
                if not rec.arts:
                    del self.records[rec.key]
            self.n_u = 0

    def bound(self, ptr):
        """the passes for which a filter at address `ptr` holds a U artefact"""
        return sorted(n[1] for rec in self.records.values() if rec.key[0] == ptr for n in rec.arts if n != "shadows")

    # ---- reports, recordings, bookkeeping -------------------------------------------------------------------------------------------
    def report(self, ranges=None):
        """weights were (or are queued to be) written: [(first byte address, end address), ...], None: everything"""
        self.log.report(ranges)
        if ranges is None and not self.pins and (self.n_shadows > SHADOW_RECORDS_MAX or self.n_u > U_BINDINGS_MAX):
            self.clear_u()                     # the one eviction rule: start over
            self.records.clear()
            self.n_shadows = 0
        elif self.n_u:
            for lo, hi in ([(None, None)] if ranges is None else ranges):
                self.lib.pnp_weights_changed(ctypes.c_void_p(lo), ctypes.c_void_p(hi))

    @contextlib.contextmanager
    def recording(self):
        """the hipGraph recording of one step: every filter shadow it reads is cast inside it, once"""
        self.token = object()
        try:
            yield self.token
        finally:
            self.token = None

    def pin(self):
        self.pins += 1

    def unpin(self):
        self.pins -= 1
        return self.pins

    def memory(self):
        """device bytes held: what kernels.memory_report adds to its workspaces"""
        nb = lambda t: 0 if t is None else int(t.numel()) * int(t.element_size())
        arts = [(n, a) for rec in self.records.values() for n, a in rec.arts.items()]
        return {"recorded_steps_alive": int(self.pins),
                "winograd_filters": sum(nb(a[2]) for n, a in arts if n != "shadows"), "winograd_filter_entries": self.n_u,
                "bf16_filter_shadows": sum(nb(a[2]) + nb(a[3]) for n, a in arts if n == "shadows"), "bf16_filter_entries": self.n_shadows}


CACHE = WeightCache()
