"""torch.autograd.Function wrappers over the C ABI (include/movae.h).

PyTorch supplies device memory, the stream and the autograd tape; every FLOP below runs in
libmovae_hip.so.  Activations are NHWC tensors of shape [N, H, W, C] (contiguous); conv weights
are the reference's parameter shapes ([Co,Ci,kh,kw] / [Ci,Co,kh,kw]) held in channels_last memory
so that `w.permute(0,2,3,1)` is the contiguous [.,kh,kw,.] image the kernels read.
"""
import ctypes as C
import os
import weakref

import torch
from torch.autograd import Function

from . import _lib as L


_call = L.call


def _knob(name, default="1"):
    """The A/B switch MOVAE_<name> of the environment: on unless set to "0" -- with default "0", off unless set to "1"."""
    v = os.environ.get("MOVAE_" + name, default)
    return v == "1" if default == "0" else v != "0"


class Destinations:
    """Where the results of ONE autograd call or one batched pull-back go, and with it what only one of a backward body's (`_run`)
    two callers does.  Two kinds, no subclasses: the engine's (engine=True) serves Function.backward (torch's engine: one cotangent,
    stacked as [1, ...], one row), the walker's serves backward_batched (autojac._batched_pullback: G cotangents, G = 1 included,
    one row per group).  The caller (autojac) builds one, installs it (`with d:`) around the call and reads its records afterwards.
      rows      per group {param data_ptr: flat slice}: the gradient is written there in place (a Jacobian row, a task-side
                parameter's buffer) -- consumed on first use, a second use of the same parameter gets a fresh buffer
      accum     {param data_ptr: its EXISTING gradient}: the weight-gradient kernels add into it (split-K reduce with accumulate)
                instead of writing a tensor that a torch add then folds in -- a task-side parameter an earlier loss already reached
      cot       {FEATURE data_ptr: slice i of a stacked [K, ...] buffer}: the op that produces d(loss i)/d(feature) (reparameterize,
                the KL term, ...) writes there, so the K cotangents of a feature are born stacked -- no torch.stack launch before
                the batched pull-back; an op that does not know about it simply returns its own buffer (and the stack copies)
      written, zeroed, taken   its records: data_ptr of every slice handed out for WRITING / as an untouched all-zero gradient, and
                of every parameter accumulated in place (autojac._accumulate checks what autograd hands back against it)
      engine    the engine takes the entry points of one cotangent (movae_act_bwd, movae_bn_act_bwd) where the walker takes the
                grouped ones: the caller's choice, never G == 1's"""
    __slots__ = ("engine", "rows", "accum", "cot", "written", "zeroed", "taken", "prev")

    def __init__(self, engine, rows=(), accum=None, cot=None, written=None):
        self.engine, self.rows, self.accum, self.cot = engine, rows, accum or {}, cot or {}
        self.written, self.zeroed, self.taken = [] if written is None else written, [], set()

    def __enter__(self):
        global _INSTALLED
        self.prev, _INSTALLED = _INSTALLED, self
        return self

    def __exit__(self, *exc):
        global _INSTALLED
        _INSTALLED = self.prev
        return False

    def _registered(self, g, param, shape, record):
        """Group g's sink registered for `param` (consumed, and its data_ptr recorded), or None."""
        row = self.rows[g] if self.rows else None
        dst = row.pop(param.data_ptr(), None) if row else None
        if dst is not None and dst.numel() == param.numel():
            record.append(dst.data_ptr())
            return dst.view(shape)
        return None

    def sink(self, g, param, shape):
        """Destination of group g's gradient of `param`: the registered sink, else a fresh buffer."""
        dst = self._registered(g, param, shape, self.written)
        return dst if dst is not None else torch.empty(shape, dtype=param.dtype, device=param.device)

    def sinks(self, G, param, shape):
        """([sink(g, ...) for the G groups], was every one of them a registered sink?)"""
        got = [self._registered(g, param, shape, self.written) for g in range(G)]
        sunk = all(d is not None for d in got)  # (`None not in got` would compare None with every tensor by ==: a torch dispatch each)
        return got if sunk else [torch.empty(shape, dtype=param.dtype, device=param.device) if d is None else d for d in got], sunk

    def zeros(self, g, param, shape):
        """An all-zero gradient: sinks are zero-initialised by their owner (autojac.JacobianBuffer) and written at most
        once, so a registered sink is returned untouched -- no fill launch.  Without a sink the walker gets a new zero tensor; the
        engine's parameter gets ONE persistent zero tensor for life, kept on the parameter itself (a bias in front of a
        training-mode BatchNorm: its gradient is identically zero, so whatever is accumulated into this tensor later is zero as
        well); nothing there launches a fill per step."""
        dst = self._registered(g, param, shape, self.zeroed)
        if dst is not None:
            return dst
        if not self.engine:
            return torch.zeros(shape, dtype=param.dtype, device=param.device)
        z = getattr(param, "_movae_zero_grad", None)
        if z is None or z.numel() != param.numel() or z.dtype != param.dtype or z.device != param.device:
            z = param._movae_zero_grad = torch.zeros(param.numel(), dtype=param.dtype, device=param.device)
        return z.view(shape)

    def accum_targets(self, w, b, need_b):
        """(dW destination in memory order, dbias destination) when BOTH of a layer's gradients can be accumulated in place, the
        engine's alone; else (None, None)."""
        if not self.accum or not self.engine:
            return None, None
        gw = self.accum.get(w.data_ptr())
        gb = self.accum.get(b.data_ptr()) if (b is not None and need_b) else None
        if gw is None or (b is not None and need_b and gb is None):
            return None, None
        v = gw.permute(0, 2, 3, 1) if gw.dim() == 4 else gw
        if not v.is_contiguous() or gw.shape != w.shape:
            return None, None
        for p in (w,) if gb is None else (w, b):
            self.accum.pop(p.data_ptr(), None)
            self.taken.add(p.data_ptr())
        return v, gb

    def cotangent(self, feature_ptr, like):
        """Destination for the gradient w.r.t. the tensor `like` (contiguous) whose memory the feature at `feature_ptr` views: the
        registered slice (consumed), seen with `like`'s shape (the feature may be a permuted view of the same memory -- logical NCHW
        over an NHWC buffer; the slice was allocated with the feature's strides, i.e. in that memory order), else a fresh buffer."""
        dst = self.cot.pop(feature_ptr, None) if self.cot else None
        if dst is not None and dst.numel() == like.numel() and dst.dtype == like.dtype and like.is_contiguous():
            if dst.shape == like.shape and dst.is_contiguous():
                return dst
            if sorted(zip(dst.stride(), dst.shape), reverse=True) == sorted(zip(like.stride(), like.shape), reverse=True):  # same memory order
                return dst.as_strided(like.shape, like.stride())
        return torch.empty_like(like)


#: the instance in scope (`with d:`), and what an op gets with none of its kind in scope: fresh buffers, the persistent zero, no
#: accumulation, nothing recorded
_INSTALLED = None
_NONE = {True: Destinations(True), False: Destinations(False)}


def installed(engine):
    """The Destinations in scope if it is of the asking kind, else the empty one of that kind: Function.backward asks for the
    engine's, backward_batched for the walker's.  The walker calls `backward` once per group on a node without `backward_batched`;
    that call must not see the walker's rows (it would write every group's gradient into row 0)."""
    d = _INSTALLED
    return d if d is not None and d.engine is engine else _NONE[engine]


def _stacked(t, G):
    """[G, ...] contiguous tensor from a stacked tensor or a list of G per-group tensors."""
    if isinstance(t, (list, tuple)):
        return torch.stack([_c(x) for x in t])
    return _c(t)


def _first(t):
    """Group 0 of a backward body's result (stacked tensor or per-group list), None staying None."""
    return t[0] if t is not None else None


def _ws(t):
    w = L.workspace(t.device)
    return w.data_ptr(), w.numel()


def _st(t):
    return L.stream_ptr(t.device)


def _c(t):
    """contiguous fp32 view/copy of an incoming gradient"""
    return t if t.is_contiguous() else t.contiguous()


def weight_mem(w):
    """[a, b, kh, kw] parameter -> contiguous [a, kh, kw, b] memory image (no copy when the
    parameter is channels_last, which is how nn.py creates it)."""
    v = w.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        v = v.contiguous()
    return v


def conv_out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def convT_out_size(h, k, s, p, op):
    return (h - 1) * s - 2 * p + k + op


# ---------------------------------------------------------------------------------------------
class NchwToNhwc(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(x)
        x = _c(x)
        n, c, h, w = x.shape
        y = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device)
        _call("movae_nchw_to_nhwc", x.data_ptr(), y.data_ptr(), n, c, h, w, _st(x))
        return y

    @staticmethod
    def _run(G, dy):
        _, n, h, w, c = dy.shape
        dx = torch.empty((G, n, c, h, w), dtype=dy.dtype, device=dy.device)
        _call("movae_nhwc_to_nchw", dy.data_ptr(), dx.data_ptr(), G * n, c, h, w, _st(dy))
        return dx

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None
        return NchwToNhwc._run(1, _c(dy).unsqueeze(0))[0]

    @staticmethod
    def backward_batched(ctx, G, dy):
        return (NchwToNhwc._run(G, _stacked(dy, G)),)


class NhwcToNchw(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(x)
        x = _c(x)
        n, h, w, c = x.shape
        y = torch.empty((n, c, h, w), dtype=x.dtype, device=x.device)
        _call("movae_nhwc_to_nchw", x.data_ptr(), y.data_ptr(), n, c, h, w, _st(x))
        return y

    @staticmethod
    def _run(G, dy):
        _, n, c, h, w = dy.shape
        dx = torch.empty((G, n, h, w, c), dtype=dy.dtype, device=dy.device)
        _call("movae_nchw_to_nhwc", dy.data_ptr(), dx.data_ptr(), G * n, c, h, w, _st(dy))
        return dx

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None
        return NhwcToNchw._run(1, _c(dy).unsqueeze(0))[0]

    @staticmethod
    def backward_batched(ctx, G, dy):
        return (NhwcToNchw._run(G, _stacked(dy, G)),)


_LAST_NHWC = [None]  # (weakref to the NCHW source, its version counter, data_ptr, capturing?, the NHWC copy)


def forget_nhwc():
    """Drop the remembered conversion (capture.capturing calls this around every capture: a result produced eagerly
    must not stand in for a launch the graph has to contain, and graph-pool memory must not leak into eager code)."""
    _LAST_NHWC[0] = None


def to_nhwc(x):
    """logical NCHW tensor -> NHWC tensor (zero copy when it already is a permuted NHWC buffer).
    A step converts the same constant input batch twice -- for the encoder and again for the losses -- so the most recent
    conversion of a tensor that needs no gradient is remembered and handed out again while that tensor is unmodified."""
    v = x.permute(0, 2, 3, 1)
    if v.is_contiguous():
        return v
    if x.requires_grad or torch.is_grad_enabled() and x.grad_fn is not None:
        return NchwToNhwc.apply(x)
    last = _LAST_NHWC[0]
    cap = torch.cuda.is_current_stream_capturing()
    if last is not None and last[0]() is x and last[1] == x._version and last[2] == x.data_ptr() and last[3] == cap:
        return last[4]
    out = NchwToNhwc.apply(x)
    _LAST_NHWC[0] = (weakref.ref(x), x._version, x.data_ptr(), cap, out)
    return out


def flatten_nchw(x_nhwc):
    """nn.Flatten over the reference's NCHW ordering (models/vae.py:128)."""
    n, h, w, c = x_nhwc.shape
    if h == 1 and w == 1:
        return x_nhwc.reshape(n, c)
    return NhwcToNchw.apply(x_nhwc).reshape(n, c * h * w)


def unflatten_nchw(x, c, h, w):
    """nn.Unflatten(1, (C, H, W)) (models/vae.py:143) producing NHWC."""
    n = x.shape[0]
    if h == 1 and w == 1:
        return x.reshape(n, 1, 1, c)
    return NchwToNhwc.apply(x.reshape(n, c, h, w))


# ---------------------------------------------------------------------------------------------
#: MOVAE_DEFER_REDUCE=0: every weight-gradient reduce is a launch of its own (A/B knob)
DEFER_REDUCE = _knob("DEFER_REDUCE")


class deferred_reduces:
    """Inside this block a convolution's weight-gradient split-K reduce whose destinations are gradient SINKS (a Jacobian row, an
    in-place accumulation target: autojac hands them over in a Destinations, and reads them only through this library's aggregation /
    optimizer entry points) is not launched on the spot: the library parks it and the next implicit-GEMM launch of the backward carries it
    as extra blocks (include/movae.h: movae_reduce_defer).  The block's exit -- and every library call that
    is not one of the backward's own ops (_lib.DEFER_PASS) -- launches a reduce that is still parked; code that hands a weight
    gradient to anything else (torch arithmetic, a collective, a caller's aggregator) inside the block calls flush_deferred()
    first: autojac does so before it adds two gradients with torch and, once the pull-back is done, before the aggregator sees J."""

    def __init__(self, enabled=True):
        self.enabled = enabled and DEFER_REDUCE
        self.prev = False

    def __enter__(self):
        if self.enabled:
            self.prev, L.DEFER_ON[0] = L.DEFER_ON[0], True
        return self

    def __exit__(self, *exc):
        if self.enabled:
            L.DEFER_ON[0] = self.prev
            if not self.prev:
                L.defer_flush()
        return False


def flush_deferred():
    L.defer_flush()


def _defer_ws(t, sunk):
    """(ws pointer, bytes) for a weight-gradient call: armed for a deferred reduce when every destination is a sink."""
    if sunk and L.DEFER_ON[0]:
        return L.defer_arm(t.device)
    return None


class ActLink:
    """Shared by a conv whose epilogue applied an activation (the producer) and the ONE conv that consumes its output (nn.Stack
    hands it to the next module only, so the output has no other reader): the consumer's input-gradient pass multiplies its
    result by act'(y) in the epilogue / split-K reduce (movae_fuse_t::ep_act_*) and records the tensor it produced in `applied`;
    the producer's backward, handed that very tensor, starts from the pre-activation gradient -- no activation-backward pass."""
    __slots__ = ("y", "act", "slope", "applied", "res_in", "res_done")

    def __init__(self):
        self.y, self.act, self.slope, self.applied = None, None, 0.0, None
        #: ResCarrier of the residual block whose branch starts with this (stand-alone) activation: the consumer's epilogue adds
        #: the identity cotangent too (res_done: it did, for the tensor in `applied`)
        self.res_in, self.res_done = None, False


class ResCarrier:
    """out = branch(x) + x (ops.residual_add): in the backward, the gradient w.r.t. `out` reaches x twice -- through the branch and
    straight.  Instead of letting the autograd engine add the two, residual_add's backward leaves its cotangent HERE and returns
    nothing for x; the FIRST op of the branch (the one applied to x: a conv, or a stand-alone activation linked to a conv) adds it
    to the input gradient it produces -- in the input-gradient kernel's epilogue where that kernel can (movae_fuse_t::ep_res),
    with one explicit add otherwise.  The first op is told at forward time (nn.Stack: res_in)."""
    __slots__ = ("res", "armed")

    def __init__(self):
        self.res, self.armed = None, False


def _res_take(carrier):
    """The identity branch's cotangent waiting in `carrier` (and disarm it), or None."""
    if carrier is None or carrier.res is None:
        return None
    r, carrier.res = carrier.res, None
    return r


#: MOVAE_FUSE_ACT=0: every conv runs its own activation-backward pass (A/B knob)
FUSE_ACT = _knob("FUSE_ACT")


class ConvFusion:
    """What a conv call is asked to fuse of its neighbouring BatchNorms (include/movae.h: movae_fuse_t).
    in_*: the input is the RAW output y of a producer conv whose BatchNorm + activation this conv applies while loading,
    x = leaky_relu(in_scale[c] * y + in_shift[c], in_slope).  want_stats: the epilogue (or split-K reduce) also emits the
    per-channel partial sums of this conv's own output for the BatchNorm that follows it: `stats` / `parts` on return."""
    __slots__ = ("in_scale", "in_shift", "in_slope", "want_stats", "stats", "parts", "link", "act_in", "act_out", "res_in", "res_out")

    def __init__(self, in_scale=None, in_shift=None, in_slope=1.0, want_stats=False, link=None, act_in=None, act_out=None, res_in=None,
                 res_out=None):
        self.in_scale, self.in_shift, self.in_slope, self.want_stats = in_scale, in_shift, float(in_slope), want_stats
        self.stats, self.parts = None, 0
        #: ActLink of the producer whose activation output is this conv's input / ActLink this conv fills for its consumer
        self.act_in, self.act_out = act_in, act_out
        #: ResCarrier of the residual block whose branch starts with THIS conv (its input is the block's input)
        self.res_in = res_in
        #: (x, ResCarrier): this conv ENDS a residual branch -- its epilogue adds the block's input x, its backward hands the
        #: cotangent of the sum to the carrier (what ops.residual_add would do, without the launches)
        self.res_out = res_out
        #: dict shared with the BatchNormLazy node whose output this conv consumes: the conv's backward leaves that
        #: BatchNorm's backward sums here (emitted by the input-gradient epilogue), the BatchNorm's backward picks them up
        self.link = link


#: (entry point, geometry) for which the library answered "unsupported" to a fused input transform: not asked again
_NO_FUSE = set()
#: A/B knobs of the fusion's three parts (development): the normalise-on-load of consumers, the statistics from producer epilogues
FUSE_NORM = _knob("FUSE_NORM")
FUSE_STATS = _knob("FUSE_STATS")


def _fuse_struct(in_norm, stats=None, bn=None, ep=None):
    """bn = (y, scale, shift, slope, part): the dispatched input-gradient pass also emits the BatchNorm backward sums.
    ep = ActLink: its epilogue multiplies by the producer's activation derivative."""
    f = L.MovaeFuse()
    if ep is not None:
        link, res = ep[0], ep[1]
        if link is not None:
            f.ep_act_y, f.ep_act, f.ep_slope = link.y.data_ptr(), L.ACT[link.act], float(link.slope)
        if res is not None:
            f.ep_res = res.data_ptr()
    if in_norm is not None:
        f.in_scale, f.in_shift, f.in_slope = in_norm[0].data_ptr(), in_norm[1].data_ptr(), float(in_norm[2])
    if stats is not None:
        f.stats, f.stats_cap = stats.data_ptr(), stats.numel()
    if bn is not None:
        f.bn_y, f.bn_scale, f.bn_shift, f.bn_slope = bn[0].data_ptr(), bn[1].data_ptr(), bn[2].data_ptr(), float(bn[3])
        f.bn_part, f.bn_cap = bn[4].data_ptr(), bn[4].numel()
    return f


#: MOVAE_FUSE_BN_BWD=0: the BatchNorm backward runs its own reduction pass (the sums are not taken from the dgrad epilogue)
FUSE_BN_BWD = _knob("FUSE_BN_BWD")


def _bn_request(ctx, x, in_norm, G):
    """(y, scale, shift, slope, part) when this conv's input is the raw output of a fused BatchNorm whose backward is waiting
    for its sums (ctx.bn_link), else None.  Room: one pair per 8 rows, group and channel (the finest granularity in use)."""
    link = getattr(ctx, "bn_link", None)
    if not FUSE_BN_BWD or link is None or in_norm is None or not ctx.needs_input_grad[0]:
        return None
    c = x.shape[-1]
    rows = x.numel() // c
    part = torch.empty(G * (rows // 8 + 64) * 2 * c, dtype=torch.float32, device=x.device)
    return (x, in_norm[0], in_norm[1], in_norm[2], part)


def _act_request(ctx, x, bn, dx_shape=None):
    """What this conv's input-gradient epilogue is asked to do besides the plain dx: (link, res, carrier) or None.
    link: the ActLink whose activation derivative to apply; res: the identity cotangent of the residual block whose branch starts
    at this conv (carrier = ctx.res_in) or at the linked stand-alone activation (carrier = link.res_in)."""
    if bn is not None or not ctx.needs_input_grad[0]:
        return None
    link = getattr(ctx, "act_in", None)
    if (not FUSE_ACT or link is None or link.y is None or link.y.shape != x.shape or link.y.data_ptr() != x.data_ptr()):
        link = None
    carrier = link.res_in if link is not None else getattr(ctx, "res_in", None)
    res = carrier.res if (carrier is not None and carrier.res is not None) else None
    if res is not None and (not FUSE_ACT or res.data_ptr() % 16 != 0 or (dx_shape is not None and tuple(res.shape) != tuple(dx_shape))):
        res = None  # (left in the carrier: added explicitly by whoever owns it)
    if link is None and res is None:
        return None
    return (link, res, carrier)


def _act_publish(req, f, dx):
    if req is None or f is None or not int(f.ep_act_done):
        return
    link, res, carrier = req
    if res is not None:
        carrier.res = None  # consumed by the epilogue
    if link is not None:
        link.applied, link.res_done = dx.data_ptr(), res is not None


def _res_finish(ctx, dx):
    """A conv that is the first op of a residual branch: whatever is still waiting in its carrier is added to dx explicitly."""
    r = _res_take(getattr(ctx, "res_in", None))
    if r is None or dx is None:
        return dx
    r = _c(r).view_as(dx)
    _call("movae_add", dx.data_ptr(), r.data_ptr(), dx.data_ptr(), dx.numel(), _st(dx))
    return dx


def _act_take(ctx, dy):
    """True when dy already is the PRE-activation gradient (the consumer's epilogue applied act'(y) -- ActLink)."""
    link = getattr(ctx, "act_out", None)
    if link is None or link.applied is None:
        return False
    ap, link.applied = link.applied, None
    if ap != dy.data_ptr():
        raise RuntimeError("activation derivative was fused into the consumer's input gradient, but a different tensor reached the "
                           "producer's backward (its output has another reader?): set MOVAE_FUSE_ACT=0")
    return True


def _bn_publish(ctx, f, bn, dx, G):
    if bn is not None and f is not None and int(f.bn_ppg) > 0:
        ctx.bn_link["bwd"] = (dx.data_ptr(), bn[4], int(f.bn_ppg), G)


def scale_shift_act(y, scale, shift, slope):
    """leaky_relu(scale[c] * y + shift[c], slope) as a real tensor (no tape: callers wrap it)."""
    y = _c(y)
    c = y.shape[-1]
    out = torch.empty_like(y)
    _call("movae_scale_shift_act", y.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), y.numel() // c, c, float(slope), _st(y))
    return out


def _act_bwd(dest, G, dy, y, dx, act, slope):
    """dx[g] = dy[g] * act'(y) for the G stacked cotangents.  Which entry point is the CALLER's choice (dest.engine), never G == 1: the
    engine's single cotangent takes movae_act_bwd; the walker -- a single-row pull-back included -- takes the grouped kernel (all
    groups in one launch, no bias sums) where the operands are aligned, and movae_act_bwd once per group where they are not."""
    c = y.shape[-1]
    if not dest.engine and c % 4 == 0 and dy.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0:
        wsp, wsb = _ws(dy)
        _call("movae_act_bwd_bias_grouped", G, dy.data_ptr(), y.data_ptr(), dx.data_ptr(), None, y.numel() // c, c, L.ACT[act], float(slope), 0,
              wsp, wsb, _st(dy))
        return
    step = y.numel() * dy.element_size()
    for g in range(G):
        _call("movae_act_bwd", dy.data_ptr() + g * step, y.data_ptr(), dx.data_ptr() + g * step, y.numel(), L.ACT[act], float(slope), _st(dy))


def _call_f(name, geom, x, in_norm, args, fuse):
    """The *_f form of entry point `name` on the operand x with the fused-BatchNorm transform in_norm (or None): args(x) -> the plain argument
    list, fuse(in_norm, retry) -> the movae_fuse_t.  Where the dispatched kernel cannot apply the transform (L.Unsupported) the shape is
    remembered in _NO_FUSE, the transformed operand is materialised and the call repeated without it (retry=True).
    -> (x as used, in_norm as used, the fuse struct of the call that ran)."""
    f = fuse(in_norm, False)
    try:
        _call(name + "_f", *args(x), C.byref(f))
    except L.Unsupported:
        if in_norm is None:
            raise
        _NO_FUSE.add((name, geom))
        x, in_norm = scale_shift_act(x, *in_norm), None
        f = fuse(None, True)
        _call(name + "_f", *args(x), C.byref(f))
    return x, in_norm, f


class Conv(Function):
    """conv2d / conv_transpose2d / linear (+bias, + fused activation).  `fusion` (ConvFusion or None): BatchNorm fused into the
    conv -- the producer's normalisation + activation applied to the input while it is loaded, and / or the statistics of the
    output emitted for the BatchNorm that follows."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, out_pad, transposed, act, slope, bias_grad_is_zero=False, fusion=None):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(x)
        x = _c(x)
        wm = weight_mem(w)
        n, hi, wi, ci = x.shape
        if transposed:
            assert wm.shape[0] == ci, "ConvTranspose2d weight/in_channels mismatch"
            kh, kw, co = wm.shape[1], wm.shape[2], wm.shape[3]
            ho, wo = convT_out_size(hi, kh, stride, pad, out_pad), convT_out_size(wi, kw, stride, pad, out_pad)
            fn = "movae_convT2d_fwd"
        else:
            assert wm.shape[3] == ci, "Conv2d weight/in_channels mismatch"
            co, kh, kw = wm.shape[0], wm.shape[1], wm.shape[2]
            ho, wo = conv_out_size(hi, kh, stride, pad), conv_out_size(wi, kw, stride, pad)
            fn = "movae_conv2d_fwd"
        y = torch.empty((n, ho, wo, co), dtype=x.dtype, device=x.device)
        wsp, wsb = _ws(x)
        geom = (n, hi, wi, ci, ho, wo, co, kh, kw, stride, pad)
        in_norm = None
        if fusion is not None and fusion.in_scale is not None:
            in_norm = (fusion.in_scale, fusion.in_shift, fusion.in_slope)
        stats = None
        if fusion is not None and fusion.want_stats and not L.ACT[act] and FUSE_STATS:
            # room for the finest partial granularity of any producer (a pair per 32-row wave tile; per 8 rows in the reduce)
            stats = torch.empty((n * ho * wo // 8 + 64) * 2 * co, dtype=torch.float32, device=x.device)
        if in_norm is not None and ((fn, geom) in _NO_FUSE or not FUSE_NORM):
            x, in_norm = scale_shift_act(x, *in_norm), None
        res_out = fusion.res_out if (fusion is not None and fusion.res_out is not None and not L.ACT[act]) else None
        if res_out is not None:
            assert tuple(res_out[0].shape) == tuple(y.shape), "residual input and branch output differ in shape"
        ep_fwd = (None, _c(res_out[0])) if res_out is not None else None
        if in_norm is None and stats is None and ep_fwd is None:
            _call(fn, x.data_ptr(), wm.data_ptr(), L.ptr(b), y.data_ptr(), *geom, L.ACT[act], float(slope), wsp, wsb, _st(x))
        else:
            x, in_norm, f = _call_f(fn, geom, x, in_norm, lambda x: (x.data_ptr(), wm.data_ptr(), L.ptr(b), y.data_ptr(), *geom, L.ACT[act],
                                                                     float(slope), wsp, wsb, _st(x)),
                                    lambda nrm, retry: _fuse_struct(nrm, stats, None, ep_fwd))
            if fusion is not None:
                fusion.stats, fusion.parts = stats, int(f.stats_parts)
            if ep_fwd is not None and not int(f.ep_act_done):  # this kernel has no such epilogue: one explicit add
                _call("movae_add", y.data_ptr(), ep_fwd[1].data_ptr(), y.data_ptr(), y.numel(), _st(x))
        ctx.geom = geom
        ctx.transposed, ctx.act, ctx.slope, ctx.has_bias = transposed, act, slope, b is not None
        ctx.bias_grad_is_zero = bias_grad_is_zero
        ctx.in_slope = in_norm[2] if in_norm is not None else None
        ctx.bn_link = fusion.link if (fusion is not None and in_norm is not None) else None
        # (a transformed input is a LazyBN's, whose backward goes through `link`: no ActLink with it)
        ctx.act_in = fusion.act_in if (fusion is not None and in_norm is None) else None
        ctx.res_in = fusion.res_in if fusion is not None else None
        ctx.res_out = res_out[1] if res_out is not None else None
        ctx.act_out = None
        if fusion is not None and fusion.act_out is not None and L.ACT[act]:
            ctx.act_out = fusion.act_out
            ctx.act_out.y, ctx.act_out.act, ctx.act_out.slope, ctx.act_out.applied = y.detach(), act, slope, None
        ctx.save_for_backward(x, w, y if L.ACT[act] else None, b, *(in_norm[:2] if in_norm is not None else ()))
        return y

    @staticmethod
    def _saved(ctx):
        """(x, w, y, b, in_norm): in_norm = (scale, shift, slope) when x is the raw output of a BatchNorm-fused producer."""
        sv = ctx.saved_tensors
        in_norm = (sv[4], sv[5], ctx.in_slope) if ctx.in_slope is not None else None
        return sv[0], sv[1], sv[2], sv[3], in_norm

    @staticmethod
    def _wgrad_call(name, in_norm, geom, args, bn=None, ep=None):
        """One weight-gradient (or paired dgrad + wgrad) call; with the fused-BatchNorm operand transform the *_f form, falling back
        to a materialised activation where the dispatched kernel cannot apply the transform.  args: (head, x_index, tail).
        bn: BatchNorm-backward request for the paired call's dgrad (_bn_request).  Returns (x as used, fuse struct or None)."""
        head, xi, tail = args
        x = head[xi]
        if in_norm is not None and (name, geom) in _NO_FUSE:
            x, in_norm = scale_shift_act(x, *in_norm), None
        argv = lambda x: [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in head[:xi] + (x,) + head[xi + 1:]] + list(tail)  # noqa: E731
        if in_norm is None and bn is None and ep is None:
            _call(name, *argv(x))
            return x, None
        # The repeated call asks for no `ep` (only a paired call on a LazyBN input without a `bn` request, its conv opening a residual
        # branch -- ctx.res_in -- gets here with one): it overwrites dx with the plain input gradient and reports ep_act_done == 0, so
        # _act_publish publishes nothing and _res_finish adds the carrier's cotangent explicitly.
        x, _, f = _call_f(name, geom, x, in_norm, argv, lambda nrm, retry: _fuse_struct(nrm, None, bn, None if retry else ep))
        return x, f

    @staticmethod
    def _run(ctx, G, dy, dest):
        """The backward of the G stacked cotangents dy [G, n, ho, wo, co] -> (dx [G, ...], [dW per group], [dbias per group]).
        dgrad runs as ONE launch over G*n images -- the pull-back is linear and per-sample, and the deep layers' grids are far
        too small to fill the chip one cotangent at a time; wgrad is one grouped launch (each group reduces over its own
        pixels, x is shared) writing straight into the groups' destinations (`dest`: a Destinations)."""
        x, w, y, b, in_norm = Conv._saved(ctx)
        if ctx.res_out is not None:  # this conv's output is branch + block input: dy is the identity branch's cotangent too
            ctx.res_out.res = dy
        n, hi, wi, ci, ho, wo, co, kh, kw, stride, pad = ctx.geom
        st = _st(dy)
        wsp, wsb = _ws(dy)
        arr = C.c_void_p * G
        db_done = None
        if L.ACT[ctx.act] and not _act_take(ctx, dy):
            dpre = torch.empty_like(dy)
            if _fuse_bias_grad(ctx, dy, y, co):
                # activation backward and the bias gradient (column sums of dpre) in one pass over dy
                db_done = [dest.sink(g, b, (co,)) for g in range(G)]
                _call("movae_act_bwd_bias_grouped", G, dy.data_ptr(), y.data_ptr(), dpre.data_ptr(), arr(*[t.data_ptr() for t in db_done]),
                      y.numel() // co, co, L.ACT[ctx.act], float(ctx.slope), 0, wsp, wsb, st)
            else:
                _act_bwd(dest, G, dy, y, dpre, ctx.act, ctx.slope)
            dy = dpre
        pre = "movae_convT2d_" if ctx.transposed else "movae_conv2d_"
        dx = dw = db = None
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        need_w = ctx.needs_input_grad[1] or need_b
        pair = need_w and ctx.needs_input_grad[0]  # both gradients: one call, one main launch
        bn = _bn_request(ctx, x, in_norm, G)
        ep = _act_request(ctx, x, bn, (G,) + tuple(x.shape))
        if ctx.needs_input_grad[0]:
            dx = torch.empty((G,) + tuple(x.shape), dtype=x.dtype, device=x.device)
            wm = weight_mem(w)
            if not pair:
                if bn is None and ep is None:
                    _call(pre + "dgrad", dy.data_ptr(), wm.data_ptr(), dx.data_ptr(), G * n, hi, wi, ci, ho, wo, co, kh, kw, stride, pad,
                          wsp, wsb, st)
                else:
                    f = _fuse_struct(None, None, bn, ep)
                    _call(pre + "dgrad_f", dy.data_ptr(), wm.data_ptr(), dx.data_ptr(), G * n, hi, wi, ci, ho, wo, co, kh, kw, stride, pad,
                          wsp, wsb, st, C.byref(f), G)
                    _bn_publish(ctx, f, bn, dx, G)
                    _act_publish(ep, f, dx)
        if need_w:
            wm_shape = (ci, kh, kw, co) if ctx.transposed else (co, kh, kw, ci)
            # a task-side parameter that an earlier loss already reached: add into its gradient inside the kernels' reduce
            plain_bias = need_b and db_done is None and not ctx.bias_grad_is_zero
            acc_w, acc_b = dest.accum_targets(w, b, plain_bias) if (db_done is None and not (ctx.has_bias and ctx.bias_grad_is_zero)) else (None, None)
            acc = 1 if acc_w is not None else 0
            dwm, sunk = ([acc_w.view(wm_shape)], True) if acc else dest.sinks(G, w, wm_shape)
            db_k = None
            if db_done is not None:
                db = db_done  # already produced by the fused activation-backward pass
            elif need_b and ctx.bias_grad_is_zero:
                # the bias feeds a training-mode BatchNorm, which subtracts the batch mean: d(loss)/d(bias) == 0
                # identically (the reference's value is rounding noise of order 1e-9); no column-sum pass
                db = [dest.zeros(g, b, (co,)) for g in range(G)]
            elif need_b:
                db, sunk_b = ([acc_b], True) if acc else dest.sinks(G, b, (co,))
                db_k, sunk = db, sunk and sunk_b
            dbp = arr(*[t.data_ptr() for t in db_k]) if db_k is not None else None
            # one grouped launch: blockIdx.z = group * splits + split, x is read by every group, dy by its own; with the
            # input gradient wanted too, dgrad and wgrad share the launch (igemm2_pair).  Every destination a sink (or an
            # in-place accumulation target): the split-K reduce may ride on a later launch (deferred_reduces)
            armed = _defer_ws(dy, sunk)
            if armed is not None:
                wsp, wsb = armed
            tail = (n, hi, wi, ci, ho, wo, co, kh, kw, stride, pad, acc, wsp, wsb, st)
            dwp = arr(*[t.data_ptr() for t in dwm])
            if pair:
                x, f = Conv._wgrad_call(pre + "dgrad_wgrad_grouped", in_norm, ctx.geom, ((G, dy, wm, x, dx, dwp, dbp), 3, tail), bn, ep)
                _bn_publish(ctx, f, bn, dx, G)
                _act_publish(ep, f, dx)
            else:
                x, _ = Conv._wgrad_call(pre + "wgrad_grouped", in_norm, ctx.geom, ((G, dy, x, dwp, dbp), 2, tail))
            dw = [t.permute(0, 3, 1, 2) for t in dwm]
        return _res_finish(ctx, dx), dw, db

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 11
        dx, dw, db = Conv._run(ctx, 1, _c(dy).unsqueeze(0), installed(True))
        return (_first(dx), _first(dw), _first(db)) + (None,) * 8

    @staticmethod
    def backward_batched(ctx, G, dy):
        """autojac._batched_pullback: dy is [G, n, ho, wo, co] (or a list of G tensors)."""
        return Conv._run(ctx, G, _stacked(dy, G), installed(False)) + (None,) * 8


def _fuse_bias_grad(ctx, dy, y, co):
    """The conv applied an activation in its epilogue and its bias needs a gradient: one fused pass (eltwise.hip) -- unless the
    weight-gradient kernel forms the column sums of dy itself while it stages dy (conv, 4-aligned channels: the implicit-GEMM
    wgrad; movae_conv2d_wgrad* falls back to the stand-alone column sum when its kernel cannot)."""
    ci = ctx.geom[3]
    if not ctx.transposed and ci % 4 == 0 and co % 4 == 0:
        return False
    return (ctx.has_bias and ctx.needs_input_grad[2] and not ctx.bias_grad_is_zero and co % 4 == 0 and
            dy.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def conv2d(x, w, b=None, stride=1, pad=0, act=None, slope=0.01, bias_grad_is_zero=False, fusion=None):
    return Conv.apply(x, w, b, stride, pad, 0, False, act, slope, bias_grad_is_zero, fusion)


def conv_transpose2d(x, w, b=None, stride=1, pad=0, out_pad=0, act=None, slope=0.01, bias_grad_is_zero=False, fusion=None):
    return Conv.apply(x, w, b, stride, pad, out_pad, True, act, slope, bias_grad_is_zero, fusion)


def linear(x, w, b=None, act=None, slope=0.01):
    """x [B, in], w [out, in] -> [B, out]  (a 1x1 convolution on a 1x1 image)."""
    n, fin = x.shape
    y = Conv.apply(x.reshape(n, 1, 1, fin), w.view(w.shape[0], fin, 1, 1), b, 1, 0, 0, False, act, slope)
    return y.reshape(n, w.shape[0])


#: MOVAE_LINEAR_PAIR=0: fc_mu / fc_var as two ordinary linear calls
LINEAR_PAIR = _knob("LINEAR_PAIR")


def linear_pair_ok(x, w1, b1, w2, b2, groups=1):
    """The range of movae_linear_pair_* (include/movae.h): two equally shaped nn.Linear layers on one [m, k] input."""
    if not (LINEAR_PAIR and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and w1.shape == w2.shape and b1 is not None and b2 is not None):
        return False
    m, k = x.shape
    n = w1.shape[0]
    if w1.shape[1] != k or n % 4 or k % 4 or max(m * n, m * k, n * k) > (1 << 20) or max(m, n, k) > 2048 or groups > 4:
        return False
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (x, w1, w2))


class LinearPair(Function):
    """(x w1^T + b1, x w2^T + b2) in one launch, and the two layers' backward in two (movae_linear_pair_*): fc_mu || fc_var of the
    VAE / BetaTC-VAE encoders (models/vae.py:187-192).  The caller checks linear_pair_ok."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        x = _c(x)
        m, k = x.shape
        n = w1.shape[0]
        y1 = torch.empty((m, n), dtype=x.dtype, device=x.device)
        y2 = torch.empty_like(y1)
        _call("movae_linear_pair_fwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y1.data_ptr(), y2.data_ptr(),
              m, n, k, _st(x))
        ctx.save_for_backward(x, w1, b1, w2, b2)
        return y1, y2

    @staticmethod
    def _run(ctx, G, dy1, dy2, dest):
        """dy_i: [G, m, n] stacked (or None: that output had no cotangent).  dest: a Destinations."""
        x, w1, b1, w2, b2 = ctx.saved_tensors
        m, k = x.shape
        n = w1.shape[0]
        ref = dy1 if dy1 is not None else dy2
        if dy1 is None:
            dy1 = torch.zeros_like(ref)
        if dy2 is None:
            dy2 = torch.zeros_like(ref)
        need_x = ctx.needs_input_grad[0]
        need_w = any(ctx.needs_input_grad[1:])
        dx = torch.empty((G, m, k), dtype=x.dtype, device=x.device) if need_x else None
        dw1 = dw2 = db1 = db2 = None
        if need_w:
            dw1, dw2 = [dest.sink(g, w1, (n, k)) for g in range(G)], [dest.sink(g, w2, (n, k)) for g in range(G)]
            db1, db2 = [dest.sink(g, b1, (n,)) for g in range(G)], [dest.sink(g, b2, (n,)) for g in range(G)]
        for g0 in range(0, G, 4):  # (the entry point takes up to four cotangent groups)
            g1 = min(G, g0 + 4)
            ptrs = lambda ts: (C.c_void_p * (g1 - g0))(*[t.data_ptr() for t in ts[g0:g1]]) if ts is not None else None  # noqa: E731
            _call("movae_linear_pair_bwd", g1 - g0, dy1[g0].data_ptr(), dy2[g0].data_ptr(), w1.data_ptr(), w2.data_ptr(), x.data_ptr(),
                  dx[g0].data_ptr() if dx is not None else 0, ptrs(dw1), ptrs(dw2), ptrs(db1), ptrs(db2), m, n, k, _st(x))
        return dx, dw1, db1, dw2, db2

    @staticmethod
    def backward(ctx, dy1, dy2):
        if dy1 is None and dy2 is None:
            return None, None, None, None, None
        one = lambda t: _c(t).unsqueeze(0) if t is not None else None  # noqa: E731
        return tuple(_first(t) for t in LinearPair._run(ctx, 1, one(dy1), one(dy2), installed(True)))

    @staticmethod
    def backward_batched(ctx, G, dy1, dy2):
        if dy1 is None and dy2 is None:
            return None, None, None, None, None
        st = lambda t: _stacked(t, G) if t is not None else None  # noqa: E731
        return LinearPair._run(ctx, G, st(dy1), st(dy2), installed(False))


def linear_pair(x, w1, b1, w2, b2):
    """(linear(x, w1, b1), linear(x, w2, b2)); one launch where the shapes allow (linear_pair_ok)."""
    if linear_pair_ok(x, w1, b1, w2, b2):
        return LinearPair.apply(x, w1, b1, w2, b2)
    return linear(x, w1, b1), linear(x, w2, b2)


# ---------------------------------------------------------------------------------------------
class BatchNormAct(Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, training, eps, momentum, act, slope, num_batches_tracked=None):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(y)
        y = _c(y)
        c = y.shape[-1]
        rows = y.numel() // c
        out = torch.empty_like(y)
        mean = torch.empty(c, dtype=y.dtype, device=y.device)
        rstd = torch.empty(c, dtype=y.dtype, device=y.device)
        wsp, wsb = _ws(y)
        _call("movae_bn_act_fwd", y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), mean.data_ptr(),
              rstd.data_ptr(), L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked), rows, c, float(eps), float(momentum),
              1 if training else 0, L.ACT[act], float(slope), wsp, wsb, _st(y))
        ctx.act, ctx.slope, ctx.training = act, slope, training
        ctx.save_for_backward(y, gamma, beta, mean, rstd)
        ctx.mark_non_differentiable(mean, rstd)
        return out

    @staticmethod
    def _run(ctx, G, dout, dest):
        if not ctx.training:
            raise RuntimeError("BatchNormAct backward is implemented for training-mode statistics only")
        gamma, beta = ctx.saved_tensors[1:3]
        dgs = [dest.sink(g, gamma, gamma.shape) for g in range(G)]
        dbs = [dest.sink(g, beta, beta.shape) for g in range(G)]
        return _bn_act_bwd(dest, G, dout, ctx.saved_tensors, dgs, dbs, ctx.act, ctx.slope), dgs, dbs

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * 11
        return tuple(t[0] for t in BatchNormAct._run(ctx, 1, _c(dout).unsqueeze(0), installed(True))) + (None,) * 8

    @staticmethod
    def backward_batched(ctx, G, dout):
        return BatchNormAct._run(ctx, G, _stacked(dout, G), installed(False)) + (None,) * 8


def _bn_act_bwd(dest, G, dout, saved, dgs, dbs, act, slope):
    """-> dy [G, ...]: the training-mode BatchNorm (+ activation) backward of the G stacked cotangents dout on the saved raw y, the
    parameter gradients written to dgs[g] / dbs[g].  The batch statistics of the cotangent are taken per group inside the kernels
    (blockIdx.y).  As in _act_bwd the entry point is the caller's choice, not G == 1's."""
    y, gamma, beta, mean, rstd = saved[:5]
    c = y.shape[-1]
    dy = torch.empty_like(dout)
    wsp, wsb = _ws(y)
    arr = C.c_void_p * G
    name, head, dg, db = ("movae_bn_act_bwd", (), dgs[0].data_ptr(), dbs[0].data_ptr()) if dest.engine else \
        ("movae_bn_act_bwd_grouped", (G,), arr(*[t.data_ptr() for t in dgs]), arr(*[t.data_ptr() for t in dbs]))
    _call(name, *head, dout.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(),
          dg, db, y.numel() // c, c, L.ACT[act], float(slope), 0, wsp, wsb, _st(y))
    return dy


# ---- BatchNorm fused into its neighbours ---------------------------------------------------------------
class LazyBN:
    """The output of a training-mode BatchNorm (+ LeakyReLU / ReLU) that has NOT been written to memory: `y` is the producer
    conv's raw output (as a node of the tape whose gradient is the gradient w.r.t. the normalised activation), scale / shift the
    folded per-channel map.  Convolutions consume it directly (ops.conv2d(..., fusion=...) applies the map while loading);
    anything else calls materialize().  Deliberately NOT a tensor: a consumer that does not know about it fails loudly."""
    __slots__ = ("y", "scale", "shift", "slope", "link")

    def __init__(self, y, scale, shift, slope, link=None):
        self.y, self.scale, self.shift, self.slope, self.link = y, scale, shift, float(slope), link

    def fusion(self, want_stats=False):
        return ConvFusion(self.scale, self.shift, self.slope, want_stats, self.link)

    def materialize(self):
        return ScaleShiftAct.apply(self.y, self.scale, self.shift, self.slope)


def materialize(x):
    return x.materialize() if isinstance(x, LazyBN) else x


class ScaleShiftAct(Function):
    """LazyBN -> real tensor.  `y` stands for the normalised activation on the tape, so the backward is the identity."""

    @staticmethod
    def forward(ctx, y, scale, shift, slope):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        return scale_shift_act(y, scale, shift, slope)

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * 4
        return dout, None, None, None

    @staticmethod
    def backward_batched(ctx, G, dout):
        return dout, None, None, None


_ACT_OF_SLOPE = {1.0: None, 0.0: "relu"}


class BatchNormLazy(Function):
    """Training-mode BatchNorm2d (+ LeakyReLU / ReLU) whose statistics come from the producer conv's partial sums
    (ConvFusion.stats) -- or from one stand-alone pass over y when that kernel could not emit them -- and whose output is
    not materialised: returns (y as a new tape node, scale, shift).  Backward: the ordinary BatchNorm backward kernels
    (movae_bn_act_bwd) on the saved raw y."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, slope, stats, parts, link=None):
        L.require_gpu(y)
        c = y.shape[-1]
        rows = y.numel() // c
        st = _st(y)
        if not parts:
            stats = torch.empty(1100 * 2 * c, dtype=torch.float32, device=y.device)  # movae_bn_stats: at most 1024 partials (+ room to fold them)
            pout = C.c_int(0)
            _call("movae_bn_stats", y.data_ptr(), rows, c, stats.data_ptr(), stats.numel(), C.byref(pout), st)
            parts = pout.value
        mean = torch.empty(c, dtype=y.dtype, device=y.device)
        rstd, scale, shift = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
        _call("movae_bn_finalize", stats.data_ptr(), stats.numel(), int(parts), rows, c, gamma.data_ptr(), beta.data_ptr(), float(eps),
              float(momentum), mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), L.ptr(running_mean),
              L.ptr(running_var), L.ptr(num_batches_tracked), st)
        ctx.act, ctx.slope = ("lrelu" if slope not in _ACT_OF_SLOPE else _ACT_OF_SLOPE[slope]), slope
        ctx.link = link
        ctx.save_for_backward(y, gamma, beta, mean, rstd, scale, shift)
        ctx.mark_non_differentiable(scale, shift)
        ctx.set_materialize_grads(False)  # no zero-fill launches for the two auxiliary outputs' (never used) gradients
        return y.view_as(y), scale, shift

    @staticmethod
    def _from_sums(ctx, G, dout, dgs, dbs):
        """The consumer conv's input-gradient pass left this BatchNorm's backward sums (ctx.link['bwd']): one tiny finalize
        launch and ONE pass that forms dy.  None when no (matching) sums are there."""
        ent = ctx.link.pop("bwd", None) if ctx.link is not None else None
        if ent is None or ent[0] != dout.data_ptr() or ent[3] != G:
            return None
        y, gamma, beta, mean, rstd, scale, shift = ctx.saved_tensors
        _, part, ppg, _ = ent
        c = y.shape[-1]
        rows = y.numel() // c
        if c % 4 != 0:
            return None
        coef = torch.empty((G, 3, c), dtype=y.dtype, device=y.device)
        arr = C.c_void_p * G
        st = _st(y)
        dy = torch.empty_like(dout)
        _call("movae_bn_bwd_finalize_apply", part.data_ptr(), part.numel(), ppg, G, rows, c, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              arr(*[t.data_ptr() for t in dgs]), arr(*[t.data_ptr() for t in dbs]), coef.data_ptr(), 0, dout.data_ptr(), y.data_ptr(),
              scale.data_ptr(), shift.data_ptr(), float(ctx.slope), dy.data_ptr(), st)
        return dy

    @staticmethod
    def _run(ctx, G, dout, dest):
        gamma, beta = ctx.saved_tensors[1:3]
        dgs = [dest.sink(g, gamma, gamma.shape) for g in range(G)]
        dbs = [dest.sink(g, beta, beta.shape) for g in range(G)]
        dy = BatchNormLazy._from_sums(ctx, G, dout, dgs, dbs)
        if dy is None:
            dy = _bn_act_bwd(dest, G, dout, ctx.saved_tensors, dgs, dbs, ctx.act, ctx.slope)
        return dy, dgs, dbs

    @staticmethod
    def backward(ctx, dout, _ds, _dh):
        if dout is None:
            return (None,) * 12
        return tuple(t[0] for t in BatchNormLazy._run(ctx, 1, _c(dout).unsqueeze(0), installed(True))) + (None,) * 9

    @staticmethod
    def backward_batched(ctx, G, dout, _ds=None, _dh=None):
        return BatchNormLazy._run(ctx, G, _stacked(dout, G), installed(False)) + (None,) * 9


def batch_norm_lazy(y, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, act, slope, fusion):
    """-> LazyBN.  act in (None, 'lrelu', 'relu'); fusion: the ConvFusion the producer conv was called with (its statistics)."""
    sl = 1.0 if act is None else (0.0 if act == "relu" else float(slope))
    stats, parts = (fusion.stats, fusion.parts) if fusion is not None else (None, 0)
    link = {}
    try:
        yv, scale, shift = BatchNormLazy.apply(y, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, sl, stats,
                                               parts, link)
    except L.Unsupported:  # no partial sums from the producer and a shape the stand-alone statistics pass does not take
        return batch_norm_act(y, gamma, beta, running_mean, running_var, True, eps, momentum, act, slope, num_batches_tracked)
    return LazyBN(yv, scale, shift, sl, link)


def batch_norm_act(y, gamma, beta, running_mean, running_var, training, eps=1e-5, momentum=0.1, act=None, slope=0.01,
                   num_batches_tracked=None):
    """num_batches_tracked (int64 device scalar) is incremented inside the statistics kernel in training mode."""
    return BatchNormAct.apply(y, gamma, beta, running_mean, running_var, training, eps, momentum, act, slope, num_batches_tracked)


# ---------------------------------------------------------------------------------------------
class Activation(Function):
    """A stand-alone activation.  act_out (ActLink or None): the output has exactly one reader, a conv whose input-gradient pass
    may apply this activation's derivative itself (nn.Stack arranges that); the backward then passes the gradient through."""

    @staticmethod
    def forward(ctx, x, act, slope, act_out=None, res_in=None):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(x)
        x = _c(x)
        y = torch.empty_like(x)
        _call("movae_act_fwd", x.data_ptr(), y.data_ptr(), x.numel(), L.ACT[act], float(slope), _st(x))
        ctx.act, ctx.slope = act, slope
        ctx.act_out, ctx.res_in = act_out, res_in  # res_in: this activation is the first op of a residual branch (ResCarrier)
        if act_out is not None:
            act_out.y, act_out.act, act_out.slope, act_out.applied = y.detach(), act, slope, None
            act_out.res_in, act_out.res_done = res_in, False
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def _run(ctx, G, dy, dest):
        (y,) = ctx.saved_tensors
        if _act_take(ctx, dy):
            return Activation._add_res(ctx, dy, ctx.act_out.res_done)
        dx = torch.empty_like(dy)
        _act_bwd(dest, G, dy, y, dx, ctx.act, ctx.slope)
        return Activation._add_res(ctx, dx, False)

    @staticmethod
    def _add_res(ctx, dx, already):
        """dx (+)= the identity cotangent of the residual block this activation opens, unless the consumer's epilogue added it."""
        r = _res_take(ctx.res_in)
        if r is not None and not already:
            r = _c(r).view_as(dx)
            _call("movae_add", dx.data_ptr(), r.data_ptr(), dx.data_ptr(), dx.numel(), _st(dx))
        return dx

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 5
        return (Activation._run(ctx, 1, _c(dy).unsqueeze(0), installed(True))[0],) + (None,) * 4

    @staticmethod
    def backward_batched(ctx, G, dy):
        return (Activation._run(ctx, G, _stacked(dy, G), installed(False)),) + (None,) * 4


def activation(x, act, slope=0.01, act_out=None, res_in=None):
    if not L.ACT[act]:
        return x
    return Activation.apply(x, act, slope, act_out, res_in)


class Add(Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(a)
        a, b = _c(a), _c(b)
        y = torch.empty_like(a)
        _call("movae_add", a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), _st(a))
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 2
        return dy, dy

    @staticmethod
    def backward_batched(ctx, G, dy):
        return dy, dy


class ResidualAdd(Function):
    """out = branch + x with the identity cotangent handed to the branch's first op (ResCarrier) instead of to the engine."""

    @staticmethod
    def forward(ctx, branch, x, carrier):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        branch, x = _c(branch), _c(x)
        y = torch.empty_like(x)
        _call("movae_add", branch.data_ptr(), x.data_ptr(), y.data_ptr(), x.numel(), _st(x))
        ctx.carrier = carrier
        return y

    @staticmethod
    def _run(ctx, dy, stacked):
        """dy passes through as it came (tensor or per-group list); the carrier gets it stacked ([G, ...]: stacked(dy))."""
        if ctx.carrier is None or not ctx.needs_input_grad[1]:
            return dy, dy, None
        ctx.carrier.res = stacked(dy)
        return dy, None, None

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 3
        return ResidualAdd._run(ctx, dy, lambda t: _c(t).unsqueeze(0))

    @staticmethod
    def backward_batched(ctx, G, dy):
        return ResidualAdd._run(ctx, dy, lambda t: _stacked(t, G))


def residual_add(branch, x, carrier):
    """branch(x) + x; carrier: the ResCarrier the branch's first op was given (None: a plain add)."""
    assert branch.shape == x.shape
    return ResidualAdd.apply(branch, x, carrier)


def add(a, b):
    assert a.shape == b.shape
    return Add.apply(a, b)


class ConcatChannels(Function):
    """torch.cat([a, b], dim=channel) for NHWC tensors (models/vq_vae2.py:228,241)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(a)
        a, b = _c(a), _c(b)
        ca, cb = a.shape[-1], b.shape[-1]
        rows = a.numel() // ca
        y = torch.empty(a.shape[:-1] + (ca + cb,), dtype=a.dtype, device=a.device)
        st = _st(a)
        _call("movae_copy_channels", a.data_ptr(), y.data_ptr(), rows, ca, ca + cb, 0, 0, ca, st)
        _call("movae_copy_channels", b.data_ptr(), y.data_ptr(), rows, cb, ca + cb, 0, ca, cb, st)
        ctx.ca, ctx.cb = ca, cb
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 2
        dy = _c(dy)
        ca, cb = ctx.ca, ctx.cb
        rows = dy.numel() // (ca + cb)
        da = torch.empty(dy.shape[:-1] + (ca,), dtype=dy.dtype, device=dy.device)
        db = torch.empty(dy.shape[:-1] + (cb,), dtype=dy.dtype, device=dy.device)
        st = _st(dy)
        _call("movae_copy_channels", dy.data_ptr(), da.data_ptr(), rows, ca + cb, ca, 0, 0, ca, st)
        _call("movae_copy_channels", dy.data_ptr(), db.data_ptr(), rows, ca + cb, cb, ca, 0, cb, st)
        return da, db


def concat_channels(a, b):
    return ConcatChannels.apply(a, b)


# ---------------------------------------------------------------------------------------------
class Reparameterize(Function):
    @staticmethod
    def forward(ctx, mu, log_var, eps):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(mu)
        mu, log_var, eps = _c(mu), _c(log_var), _c(eps)
        z = torch.empty_like(mu)
        _call("movae_reparam_fwd", mu.data_ptr(), log_var.data_ptr(), eps.data_ptr(), z.data_ptr(), mu.numel(), _st(mu))
        ctx.save_for_backward(log_var, eps)
        ctx.in_ptrs = (mu.data_ptr(), log_var.data_ptr())  # (the cotangent sinks are keyed by the feature tensors)
        return z

    @staticmethod
    def backward(ctx, dz):
        if dz is None:
            return (None,) * 3
        log_var, eps = ctx.saved_tensors
        dz = _c(dz)
        dmu, dlv = installed(True).cotangent(ctx.in_ptrs[0], dz), installed(True).cotangent(ctx.in_ptrs[1], dz)
        _call("movae_reparam_bwd", dz.data_ptr(), log_var.data_ptr(), eps.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), dz.numel(), _st(dz))
        return dmu, dlv, None


def reparameterize(mu, log_var, eps):
    return Reparameterize.apply(mu, log_var, eps)


class ReparameterizeRNG(Function):
    """z = mu + exp(0.5 * log_var) * eps with eps ~ N(0, 1) drawn inside the kernel (movae_reparam_rng_fwd): `state` is a device
    int64[2] = {seed, draws so far}, advanced by the launch itself -- one launch per step where torch.randn_like under graph capture
    plus the reparameterisation are four.  The backward is Reparameterize's (eps is kept)."""

    @staticmethod
    def forward(ctx, mu, log_var, state):
        ctx.set_materialize_grads(False)
        L.require_gpu(mu)
        mu, log_var = _c(mu), _c(log_var)
        assert state.dtype == torch.int64 and state.numel() == 2 and state.device == mu.device
        z, eps = torch.empty_like(mu), torch.empty_like(mu)
        _call("movae_reparam_rng_fwd", mu.data_ptr(), log_var.data_ptr(), eps.data_ptr(), z.data_ptr(), mu.numel(), state.data_ptr(), 1, _st(mu))
        ctx.save_for_backward(log_var, eps)
        ctx.in_ptrs = (mu.data_ptr(), log_var.data_ptr())
        return z

    @staticmethod
    def backward(ctx, dz):
        if dz is None:
            return (None,) * 3
        log_var, eps = ctx.saved_tensors
        dz = _c(dz)
        dmu, dlv = installed(True).cotangent(ctx.in_ptrs[0], dz), installed(True).cotangent(ctx.in_ptrs[1], dz)
        _call("movae_reparam_bwd", dz.data_ptr(), log_var.data_ptr(), eps.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), dz.numel(), _st(dz))
        return dmu, dlv, None


def reparameterize_rng(mu, log_var, state):
    return ReparameterizeRNG.apply(mu, log_var, state)


class ReparameterizePriorRNG(Function):
    """ReparameterizeRNG that also draws z_prior ~ N(0, I) [n_prior rows, latent] in the same launch, from the same generator state
    and draw number (movae_reparam_prior_rng_fwd): the cycle branch's prior sample of the cycle / recursive-cyclic VAEs costs no
    launch and no counter advance of its own.  z's noise is exactly ReparameterizeRNG's.  Returns (z, z_prior); z_prior is a
    constant of the tape."""

    @staticmethod
    def forward(ctx, mu, log_var, state, n_prior):
        ctx.set_materialize_grads(False)
        L.require_gpu(mu)
        mu, log_var = _c(mu), _c(log_var)
        assert state.dtype == torch.int64 and state.numel() == 2 and state.device == mu.device and mu.dim() == 2
        z, eps = torch.empty_like(mu), torch.empty_like(mu)
        prior = torch.empty((int(n_prior), mu.shape[1]), dtype=mu.dtype, device=mu.device)
        _call("movae_reparam_prior_rng_fwd", mu.data_ptr(), log_var.data_ptr(), eps.data_ptr(), z.data_ptr(), mu.numel(), prior.data_ptr(),
              prior.numel(), state.data_ptr(), 1, _st(mu))
        ctx.mark_non_differentiable(prior)
        ctx.save_for_backward(log_var, eps)
        ctx.in_ptrs = (mu.data_ptr(), log_var.data_ptr())
        return z, prior

    @staticmethod
    def backward(ctx, dz, _dprior):
        if dz is None:
            return (None,) * 4
        log_var, eps = ctx.saved_tensors
        dz = _c(dz)
        dmu, dlv = installed(True).cotangent(ctx.in_ptrs[0], dz), installed(True).cotangent(ctx.in_ptrs[1], dz)
        _call("movae_reparam_bwd", dz.data_ptr(), log_var.data_ptr(), eps.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), dz.numel(), _st(dz))
        return dmu, dlv, None, None


def reparameterize_prior_rng(mu, log_var, state, n_prior):
    """-> (z, z_prior)"""
    return ReparameterizePriorRNG.apply(mu, log_var, state, n_prior)


# ---------------------------------------------------------------------------------------------
def _links_output(link, recons):
    """Is `link` the ActLink of the conv + tanh / sigmoid pair that produced this very `recons`?  (The caller vouches that the loss
    is the one reader of `recons` on the tape; whether the link it took from its decoder belongs to this tensor is checked here.)"""
    return (FUSE_ACT and link is not None and link.act in ("tanh", "sigmoid") and link.y is not None
            and link.y.data_ptr() == recons.data_ptr() and link.y.shape == recons.shape)


class ReconLoss(Function):
    """scale * mean(objective(recons, inputs)); both tensors must share one memory order."""

    @staticmethod
    def forward(ctx, recons, inputs, kind, scale, act_link=None):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(recons)
        recons, inputs = _c(recons), _c(inputs)
        assert recons.shape == inputs.shape, (recons.shape, inputs.shape)
        out = torch.empty((), dtype=recons.dtype, device=recons.device)
        wsp, wsb = _ws(recons)
        _call("movae_recon_loss_fwd", recons.data_ptr(), inputs.data_ptr(), out.data_ptr(), recons.numel(), L.RECON[kind],
              float(scale), wsp, wsb, _st(recons))
        ctx.kind, ctx.scale = kind, scale
        # recons = act(pre), this loss its one reader (ActLink): the backward kernel hands the producing conv the PRE-activation gradient
        ctx.act_link = act_link if _links_output(act_link, recons) else None
        ctx.save_for_backward(recons, inputs)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 5
        recons, inputs = ctx.saved_tensors
        g = _c(g)
        dr = torch.empty_like(recons)
        link = ctx.act_link
        if link is not None:
            _call("movae_recon_loss_bwd_act", recons.data_ptr(), inputs.data_ptr(), g.data_ptr(), dr.data_ptr(), recons.numel(),
                  L.RECON[ctx.kind], float(ctx.scale), L.ACT[link.act], float(link.slope), _st(recons))
            link.applied = dr.data_ptr()
        else:
            _call("movae_recon_loss_bwd", recons.data_ptr(), inputs.data_ptr(), g.data_ptr(), dr.data_ptr(), recons.numel(),
                  L.RECON[ctx.kind], float(ctx.scale), _st(recons))
        return dr, None, None, None, None


class EdgeWeightedPixelLoss(Function):
    """models/gg_vae.py:125-137: scale * mean(w * (recons - inputs)^2), w = Sobel magnitude of `inputs` (max over channels,
    normalised by the batch maximum).  NHWC operands; no gradient flows into `inputs`."""

    @staticmethod
    def forward(ctx, recons, inputs, scale):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(recons)
        recons, inputs = _c(recons), _c(inputs)
        assert recons.shape == inputs.shape and recons.dim() == 4, (recons.shape, inputs.shape)
        n, h, w, c = recons.shape
        w_raw = torch.empty((n, h, w), dtype=recons.dtype, device=recons.device)
        wmax = torch.empty((), dtype=recons.dtype, device=recons.device)
        out = torch.empty((), dtype=recons.dtype, device=recons.device)
        wsp, wsb = _ws(recons)
        st = _st(recons)
        _call("movae_edge_weights", inputs.data_ptr(), w_raw.data_ptr(), wmax.data_ptr(), n, h, w, c, wsp, wsb, st)
        _call("movae_edge_weighted_mse_fwd", recons.data_ptr(), inputs.data_ptr(), w_raw.data_ptr(), wmax.data_ptr(), out.data_ptr(),
              n, h, w, c, float(scale), wsp, wsb, st)
        ctx.scale = scale
        ctx.save_for_backward(recons, inputs, w_raw, wmax)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 3
        recons, inputs, w_raw, wmax = ctx.saved_tensors
        g = _c(g)
        n, h, w, c = recons.shape
        dr = torch.empty_like(recons)
        _call("movae_edge_weighted_mse_bwd", recons.data_ptr(), inputs.data_ptr(), w_raw.data_ptr(), wmax.data_ptr(), g.data_ptr(),
              dr.data_ptr(), n, h, w, c, float(ctx.scale), _st(recons))
        return dr, None, None


class EdgeMatchingLoss(Function):
    """scale * mean f(sobel recons, sobel inputs) for the reference's edge-matching variants (`mode`, a key of
    _lib.EDGE_MATCH; include/movae.h lists each variant's reference lines).  NHWC; no gradient flows into `inputs`."""

    @staticmethod
    def forward(ctx, recons, inputs, scale, mode):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(recons)
        recons, inputs = _c(recons), _c(inputs)
        assert recons.shape == inputs.shape and recons.dim() == 4, (recons.shape, inputs.shape)
        n, h, w, c = recons.shape
        out = torch.empty((), dtype=recons.dtype, device=recons.device)
        stats = torch.empty(8, dtype=recons.dtype, device=recons.device)
        wsp, wsb = _ws(recons)
        _call("movae_edge_match_fwd", recons.data_ptr(), inputs.data_ptr(), out.data_ptr(), n, h, w, c, float(scale),
              L.EDGE_MATCH[mode], stats.data_ptr(), wsp, wsb, _st(recons))
        ctx.scale, ctx.mode = scale, mode
        ctx.save_for_backward(recons, inputs, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 4
        recons, inputs, stats = ctx.saved_tensors
        g = _c(g)
        n, h, w, c = recons.shape
        dr, ta, tb = torch.empty_like(recons), torch.empty_like(recons), torch.empty_like(recons)
        _call("movae_edge_match_bwd", recons.data_ptr(), inputs.data_ptr(), g.data_ptr(), dr.data_ptr(), ta.data_ptr(), tb.data_ptr(),
              n, h, w, c, float(ctx.scale), L.EDGE_MATCH[ctx.mode], stats.data_ptr(), _st(recons))
        return dr, None, None, None


def edge_weighted_pixel_loss(recons, inputs, scale=1.0):
    return EdgeWeightedPixelLoss.apply(recons, inputs, scale)


def edge_matching_loss(recons, inputs, scale=1.0, mode="mag"):
    return EdgeMatchingLoss.apply(recons, inputs, scale, mode)


def recon_loss(recons, inputs, kind, scale, act_link=None):
    return ReconLoss.apply(recons, inputs, kind, scale, act_link)


class KLDivergence(Function):
    @staticmethod
    def forward(ctx, mu, log_var, scale):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(mu)
        mu, log_var = _c(mu), _c(log_var)
        b, d = mu.shape
        out = torch.empty((), dtype=mu.dtype, device=mu.device)
        wsp, wsb = _ws(mu)
        _call("movae_kl_fwd", mu.data_ptr(), log_var.data_ptr(), out.data_ptr(), b, d, float(scale), wsp, wsb, _st(mu))
        ctx.scale = scale
        ctx.save_for_backward(mu, log_var)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 3
        mu, log_var = ctx.saved_tensors
        g = _c(g)
        b, d = mu.shape
        dmu, dlv = installed(True).cotangent(mu.data_ptr(), mu), installed(True).cotangent(log_var.data_ptr(), mu)
        _call("movae_kl_bwd", mu.data_ptr(), log_var.data_ptr(), g.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), b, d,
              float(ctx.scale), _st(mu))
        return dmu, dlv, None


def kl_divergence(mu, log_var, scale=1.0):
    return KLDivergence.apply(mu, log_var, scale)


class VAELosses(Function):
    """(reconstruction_loss, kld_loss, total_loss) of models/vae.py:211-228 in three launches instead of five (the two partial-sum
    passes and ONE final kernel that also adds the two): scale_r * mean(objective(recons, inputs)), scale_k * kl(mu, log_var) and
    their fp32 sum.  Bit-identical to ReconLoss + KLDivergence + a tensor add.  The backward serves whichever of the three
    cotangents arrive (mtl_backward differentiates the components one at a time, `--agg sum` the total)."""

    @staticmethod
    def forward(ctx, recons, inputs, kind, scale_r, mu, log_var, scale_k, act_link=None):
        ctx.set_materialize_grads(False)
        L.require_gpu(recons)
        recons, inputs, mu, log_var = _c(recons), _c(inputs), _c(mu), _c(log_var)
        assert recons.shape == inputs.shape, (recons.shape, inputs.shape)
        b, d = mu.shape
        out = torch.empty(3, dtype=recons.dtype, device=recons.device)
        wsp, wsb = _ws(recons)
        _call("movae_vae_losses_fwd", recons.data_ptr(), inputs.data_ptr(), recons.numel(), L.RECON[kind], float(scale_r), mu.data_ptr(),
              log_var.data_ptr(), b, d, float(scale_k), out.data_ptr(), wsp, wsb, _st(recons))
        ctx.kind, ctx.scale_r, ctx.scale_k = kind, scale_r, scale_k
        # recons = act(pre) is the decoder's output activation and this loss its one reader (ActLink): the backward kernel applies
        # act'(pre) and hands the producing conv the PRE-activation gradient
        ctx.act_link = act_link if _links_output(act_link, recons) else None
        ctx.save_for_backward(recons, inputs, mu, log_var)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_rec, g_kld, g_tot):
        recons, inputs, mu, log_var = ctx.saved_tensors
        both = lambda a, b: a if b is None else (b if a is None else a + b)  # noqa: E731  (total_loss feeds both terms)
        gr, gk = both(g_rec, g_tot), both(g_kld, g_tot)
        dr = dmu = dlv = None
        if gr is not None and ctx.needs_input_grad[0]:
            gr = _c(gr)
            dr = torch.empty_like(recons)
            link = ctx.act_link
            if link is not None:
                _call("movae_recon_loss_bwd_act", recons.data_ptr(), inputs.data_ptr(), gr.data_ptr(), dr.data_ptr(), recons.numel(),
                      L.RECON[ctx.kind], float(ctx.scale_r), L.ACT[link.act], float(link.slope), _st(recons))
                link.applied = dr.data_ptr()
            else:
                _call("movae_recon_loss_bwd", recons.data_ptr(), inputs.data_ptr(), gr.data_ptr(), dr.data_ptr(), recons.numel(),
                      L.RECON[ctx.kind], float(ctx.scale_r), _st(recons))
        if gk is not None and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]):
            gk = _c(gk)
            b, d = mu.shape
            dmu, dlv = installed(True).cotangent(mu.data_ptr(), mu), installed(True).cotangent(log_var.data_ptr(), mu)
            _call("movae_kl_bwd", mu.data_ptr(), log_var.data_ptr(), gk.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), b, d,
                  float(ctx.scale_k), _st(mu))
        return dr, None, None, None, dmu, dlv, None, None


def vae_losses(recons, inputs, kind, scale_r, mu, log_var, scale_k, act_link=None):
    return VAELosses.apply(recons, inputs, kind, scale_r, mu, log_var, scale_k, act_link)


class RecursiveLosses(Function):
    """loss_function of the recursive-KL / cycle / recursive-cyclic VAEs (models/recursive_vaes.py) in two launches forward and
    one backward: w_rec * mean(objective(recons, inputs)); anneal * w_kl * kl(mu_hat, log_var_hat) when mu_hat is given; w_cyc *
    mean_b sum_d (z_prior - mu_gen)^2 when z_prior is given; and their fp32 sum.  Returns those K + 1 scalars (adjacent in one
    buffer).  `anneal`: (iter_dev or None, host factor, steps, training) -- with iter_dev the counter is advanced and the factor
    formed inside the final kernel (graph mode), else the host factor is used; eval mode (training False) uses 1.  The backward
    serves whichever cotangents arrive and writes only the cotangents they reach."""

    @staticmethod
    def forward(ctx, recons, inputs, kind, w_rec, mu_hat, log_var_hat, w_kl, anneal, z_prior, mu_gen, w_cyc):
        ctx.set_materialize_grads(False)
        L.require_gpu(recons)
        recons, inputs = _c(recons), _c(inputs)
        assert recons.shape == inputs.shape, (recons.shape, inputs.shape)
        has_kl, has_cyc = mu_hat is not None, z_prior is not None
        lat = mu_hat if has_kl else mu_gen
        b, d = lat.shape
        mu_hat, log_var_hat = (_c(mu_hat), _c(log_var_hat)) if has_kl else (None, None)
        z_prior, mu_gen = (_c(z_prior), _c(mu_gen)) if has_cyc else (None, None)
        K = 1 + int(has_kl) + int(has_cyc)
        out = torch.empty(K + 1, dtype=torch.float32, device=recons.device)
        it_dev, host, steps, training = anneal if anneal is not None else (None, 1.0, 1.0, False)
        fac = torch.empty(1, dtype=torch.float32, device=out.device) if has_kl else None
        wsp, wsb = _ws(recons)
        p = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        _call("movae_recursive_losses_fwd", recons.data_ptr(), inputs.data_ptr(), recons.numel(), L.RECON[kind], p(mu_hat), p(log_var_hat),
              p(z_prior), p(mu_gen), b, d, float(w_rec), float(w_kl), float(w_cyc), p(it_dev), float(host), float(steps), int(bool(training)),
              out.data_ptr(), p(fac), wsp, wsb, _st(recons))
        ctx.kind, ctx.w = kind, (float(w_rec), float(w_kl), float(w_cyc))
        ctx.has, ctx.fac, ctx.bd = (has_kl, has_cyc), fac, (b, d)
        ctx.save_for_backward(recons, inputs, mu_hat, log_var_hat, z_prior, mu_gen)
        return tuple(out[k] for k in range(K + 1))

    @staticmethod
    def backward(ctx, *g):
        recons, inputs, mu_hat, log_var_hat, z_prior, mu_gen = ctx.saved_tensors
        has_kl, has_cyc = ctx.has
        g = [None if x is None else _c(x) for x in g]
        g_rec, g_tot = g[0], g[-1]
        g_kl = g[1] if has_kl else None
        g_cyc = g[1 + int(has_kl)] if has_cyc else None
        reach = lambda t: t is not None or g_tot is not None  # noqa: E731
        dr = dmh = dlh = dmg = None
        if reach(g_rec) and ctx.needs_input_grad[0]:
            dr = torch.empty_like(recons)
        if has_kl and reach(g_kl) and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]):
            dmh, dlh = installed(True).cotangent(mu_hat.data_ptr(), mu_hat), installed(True).cotangent(log_var_hat.data_ptr(), mu_hat)
        if has_cyc and reach(g_cyc) and ctx.needs_input_grad[9]:
            dmg = installed(True).cotangent(mu_gen.data_ptr(), mu_gen)
        if dr is None and dmh is None and dmg is None:
            return (None,) * 11
        p = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        b, d = ctx.bd
        _call("movae_recursive_losses_bwd", recons.data_ptr(), inputs.data_ptr(), recons.numel(), L.RECON[ctx.kind], p(mu_hat), p(log_var_hat),
              p(z_prior), p(mu_gen), b, d, ctx.w[0], ctx.w[1], ctx.w[2], p(ctx.fac), p(g_rec), p(g_kl), p(g_cyc), p(g_tot), p(dr), p(dmh),
              p(dlh), p(dmg), _st(recons))
        return dr, None, None, None, dmh, dlh, None, None, None, dmg, None

    #: forward-argument positions of the differentiable inputs: recons, mu_hat, log_var_hat, mu_gen
    _DIFF_ARGS = (0, 4, 5, 9)

    @staticmethod
    @torch.no_grad()
    def input_cotangents(node, outputs):
        """For the Jacobian pull-back (autojac.backward_through): the op's differentiable input tensors that need a gradient and,
        per loss output index in `outputs`, its cotangents of those inputs (a unit cotangent on that output alone) -- the direct
        edges of the loss op only."""
        saved = node.saved_tensors
        by_pos = dict(zip(RecursiveLosses._DIFF_ARGS, (saved[0], saved[2], saved[3], saved[5])))
        live = [p for p in RecursiveLosses._DIFF_ARGS if by_pos[p] is not None and node.needs_input_grad[p]]
        roots = [by_pos[p] for p in live]
        n_out = len(node._input_metadata)
        one = torch.ones((), dtype=torch.float32, device=roots[0].device)
        cots = []
        for k in outputs:
            g = [None] * n_out
            g[k] = one
            res = RecursiveLosses.backward(node, *g)
            cots.append([res[p] for p in live])
        return roots, cots


def recursive_losses(recons, inputs, kind, w_rec, mu_hat=None, log_var_hat=None, w_kl=0.0, anneal=None, z_prior=None, mu_gen=None,
                     w_cyc=0.0):
    return RecursiveLosses.apply(recons, inputs, kind, w_rec, mu_hat, log_var_hat, w_kl, anneal, z_prior, mu_gen, w_cyc)


# ---- the conv Sphere Encoder (models/sphere_encoder.py) ---------------------------------------------------------------------------
SPHERE_EPS = 1e-6  # rms_norm's eps (models/sphere_encoder.py:23)


def _p(t):
    return t.data_ptr() if t is not None else 0


def _sphere_fwd(z, e, u, sigma, state, sched, radius, want):
    """One movae_sphere_latents_fwd launch on z[B][L].  `sigma`: None (the angle schedule from u, given or drawn), a float or a tensor of
    1 or B values (given sigma).  `want`: which of (v, v_noisy, v_noisy_small) to produce.  -> dict of the buffers written."""
    b, l = z.shape
    new = lambda *shape: torch.empty(shape, dtype=z.dtype, device=z.device)  # noqa: E731
    o = {"v": new(b, l) if want[0] else None, "vn": new(b, l) if want[1] else None, "vs": new(b, l) if want[2] else None,
         "inv": new(3, b), "e": e, "u": u, "sigma": None, "sigma_sub": None}
    fixed = sigma is not None
    sig_t, sig_val = (sigma, 0.0) if isinstance(sigma, torch.Tensor) else (None, float(sigma) if fixed else 0.0)
    if sig_t is not None:
        sig_t = _c(sig_t.to(device=z.device, dtype=z.dtype).reshape(-1))
        assert sig_t.numel() in (1, b), f"sigma must hold 1 or {b} values, got {sig_t.numel()}"
    if state is not None:
        assert state.dtype == torch.int64 and state.numel() == 2 and state.device == z.device
        o["e"], o["u"] = new(b, l), new(b, 4)
    if o["e"] is not None:
        o["sigma"] = new(b, 1)
        if not fixed:
            o["sigma_sub"] = new(b, 1)
            assert o["u"].shape == (b, 4) and o["u"].is_contiguous()
        assert o["e"].shape == (b, l) and o["e"].is_contiguous()
    angle_max, mix_prob, mix_min, mix_max = sched
    _call("movae_sphere_latents_fwd", z.data_ptr(), _p(o["e"]), _p(None if fixed else o["u"]), _p(sig_t),
          int(sig_t is not None and sig_t.numel() > 1), sig_val, int(fixed), _p(state), 1, b, l, float(angle_max), float(mix_prob),
          float(mix_min), float(mix_max), float(radius), SPHERE_EPS, _p(o["v"]), _p(o["vn"]), _p(o["vs"]), _p(o["sigma"]),
          _p(o["sigma_sub"]), o["inv"].data_ptr(), _st(z))
    return o


def _sphere_bwd(v, e, sigma, sigma_sub, inv, g_v, g_n, g_s, radius):
    g_v, g_n, g_s = (None if g is None else _c(g) for g in (g_v, g_n, g_s))
    dz = torch.empty_like(v)
    b, l = v.shape
    _call("movae_sphere_latents_bwd", v.data_ptr(), _p(e), _p(sigma), _p(sigma_sub), inv.data_ptr(), _p(g_v), _p(g_n), _p(g_s),
          dz.data_ptr(), b, l, float(radius), _st(v))
    return dz


class SphereLatents(Function):
    """Everything between SphereEncoder's encoder_proj and its two decoder calls (models/sphere_encoder.py:146-162, 196-220) in one
    launch forward and one backward: v = spherify(z), the jitter angle per row -> sigma = tan(angle), sigma_sub = s * sigma, v_noisy =
    spherify(v + sigma e), v_noisy_small = spherify(v + sigma_sub e).  `sched` = (angle_max_deg, mix_prob or 0, mix_min_deg,
    mix_max_deg).  The draws: e [B, L] ~ N(0, I) and u [B, 4] ~ U[0, 1) (angle, mix mask, mix angle, s) are given, or -- `state`, a
    device int64[2] = {seed, draws so far} advanced by the launch -- drawn inside it (graph mode; one such call at a time per
    process, like ReparameterizeRNG).  Returns (v, v_noisy, v_noisy_small, sigma [B, 1], sigma_sub [B, 1], e, u); the last four are
    constants of the tape.  The backward serves whichever of the three cotangents arrive."""

    @staticmethod
    def forward(ctx, z, e, u, state, sched, radius):
        ctx.set_materialize_grads(False)
        L.require_gpu(z)
        z = _c(z)
        assert z.dim() == 2 and ((e is None) == (u is None)) and ((e is None) != (state is None)), "give e and u, or the generator state"
        o = _sphere_fwd(z, None if e is None else _c(e), None if u is None else _c(u), None, state, sched, radius, (True, True, True))
        ctx.radius = radius
        ctx.save_for_backward(o["v"], o["e"], o["sigma"], o["sigma_sub"], o["inv"])
        drawn = (o["e"], o["u"]) if state is not None else ()  # (given draws are the caller's own tensors: sphere_latents hands them back)
        ctx.mark_non_differentiable(o["sigma"], o["sigma_sub"], *drawn)
        return (o["v"], o["vn"], o["vs"], o["sigma"], o["sigma_sub"]) + (drawn or (None, None))

    @staticmethod
    def backward(ctx, g_v, g_n, g_s, *_):
        if (g_v is None and g_n is None and g_s is None) or not ctx.needs_input_grad[0]:
            return (None,) * 6
        v, e, sigma, sigma_sub, inv = ctx.saved_tensors
        return (_sphere_bwd(v, e, sigma, sigma_sub, inv, g_v, g_n, g_s, ctx.radius),) + (None,) * 5


def sphere_latents(z, sched, radius, e=None, u=None, state=None):
    """-> (v, v_noisy, v_noisy_small, sigma, sigma_sub, e, u)"""
    out = SphereLatents.apply(z, e, u, state, sched, radius)
    return out if state is not None else out[:5] + (e, u)


class Spherify(Function):
    """spherify(z) = radius * z / sqrt(mean(z^2) + 1e-6) per row (models/sphere_encoder.py:23-38) and, with `e` and `sigma` (a float, or a
    tensor of 1 or B values), spherify(spherify(z) + sigma * e) (SphereEncoder.spherify with add_noise): the kernels of SphereLatents
    in their clean / given-sigma modes.  sigma and e are constants of the tape."""

    @staticmethod
    def forward(ctx, z, radius, sigma, e):
        ctx.set_materialize_grads(False)
        L.require_gpu(z)
        z = _c(z)
        assert z.dim() == 2 and (sigma is None) == (e is None)
        noisy = e is not None
        keep = noisy and ctx.needs_input_grad[0]  # (the backward recomputes w = v + sigma e from v)
        o = _sphere_fwd(z, _c(e.to(device=z.device, dtype=z.dtype)) if noisy else None, None, sigma, None, (0.0, 0.0, 0.0, 0.0), radius,
                        (not noisy or keep, noisy, False))
        ctx.radius, ctx.noisy = radius, noisy
        ctx.save_for_backward(o["v"], o["e"], o["sigma"], o["inv"])
        return o["vn"] if noisy else o["v"]

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 4
        v, e, sigma, inv = ctx.saved_tensors
        dz = _sphere_bwd(v, e, sigma, None, inv, None, g, None, ctx.radius) if ctx.noisy else _sphere_bwd(v, None, None, None, inv, g, None, None, ctx.radius)
        return dz, None, None, None


def spherify(z, radius, sigma=None, e=None):
    return Spherify.apply(z, radius, sigma, e)


class SphereLosses(Function):
    """SphereEncoder.loss_function (models/sphere_encoder.py:249-283, without the perceptual term) in two launches forward and one
    backward: pix_recon = lam[0] * (w[0] * mean smooth_l1(recons - inputs)), pix_con = lam[1] * (w[1] * mean smooth_l1(x_noisy - sg)),
    lat_con = lam[2] * mean_b(1 - cos(v, v_enc_dec)) and their fp32 sum, adjacent in one buffer.  `sg` is the reference's detached
    reconstruction: None, or a tensor that shares recons's memory, means recons itself, which is then read once for both pixel terms.
    The image tensors share one memory order.  The backward serves whichever cotangents arrive and writes only what they reach;
    pix_con sends nothing to recons."""

    @staticmethod
    def forward(ctx, recons, inputs, x_noisy, v, v_enc_dec, sg, lam, w):
        ctx.set_materialize_grads(False)
        L.require_gpu(recons)
        recons, inputs, x_noisy, v, v_enc_dec = _c(recons), _c(inputs), _c(x_noisy), _c(v), _c(v_enc_dec)
        assert recons.shape == inputs.shape == x_noisy.shape, (recons.shape, inputs.shape, x_noisy.shape)
        assert v.dim() == 2 and v.shape == v_enc_dec.shape, (v.shape, v_enc_dec.shape)
        if sg is not None:
            assert sg.shape == recons.shape and not sg.requires_grad, "sg is the detached reconstruction"
            sg = None if sg.data_ptr() == recons.data_ptr() and sg.stride() == recons.stride() else _c(sg)
        out = torch.empty(4, dtype=torch.float32, device=recons.device)
        b, l = v.shape
        wsp, wsb = _ws(recons)
        ctx.scal = tuple(float(t) for t in (lam[0], w[0], lam[1], w[1], lam[2]))
        _call("movae_sphere_losses_fwd", recons.data_ptr(), inputs.data_ptr(), x_noisy.data_ptr(), _p(sg), recons.numel(), v.data_ptr(),
              v_enc_dec.data_ptr(), b, l, *ctx.scal, out.data_ptr(), wsp, wsb, _st(recons))
        ctx.save_for_backward(recons, inputs, x_noisy, v, v_enc_dec, sg)
        return out[0], out[1], out[2], out[3]

    #: forward-argument positions of the differentiable inputs: recons, x_noisy, v, v_enc_dec
    _DIFF_ARGS = (0, 2, 3, 4)

    @staticmethod
    def backward(ctx, g_rec, g_con, g_lat, g_tot):
        recons, inputs, x_noisy, v, v_enc_dec, sg = ctx.saved_tensors
        g_rec, g_con, g_lat, g_tot = (None if g is None else _c(g) for g in (g_rec, g_con, g_lat, g_tot))
        reach = lambda t: t is not None or g_tot is not None  # noqa: E731
        need = ctx.needs_input_grad
        dr = torch.empty_like(recons) if reach(g_rec) and need[0] else None
        dxn = torch.empty_like(x_noisy) if reach(g_con) and need[2] else None
        dv = torch.empty_like(v) if reach(g_lat) and need[3] else None
        dve = torch.empty_like(v_enc_dec) if reach(g_lat) and need[4] else None
        if dr is None and dxn is None and dv is None and dve is None:
            return (None,) * 8
        b, l = v.shape
        _call("movae_sphere_losses_bwd", recons.data_ptr(), inputs.data_ptr(), x_noisy.data_ptr(), _p(sg), recons.numel(), v.data_ptr(),
              v_enc_dec.data_ptr(), b, l, *ctx.scal, _p(g_rec), _p(g_con), _p(g_lat), _p(g_tot), _p(dr), _p(dxn), _p(dv), _p(dve), _st(recons))
        return dr, None, dxn, dv, dve, None, None, None

    @staticmethod
    @torch.no_grad()
    def input_cotangents(node, outputs):
        """RecursiveLosses.input_cotangents for this op (autojac.backward_through): the differentiable inputs that need a gradient and,
        per loss output index, its cotangents of them."""
        saved = node.saved_tensors
        by_pos = dict(zip(SphereLosses._DIFF_ARGS, (saved[0], saved[2], saved[3], saved[4])))
        live = [p for p in SphereLosses._DIFF_ARGS if node.needs_input_grad[p]]
        roots = [by_pos[p] for p in live]
        one = torch.ones((), dtype=torch.float32, device=saved[0].device)
        cots = []
        for k in outputs:
            g = [None] * 4
            g[k] = one
            res = SphereLosses.backward(node, *g)
            cots.append([res[p] for p in live])
        return roots, cots


def sphere_losses(recons, inputs, x_noisy, v, v_enc_dec, lam, w, sg=None):
    """-> (pix_recon, pix_con, lat_con, total_loss)"""
    return SphereLosses.apply(recons, inputs, x_noisy, v, v_enc_dec, sg, lam, w)


class CombineLosses(Function):
    """The scalar arithmetic of a loss_function (models/vq_vae.py:381-391, vq_vae2.py:313-334, betatc_vae.py:298-324) in one
    launch forward and one backward: `inputs` are device tensors of 1..n fp32 scalars each (T scalars in all, in order), `coef`
    a K x T list of rows, out[k] = f_k * w_k * (sum of the row's terms) and out[K] = out[0] + out[1] + ...  Returns the K + 1
    scalars.  `anneal`: None or (row, iter_dev, steps, training) -- BetaTC's annealing counter on the device.  The backward
    returns a cotangent only for the inputs a present cotangent reaches (the others stay None, so a per-loss backward of
    mtl_backward does not walk the other losses' subgraphs)."""

    @staticmethod
    def forward(ctx, coef, anneal, *inputs):
        ctx.set_materialize_grads(False)
        L.require_gpu(inputs[0])
        inputs = [_c(t) for t in inputs]
        sizes = [t.numel() for t in inputs]
        T, K = sum(sizes), len(coef)
        assert all(len(r) == T for r in coef) and all(t.dtype == torch.float32 for t in inputs), (T, [len(r) for r in coef])
        ptrs = (C.c_void_p * T)(*[t.data_ptr() + 4 * j for t, n in zip(inputs, sizes) for j in range(n)])
        flat = (C.c_float * (K * T))(*[float(c) for r in coef for c in r])
        out = torch.empty(K + 1, dtype=torch.float32, device=inputs[0].device)
        row, it_dev, steps, training = anneal if anneal is not None else (-1, None, 1.0, False)
        fac = torch.empty(1, dtype=torch.float32, device=out.device) if it_dev is not None else None
        # (the host arrays are passed as ctypes objects, not addresses: a recorded call -- bench.py's replay -- keeps them alive)
        _call("movae_combine_losses_fwd", T, ptrs, K, flat, it_dev.data_ptr() if it_dev is not None else 0,
              float(steps), int(row), int(bool(training)), out.data_ptr(), fac.data_ptr() if fac is not None else 0, _st(out))
        ctx.coef, ctx.sizes, ctx.row, ctx.fac, ctx.flat = coef, sizes, int(row), fac, flat
        ctx.shapes = [t.shape for t in inputs]
        return tuple(out[k] for k in range(K + 1))

    @staticmethod
    def backward(ctx, *g):
        K, T = len(ctx.coef), sum(ctx.sizes)
        if all(x is None for x in g):
            return (None,) * (2 + len(ctx.sizes))
        g = [None if x is None else _c(x) for x in g]
        dev = next(x for x in g if x is not None).device
        gp = (C.c_void_p * (K + 1))(*[0 if x is None else x.data_ptr() for x in g])
        gterms = torch.empty(T, dtype=torch.float32, device=dev)
        _call("movae_combine_losses_bwd", T, K, gp, ctx.flat,
              ctx.fac.data_ptr() if ctx.fac is not None else 0, ctx.row, gterms.data_ptr(), _st(gterms))
        reached = [any(ctx.coef[k][t] != 0 and (g[k] is not None or g[K] is not None) for k in range(K)) for t in range(T)]
        grads, off = [], 0
        for i, n in enumerate(ctx.sizes):
            if ctx.needs_input_grad[2 + i] and any(reached[off: off + n]):
                grads.append(gterms[off: off + n].view(ctx.shapes[i]))
            else:
                grads.append(None)
            off += n
        return (None, None, *grads)


def combine_losses(inputs, coef, anneal=None):
    return CombineLosses.apply(coef, anneal, *inputs)


class TCDecomposition(Function):
    """-> tensor [3] = (mi, tc, kld) of models/betatc_vae.py:294-296 (unweighted)."""

    @staticmethod
    def forward(ctx, z, mu, log_var, log_iw):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(z)
        z, mu, log_var, log_iw = _c(z), _c(mu), _c(log_var), _c(log_iw)
        b, d = z.shape
        out = torch.empty(3, dtype=z.dtype, device=z.device)
        lj = torch.empty(b + b * b, dtype=z.dtype, device=z.device)
        lm = torch.empty(b, d, dtype=z.dtype, device=z.device)
        wsp, wsb = _ws(z)
        _call("movae_tc_decomp_fwd", z.data_ptr(), mu.data_ptr(), log_var.data_ptr(), log_iw.data_ptr(), out.data_ptr(),
              lj.data_ptr(), lm.data_ptr(), b, d, wsp, wsb, _st(z))
        ctx.save_for_backward(z, mu, log_var, log_iw, lj, lm)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 4
        z, mu, log_var, log_iw, lj, lm = ctx.saved_tensors
        g = _c(g)
        b, d = z.shape
        dz, dmu, dlv = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        _call("movae_tc_decomp_bwd", z.data_ptr(), mu.data_ptr(), log_var.data_ptr(), log_iw.data_ptr(), lj.data_ptr(),
              lm.data_ptr(), g.data_ptr(), dz.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), b, d, _st(z))
        return dz, dmu, dlv, None


def tc_decomposition(z, mu, log_var, log_iw):
    return TCDecomposition.apply(z, mu, log_var, log_iw)


# ---------------------------------------------------------------------------------------------
class VectorQuantize(Function):
    """x [.., D] latents (NHWC), codebook [K, D] -> (q_st, commitment, embedding, idx, used_count).

    q_st carries the straight-through gradient to x; commitment = mse(q.detach(), x),
    embedding = mse(q, x.detach()) (models/vq_vae.py:51-55)."""

    @staticmethod
    def forward(ctx, x, codebook):
        L.require_gpu(x)
        x, e = _c(x), _c(codebook)
        k, d = e.shape
        rows = x.numel() // d
        q = torch.empty_like(x)
        idx = torch.empty(rows, dtype=torch.int64, device=x.device)
        sse = torch.empty((), dtype=x.dtype, device=x.device)
        used = torch.empty((), dtype=torch.int32, device=x.device)
        mse2 = torch.empty(2, dtype=x.dtype, device=x.device)
        wsp, wsb = _ws(x)
        # commitment = mse(q.detach(), x) and embedding = mse(q, x.detach()): one value, written twice by the finalize kernel
        _call("movae_vq_nearest_fwd_mse", x.data_ptr(), e.data_ptr(), q.data_ptr(), idx.data_ptr(), sse.data_ptr(), used.data_ptr(),
              mse2.data_ptr(), rows, k, d, wsp, wsb, _st(x))
        commitment, embedding = mse2[0], mse2[1]
        ctx.save_for_backward(x, q, idx)
        ctx.x_ptr = x.data_ptr()
        ctx.kd = (k, d)
        ctx.mark_non_differentiable(idx, used)
        ctx.set_materialize_grads(False)  # a loss that does not reach an output hands None (not zeros): that part is skipped
        return q, commitment, embedding, idx, used

    @staticmethod
    def backward(ctx, dq, gc, ge, _gi, _gu):
        x, q, idx = ctx.saved_tensors
        k, d = ctx.kd
        rows = x.numel() // d
        dq = _c(dq) if dq is not None else None
        need_x, need_e = ctx.needs_input_grad
        # a cotangent that reaches neither the straight-through output nor the commitment term (the embedding loss alone) has NO
        # gradient w.r.t. x: None, not a tensor of zeros -- mtl_backward then skips that loss's pull-back through the encoder
        # (a zero Jacobian row costs nothing); likewise no codebook gradient without an embedding-loss cotangent
        dx = installed(True).cotangent(ctx.x_ptr, x) if (need_x and (dq is not None or gc is not None)) else None  # (x is a feature: born stacked)
        de = torch.empty((k, d), dtype=x.dtype, device=x.device) if (need_e and ge is not None) else None
        if dx is None and de is None:
            return None, None
        wsp, wsb = _ws(x)
        _call("movae_vq_bwd", x.data_ptr(), q.data_ptr(), idx.data_ptr(), L.ptr(dq), L.ptr(_c(gc) if gc is not None else None),
              L.ptr(_c(ge) if ge is not None else None), L.ptr(dx), L.ptr(de), rows, k, d, wsp, wsb, _st(x))
        return dx, de


def vector_quantize(x, codebook):
    return VectorQuantize.apply(x, codebook)


# ---------------------------------------------------------------------------------------------
# PixelCNN prior (models/pixelcnn_prior.py)
class EmbeddingLookup(Function):
    """nn.Embedding forward over a [B, H, W] int64 code grid -> NHWC activations [B, H, W, D] (pixelcnn_prior.py:306,371); the
    weight gradient is a fixed-order segmented sum over the sorted codes (no float atomics)."""

    @staticmethod
    def forward(ctx, idx, weight):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(weight)
        idx = idx.contiguous()
        w = _c(weight)
        k, d = w.shape
        y = torch.empty(tuple(idx.shape) + (d,), dtype=w.dtype, device=w.device)
        _call("movae_embedding_fwd", w.data_ptr(), idx.data_ptr(), y.data_ptr(), idx.numel(), k, d, _st(w))
        ctx.save_for_backward(idx)
        ctx.kd = (k, d)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 2
        (idx,) = ctx.saved_tensors
        k, d = ctx.kd
        dy = _c(dy)
        dw = torch.empty((k, d), dtype=dy.dtype, device=dy.device)
        wsp, wsb = _ws(dy)
        _call("movae_embedding_bwd", dy.data_ptr(), idx.data_ptr(), dw.data_ptr(), idx.numel(), k, d, wsp, wsb, _st(dy))
        return None, dw


def embedding(idx, weight):
    return EmbeddingLookup.apply(idx, weight)


class GatedResidual(Function):
    """out = res + gate * feat (gate / feat already activated by the conv epilogues; pixelcnn_prior.py:85-90)."""

    @staticmethod
    def forward(ctx, res, gate, feat):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(res)
        res, gate, feat = _c(res), _c(gate), _c(feat)
        out = torch.empty_like(res)
        _call("movae_gated_residual_fwd", res.data_ptr(), gate.data_ptr(), feat.data_ptr(), out.data_ptr(), res.numel(), _st(res))
        ctx.save_for_backward(gate, feat)
        return out

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * 3
        gate, feat = ctx.saved_tensors
        dout = _c(dout)
        dg, df = torch.empty_like(dout), torch.empty_like(dout)
        _call("movae_gated_residual_bwd", dout.data_ptr(), gate.data_ptr(), feat.data_ptr(), dg.data_ptr(), df.data_ptr(), dout.numel(),
              _st(dout))
        return dout, dg, df


def gated_residual(res, gate, feat):
    assert res.shape == gate.shape == feat.shape and res.numel() % 4 == 0
    return GatedResidual.apply(res, gate, feat)


@torch.no_grad()
def mask_weight_(weight, mask):
    """MaskedConv2d's `self.weight.data *= self.mask` (pixelcnn_prior.py:52): in place, outside the tape.  Both tensors share one
    dense memory layout (channels_last), so the flat product is the element-wise one."""
    L.require_gpu(weight)
    assert weight.shape == mask.shape and weight.stride() == mask.stride(), "mask must share the weight's memory layout"
    _call("movae_mul", weight.data_ptr(), mask.data_ptr(), weight.data_ptr(), weight.numel(), _st(weight))
    return weight


def prior_sample_pack_floats(d0, e, c, layers, k, ks):
    """Length of the packed weight buffer prior_sample_step reads (include/movae.h); 0 for a shape it does not support."""
    return int(L.load().movae_prior_sample_pack_floats(d0, e, c, layers, k, ks))


@torch.no_grad()
def prior_sample_step(wpack, h0, acache, codes, dims, i, j, inv_temperature, seed, draw, sample_base=0, forced=None, uniforms=None,
                      logits_out=None):
    """Raster position (i, j) of cached PixelCNN sampling for every sample of the batch, in one launch and in place: reads the causal
    taps of h0 [B,H,W,D0] and of acache [layers,B,H,W,hidden/2], writes acache, codes [B,H,W] int64 and h0's embedding channels at
    (i, j) (include/movae.h: movae_prior_sample_step; sampling.py drives it).  dims = (embedding_dim, hidden, layers, K, kernel)."""
    L.require_gpu(h0)
    B, H, W, d0 = h0.shape
    e, c, layers, k, ks = dims
    for t, shape, dt in ((wpack, (wpack.numel(),), torch.float32), (acache, (layers, B, H, W, c // 2), torch.float32),
                         (codes, (B, H, W), torch.int64), (forced, (B, H, W), torch.int64), (uniforms, (B, H, W), torch.float32),
                         (logits_out, (B, H, W, k), torch.float32)):
        assert t is None or (tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()), (tuple(t.shape), shape, t.dtype)
    assert h0.dtype == torch.float32 and h0.is_contiguous() and (acache is not None or layers == 0)
    _call("movae_prior_sample_step", wpack.data_ptr(), wpack.numel(), h0.data_ptr(), L.ptr(acache), codes.data_ptr(), L.ptr(forced),
          L.ptr(uniforms), L.ptr(logits_out), B, H, W, d0, e, c, layers, k, ks, i, j, float(inv_temperature), int(seed), int(draw),
          int(sample_base), _st(h0))


def prior_snail_sample_pack_floats(d0, e, c, blocks, res_blocks, heads, head_dim, k, ks):
    """Length of the packed weight buffer prior_snail_sample_step reads (include/movae.h); 0 for a shape it does not support."""
    return int(L.load().movae_prior_snail_sample_pack_floats(d0, e, c, blocks, res_blocks, heads, head_dim, k, ks))


@torch.no_grad()
def prior_snail_sample_step(wpack, h0, acache, kvcache, codes, dims, i, j, inv_temperature, seed, draw, sample_base=0, forced=None,
                            uniforms=None, logits_out=None):
    """Raster position (i, j) of cached PixelSNAIL sampling for every sample of the batch, in one launch and in place: as
    prior_sample_step, and the attention layers' k / v rows of (i, j) go to kvcache [blocks,B,H*W,2*heads*head_dim], whose earlier rows
    they attend over (include/movae.h: movae_prior_snail_sample_step).
    dims = (embedding_dim, hidden, blocks, res_blocks, heads, head_dim, K, kernel)."""
    L.require_gpu(h0)
    B, H, W, d0 = h0.shape
    e, c, nb, nr, heads, hd, k, ks = dims
    for t, shape, dt in ((wpack, (wpack.numel(),), torch.float32), (acache, (nb * nr, B, H, W, c // 2), torch.float32),
                         (kvcache, (nb, B, H * W, 2 * heads * hd), torch.float32), (codes, (B, H, W), torch.int64),
                         (forced, (B, H, W), torch.int64), (uniforms, (B, H, W), torch.float32), (logits_out, (B, H, W, k), torch.float32)):
        assert t is None or (tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()), (tuple(t.shape), shape, t.dtype)
    assert h0.dtype == torch.float32 and h0.is_contiguous() and (acache is not None or nb * nr == 0) and (kvcache is not None or nb == 0)
    _call("movae_prior_snail_sample_step", wpack.data_ptr(), wpack.numel(), h0.data_ptr(), L.ptr(acache), L.ptr(kvcache), codes.data_ptr(),
          L.ptr(forced), L.ptr(uniforms), L.ptr(logits_out), B, H, W, d0, e, c, nb, nr, heads, hd, k, ks, i, j, float(inv_temperature),
          int(seed), int(draw), int(sample_base), _st(h0))


class CrossEntropy(Function):
    """F.cross_entropy(logits[rows, K], target[rows]) with mean reduction (main.py:1003-1006; pixelcnn_prior.py:392-395)."""

    @staticmethod
    def forward(ctx, logits, target):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(logits)
        logits, target = _c(logits), target.contiguous()
        rows, k = logits.shape
        assert target.numel() == rows and target.dtype == torch.int64
        loss = torch.empty((), dtype=logits.dtype, device=logits.device)
        lse = torch.empty(rows, dtype=logits.dtype, device=logits.device)
        wsp, wsb = _ws(logits)
        _call("movae_cross_entropy_fwd", logits.data_ptr(), target.data_ptr(), loss.data_ptr(), lse.data_ptr(), rows, k, wsp, wsb,
              _st(logits))
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 2
        logits, target, lse = ctx.saved_tensors
        g = _c(g)
        rows, k = logits.shape
        dl = torch.empty_like(logits)
        _call("movae_cross_entropy_bwd", logits.data_ptr(), target.data_ptr(), lse.data_ptr(), g.data_ptr(), dl.data_ptr(), rows, k,
              _st(logits))
        return dl, None


def cross_entropy(logits, target):
    return CrossEntropy.apply(logits, target)


# ---------------------------------------------------------------------------------------------
# PixelSNAIL's causal self-attention (models/pixelcnn_prior.py:95-135; csrc/attention.hip)
def _ws_at_least(device, nbytes):
    """The shared workspace when it is large enough, else a buffer of this call's own (the first 4 KiB header stays zero)."""
    w = L.workspace(device)
    if w.numel() >= nbytes:
        return w
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def _same_compute_dtype(name, fwd_dtype):
    """The saved lse carries the forward's rounding: a backward under the other compute dtype would recompute other probabilities."""
    now = L.compute_dtype()
    if now != fwd_dtype:
        raise RuntimeError(f"{name}: the forward ran under compute dtype {fwd_dtype} and the backward finds {now}; "
                           "keep movae_set_compute_dtype unchanged between the two")


class CausalAttention(Function):
    """softmax(mask(Q K^T / sqrt(hd))) with dropout, times V, over the [..., proj] NHWC outputs of the three 1x1 projections; the
    result is [..., proj] in the reference's channel order d * heads + h (pixelcnn_prior.py:130).  The backward regenerates the
    dropout mask from (seed, draw) instead of storing it."""

    @staticmethod
    def forward(ctx, q, k, v, heads, p, seed, draw):
        ctx.set_materialize_grads(False)  # an absent cotangent arrives as None: no zero-fill, no kernels on zeros
        L.require_gpu(q)
        q, k, v = _c(q), _c(k), _c(v)
        assert q.shape == k.shape == v.shape and q.dtype == torch.float32
        proj = q.shape[-1]
        if proj % heads:
            raise ValueError(f"causal_attention: {proj} channels do not split into {heads} heads")
        B = q.shape[0]
        n = q.numel() // (B * proj)
        o = torch.empty_like(q)
        lse = torch.empty((B * heads, n), dtype=q.dtype, device=q.device)
        p = float(p)
        _call("movae_causal_attn_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), proj, o.data_ptr(), lse.data_ptr(), B, heads, n,
              proj // heads, p, seed, draw, _st(q))
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.cfg = (B, heads, n, proj // heads, p, seed, draw)
        ctx.compute_dtype = L.compute_dtype()
        return o

    @staticmethod
    def backward(ctx, do):
        if do is None:
            return (None,) * 7
        q, k, v, o, lse = ctx.saved_tensors
        B, heads, n, hd, p, seed, draw = ctx.cfg
        _same_compute_dtype("causal_attention", ctx.compute_dtype)
        do = _c(do)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = _ws_at_least(q.device, L.load().movae_causal_attn_ws_bytes(B, heads, n))
        _call("movae_causal_attn_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), heads * hd, o.data_ptr(), do.data_ptr(), lse.data_ptr(),
              dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, heads, n, hd, p, seed, draw, ws.data_ptr(), ws.numel(), _st(q))
        return dq, dk, dv, None, None, None, None


def causal_attention(q, k, v, heads, p=0.0, seed=0, draw=0):
    """q, k, v: [B, ..., heads * hd] (NHWC; head h at channels h*hd ..), causal over the flattened positions; p = 0 (or eval mode
    in the caller) takes the no-dropout kernels.  (seed, draw) select the dropout mask (causal_attention_dropout_mask)."""
    return CausalAttention.apply(q, k, v, int(heads), float(p), int(seed), int(draw))


def causal_attention_dropout_mask(bh, n, p, seed, draw, device):
    """The keep mask [bh, n, n] (uint8, 1 = kept) that causal_attention(p, seed, draw) applies (test / measurement hook)."""
    keep = torch.empty((bh, n, n), dtype=torch.uint8, device=device)
    _call("movae_causal_attn_dropout_mask", keep.data_ptr(), bh, n, float(p), int(seed), int(draw), L.stream_ptr(keep.device))
    return keep


# ---------------------------------------------------------------------------------------------
# The transformer operator set of the ViT Sphere Encoder (models/sphere_encoder_vit.py; csrc/attention.hip, csrc/vit.hip).  The
# batched full-Jacobian walker (autojac._batched_pullback) does not cover these ops: their backward_batched says so, and
# autojac.backward_through then takes one autograd pass per loss.
def _no_walker(name):
    def backward_batched(ctx, G, *dy):
        raise NotImplementedError(f"{name}: the batched Jacobian walker does not cover this op; one autograd pass per loss instead")

    return staticmethod(backward_batched)


class Attention(Function):
    """softmax(rope(Q) rope(K)^T / sqrt(hd)) V over the packed projection qkv [B, N, 3C] (q at channel 0, k at C, v at 2C; head h at
    h*hd), read in place; the result is [B, N, C] head-major (AttentionWithRoPE.forward, sphere_encoder_vit.py:157-167).  cos / sin:
    the RoPE tables [N, hd/2] (rope_tables), or None for no rotation.  dqkv comes back as one [B, N, 3C] buffer."""

    @staticmethod
    def forward(ctx, qkv, heads, cos, sin):
        ctx.set_materialize_grads(False)
        L.require_gpu(qkv)
        qkv = _c(qkv)
        assert qkv.dim() == 3 and qkv.dtype == torch.float32, "attention: qkv is the packed fp32 projection [B, N, 3C]"
        B, n, c3 = qkv.shape
        if c3 % 3 or (c3 // 3) % heads:
            raise ValueError(f"attention: {c3} channels do not split into q, k, v of {heads} heads")
        c = c3 // 3
        hd = c // heads
        assert (cos is None) == (sin is None), "attention: give both RoPE tables or neither"
        if cos is not None:
            cos, sin = _c(cos), _c(sin)
            assert cos.shape == sin.shape == (n, hd // 2) and cos.dtype == sin.dtype == torch.float32 and cos.device == qkv.device, \
                f"attention: RoPE tables must be fp32 [{n}, {hd // 2}] on the input's device"
        o = torch.empty((B, n, c), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B * heads, n), dtype=qkv.dtype, device=qkv.device)
        base = qkv.data_ptr()
        _call("movae_attn_fwd", base, base + 4 * c, base + 8 * c, c3, _p(cos), _p(sin), o.data_ptr(), lse.data_ptr(), B, heads, n, hd, 0.0,
              _st(qkv))
        ctx.save_for_backward(qkv, o, lse, cos, sin)
        ctx.cfg = (B, heads, n, hd)
        ctx.compute_dtype = L.compute_dtype()
        return o

    @staticmethod
    def backward(ctx, do):
        if do is None or not ctx.needs_input_grad[0]:
            return (None,) * 4
        qkv, o, lse, cos, sin = ctx.saved_tensors
        B, heads, n, hd = ctx.cfg
        _same_compute_dtype("attention", ctx.compute_dtype)
        c = heads * hd
        do = _c(do)
        dqkv = torch.empty_like(qkv)
        ws = _ws_at_least(qkv.device, L.load().movae_attn_ws_bytes(B, heads, n))
        base, dbase = qkv.data_ptr(), dqkv.data_ptr()
        _call("movae_attn_bwd", base, base + 4 * c, base + 8 * c, 3 * c, _p(cos), _p(sin), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dbase,
              dbase + 4 * c, dbase + 8 * c, B, heads, n, hd, 0.0, ws.data_ptr(), ws.numel(), _st(qkv))
        return dqkv, None, None, None

    backward_batched = _no_walker("Attention")


def attention(qkv, heads, cos=None, sin=None):
    return Attention.apply(qkv, int(heads), cos, sin)


def rope_tables(n, inv_freq, device):
    """(cos, sin) [n, hd/2] of RotaryEmbedding.forward / apply_rotary_pos_emb (sphere_encoder_vit.py:71-106), formed on the CPU in fp32
    with the reference's own expressions -- the kernels' parity with it then rests on no device sincosf -- and moved to `device`."""
    freqs = torch.outer(torch.arange(n, dtype=torch.float32), inv_freq.detach().to(device="cpu", dtype=torch.float32))
    return freqs.cos().contiguous().to(device), freqs.sin().contiguous().to(device)


ROWNORM = {"layer": 0, "rms": 1}


class RowNorm(Function):
    """LayerNorm ("layer": biased variance, weight and bias) or RMSNorm ("rms": x / sqrt(mean(x^2) + eps) * weight) over the last
    dimension of x [..., D]; weight / bias may be None.  `pos` [N, D] (a constant of the tape; the leading dimensions of x flatten to a
    multiple of N rows) is added after the affine: out = norm(x) * w + b + pos[row % N]."""

    @staticmethod
    def forward(ctx, x, weight, bias, pos, mode, eps):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        x = _c(x)
        d = x.shape[-1]
        rows = x.numel() // d
        assert x.dtype == torch.float32 and (weight is None or weight.shape == (d,)) and (bias is None or bias.shape == (d,))
        assert mode in ROWNORM and not (mode == "rms" and bias is not None), "RMSNorm has no bias"
        if pos is not None:
            pos = _c(pos)
            assert pos.dim() == 2 and pos.shape[1] == d and rows % pos.shape[0] == 0 and not pos.requires_grad, "pos is a constant [N, D] table"
        y = torch.empty_like(x)
        rstd = torch.empty(rows, dtype=x.dtype, device=x.device)
        mean = torch.empty(rows, dtype=x.dtype, device=x.device) if mode == "layer" else None
        _call("movae_rownorm_fwd", x.data_ptr(), _p(weight), _p(bias), _p(pos), pos.shape[0] if pos is not None else 0, y.data_ptr(), _p(mean),
              rstd.data_ptr(), rows, d, ROWNORM[mode], float(eps), _st(x))
        ctx.mode = mode
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 6
        x, weight, bias, mean, rstd = ctx.saved_tensors
        dy = _c(dy)
        d = x.shape[-1]
        rows = x.numel() // d
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None
        dw = installed(True).sink(0, weight, (d,)) if weight is not None and need[1] else None
        db = installed(True).sink(0, bias, (d,)) if bias is not None and need[2] else None
        if dx is None and dw is None and db is None:
            return (None,) * 6
        ws = _ws_at_least(x.device, L.load().movae_rownorm_ws_bytes(rows, d))
        _call("movae_rownorm_bwd", dy.data_ptr(), x.data_ptr(), _p(weight), _p(mean), rstd.data_ptr(), _p(dx), _p(dw), _p(db), rows, d,
              ROWNORM[ctx.mode], ws.data_ptr(), ws.numel(), _st(x))
        return dx, dw, db, None, None, None

    backward_batched = _no_walker("RowNorm")


def layer_norm(x, weight=None, bias=None, eps=1e-5, pos=None):
    return RowNorm.apply(x, weight, bias, pos, "layer", eps)


def rms_norm(x, weight=None, eps=1e-6, pos=None):
    return RowNorm.apply(x, weight, None, pos, "rms", eps)


class BiasGelu(Function):
    """gelu(x + bias) with the exact erf form (nn.GELU()), on the BIAS-FREE output x [..., C] of the linear in front; bias [C] or None.
    The backward recomputes x + bias from the saved x, writes dx and -- the bias gradient of that linear -- the column sums of dx."""

    @staticmethod
    def forward(ctx, x, bias):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        x = _c(x)
        c = x.shape[-1]
        assert x.dtype == torch.float32 and (bias is None or bias.shape == (c,))
        y = torch.empty_like(x)
        _call("movae_bias_gelu_fwd", x.data_ptr(), _p(bias), y.data_ptr(), x.numel() // c, c, _st(x))
        ctx.save_for_backward(x, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 2
        x, bias = ctx.saved_tensors
        dy = _c(dy)
        c = x.shape[-1]
        rows = x.numel() // c
        dx = torch.empty_like(x)
        _call("movae_bias_gelu_bwd", dy.data_ptr(), x.data_ptr(), _p(bias), dx.data_ptr(), rows, c, _st(x))
        db = None
        if bias is not None and ctx.needs_input_grad[1]:
            db = installed(True).sink(0, bias, (c,))
            wsp, wsb = _ws(x)
            _call("movae_colsum", dx.data_ptr(), db.data_ptr(), rows, c, 0, wsp, wsb, _st(x))
        return (dx if ctx.needs_input_grad[0] else None), db

    backward_batched = _no_walker("BiasGelu")


def bias_gelu(x, bias=None):
    return BiasGelu.apply(x, bias)


class UnpatchifyAct(Function):
    """tanh(Unpatchify(x)) (sphere_encoder_vit.py:125-140, :388): x [B, N, p*p*C] -> the NHWC image [B, H, W, C]."""

    @staticmethod
    def forward(ctx, x, h, w, c, patch):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        x = _c(x)
        b = x.shape[0]
        assert x.dtype == torch.float32 and h % patch == 0 and w % patch == 0 and x.numel() == b * h * w * c, \
            f"unpatchify: {tuple(x.shape)} is not {h}x{w}x{c} in patches of {patch}"
        y = torch.empty((b, h, w, c), dtype=x.dtype, device=x.device)
        _call("movae_unpatchify_act_fwd", x.data_ptr(), y.data_ptr(), b, h, w, c, patch, _st(x))
        ctx.geom = (b, h, w, c, patch)
        ctx.xshape = tuple(x.shape)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None or not ctx.needs_input_grad[0]:
            return (None,) * 5
        (y,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty(ctx.xshape, dtype=y.dtype, device=y.device)
        _call("movae_unpatchify_act_bwd", dy.data_ptr(), y.data_ptr(), dx.data_ptr(), *ctx.geom, _st(y))
        return (dx,) + (None,) * 4

    backward_batched = _no_walker("UnpatchifyAct")


def unpatchify_act(x, h, w, c, patch):
    return UnpatchifyAct.apply(x, int(h), int(w), int(c), int(patch))


class AddRowsBcast(Function):
    """x [..., N, D] + pos [N, D] (SinusoidalPosEmbedding.forward); pos is a constant of the tape, the backward the identity."""

    @staticmethod
    def forward(ctx, x, pos):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        x, pos = _c(x), _c(pos)
        n, d = pos.shape
        assert x.shape[-1] == d and (x.numel() // d) % n == 0 and not pos.requires_grad
        y = torch.empty_like(x)
        _call("movae_add_rows_bcast", x.data_ptr(), pos.data_ptr(), y.data_ptr(), x.numel() // d, n, d, _st(x))
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, None

    backward_batched = _no_walker("AddRowsBcast")


def add_rows_bcast(x, pos):
    return AddRowsBcast.apply(x, pos)


def token_linear(x, w, b=None):
    """x [..., in], w [out, in] -> [..., out]: a 1x1 convolution over the flattened rows, as `linear` is for two dimensions."""
    fin = x.shape[-1]
    rows = x.numel() // fin
    y = Conv.apply(x.reshape(rows, 1, 1, fin), w.view(w.shape[0], fin, 1, 1), b, 1, 0, 0, False, None, 0.01)
    return y.reshape(*x.shape[:-1], w.shape[0])


# ---- the perceptual loss around its convolutions (csrc/perceptual.hip) ---------------------------------------------------------------
class VggPrep(Function):
    """PerceptualLoss._norm_input (utils/objectives.py:66-72) on G same-shape NHWC images [B, H, W, 3] in two launches for the whole
    group and without a host sync: per tensor, (x + 1) / 2 if any of its elements is negative, clamp to [0, 1], ImageNet mean / std.
    Returns G tensors.  The backward recomputes the clamp mask from the saved x and the saved per-tensor flags (a device int[G]) and
    serves whichever cotangents arrive, in one launch."""

    @staticmethod
    def forward(ctx, *xs):
        ctx.set_materialize_grads(False)
        L.require_gpu(xs[0])
        xs = [_c(x) for x in xs]
        G, first = len(xs), xs[0]
        assert all(x.dtype == torch.float32 and x.shape == first.shape for x in xs) and first.shape[-1] == 3, \
            f"vgg_prep: same-shape fp32 NHWC tensors with 3 channels, got {[tuple(x.shape) for x in xs]}"
        ys = [torch.empty_like(x) for x in xs]
        flags = torch.empty(G, dtype=torch.int32, device=first.device)
        wsp, wsb = _ws(first)
        arr = C.c_void_p * G
        _call("movae_vgg_prep_fwd", G, arr(*[x.data_ptr() for x in xs]), arr(*[y.data_ptr() for y in ys]), flags.data_ptr(),
              first.numel(), wsp, wsb, _st(first))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(flags, *[x if need else None for x, need in zip(xs, ctx.needs_input_grad)])
            # a member that needs no gradient (the input image next to two reconstructions) stays a constant of the tape
            ctx.mark_non_differentiable(*[y for y, need in zip(ys, ctx.needs_input_grad) if not need])
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        live = [dy is not None and need for dy, need in zip(dys, ctx.needs_input_grad)]
        if not any(live):
            return (None,) * len(dys)
        flags, *xs = ctx.saved_tensors
        G = len(dys)
        dys = [_c(dy) if ok else None for dy, ok in zip(dys, live)]
        dxs = [torch.empty_like(x) if ok else None for x, ok in zip(xs, live)]
        arr = C.c_void_p * G
        _call("movae_vgg_prep_bwd", G, arr(*[_p(t) for t in dys]), arr(*[_p(x) if ok else 0 for x, ok in zip(xs, live)]), flags.data_ptr(),
              arr(*[_p(t) for t in dxs]), next(x for x in xs if x is not None).numel(), _st(flags))
        return tuple(dxs)

    backward_batched = _no_walker("VggPrep")


def vgg_prep(*xs):
    """One NHWC image tensor -> its normalised tensor; several -> a tuple, normalised in the same two launches."""
    out = VggPrep.apply(*xs)
    return out[0] if len(xs) == 1 else out


def batch_u8(store, idx, lut, flip, seed, epoch):
    """One batch from a device-resident uint8 image set (csrc/data.hip; data.DeviceBatchLoader): store uint8 [N][H][W][C], idx int32 [B]
    row numbers into it (range-checked by the caller), lut float32 [C][256] -> a fresh fp32 NHWC [B][H][W][C] with
    out[j] = lut[ch][store[idx[j]]], row idx[j] mirrored along W where the Philox bit of (seed, epoch, idx[j]) says so and `flip` is set.
    One launch; not differentiable (a data source)."""
    L.require_gpu(store)
    assert store.dtype == torch.uint8 and store.dim() == 4 and store.is_contiguous(), "batch_u8: store is contiguous uint8 [N][H][W][C]"
    _, h, w, c = store.shape
    assert idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous() and idx.device == store.device, "batch_u8: idx is int32 [B]"
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (c, 256) and lut.is_contiguous() and lut.device == store.device, \
        f"batch_u8: lut is float32 [{c}][256]"
    out = torch.empty((idx.numel(), h, w, c), dtype=torch.float32, device=store.device)
    _call("movae_batch_u8", store.data_ptr(), idx.data_ptr(), idx.numel(), h, w, c, lut.data_ptr(), int(bool(flip)), int(seed), int(epoch),
          out.data_ptr(), _st(store))
    return out


def batch_u8_staged(stage, ids, lut, flip, seed, epoch):
    """The device step of a streamed batch (csrc/data.hip; data.StreamedBatchLoader): stage uint8 [B][H][W][C], the batch's images in
    batch order (a view into a larger staging buffer is fine: only its first byte need not be aligned), ids int32 [B] their dataset
    indices, lut float32 [C][256] -> a fresh fp32 NHWC [B][H][W][C] with out[j] = lut[ch][stage[j]], row j mirrored along W where the
    Philox bit of (seed, epoch, ids[j]) says so and `flip` is set: batch_u8's bits for stage = store[ids].  One launch."""
    L.require_gpu(stage)
    assert stage.dtype == torch.uint8 and stage.dim() == 4 and stage.is_contiguous(), "batch_u8_staged: stage is contiguous uint8 [B][H][W][C]"
    b, h, w, c = stage.shape
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (b,) and ids.is_contiguous() and ids.device == stage.device, \
        f"batch_u8_staged: ids is int32 [{b}]"
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (c, 256) and lut.is_contiguous() and lut.device == stage.device, \
        f"batch_u8_staged: lut is float32 [{c}][256]"
    out = torch.empty((b, h, w, c), dtype=torch.float32, device=stage.device)
    _call("movae_batch_u8_staged", stage.data_ptr(), ids.data_ptr(), b, h, w, c, lut.data_ptr(), int(bool(flip)), int(seed), int(epoch),
          out.data_ptr(), _st(stage))
    return out


def batch_rrc_u8(blob, offsets, dims, boxes, idx, size, channels, kmax, lut, flip, seed, epoch):
    """One RandomResizedCrop batch from a device-resident ragged image set (csrc/data.hip; data.RaggedBatchLoader): blob uint8 (the
    images back to back, HWC), offsets int64 [N] (bytes), dims int32 [N][2] = (h, w), boxes int32 [N][4] = (top, left, bh, bw), idx
    int32 [B] (rows and boxes range-checked by the caller), lut float32 [C][256] -> a fresh fp32 NHWC [B][size][size][C]:
    out[j] = lut[ch][PIL's crop(box).resize((size, size), BICUBIC) of image idx[j]], bit for bit, its columns mirrored where the Philox
    bit of (seed, epoch, idx[j]) says so and `flip` is set.  kmax: 2 ceil(2 max(1, largest crop side / size)) + 1.  The kernel cannot
    check either promise: a crop side over 8 * size, or a kmax below that bound, gives undefined pixels (inside the buffers), not an
    error -- data.RaggedImages is what guarantees both.  One launch; not differentiable (a data source)."""
    L.require_gpu(blob)
    n = offsets.numel()
    assert blob.dtype == torch.uint8 and blob.dim() == 1 and blob.is_contiguous(), "batch_rrc_u8: blob is flat contiguous uint8"
    for t, dt, shape, what in ((offsets, torch.int64, (n,), "offsets is int64 [N]"), (dims, torch.int32, (n, 2), "dims is int32 [N][2]"),
                               (boxes, torch.int32, (n, 4), "boxes is int32 [N][4]"), (idx, torch.int32, (idx.numel(),), "idx is int32 [B]"),
                               (lut, torch.float32, (channels, 256), f"lut is float32 [{channels}][256]")):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == blob.device, f"batch_rrc_u8: {what}"
    out = torch.empty((idx.numel(), size, size, channels), dtype=torch.float32, device=blob.device)
    _call("movae_batch_rrc_u8", blob.data_ptr(), offsets.data_ptr(), dims.data_ptr(), boxes.data_ptr(), idx.data_ptr(), idx.numel(), size,
          channels, kmax, lut.data_ptr(), int(bool(flip)), int(seed), int(epoch), out.data_ptr(), _st(blob))
    return out


def resample_coeffs(in_sizes, out_size, kmax):
    """The coefficient tables of batch_rrc_u8 for the input sizes `in_sizes` (device int32 [n]) at `out_size` output samples, computed
    by the kernel's own routine -> (k int32 [n][out_size][kmax], zero past the last tap; bounds int32 [n][out_size][2] = (first tap,
    taps))."""
    L.require_gpu(in_sizes)
    assert in_sizes.dtype == torch.int32 and in_sizes.dim() == 1 and in_sizes.is_contiguous(), "resample_coeffs: in_sizes is int32 [n]"
    n = in_sizes.numel()
    k = torch.empty((n, out_size, kmax), dtype=torch.int32, device=in_sizes.device)
    bounds = torch.empty((n, out_size, 2), dtype=torch.int32, device=in_sizes.device)
    _call("movae_resample_coeffs", in_sizes.data_ptr(), n, out_size, kmax, k.data_ptr(), bounds.data_ptr(), _st(in_sizes))
    return k, bounds


def check_rows(idx, n):
    """Host-side range check of a row list (a sequence or a CPU tensor) against a store of n rows: ValueError before anything is
    launched.  -> the list as a CPU int32 tensor."""
    t = torch.as_tensor(idx).reshape(-1)
    if t.is_cuda:
        raise TypeError("check_rows: a host row list (a device list was range-checked where it was built)")
    if t.numel() == 0:
        raise ValueError("an empty row list")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"row numbers are integers, got {t.dtype}")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= n:
        raise ValueError(f"row numbers {lo} .. {hi} outside the store's 0 .. {n - 1}")
    return t.to(torch.int32)


def codes_batch(store_top, idx, store_bottom=None, out_top=None, out_bottom=None):
    """One batch of VQ code grids from device-resident stores (csrc/prior.hip: movae_codes_batch; prior.DeviceCodeLoader):
    store_top [N][H][W] and, for the two-level models, store_bottom [N][H2][W2], both int16 or both int32; idx the b row numbers --
    a host sequence / CPU tensor (range-checked here: ValueError, then uploaded) or a device int32 [b] its builder has range-checked.
    -> int64 [b][H][W], or the pair (top, bottom): out[j] = store[idx[j]] widened, both levels in ONE launch.  out_top / out_bottom:
    caller-supplied int64 buffers written in place and returned (a captured step's static inputs); fresh ones otherwise.
    Not differentiable (a data source)."""
    n = store_top.size(0)
    if not (torch.is_tensor(idx) and idx.is_cuda):
        idx = check_rows(idx, n).to(store_top.device)
    L.require_gpu(store_top)
    assert store_top.dtype in (torch.int16, torch.int32) and store_top.dim() == 3 and store_top.is_contiguous(), \
        "codes_batch: store is contiguous int16 / int32 [N][H][W]"
    assert idx.dtype == torch.int32 and idx.dim() == 1 and idx.numel() > 0 and idx.is_contiguous() and idx.device == store_top.device, \
        "codes_batch: idx is int32 [b]"
    b, outs = idx.numel(), []
    for store, out in ((store_top, out_top), (store_bottom, out_bottom)):
        if store is None:
            assert out is None, "codes_batch: an output buffer without its store"
            outs.append(None)
            continue
        assert store.dtype == store_top.dtype and store.dim() == 3 and store.size(0) == n and store.is_contiguous() and \
            store.device == store_top.device, "codes_batch: both stores share dtype, device and row count"
        shape = (b,) + tuple(store.shape[1:])
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=store.device)
        assert out.dtype == torch.int64 and tuple(out.shape) == shape and out.is_contiguous() and out.device == store.device, \
            f"codes_batch: an output buffer is contiguous int64 {shape}"
        outs.append(out)
    lens = [s[0].numel() if s is not None else 0 for s in (store_top, store_bottom)]
    _call("movae_codes_batch", store_top.data_ptr(), L.ptr(store_bottom), 1 if store_top.dtype == torch.int32 else 0, n, lens[0], lens[1],
          idx.data_ptr(), b, outs[0].data_ptr(), L.ptr(outs[1]), _st(store_top))
    return outs[0] if store_bottom is None else (outs[0], outs[1])


class MaxPool2x2(Function):
    """nn.MaxPool2d(kernel_size=2, stride=2) (floor mode) on NHWC [N, H, W, C], C % 4 == 0.  The backward writes every element of dx
    in one launch: dy to the first maximum of each window in scan order (torch's tie rule), zeros elsewhere and in the row / column
    an odd size drops."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        L.require_gpu(x)
        x = _c(x)
        n, h, w, c = x.shape
        assert x.dtype == torch.float32 and c % 4 == 0 and h >= 2 and w >= 2, f"max_pool2x2: fp32 NHWC with C % 4 == 0, got {tuple(x.shape)}"
        y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
        _call("movae_maxpool2x2_fwd", x.data_ptr(), y.data_ptr(), n, h, w, c, _st(x))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None or not ctx.needs_input_grad[0]:
            return None
        x, y = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(x)
        _call("movae_maxpool2x2_bwd", dy.data_ptr(), x.data_ptr(), y.data_ptr(), dx.data_ptr(), *x.shape, _st(x))
        return dx

    backward_batched = _no_walker("MaxPool2x2")


def max_pool2x2(x):
    return MaxPool2x2.apply(x)


# ---- forward-only inference kernels of the Inception-v3 feature stack (csrc/inception.hip; inception.py, metrics.fid) ------------------
# No autograd: the operands are frozen weights and images nobody differentiates.  `out` / `offset`: the NHWC buffer a result is written
# into and the first of its channels the result takes -- a branch of an Inception block writes its slice of the block's concat buffer.
def _infer_operand(t, what):
    L.require_gpu(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor, got {t.dtype} {tuple(t.shape)} (contiguous: {t.is_contiguous()})")
    return t


def _infer_out(out, offset, shape, like):
    n, ho, wo, c = shape
    if out is None:
        if offset:
            raise ValueError("a channel offset needs the buffer it points into")
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    _infer_operand(out, "out")
    if out.dim() != 4 or tuple(out.shape[:3]) != (n, ho, wo) or offset < 0 or out.size(3) < offset + c or out.device != like.device:
        raise ValueError(f"out {tuple(out.shape)} cannot take channels {offset} .. {offset + c} of a [{n}, {ho}, {wo}, .] result")
    return out


def infer_conv2d(x, weight, scale, shift, stride=1, pad=(0, 0), out=None, offset=0):
    """relu(conv(x, weight) * scale + shift) without autograd (movae_infer_conv2d): x NHWC [n, h, w, ci], weight the MEMORY image
    [co, kh, kw, ci], scale / shift [co]; pad = (pad_h, pad_w).  -> out ([n, ho, wo, co] when not given)."""
    x, weight = _infer_operand(x, "x"), _infer_operand(weight, "weight")
    scale, shift = _infer_operand(scale, "scale"), _infer_operand(shift, "shift")
    if x.dim() != 4 or weight.dim() != 4 or weight.size(3) != x.size(3):
        raise ValueError(f"infer_conv2d: x {tuple(x.shape)} (NHWC) and weight {tuple(weight.shape)} ([co, kh, kw, ci]) do not match")
    n, h, w, ci = x.shape
    co, kh, kw, _ = weight.shape
    if scale.numel() != co or shift.numel() != co:
        raise ValueError(f"infer_conv2d: scale / shift must hold {co} elements")
    ph, pw = pad
    ho, wo = conv_out_size(h, kh, stride, ph), conv_out_size(w, kw, stride, pw)
    if ho < 1 or wo < 1:
        raise ValueError(f"infer_conv2d: a {kh} x {kw} kernel (padding {ph}, {pw}) does not fit {h} x {w}")
    out = _infer_out(out, offset, (n, ho, wo, co), x)
    _call("movae_infer_conv2d", x.data_ptr(), weight.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), n, h, w, ci, co, kh, kw,
          int(stride), int(ph), int(pw), out.size(3), int(offset), _st(x))
    return out


def infer_pool3x3(x, mode, out=None, offset=0):
    """mode "max": F.max_pool2d(x, 3, stride=2); mode "avg": F.avg_pool2d(x, 3, stride=1, padding=1) (count_include_pad), on NHWC
    (movae_infer_pool3x3)."""
    x = _infer_operand(x, "x")
    if mode not in ("max", "avg") or x.dim() != 4:
        raise ValueError(f"infer_pool3x3: mode 'max' or 'avg' on an NHWC tensor, got {mode!r} {tuple(x.shape)}")
    n, h, w, c = x.shape
    if mode == "max" and min(h, w) < 3:
        raise ValueError(f"infer_pool3x3: the unpadded 3x3 window does not fit {h} x {w}")
    ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == "max" else (h, w)
    out = _infer_out(out, offset, (n, ho, wo, c), x)
    _call("movae_infer_pool3x3", x.data_ptr(), out.data_ptr(), n, h, w, c, 0 if mode == "max" else 1, out.size(3), int(offset), _st(x))
    return out


def infer_global_mean(x, out=None):
    """NHWC [n, h, w, c] -> [n, c], the mean over the pixels (movae_infer_global_mean)."""
    x = _infer_operand(x, "x")
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    elif tuple(_infer_operand(out, "out").shape) != (n, c) or out.device != x.device:
        raise ValueError(f"infer_global_mean: out must be [{n}, {c}] on the input's device")
    _call("movae_infer_global_mean", x.data_ptr(), out.data_ptr(), n, h * w, c, _st(x))
    return out


INCEPTION_SIDE = 299


RESIZE_FILTERS = {"bicubic": 0, "bilinear": 1}  # include/movae.h: MOVAE_RESIZE_*


def inception_prep(x, out=None, filter="bicubic"):
    """calculate_fid's input pipeline (utils/metrics.py:542-553) in one launch: NCHW [n, 3, h, w] -> NHWC [n, 299, 299, 3] =
    normalize(center_crop(resize(clamp(0.5 x + 0.5, 0, 1), 299, BICUBIC, antialias=True))).  filter="bilinear": the same with
    TF.resize's default filter, calculate_inception_score's pipeline (utils/metrics.py:872-875).  A side above 299 raises
    NotImplementedError (reducing needs a true antialiasing filter)."""
    L.require_gpu(x)
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"inception_prep: filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
    if x.dim() != 4 or x.size(1) != 3:
        raise ValueError(f"inception_prep takes [n, 3, h, w] images, got {tuple(x.shape)}")
    n, _, h, w = x.shape
    if max(h, w) > INCEPTION_SIDE:
        raise NotImplementedError(f"inception_prep: {h} x {w} has a side above {INCEPTION_SIDE}; reducing an image needs an antialiasing "
                                  "filter this build does not have")
    x = x if x.dtype == torch.float32 else x.float()
    x = x.contiguous()
    shape = (n, INCEPTION_SIDE, INCEPTION_SIDE, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(_infer_operand(out, "out").shape) != shape or out.device != x.device:
        raise ValueError(f"inception_prep: out must be {shape} on the input's device")
    if filter == "bicubic":
        _call("movae_inception_prep", x.data_ptr(), out.data_ptr(), n, h, w, _st(x))
    else:
        _call("movae_inception_prep_filter", x.data_ptr(), out.data_ptr(), n, h, w, RESIZE_FILTERS[filter], _st(x))
    return out


# ---- feature-space kernels of the generative evaluation (csrc/gen_metrics.hip; metrics.inception_score / kid_from_features /
# precision_recall_from_features) -------------------------------------------------------------------------------------------------------
def _matrix(t, what):
    _infer_operand(t, what)
    if t.dim() != 2 or t.size(0) < 1 or t.size(1) < 1:
        raise ValueError(f"{what} must be a non-empty [rows, columns] matrix, got {tuple(t.shape)}")
    return t


def linear_softmax(feat, weight, bias, out=None):
    """softmax(feat @ weight.T + bias, dim=1) in fp32 (movae_linear_softmax): feat [n, D], weight [C, D], bias [C] -> [n, C]."""
    feat, weight = _matrix(feat, "feat"), _matrix(weight, "weight")
    _infer_operand(bias, "bias")
    n, d = feat.shape
    c = weight.size(0)
    if weight.size(1) != d or tuple(bias.shape) != (c,) or weight.device != feat.device or bias.device != feat.device:
        raise ValueError(f"linear_softmax: feat {tuple(feat.shape)}, weight {tuple(weight.shape)} and bias {tuple(bias.shape)} do not match")
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=feat.device)
    elif tuple(_infer_operand(out, "out").shape) != (n, c) or out.device != feat.device:
        raise ValueError(f"linear_softmax: out must be [{n}, {c}] on the input's device")
    _call("movae_linear_softmax", feat.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), n, c, d, _st(feat))
    return out


def inception_score_splits(probs, splits=10):
    """-> [splits] fp64 on the device: exp(mean KL(p(y|x) || p(y))) of every split of probs [n, C] (movae_inception_score; split i is
    rows i (n // splits) .. (i + 1) (n // splits), both distributions clipped to [1e-16, 1]).  n >= splits."""
    probs = _matrix(probs, "probs")
    n, c = probs.shape
    splits = int(splits)
    if splits < 1 or n // splits < 1:
        raise ValueError(f"inception_score_splits: {n} rows leave every one of {splits} splits empty")
    out = torch.empty(splits, dtype=torch.float64, device=probs.device)
    _call("movae_inception_score", probs.data_ptr(), n, c, splits, out.data_ptr(), _st(probs))
    return out


def kid_subsets(real, fake, idx_real, idx_fake, gamma, degree=3):
    """-> [S] fp64 on the device: the clamped unbiased MMD^2 of every subset under the kernel (gamma x.y + 1)^degree
    (movae_kid_subsets).  real [nr, D], fake [nf, D]; idx_real / idx_fake [S, m] int32 row numbers on the same device."""
    real, fake = _matrix(real, "real"), _matrix(fake, "fake")
    if real.size(1) != fake.size(1) or fake.device != real.device:
        raise ValueError(f"kid_subsets: real {tuple(real.shape)} and fake {tuple(fake.shape)} do not match")
    for t, what in ((idx_real, "idx_real"), (idx_fake, "idx_fake")):
        L.require_gpu(t)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 2 or t.shape != idx_real.shape or t.device != real.device:
            raise ValueError(f"kid_subsets: {what} must be a contiguous int32 [S, m] tensor on the features' device, got {t.dtype} {tuple(t.shape)}")
    s, m = idx_real.shape
    if s < 1 or m < 2:
        raise ValueError(f"kid_subsets: needs at least one subset of at least two rows, got [{s}, {m}]")
    out = torch.empty(s, dtype=torch.float64, device=real.device)
    _call("movae_kid_subsets", real.data_ptr(), fake.data_ptr(), idx_real.data_ptr(), idx_fake.data_ptr(), real.size(0), fake.size(0), s, m,
          real.size(1), float(gamma), int(degree), out.data_ptr(), _st(real))
    return out


KNN_MAX_K = 8


def knn_rows(a, b, k, exclude_diag=False, tile=None):
    """-> (dist2 [na, k] fp32: every row's k smallest SQUARED Euclidean distances to the rows of b, ascending, clamped at 0;
    idx [na] int32: the row of b nearest to each row of a) without the na x nb matrix (movae_knn_rows).  exclude_diag: leave j == i
    out (a against itself).  tile: 64 or 128 rows of a per block; None lets the library choose."""
    a, b = _matrix(a, "a"), _matrix(b, "b")
    if a.size(1) != b.size(1) or a.device != b.device:
        raise ValueError(f"knn_rows: a {tuple(a.shape)} and b {tuple(b.shape)} do not match")
    na, nb, k = a.size(0), b.size(0), int(k)
    if not 1 <= k <= KNN_MAX_K or nb - int(bool(exclude_diag)) < k:
        raise ValueError(f"knn_rows: k must be 1 .. {KNN_MAX_K} and at most the candidates per row, got k {k} for {nb} rows of b")
    if tile not in (None, 64, 128):
        raise ValueError(f"knn_rows: tile must be None, 64 or 128, got {tile!r}")
    norms = torch.empty(na + nb, dtype=torch.float32, device=a.device)
    dist2 = torch.empty((na, k), dtype=torch.float32, device=a.device)
    idx = torch.empty(na, dtype=torch.int32, device=a.device)
    _call("movae_knn_rows", a.data_ptr(), b.data_ptr(), na, nb, a.size(1), k, int(bool(exclude_diag)), int(tile or 0), norms.data_ptr(),
          dist2.data_ptr(), idx.data_ptr(), _st(a))
    return dist2, idx
