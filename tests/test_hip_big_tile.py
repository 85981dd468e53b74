"""The big implicit-GEMM tiles (csrc/igemm_v2.h: igemm2_fwd / igemm2_bwd / igemm2_wgrad at <128,128>, their bf16-operand
instantiations <128,128,true>, igemm2_fwd / igemm2_bwd <128,64> and igemm2_wgrad<64,128>) through the C entry points, at shapes
of a few ragged tiles: movae_bench_big_tile_min(1) lowers the dispatcher's threshold so that they are reached at all.

Two data sets per case:
  * integers (x, dy in -3..3, w in -2..2, bias in -8..8, LeakyReLU slope 0.5): every operand is a bf16 number, every product and
    every partial sum an integer (a half-integer with the virtual operand) far below 2^24 -- fp32 accumulation is exact in any order,
    through split-K slabs and `accumulate`, and the rounding to bf16 is the identity.  The result must EQUAL the float64 reference,
    in both compute dtypes: any indexing, masking, padding, parity-class, split-boundary or transposition error shows.
  * seeded normal data: relative L2 < 1e-5 against float64 in fp32 mode; in bf16 mode < 1e-5 against the float64 reference of the
    operands rounded to bf16 (RNE, what v_cvt_pk_bf16_f32 does: exact bf16 products accumulated in fp32 are the arithmetic of the
    fp32 kernels) and inside (1e-4, 1e-2) against the unrounded reference (test_hip_bf16.py's window; its lower bound proves that
    rounding happened).  The bias gradient of the conv weight gradient is formed from the fp32 registers before rounding: equal
    bits in both modes.
Every output lies between two guard zones and starts as NaN: finite everywhere afterwards, guards untouched.  Every call must
have dispatched the kernel the case is about (movae_bench_last_kernel).  The float64 reference is a plain tap loop over NHWC
tensors, itself checked against torch (CPU tests at the end, with the other checks of this file's own machinery)."""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

GUARD = 256          # floats before and after every output
SENTINEL = -7777.0
LRELU = 1            # MOVAE_ACT_LRELU
SLOPE = 0.5

# conv: (n, hi, wi, ci, co, k, s, p); transposed conv: (..., output_padding)
CASES = {
    "A": (8, 8, 8, 128, 128, 3, 1, 1),        # whole tiles, the k-aligned loop; wgrad Kl = 512
    "B": (10, 15, 13, 132, 160, 3, 2, 1),     # M = 560, N = 160, Cr = 132 (general k loop, K = 1188); dgrad: odd 15 x 13 grid at stride 2
    "C": (9, 16, 16, 128, 256, 4, 2, 1),      # 4 x 4 taps at stride 2, two column tiles, K = 2048
    "D": (9, 8, 8, 160, 128, 1, 1, 0),        # 1 x 1 taps
    "E": (520, 2, 2, 64, 128, 3, 2, 1),       # 1 x 1 outputs: tap window (K 576 -> 256) forward; zero-tile shortcut of the wgrad
    "T1": (8, 8, 8, 128, 128, 4, 2, 1, 0),    # transposed: fwd = BWD form, dgrad = FWD form, wgrad with the convT mapping
    "T2": (9, 7, 9, 132, 160, 3, 2, 1, 1),    # transposed, everything ragged, output padding
    "BT": (10, 15, 13, 132, 160, 3, 2, 1, 0),  # case B's numbers as a transposed conv (virtual small-side operand)
    "W64": (1, 259, 255, 36, 36, 3, 1, 1),    # igemm2_fwd / igemm2_bwd <128,64>: M = 66045, N = 36 of 64
    "G64": (9, 8, 8, 32, 48, 3, 1, 1),        # igemm2_wgrad<64,128>
}


class Geo:
    def __init__(self, name, case=None):
        c = CASES[name] if case is None else case  # (case: a geometry of another file's, under that file's name for it)
        self.name, self.tr = name, len(c) == 9
        self.n, self.hi, self.wi, self.ci, self.co, self.k, self.s, self.p = c[:8]
        if self.tr:
            self.ho = (self.hi - 1) * self.s - 2 * self.p + self.k + c[8]
            self.wo = (self.wi - 1) * self.s - 2 * self.p + self.k + c[8]
        else:
            self.ho = (self.hi + 2 * self.p - self.k) // self.s + 1
            self.wo = (self.wi + 2 * self.p - self.k) // self.s + 1
        self.wshape = (self.ci, self.k, self.k, self.co) if self.tr else (self.co, self.k, self.k, self.ci)

    def args(self, groups=1):
        return (groups * self.n, self.hi, self.wi, self.ci, self.ho, self.wo, self.co, self.k, self.k, self.s, self.p)


# ---- the float64 reference: tap loops over NHWC tensors ------------------------------------------------------------------------
def _pad(t, p):
    return F.pad(t, (0, 0, p, p, p, p))


def _win(tp, kh, kw, s, h, w):
    return tp[:, kh:kh + s * (h - 1) + 1:s, kw:kw + s * (w - 1) + 1:s, :]


def _gather(big, wt, g, h, w):
    """out[n, a, b, :] = sum_tap big[n, a * s - p + kh, b * s - p + kw, :] @ wt[kh][kw]   (wt [k][k][c_big][c_out])"""
    bp = _pad(big, g.p)
    out = torch.zeros(big.shape[0], h, w, wt.shape[3], dtype=torch.float64)
    for kh in range(g.k):
        for kw in range(g.k):
            out += _win(bp, kh, kw, g.s, h, w) @ wt[kh, kw]
    return out


def _scatter(small, wt, g, H, W):
    """out[n, a * s - p + kh, b * s - p + kw, :] += small[n, a, b, :] @ wt[kh][kw]   (wt [k][k][c_small][c_out]; out H x W)"""
    h, w = small.shape[1:3]
    op = torch.zeros(small.shape[0], H + 2 * g.p, W + 2 * g.p, wt.shape[3], dtype=torch.float64)
    for kh in range(g.k):
        for kw in range(g.k):
            _win(op, kh, kw, g.s, h, w).add_(small @ wt[kh, kw])
    return op[:, g.p:g.p + H, g.p:g.p + W, :].contiguous()


def _outer(small, big, g):
    """dW[a][kh][kw][b] = sum_pixels small[.., a] * big[pixel * s - p + tap][b]"""
    h, w = small.shape[1:3]
    bp = _pad(big, g.p)
    sm = small.reshape(-1, small.shape[3]).t()
    out = torch.zeros(small.shape[3], g.k, g.k, big.shape[3], dtype=torch.float64)
    for kh in range(g.k):
        for kw in range(g.k):
            out[:, kh, kw, :] = sm @ _win(bp, kh, kw, g.s, h, w).reshape(-1, big.shape[3])
    return out


def lrelu(z, slope):
    return torch.where(z > 0, z, z * slope)


def virt(x, nrm):
    """The virtual operand: x -> LeakyReLU(scale[c] * x + shift[c]) in float64 (padding is added afterwards and stays zero)."""
    if nrm is None:
        return x.double()
    scale, shift, slope = nrm
    return lrelu(x.double() * scale.double() + shift.double(), slope)


def ref_fwd(g, x, w, b=None, slope=None):
    """x float64 NHWC (already transformed / rounded as the caller wants), w in its memory layout."""
    x, w = x.double(), w.double()
    if g.tr:
        y = _scatter(x, w.permute(1, 2, 0, 3), g, g.ho, g.wo)   # w [ci][k][k][co]
    else:
        y = _gather(x, w.permute(1, 2, 3, 0), g, g.ho, g.wo)    # w [co][k][k][ci]
    if b is not None:
        y = y + b.double()
    return y if slope is None else lrelu(y, slope)


def ref_dgrad(g, dy, w):
    dy, w = dy.double(), w.double()
    if g.tr:
        return _gather(dy, w.permute(1, 2, 3, 0), g, g.hi, g.wi)
    return _scatter(dy, w.permute(1, 2, 0, 3), g, g.hi, g.wi)


def ref_wgrad(g, dy, x):
    """One cotangent group: (dW in the weight's memory layout, dbias)."""
    dy, x = dy.double(), x.double()
    dw = _outer(x, dy, g) if g.tr else _outer(dy, x, g)
    return dw, dy.reshape(-1, g.co).sum(0)


def rb(t):
    """Round to bf16 (RNE) and back."""
    return t.float().bfloat16().double()


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


# ---- data -----------------------------------------------------------------------------------------------------------------------
_DATA = {}


def data(name, kind, groups=1, grid=False):
    """(x, dy, w, bias) float32 on the CPU, the same for every test of a case.  grid: x on a 2^-10 grid below 4 (virtual operand)."""
    key = (name, kind, groups, grid)
    if key not in _DATA:
        g = Geo(name)
        gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)) + groups)
        xs, dys = (g.n, g.hi, g.wi, g.ci), (groups * g.n, g.ho, g.wo, g.co)
        if kind == "int":
            x = torch.randint(-3, 4, xs, generator=gen).float()
            dy = torch.randint(-3, 4, dys, generator=gen).float()
            w = torch.randint(-2, 3, g.wshape, generator=gen).float()
            b = torch.randint(-8, 9, (g.co,), generator=gen).float()
        else:
            x = torch.randn(xs, generator=gen)
            dy = torch.randn(dys, generator=gen)
            w = torch.randn(g.wshape, generator=gen) * float(g.ci * g.k * g.k) ** -0.5
            b = torch.randn(g.co, generator=gen) * 0.1
            if grid:
                x = ((x * 1024).round() / 1024).clamp(-3.75, 3.75)
        _DATA[key] = (x, dy, w, b)
    return _DATA[key]


def norm_params(c, kind, seed):
    """(scale, shift, slope) of a virtual operand whose transform is exact in fp32, fused to an fma or not."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "int":
        scale = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (c,), generator=gen)]
        shift = torch.randint(-2, 3, (c,), generator=gen).float()
        return scale, shift, 0.5
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=gen)]
    shift = (torch.randn(c, generator=gen) * 1024).round() / 1024
    return scale, shift, 0.25


_REF = {}


def memo(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


# ---- GPU plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(gpu_device):
    import movae_amd
    import movae_amd._lib as lib

    movae_amd.load_library()
    return lib


@contextlib.contextmanager
def pinned(L, big_tile_min, split):
    lib = L.load()
    kgemm, big, sp = lib.movae_bench_force_kgemm(-1), lib.movae_bench_big_tile_min(big_tile_min), lib.movae_bench_force_split(split)
    try:
        yield lib
    finally:
        lib.movae_bench_force_split(sp)
        lib.movae_bench_big_tile_min(big)
        lib.movae_bench_force_kgemm(kgemm)


@pytest.fixture
def big(L):
    """No block-internal split-K family, the big tiles from one work item on, split factor 1 (a case that asks for another pins
    it through the library handle this yields; all three settings are restored afterwards)."""
    with pinned(L, 1, 1) as lib:
        yield lib


@pytest.fixture
def tiled(L):
    """The same without the threshold hook: the dispatcher's own choice between the tiles."""
    with pinned(L, 0, 1) as lib:
        yield lib


@pytest.fixture(params=["f32", "bf16"])
def dtype(request, L):
    prev = L.set_compute_dtype(request.param)
    try:
        yield request.param
    finally:
        L.set_compute_dtype(prev)


@contextlib.contextmanager
def mode(L, name):
    prev = L.set_compute_dtype(name)
    try:
        yield
    finally:
        L.set_compute_dtype(prev)


def kern(form, dtype, tile="128,128"):
    return f"igemm2_{form}<{tile}{',true' if dtype == 'bf16' else ''}>"


class Out:
    """An output between two guard zones: NaN (or `init`) inside, the sentinel around it.  off: floats past a 16-byte boundary."""

    def __init__(self, shape, dev, init=None, off=0):
        n = 1
        for d in shape:
            n *= d
        self.lo = GUARD + off
        self.buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=dev)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        assert self.t.data_ptr() % 16 == 4 * off
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def get(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        lo, hi = self.buf[:self.lo], self.buf[self.lo + n:]
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{what}: a store outside the output"
        bad = ~torch.isfinite(self.t)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements unwritten or not finite, first at flat index {int(bad.flatten().nonzero()[0])}"
        return self.t.cpu()


WS_HEADER = 4096 // 4  # floats of the workspace header (include/movae.h): zero; the split-K slabs start right behind it


class Scratch:
    """A workspace of the test's own whose scratch starts as NaN: what a call wrote there tells how many split-K slabs it used.
    The kernel's name does not change with the split factor, so this is what shows that a pinned factor reached the launch."""

    def __init__(self, dev, floats=1 << 21):
        self.buf = torch.full((WS_HEADER + floats,), float("nan"), device=dev)
        self.buf[:WS_HEADER].zero_()

    def data_ptr(self):
        return self.buf.data_ptr()

    def numel(self):
        return self.buf.numel() * 4  # bytes, as L.workspace()

    def slabs(self, per_slab, start=0, stop=None):
        """Slabs of `per_slab` floats that were written to: the last one may be ragged (rows past M are not stored), so the
        count is taken from the last float written.  start, stop: the region of the scratch to look at, in floats (a paired
        call keeps its input gradient's slabs in front of its weight gradient's)."""
        torch.cuda.synchronize()
        written = (~torch.isnan(self.buf[WS_HEADER:][start:stop])).nonzero()
        return 0 if written.numel() == 0 else -(-(int(written[-1]) + 1) // per_slab)


def fuse_of(L, nrm, dev, f=None):
    """f: a movae_fuse_t of the caller's with further requests, which gets the transform added."""
    if nrm is None:
        return f, ()
    sc, sh = nrm[0].to(dev), nrm[1].to(dev)
    f = f or L.MovaeFuse()
    f.in_scale, f.in_shift, f.in_slope = sc.data_ptr(), sh.data_ptr(), nrm[2]
    return f, (sc, sh)


def last(lib):
    return lib.movae_bench_last_kernel().decode()


def last_reduce(lib):
    """The split-K reduce kernels chosen since the previous read, " + "-joined ("": none); reading clears the list."""
    return lib.movae_bench_last_reduce().decode()


def put(t, dev, off=False):
    """t on the device; off: the same values one float past a 16-byte boundary, a view into a larger buffer."""
    if not off:
        return t.to(dev)
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def run_fwd(L, lib, dev, g, x, w, b, expect, nrm=None, act=True, ws=None, fuse=None, off=""):
    """b None: no bias.  fuse: a movae_fuse_t with side-product requests (the caller reads its out fields afterwards).
    off: which of "x", "w", "y" lie one float past a 16-byte boundary, e.g. "xw"."""
    xd, wd, bd = put(x, dev, "x" in off), put(w, dev, "w" in off), None if b is None else b.to(dev)
    y = Out((g.n, g.ho, g.wo, g.co), dev, off="y" in off)
    ws, st = ws or L.workspace(dev), torch.cuda.current_stream().cuda_stream
    f, keep = fuse_of(L, nrm, dev, fuse)
    pre = "movae_convT2d_fwd" if g.tr else "movae_conv2d_fwd"
    head = (xd.data_ptr(), wd.data_ptr(), None if bd is None else bd.data_ptr(), y.ptr(), *g.args(), LRELU if act else 0, SLOPE, ws.data_ptr(), ws.numel(), st)
    if f is None:
        L.call(pre, *head)
    else:
        L.call(pre + "_f", *head, C.byref(f))
    assert last(lib) == expect
    return y.get(f"{g.name} forward")


def run_dgrad(L, lib, dev, g, dy, w, expect, groups=1, ws=None, fuse=None, off=""):
    """off: which of "w" and "y" (the result, dx) lie one float past a 16-byte boundary."""
    dyd, wd = dy.to(dev), put(w, dev, "w" in off)
    dx = Out((groups * g.n, g.hi, g.wi, g.ci), dev, off="y" in off)
    ws, st = ws or L.workspace(dev), torch.cuda.current_stream().cuda_stream
    pre = "movae_convT2d_dgrad" if g.tr else "movae_conv2d_dgrad"
    head = (dyd.data_ptr(), wd.data_ptr(), dx.ptr(), *g.args(groups), ws.data_ptr(), ws.numel(), st)
    if groups == 1 and fuse is None:
        L.call(pre, *head)
    else:
        L.call(pre + "_f", *head, None if fuse is None else C.byref(fuse), groups)
    assert last(lib) == expect
    return dx.get(f"{g.name} input gradient")


def run_wgrad(L, lib, dev, g, dy, x, expect, groups=1, nrm=None, init=None, bias=True, ws=None, off=""):
    """-> ([dW per group], [dbias per group] or None); init = ([dW0 per group], [db0 per group]): accumulate into them.
    off: "x" puts x one float past a 16-byte boundary, "d" every dW."""
    dyd, xd = dy.to(dev), put(x, dev, "x" in off)
    dws = [Out(g.wshape, dev, None if init is None else init[0][i], off=1 if "d" in off else 0) for i in range(groups)]
    dbs = [Out((g.co,), dev, None if init is None else init[1][i]) for i in range(groups)] if bias else None
    arr = C.c_void_p * groups
    dwp = arr(*[o.ptr() for o in dws])
    dbp = arr(*[o.ptr() for o in dbs]) if bias else None
    ws, st = ws or L.workspace(dev), torch.cuda.current_stream().cuda_stream
    f, keep = fuse_of(L, nrm, dev)
    pre = "movae_convT2d_wgrad_grouped" if g.tr else "movae_conv2d_wgrad_grouped"
    head = (groups, dyd.data_ptr(), xd.data_ptr(), dwp, dbp, *g.args(), 0 if init is None else 1, ws.data_ptr(), ws.numel(), st)
    if f is None:
        L.call(pre, *head)
    else:
        L.call(pre + "_f", *head, C.byref(f))
    assert last(lib) == expect
    return ([o.get(f"{g.name} weight gradient {i}") for i, o in enumerate(dws)],
            [o.get(f"{g.name} bias gradient {i}") for i, o in enumerate(dbs)] if bias else None)


def run_pair(L, lib, dev, g, dy, w, x, expect, groups=1, init=None, ws=None):
    """The paired entry point (input gradient over all groups + grouped weight gradient with bias gradient of one layer):
    -> (dx, [dW per group], [dbias per group])."""
    dyd, wd, xd = dy.to(dev), w.to(dev), x.to(dev)
    dx = Out((groups * g.n, g.hi, g.wi, g.ci), dev)
    dws = [Out(g.wshape, dev, None if init is None else init[0][i]) for i in range(groups)]
    dbs = [Out((g.co,), dev, None if init is None else init[1][i]) for i in range(groups)]
    arr = C.c_void_p * groups
    dwp, dbp = arr(*[o.ptr() for o in dws]), arr(*[o.ptr() for o in dbs])
    ws, st = ws or L.workspace(dev), torch.cuda.current_stream().cuda_stream
    pre = "movae_convT2d_dgrad_wgrad_grouped" if g.tr else "movae_conv2d_dgrad_wgrad_grouped"
    L.call(pre, groups, dyd.data_ptr(), wd.data_ptr(), xd.data_ptr(), dx.ptr(), dwp, dbp, *g.args(), 0 if init is None else 1,
           ws.data_ptr(), ws.numel(), st)
    assert last(lib) == expect
    return (dx.get(f"{g.name} input gradient (paired)"), [o.get(f"{g.name} weight gradient {i} (paired)") for i, o in enumerate(dws)],
            [o.get(f"{g.name} bias gradient {i} (paired)") for i, o in enumerate(dbs)])


def judge(what, got, ref, ops, dtype, kind, refkey=None):
    """ref(*ops) -> float64 reference from float32 / float64 CPU operands; ops: the two operands the kernel rounds in bf16 mode.
    refkey: the name under which the references are shared (cases that differ in the split factor only compute them once)."""
    key = (refkey or what, kind)
    if kind == "int":
        want = memo(key + ("exact",), lambda: ref(*ops)).float()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{what} [{dtype}]: {bad.shape[0]} of {got.numel()} elements differ from the exact result, first at "
                                 f"{bad[0].tolist()} (got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])}), last at {bad[-1].tolist()}")
        return
    plain = rel(got, memo(key + ("plain",), lambda: ref(*ops)))
    if dtype == "f32":
        print(f"[big tile] {what} f32: rel-L2 {plain:.2e}")
        assert plain < 1e-5, (what, plain)
        return
    rounded = rel(got, memo(key + ("rounded",), lambda: ref(*[rb(o) for o in ops])))
    print(f"[big tile] {what} bf16: rel-L2 {rounded:.2e} against rounded operands, {plain:.2e} against unrounded")
    assert rounded < 1e-5, (what, rounded)
    assert 1e-4 < plain < 1e-2, (what, plain)


def judge_bias_grad(what, got, dy, kind, dtype):
    """Column sums of the unrounded cotangent, in either mode."""
    want = dy.double().reshape(-1, dy.shape[-1]).sum(0)
    if kind == "int":
        assert torch.equal(got, want.float()), f"{what} [{dtype}]: bias gradient differs from the exact column sums"
    else:
        e = rel(got, want)
        print(f"[big tile] {what} {dtype} bias gradient: rel-L2 {e:.2e}")
        assert e < 1e-5, (what, e)


KINDS = ["int", "normal"]
FWD_FORM = {False: "fwd", True: "bwd"}  # gather form of the forward pass by `transposed`; the input gradient takes the other one


def fwd_kernel(g, dtype):
    return kern(FWD_FORM[g.tr], dtype)


def dgrad_kernel(g, dtype):
    return kern(FWD_FORM[not g.tr], dtype)


def check_fwd(L, lib, dev, name, kind, dtype, tag="", ws=None):
    g = Geo(name)
    x, _, w, b = data(name, kind)
    y = run_fwd(L, lib, dev, g, x, w, b, fwd_kernel(g, dtype), ws=ws)
    judge(f"{name} forward{tag}", y, lambda xx, ww: ref_fwd(g, xx, ww, b, SLOPE), (x, w), dtype, kind, f"{name} forward")


def check_dgrad(L, lib, dev, name, kind, dtype, tag="", groups=1, ws=None):
    g = Geo(name)
    _, dy, w, _ = data(name, kind, groups)
    dx = run_dgrad(L, lib, dev, g, dy, w, dgrad_kernel(g, dtype), groups, ws=ws)
    judge(f"{name} input gradient{tag}", dx, lambda d, ww: ref_dgrad(g, d, ww), (dy, w), dtype, kind, f"{name} input gradient {groups}")


def check_wgrad(L, lib, dev, name, kind, dtype, tag="", groups=1, bias=True, ws=None):
    g = Geo(name)
    x, dy, _, _ = data(name, kind, groups)
    dws, dbs = run_wgrad(L, lib, dev, g, dy, x, kern("wgrad", dtype), groups, bias=bias, ws=ws)
    dyg = dy.view(groups, g.n, g.ho, g.wo, g.co)
    for i in range(groups):
        judge(f"{name} weight gradient{tag}" + (f" group {i}" if groups > 1 else ""), dws[i], lambda d, xx: ref_wgrad(g, d, xx)[0],
              (dyg[i], x), dtype, kind, f"{name} weight gradient {groups} {i}")
        if bias:
            judge_bias_grad(f"{name}{tag} group {i}", dbs[i], dyg[i], kind, dtype)
    if bias and dtype == "bf16" and not g.tr:  # the column sums leave the fp32 registers before the rounding: same bits in fp32 mode
        with mode(L, "f32"):
            _, dbs32 = run_wgrad(L, lib, dev, g, dy, x, kern("wgrad", "f32"), groups)
        for i in range(groups):
            assert torch.equal(dbs[i], dbs32[i]), f"{name}{tag}: bias gradient of group {i} differs between the compute dtypes"
    return dws


def slab_floats(g, op):
    """Floats of one split-K slab: the output; the conv weight gradient keeps its bias-gradient partial (one float per row of
    dW, i.e. per output channel) behind each slab, the transposed one takes its bias gradient from another kernel."""
    if op == "fwd":
        return g.n * g.ho * g.wo * g.co
    if op == "dgrad":
        return g.n * g.hi * g.wi * g.ci
    return g.co * g.k * g.k * g.ci + (0 if g.tr else g.co)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "T1", "T2"])
def test_forward(L, big, gpu_device, dtype, name, kind):
    check_fwd(L, big, gpu_device, name, kind, dtype)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "T1", "T2"])  # (E's input gradient has 64 columns: not a big tile)
def test_input_gradient(L, big, gpu_device, dtype, name, kind):
    check_dgrad(L, big, gpu_device, name, kind, dtype)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "T1", "T2"])
def test_weight_gradient(L, big, gpu_device, dtype, name, kind):
    check_wgrad(L, big, gpu_device, name, kind, dtype)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_weight_gradient_zero_tile_shortcut(L, big, gpu_device, dtype, kind):
    """Case E without a bias gradient (with one, the first column tile stages its operand for the column sums): a 1 x 1 small
    side meets tap (kh, kw) at pixel (kh - 1, kw - 1) only, so the taps of row 0 and column 0 multiply padding alone; column tile
    0 holds taps (0, 0) and (0, 1) and is stored as zeros without a reduction."""
    dw = check_wgrad(L, big, gpu_device, "E", kind, dtype, tag=" (no bias)", bias=False)[0]
    assert bool((dw[:, 0, :, :] == 0).all()) and bool((dw[:, :, 0, :] == 0).all())
    assert bool((dw[:, 1:, 1:, :] != 0).any())


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("name", ["B", "T2"])
def test_split_k(L, big, gpu_device, dtype, name, op, kind):
    """Three slabs and the reduce; the forward runs with bias and activation, which the reduce then applies.  (The input
    gradient splits its heaviest parity class in three and the lighter ones in fewer.)"""
    big.movae_bench_force_split(3)
    ws = Scratch(gpu_device)
    {"fwd": check_fwd, "dgrad": check_dgrad, "wgrad": check_wgrad}[op](L, big, gpu_device, name, kind, dtype, tag=" (split 3)", ws=ws)
    assert ws.slabs(slab_floats(Geo(name), op)) == 3


@gpu
def test_forward_takes_the_tap_window(L, big, gpu_device, dtype):
    """Case E's forward with one 32-deep k stage per slab: the tap window leaves K = 2 * 2 * 64 = 256, eight stages, where the
    plain loop over all nine taps (K = 576) would have eighteen."""
    big.movae_bench_force_split(256)
    ws = Scratch(gpu_device)
    check_fwd(L, big, gpu_device, "E", "int", dtype, tag=" (one k stage per slab)", ws=ws)
    assert ws.slabs(slab_floats(Geo("E"), "fwd")) == 8


@gpu
@pytest.mark.parametrize("split", [1, 3])
def test_accumulate(L, big, gpu_device, dtype, split):
    big.movae_bench_force_split(split)
    g = Geo("B")
    x, dy, _, _ = data("B", "int")
    gen = torch.Generator().manual_seed(5)
    dw0, db0 = torch.randint(-5, 6, g.wshape, generator=gen).float(), torch.randint(-5, 6, (g.co,), generator=gen).float()
    ws = Scratch(gpu_device)
    dws, dbs = run_wgrad(L, big, gpu_device, g, dy, x, kern("wgrad", dtype), init=([dw0], [db0]), ws=ws)
    assert ws.slabs(slab_floats(g, "wgrad")) == split  # accumulate goes through the slabs and the reduce at any split factor
    dw, db = memo(("B wgrad", "int", "both"), lambda: ref_wgrad(g, dy, x))
    assert torch.equal(dws[0], (dw0.double() + dw).float()), "accumulated weight gradient"
    assert torch.equal(dbs[0], (db0.double() + db).float()), "accumulated bias gradient"


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["dgrad", "wgrad"])
def test_cotangent_groups(L, big, gpu_device, dtype, op, kind):
    """Two stacked cotangents: one input-gradient launch over both, two weight gradients from a shared x."""
    {"dgrad": check_dgrad, "wgrad": check_wgrad}[op](L, big, gpu_device, "B", kind, dtype, tag=" (2 groups)", groups=2)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op,name", [("fwd", "B"), ("wgrad", "B"), ("wgrad", "BT"), ("wgrad", "T2")])
def test_virtual_operand(L, big, gpu_device, dtype, op, name, kind):
    """BatchNorm + LeakyReLU applied to x on load: gathered operand of the forward and of the conv weight gradient (side 2), small
    side of the transposed-conv weight gradient (side 1).  Padding is non-trivial and the shift non-zero: a transform applied to
    padding shows.  Scale, shift, slope and (normal data) x are chosen so that the transform is exact in fp32."""
    g = Geo(name)
    x, dy, w, b = data(name, kind, grid=True)
    nrm = norm_params(g.ci, kind, 77)
    xv = virt(x, nrm)  # float64, exact
    if op == "fwd":
        y = run_fwd(L, big, gpu_device, g, x, w, b, fwd_kernel(g, dtype), nrm=nrm)
        judge(f"{name} forward (virtual x)", y, lambda xx, ww: ref_fwd(g, xx, ww, b, SLOPE), (xv, w), dtype, kind)
    else:
        dws, dbs = run_wgrad(L, big, gpu_device, g, dy, x, kern("wgrad", dtype), nrm=nrm)
        judge(f"{name} weight gradient (virtual x)", dws[0], lambda d, xx: ref_wgrad(g, d, xx)[0], (dy, xv), dtype, kind)
        judge_bias_grad(f"{name} (virtual x)", dbs[0], dy, kind, dtype)
        if dtype == "bf16" and not g.tr:  # in-kernel column sums of dy, taken before the rounding: same bits in fp32 mode
            with mode(L, "f32"):
                _, dbs32 = run_wgrad(L, big, gpu_device, g, dy, x, kern("wgrad", "f32"), nrm=nrm)
            assert torch.equal(dbs[0], dbs32[0]), f"{name} (virtual x): bias gradient differs between the compute dtypes"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_128x64_tiles(L, tiled, gpu_device, kind):
    """fp32 only (no bf16 form), and reached without the threshold hook: 66045 rows, 36 of 64 columns."""
    name, g = "W64", Geo("W64")
    x, dy, w, b = data(name, kind)
    y = run_fwd(L, tiled, gpu_device, g, x, w, b, "igemm2_fwd<128,64>")
    judge(f"{name} forward <128,64>", y, lambda xx, ww: ref_fwd(g, xx, ww, b, SLOPE), (x, w), "f32", kind)
    dx = run_dgrad(L, tiled, gpu_device, g, dy, w, "igemm2_bwd<128,64>")
    judge(f"{name} input gradient <128,64>", dx, lambda d, ww: ref_dgrad(g, d, ww), (dy, w), "f32", kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_64x128_weight_gradient_tile(L, big, gpu_device, kind):
    name, g = "G64", Geo("G64")
    x, dy, _, _ = data(name, kind)
    dws, dbs = run_wgrad(L, big, gpu_device, g, dy, x, "igemm2_wgrad<64,128>")
    judge(f"{name} weight gradient <64,128>", dws[0], lambda d, xx: ref_wgrad(g, d, xx)[0], (dy, x), "f32", kind)
    judge_bias_grad(f"{name} <64,128>", dbs[0], dy, kind, "f32")


@gpu
@pytest.mark.parametrize("name", ["B", "T2"])
def test_autograd_round_trip(L, big, gpu_device, dtype, name):
    """Through ops.conv2d / ops.conv_transpose2d and the paired dgrad + wgrad entry point, where a big tile does not pair: the
    input gradient is launched on its own, then the weight gradient."""
    from movae_amd import ops

    g = Geo(name)
    x, dy, w, b = data(name, "int")
    xg = x.to(gpu_device).requires_grad_(True)
    wg = w.to(gpu_device).permute(0, 3, 1, 2).requires_grad_(True)  # the parameter's logical shape over its channels-last memory
    bg = b.to(gpu_device).requires_grad_(True)
    if g.tr:
        y = ops.conv_transpose2d(xg, wg, bg, g.s, g.p, CASES[name][8], None, 0.01)
    else:
        y = ops.conv2d(xg, wg, bg, g.s, g.p, None, 0.01)
    assert last(big) == fwd_kernel(g, dtype)
    y.backward(dy.to(gpu_device))
    assert last(big) == f"{dgrad_kernel(g, dtype)} + {kern('wgrad', dtype)}"
    L.defer_flush()
    torch.cuda.synchronize()
    dw, db = memo((f"{name} wgrad", "int", "both"), lambda: ref_wgrad(g, dy, x))
    assert torch.equal(y.detach().cpu(), memo((f"{name} forward (no act)", "int"), lambda: ref_fwd(g, x, w, b)).float())
    assert torch.equal(xg.grad.cpu(), memo((f"{name} input gradient 1", "int", "exact"), lambda: ref_dgrad(g, dy, w)).float())
    assert torch.equal(wg.grad.permute(0, 2, 3, 1).cpu(), dw.float())
    assert torch.equal(bg.grad.cpu(), db.float())


@gpu
def test_f32_results_unchanged_by_a_visit_to_bf16(L, big, gpu_device):
    g = Geo("B")
    x, dy, w, b = data("B", "normal")

    def run(dt):
        with mode(L, dt):
            y = run_fwd(L, big, gpu_device, g, x, w, b, fwd_kernel(g, dt))
            dx = run_dgrad(L, big, gpu_device, g, dy, w, dgrad_kernel(g, dt))
            dws, dbs = run_wgrad(L, big, gpu_device, g, dy, x, kern("wgrad", dt))
        return y, dx, dws[0], dbs[0]

    before, visit, after = run("f32"), run("bf16"), run("f32")
    for a, v, c, what in zip(before, visit, after, ("y", "dx", "dW", "db")):
        assert torch.equal(a, c), f"{what}: the fp32 result changed after a visit to bf16"
        assert what == "db" or not torch.equal(a, v), f"{what}: the bf16 mode computed the fp32 result"


# ---- CPU checks of this file's own machinery ------------------------------------------------------------------------------------
def _torch_ops(g, x, w, b, nrm=None):
    """The same operation through torch in float64: (y, autograd function of dy -> (dx, dW in memory layout, db))."""
    xt = virt(x, nrm).permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.double().permute(0, 3, 1, 2).requires_grad_(True)  # [co][ci][k][k] / [ci][co][k][k]
    bt = b.double().requires_grad_(True)
    if g.tr:
        y = F.conv_transpose2d(xt, wt, bt, stride=g.s, padding=g.p, output_padding=CASES[g.name][8])
    else:
        y = F.conv2d(xt, wt, bt, stride=g.s, padding=g.p)

    def grads(dy):
        dx, dw, db = torch.autograd.grad(y, (xt, wt, bt), dy.double().permute(0, 3, 1, 2), retain_graph=True)
        return dx.permute(0, 2, 3, 1), dw.permute(0, 2, 3, 1), db

    return y.permute(0, 2, 3, 1), grads


def close(a, b):
    return rel(a, b) < 1e-13


@pytest.mark.parametrize("name", ["B", "T2"])
def test_reference_agrees_with_torch(name):
    g = Geo(name)
    x, dy, w, b = data(name, "normal", groups=2)
    y, grads = _torch_ops(g, x, w, b)
    assert tuple(y.shape) == (g.n, g.ho, g.wo, g.co)
    assert close(ref_fwd(g, x, w, b), y)
    assert close(ref_fwd(g, x, w, b, SLOPE), F.leaky_relu(y, SLOPE))
    dyg = dy.view(2, g.n, g.ho, g.wo, g.co)
    dxs = []
    for i in range(2):  # cotangent groups: the stacked input gradient is the groups' gradients stacked, x is shared
        dx, dw, db = grads(dyg[i])
        dxs.append(dx)
        rw, rbias = ref_wgrad(g, dyg[i], x)
        assert tuple(rw.shape) == g.wshape and close(rw, dw) and close(rbias, db)
        # accumulate: the expression test_accumulate expects, on a gradient of torch's with an initial value of its own
        dw0 = torch.full(g.wshape, 3.0) if i else torch.arange(rw.numel(), dtype=torch.float32).view(g.wshape) % 11 - 5
        wacc = w.double().permute(0, 3, 1, 2).requires_grad_(True)
        wacc.grad = dw0.double().permute(0, 3, 1, 2).clone()
        conv = F.conv_transpose2d if g.tr else F.conv2d
        kw = {"output_padding": CASES[name][8]} if g.tr else {}
        conv(x.double().permute(0, 3, 1, 2), wacc, None, stride=g.s, padding=g.p, **kw).backward(dyg[i].double().permute(0, 3, 1, 2))
        assert close(dw0.double() + rw, wacc.grad.permute(0, 2, 3, 1))
    assert close(ref_dgrad(g, dy, w), torch.cat(dxs))
    # virtual operand: the transform acts on x, not on the padding
    nrm = norm_params(g.ci, "normal", 77)
    yv, gradsv = _torch_ops(g, x, w, b, nrm)
    assert close(ref_fwd(g, virt(x, nrm), w, b), yv) and not close(yv, y)
    assert close(ref_wgrad(g, dyg[0], virt(x, nrm))[0], gradsv(dyg[0])[1])


def test_integer_data_is_exact_in_fp32():
    """The longest reductions of the integer cases: sum |a| |b| bounds every partial sum of every summation order."""
    two24 = 2.0 ** 24
    for name in ("C", "B", "W64"):
        g = Geo(name)
        x, dy, w, b = (t.abs() for t in data(name, "int"))
        assert float(ref_fwd(g, x, w, b).max()) < two24
        assert float(ref_dgrad(g, dy, w).max()) < two24
        dw, db = ref_wgrad(g, dy, x)
        assert float(dw.max()) + 5 < two24 and float(db.max()) + 5 < two24
    # the virtual operand: half-integers of at most 5 significant bits, exact in bf16
    g = Geo("B")
    xv = virt(data("B", "int", grid=True)[0], norm_params(g.ci, "int", 77))
    assert torch.equal(xv * 2, (xv * 2).round()) and float(xv.abs().max()) <= 8 and torch.equal(rb(xv), xv)
    xn = virt(data("B", "normal", grid=True)[0], norm_params(g.ci, "normal", 77))
    assert torch.equal(xn.float().double(), xn)  # the normal-data transform is exact in fp32: the rounding to bf16 is the only one


def test_random_data_criterion_separates():
    """What `< 1e-5 against the rounded reference` accepts and what it rejects, on case B's forward (K = 1188)."""
    g = Geo("B")
    x, _, w, b = data("B", "normal")
    want = ref_fwd(g, rb(x), rb(w), b)

    def conv32(xx, ww):
        return F.conv2d(xx.float().permute(0, 3, 1, 2), ww.float().permute(0, 3, 1, 2), b, stride=g.s, padding=g.p).permute(0, 2, 3, 1)

    def trunc(t):
        return (t.float().view(torch.int32) & -65536).view(torch.float32)

    assert rel(conv32(rb(x), rb(w)), want) < 1e-5     # fp32 accumulation of exact bf16 products
    assert rel(conv32(trunc(x), trunc(w)), want) > 1e-3  # truncation instead of round-to-nearest-even
    assert rel(conv32(x, w), want) > 1e-3             # no rounding at all
    w1 = rb(w).clone()
    w1[:, 1, 1, 7] = 0                                # one reduction index dropped
    assert rel(conv32(rb(x), w1), want) > 1e-3
