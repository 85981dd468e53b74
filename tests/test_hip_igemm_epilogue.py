"""The store epilogues of the tiled conv kernels (csrc/igemm_v2.h: igemm2_fwd / igemm2_bwd) through the C entry points, on the
paths the model never takes: the scalar per-lane epilogue with one partial pair per wave row, which a kernel reaches only when
the bias or bn_y is not 16-byte aligned, next to the through-LDS epilogue with one partial pair per block that aligned operands
get.  Both must store the same bits, and their BatchNorm side products must be the column sums of what was stored.

Bounds: a partial is a float32 sum of at most R = BM terms (BM: rows of the tile), so it is off by at most R * 2^-24 * sum|term|
(the squares and the d * y products enter their sums through fmaf, i.e. unrounded); the partials are folded in float64 here.

The 128x128 tile (and its bf16-operand instantiation) is reached through movae_bench_big_tile_min(1) by the cases with 160
channels; the side products are sums of what was stored, so the same bounds hold in either compute dtype."""
import contextlib
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K, STRIDE, PAD = 3, 2, 1
LRELU = 1  # MOVAE_ACT_LRELU


@pytest.fixture(scope="module")
def L(gpu_device):
    import movae_amd
    import movae_amd._lib as lib

    movae_amd.load_library()
    return lib


@pytest.fixture
def tiled(L):
    """Keeps every shape on the unsplit tiled kernels: no block-internal split-K family, split factor 1."""
    lib = L.load()
    kgemm, split = lib.movae_bench_force_kgemm(-1), lib.movae_bench_force_split(1)
    try:
        yield lib
    finally:
        lib.movae_bench_force_split(split)
        lib.movae_bench_force_kgemm(kgemm)


@contextlib.contextmanager
def compute(L, dtype, channels):
    """The compute dtype; for 128 or more columns also the 128x128 tile from one work item on.  The cases below that keep the
    dispatcher's own threshold."""
    prev = L.set_compute_dtype(dtype)
    big = L.load().movae_bench_big_tile_min(1) if channels >= 128 else None
    try:
        yield
    finally:
        if big is not None:
            L.load().movae_bench_big_tile_min(big)
        L.set_compute_dtype(prev)


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen).cuda()


def off4(t):
    """The same values 4 bytes past a 16-byte boundary: a view one float into a larger buffer."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def tile_of(channels):  # the dispatcher's choice for these small shapes under `tiled` and `compute`: (BM, BN, WM)
    if channels >= 128:
        return (128, 128, 2)
    return (128, 32, 4) if channels <= 32 else (64, 64, 2)


def kernel_of(form, channels, dtype="f32"):
    BM, BN, _ = tile_of(channels)
    return f"igemm2_{form}<{BM},{BN}{',true' if dtype == 'bf16' and BM == BN == 128 else ''}>"


BIG_BOTH = [pytest.param((160, "f32"), id="160"), pytest.param((160, "bf16"), id="160-bf16")]  # the 128x128 tile, both compute dtypes


def channels_dtype(p):  # a channel count alone: fp32 (the small tiles have no bf16 form)
    return p if isinstance(p, tuple) else (p, "f32")


def last_kernel(lib):
    return lib.movae_bench_last_kernel().decode()


def within(got, want, bound, what):
    err = (got - want).abs()
    assert bool((err <= bound).all()), f"{what}: worst error {float(err.max()):.3e}, bound there {float(bound.flatten()[err.argmax()]):.3e}"


STATS_CASES = [  # (transposed, n, hi, wi, ci, ho, wo, co)
    (False, 5, 8, 8, 16, 4, 4, 32),  # FWD form <128,32>: M = 80, a ragged row block
    (False, 5, 8, 8, 16, 4, 4, 64),  # FWD form <64,64>: two row blocks, the second ragged
    (True, 5, 4, 4, 32, 8, 8, 16),   # BWD form <128,32>: four parity classes of 80 rows (output_padding 1)
    (True, 5, 4, 4, 32, 8, 8, 64),   # BWD form <64,64>: two row blocks per class
    (False, 5, 12, 12, 16, 6, 6, 160),  # FWD form <128,128>: M = 180, N = 160, both ragged
    (True, 5, 6, 6, 32, 12, 12, 160),   # BWD form <128,128>: four parity classes of 180 rows
    (False, 5, 12, 12, 16, 6, 6, 160, "bf16"),  # the same two with bf16 operands: <128,128,true>
    (True, 5, 6, 6, 32, 12, 12, 160, "bf16"),
]


@pytest.mark.parametrize("case", STATS_CASES)
def test_statistics_are_the_column_sums_of_what_was_stored(L, tiled, case):
    dtype = case[8] if len(case) > 8 else "f32"
    with compute(L, dtype, case[7]):
        _statistics(L, tiled, case[:8], dtype)


def _statistics(L, tiled, case, dtype):
    tr, n, hi, wi, ci, ho, wo, co = case
    gen = torch.Generator().manual_seed(11)
    x, bias = rnd(gen, n, hi, wi, ci), rnd(gen, co)
    w = (rnd(gen, ci, K, K, co) if tr else rnd(gen, co, K, K, ci)) * 0.1
    ws, st = L.workspace(x.device), torch.cuda.current_stream().cuda_stream
    BM, BN, WM = tile_of(co)
    name = "movae_convT2d_fwd_f" if tr else "movae_conv2d_fwd_f"

    def run(b):
        y = torch.full((n, ho, wo, co), float("nan"), device=x.device)
        stats = torch.full((64 * 2 * co,), float("nan"), device=x.device)
        f = L.MovaeFuse()
        f.stats, f.stats_cap = stats.data_ptr(), stats.numel()
        L.call(name, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), n, hi, wi, ci, ho, wo, co, K, K, STRIDE, PAD, 0, 0.0,
               ws.data_ptr(), ws.numel(), st, C.byref(f))
        torch.cuda.synchronize()
        assert last_kernel(tiled) == kernel_of("bwd" if tr else "fwd", co, dtype)
        assert f.stats_parts > 0
        return y, stats[:f.stats_parts * 2 * co].view(f.stats_parts, 2, co).double().sum(0).cpu(), f.stats_parts

    y1, s_lds, parts_lds = run(bias)
    y2, s_wave, parts_wave = run(off4(bias))
    assert torch.isfinite(y1).all() and torch.equal(y1, y2)  # both compute acc + bias
    assert parts_wave == WM * parts_lds  # one partial pair per wave row against one per block
    yd = y1.double().view(-1, co).cpu()
    for got, what in ((s_lds, "one pair per block"), (s_wave, "one pair per wave row")):
        within(got[0], yd.sum(0), BM * U * yd.abs().sum(0), f"sum y ({what})")
        within(got[1], (yd * yd).sum(0), BM * U * (yd * yd).sum(0), f"sum y^2 ({what})")


def dgrad_operands(tr, groups, ci, seed):
    """An input-gradient problem whose dx is [groups * n][8][8][ci]: whole row blocks per group and parity class (n = 8; 16 for
    the 128-row tile: two row blocks per group and class)."""
    n, hi, wi, co = (16 if ci >= 128 else 8), 8, 8, 16
    ho, wo = (16, 16) if tr else (4, 4)
    gen = torch.Generator().manual_seed(seed)
    dy = rnd(gen, groups * n, ho, wo, co)
    w = (rnd(gen, ci, K, K, co) if tr else rnd(gen, co, K, K, ci)) * 0.1
    return dy, w, (groups * n, hi, wi, ci, ho, wo, co, K, K, STRIDE, PAD), gen


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("ci", [32, 64] + BIG_BOTH)
@pytest.mark.parametrize("tr", [True, False], ids=["fwd_form", "bwd_form"])
def test_batchnorm_backward_sums_match_the_stored_gradient(L, tiled, tr, ci, groups):
    ci, dtype = channels_dtype(ci)
    with compute(L, dtype, ci):
        _batchnorm_backward_sums(L, tiled, tr, ci, dtype, groups)


def _batchnorm_backward_sums(L, tiled, tr, ci, dtype, groups):
    dy, w, geom, gen = dgrad_operands(tr, groups, ci, 23)
    n, hi, wi = geom[0] // groups, geom[1], geom[2]
    slope = 0.01
    bn_y = torch.randn(n, hi, wi, ci, generator=gen)
    scale, shift = torch.rand(ci, generator=gen) + 0.5, torch.randn(ci, generator=gen) * 0.2
    # LeakyReLU' jumps at zero: no pre-activation may sit where float32 and float64 could disagree about its sign
    z = scale.double() * bn_y.double() + shift.double()
    assert float(z.abs().min()) > 1e-6
    ws, st = L.workspace(dy.device), torch.cuda.current_stream().cuda_stream
    BM, BN, WM = tile_of(ci)
    sc_d, sh_d = scale.cuda(), shift.cuda()

    def run(y_dev):
        dx = torch.full((groups * n, hi, wi, ci), float("nan"), device=dy.device)
        part = torch.full((groups * 64 * 2 * ci,), float("nan"), device=dy.device)
        f = L.MovaeFuse()
        f.bn_y, f.bn_scale, f.bn_shift, f.bn_slope = y_dev.data_ptr(), sc_d.data_ptr(), sh_d.data_ptr(), slope
        f.bn_part, f.bn_cap = part.data_ptr(), part.numel()
        L.call("movae_convT2d_dgrad_f" if tr else "movae_conv2d_dgrad_f", dy.data_ptr(), w.data_ptr(), dx.data_ptr(), *geom,
               ws.data_ptr(), ws.numel(), st, C.byref(f), groups)
        torch.cuda.synchronize()
        assert last_kernel(tiled) == kernel_of("fwd" if tr else "bwd", ci, dtype)
        assert f.bn_ppg > 0
        return dx, part[:groups * f.bn_ppg * 2 * ci].view(groups, f.bn_ppg, 2, ci).double().sum(1).cpu(), f.bn_ppg

    dx1, s_lds, ppg_lds = run(bn_y.cuda())
    dx2, s_wave, ppg_wave = run(off4(bn_y.cuda()))
    assert torch.isfinite(dx1).all() and torch.equal(dx1, dx2)
    assert ppg_wave == WM * ppg_lds
    # d as the kernel forms it (one float32 product), summed in float64
    d = (dx1.cpu().view(groups, -1, ci) * torch.where(z > 0, 1.0, slope).float().view(1, -1, ci)).double()
    dyy = d * bn_y.double().view(1, -1, ci)
    for got, what in ((s_lds, "one pair per block"), (s_wave, "one pair per wave row")):
        within(got[:, 0], d.sum(1), BM * U * d.abs().sum(1), f"sum d ({what})")
        within(got[:, 1], dyy.sum(1), BM * U * dyy.abs().sum(1), f"sum d * y ({what})")


@pytest.mark.parametrize("tr", [True, False], ids=["fwd_form", "bwd_form"])
def test_activation_derivative_and_residual_in_the_epilogue(L, tiled, tr):
    _activation_derivative_and_residual(L, tiled, tr, 32, "f32")


@pytest.mark.parametrize("ci", BIG_BOTH)
@pytest.mark.parametrize("tr", [True, False], ids=["fwd_form", "bwd_form"])
def test_activation_derivative_and_residual_in_the_big_tile_epilogue(L, tiled, tr, ci):
    ci, dtype = ci
    with compute(L, dtype, ci):
        _activation_derivative_and_residual(L, tiled, tr, ci, dtype)


def _activation_derivative_and_residual(L, tiled, tr, ci, dtype):
    groups, slope = 2, 0.2
    dy, w, geom, gen = dgrad_operands(tr, groups, ci, 37)
    n, hi, wi = geom[0] // groups, geom[1], geom[2]
    act_y, res = rnd(gen, n, hi, wi, ci), rnd(gen, groups * n, hi, wi, ci)
    ws, st = L.workspace(dy.device), torch.cuda.current_stream().cuda_stream
    pre = "movae_convT2d_dgrad" if tr else "movae_conv2d_dgrad"
    kernel = kernel_of("fwd" if tr else "bwd", ci, dtype)
    plain = torch.full((groups * n, hi, wi, ci), float("nan"), device=dy.device)
    L.call(pre, dy.data_ptr(), w.data_ptr(), plain.data_ptr(), *geom, ws.data_ptr(), ws.numel(), st)
    assert last_kernel(tiled) == kernel
    fused = torch.full_like(plain, float("nan"))
    f = L.MovaeFuse()
    f.ep_act_y, f.ep_act, f.ep_slope, f.ep_res = act_y.data_ptr(), LRELU, slope, res.data_ptr()
    L.call(pre + "_f", dy.data_ptr(), w.data_ptr(), fused.data_ptr(), *geom, ws.data_ptr(), ws.numel(), st, C.byref(f), groups)
    torch.cuda.synchronize()
    assert last_kernel(tiled) == kernel and f.ep_act_done == 1
    # the product and the add are single roundings on both sides
    factor = torch.where(act_y > 0, 1.0, slope).to(plain.dtype)
    want = (plain.view(groups, n, hi, wi, ci) * factor).view_as(res) + res
    assert torch.isfinite(fused).all() and torch.equal(fused, want)
