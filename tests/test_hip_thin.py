"""The thin-channel conv kernels (csrc/conv_thin.h: the 3-channel image ends of every network) through the C entry points, with
the machinery of test_hip_big_tile.py: a float64 tap-loop reference, outputs between guard zones that start as NaN, and the
asserted name of the kernel that ran (movae_bench_last_kernel names the launched instantiation as rocprofv3 prints it).  The
dispatcher is pinned as by that file's `tiled`: no block-internal split-K family, split factor 1, its own tile threshold.

Two data sets per case:
  * integers (x, dy in -3..3, w in -2..2, bias in -8..8, LeakyReLU slope 0.5, the fused input transform of norm_params "int"):
    every partial sum is an integer or half-integer below 2^24 (checked on the CPU below for the longest reductions), so
    v_mfma_f32_32x32x2f32 and the VALU FMAs are exact in any order and the result must EQUAL the float64 reference;
  * seeded normal data: rel-L2 < 1e-5 against float64 for reductions of up to 2^15 terms; the longer weight gradients (R5, R6, R12)
    stay below max(1e-5, 4 * e_cpu), e_cpu being the rel-L2 of the same gradient formed on the CPU in float32 by torch (another
    legitimate summation order; the factor 4 because the orders differ).  Both figures are printed.

ALL_THIN_KERNELS lists every instantiation the launchers of conv_thin.h can launch (read off their hipLaunchKernelGGL sites); a
CPU test checks that each is the expected kernel of a case here.  The shapes are the smallest at which each kernel still has a
ragged edge, two tiles or two channel blocks."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_hip_big_tile as bt

gpu = pytest.mark.gpu
L = bt.L  # (the module-scoped library fixture)
SLOPE, LRELU, U = bt.SLOPE, bt.LRELU, 2.0 ** -24

# conv: (n, hi, wi, ci, co, k, s, p); transposed conv: (..., output_padding)
CASES = {
    # thin_in: at most 4 reduction channels, at least 8 outputs
    "I1": (2, 32, 32, 3, 32, 3, 2, 1),       # a block is one whole 16 x 16 output image
    "I2": (1, 64, 64, 3, 64, 4, 2, 1),       # two column tiles, 8 rows of 32 per block
    "I3": (1, 4, 512, 3, 32, 3, 1, 1),       # row-segment blocks (Wo = 512)
    "I4": (1, 64, 16, 3, 32, 3, 2, 1),       # narrow and tall: Wo = 8, 32 rows per block
    "I5": (3, 13, 11, 3, 32, 3, 2, 1),       # M = 126: one ragged block, LDS-tile output path
    "I6": (2, 9, 7, 1, 16, 5, 1, 2),         # 1 input channel, 16 outputs (the non-tile store path), 5 x 5 taps
    "I7": (2, 9, 7, 4, 72, 3, 2, 1),         # 4 channels; the second column tile has 8 of 64
    "I8": (2, 9, 7, 2, 10, 3, 1, 1),         # N % 4 != 0: scalar stores
    "I9": (2, 16, 16, 32, 3, 3, 1, 1),       # (dgrad) the last conv's input gradient
    "I10": (1, 8, 32, 64, 3, 4, 1, 1),       # (dgrad) two column tiles; dx is 8 x 32 = one 256-pixel block of 8 rows
    "I11": (3, 9, 7, 32, 3, 3, 1, 1),        # (dgrad) ragged
    "I12": (2, 5, 6, 3, 40, 4, 2, 1, 0),     # stride-2 parity tests of the VALU BWD form, 40 of 64
    "I13": (2, 16, 16, 128, 3, 4, 2, 1, 0),  # (dgrad) 128 outputs = four column tiles (VQ last layer)
    # thin_out: at most 4 outputs
    "O1": (2, 9, 35, 32, 3, 3, 1, 1),        # 2 x 2 tiles of 8 x 32, both ragged
    "O2": (1, 9, 35, 64, 3, 3, 1, 1),        # two reduction chunks
    "O3": (2, 9, 35, 24, 2, 3, 1, 1),        # 2 outputs; 24 channels is not a multiple of the chunk
    "O4": (2, 10, 36, 16, 4, 4, 1, 1),       # the 16-channel chunk (4 x 4 taps do not fit with 32)
    "O5": (1, 448, 448, 4, 3, 3, 1, 1),      # two pixels per thread (from 200 000 pixels)
    "O6": (2, 10, 10, 16, 3, 3, 2, 1),       # stride 2: no tile plan fits
    "O7": (2, 7, 5, 16, 1, 5, 1, 2),         # 25 taps, 1 output
    "O8": (2, 9, 35, 32, 3, 4, 2, 1, 0),     # 2 x 2 input tiles, ragged, four parity classes
    "O9": (2, 9, 5, 96, 3, 4, 2, 1, 0),      # three channel chunks, width below a tile
    "O10": (3, 8, 8, 32, 3, 3, 2, 1, 1),     # 3 x 3 taps with output padding
    "O11": (2, 9, 7, 24, 2, 4, 2, 1, 1),     # odd output width 15: a tile width rounded up to 16 (see SHAPES_CHANGED)
    "O12": (8, 32, 32, 3, 32, 3, 2, 1),      # (dgrad, 2 groups) the first conv's (unused but offered) input gradient
    "O13": (1, 224, 224, 32, 3, 3, 2, 1, 1),  # the transposed form with two pixels per thread (448 x 448 outputs)
    "O14": (1, 50000, 1, 4, 3, 4, 2, 1, 0),  # 2 outputs wide, 256 rows per tile: only there the 16-channel chunk meets two pixels
    # weight gradients
    "R1": (2, 16, 16, 32, 3, 3, 1, 1),       # thin = dy; one 16 x 16 tile per image
    "R2": (2, 32, 32, 3, 64, 4, 2, 1),       # thin = x, stride 2, two wide slices
    "R3": (2, 9, 35, 64, 3, 4, 2, 1, 0),     # the convT operand mapping, ragged tiles
    "R4": (2, 9, 24, 32, 3, 3, 1, 1),        # width 24: tile width not a power of two, VALU sweep
    "R5": (4, 80, 80, 128, 3, 3, 1, 1),      # 120 tiles on 96 persistent blocks: blocks loop over tiles
    "R6": (1, 512, 512, 32, 3, 3, 1, 1),     # 2^18 pixels: the bias gradient comes from the kernel's own column sums (cs_on)
    "R7": (2, 9, 7, 20, 2, 3, 1, 1),         # wide side not a multiple of 32
    "R8": (2, 9, 7, 1, 16, 5, 1, 2),         # 1 thin channel, 25 taps
    "R9": (2, 9, 7, 4, 72, 3, 2, 1),         # 4 thin channels, stride 2
    "R10": (2, 13, 11, 32, 3, 3, 2, 1),      # thin = dy at stride 2 (the sweep kernels need stride 1 there)
    "R12": (2, 20, 20, 128, 3, 4, 2, 1, 0),  # four wide slices, several tiles, long reduction
    # the instantiations the rows above leave out
    "R13": (2, 9, 7, 20, 1, 3, 1, 1),        # thin = dy, 1 channel
    "R14": (2, 9, 7, 20, 4, 3, 1, 1),        # thin = dy, 4 channels
    "R15": (2, 9, 7, 2, 10, 3, 1, 1),        # thin = x, 2 channels
    "R16": (2, 9, 7, 3, 40, 3, 2, 1),        # thin = x, 3 channels, wide side not a multiple of 32
    "R17": (2, 9, 24, 3, 32, 3, 1, 1),       # the VALU sweep with thin = x
    "R18": (2, 9, 25, 32, 3, 4, 1, 1),       # the VALU sweep with 4 x 4 taps, thin = dy (x is 25 wide)
    "R19": (1, 8, 32, 64, 3, 4, 1, 1),       # the MFMA sweep with 4 x 4 taps, thin = dy
}

# (case, what the issue asked for, why it changed)
SHAPES_CHANGED = [
    ("O11", "convT 2,9,5, 24->2, k4 s2 p1 op0",
     "a 10-wide output gives a tile width of 10, and thin_out_tile_plan<true> needs 256 % (2 * TW) == 0: no plan, the generic kernel "
     "runs.  Only an odd output width is rounded up at all, and k4 s2 p1 gives one with output padding 1: 7 -> 15 wide, TW = 16."),
    ("R5", "400 tiles", "80 x 80 images in 8 x 32 tiles are 10 x 3 = 30 tiles each, 120 in all; the 96 persistent blocks still loop"),
]

FWD = {
    "I1": "thin_in_mfma_k<3,3,false>", "I2": "thin_in_mfma_k<4,4,false>", "I3": "thin_in_mfma_k<3,3,false>",
    "I4": "thin_in_mfma_k<3,3,false>", "I5": "thin_in_k<32,false>", "I6": "thin_in_k<32,false>", "I7": "thin_in_k<64,false>",
    "I8": "thin_in_k<32,false>", "I12": "thin_in_k<64,true>",
    "O1": "thin_out_mfma_k<3,3,true>", "O2": "thin_out_mfma_k<3,3,false>", "O3": "thin_out_tile_k<false,32,1>",
    "O4": "thin_out_tile_k<false,16,1>", "O5": "thin_out_tile_k<false,16,2>", "O6": "thin_out_fwd_k<4>", "O7": "thin_out_fwd_k<4>",
    "O8": "thin_outT_mfma_k", "O9": "thin_outT_mfma_k", "O10": "thin_out_tile_k<true,32,1>", "O11": "thin_out_tile_k<true,32,1>",
    "O13": "thin_out_tile_k<true,32,2>", "O14": "thin_out_tile_k<true,16,2>",
}
PLAIN = ["I1", "I2", "I5", "I7", "I12", "O1", "O2", "O3", "O4", "O5", "O6", "O8", "O10", "O13", "O14"]  # once without bias and activation
VIRTUAL_FWD = ["O1", "O2", "O3", "O4", "O8", "O10"]
DGRAD = {  # case: (kernel, group counts)
    "I9": ("thin_in_mfma_k<3,3,true>", (1, 2)), "I10": ("thin_in_mfma_k<4,4,true>", (1,)), "I11": ("thin_in_k<32,true>", (1,)),
    "I13": ("thin_in_mfma_k<4,4,false>", (1,)), "O12": ("thin_out_tile_k<true,32,1>", (2,)),
}
WGRAD = {  # case: (kernel, group counts)
    "R1": ("thin_wgrad_mfma_k<3,3,3,true>", (1, 2)), "R2": ("thin_wgrad_mfma_k<3,4,4,false>", (1, 2)),
    "R3": ("thin_wgrad_mfma_k<3,4,4,false>", (1, 2)), "R4": ("thin_wgrad_sweep_k<3,3,3,true>", (1, 2)),
    "R5": ("thin_wgrad_mfma_k<3,3,3,true>", (2,)), "R6": ("thin_wgrad_mfma_k<3,3,3,true>", (1,)),
    "R7": ("thin_wgrad_tiled_k<true,2>", (1, 2)), "R8": ("thin_wgrad_tiled_k<false,1>", (1, 2)),
    "R9": ("thin_wgrad_tiled_k<false,4>", (1, 2)), "R10": ("thin_wgrad_tiled_k<true,3>", (1, 2)),
    "R12": ("thin_wgrad_sweep_k<3,4,4,false>", (1, 2)),
    "R13": ("thin_wgrad_tiled_k<true,1>", (1,)), "R14": ("thin_wgrad_tiled_k<true,4>", (1,)), "R15": ("thin_wgrad_tiled_k<false,2>", (1,)),
    "R16": ("thin_wgrad_tiled_k<false,3>", (1,)), "R17": ("thin_wgrad_sweep_k<3,3,3,false>", (1,)),
    "R18": ("thin_wgrad_sweep_k<3,4,4,true>", (1,)), "R19": ("thin_wgrad_mfma_k<3,4,4,true>", (1,)),
    "I1": ("thin_wgrad_mfma_k<3,3,3,false>", (2,)),  # (the first conv of the networks: the shape of the recorded conv pair)
}
LAST_FALLBACK = {"R7": "thin_wgrad_k<true>", "R9": "thin_wgrad_k<false>"}  # R11: with a workspace of fewer slabs than tiles
VIRTUAL_WGRAD = ["R1", "R3", "R4"]  # the transform is x's: R2's wide operand is dy, and x has 3 channels there (see the refusals)
LONG = ("R5", "R6", "R12")

ALL_THIN_KERNELS = [
    "thin_in_k<32,false>", "thin_in_k<32,true>", "thin_in_k<64,false>", "thin_in_k<64,true>",
    "thin_in_mfma_k<3,3,false>", "thin_in_mfma_k<3,3,true>", "thin_in_mfma_k<4,4,false>", "thin_in_mfma_k<4,4,true>",
    "thin_out_fwd_k<4>",
    "thin_out_mfma_k<3,3,true>", "thin_out_mfma_k<3,3,false>",
    "thin_outT_mfma_k",
    "thin_out_tile_k<false,32,1>", "thin_out_tile_k<false,16,1>", "thin_out_tile_k<false,16,2>",
    "thin_out_tile_k<true,32,1>", "thin_out_tile_k<true,32,2>", "thin_out_tile_k<true,16,2>",
    "thin_wgrad_sweep_k<3,3,3,true>", "thin_wgrad_sweep_k<3,3,3,false>", "thin_wgrad_sweep_k<3,4,4,true>", "thin_wgrad_sweep_k<3,4,4,false>",
    "thin_wgrad_mfma_k<3,3,3,true>", "thin_wgrad_mfma_k<3,3,3,false>", "thin_wgrad_mfma_k<3,4,4,true>", "thin_wgrad_mfma_k<3,4,4,false>",
    "thin_wgrad_tiled_k<true,1>", "thin_wgrad_tiled_k<true,2>", "thin_wgrad_tiled_k<true,3>", "thin_wgrad_tiled_k<true,4>",
    "thin_wgrad_tiled_k<false,1>", "thin_wgrad_tiled_k<false,2>", "thin_wgrad_tiled_k<false,3>", "thin_wgrad_tiled_k<false,4>",
    "thin_wgrad_k<true>", "thin_wgrad_k<false>",
]
# instantiated by launch_thin_out_tile's macro, but chosen by thin_out_tile_plan for no shape
UNREACHABLE = {
    "thin_out_tile_k<false,32,2>": "two pixels per thread are TH * TW = 512 pixels; the staged region has at least as many, and 512 * "
                                   "(32 + 4) floats are 72 KiB, above the plan's 62 KiB: the plan always falls to the 16-channel chunk",
    "thin_out_tile_k<true,16,1>": "at one pixel per thread the region of the largest plan (TW = 2, TH = 128, 4 x 4 taps: 67 x 4 inputs) "
                                  "takes 46 KiB with the 32-channel chunk, which the plan tries first: it always fits",
}


def geo(name):
    return bt.Geo(name, CASES[name])


_DATA = {}


def data(name, kind, groups=1):
    """(x, dy, w, bias) float32 on the CPU, as test_hip_big_tile.data draws them."""
    key = (name, kind, groups)
    if key not in _DATA:
        g = geo(name)
        gen = torch.Generator().manual_seed(2000 + sum(map(ord, name)) + groups)
        xs, dys = (g.n, g.hi, g.wi, g.ci), (groups * g.n, g.ho, g.wo, g.co)
        if kind == "int":
            x, dy = torch.randint(-3, 4, xs, generator=gen).float(), torch.randint(-3, 4, dys, generator=gen).float()
            w, b = torch.randint(-2, 3, g.wshape, generator=gen).float(), torch.randint(-8, 9, (g.co,), generator=gen).float()
        else:
            x, dy = torch.randn(xs, generator=gen), torch.randn(dys, generator=gen)
            x = ((x * 1024).round() / 1024).clamp(-3.75, 3.75)  # (on a grid: the fused input transform is then exact in fp32)
            w, b = torch.randn(g.wshape, generator=gen) * float(g.ci * g.k * g.k) ** -0.5, torch.randn(g.co, generator=gen) * 0.1
        _DATA[key] = (x, dy, w, b)
    return _DATA[key]


@pytest.fixture
def tiled(L):
    with bt.pinned(L, 0, 1) as lib:
        yield lib


KINDS = bt.KINDS


def judge(what, got, ref, ops, kind):
    bt.judge(f"thin {what}", got, ref, ops, "f32", kind)


# ---- forward form and input gradient ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(FWD))
def test_forward(L, tiled, gpu_device, name, kind):
    g = geo(name)
    x, _, w, b = data(name, kind)
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, FWD[name])
    judge(f"{name} forward", y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b, SLOPE), (x, w), kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", PLAIN)
def test_forward_without_bias_and_activation(L, tiled, gpu_device, name, kind):
    g = geo(name)
    x, _, w, _ = data(name, kind)
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, None, FWD[name], act=False)
    judge(f"{name} forward (plain)", y, lambda xx, ww: bt.ref_fwd(g, xx, ww), (x, w), kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", VIRTUAL_FWD)
def test_forward_virtual_operand(L, tiled, gpu_device, name, kind):
    """BatchNorm + LeakyReLU applied to x while it is staged; padding stays zero after the transform (the shift is not)."""
    g = geo(name)
    x, _, w, b = data(name, kind)
    nrm = bt.norm_params(g.ci, kind, 77)
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, FWD[name], nrm=nrm)
    judge(f"{name} forward (virtual x)", y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b, SLOPE), (bt.virt(x, nrm), w), kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,groups", [(n, gr) for n, (_, grs) in DGRAD.items() for gr in grs])
def test_input_gradient(L, tiled, gpu_device, name, groups, kind):
    g = geo(name)
    _, dy, w, _ = data(name, kind, groups)
    dx = bt.run_dgrad(L, tiled, gpu_device, g, dy, w, DGRAD[name][0], groups)
    judge(f"{name} input gradient ({groups} groups)", dx, lambda d, ww: bt.ref_dgrad(g, d, ww), (dy, w), kind)


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------
def wgrad_cpu_f32(g, dy, x):
    """The same weight gradient (memory layout) by torch on the CPU in float32: another summation order."""
    xt, dyt = x.float().permute(0, 3, 1, 2), dy.float().permute(0, 3, 1, 2)
    if g.tr:
        wt = torch.zeros(g.ci, g.co, g.k, g.k, requires_grad=True)
        y = F.conv_transpose2d(xt, wt, None, stride=g.s, padding=g.p, output_padding=CASES[g.name][8])
    else:
        wt = torch.zeros(g.co, g.ci, g.k, g.k, requires_grad=True)
        y = F.conv2d(xt, wt, None, stride=g.s, padding=g.p)
    return torch.autograd.grad(y, wt, dyt)[0].permute(0, 2, 3, 1)


def judge_long(what, got, want, cpu32):
    """want float64; the bound comes from the float32 result of another summation order."""
    e, e_cpu = bt.rel(got, want), bt.rel(cpu32, want)
    print(f"[thin] {what}: rel-L2 {e:.2e}, e_cpu {e_cpu:.2e}")
    assert e < max(1e-5, 4 * e_cpu), (what, e, e_cpu)


def check_wgrad(L, lib, dev, name, kind, groups, acc, expect, nrm=None, ws=None):
    g = geo(name)
    x, dy, _, _ = data(name, kind, groups)
    init = None
    if acc:
        gen = torch.Generator().manual_seed(5)
        init = ([torch.randint(-5, 6, g.wshape, generator=gen).float() for _ in range(groups)],
                [torch.randint(-5, 6, (g.co,), generator=gen).float() for _ in range(groups)])
    dws, dbs = bt.run_wgrad(L, lib, dev, g, dy, x, expect, groups, nrm=nrm, init=init, ws=ws)
    xv = bt.virt(x, nrm)
    dyg = dy.view(groups, g.n, g.ho, g.wo, g.co)
    for i in range(groups):
        what = f"{name} weight gradient ({groups} groups, accumulate {acc}{', virtual x' if nrm else ''}) group {i}"
        w0 = init[0][i].double() if acc else 0.0
        b0 = init[1][i].double() if acc else 0.0
        key = (name, kind, groups, i, nrm is not None)
        dw = bt.memo(key + ("dw",), lambda: bt.ref_wgrad(g, dyg[i], xv)[0])
        db = dyg[i].double().reshape(-1, g.co).sum(0)
        if kind == "int":
            assert torch.equal(dws[i], (dw + w0).float()), f"{what}: differs from the exact result"
            assert torch.equal(dbs[i], (db + b0).float()), f"{what}: bias gradient differs from the exact column sums"
        elif name in LONG:
            cpu = bt.memo(key + ("cpu32",), lambda: wgrad_cpu_f32(g, dyg[i], xv))
            judge_long(what, dws[i], dw + w0, cpu + w0)
            judge_long(what + " bias", dbs[i], db + b0, dyg[i].reshape(-1, g.co).sum(0) + b0)
        else:
            e, eb = bt.rel(dws[i], dw + w0), bt.rel(dbs[i], db + b0)
            print(f"[thin] {what}: rel-L2 {e:.2e}, bias gradient {eb:.2e}")
            assert e < 1e-5 and eb < 1e-5, (what, e, eb)
    return dws


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("name,groups", [(n, gr) for n, (_, grs) in WGRAD.items() for gr in grs])
def test_weight_gradient(L, tiled, gpu_device, name, groups, acc, kind):
    check_wgrad(L, tiled, gpu_device, name, kind, groups, acc, WGRAD[name][0])


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", VIRTUAL_WGRAD)
def test_weight_gradient_virtual_operand(L, tiled, gpu_device, name, kind):
    """The transform on the wide operand x: gathered side of the conv (R1, R4), small side of the transposed conv (R3)."""
    check_wgrad(L, tiled, gpu_device, name, kind, 2, 0, WGRAD[name][0], nrm=bt.norm_params(geo(name).ci, kind, 77))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", list(LAST_FALLBACK))
def test_weight_gradient_last_fallback(L, tiled, gpu_device, name, groups, kind):
    """R11: one tile per image, so the tiled kernel wants two slabs; a scratch of one and a half sends the call to thin_wgrad_k,
    which splits the pixels into as many chunks as slabs fit: one."""
    g = geo(name)
    slab = g.co * g.k * g.k * g.ci
    ws = bt.Scratch(gpu_device, floats=slab + slab // 2)
    check_wgrad(L, tiled, gpu_device, name, kind, groups, 0, LAST_FALLBACK[name], ws=ws)
    assert 1 <= ws.slabs(slab) < g.n  # (g.n tiles)


# ---- side products of the 32-output thin_in kernels (thin_in_tile_out) ---------------------------------------------------------------
def fold_stats(raw, parts, c=32):
    """[parts][2][c] float32 partial pairs -> (sum, sum of squares) per column in float64."""
    s = raw[:parts * 2 * c].view(parts, 2, c).double().sum(0)
    return s[0], s[1]


def judge_stats(what, s, sq, y, kind, R=64):
    """s, sq: folded partials; y: what was stored, [rows][c].  Exact with integer data; with normal data each partial is a float32
    sum of at most R terms (the squares enter through fmaf), off by at most R * 2^-24 * sum |term| (test_hip_igemm_epilogue.py)."""
    yd = y.double()
    for got, want, mag, nm in ((s, yd.sum(0), yd.abs().sum(0), "sum y"), (sq, (yd * yd).sum(0), (yd * yd).sum(0), "sum y^2")):
        if kind == "int":
            assert torch.equal(got, want), f"{what}: {nm} differs from the exact column sums at columns {(got != want).nonzero().flatten().tolist()}"
        else:
            err = (got - want).abs()
            assert bool((err <= R * U * mag).all()), f"{what}: {nm} worst error {float(err.max()):.3e}"


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["I1", "I5"])
def test_statistics(L, tiled, gpu_device, name, kind):
    """One partial pair per wave (64 rows); I5's single block is ragged (126 of 256 rows: the rows_left mask)."""
    g = geo(name)
    x, _, w, b = data(name, kind)
    blocks = -(-(g.n * g.ho * g.wo) // 256)
    st = bt.Out((4 * blocks * 2 * 32,), gpu_device)
    f = L.MovaeFuse()
    f.stats, f.stats_cap = st.ptr(), st.t.numel()
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, FWD[name], act=False, fuse=f)
    assert f.stats_parts == 4 * blocks
    judge(f"{name} forward (statistics)", y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b), (x, w), kind)
    s, sq = fold_stats(st.get(f"{name} statistics"), f.stats_parts)
    judge_stats(f"{name} statistics", s, sq, y.view(-1, 32), kind)


def bn_operands(g, kind, seed):
    """(bn_y [n][hi][wi][ci], (scale, shift, slope)) with no pre-activation where float32 and float64 could disagree about its sign."""
    gen = torch.Generator().manual_seed(seed)
    shape = (g.n, g.hi, g.wi, g.ci)
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=gen).float(), bt.norm_params(g.ci, "int", seed)
    y = torch.randn(shape, generator=gen)
    scale, shift = torch.rand(g.ci, generator=gen) + 0.5, torch.randn(g.ci, generator=gen) * 0.2
    assert float((scale.double() * y.double() + shift.double()).abs().min()) > 1e-6
    return y, (scale, shift, 0.01)


def fold_bn(raw, groups, ppg, c=32):
    """[groups * ppg][2][c] -> ([groups][c] sums of d, [groups][c] sums of d * y) in float64."""
    s = raw[:groups * ppg * 2 * c].view(groups, ppg, 2, c).double().sum(1)
    return s[:, 0], s[:, 1]


def judge_bn(what, s1, s2, dx, bn_y, nrm, kind, R=64):
    """dx: what was stored, [groups][rows][c]; d = dx * act'(scale * y + shift) as the kernel forms it (one float32 product)."""
    scale, shift, slope = nrm
    z = scale.double() * bn_y.double().view(-1, bn_y.shape[-1]) + shift.double()
    d = (dx * torch.where(z > 0, 1.0, slope).float()).double()
    dyy = d * bn_y.double().view(1, -1, bn_y.shape[-1])
    for got, want, mag, nm in ((s1, d.sum(1), d.abs().sum(1), "sum d"), (s2, dyy.sum(1), dyy.abs().sum(1), "sum d * y")):
        if kind == "int":
            assert torch.equal(got, want), f"{what}: {nm} differs from the exact sums at {(got != want).nonzero().tolist()}"
        else:
            err = (got - want).abs()
            assert bool((err <= R * U * mag).all()), f"{what}: {nm} worst error {float(err.max()):.3e}"


def bn_fuse(L, dev, g, kind, groups, parts):
    bn_y, nrm = bn_operands(g, kind, 23)
    part = bt.Out((max(1, groups * parts) * 2 * 32,), dev)
    keep = (bn_y.to(dev), nrm[0].to(dev), nrm[1].to(dev), part)
    f = L.MovaeFuse()
    f.bn_y, f.bn_scale, f.bn_shift, f.bn_slope = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), nrm[2]
    f.bn_part, f.bn_cap = part.ptr(), part.t.numel()
    return f, keep, bn_y, nrm


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups", [1, 2])
def test_batchnorm_backward_sums(L, tiled, gpu_device, groups, kind):
    """I9's input gradient is the output gradient of a fused BatchNorm over bn_y: four partial pairs per 256-row block."""
    g = geo("I9")
    _, dy, w, _ = data("I9", kind, groups)
    ppg = g.n * g.hi * g.wi // 256 * 4
    f, keep, bn_y, nrm = bn_fuse(L, gpu_device, g, kind, groups, ppg)
    dx = bt.run_dgrad(L, tiled, gpu_device, g, dy, w, DGRAD["I9"][0], groups, fuse=f)
    assert f.bn_ppg == ppg
    judge(f"I9 input gradient ({groups} groups, BatchNorm sums)", dx, lambda d, ww: bt.ref_dgrad(g, d, ww), (dy, w), kind)
    s1, s2 = fold_bn(keep[3].get("I9 bn_part"), groups, f.bn_ppg)
    judge_bn(f"I9 bn_part ({groups} groups)", s1, s2, dx.view(groups, -1, 32), bn_y, nrm, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batchnorm_backward_sums_declined_on_ragged_rows(L, tiled, gpu_device, kind):
    """I11: 189 rows, no multiple of 256 -- bn_ppg comes back 0, nothing is written to bn_part, dx is the plain input gradient."""
    g = geo("I11")
    _, dy, w, _ = data("I11", kind)
    f, keep, _, _ = bn_fuse(L, gpu_device, g, kind, 1, 4)
    dx = bt.run_dgrad(L, tiled, gpu_device, g, dy, w, DGRAD["I11"][0], 1, fuse=f)
    assert f.bn_ppg == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(keep[3].t).all()) and bool((keep[3].buf[:bt.GUARD] == bt.SENTINEL).all())
    judge("I11 input gradient (BatchNorm sums declined)", dx, lambda d, ww: bt.ref_dgrad(g, d, ww), (dy, w), kind)


def ref_actmul(plain, act_y, res, groups, slope):
    """plain [groups * n][h][w][c] float64; act_y [n][h][w][c] (shared by the groups) or None; res like plain or None."""
    out = plain.double()
    if act_y is not None:
        out = (out.view(groups, *act_y.shape) * torch.where(act_y.double() > 0, 1.0, slope)).view_as(plain)
    return out if res is None else out + res.double()


def judge_actmul(what, got, plain, act_y, res, groups, slope, kind):
    want = ref_actmul(plain, act_y, res, groups, slope)
    if kind == "int":
        assert torch.equal(got, want.float()), f"{what}: differs from dgrad * act'(y) + res at {(got != want.float()).nonzero()[0].tolist()}"
    else:
        e = bt.rel(got, want)
        print(f"[thin] {what}: rel-L2 {e:.2e}")
        assert e < 1e-5, (what, e)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["act", "res", "both"])
@pytest.mark.parametrize("name,groups", [("I9", 1), ("I9", 2), ("I11", 1), ("I11", 2)])
def test_activation_derivative_and_residual(L, tiled, gpu_device, name, groups, which, kind):
    """ep_act_y is shared by the groups, ep_res is per group; I11's ragged block masks both loads."""
    g = geo(name)
    _, dy, w, _ = data(name, kind, groups)
    gen = torch.Generator().manual_seed(37)
    draw = (lambda *s: torch.randint(-3, 4, s, generator=gen).float()) if kind == "int" else (lambda *s: torch.randn(*s, generator=gen))
    act_y, res = draw(g.n, g.hi, g.wi, g.ci), draw(groups * g.n, g.hi, g.wi, g.ci)
    if which == "res":
        act_y = None
    if which == "act":
        res = None
    keep = [None if t is None else t.to(gpu_device) for t in (act_y, res)]
    f = L.MovaeFuse()
    if act_y is not None:
        f.ep_act_y, f.ep_act, f.ep_slope = keep[0].data_ptr(), LRELU, SLOPE
    if res is not None:
        f.ep_res = keep[1].data_ptr()
    dx = bt.run_dgrad(L, tiled, gpu_device, g, dy, w, DGRAD[name][0], groups, fuse=f)
    assert f.ep_act_done == 1
    plain = bt.memo((name, kind, groups, "plain dgrad"), lambda: bt.ref_dgrad(g, dy, w))
    judge_actmul(f"{name} input gradient ({groups} groups, {which})", dx, plain, act_y, res, groups, SLOPE, kind)


@gpu
def test_residual_declined_by_the_64_column_kernel(L, tiled, gpu_device):
    """I7 (thin_in_k<64>) has no LDS output tile: ep_act_done comes back 0 and the result is the plain one."""
    g = geo("I7")
    x, _, w, b = data("I7", "int")
    res = torch.ones(g.n, g.ho, g.wo, g.co, device=gpu_device)
    f = L.MovaeFuse()
    f.ep_res = res.data_ptr()
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, FWD["I7"], act=False, fuse=f)
    assert f.ep_act_done == 0
    judge("I7 forward (residual declined)", y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b), (x, w), "int")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def refused(L, lib, call, out, code):
    """The call fails with `code` (-2: the library's unsupported code, L.Unsupported; -1: invalid argument), launches nothing
    (the last kernel's name stays) and leaves the NaN-filled output untouched."""
    before = bt.last(lib)
    with pytest.raises(RuntimeError) as e:
        call()
    assert isinstance(e.value, L.Unsupported) == (code == -2) and (code == -2 or "rc=-1" in str(e.value)), str(e.value)
    torch.cuda.synchronize()
    assert bt.last(lib) == before
    outs = out if isinstance(out, list) else [out]
    for o in outs:
        assert bool(torch.isnan(o.t).all()) and bool((o.buf[:bt.GUARD] == bt.SENTINEL).all()) and bool((o.buf[-bt.GUARD:] == bt.SENTINEL).all())


def fwd_call(L, dev, name, nrm):
    g = geo(name)
    x, _, w, b = data(name, "int")
    xd, wd, bd, y = x.to(dev), w.to(dev), b.to(dev), bt.Out((g.n, g.ho, g.wo, g.co), dev)
    f, keep = bt.fuse_of(L, nrm, dev)
    ws, st = L.workspace(dev), torch.cuda.current_stream().cuda_stream
    pre = "movae_convT2d_fwd_f" if g.tr else "movae_conv2d_fwd_f"
    return (lambda: L.call(pre, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr(), *g.args(), LRELU, SLOPE, ws.data_ptr(), ws.numel(),
                           st, C.byref(f)), (xd, wd, bd, keep)), y


def wgrad_call(L, dev, name, nrm):
    g = geo(name)
    x, dy, _, _ = data(name, "int")
    xd, dyd, dw, db = x.to(dev), dy.to(dev), bt.Out(g.wshape, dev), bt.Out((g.co,), dev)
    f, keep = bt.fuse_of(L, nrm, dev)
    arr = C.c_void_p * 1
    dwp, dbp = arr(dw.ptr()), arr(db.ptr())
    ws, st = L.workspace(dev), torch.cuda.current_stream().cuda_stream
    pre = "movae_convT2d_wgrad_grouped_f" if g.tr else "movae_conv2d_wgrad_grouped_f"
    return (lambda: L.call(pre, 1, dyd.data_ptr(), xd.data_ptr(), dwp, dbp, *g.args(), 0, ws.data_ptr(), ws.numel(), st, C.byref(f)),
            (xd, dyd, dwp, dbp, keep)), [dw, db]


@gpu
@pytest.mark.parametrize("name,op,code", [("I7", "fwd", -2), ("O6", "fwd", -2), ("R7", "wgrad", -2), ("I1", "fwd", -1), ("R2", "wgrad", -1)])
def test_input_transform_refused(L, tiled, gpu_device, name, op, code):
    """A requested input transform on a shape whose kernel cannot apply it: -2 from the sites "thin-channel input conv" (I7),
    "thin-channel output conv" (O6) and "thin wgrad (non-sweep kernels)" (R7).  The transform needs ci % 4 == 0 (include/movae.h),
    which the entry points check first: on the 3-channel x of I1 and R2 (the thin operand of its weight gradient) the request is an
    invalid argument, -1 -- so the "thin-channel input conv" site is reached with I7's 4 channels, and the nrm_side check of
    launch_thin_wgrad_impl (3 thin channels AND the transform on them) by no call."""
    (call, keep), out = (fwd_call if op == "fwd" else wgrad_call)(L, gpu_device, name, bt.norm_params(geo(name).ci, "int", 77))
    refused(L, tiled, call, out, code)


# ---- compute dtype --------------------------------------------------------------------------------------------------------------------
@gpu
def test_bf16_mode_runs_the_same_kernels_to_the_same_bits(L, tiled, gpu_device):
    """conv_thin.h never reads the compute dtype: I1, O1, O8 forward and R1's weight gradient under bf16."""
    def run():
        out = []
        for name in ("I1", "O1", "O8"):
            x, _, w, b = data(name, "normal")
            out.append(bt.run_fwd(L, tiled, gpu_device, geo(name), x, w, b, FWD[name]))
        x, dy, _, _ = data("R1", "normal")
        dws, dbs = bt.run_wgrad(L, tiled, gpu_device, geo("R1"), dy, x, WGRAD["R1"][0])
        return out + [dws[0], dbs[0]]

    f32 = run()
    with bt.mode(L, "bf16"):
        b16 = run()
    for a, b, what in zip(f32, b16, ("I1 y", "O1 y", "O8 y", "R1 dW", "R1 db")):
        assert torch.equal(a, b), f"{what}: differs between the compute dtypes"


# ---- CPU checks of this file's own tables and machinery -------------------------------------------------------------------------------
def test_every_thin_kernel_is_the_expected_kernel_of_a_case():
    expected = set(FWD.values()) | {k for k, _ in DGRAD.values()} | {k for k, _ in WGRAD.values()} | set(LAST_FALLBACK.values())
    assert expected == set(ALL_THIN_KERNELS), (expected ^ set(ALL_THIN_KERNELS))
    assert len(set(ALL_THIN_KERNELS)) == len(ALL_THIN_KERNELS) and not set(UNREACHABLE) & expected


def test_thin_out_tile_plan_never_takes_the_unreachable_forms():
    """thin_out_tile_plan's LDS rule, over every tile it can form: what UNREACHABLE claims."""
    def fits(bwd, th, tw, k, s, cc):
        ih = (th + k - 2) // 2 + 2 if bwd else (th - 1) * s + k
        iw = (tw + k - 2) // 2 + 2 if bwd else (tw - 1) * s + k
        return (ih * iw * (cc + 4) + k * k * 4 * cc) * 4 <= 62 * 1024

    for tw in range(1, 33):
        for k in (1, 2, 3, 4):
            for s in (1, 2, 3):
                if 512 % tw == 0:
                    assert not fits(False, 512 // tw, tw, k, s, 32)      # <false,32,2>
            if tw % 2 == 0 and 256 % (2 * tw) == 0 and 256 // tw // 2 * 2 >= 2:
                assert fits(True, 256 // tw // 2 * 2, tw, k, 2, 32)     # <true,16,1> is never needed


def test_integer_data_is_exact_in_fp32():
    """sum |a| |b| bounds every partial sum of every summation order: the longest reductions here stay below 2^24."""
    g = geo("R6")
    x, dy, _, _ = (t.abs() for t in data("R6", "int"))
    dw, db = bt.ref_wgrad(g, dy, x)
    assert float(dw.max()) + 5 < 2.0 ** 24 and float(db.max()) + 5 < 2.0 ** 24
    xv = bt.virt(data("R1", "int")[0], bt.norm_params(32, "int", 77))
    assert torch.equal(xv * 2, (xv * 2).round()) and float(xv.abs().max()) <= 8
    for name in ("O2", "O9", "I13"):  # the most reduction channels; x scaled to the virtual operand's largest magnitude, 8
        g = geo(name)
        x, dy, w, b = (t.abs() for t in data(name, "int"))
        assert float(bt.ref_fwd(g, x * 8 / 3, w, b).max()) < 2.0 ** 24 and float(bt.ref_dgrad(g, dy, w).max()) < 2.0 ** 24
    xn = bt.virt(data("O1", "normal")[0], bt.norm_params(32, "normal", 77))
    assert torch.equal(xn.float().double(), xn)  # the normal-data transform is exact in fp32


def test_reference_and_float32_order_agree_with_torch():
    """The references on this file's geometries (output padding, 5 x 5 taps, 1 channel), and wgrad_cpu_f32's layout."""
    for name in ("O11", "I6", "R3"):
        g = geo(name)
        x, dy, w, b = data(name, "normal")
        xt, wt = x.double().permute(0, 3, 1, 2).requires_grad_(True), w.double().permute(0, 3, 1, 2).requires_grad_(True)
        if g.tr:
            y = F.conv_transpose2d(xt, wt, b.double(), stride=g.s, padding=g.p, output_padding=CASES[name][8])
        else:
            y = F.conv2d(xt, wt, b.double(), stride=g.s, padding=g.p)
        dx, dw = torch.autograd.grad(y, (xt, wt), dy.double().permute(0, 3, 1, 2))
        assert bt.close(bt.ref_fwd(g, x, w, b), y.permute(0, 2, 3, 1)) and bt.close(bt.ref_dgrad(g, dy, w), dx.permute(0, 2, 3, 1))
        assert bt.close(bt.ref_wgrad(g, dy, x)[0], dw.permute(0, 2, 3, 1))
        assert bt.rel(wgrad_cpu_f32(g, dy, x), dw.permute(0, 2, 3, 1)) < 1e-5


def _raises(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


@pytest.mark.parametrize("kind", KINDS)
def test_the_judges_can_fail(kind):
    """Each judge accepts a correct result computed on the CPU as the kernel forms it, and raises when one element at a tile edge
    (the last row of a 64-row partial, the last column) is off by one unit."""
    gen = torch.Generator().manual_seed(3)
    draw = (lambda *s: torch.randint(-3, 4, s, generator=gen).float()) if kind == "int" else (lambda *s: torch.randn(*s, generator=gen))
    # statistics: 126 rows (I5's ragged block) in partials of 64 rows
    y = draw(126, 32)
    raw = torch.zeros(4, 2, 32)
    for p in range(2):
        rows = y[64 * p:64 * (p + 1)]
        raw[p, 0], raw[p, 1] = rows.sum(0), (rows * rows).sum(0)
    s, sq = fold_stats(raw.flatten(), 4)
    judge_stats("stats", s, sq, y, kind)
    bad = raw.clone()
    bad[1, 0, 31] += 1.0
    _raises(judge_stats, "stats", *fold_stats(bad.flatten(), 4), y, kind)
    bad = raw.clone()
    bad[1, 1, 31] += 1.0
    _raises(judge_stats, "stats", *fold_stats(bad.flatten(), 4), y, kind)
    dropped = raw.clone()  # the last row of the ragged block left out of its partial
    dropped[1, 0] -= y[125]
    if bool((y[125] != 0).any()):
        _raises(judge_stats, "stats", *fold_stats(dropped.flatten(), 4), y, kind)
    # bn_part: 2 groups of 256 rows, four partials each
    g = geo("I9")
    bn_y, nrm = bn_operands(g, kind, 23)
    bn_y = bn_y[:1]
    dx = draw(2, 256, 32)
    z = nrm[0].double() * bn_y.double().view(-1, 32) + nrm[1].double()
    d = dx * torch.where(z > 0, 1.0, nrm[2]).float()
    raw = torch.zeros(2, 4, 2, 32)
    for p in range(4):
        rows = slice(64 * p, 64 * (p + 1))
        raw[:, p, 0], raw[:, p, 1] = d[:, rows].sum(1), (d[:, rows] * bn_y.view(1, -1, 32)[:, rows]).sum(1)
    judge_bn("bn", *fold_bn(raw.flatten(), 2, 4), dx, bn_y, nrm, kind)
    for which in (0, 1):
        bad = raw.clone()
        bad[1, 3, which, 31] += 1.0
        _raises(judge_bn, "bn", *fold_bn(bad.flatten(), 2, 4), dx, bn_y, nrm, kind)
    # ActMul: the reference against torch's own LeakyReLU backward, then one element off
    plain, act_y, res = draw(4, 3, 5, 32).double(), draw(2, 3, 5, 32), draw(4, 3, 5, 32)
    pre = torch.where(act_y > 0, act_y, act_y / SLOPE).double().requires_grad_(True)  # a pre-activation whose LeakyReLU is act_y
    out = F.leaky_relu(pre, SLOPE)
    assert torch.equal(out.detach(), act_y.double())
    want = torch.cat([torch.autograd.grad(out, pre, plain[2 * i:2 * i + 2], retain_graph=True)[0] for i in range(2)]) + res.double()
    assert torch.equal(ref_actmul(plain, act_y, res, 2, SLOPE), want)
    got = want.float()
    judge_actmul("actmul", got, plain, act_y, res, 2, SLOPE, kind)
    bad = got.clone()
    bad[3, 2, 4, 31] += 1.0
    _raises(judge_actmul, "actmul", bad, plain, act_y, res, 2, SLOPE, kind)
    _raises(judge_actmul, "actmul", ref_actmul(plain, act_y, None, 2, SLOPE).float(), plain, act_y, res, 2, SLOPE, kind)  # res forgotten
    # the long-reduction rule
    w64 = draw(64, 27).double() * 1000
    judge_long("long", w64.float(), w64, w64.float())
    off = w64.float().clone()
    off[63, 26] += max(1.0, float(w64.norm()) * 1e-4)
    _raises(judge_long, "long", off, w64, w64.float())
