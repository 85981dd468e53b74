"""The kernels of the conv dispatcher that test_hip_big_tile.py and test_hip_thin.py leave out, through the C entry points and with
the machinery of test_hip_big_tile.py (float64 tap-loop reference, outputs between guard zones that start as NaN, a scratch that
starts as NaN and so counts the split-K slabs written, the asserted name of the kernel that ran):
  * the small tiles of csrc/igemm_v2.h (igemm2_fwd / igemm2_bwd <64,64> and <128,32>, igemm2_wgrad <64,64>, <128,32>, <32,128>) and
    their paired launch igemm2_pair<form, dgrad tile, wgrad tile>;
  * the generic fallback of csrc/conv_igemm.hip (igemm_fwd / igemm_bwd / igemm_wgrad), which takes what the fast path refuses:
    channel counts that are no multiple of 4, operands off a 16-byte boundary, a stride above 2 in the BWD gather form;
  * the split-K reduces (splitk_reduce, _wide, _vec, _flat, _cls, _stats), named by movae_bench_last_reduce().
The dispatcher is pinned as by test_hip_big_tile's `tiled`: no block-internal split-K family (csrc/kgemm.h has its own file), its
own big-tile threshold, split factor 1 unless a case pins another.

Two data sets per case, as in the two other files:
  * integers (x, dy in -3..3, w in -2..2, bias in -8..8, LeakyReLU slope 0.5, norm_params "int" for the virtual operand): every
    partial sum is an integer or half-integer below 2^24 (CPU test below: the longest reduction is 65536 pixels x |3 * 3|), so the
    result must EQUAL float64 through slabs, every reduce kind, `accumulate` and cotangent groups;
  * seeded normal data: rel-L2 < 1e-5 against float64; the 65536-pixel weight gradients (G3, G13) stay below max(1e-5, 4 * e_cpu),
    e_cpu being the rel-L2 of torch's float32 CPU result (test_hip_thin.py's rule).  Both figures are printed.
Every call asserts its kernel's name and the reduce names ("" where nothing was split); split calls assert the slab count.

A pinned split factor s over nk k-tiles becomes ceil(nk / ceil(nk / min(s, nk))) slabs in the forward forms and
ceil(K / (ceil(ceil(K / s) / BK) * BK)) in the weight gradient (BK = 32 in igemm_v2.h, 16 in the generic kernels): the counts
asserted below are worked out from that rule (`slabs_of`), not read off a run."""
import ctypes as C

import pytest
import torch

import test_hip_big_tile as bt
import test_hip_thin as th

gpu = pytest.mark.gpu
L = bt.L  # (the module-scoped library fixture)
SLOPE, LRELU = bt.SLOPE, bt.LRELU
KINDS = bt.KINDS

# conv: (n, hi, wi, ci, co, k, s, p); transposed conv: (..., output_padding)
CASES = {
    # the small igemm_v2.h tiles
    "M1": (4, 9, 7, 36, 72, 3, 2, 1),         # 80 rows = two row blocks, the second ragged; 72 = 64 + 8 columns; K = 324 (general k loop);
                                              # odd 9 x 7 dx: four parity classes of different size; wgrad 72 x 324 ragged both ways
    "M2": (5, 8, 8, 16, 24, 3, 1, 1),         # 320 rows = 2 1/2 blocks of 128; 24 of 32 columns; 24 rows of dW in a 32-row tile
    "M3": (3, 5, 5, 24, 40, 1, 1, 0),         # 1 x 1 taps; weight gradient with N = 24 <= 32
    "M4": (2, 10, 6, 32, 48, 4, 2, 1),        # 4 x 4 taps, 2 x 2 per class
    "M5": (3, 9, 7, 40, 24, 3, 2, 1),         # the fourth conv pair combination
    "M6": (2, 6, 5, 8, 10, 3, 1, 1),          # Nn % 4 != 0 on the fast forward path: scalar store epilogue
    "M6K": (3, 5, 5, 32, 10, 3, 1, 1),        # the same with K = 288 (nine k stages) and 750 outputs, no multiple of 4
    "M7": (4, 2, 2, 64, 72, 3, 2, 1),         # 1 x 1 outputs: tap window (K 576 -> 256), zero-tile shortcut of the wgrad
    "M9": (2, 9, 7, 40, 136, 3, 2, 1),        # three column tiles (64 + 64 + 8); dgrad Cr = 136: launch_bwd2's imbalance split
    "MT1": (4, 5, 4, 72, 36, 3, 2, 1, 1),     # transposed mapping, output padding
    "MT2": (5, 4, 4, 16, 24, 4, 2, 1, 0),
    "MT3": (3, 5, 4, 24, 72, 3, 2, 1, 0),     # odd 9 x 7 output
    "MT4": (2, 5, 3, 8, 8, 3, 2, 1, 1),       # weight gradient with N = 72 < 128 and Cs <= 32
    "MT5": (3, 4, 5, 136, 40, 3, 2, 1, 1),    # the imbalance split in a forward pass: bias and activation applied by splitk_reduce_cls
    # the generic fallback
    "G1": (2, 9, 7, 6, 10, 3, 2, 1),          # nothing divisible by 4; K = 54 (partial k-tile); classes with 1 / 2 / 2 / 4 taps
    "G2": (2, 9, 7, 10, 70, 3, 1, 1),         # two column tiles, 70 = 64 + 6; two row blocks
    "G3": (1, 256, 256, 6, 36, 3, 1, 1),      # 65536 rows reach the <128,64> tile; a 65536-term weight gradient
    "G13": (1, 256, 256, 36, 6, 3, 1, 1),     # the same for the BWD form
    "G5": (2, 9, 9, 8, 32, 3, 3, 0),          # stride 3: nine parity classes, VEC loads
    "G6": (2, 8, 8, 40, 64, 4, 4, 0),         # stride 4 (a patchify conv): sixteen classes
    "G7": (2, 7, 8, 6, 5, 2, 3, 0),           # stride above the kernel size: parity classes with no tap must come out as zero
    "G9": (2, 6, 5, 7, 8, 2, 1, 0),
    "G11": (3, 5, 5, 8, 7, 1, 1, 0),
    "G12": (2, 9, 7, 6, 12, 3, 2, 1),         # the small form of G3's weight gradient
    "G14": (2, 6, 6, 8, 32, 3, 1, 1),         # aligned 8 <- 32 input gradient: generic only where dx is off its boundary
    "G15": (1, 256, 256, 36, 16, 3, 1, 1),    # the same at 36 <- 16 and 65536 rows: the <128,64> tile with VEC loads
    "GT1": (2, 5, 4, 10, 6, 3, 2, 1, 1),      # transposed mapping
    "GT2": (2, 4, 4, 6, 70, 4, 2, 1, 0),
    "GT3": (2, 3, 3, 32, 8, 3, 3, 0, 0),
    "GT6": (2, 3, 3, 6, 10, 2, 3, 0, 0),      # classes with no tap must hold act(bias)
    "GT7": (1, 256, 256, 6, 36, 3, 1, 1, 0),
    "GT8": (2, 2, 2, 64, 40, 4, 4, 0, 0),
    # the reduces
    "V1": (7, 6, 6, 256, 256, 3, 1, 1),       # wgrad: 589824 + 256 outputs >= 2^19, eight 32-pixel chunks
    "V1T": (8, 6, 6, 256, 256, 3, 1, 1),      # the same in nine chunks: the four-slab trips of splitk_reduce_vec and its tail loop
    "V2": (2, 6, 6, 128, 40, 4, 2, 1),        # forward: K = 2048 = 64 k stages over 720 outputs
    "V3": (2, 32, 32, 8, 8, 3, 1, 1),         # wgrad: 2048 pixels = 64 chunks over 576 + 8 outputs
    "S1": (4, 9, 7, 36, 64, 3, 2, 1),         # M1 with 64 columns (splitk_reduce_stats: N / 4 must divide 256)
    "ST1": (4, 5, 4, 72, 64, 3, 2, 1, 1),     # MT1 with 64 columns
}

# (case, what the issue asked for, what it became and why)
SHAPES_CHANGED = [
    ("M1", "5,9,7", "4,9,7: the weight gradient reduces over 5 * 5 * 4 = 100 pixels = 4 k-tiles, which a pinned split of 3 rounds to 2 "
                    "chunks of 64; 80 pixels are 3 k-tiles and 3 slabs.  Still two row blocks with a ragged second one (80 rows)."),
    ("MT1", "3,5,4", "4,5,4: 60 pixels are 2 k-tiles (2 slabs under a pinned split of 3); 80 give 3"),
    ("M6K", "M6 forward split for splitk_reduce with Nn % 4 != 0 and a total that is no multiple of 4",
     "M6 has K = 72 = 3 k stages, so at most 3 slabs: splitk_reduce_flat (splitk_reduce needs 8), and its 600 outputs are a multiple "
     "of 4.  3,5,5, 32->10, k3 s1 p1 has nine k stages and 750 outputs.  M6 itself runs split 3 ways through splitk_reduce_flat."),
    ("V1", "4,6,6, 256->256 with force_split(8)", "7,6,6: 144 pixels are 5 k-tiles, so 5 slabs and splitk_reduce_flat; 252 pixels are 8 "
                                                   "k-tiles in 8 chunks of 32 (8 images would be 9 k-tiles in 5 chunks of 64)"),
    ("V1T", "not named", "V1 with 8 images and force_split(9): 288 pixels in 9 chunks of 32.  Eight slabs are two whole four-slab trips "
                         "of splitk_reduce_vec and never enter its tail loop; nine do."),
    ("V3", "V2's weight gradient with accumulate for splitk_reduce_wide",
     "V2's weight gradient reduces over 18 pixels: one slab, splitk_reduce_flat (asserted as such).  splitk_reduce_wide needs 64 slabs: "
     "2,32,32, 8->8, k3 s1 p1 has 2048 pixels = 64 chunks, with the bias-gradient tail and accumulate."),
    ("S1, ST1", "M1 and MT1 forward with a statistics request and force_split(3)",
     "splitk_reduce_stats needs N / 4 to divide 256 (reduce_stats_shape_ok); 72 and 36 columns fall back to the plain reduce without "
     "statistics.  The same shapes with 64 columns."),
    ("G1 forward, GT1 input gradient at force_split(3)", "3 slabs", "K = 54 is 4 k-tiles of 16: 2 slabs of 2 (the rule in the docstring)"),
    ("G15", "igemm_bwd<128,64,true> not named", "reachable at G13's size with a misaligned dx, so it has a case instead of an UNREACHABLE entry"),
]

# expected kernels: forward, input gradient, weight gradient
FWD = {
    "M1": "igemm2_fwd<64,64>", "M2": "igemm2_fwd<128,32>", "M3": "igemm2_fwd<64,64>", "M4": "igemm2_fwd<64,64>", "M5": "igemm2_fwd<128,32>",
    "M6": "igemm2_fwd<128,32>", "M6K": "igemm2_fwd<128,32>", "M7": "igemm2_fwd<64,64>", "M9": "igemm2_fwd<64,64>",
    "MT1": "igemm2_bwd<64,64>", "MT2": "igemm2_bwd<128,32>", "MT3": "igemm2_bwd<64,64>", "MT4": "igemm2_bwd<128,32>", "MT5": "igemm2_bwd<64,64>",
    "G1": "igemm_fwd<128,32,false>", "G2": "igemm_fwd<64,64,false>", "G3": "igemm_fwd<128,64,false>", "G7": "igemm_fwd<128,32,false>",
    "G9": "igemm_fwd<128,32,false>",
    "GT1": "igemm_bwd<128,32,false>", "GT2": "igemm_bwd<64,64,false>", "GT3": "igemm_bwd<128,32,true>", "GT6": "igemm_bwd<128,32,false>",
    "GT7": "igemm_bwd<128,64,false>", "GT8": "igemm_bwd<64,64,true>",
    "V2": "igemm2_fwd<64,64>", "S1": "igemm2_fwd<64,64>", "ST1": "igemm2_bwd<64,64>",
}
DGRAD = {
    "M1": "igemm2_bwd<64,64>", "M2": "igemm2_bwd<128,32>", "M3": "igemm2_bwd<128,32>", "M4": "igemm2_bwd<128,32>", "M5": "igemm2_bwd<64,64>",
    "M6": "igemm_bwd<128,32,false>", "M7": "igemm2_bwd<64,64>", "M9": "igemm2_bwd<64,64>",
    "MT1": "igemm2_fwd<64,64>", "MT2": "igemm2_fwd<128,32>", "MT3": "igemm2_fwd<128,32>", "MT4": "igemm2_fwd<128,32>", "MT5": "igemm2_fwd<64,64>",
    "G1": "igemm_bwd<128,32,false>", "G2": "igemm_bwd<128,32,false>", "G13": "igemm_bwd<128,64,false>", "G5": "igemm_bwd<128,32,true>",
    "G6": "igemm_bwd<64,64,true>", "G7": "igemm_bwd<128,32,false>", "G9": "igemm_bwd<128,32,false>", "G11": "igemm_bwd<128,32,false>",
    "GT1": "igemm_fwd<128,32,false>", "GT2": "igemm_fwd<128,32,false>", "GT6": "igemm_fwd<128,32,false>",
}
WGRAD = {
    "M1": "igemm2_wgrad<64,64>", "M2": "igemm2_wgrad<32,128>", "M3": "igemm2_wgrad<128,32>", "M4": "igemm2_wgrad<64,64>", "M5": "igemm2_wgrad<32,128>",
    "M6": "igemm_wgrad<64,64,false,true>", "M7": "igemm2_wgrad<64,64>", "M9": "igemm2_wgrad<64,64>",
    "MT1": "igemm2_wgrad<64,64>", "MT2": "igemm2_wgrad<32,128>", "MT3": "igemm2_wgrad<32,128>", "MT4": "igemm2_wgrad<64,64>", "MT5": "igemm2_wgrad<64,64>",
    "G1": "igemm_wgrad<64,64,false,false>", "G2": "igemm_wgrad<64,64,false,false>", "G3": "igemm_wgrad<64,64,true,false>",
    "G13": "igemm_wgrad<64,64,false,true>", "G7": "igemm_wgrad<128,32,false,false>", "G9": "igemm_wgrad<128,32,true,false>",
    "G11": "igemm_wgrad<128,32,false,true>", "G12": "igemm_wgrad<64,64,true,false>",
    "GT1": "igemm_wgrad<64,64,false,false>", "GT2": "igemm_wgrad<64,64,false,false>", "GT6": "igemm_wgrad<64,64,false,false>",
    "V1": "igemm2_wgrad<64,64>", "V1T": "igemm2_wgrad<64,64>", "V2": "igemm2_wgrad<64,64>", "V3": "igemm2_wgrad<64,64>",
}
# the paired entry points: the name the separate kernels imply
PAIRS = {
    "M1": "igemm2_pair<1,64,64,64,64>", "M2": "igemm2_pair<1,128,32,32,128>", "M4": "igemm2_pair<1,128,32,64,64>",
    "M5": "igemm2_pair<1,64,64,32,128>", "MT1": "igemm2_pair<0,64,64,64,64>", "MT2": "igemm2_pair<0,128,32,32,128>",
    "MT4": "igemm2_pair<0,128,32,64,64>",
}
# under the imbalance split of launch_bwd2 (heaviest parity class >= 2x the lightest, at least 4 k-tiles each) the BWD form splits
# on its own at a pinned factor of 1: per-class factors 1 / 2 / 2 / 3, three slabs
IMBALANCED = {("M9", "dgrad"), ("MT5", "fwd")}
LONG = ("G3", "G13")  # weight gradients over 65536 pixels
# misaligned operands (x and w one float past a 16-byte boundary) at channel counts the fast path would take
OFF4 = {
    "M1": ("igemm_fwd<64,64,false>", "igemm_bwd<64,64,false>", "igemm_wgrad<64,64,true,false>"),
    "MT1": ("igemm_bwd<64,64,false>", "igemm_fwd<64,64,false>", "igemm_wgrad<64,64,false,true>"),
}
MISALIGNED_DX = {"G14": "igemm_bwd<128,32,true>", "G15": "igemm_bwd<128,64,true>"}  # aligned operands, dx alone off its boundary
# a pinned split of 3 that the rounding rule turns into 2 slabs: 4 k-tiles (K = 54 or 60 in tiles of 16)
SPLIT3_TWO = {("G1", "fwd"), ("GT1", "dgrad"), ("M6", "wgrad")}

ALL_MID_KERNELS = (
    # igemm_v2.h, launch_fwd2 / launch_bwd2 / launch_wgrad2 at the small tiles, and pair.h's igemm2_pair
    ["igemm2_fwd<64,64>", "igemm2_fwd<128,32>", "igemm2_bwd<64,64>", "igemm2_bwd<128,32>",
     "igemm2_wgrad<64,64>", "igemm2_wgrad<128,32>", "igemm2_wgrad<32,128>"] +
    [f"igemm2_pair<{f},{d},{w}>" for f in (0, 1) for d in ("64,64", "128,32") for w in ("64,64", "32,128")] +
    # conv_igemm.hip, launch_fwd_t / launch_bwd_t / launch_wgrad_t
    [f"igemm_{f}<{t},{v}>" for f in ("fwd", "bwd") for t in ("128,32", "128,64", "64,64") for v in ("false", "true")] +
    [f"igemm_wgrad<{t},{a},{b}>" for t in ("128,32", "64,64") for a in ("false", "true") for b in ("false", "true")] +
    # reduce_launch, finish_splitk, launch_reduce_stats / launch_reduce_bnbwd
    ["splitk_reduce", "splitk_reduce_wide", "splitk_reduce_vec", "splitk_reduce_flat", "splitk_reduce_cls", "splitk_reduce_stats"])
REDUCES_COVERED = {  # reduce: the test that asserts it
    "splitk_reduce": "test_reduce_sixteen_split_lanes", "splitk_reduce_wide": "test_reduce_wide", "splitk_reduce_vec": "test_reduce_vec",
    "splitk_reduce_flat": "test_split_k", "splitk_reduce_cls": "test_split_k", "splitk_reduce_stats": "test_reduce_with_statistics",
}
_SPAN = ("taken only where the fast path refuses operands that are multiples of 4 channels AND 16-byte aligned, which leaves its "
         "buf_span_ok check: a tensor above 2 GiB")
UNREACHABLE = {
    "igemm2_pair<0,64,64,32,128>": "a transposed conv's input gradient has Nn = ci and its weight gradient Cs = ci: the <64,64> FWD-form "
                                   "tile needs ci > 32, the <32,128> weight-gradient tile ci <= 32",
    **{f"igemm_fwd<{t},true>": _SPAN for t in ("128,32", "128,64", "64,64")},
    **{f"igemm_wgrad<{t},true,true>": _SPAN for t in ("128,32", "64,64")},
}


def geo(name):
    return bt.Geo(name, CASES[name])


_DATA = {}


def data(name, kind, groups=1):
    """(x, dy, w, bias) float32 on the CPU, as test_hip_big_tile.data draws them (normal x on a 2^-10 grid: the virtual operand)."""
    key = (name, kind, groups)
    if key not in _DATA:
        g = geo(name)
        gen = torch.Generator().manual_seed(3000 + sum(map(ord, name)) + groups)
        xs, dys = (g.n, g.hi, g.wi, g.ci), (groups * g.n, g.ho, g.wo, g.co)
        if kind == "int":
            x, dy = torch.randint(-3, 4, xs, generator=gen).float(), torch.randint(-3, 4, dys, generator=gen).float()
            w, b = torch.randint(-2, 3, g.wshape, generator=gen).float(), torch.randint(-8, 9, (g.co,), generator=gen).float()
        else:
            x, dy = torch.randn(xs, generator=gen), torch.randn(dys, generator=gen)
            x = ((x * 1024).round() / 1024).clamp(-3.75, 3.75)
            w, b = torch.randn(g.wshape, generator=gen) * float(g.ci * g.k * g.k) ** -0.5, torch.randn(g.co, generator=gen) * 0.1
        _DATA[key] = (x, dy, w, b)
    return _DATA[key]


def ceil_div(a, b):
    return -(-a // b)


def slabs_of(name, op, split, kernel=None):
    """Slabs a pinned split factor gives (the rule in the docstring), by the gather form and k-tile depth of the case's kernel."""
    g = geo(name)
    kernel = kernel or {"fwd": FWD, "dgrad": DGRAD, "wgrad": WGRAD}[op][name]
    bk = 32 if kernel.startswith("igemm2_") else 16
    if op == "wgrad":
        K = g.n * g.hi * g.wi if g.tr else g.n * g.ho * g.wo  # pixels of the small side
        nk = ceil_div(K, bk)
        s = 1 if nk < 2 else min(split, nk)
        return ceil_div(K, ceil_div(ceil_div(K, s), bk) * bk)
    cr = g.ci if op == "fwd" else g.co
    if "_fwd<" in kernel:
        nk = ceil_div(g.k * g.k * cr, bk)
    else:  # BWD form: the parity class with the most taps
        nk = ceil_div(ceil_div(g.k, g.s) ** 2 * cr, bk)
    s = 1 if nk < 2 else min(split, nk)
    return ceil_div(nk, ceil_div(nk, s))


def own_bias_gradient(g, kernel):
    """The tiled conv weight gradient forms its bias gradient itself; the transposed and the generic ones leave it to movae_colsum."""
    return not g.tr and kernel.startswith("igemm2_")


def slab_floats(g, op, groups=1, bias=True, kernel=None):
    """Floats of one split-K slab: the output over all groups; a weight gradient that forms its bias gradient itself keeps the
    partial (one float per output channel) behind each slab."""
    if op == "fwd":
        return g.n * g.ho * g.wo * g.co
    if op == "dgrad":
        return groups * g.n * g.hi * g.wi * g.ci
    return g.co * g.k * g.k * g.ci + (g.co if bias and own_bias_gradient(g, kernel or WGRAD[g.name]) else 0)


def untouched(ws, g, start=0, colsum=False):
    """Nothing was written to the scratch from `start` on -- but for movae_colsum's partials where it ran: at most 256 rows of
    doubles at the start."""
    return ws.slabs(1, start + (512 * g.co if colsum else 0)) == 0


@pytest.fixture
def tiled(L):
    with bt.pinned(L, 0, 1) as lib:
        lib.movae_bench_last_reduce()  # (reading clears what earlier tests left)
        yield lib


def judge(what, got, ref, ops, kind, refkey=None):
    bt.judge(f"mid {what}", got, ref, ops, "f32", kind, refkey)


def reduced(lib, expect, what):
    got = bt.last_reduce(lib)
    assert got == expect, f"{what}: reduced by {got!r}, expected {expect!r}"


def draw_init(g, groups):
    gen = torch.Generator().manual_seed(5)
    return ([torch.randint(-5, 6, g.wshape, generator=gen).float() for _ in range(groups)],
            [torch.randint(-5, 6, (g.co,), generator=gen).float() for _ in range(groups)])


def check_fwd(L, lib, dev, name, kind, plain=False, split=1, reduce=None, ws=None, off="", expect=None, nrm=None):
    """plain: without bias and activation.  split: the pinned factor (the slab count is asserted from it, with a scratch of the
    test's own)."""
    g = geo(name)
    x, _, w, b = data(name, kind)
    kernel = expect or FWD[name]
    slabs = 3 if (name, "fwd") in IMBALANCED and split == 1 else slabs_of(name, "fwd", split, kernel)
    if reduce is None:
        reduce = "" if slabs == 1 else ("splitk_reduce_cls" if kernel.startswith("igemm2_bwd") else "splitk_reduce_flat")
    ws = ws or bt.Scratch(dev)
    y = bt.run_fwd(L, lib, dev, g, x, w, None if plain else b, kernel, nrm=nrm, act=not plain, ws=ws, off=off)
    what = f"{name} forward{' (plain)' if plain else ''}{' (virtual x)' if nrm else ''}"
    reduced(lib, reduce, what)
    assert ws.slabs(slab_floats(g, "fwd")) == (slabs if slabs > 1 else 0), what
    xv = bt.virt(x, nrm)
    judge(what + (f" split {split}" if split > 1 else "") + (" off " + off if off else ""), y,
          lambda xx, ww: bt.ref_fwd(g, xx, ww, None if plain else b, None if plain else SLOPE), (xv, w), kind, what)
    return y


def check_dgrad(L, lib, dev, name, kind, groups=1, split=1, ws=None, off="", expect=None):
    g = geo(name)
    _, dy, w, _ = data(name, kind, groups)
    kernel = expect or DGRAD[name]
    slabs = 3 if (name, "dgrad") in IMBALANCED and split == 1 else slabs_of(name, "dgrad", split, kernel)
    reduce = "" if slabs == 1 else ("splitk_reduce_cls" if kernel.startswith("igemm2_bwd") else "splitk_reduce_flat")
    ws = ws or bt.Scratch(dev)
    dx = bt.run_dgrad(L, lib, dev, g, dy, w, kernel, groups, ws=ws, off=off)
    what = f"{name} input gradient ({groups} groups)"
    reduced(lib, reduce, what)
    assert ws.slabs(slab_floats(g, "dgrad", groups)) == (slabs if slabs > 1 else 0), what
    judge(what + (f" split {split}" if split > 1 else "") + (" off " + off if off else ""), dx, lambda d, ww: bt.ref_dgrad(g, d, ww), (dy, w),
          kind, what)
    return dx


def judge_wgrad(what, g, name, kind, dws, dbs, dy, xv, groups, init, key):
    dyg = dy.view(groups, g.n, g.ho, g.wo, g.co)
    for i in range(groups):
        wh = f"{what} group {i}"
        w0 = init[0][i].double() if init else 0.0
        b0 = init[1][i].double() if init else 0.0
        dw = bt.memo(key + (i, "dw"), lambda: bt.ref_wgrad(g, dyg[i], xv)[0])
        db = dyg[i].double().reshape(-1, g.co).sum(0)
        if kind == "int":
            assert torch.equal(dws[i], (dw + w0).float()), f"{wh}: differs from the exact result at {(dws[i] != (dw + w0).float()).nonzero()[0].tolist()}"
            assert dbs is None or torch.equal(dbs[i], (db + b0).float()), f"{wh}: bias gradient differs from the exact column sums"
        elif name in LONG:
            cpu = bt.memo(key + (i, "cpu32"), lambda: th.wgrad_cpu_f32(g, dyg[i], xv))
            th.judge_long(wh, dws[i], dw + w0, cpu + w0)
            if dbs is not None:
                th.judge_long(wh + " bias", dbs[i], db + b0, dyg[i].reshape(-1, g.co).sum(0) + b0)
        else:
            e, eb = bt.rel(dws[i], dw + w0), 0.0 if dbs is None else bt.rel(dbs[i], db + b0)
            print(f"[mid] {wh}: rel-L2 {e:.2e}, bias gradient {eb:.2e}")
            assert e < 1e-5 and eb < 1e-5, (wh, e, eb)


def check_wgrad(L, lib, dev, name, kind, groups=1, bias=True, acc=False, split=1, reduce=None, ws=None, off="", expect=None, nrm=None):
    g = geo(name)
    x, dy, _, _ = data(name, kind, groups)
    kernel = expect or WGRAD[name]
    slabs = slabs_of(name, "wgrad", split, kernel)
    through_slabs = slabs > 1 or acc
    if reduce is None:  # the generic kernels have no group dimension: one launch and one reduce per group
        reduce = " + ".join(["splitk_reduce_flat"] * (1 if kernel.startswith("igemm2_") else groups)) if through_slabs else ""
    init = draw_init(g, groups) if acc else None
    ws = ws or bt.Scratch(dev)
    dws, dbs = bt.run_wgrad(L, lib, dev, g, dy, x, kernel, groups, nrm=nrm, init=init, bias=bias, ws=ws, off=off)
    what = f"{name} weight gradient ({groups} groups{', accumulate' if acc else ''}{', virtual x' if nrm else ''})"
    reduced(lib, reduce, what)
    # (the generic kernels run group after group over the same slabs, the tiled ones side by side)
    if through_slabs:
        assert ws.slabs(slab_floats(g, "wgrad", bias=bias, kernel=kernel)) == slabs * (groups if kernel.startswith("igemm2_") else 1), what
    else:
        assert untouched(ws, g, colsum=bias and not own_bias_gradient(g, kernel)), what
    judge_wgrad(what + (f" split {split}" if split > 1 else "") + (" off " + off if off else ""), g, name, kind, dws, dbs, dy, bt.virt(x, nrm),
                groups, init, (name, kind, groups, nrm is not None))
    return dws


# ---- every case: forward, input gradient, weight gradient -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("plain", [False, True], ids=["bias_act", "plain"])
@pytest.mark.parametrize("name", [n for n in FWD if n not in ("V2", "S1", "ST1", "M6K")])
def test_forward(L, tiled, gpu_device, name, plain, kind):
    """G7 / GT6: the parity classes without a tap hold act(bias), or zero in the plain run."""
    check_fwd(L, tiled, gpu_device, name, kind, plain)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", list(DGRAD))
def test_input_gradient(L, tiled, gpu_device, name, groups, kind):
    check_dgrad(L, tiled, gpu_device, name, kind, groups)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups,bias", [(1, True), (2, True), (1, False)])
@pytest.mark.parametrize("name", [n for n in WGRAD if n not in ("V1", "V1T", "V2", "V3")])
def test_weight_gradient(L, tiled, gpu_device, name, groups, bias, kind):
    """The generic kernels take their bias gradient from movae_colsum, the tiled conv ones from the kernel's own column sums."""
    dws = check_wgrad(L, tiled, gpu_device, name, kind, groups, bias)
    if name == "M7" and not bias:
        # the zero-tile shortcut (with a bias gradient the first column tile stages its operand for the column sums): a 1 x 1 small
        # side meets tap (kh, kw) at pixel (kh - 1, kw - 1) only, so the taps of row 0 and column 0 multiply padding alone
        assert bool((dws[0][:, 0, :, :] == 0).all()) and bool((dws[0][:, :, 0, :] == 0).all()) and bool((dws[0][:, 1:, 1:, :] != 0).any())


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", ["M1", "M2", "M3", "MT1", "G1"])
def test_accumulate(L, tiled, gpu_device, name, groups, split, kind):
    """Into non-zero dW and db: through the slabs and the reduce at any split factor (G1: the bias gradient through movae_colsum)."""
    tiled.movae_bench_force_split(split)
    assert slabs_of(name, "wgrad", split) == split
    check_wgrad(L, tiled, gpu_device, name, kind, groups, acc=True, split=split)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op,name", [("fwd", "M1"), ("wgrad", "M1"), ("wgrad", "MT1")])
def test_virtual_operand(L, tiled, gpu_device, op, name, kind):
    """BatchNorm + LeakyReLU applied to x on load (gathered operand of the forward and of the conv weight gradient, side 2; small
    side of the transposed one, side 1), on grid data: the transform is exact in fp32.  The shift is non-zero and padding stays zero."""
    nrm = bt.norm_params(geo(name).ci, kind, 77)
    if op == "fwd":
        check_fwd(L, tiled, gpu_device, name, kind, nrm=nrm)
    else:
        check_wgrad(L, tiled, gpu_device, name, kind, 2, nrm=nrm)


# ---- split-K ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("name", ["M1", "M2", "MT1", "M6", "G1", "G2", "GT1"])
def test_split_k(L, tiled, gpu_device, name, op, kind):
    """force_split(3): three slabs on the small tiles, reduced by splitk_reduce_flat (FWD form, weight gradient) or splitk_reduce_cls
    (BWD form: the heaviest parity class in three, the lighter ones in fewer).  The generic BWD form reduces with the plain kinds
    over all slabs: a class whose k range ends before the last slab must still have written zeros there, or the NaN of the scratch
    comes through."""
    tiled.movae_bench_force_split(3)
    assert slabs_of(name, op, 3) == (2 if (name, op) in SPLIT3_TWO else 3) and not any(n in ("M1", "M2", "MT1") for n, _ in SPLIT3_TWO)
    {"fwd": check_fwd, "dgrad": check_dgrad, "wgrad": check_wgrad}[op](L, tiled, gpu_device, name, kind, split=3)


@gpu
def test_forward_takes_the_tap_window(L, tiled, gpu_device):
    """M7's forward with one 32-deep k stage per slab: the tap window leaves K = 2 * 2 * 64 = 256, eight stages, where the plain
    loop over all nine taps (K = 576) would have eighteen."""
    tiled.movae_bench_force_split(256)
    ws = bt.Scratch(gpu_device)
    g = geo("M7")
    x, _, w, b = data("M7", "int")
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, FWD["M7"], ws=ws)
    reduced(tiled, "splitk_reduce", "M7 forward")
    assert ws.slabs(slab_floats(g, "fwd")) == 8
    judge("M7 forward (one k stage per slab)", y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b, SLOPE), (x, w), "int", "M7 forward")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,slabs", [("M1", 11), ("M6K", 9)])
def test_reduce_sixteen_split_lanes(L, tiled, gpu_device, name, slabs, kind):
    """One k stage per slab, 8 <= S < 64 over few outputs: splitk_reduce.  M6K: Nn = 10 and 750 outputs, no multiple of 4."""
    tiled.movae_bench_force_split(256)
    assert slabs_of(name, "fwd", 256) == slabs
    check_fwd(L, tiled, gpu_device, name, kind, split=256, reduce="splitk_reduce")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_reduce_wide(L, tiled, gpu_device, kind):
    """64 slabs: V2's forward (720 outputs, bias and activation applied by the reduce) and V3's weight gradient (576 + 8 outputs:
    the bias-gradient tail, into non-zero dW and db).  V2's own weight gradient reduces over 18 pixels: one slab, splitk_reduce_flat."""
    tiled.movae_bench_force_split(256)
    assert slabs_of("V2", "fwd", 256) == 64 and slabs_of("V3", "wgrad", 256) == 64 and slabs_of("V2", "wgrad", 256) == 1
    check_fwd(L, tiled, gpu_device, "V2", kind, split=256, reduce="splitk_reduce_wide")
    check_wgrad(L, tiled, gpu_device, "V3", kind, acc=True, split=256, reduce="splitk_reduce_wide")
    check_wgrad(L, tiled, gpu_device, "V2", kind, acc=True, split=256, reduce="splitk_reduce_flat")


@gpu
@pytest.mark.parametrize("groups,kind", [(1, "int"), (1, "normal"), (2, "int")])
@pytest.mark.parametrize("name,split", [("V1", 8), ("V1T", 9)])
def test_reduce_vec(L, tiled, gpu_device, name, split, groups, kind):
    """Eight or nine slabs of 589824 + 256 floats per group, so the bias-gradient tail (n1 / out2) goes through the 16-byte reduce too."""
    tiled.movae_bench_force_split(split)
    assert slabs_of(name, "wgrad", split) == split and slab_floats(geo(name), "wgrad") >= 1 << 19
    check_wgrad(L, tiled, gpu_device, name, kind, groups, split=split, reduce="splitk_reduce_vec", ws=bt.Scratch(gpu_device, floats=11 << 20))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["S1", "ST1"])
def test_reduce_with_statistics(L, tiled, gpu_device, name, kind):
    """A statistics request on a split forward without activation: y exact, and the partial sums / sums of squares fold to the float64
    column sums of the stored y (exactly on integer data; a partial is a float32 sum of at most 32 terms).  ST1: the BWD form,
    per-class slab counts inside the same kernel."""
    tiled.movae_bench_force_split(3)
    g = geo(name)
    x, _, w, b = data(name, kind)
    rows = g.n * g.ho * g.wo
    parts = ceil_div(rows, 32)  # 16 row groups of 16 column quads per block, two rows per thread
    st = bt.Out((parts * 2 * g.co,), gpu_device)
    f = L.MovaeFuse()
    f.stats, f.stats_cap = st.ptr(), st.t.numel()
    ws = bt.Scratch(gpu_device)
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, FWD[name], act=False, ws=ws, fuse=f)
    reduced(tiled, "splitk_reduce_stats", f"{name} forward")
    assert ws.slabs(slab_floats(g, "fwd")) == 3 and f.stats_parts == parts
    judge(f"{name} forward (statistics, split 3)", y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b), (x, w), kind)
    s, sq = th.fold_stats(st.get(f"{name} statistics"), parts, g.co)
    th.judge_stats(f"{name} statistics", s, sq, y.view(-1, g.co), kind, R=32)


# ---- the paired entry points --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", list(PAIRS))
def test_paired_entry_points(L, tiled, gpu_device, name, groups, split, kind):
    """One launch for the input gradient and the weight gradient with its bias gradient.  A tiled input gradient is paired only if
    the workspace leaves 32 MiB beside its slabs: a scratch of 2^24 floats.  The weight gradient's slabs lie behind the input
    gradient's (rounded up to 256 bytes) and behind a second workspace header."""
    tiled.movae_bench_force_split(split)
    g = geo(name)
    x, dy, w, _ = data(name, kind, groups)
    ws = bt.Scratch(gpu_device, floats=1 << 24)
    dx, dws, dbs = bt.run_pair(L, tiled, gpu_device, g, dy, w, x, PAIRS[name], groups, ws=ws)
    sd, sw = slabs_of(name, "dgrad", split), slabs_of(name, "wgrad", split)
    what = f"{name} pair ({groups} groups, split {split})"
    first = "splitk_reduce_cls" if DGRAD[name].startswith("igemm2_bwd") else "splitk_reduce_flat"
    reduced(tiled, " + ".join(([first] if sd > 1 else []) + (["splitk_reduce_flat"] if sw > 1 else [])), what)
    per_d = slab_floats(g, "dgrad", groups)
    used = ceil_div(sd * per_d * 4, 256) * 64 if sd > 1 else 0  # floats
    assert ws.slabs(per_d, 0, used) == (sd if sd > 1 else 0), what
    if sw > 1:
        assert ws.slabs(slab_floats(g, "wgrad"), used + bt.WS_HEADER) == sw * groups, what
    else:
        assert untouched(ws, g, used + bt.WS_HEADER, colsum=g.tr), what
    judge(f"{name} input gradient ({groups} groups)" + (" paired, split 3" if split > 1 else " paired"), dx, lambda d, ww: bt.ref_dgrad(g, d, ww),
          (dy, w), kind, f"{name} input gradient ({groups} groups)")
    judge_wgrad(what, g, name, kind, dws, dbs, dy, x.double(), groups, None, (name, kind, groups, False))


# ---- what the fast path refuses -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(OFF4))
def test_misaligned_operands_take_the_generic_kernels(L, tiled, gpu_device, name, kind):
    """x and w one float past a 16-byte boundary (valid memory inside a larger buffer): the generic kernels with scalar loads,
    exact, and on integer data therefore equal to what the aligned call gives."""
    fwd, dgrad, wgrad = OFF4[name]
    y = check_fwd(L, tiled, gpu_device, name, kind, off="xw", expect=fwd)
    dx = check_dgrad(L, tiled, gpu_device, name, kind, off="w", expect=dgrad)
    dw = check_wgrad(L, tiled, gpu_device, name, kind, off="x", expect=wgrad)[0]
    if kind == "int":
        assert torch.equal(y, check_fwd(L, tiled, gpu_device, name, kind))
        assert torch.equal(dx, check_dgrad(L, tiled, gpu_device, name, kind))
        assert torch.equal(dw, check_wgrad(L, tiled, gpu_device, name, kind)[0])


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MISALIGNED_DX))
def test_misaligned_input_gradient_alone(L, tiled, gpu_device, name, kind):
    """Aligned operands at channel counts the fast path takes; only dx lies off its boundary.  The VEC loads of igemm_bwd without a
    large stride, and the only way to its <128,64,true> form short of a 768 x 768 image at stride 3."""
    check_dgrad(L, tiled, gpu_device, name, kind, off="y", expect=MISALIGNED_DX[name])


@gpu
@pytest.mark.parametrize("op", ["fwd", "wgrad"])
def test_input_transform_refused_by_the_generic_kernels(L, tiled, gpu_device, op):
    """The fused input transform needs ci % 4 == 0 (an invalid argument otherwise), so a generic kernel meets it with misaligned
    operands (M1's forward) or where the other operand refuses the fast path (G11's weight gradient, co = 7): MOVAE_EUNSUPPORTED,
    nothing launched, the output untouched."""
    dev = gpu_device
    name = "M1" if op == "fwd" else "G11"
    g = geo(name)
    x, dy, w, b = data(name, "int")
    f, keep = bt.fuse_of(L, bt.norm_params(g.ci, "int", 77), dev)
    ws, st = L.workspace(dev), torch.cuda.current_stream().cuda_stream
    if op == "fwd":
        xd, wd, bd, y = bt.put(x, dev, True), bt.put(w, dev, True), b.to(dev), bt.Out((g.n, g.ho, g.wo, g.co), dev)
        th.refused(L, tiled, lambda: L.call("movae_conv2d_fwd_f", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr(), *g.args(), LRELU, SLOPE,
                                            ws.data_ptr(), ws.numel(), st, C.byref(f)), y, -2)
    else:
        xd, dyd, dw, db = x.to(dev), dy.to(dev), bt.Out(g.wshape, dev), bt.Out((g.co,), dev)
        arr = C.c_void_p * 1
        dwp, dbp = arr(dw.ptr()), arr(db.ptr())
        th.refused(L, tiled, lambda: L.call("movae_conv2d_wgrad_grouped_f", 1, dyd.data_ptr(), xd.data_ptr(), dwp, dbp, *g.args(), 0, ws.data_ptr(),
                                            ws.numel(), st, C.byref(f)), [dw, db], -2)


# ---- compute dtype ------------------------------------------------------------------------------------------------------------------
@gpu
def test_bf16_mode_runs_the_same_kernels_to_the_same_bits(L, tiled, gpu_device):
    """The small tiles have no bf16 form: M1's three results under set_compute_dtype("bf16")."""
    def run():
        return (check_fwd(L, tiled, gpu_device, "M1", "normal"), check_dgrad(L, tiled, gpu_device, "M1", "normal"),
                check_wgrad(L, tiled, gpu_device, "M1", "normal")[0])

    f32 = run()
    with bt.mode(L, "bf16"):
        b16 = run()
    for a, b, what in zip(f32, b16, ("y", "dx", "dW")):
        assert torch.equal(a, b), f"M1 {what}: differs between the compute dtypes"


# ---- CPU checks of this file's own tables and machinery -----------------------------------------------------------------------------
def test_every_kernel_is_the_expected_kernel_of_a_case_or_unreachable():
    expected = (set(FWD.values()) | set(DGRAD.values()) | set(WGRAD.values()) | set(PAIRS.values()) | {k for v in OFF4.values() for k in v} |
                set(MISALIGNED_DX.values()) | set(REDUCES_COVERED))
    assert len(set(ALL_MID_KERNELS)) == len(ALL_MID_KERNELS)
    assert expected | set(UNREACHABLE) == set(ALL_MID_KERNELS), (expected | set(UNREACHABLE)) ^ set(ALL_MID_KERNELS)
    assert not expected & set(UNREACHABLE)
    for test in set(REDUCES_COVERED.values()):
        assert callable(globals()[test])


@pytest.mark.parametrize("name", ["G5", "G6", "G7", "GT6", "M9"])
def test_reference_agrees_with_torch(name):
    """Strides above 2, strides above the kernel size (outputs / input gradients no tap reaches) and 136 channels."""
    import torch.nn.functional as F

    g = geo(name)
    x, dy, w, b = data(name, "normal")
    xt, wt = x.double().permute(0, 3, 1, 2).requires_grad_(True), w.double().permute(0, 3, 1, 2).requires_grad_(True)
    if g.tr:
        y = F.conv_transpose2d(xt, wt, b.double(), stride=g.s, padding=g.p, output_padding=CASES[name][8])
    else:
        y = F.conv2d(xt, wt, b.double(), stride=g.s, padding=g.p)
    assert tuple(y.shape) == (g.n, g.co, g.ho, g.wo)
    dx, dw = torch.autograd.grad(y, (xt, wt), dy.double().permute(0, 3, 1, 2))
    assert bt.close(bt.ref_fwd(g, x, w, b), y.permute(0, 2, 3, 1)) and bt.close(bt.ref_dgrad(g, dy, w), dx.permute(0, 2, 3, 1))
    rw, rb = bt.ref_wgrad(g, dy, x)
    assert bt.close(rw, dw.permute(0, 2, 3, 1)) and bt.close(rb, dy.double().sum((0, 1, 2)))
    if name in ("G7", "GT6"):  # the stride skips pixels: what no tap reaches is exactly the bias / zero
        plain = bt.ref_fwd(g, x, w) if g.tr else bt.ref_dgrad(g, dy, w)
        assert bool((plain == 0).all(-1).any())


def test_integer_data_is_exact_in_fp32():
    """sum |a| |b| bounds every partial sum of every summation order: the longest reductions here stay below 2^24."""
    two24 = 2.0 ** 24
    assert 65536 * 9 < two24
    for name in ("G3", "G13", "V1T", "V2", "V3", "M9", "MT5"):  # 65536 pixels; the most channels and taps
        g = geo(name)
        x, dy, w, b = (t.abs() for t in data(name, "int", 2))
        dw, db = bt.ref_wgrad(g, dy[:g.n], x)
        assert float(dw.max()) + 5 < two24 and float(db.max()) + 5 < two24
        # x scaled to the virtual operand's largest magnitude, 8
        assert float(bt.ref_fwd(g, x * 8 / 3, w, b).max()) < two24 and float(bt.ref_dgrad(g, dy, w).max()) < two24
    for name in ("M1", "MT1"):
        xv = bt.virt(data(name, "int")[0], bt.norm_params(geo(name).ci, "int", 77))
        assert torch.equal(xv * 2, (xv * 2).round()) and float(xv.abs().max()) <= 8
        xn = bt.virt(data(name, "normal")[0], bt.norm_params(geo(name).ci, "normal", 77))
        assert torch.equal(xn.float().double(), xn)  # the normal-data transform is exact in fp32
    for name in ("S1", "ST1"):  # the statistics: column sums of y^2, and so every partial of them
        g = geo(name)
        x, _, w, b = data(name, "int")
        y = bt.ref_fwd(g, x, w, b).reshape(-1, g.co)
        assert float((y * y).sum(0).max()) < two24


def test_split_rule_on_the_cases_that_state_a_count():
    """What the docstring's rounding rule gives where the tests assert a count the issue names."""
    for name in ("M1", "M2", "MT1"):
        assert [slabs_of(name, op, 3) for op in ("fwd", "dgrad", "wgrad")] == [3, 3, 3], name
    assert slabs_of("M7", "fwd", 256) == 18  # without the tap window: K = 576; the test asserts the 8 of K = 256
    assert slabs_of("M1", "fwd", 256) == 11 and slabs_of("V2", "fwd", 256) == 64 and slabs_of("V1", "wgrad", 8) == 8
    assert [slabs_of(n, op, 3) for n in ("G1", "G2", "GT1") for op in ("fwd", "dgrad", "wgrad")] == [2, 3, 3, 3, 3, 3, 3, 2, 3]
    assert [slabs_of("M6", op, 3) for op in ("fwd", "dgrad", "wgrad")] == [3, 3, 2]
    # the parity classes of the imbalance split: 1, 2, 2 and 4 taps of 136 channels in 32-deep k-tiles
    nk = [ceil_div(t * 136, 32) for t in (1, 2, 2, 4)]
    assert max(nk) >= 2 * min(nk) and min(nk) >= 4 and [ceil_div(max(nk) // min(nk) * k, max(nk)) for k in nk] == [1, 2, 2, 3]
