"""The block-internal split-K family (csrc/kgemm.h: kgemm_k in its FWD and BWD gather forms, kwgrad_k, and the paired launch
kpair_k) through the C entry points, with the machinery of test_hip_big_tile.py: float64 tap-loop reference, outputs between guard
zones that start as NaN, a scratch that starts as NaN and so counts the slabs written, the asserted FULL name of the kernel that ran.
The dispatcher is pinned the other way round from the other exact files: movae_bench_force_kgemm(1) (every shape the family can
serve takes it), the dispatcher's own big-tile threshold, split factor 0 (its own choice) unless a case pins one.

Two data sets per case:
  * integers (x, dy in -3..3, w in -2..2, bias in -8..8, LeakyReLU slope 0.5, norm_params "int" for the virtual operand): every
    partial sum is an integer or half-integer below 2^24 (CPU test below), so the result must EQUAL float64 through the fold of the
    KS waves, the slabs of kwgrad_k, `accumulate` and cotangent groups;
  * seeded normal data: rel-L2 < 1e-5 against float64; the figure is printed with the kernel's name.
The side products are checked partial by partial (a partial written to the wrong class or group slot can still sum to the right
total): a partial is a float32 sum of 32 terms, so on normal data it is held to 34 * 2^-24 * sum |term| -- 31 additions, up to two
roundings of a term (the square / the product d * y, and d itself), one to spare; on integer data the statistics are exact.

The split degree KS follows the tile count (choose_ks: 4 up to 1024 32 x 32 tiles, 2 up to 2048, 1 above); a wave's slice of the
reduction is ceil(K / 8 / KS) groups of 8 and runs through a ring of six 2-group chunks.  The tile counts, slice lengths, ring
trips and class windows the case table states are worked out from those rules in `ks_of`, `slices`, `trips`, `class_windows`
(CPU tests at the end), not read off a run.  kwgrad_k splits the IMAGES of its reduction instead: groups of 8 images over the KS waves
(`slices(8 * ceil(n / 8), KS)`), each group once per small-side position whose tap meets the image (`kw_window`), through a ring of
eight one-group chunks (`kw_chunks`); its cases reach waves with 2 and 3 groups, a fourth wave with data, a last group of one image,
up to five trips round the ring, and non-square sides.  KS = 8 exists only under MOVAE_KGEMM_KS=8, read once per process: one test starts one
child process that runs this file's check functions with it."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":  # the KS = 8 child: no conftest in front of it
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

import test_hip_big_tile as bt

gpu = pytest.mark.gpu
L = bt.L  # (the module-scoped library fixture)
SLOPE, LRELU = bt.SLOPE, bt.LRELU
KINDS = bt.KINDS
U = 2.0 ** -24
NORM_MAX_C = 1024

# conv: (n, hi, wi, ci, co, k, s, p); transposed conv: (..., output_padding)
CASES = {
    # FWD gather form: conv forward
    "KF1": (12, 4, 4, 64, 96, 3, 2, 1),       # M 48 (ragged second row tile), three column tiles, K 576: 18 groups per slice = one trip + 3
    "KF2": (5, 5, 7, 16, 40, 3, 2, 1),        # M 60, a partial column tile, K 144: slices 5/5/5/3, no whole trip
    "KF3": (3, 8, 8, 32, 64, 3, 1, 1),        # stride 1, padding on all sides
    "KF4": (2, 6, 6, 48, 36, 1, 1, 0),        # 1 x 1 taps, K 48: the fourth slice is empty
    "KF5": (2, 9, 9, 24, 32, 4, 2, 1),        # 24 channels: a tap ends inside a 16-index chunk; exactly one tile, one trip, remainder 0
    "KF6": (2, 6, 5, 8, 8, 3, 1, 1),          # the narrowest shape the family takes, K 72: empty slice
    "KF7": (5, 2, 2, 32, 40, 3, 2, 1),        # 1 x 1 output: the tap window (K 288 -> 128, wjump != 0)
    "KF8": (4, 1, 1, 32, 64, 3, 1, 1),        # 1 x 1 image: the window is the centre tap (a windowed geometry is no linear layer: kgemm_k)
    "KF9": (3, 4, 4, 128, 32, 3, 2, 1),       # K 1152: three whole trips, remainder 0
    "KN": (2, 2, 2, 1024, 8, 1, 1, 0),        # virtual operand at exactly NORM_MAX_C (2 trips + 4)
    "KN+": (2, 2, 2, 1032, 8, 1, 1, 0),       # ... and above it: refused with the virtual operand, taken without
    "KL2": (5, 79, 83, 8, 32, 3, 1, 1),       # 32785 rows = 1025 tiles: KS 2, the last block's second tile absent, slices 5/4
    "KL1": (5, 79, 83, 8, 64, 3, 1, 1),       # 2050 tiles: KS 1, the last block has one tile of four
    # BWD gather form: transposed conv forward
    "KB1": (8, 2, 2, 128, 64, 3, 2, 1, 1),    # classes with 1 / 2 / 2 / 4 taps
    "KB2": (6, 1, 1, 64, 40, 3, 2, 1, 1),     # every class's window shrinks to one tap; Mc = 6
    "KB3": (3, 5, 3, 32, 32, 4, 2, 1, 0),     # k4, ragged class rows (45)
    "KB3b": (4, 1, 1, 32, 16, 4, 2, 1, 0),    # k4 windowed to 1 x 1
    "KB4": (2, 3, 3, 16, 8, 1, 2, 0, 1),      # three of four classes have no tap: act(bias) there, zero in the plain run
    "KB6": (4, 1, 3, 32, 16, 3, 2, 1, 1),     # non-square: windows 1x1, 1x2, 1x1, 1x2
    "KB7": (2, 5, 4, 32, 16, 3, 2, 1, 0),     # 9 x 7 output: refused
    "KBL2": (1, 91, 91, 8, 32, 3, 2, 1, 1),   # 4 x 259 tiles: KS 2 with an absent tile
    "KBL1": (1, 91, 91, 8, 64, 3, 2, 1, 1),   # KS 1
    # side products: whole 32-row tiles per cotangent group (and class) -- and the refusals
    "SB4": (8, 4, 4, 40, 16, 3, 2, 1),        # conv: dx in the BWD form, 32 rows per group and class
    "SB8": (8, 8, 8, 40, 16, 3, 2, 1),        # ... 128
    "SB5": (5, 4, 4, 40, 16, 3, 2, 1),        # 20 rows per class: the BatchNorm-backward epilogue is refused
    "SF4": (8, 4, 4, 40, 16, 3, 2, 1, 1),     # transposed: dx in the FWD form, 128 rows per group
    "SF8": (8, 8, 8, 40, 16, 3, 2, 1, 1),
    "SF5": (5, 4, 4, 40, 16, 3, 2, 1, 1),     # 80 rows
    "SBL2": (8, 56, 74, 32, 8, 3, 2, 1),      # dx: 4 x 259 tiles of whole rows: KS 2 with an absent tile
    "SFL2": (8, 50, 82, 32, 8, 3, 2, 1, 1),   # dx: 1025 tiles
    # the paired entry points
    "P3": (3, 4, 4, 64, 40, 3, 2, 1, 1),      # convT, co no multiple of 32: the weight gradient stays tiled, <64,64>
    "P4": (3, 4, 4, 32, 40, 3, 2, 1, 1),      # ... <32,128>
    "P5": (2, 6, 6, 32, 40, 1, 1, 0),         # conv 1 x 1 taps, N = 32: igemm2_wgrad<128,32> does not pair
    "P6": (3, 4, 4, 64, 32, 3, 2, 1, 1),      # convT with co = 32: the weight gradient goes to kwgrad_k
    # kwgrad_k
    "KW1": (20, 4, 4, 32, 40, 3, 2, 1),       # M 40 ragged, 20 images = 8 + 8 + 4, the fourth slice empty, padding-only positions skipped
    "KW2": (6, 3, 3, 24, 32, 4, 2, 1, 0),     # convT mapping
    "KW3": (9, 2, 2, 32, 16, 3, 2, 1),        # 1 x 1 small side: taps that never meet the image
    "KW4": (3, 2, 2, 1216, 72, 3, 1, 1),      # 3 x 342 = 1026 tiles: KS 2 with an absent row tile
    "KW5": (3, 2, 2, 2432, 72, 3, 1, 1),      # 2052 tiles: KS 1
    "KW6": (40, 8, 10, 32, 40, 3, 2, 1),      # non-square; 40 images = 5 groups of 8: image slices 2/2/1/0, up to 40 chunks = 5 trips of the ring
    "KW7": (57, 3, 2, 24, 32, 3, 2, 1, 1),    # convT, non-square; 57 images: slices 2/2/2/2, the last group holds one image
    "KW8": (17, 2, 2, 1216, 72, 3, 1, 1),     # KW4's 1026 tiles (KS 2) with 17 images: slices 2/1
    "KW9": (72, 4, 5, 32, 40, 3, 2, 1),       # 9 groups: slices 3/3/3/0, and 2/2/2/2/1/0/0/0 at KS 8
    "KW4T": (3, 2, 2, 72, 1216, 3, 1, 1, 0),  # the same two with the convT mapping (virtual operand on the small side at KS 2 / 1)
    "KW5T": (3, 2, 2, 72, 2432, 3, 1, 1, 0),
}

# (case, what the issue asked for, what it became and why)
SHAPES_CHANGED = [
    ("KF8", "kgemm_k or linear_small_k", "kgemm_k<0,4,4,false>: the tap window turns the geometry into 1 x 1 taps with a windowed weight "
            "(wlen != 0), which is_linear() excludes, so linear_small_k never sees it under this pin"),
    ("weight gradient with 9 groups", "refused by kwgrad_k, the tiled name asserted",
     "the entry point itself refuses more than 8 groups (invalid argument, nothing launched): kwgrad_k's own G > 8 check cannot be "
     "reached through the C ABI.  The test asserts that refusal and an untouched output."),
    ("P5 / P6 expected last kernel", "igemm2_wgrad<128,32> / kwgrad_k<4,4,0>",
     "two main launches: movae_bench_last_kernel() names both, 'kgemm_k<1,4,4,false> + igemm2_wgrad<128,32>' and "
     "'kgemm_k<0,4,4,false> + kwgrad_k<4,4,0>'; the full string is asserted"),
    ("P6 dW", "equal to the tiled weight gradient alone", "its weight gradient is kwgrad_k's, so it is compared bit for bit with the "
              "stand-alone kwgrad_k call (and, like every other, with float64)"),
    ("KW4T, KW5T, SBL2, SFL2", "not named", "kwgrad_k<4,2,1> / <4,1,1> need a transposed conv of more than 1024 tiles; the BatchNorm-backward "
                                            "and ActMul epilogues at KS 2 need whole 32-row tiles per group, which KL2 / KBL2 (ragged) do not have"),
    ("largest tile sum of squares 170309", "asserted figure", "depends on the seed of the draw; the CPU test asserts < 2^24 on this file's data"),
]

FORCED_KS = 0  # the child process under MOVAE_KGEMM_KS=8 sets 8


def geo(name):
    return bt.Geo(name, CASES[name])


_DATA = {}


def data(name, kind, groups=1):
    """(x, dy, w, bias) float32 on the CPU, as test_hip_big_tile.data draws them (normal x on a 2^-10 grid: the virtual operand)."""
    key = (name, kind, groups)
    if key not in _DATA:
        g = geo(name)
        gen = torch.Generator().manual_seed(7000 + sum(map(ord, name)) + groups)
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


# ---- the rules of kgemm.h, transcribed ------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def ks_of(tiles, forced=0):
    """choose_ks: waves that split one tile's reduction (forced: MOVAE_KGEMM_KS)."""
    if forced:
        return forced
    return 4 if tiles <= 1024 else (2 if tiles <= 2048 else 1)


def slices(K, KS):
    """Groups of 8 reduction indices per wave of a tile."""
    g8 = K // 8
    gper = ceil_div(g8, KS)
    return [max(0, min(g8, (s + 1) * gper) - s * gper) for s in range(KS)]


def trips(groups, cg=2, nb=6):
    """(whole trips round the register ring, chunks left) of a slice of `groups` groups."""
    nch = ceil_div(groups, cg) if groups > 0 else 0
    return nch // nb, nch % nb


def form_of(g, op):
    """(gather form, images' output grid H x W, columns N, reduction channels Cr, gathered grid) of the forward / input gradient."""
    if op == "fwd":
        return (1 if g.tr else 0), g.ho, g.wo, g.co, g.ci, (g.hi, g.wi)
    return (0 if g.tr else 1), g.hi, g.wi, g.ci, g.co, (g.ho, g.wo)


def tiles_of(g, op, groups=1):
    form, H, W, N, _, _ = form_of(g, op)
    nimg = g.n * (groups if op == "dgrad" else 1)
    if form == 0:
        return ceil_div(nimg * H * W, 32) * ceil_div(N, 32)
    return ceil_div(nimg * (H // g.s) * (W // g.s), 32) * ceil_div(N, 32) * g.s * g.s


def takes(g, op, nrm=False):
    """launch_kfwd / launch_kbwd under the forced pin: the shape conditions (every operand of these tests is 16-byte aligned)."""
    form, H, W, N, Cr, _ = form_of(g, op)
    if Cr % 8 or N % 4 or (nrm and Cr > NORM_MAX_C):
        return False
    return form == 0 or (g.s <= 2 and H % g.s == 0 and W % g.s == 0)


def window_k(g):
    """tap_window: the reduction length of a conv forward with a 1 x 1 output (the taps that can meet the image)."""
    if g.tr or g.ho != 1 or g.wo != 1 or g.p >= g.k:
        return g.k * g.k * g.ci
    return min(g.k - g.p, g.hi) * min(g.k - g.p, g.wi) * g.ci


def class_windows(g, op="fwd"):
    """launch_kbwd: per output-parity class (ph * s + pw) the window (taps in h, taps in w) that meets the gathered image."""
    _, H, W, _, _, (Hi, Wi) = form_of(g, op)
    s, out = g.s, []
    for c in range(s * s):
        win = []
        for par, Hg, Ho in ((c // s, Hi, H), (c % s, Wi, W)):
            k0 = (par + g.p) % s
            nA = (g.k - k0 + s - 1) // s if k0 < g.k else 0
            q = (par + g.p - k0) // s
            lo, hi = max(0, q - (Hg - 1)), min(nA - 1, q + Ho // s - 1)
            win.append(hi - lo + 1 if hi >= lo else 0)
        out.append((0, 0) if 0 in win else tuple(win))
    return out


def kname(form, tiles, nrm=False, forced=0):
    ks = ks_of(tiles, forced)
    return f"kgemm_k<{form},{8 if ks == 8 else 4},{ks},{'true' if nrm else 'false'}>"


def kwname(tiles, nside=0, forced=0):
    ks = ks_of(tiles, forced)
    return f"kwgrad_k<{8 if ks == 8 else 4},{ks},{nside}>"


def kw_tiles(g, groups=1):
    cs, cb = (g.ci, g.co) if g.tr else (g.co, g.ci)
    return ceil_div(cs, 32) * (g.k * g.k * cb // 32) * groups


def kw_window(g, kh, kw):
    """kwgrad_body: the small-side positions (rows, columns) whose tap (kh, kw) meets the big side; a 0: the tile is a zero tile."""
    Hs, Ws, Hb, Wb = (g.hi, g.wi, g.ho, g.wo) if g.tr else (g.ho, g.wo, g.hi, g.wi)

    def span(k, S, B):
        lo = ceil_div(g.p - k, g.s) if g.p - k > 0 else 0
        hi = min(S - 1, (B - 1 + g.p - k) // g.s) if B - 1 + g.p - k >= 0 else -1
        return max(0, hi - lo + 1)

    return span(kh, Hs, Hb), span(kw, Ws, Wb)


def kw_chunks(g, kh, kw, ks, split=1, nbw=8):
    """Per wave of a tile at tap (kh, kw), first slab: (chunks = image groups of the wave's slice x positions, whole trips round the
    ring of NBW = 8 one-group chunks, chunks left)."""
    nh, nw = kw_window(g, kh, kw)
    n = min(g.n, ceil_div(ceil_div(g.n, split), 8) * 8)
    return [(ng * nh * nw, ng * nh * nw // nbw, ng * nh * nw % nbw) for ng in slices(8 * ceil_div(n, 8), ks)]


def kw_slabs(n, split):
    return ceil_div(n, ceil_div(ceil_div(n, split), 8) * 8)


# what the tiled dispatcher launches where the family refuses
TILED = {("KB7", "fwd"): "igemm2_bwd<128,32>", ("KN+", "fwd"): "igemm2_fwd<128,32>", ("SB5", "dgrad"): "igemm2_bwd<64,64>",
         ("SF5", "dgrad"): "igemm2_fwd<64,64>"}


def expect(name, op, groups=1, nrm=False, forced=None):
    """forced None: this process's own degree (FORCED_KS: 8 in the child, else by tile count)."""
    forced = FORCED_KS if forced is None else forced
    g = geo(name)
    if not takes(g, op, nrm):
        return TILED[(name, op)]
    return kname(form_of(g, op)[0], tiles_of(g, op, groups), nrm, forced)


FWD_CASES = ["KF1", "KF2", "KF3", "KF4", "KF5", "KF6", "KF7", "KF8", "KF9", "KN", "KN+", "KL2", "KL1",
             "KB1", "KB2", "KB3", "KB3b", "KB4", "KB6", "KB7", "KBL2", "KBL1"]
DGRAD_CASES = ["KF1", "KF3", "KF9",                                                  # conv: BWD form (stride 1: one class)
               "KB1", "KB2", "KB3", "KB3b", "KB4", "KB6", "KB7", "KBL2", "KBL1"]    # transposed: FWD form, no parity condition
VIRTUAL_CASES = ["KF1", "KN", "KN+", "KL2", "KL1", "KB1", "KB6", "KBL2", "KBL1"]
STATS_CASES = ["KF1", "KF2", "KF6", "KL2", "KB1", "KB3", "KBL2"]
BN_CASES = ["SB4", "SB8", "SF4", "SF8", "SBL2", "SFL2"]
# paired entry points: (tiled weight gradient alone, last kernel of the paired call)
PAIRS = {
    "KF1": ("igemm2_wgrad<64,64>", "kpair_k<1,64,64>"),
    "KF9": ("igemm2_wgrad<32,128>", "kpair_k<1,32,128>"),
    "P3": ("igemm2_wgrad<64,64>", "kpair_k<0,64,64>"),
    "P4": ("igemm2_wgrad<32,128>", "kpair_k<0,32,128>"),
    "P5": ("igemm2_wgrad<128,32>", "kgemm_k<1,4,4,false> + igemm2_wgrad<128,32>"),
    "P6": ("kwgrad_k<4,4,0>", "kgemm_k<0,4,4,false> + kwgrad_k<4,4,0>"),
}
KW_CASES = ["KW1", "KW2", "KW3", "KW4", "KW5", "KW4T", "KW5T", "KW6", "KW7", "KW8", "KW9"]
# the KS = 8 child: (check, arguments)
KS8_RUNS = [("fwd", "KF1"), ("fwd", "KF4"), ("fwd", "KF9"), ("fwd", "KB1"), ("fwd", "KB4"), ("virtual", "KF1"), ("virtual", "KB1"),
            ("stats", "KF1"), ("stats", "KB1"), ("kw", "KW1"), ("kw", "KW2"), ("kw", "KW6"), ("kw", "KW7"), ("kw", "KW9"), ("kw_virtual", "KW1"), ("kw_virtual", "KW2")]

ALL_KGEMM_KERNELS = ([f"kgemm_k<{f},{nw},{n}>" for f in (0, 1) for nw in ("8,8", "4,4", "4,2", "4,1") for n in ("false", "true")] +
                     [f"kwgrad_k<{nw},{s}>" for nw in ("8,8", "4,4", "4,2", "4,1") for s in (0, 1, 2)] +
                     [f"kpair_k<{f},{t}>" for f in (0, 1) for t in ("64,64", "32,128")])
UNREACHABLE = {}  # every instantiation has a case


def expected_kernels():
    """The names the GPU tests below assert, from the same tables and rules they use."""
    names = set()
    for n in FWD_CASES:
        names.add(expect(n, "fwd", forced=0))
    for n in DGRAD_CASES:
        names.update(expect(n, "dgrad", gr, forced=0) for gr in (1, 2))
    for n in VIRTUAL_CASES:
        names.add(expect(n, "fwd", nrm=True, forced=0))
    for n in KW_CASES:
        g = geo(n)
        names.update(kwname(kw_tiles(g), side) for side in (0, 1 if g.tr else 2))
    names.update(p for _, p in PAIRS.values() if " + " not in p)
    for what, n in KS8_RUNS:  # the child
        g = geo(n)
        if what in ("fwd", "stats", "virtual"):
            names.add(expect(n, "fwd", nrm=what == "virtual", forced=8))
        else:
            names.add(kwname(kw_tiles(g), 0 if what == "kw" else (1 if g.tr else 2), 8))
    return names


# ---- GPU plumbing ---------------------------------------------------------------------------------------------------------------------
def pin(lib):
    return lib.movae_bench_force_kgemm(1), lib.movae_bench_big_tile_min(0), lib.movae_bench_force_split(0)


@pytest.fixture
def kg(L):
    """Every shape the family can serve takes it; the dispatcher's own big-tile threshold; no pinned split factor.  All three
    settings are restored afterwards."""
    lib = L.load()
    kgemm, big, sp = pin(lib)
    lib.movae_bench_last_reduce()  # (reading clears what earlier tests left)
    try:
        yield lib
    finally:
        lib.movae_bench_force_split(sp)
        lib.movae_bench_big_tile_min(big)
        lib.movae_bench_force_kgemm(kgemm)


def judge(what, got, want, kind, kernel):
    """want: float64."""
    if kind == "int":
        want = want.float()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{kernel} {what}: {bad.shape[0]} of {got.numel()} elements differ from the exact result, first at "
                                 f"{bad[0].tolist()} (got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])}), last at {bad[-1].tolist()}")
        return
    e = bt.rel(got, want)
    print(f"[kgemm exact] {kernel} | {what}: rel-L2 {e:.2e}")
    assert e < 1e-5, (what, kernel, e)


def reduced(lib, want, what):
    got = bt.last_reduce(lib)
    assert got == want, f"{what}: reduced by {got!r}, expected {want!r}"


def check_fwd(L, lib, dev, name, kind, plain=False, nrm=None):
    g = geo(name)
    x, _, w, b = data(name, kind)
    kernel = expect(name, "fwd", nrm=nrm is not None)
    y = bt.run_fwd(L, lib, dev, g, x, w, None if plain else b, kernel, nrm=nrm, act=not plain)
    what = f"{name} forward{' (plain)' if plain else ''}{' (virtual x)' if nrm else ''}"
    want = bt.memo((what, kind), lambda: bt.ref_fwd(g, bt.virt(x, nrm), w, None if plain else b, None if plain else SLOPE))
    judge(what, y, want, kind, kernel)
    return y


def check_dgrad(L, lib, dev, name, kind, groups=1):
    g = geo(name)
    _, dy, w, _ = data(name, kind, groups)
    kernel = expect(name, "dgrad", groups)
    dx = bt.run_dgrad(L, lib, dev, g, dy, w, kernel, groups)
    what = f"{name} input gradient ({groups} groups)"
    judge(what, dx, bt.memo((what, kind), lambda: bt.ref_dgrad(g, dy, w)), kind, kernel)
    return dx


def class_tiles(t, g, form, groups=1):
    """t: [groups * n][H][W][C] in memory order -> [groups][classes][tiles][32][C]: the rows of every 32-row tile of every class (and
    cotangent group) in the order the kernel walks them, zero rows behind a ragged end."""
    s = g.s if form == 1 else 1
    N, H, W, Cc = t.shape
    t = t.reshape(groups, N // groups, H // s, s, W // s, s, Cc).permute(0, 3, 5, 1, 2, 4, 6).reshape(groups, s * s, -1, Cc)
    rows = t.shape[2]
    tiles = ceil_div(rows, 32)
    pad = torch.zeros(groups, s * s, tiles * 32 - rows, Cc, dtype=t.dtype)
    return torch.cat([t, pad], 2).reshape(groups, s * s, tiles, 32, Cc)


def partials_ok(what, got, terms, kind, exact):
    """got [parts][C] float32 partials; terms [parts][32][C] float64.  exact: integer terms, the sums must be equal."""
    want, mag = terms.sum(1), terms.abs().sum(1)
    if exact and kind == "int":
        assert torch.equal(got.double(), want), f"{what}: partials {(got.double() != want).any(1).nonzero().flatten().tolist()} differ from the exact sums"
        return
    err = (got.double() - want).abs()
    ok = err <= 34 * U * mag
    assert bool(ok.all()), f"{what}: partials {(~ok).any(1).nonzero().flatten().tolist()} out of bound, worst error {float(err.max()):.3e}"


def check_stats(L, lib, dev, name, kind):
    """A statistics request on a forward without activation: partial cls * tiles_c + T holds the column sum and sum of squares of the
    stored rows of tile T of class cls = ph * s + pw, bias included."""
    g = geo(name)
    x, _, w, b = data(name, kind)
    form = form_of(g, "fwd")[0]
    ncls = g.s * g.s if form == 1 else 1
    tiles_c = ceil_div(g.n * g.ho * g.wo // ncls, 32)
    parts = ncls * tiles_c
    st = bt.Out((parts * 2 * g.co,), dev)
    f = L.MovaeFuse()
    f.stats, f.stats_cap = st.ptr(), st.t.numel()
    kernel = expect(name, "fwd")
    y = bt.run_fwd(L, lib, dev, g, x, w, b, kernel, act=False, fuse=f)
    assert f.stats_parts == parts, (name, f.stats_parts, parts)
    judge(f"{name} forward (statistics)", y, bt.memo((f"{name} forward (bias)", kind), lambda: bt.ref_fwd(g, x, w, b)), kind, kernel)
    raw = st.get(f"{name} statistics").view(parts, 2, g.co)
    rows = class_tiles(y.double(), g, form).reshape(parts, 32, g.co)
    partials_ok(f"{name} statistics, sums", raw[:, 0], rows, kind, True)
    partials_ok(f"{name} statistics, sums of squares", raw[:, 1], rows * rows, kind, True)


def side_operands(name, groups, seed):
    """(y of the layer in front [n][hi][wi][ci], scale, shift, residual cotangent) for an input gradient's epilogue; no pre-activation
    sits where float32 and float64 could disagree about its sign."""
    g = geo(name)
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(g.n, g.hi, g.wi, g.ci, generator=gen)
    scale, shift = torch.rand(g.ci, generator=gen) + 0.5, torch.randn(g.ci, generator=gen) * 0.2
    near = (scale.double() * y.double() + shift.double()).abs() <= 1e-3  # (a million draws come closer to zero than 1e-6: moved by scale / 2)
    y = torch.where(near, y + 0.5, y)
    assert float((scale.double() * y.double() + shift.double()).abs().min()) > 1e-6
    res = torch.randint(-4, 5, (groups * g.n, g.hi, g.wi, g.ci), generator=gen).float()
    return y, scale, shift, res


def check_bnbwd(L, lib, dev, name, kind, groups):
    """The BatchNorm-backward sums of an input gradient: partial gi * ppg + cls * tpg + T against d = dx * act' formed in fp32 from the
    stored dx, summed in float64 over that tile's rows."""
    g = geo(name)
    _, dy, w, _ = data(name, kind, groups)
    form = form_of(g, "dgrad")[0]
    ncls = g.s * g.s if form == 1 else 1
    y, scale, shift, _ = side_operands(name, groups, 23)
    slope = 0.01
    rows_c = groups * g.n * g.hi * g.wi // ncls
    served = takes(g, "dgrad") and rows_c % groups == 0 and (rows_c // groups) % 32 == 0
    ppg = rows_c // groups // 32 * ncls
    yd, scd, shd = y.to(dev), scale.to(dev), shift.to(dev)
    part = bt.Out(((groups * ppg if served else 64) * 2 * g.ci,), dev)  # (exactly the room the served request needs)
    f = L.MovaeFuse()
    f.bn_y, f.bn_scale, f.bn_shift, f.bn_slope = yd.data_ptr(), scd.data_ptr(), shd.data_ptr(), slope
    f.bn_part, f.bn_cap = part.ptr(), part.t.numel()
    kernel = expect(name, "dgrad", groups) if served else TILED[(name, "dgrad")]
    dx = bt.run_dgrad(L, lib, dev, g, dy, w, kernel, groups, fuse=f)
    what = f"{name} input gradient ({groups} groups, BatchNorm-backward sums)"
    judge(what, dx, bt.memo((f"{name} input gradient ({groups} groups)", kind), lambda: bt.ref_dgrad(g, dy, w)), kind, kernel)
    if not served:
        return
    assert f.bn_ppg == ppg, (name, f.bn_ppg, ppg)
    z = scale * y + shift
    fac = torch.where(z > 0, 1.0, slope).float()
    d = dx.view(groups, g.n, g.hi, g.wi, g.ci) * fac  # (one float32 product, as the kernel forms it)
    dyy = d.double() * y.double()
    raw = part.get(f"{name} BatchNorm-backward partials")[:groups * ppg * 2 * g.ci].view(groups * ppg, 2, g.ci)
    partials_ok(what + ", sum d", raw[:, 0], class_tiles(d.double().reshape(-1, g.hi, g.wi, g.ci), g, form, groups).reshape(-1, 32, g.ci), kind, False)
    partials_ok(what + ", sum d * y", raw[:, 1], class_tiles(dyy.reshape(-1, g.hi, g.wi, g.ci), g, form, groups).reshape(-1, 32, g.ci), kind, False)


def check_actmul(L, lib, dev, name, kind, groups, act_y=True, res=True, done=1):
    """ActMul / residual epilogue of an input gradient: fused == plain * act'(y) + res with single roundings on both sides."""
    g = geo(name)
    _, dy, w, _ = data(name, kind, groups)
    y, _, _, r = side_operands(name, groups, 37)
    slope = 0.5  # (a power of two: the product is exact, so the equality holds whether or not the compiler contracts v * f + res into an fma)
    kernel = expect(name, "dgrad", groups)
    plain = bt.run_dgrad(L, lib, dev, g, dy, w, kernel, groups)
    yd, rd = y.to(dev), r.to(dev)
    f = L.MovaeFuse()
    if act_y:
        f.ep_act_y, f.ep_act, f.ep_slope = yd.data_ptr(), LRELU, slope
    if res:
        f.ep_res = rd.data_ptr()
    fused = bt.run_dgrad(L, lib, dev, g, dy, w, kernel, groups, fuse=f)
    assert f.ep_act_done == done, (name, f.ep_act_done)
    want = plain
    if done:
        if act_y:
            want = (want.view(groups, g.n, g.hi, g.wi, g.ci) * torch.where(y > 0, 1.0, slope).float()).view_as(plain)
        if res:
            want = want + r
    assert torch.equal(fused, want), f"{name} ({groups} groups): the fused epilogue differs at {(fused != want).nonzero()[0].tolist()}"
    judge(f"{name} input gradient ({groups} groups, before the epilogue)", plain,
          bt.memo((f"{name} input gradient ({groups} groups)", kind), lambda: bt.ref_dgrad(g, dy, w)), kind, kernel)


def draw_init(g, groups):
    gen = torch.Generator().manual_seed(5)
    return ([torch.randint(-5, 6, g.wshape, generator=gen).float() for _ in range(groups)],
            [torch.randint(-5, 6, (g.co,), generator=gen).float() for _ in range(groups)])


def judge_dw(what, g, kind, dws, dy, xv, groups, init, key, kernel):
    dyg = dy.view(groups, g.n, g.ho, g.wo, g.co)
    for i in range(groups):
        dw = bt.memo(key + (i,), lambda: bt.ref_wgrad(g, dyg[i], xv)[0])
        judge(f"{what} group {i}", dws[i], dw + (init[0][i].double() if init else 0.0), kind, kernel)


def check_kw(L, lib, dev, name, kind, groups=1, acc=False, split=1, nrm=None, off=""):
    """kwgrad_k: a conv's weight gradient without a bias gradient, a transposed conv's.  split: the pinned factor; the slab count
    ceil(n / (ceil(ceil(n / split) / 8) * 8)) is asserted with a scratch of the test's own, and the reduce by name."""
    g = geo(name)
    x, dy, _, _ = data(name, kind, groups)
    kernel = kwname(kw_tiles(g, groups), 0 if nrm is None else (1 if g.tr else 2), FORCED_KS)
    slabs = kw_slabs(g.n, split)
    init = draw_init(g, groups) if acc else None
    ws = bt.Scratch(dev)
    lib.movae_bench_force_split(split)
    try:
        dws, _ = bt.run_wgrad(L, lib, dev, g, dy, x, kernel, groups, nrm=nrm, init=init, bias=False, ws=ws, off=off)
    finally:
        lib.movae_bench_force_split(0)
    what = f"{name} weight gradient ({groups} groups{', accumulate' if acc else ''}{', virtual x' if nrm else ''}{', split %d' % split if split > 1 else ''}{', off ' + off if off else ''})"
    reduced(lib, " + ".join(["splitk_reduce_flat"] * groups) if slabs > 1 else "", what)
    assert ws.slabs(g.co * g.k * g.k * g.ci) == (slabs * groups if slabs > 1 else 0), what
    judge_dw(what, g, kind, dws, dy, bt.virt(x, nrm), groups, init, (name, kind, groups, nrm is not None), kernel)
    return dws


def check_pair(L, lib, dev, name, kind, groups, acc):
    """The paired entry point: dx must be the stand-alone input gradient's bits, dW the stand-alone weight gradient's (the tiled
    kernel with the family switched off; P6: kwgrad_k under this pin), and both must meet float64."""
    g = geo(name)
    x, dy, w, _ = data(name, kind, groups)
    alone, paired = PAIRS[name]
    init = draw_init(g, groups) if acc else None
    dx, dws, dbs = bt.run_pair(L, lib, dev, g, dy, w, x, paired, groups, init=init)
    dk = expect(name, "dgrad", groups)
    assert dk.endswith(",4,4,false>") and (" + " not in paired or paired.startswith(dk + " + "))
    dx1 = bt.run_dgrad(L, lib, dev, g, dy, w, dk, groups)
    what = f"{name} pair ({groups} groups{', accumulate' if acc else ''})"
    assert torch.equal(dx, dx1), f"{what}: dx differs from the stand-alone input gradient"
    judge(what + " dx", dx, bt.memo((f"{name} input gradient ({groups} groups)", kind), lambda: bt.ref_dgrad(g, dy, w)), kind, paired)
    if alone.startswith("kwgrad_k"):
        dws1, _ = bt.run_wgrad(L, lib, dev, g, dy, x, alone, groups, init=init, bias=False)
    else:
        prev = lib.movae_bench_force_kgemm(-1)
        try:
            dws1, dbs1 = bt.run_wgrad(L, lib, dev, g, dy, x, alone, groups, init=init)
        finally:
            lib.movae_bench_force_kgemm(prev)
        for i in range(groups):
            assert torch.equal(dbs[i], dbs1[i]), f"{what}: bias gradient {i} differs from the stand-alone call's"
    for i in range(groups):
        assert torch.equal(dws[i], dws1[i]), f"{what}: dW {i} differs from the stand-alone weight gradient"
    judge_dw(what + " dW", g, kind, dws, dy, x.double(), groups, init, (name, kind, groups, False), paired)
    dyg = dy.view(groups, g.n, g.ho, g.wo, g.co)
    for i in range(groups):
        judge(f"{what} bias gradient {i}", dbs[i], dyg[i].double().reshape(-1, g.co).sum(0) + (init[1][i].double() if init else 0.0), kind, paired)


# ---- FWD and BWD gather forms -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("plain", [False, True], ids=["bias_act", "plain"])
@pytest.mark.parametrize("name", FWD_CASES)
def test_forward(L, kg, gpu_device, name, plain, kind):
    """KB4: the parity classes without a tap hold act(bias), or zero in the plain run.  KB7 (9 x 7 output) is refused: the tiled
    kernel, and the right result.  KN+ without a virtual operand is the family's."""
    y = check_fwd(L, kg, gpu_device, name, kind, plain)
    if name == "KB4":
        b = data(name, kind)[3]
        rest = y[:, 1::2, :, :], y[:, 0::2, 1::2, :]  # every class but (0, 0)
        want = torch.zeros_like(b) if plain else bt.lrelu(b.double(), SLOPE).float()
        assert all(bool((r == want).all()) for r in rest)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", DGRAD_CASES)
def test_input_gradient(L, kg, gpu_device, name, groups, kind):
    check_dgrad(L, kg, gpu_device, name, kind, groups)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", VIRTUAL_CASES)
def test_virtual_operand(L, kg, gpu_device, name, kind):
    """BatchNorm + LeakyReLU applied to x on load, the per-channel map staged in LDS: at exactly NORM_MAX_C channels (KN), refused
    above (KN+: the tiled kernel), in the BWD form (KB1, KB6) and at KS 2 and 1.  The shift is non-zero and padding stays zero: a
    kernel that transforms padding gives a wrong result."""
    check_fwd(L, kg, gpu_device, name, kind, nrm=bt.norm_params(geo(name).ci, kind, 77))


# ---- side products --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", STATS_CASES)
def test_statistics_partial_by_partial(L, kg, gpu_device, name, kind):
    check_stats(L, kg, gpu_device, name, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", BN_CASES)
def test_batchnorm_backward_sums_partial_by_partial(L, kg, gpu_device, name, groups, kind):
    if name == "SFL2" and groups == 2:
        assert ks_of(tiles_of(geo(name), "dgrad", 2)) == 1  # (2050 tiles: the epilogue at KS 1)
    check_bnbwd(L, kg, gpu_device, name, kind, groups)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["SB5", "SF5"])
def test_batchnorm_backward_refused_without_whole_tiles_per_group(L, kg, gpu_device, name, kind):
    """n = 5: rows per group and class are no multiple of 32 -- plan_side refuses, the tiled kernel runs, dx is right."""
    check_bnbwd(L, kg, gpu_device, name, kind, 1)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["SB4", "SF4", "SB8", "SBL2", "SFL2"])
def test_actmul_and_residual_epilogue(L, kg, gpu_device, name, kind):
    check_actmul(L, kg, gpu_device, name, kind, 2)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["SB5", "SF5", "KF1"])
def test_residual_alone_at_a_ragged_shape(L, kg, gpu_device, name, kind):
    check_actmul(L, kg, gpu_device, name, kind, 1, act_y=False)


@gpu
@pytest.mark.parametrize("name", ["SB5", "SF5"])
def test_grouped_activation_derivative_refused_without_whole_tiles(L, kg, gpu_device, name):
    """ep_act_y over two groups at n = 5: not applied (ep_act_done == 0), the kernel is still the family's and dx the plain gradient."""
    check_actmul(L, kg, gpu_device, name, "int", 2, res=False, done=0)


# ---- the paired entry points --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", list(PAIRS))
def test_paired_entry_points(L, kg, gpu_device, name, groups, acc, kind):
    check_pair(L, kg, gpu_device, name, kind, groups, acc)


# ---- kwgrad_k -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", KW_CASES)
def test_kwgrad(L, kg, gpu_device, name, kind):
    dws = check_kw(L, kg, gpu_device, name, kind)
    if name == "KW3":  # a 1 x 1 small side meets tap (kh, kw) at pixel (kh - 1, kw - 1) only: row 0 and column 0 of the taps are zero tiles
        assert bool((dws[0][:, 0] == 0).all()) and bool((dws[0][:, :, 0] == 0).all()) and bool((dws[0][:, 1:, 1:] != 0).any())


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("groups", [2, 8])
@pytest.mark.parametrize("name", ["KW1", "KW2"])
def test_kwgrad_cotangent_groups(L, kg, gpu_device, name, groups, kind):
    check_kw(L, kg, gpu_device, name, kind, groups)


@gpu
def test_kwgrad_nine_groups_are_refused_by_the_entry_point(L, kg, gpu_device):
    import test_hip_thin as th

    dev, g = gpu_device, geo("KW1")
    x, dy, _, _ = data("KW1", "int")
    xd, dyd = x.to(dev), dy.repeat(9, 1, 1, 1).to(dev)
    dws = [bt.Out(g.wshape, dev) for _ in range(9)]
    dwp = (C.c_void_p * 9)(*[o.ptr() for o in dws])
    ws, st = L.workspace(dev), torch.cuda.current_stream().cuda_stream
    th.refused(L, kg, lambda: L.call("movae_conv2d_wgrad_grouped", 9, dyd.data_ptr(), xd.data_ptr(), dwp, None, *g.args(), 0, ws.data_ptr(),
                                     ws.numel(), st), dws, -1)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("name", ["KW1", "KW3"])
def test_kwgrad_split_and_accumulate(L, kg, gpu_device, name, acc, split, kind):
    """KW1: 20 images in slabs of 16 + 4 (split 2) and 8 + 8 + 4 (split 3).  KW3 (9 images: 8 + 1 under either split): a tap that
    never meets the image is zero without `accumulate`, the old value with it, and zeros in a slab under a split."""
    g = geo(name)
    assert [kw_slabs(g.n, s) for s in (1, 2, 3)] == ([1, 2, 3] if name == "KW1" else [1, 2, 2])
    dws = check_kw(L, kg, gpu_device, name, kind, groups=2, acc=acc, split=split)
    if name == "KW3":
        init = draw_init(g, 2)
        for i in range(2):
            want = init[0][i][:, 0] if acc else torch.zeros_like(dws[i][:, 0])
            assert torch.equal(dws[i][:, 0], want)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", KW_CASES)
def test_kwgrad_virtual_operand(L, kg, gpu_device, name, kind):
    """On the small side (transposed: NSIDE 1) and on the big side (conv: NSIDE 2, pad 1, non-zero shift: padding must stay zero)."""
    check_kw(L, kg, gpu_device, name, kind, nrm=bt.norm_params(geo(name).ci, kind, 77))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("name", ["KW1", "KW2", "KW3"])
def test_kwgrad_into_a_misaligned_gradient(L, kg, gpu_device, name, acc, kind):
    """dW one float past a 16-byte boundary: the scalar store loop (KW3: also the zero tiles')."""
    check_kw(L, kg, gpu_device, name, kind, acc=acc, off="d")


# ---- KS = 8 and the compute dtype -------------------------------------------------------------------------------------------------
def run_ks8(L, lib, dev):
    for what, name in KS8_RUNS:
        g = geo(name)
        for kind in KINDS:
            if what == "fwd":
                check_fwd(L, lib, dev, name, kind)
                check_fwd(L, lib, dev, name, kind, plain=True)
            elif what == "virtual":
                check_fwd(L, lib, dev, name, kind, nrm=bt.norm_params(g.ci, kind, 77))
            elif what == "stats":
                check_stats(L, lib, dev, name, kind)
            elif what == "kw":
                check_kw(L, lib, dev, name, kind)
            else:
                check_kw(L, lib, dev, name, kind, nrm=bt.norm_params(g.ci, kind, 77))
        print(f"ks8 {what} {name}: ok", flush=True)


@gpu
def test_eight_waves_per_tile_in_a_fresh_process(gpu_device):
    """MOVAE_KGEMM_KS=8 is read once per process: one child runs KF1, KF4 (slices 6 and 7 empty), KF9, KB1, KB4, the statistics and
    kwgrad_k checks of this file and asserts names <..,8,8,..>."""
    assert slices(48, 8) == [1, 1, 1, 1, 1, 1, 0, 0]
    env = dict(os.environ, MOVAE_KGEMM_KS="8", MOVAE_NO_REBUILD="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ks8"], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == len(KS8_RUNS)


@gpu
def test_bf16_mode_runs_the_same_kernels_to_the_same_bits(L, kg, gpu_device):
    """The family has no bf16 form."""
    def run():
        g = geo("KF1")
        x, dy, w, _ = data("KF1", "normal")
        return (check_fwd(L, kg, gpu_device, "KF1", "normal"), check_fwd(L, kg, gpu_device, "KB1", "normal"),
                *(lambda r: (r[0], r[1][0], r[2][0]))(bt.run_pair(L, kg, gpu_device, g, dy, w, x, PAIRS["KF1"][1])))

    f32 = run()
    with bt.mode(L, "bf16"):
        b16 = run()
    for a, b, what in zip(f32, b16, ("KF1 y", "KB1 y", "pair dx", "pair dW", "pair db")):
        assert torch.equal(a, b), f"{what}: differs between the compute dtypes"


# ---- CPU checks of this file's own tables and machinery -----------------------------------------------------------------------------
def test_every_kernel_is_the_expected_kernel_of_a_case_or_unreachable():
    assert len(ALL_KGEMM_KERNELS) == len(set(ALL_KGEMM_KERNELS)) == 32
    assert sum(n.startswith("kgemm_k") for n in ALL_KGEMM_KERNELS) == 16 and sum(n.startswith("kwgrad_k") for n in ALL_KGEMM_KERNELS) == 12
    expected = {n for n in expected_kernels() if n.startswith("k")}
    assert expected | set(UNREACHABLE) == set(ALL_KGEMM_KERNELS), (expected | set(UNREACHABLE)) ^ set(ALL_KGEMM_KERNELS)
    assert not expected & set(UNREACHABLE)
    # the refusals launch what TILED says, and nothing else of the tables is refused
    refused = {(n, op) for n in FWD_CASES for op in ("fwd",) if not takes(geo(n), op)} | {(n, "dgrad") for n in DGRAD_CASES if not takes(geo(n), "dgrad")}
    assert refused == {("KB7", "fwd")} and not takes(geo("KN+"), "fwd", True) and takes(geo("KN+"), "fwd") and takes(geo("KN"), "fwd", True)


@pytest.mark.parametrize("name", ["KB4", "KB6", "KB2", "KF7", "KW3"])
def test_reference_agrees_with_torch(name):
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
    assert bt.close(bt.ref_wgrad(g, dy, x)[0], dw.permute(0, 2, 3, 1))
    if name == "KB4":  # three of four classes see no tap: exactly the bias
        yy = bt.ref_fwd(g, x, w, b)
        assert bool((yy[:, 1::2] == b.double()).all()) and bool((yy[:, ::2, 1::2] == b.double()).all()) and not bool((yy[:, ::2, ::2] == b.double()).all())


def test_integer_data_is_exact_in_fp32():
    """sum |a| |b| bounds every partial sum of every summation order.  The virtual operand is at most 8 in magnitude (half-integers),
    weights 2, cotangents 3, bias 8, an accumulated gradient starts within 5."""
    two24 = 2.0 ** 24
    for name in CASES:
        g = geo(name)
        k_fwd = g.k * g.k * (g.co if g.tr else g.ci)  # (an upper bound in the BWD form: all taps of all classes)
        k_dgrad = g.k * g.k * (g.ci if g.tr else g.co)
        pixels = g.n * max(g.hi * g.wi, g.ho * g.wo)  # (cotangent groups are separate sums)
        assert 8 * 2 * max(k_fwd, k_dgrad) + 8 < two24 and 8 * 3 * pixels + 5 < two24, name
    for name in ("KF1", "KB1", "KW1", "KW2"):
        xv = bt.virt(data(name, "int")[0], bt.norm_params(geo(name).ci, "int", 77))
        assert torch.equal(xv * 2, (xv * 2).round()) and float(xv.abs().max()) <= 8
        xn = bt.virt(data(name, "normal")[0], bt.norm_params(geo(name).ci, "normal", 77))
        assert torch.equal(xn.float().double(), xn)  # the normal-data transform is exact in fp32
    worst = 0.0
    for name in STATS_CASES:  # the statistics: every 32-row tile's sum of squares
        g = geo(name)
        x, _, w, b = data(name, "int")
        y = bt.ref_fwd(g, x, w, b)
        t = class_tiles(y, g, form_of(g, "fwd")[0])
        worst = max(worst, float((t * t).sum(3).max()))
    print(f"largest sum of squares of a tile: {worst:.0f}")
    assert worst < two24


def test_class_tiles_walks_rows_as_the_kernel_does():
    """Row m of class (ph, pw) is pixel (img, hc * s + ph, wc * s + pw) with m = (img * Hc + hc) * Wc + wc."""
    g = geo("KB3")  # 3 images of 10 x 6: classes of 3 * 5 * 3 = 45 rows
    t = torch.arange(3 * 10 * 6, dtype=torch.float64).view(3, 10, 6, 1)
    ct = class_tiles(t, g, 1)
    assert tuple(ct.shape) == (1, 4, 2, 32, 1)
    for cls, m in ((0, 0), (1, 7), (2, 31), (3, 44)):
        img, rem = divmod(m, 15)
        hc, wc = divmod(rem, 3)
        assert float(ct[0, cls, m // 32, m % 32, 0]) == (img * 10 + hc * 2 + cls // 2) * 6 + wc * 2 + cls % 2
    assert bool((ct[0, :, 1, 13:] == 0).all())
    two = class_tiles(torch.arange(128.0).view(8, 4, 4, 1).double(), geo("SF4"), 0, 2)  # FWD form, two groups of 4 images
    assert tuple(two.shape) == (2, 1, 2, 32, 1) and float(two[1, 0, 1, 31, 0]) == 127.0 and float(two[1, 0, 0, 0, 0]) == 64.0


def test_derived_counts():
    """The figures of the case table, from the transcribed rules."""
    def K(name):
        return window_k(geo(name))

    def fwd_tiles(name):
        return tiles_of(geo(name), "fwd")

    assert [ks_of(t) for t in (1, 1024, 1025, 2048, 2049)] == [4, 4, 2, 2, 1]
    assert K("KF1") == 576 and slices(576, 4) == [18] * 4 and trips(18) == (1, 3) and fwd_tiles("KF1") == 2 * 3
    assert K("KF2") == 144 and slices(144, 4) == [5, 5, 5, 3] and trips(5) == (0, 3) and fwd_tiles("KF2") == 2 * 2
    assert K("KF4") == 48 and slices(48, 4) == [2, 2, 2, 0]
    assert K("KF5") == 384 and slices(384, 4) == [12] * 4 and trips(12) == (1, 0) and fwd_tiles("KF5") == 1 and 24 % 16 != 0
    assert K("KF6") == 72 and slices(72, 4) == [3, 3, 3, 0]
    assert K("KF7") == 128 and 9 * 32 == 288 and K("KF8") == 32
    assert K("KF9") == 1152 and slices(1152, 4) == [36] * 4 and trips(36) == (3, 0)
    assert K("KN") == 1024 == NORM_MAX_C and trips(slices(1024, 4)[0]) == (2, 4)
    assert fwd_tiles("KL2") == 1025 and 5 * 79 * 83 == 32785 and ks_of(1025) == 2 and slices(72, 2) == [5, 4] and 1025 % 2 == 1
    assert fwd_tiles("KL1") == 2050 and ks_of(2050) == 1 and ceil_div(1025, 4) * 4 - 1025 == 3
    assert fwd_tiles("KBL2") == 4 * 259 and ks_of(4 * 259) == 2 and 259 % 2 == 1 and fwd_tiles("KBL1") == 8 * 259 and ks_of(8 * 259) == 1
    assert class_windows(geo("KB1")) == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert class_windows(geo("KB2")) == [(1, 1)] * 4 and geo("KB2").n * 1 * 1 == 6
    assert class_windows(geo("KB3")) == [(2, 2)] * 4 and 3 * 5 * 3 == 45
    assert class_windows(geo("KB3b")) == [(1, 1)] * 4
    assert class_windows(geo("KB4")) == [(1, 1), (0, 0), (0, 0), (0, 0)]
    assert class_windows(geo("KB6")) == [(1, 1), (1, 2), (1, 1), (1, 2)]
    assert (geo("KB7").ho, geo("KB7").wo) == (9, 7)
    assert class_windows(geo("KF1"), "dgrad") == [(1, 1), (1, 2), (2, 1), (2, 2)] and class_windows(geo("KF3"), "dgrad") == [(3, 3)]
    # side products: whole tiles per group and class; the KS 2 shapes with an odd tile count per class
    for name, rows in (("SB4", 32), ("SB8", 128), ("SF4", 128), ("SF8", 512)):
        g = geo(name)
        ncls = 1 if g.tr else 4
        assert g.n * g.hi * g.wi // ncls == rows
    assert tiles_of(geo("SBL2"), "dgrad") == 4 * 259 and tiles_of(geo("SFL2"), "dgrad") == 1025 and tiles_of(geo("SFL2"), "dgrad", 2) == 2050
    assert tiles_of(geo("SBL2"), "dgrad", 2) == 8 * 259
    # kwgrad_k: tiles, image slices, slabs
    assert kw_tiles(geo("KW1")) == 2 * 9 and [kw_slabs(20, s) for s in (2, 3)] == [2, 3] and slices(24, 4) == [1, 1, 1, 0]
    assert kw_tiles(geo("KW4")) == 1026 == kw_tiles(geo("KW4T")) and kw_tiles(geo("KW5")) == 2052 == kw_tiles(geo("KW5T"))
    assert kw_tiles(geo("KW1"), 8) <= 1024
    # kwgrad_k: image slices per wave (groups of 8 images), position windows, chunks and trips round the ring of eight
    assert slices(8 * ceil_div(40, 8), 4) == [2, 2, 1, 0] and slices(8 * ceil_div(57, 8), 4) == [2, 2, 2, 2] and 57 % 8 == 1
    assert slices(8 * ceil_div(17, 8), 2) == [2, 1] and kw_tiles(geo("KW8")) == 1026 and ks_of(1026) == 2
    assert slices(8 * ceil_div(72, 8), 4) == [3, 3, 3, 0] and slices(8 * ceil_div(72, 8), 8) == [2, 2, 2, 2, 1, 0, 0, 0]
    assert max(kw_tiles(geo(n)) for n in ("KW6", "KW7", "KW9")) <= 1024
    assert [kw_window(geo("KW1"), k, k) for k in range(3)] == [(1, 1), (2, 2), (2, 2)] and kw_chunks(geo("KW1"), 1, 1, 4)[0] == (4, 0, 4)
    assert kw_window(geo("KW2"), 1, 1) == (3, 3) and kw_chunks(geo("KW2"), 1, 1, 4) == [(9, 1, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    assert [kw_window(geo("KW3"), k, k) for k in range(3)] == [(0, 0), (1, 1), (1, 1)]
    assert kw_window(geo("KW6"), 1, 1) == (4, 5) and kw_chunks(geo("KW6"), 1, 1, 4) == [(40, 5, 0), (40, 5, 0), (20, 2, 4), (0, 0, 0)]
    assert kw_window(geo("KW6"), 0, 0) == (3, 4) and kw_chunks(geo("KW6"), 0, 0, 4)[0] == (24, 3, 0)
    assert kw_window(geo("KW7"), 1, 1) == (3, 2) and kw_chunks(geo("KW7"), 1, 1, 4) == [(12, 1, 4)] * 4
    assert kw_window(geo("KW8"), 1, 1) == (2, 2) and kw_chunks(geo("KW8"), 1, 1, 2) == [(8, 1, 0), (4, 0, 4)]
    assert kw_window(geo("KW9"), 1, 1) == (2, 3) and kw_chunks(geo("KW9"), 1, 1, 4)[:3] == [(18, 2, 2)] * 3
    assert kw_chunks(geo("KW9"), 1, 1, 8) == [(12, 1, 4)] * 4 + [(6, 0, 6)] + [(0, 0, 0)] * 3
    assert kw_chunks(geo("KW1"), 1, 1, 4, split=3) == [(4, 0, 4), (0, 0, 0), (0, 0, 0), (0, 0, 0)]  # (8 images per slab)
    for name, (alone, paired) in PAIRS.items():
        g = geo(name)
        assert tiles_of(g, "dgrad", 2) <= 1024 and takes(g, "dgrad")
        cs, cb = (g.ci, g.co) if g.tr else (g.co, g.ci)
        N = g.k * g.k * cb
        tile = "128,32" if N <= 32 else ("32,128" if cs <= 32 and N >= 128 else "64,64")
        if name == "P6":
            assert g.tr and g.co % 32 == 0
        else:
            assert alone == f"igemm2_wgrad<{tile}>" and (not g.tr or g.co % 32 != 0)
            assert paired == (f"kpair_k<{0 if g.tr else 1},{tile}>" if tile != "128,32" else f"kgemm_k<1,4,4,false> + {alone}")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--ks8"] and os.environ.get("MOVAE_KGEMM_KS") == "8"
    FORCED_KS = 8
    import movae_amd
    import movae_amd._lib as lib_mod

    movae_amd.load_library()
    handle = lib_mod.load()
    pin(handle)
    run_ks8(lib_mod, handle, torch.device("cuda:0"))
    print("ks8: all ok")
