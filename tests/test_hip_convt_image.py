"""The whole-image-row forward kernel of the 3x3 stride-2 transposed conv with 32 input and 32 output channels
(csrc/convt_img.h: igemm2_bwd_img<32>), through movae_convT2d_fwd / movae_convT2d_fwd_f and with the machinery of
test_hip_big_tile.py (float64 tap-loop reference, outputs between guard zones that start as NaN, the asserted name of the kernel
that ran).  The dispatcher is pinned as by that file's `tiled`: the block-internal split-K family (csrc/kgemm.h) comes first in
the dispatch order and would take shapes this small.

A group is 32 input pixels, a block four groups = the 128 rows of one of the tiled kernel's row blocks.  Cases (n, hi, wi, ci):
  I1 (3, 8, 8, 32)    6 groups: a ragged second block        I2 (2, 16, 16, 32)  16 groups: two rows per group, four blocks
  I5 (2, 4, 8, 32)    a non-square image, one group each
  I3 (5, 8, 8, 64), I4 (1, 16, 16, 64), I6 (3, 4, 8, 64): 64 input channels KEEP igemm2_bwd<128,32> -- a 64-channel form of the
  kernel was faster per call (11.5 against 19.5 us at batch 256) but needs two waves per group and so two groups per block to fill
  the machine, and half a row block cannot reproduce the tiled kernel's statistics partials bit for bit (below); the cases stay,
  with the tiled kernel's name, and every check below runs on them too.
Per case: integer data (x in -3..3, w in -2..2, bias in -8..8, LeakyReLU slope 0.5) must EQUAL float64 with bias and activation,
with bias alone and without either; the same under a fused input transform with integer scale and non-zero integer shift (a
transform applied to padding shows); seeded normal data stays below rel-L2 1e-5; the statistics partials are the column sums of
the stored y to rows-per-partial * 2^-24 * sum |y| (test_hip_igemm_epilogue.py's bound, 128 rows per partial), nothing is written
behind them, and a second call gives the same bits.

Same bits as the tiled kernel (a training step amplifies a last-bit difference in these layers to the third digit of the loss
within twenty steps, so the new kernel reproduces the old one's summation orders): the plain result EQUALS that of
movae_conv2d_dgrad on the mirrored geometry -- the same BWD-form problem on the same weight memory, which runs
igemm2_bwd<128,32> -- and every statistics partial sum EQUALS the tiled kernel's order of float32 additions replayed on the CPU
from the stored y: slot class * blocks + block, q[i] = ((y[i] + y[32 + i]) + y[64 + i]) + y[96 + i] over the block's rows of
the class, then q[0] + ... + q[31] from zero.  The 64-channel cases check that replay against the tiled kernel itself.

Neighbours just outside the gate keep the kernel they had and stay right.  One of them is not the tiled kernel: with x one float
off its 16-byte boundary the dispatcher has always taken the generic igemm_bwd<128,32,false> (the tiled kernels need aligned
operands too; test_hip_mid_tile.py OFF4), and that is the name asserted here.  The input-gradient entry points at the shape
16 x 16 x 32 <- 8 x 8 x 64 keep igemm2_bwd<128,32> and igemm2_pair<1,128,32,64,64>: the new kernel is a forward kernel only."""
import ctypes as C

import pytest
import torch

import test_hip_big_tile as bt

gpu = pytest.mark.gpu
L = bt.L  # (the module-scoped library fixture)
SLOPE = bt.SLOPE
U = 2.0 ** -24

# transposed conv: (n, hi, wi, ci, co, k, s, p, output_padding)
CASES = {
    "I1": (3, 8, 8, 32, 32, 3, 2, 1, 1),
    "I2": (2, 16, 16, 32, 32, 3, 2, 1, 1),
    "I3": (5, 8, 8, 64, 32, 3, 2, 1, 1),
    "I4": (1, 16, 16, 64, 32, 3, 2, 1, 1),
    "I5": (2, 4, 8, 32, 32, 3, 2, 1, 1),
    "I6": (3, 4, 8, 64, 32, 3, 2, 1, 1),
    # just outside the gate
    "N16": (2, 8, 8, 32, 16, 3, 2, 1, 1),    # co = 16
    "NK4": (2, 8, 8, 32, 32, 4, 2, 1, 0),    # 4 x 4 taps (ho == 2 * hi all the same)
    "NOP": (2, 8, 8, 32, 32, 3, 2, 1, 0),    # ho == 2 * hi - 1
    "NPX": (4, 4, 4, 32, 32, 3, 2, 1, 1),    # hi * wi = 16
    # the gate's shape as an input gradient: conv 16 x 16 x 32 -> 8 x 8 x 64
    "D": (64, 16, 16, 32, 64, 3, 2, 1),
}
IMG = ["I1", "I2", "I3", "I4", "I5", "I6"]
TILED = "igemm2_bwd<128,32>"


def geo(name):
    return bt.Geo(name, CASES[name])


def kernel_of(g):
    return "igemm2_bwd_img<32>" if g.ci == 32 else TILED


def blocks_of(g):
    """Row blocks of 128 pixels per output-parity class: one statistics partial pair per (class, block), in both kernels."""
    return -(-(g.n * g.hi * g.wi) // 128)


def mirrored(g):
    """The conv whose input gradient is the same BWD-form problem: dy = x, dx = y, the weight memory as it is."""
    return bt.Geo(g.name + " mirrored", (g.n, g.ho, g.wo, g.co, g.ci, g.k, g.s, g.p))


def replay_partial_sums(y, blocks):
    """[4 * blocks][32]: the tiled kernel's float32 additions, in its order, on the stored y [n][ho][wo][32]."""
    out = torch.zeros(4 * blocks, 32)
    for c in range(4):
        rows = y[:, c // 2::2, c % 2::2, :].reshape(-1, 32)
        for b in range(blocks):
            blk = rows[b * 128:(b + 1) * 128]
            q = torch.zeros(32, 32)
            for u in range(blk.shape[0] // 32):
                q = q + blk[32 * u:32 * u + 32]
            c1 = torch.zeros(32)
            for i in range(32):
                c1 = c1 + q[i]
            out[c * blocks + b] = c1
    return out


_DATA = {}


def data(name, kind, groups=1):
    key = (name, kind, groups)
    if key not in _DATA:
        g = geo(name)
        gen = torch.Generator().manual_seed(7000 + sum(map(ord, name)))
        xs, dys = (g.n, g.hi, g.wi, g.ci), (groups * g.n, g.ho, g.wo, g.co)
        if kind == "int":
            x, dy = torch.randint(-3, 4, xs, generator=gen).float(), torch.randint(-3, 4, dys, generator=gen).float()
            w, b = torch.randint(-2, 3, g.wshape, generator=gen).float(), torch.randint(-8, 9, (g.co,), generator=gen).float()
        else:
            x, dy = torch.randn(xs, generator=gen), torch.randn(dys, generator=gen)
            w, b = torch.randn(g.wshape, generator=gen) * float(g.ci * g.k * g.k) ** -0.5, torch.randn(g.co, generator=gen) * 0.1
        _DATA[key] = (x, dy, w, b)
    return _DATA[key]


def int_transform(c):
    """Integer scale, NON-ZERO integer shift, slope 0.5: the transformed operand is a half-integer of magnitude <= 8."""
    gen = torch.Generator().manual_seed(91)
    scale = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (c,), generator=gen)]
    shift = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (c,), generator=gen)]
    return scale, shift, 0.5


@pytest.fixture
def tiled(L):
    with bt.pinned(L, 0, 1) as lib:
        yield lib


def check(L, lib, dev, name, kind, expect, bias=True, act=True, nrm=None, off=""):
    g = geo(name)
    x, _, w, b = data(name, kind)
    y = bt.run_fwd(L, lib, dev, g, x, w, b if bias else None, expect, nrm=nrm, act=act, off=off)
    what = f"convT image {name} forward{'' if bias else ' no bias'}{' act' if act else ''}{' (virtual x)' if nrm else ''}"
    bt.judge(what, y, lambda xx, ww: bt.ref_fwd(g, xx, ww, b if bias else None, SLOPE if act else None), (bt.virt(x, nrm), w), "f32", kind)
    return y


@gpu
@pytest.mark.parametrize("variant", ["bias_act", "bias", "plain"])
@pytest.mark.parametrize("name", IMG)
def test_integer_data_is_exact(L, tiled, gpu_device, name, variant):
    check(L, tiled, gpu_device, name, "int", kernel_of(geo(name)), bias=variant != "plain", act=variant == "bias_act")


@gpu
@pytest.mark.parametrize("name", IMG)
def test_integer_data_with_a_fused_input_transform_is_exact(L, tiled, gpu_device, name):
    g = geo(name)
    nrm = int_transform(g.ci)
    assert bool((nrm[1] != 0).all())
    check(L, tiled, gpu_device, name, "int", kernel_of(g), nrm=nrm)


@gpu
@pytest.mark.parametrize("name", IMG)
def test_normal_data(L, tiled, gpu_device, name):
    check(L, tiled, gpu_device, name, "normal", kernel_of(geo(name)))


@gpu
@pytest.mark.parametrize("name", IMG)
def test_statistics_and_reproducibility(L, tiled, gpu_device, name):
    g = geo(name)
    x, _, w, b = data(name, "normal")
    blocks, rows = blocks_of(g), 128
    parts = 4 * blocks
    cap = (parts + 3) * 2 * g.co

    def run():
        stats = torch.full((cap + 2 * bt.GUARD,), float("nan"), device=gpu_device)
        f = L.MovaeFuse()
        f.stats, f.stats_cap = stats[bt.GUARD:].data_ptr(), cap
        y = bt.run_fwd(L, tiled, gpu_device, g, x, w, b, kernel_of(g), act=False, fuse=f)
        torch.cuda.synchronize()
        assert f.stats_parts == parts
        used = f.stats_parts * 2 * g.co
        s = stats.cpu()
        assert bool(torch.isnan(s[:bt.GUARD]).all()) and bool(torch.isnan(s[bt.GUARD + used:]).all()), "a store outside the partials"
        part = s[bt.GUARD:bt.GUARD + used]
        assert bool(torch.isfinite(part).all())
        return y, part

    y1, p1 = run()
    y2, p2 = run()
    assert torch.equal(y1, y2) and torch.equal(p1, p2)
    assert torch.equal(p1.view(parts, 2, g.co)[:, 0], replay_partial_sums(y1, blocks)), "a partial sum differs from the tiled kernel's order"
    got = p1.view(parts, 2, g.co).double().sum(0)
    yd = y1.double().view(-1, g.co)
    for i, (want, mag, what) in enumerate(((yd.sum(0), yd.abs().sum(0), "sum y"), ((yd * yd).sum(0), (yd * yd).sum(0), "sum y^2"))):
        err, bound = (got[i] - want).abs(), rows * U * mag
        print(f"[convT image] {name} {what}: worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), f"{name} {what}: worst error {float(err.max()):.3e}, bound there {float(bound[err.argmax()]):.3e}"
    # the y of the statistics run is the y of the plain entry point
    assert torch.equal(y1, bt.run_fwd(L, tiled, gpu_device, g, x, w, b, kernel_of(g), act=False))


@gpu
@pytest.mark.parametrize("name", ["I1", "I2", "I5"])
def test_same_bits_as_the_tiled_kernel(L, tiled, gpu_device, name):
    g = geo(name)
    x, _, w, _ = data(name, "normal")
    y = bt.run_fwd(L, tiled, gpu_device, g, x, w, None, kernel_of(g), act=False)
    assert torch.equal(y, bt.run_dgrad(L, tiled, gpu_device, mirrored(g), x, w, TILED))


@gpu
def test_statistics_that_do_not_fit_are_not_written(L, tiled, gpu_device):
    g = geo("I1")
    x, _, w, b = data("I1", "normal")
    parts = 4 * blocks_of(g)
    stats = torch.full((parts * 2 * g.co,), float("nan"), device=gpu_device)
    f = L.MovaeFuse()
    f.stats, f.stats_cap = stats.data_ptr(), parts * 2 * g.co - 1
    bt.run_fwd(L, tiled, gpu_device, g, x, w, b, kernel_of(g), act=False, fuse=f)
    torch.cuda.synchronize()
    assert f.stats_parts == 0 and bool(torch.isnan(stats).all())


@gpu
@pytest.mark.parametrize("kind", bt.KINDS)
@pytest.mark.parametrize("name,off,expect", [("N16", "", TILED), ("NK4", "", TILED), ("NOP", "", TILED), ("NPX", "", TILED),
                                             ("I1", "x", "igemm_bwd<128,32,false>")])
def test_neighbours_of_the_gate_keep_their_kernel(L, tiled, gpu_device, name, off, expect, kind):
    check(L, tiled, gpu_device, name, kind, expect, off=off)


@gpu
def test_input_gradient_entry_points_keep_their_kernels(L, tiled, gpu_device):
    g = geo("D")
    x, dy, w, _ = data("D", "int")
    dx = bt.run_dgrad(L, tiled, gpu_device, g, dy, w, TILED)
    want = bt.memo(("convT image D dgrad",), lambda: bt.ref_dgrad(g, dy, w)).float()
    assert torch.equal(dx, want)
    dx2, dws, dbs = bt.run_pair(L, tiled, gpu_device, g, dy, w, x, "igemm2_pair<1,128,32,64,64>")
    L.defer_flush()
    torch.cuda.synchronize()
    assert torch.equal(dx2, want)
    dw, db = bt.ref_wgrad(g, dy, x)
    assert torch.equal(dws[0], dw.float()) and torch.equal(dbs[0], db.float())


# ---- CPU checks of this file's own machinery ------------------------------------------------------------------------------------
def test_cases_sit_where_the_docstring_says():
    for name in IMG:
        g = geo(name)
        assert (g.ho, g.wo, g.co, g.k, g.s, g.p) == (2 * g.hi, 2 * g.wi, 32, 3, 2, 1) and g.hi * g.wi % 32 == 0 and g.hi * g.wi <= 256
    assert [blocks_of(geo(n)) for n in IMG] == [2, 4, 3, 2, 1, 1]
    assert (3 * 64) % 128 != 0 and (5 * 64) % 128 != 0 and (3 * 32) % 128 != 0  # I1, I3 and I6 end in a ragged block
    m = mirrored(geo("I1"))
    assert (m.ho, m.wo, m.wshape) == (8, 8, geo("I1").wshape)
    for name, what in (("N16", "co"), ("NK4", "k"), ("NOP", "ho"), ("NPX", "px")):
        g = geo(name)
        inside = {"co": g.co == 32, "k": g.k == 3, "ho": g.ho == 2 * g.hi, "px": g.hi * g.wi % 32 == 0}
        assert not inside[what] and all(v for k, v in inside.items() if k != what), name
    d = geo("D")
    assert (d.ho, d.wo) == (8, 8)


def test_integer_data_is_exact_in_fp32():
    """sum |a| |b| bounds every partial sum of every summation order, with the transformed operand too (half-integers <= 8)."""
    for name in IMG:
        g = geo(name)
        x, _, w, b = (t.abs() for t in data(name, "int"))
        assert float(bt.ref_fwd(g, x, w, b).max()) < 2.0 ** 24
        xv = bt.virt(data(name, "int")[0], int_transform(g.ci))
        assert torch.equal(xv * 2, (xv * 2).round()) and float(xv.abs().max()) <= 8
        assert float(bt.ref_fwd(g, xv.abs() * 2, w, b).max()) < 2.0 ** 24
