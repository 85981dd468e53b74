"""Every BatchNorm kernel path of csrc/bn_act.hip (and movae_bn_stats's reducer) through the C entry points, against float64.

Each case calls the C ABI on tensors of its own and asserts movae_bn_last_path(): a moved dispatch threshold fails the case instead
of changing what it covers.  No branch is selected through the environment -- the MOVAE_BN_* knobs are read once per process, so the
library fixture fails when one of them is set.

Harness
  * every tensor is [rows][C] fp32 (cotangents [G][rows][C]); every output the library writes -- out, dy, save_mean, save_rstd,
    scale, shift, coef, each dgamma[g] / dbeta[g], the running statistics, num_batches_tracked, and the partials buffer that a fold
    uses as scratch -- is a view between two guard zones of GUARD elements of one bit pattern and starts as NaN (or as the known
    vector accumulate = 1 adds to); the guards must be unchanged and nothing may stay NaN.  Inputs are compared with copies after
    each call, and the first 4096 bytes of the workspace must still be zero.  Misaligned operands are views one float past a
    16-byte boundary.
  * the reference is float64 torch on the CPU, from the very fp32 inputs and written from the definition (ref_stats / act_fn / ref_bwd).  The
    stand-alone backward gets the statistics its own forward saved (they are checked against float64 on their own).
  * LeakyReLU / ReLU: inputs are redrawn from manual_seed(base + attempt) until min |z| > 1e-5 in float64 (at most 20 attempts,
    then the test fails); nothing else is excluded from any comparison.  One shape is past what the rule can meet: among the 1.05 M
    pre-activations of (1025, 1028) one always lies within 1e-5 of zero.  Its forward runs all five activations on a plain draw (the
    output is continuous across the kink: a flipped sign moves it by no more than z's own error), its backward the smooth ones only.
  * two input regimes: usual, y = 2 randn + 0.5, and far-mean, y = randn + 8 (mean^2 / var ~ 64).

Tolerances.  |got - ref| <= K[q] * 2^-24 * mag, mag being the magnitude of the terms the kernel adds for that quantity (the formulas
stand where they are used).  K[q] = 4 x the worst ratio |got - ref| / (2^-24 * mag) that one run on an MI355X showed over all cases of
the quantity, rounded up to the next half.  In the usual regime the tolerance is in addition capped by what the project accepts
already: rtol 2e-4 + 2e-5 max|ref| for forward values and statistics, rtol 1e-3 + 2e-5 max|ref| for gradients (min(bound, ceiling) elementwise, so
it is never looser).  rows <= 2 is degenerate and counts as far-mean: one row has var = 0, so mean^2 / var has no bound; two rows have
x_hat = +-1 whatever y is, so dy is zero up to eps / var and what is left of it is the rounding of terms 10^3 times its size.

  |A: against the kernels' algebra in float64 on the rounded partials they were given; |B: against the definition on (dout, y).
  fwd / bwd: the stand-alone kernels; fin: movae_bn_finalize on synthetic partials; stats: movae_bn_stats's partials; sfin:
  movae_bn_finalize on those; coef: the coefficient backward; ssa: movae_scale_shift_act.
  quantity                   worst ratio       K
  fwd.mean                         0.985     4.0
  fwd.rstd                         1.442     6.0
  fwd.running_mean                 1.140     5.0
  fwd.running_var                  1.072     4.5
  fwd.out                          1.371     5.5
  bwd.dbeta                        0.800     3.5
  bwd.dgamma                       0.910     4.0
  bwd.dy                           2.419    10.0
  fin.mean|A                       0.996     4.0
  fin.rstd|A                       1.016     4.5
  fin.scale|A                      2.551    10.5
  fin.shift|A                      3.165    13.0
  fin.running_mean|A               1.168     5.0
  fin.running_var|A                1.060     4.5
  fin.mean|B                       1.751     7.5
  fin.rstd|B                       1.201     5.0
  fin.scale|B                      1.834     7.5
  fin.shift|B                      1.332     5.5
  fin.running_mean|B               1.546     6.5
  fin.running_var|B                1.102     4.5
  sfin.mean|B                      4.682    19.0
  sfin.rstd|B                      6.212    25.0
  sfin.scale|B                     6.212    25.0
  sfin.shift|B                     6.183    25.0
  sfin.running_mean|B              4.179    17.0
  sfin.running_var|B               3.993    16.0
  stats.sum                        9.033    36.5
  stats.sumsq                     10.055    40.5
  coef.dbeta|A                     0.999     4.0
  coef.dgamma|A                    0.989     4.0
  coef.coef|A                      0.987     4.0
  coef.dy|A                        2.530    10.5
  coef.dbeta|B                     1.559     6.5
  coef.dgamma|B                    1.555     6.5
  coef.dy|B                        1.860     7.5
  ssa.out                          0.998     4.0

Kernels -> the tests that run them (each asserts the path in brackets)
  bn_fwd_small                                test_fwd[S*]                                   [fwd_small]
  bn_stats_partial4, bn_stats_final           test_fwd[V*], [M3] (+ bn_apply<true> / <false>)  [fwd_stats4+apply_vec / _scalar]
  bn_stats_partial, bn_stats_final            test_fwd[C*], [M1]                             [fwd_stats+apply_scalar]
  bn_apply<true>, bn_apply<false>             test_fwd[V*] / [C*], [M*]; test_fwd_eval
  bn_eval_prepare                             test_fwd_eval                                  [fwd_eval+apply_vec / _scalar]
  bn_bwd_small                                test_bwd_shapes[S*], test_bwd_matrix[small]    [bwd_small]
  bn_bwd_partial4, bn_bwd_final, bn_bwd_apply4   test_bwd_shapes[V*], test_bwd_matrix[vec4]  [bwd_vec4]
  bn_bwd_partial, bn_bwd_final, bn_bwd_apply  test_bwd_shapes[C*, M*], test_bwd_matrix[scalar]   [bwd_scalar]
  bn_finalize_k                               test_finalize, test_stats_then_finalize        [finalize]
  bn_partials_fold_k                          test_finalize[P2049f, P2500f], test_coef_bwd[ppg 2049]   [fold+finalize, bwd_fold+...]
  bn_bwd_fused_k                              test_coef_bwd[ppg <= 256], test_coef_bwd_extra (accumulate over many row chunks)   [bwd_fused]
  bn_bwd_finalize_k, bn_bwd_apply_coef_k      test_coef_bwd[ppg 257, 2049] (also called one by one)
                                                                   [bwd_finalize+apply, bwd_fold+finalize+apply, bwd_finalize, bwd_apply]
  scale_shift_act_k                           test_scale_shift_act                           [scale_shift_act]
  splitk_reduce_stats (movae_bn_stats)        test_stats_then_finalize
The refusals (test_standalone_refusals, test_stats_refusals, test_coef_refusals) launch nothing; test_workspace_of_the_stated_size
runs the scalar kernels in a workspace of exactly movae_bn_ws_bytes.
"""
import ctypes as C
import itertools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
PATTERN = -1.2345678e30
EPS, MOM, SLOPE = 1e-5, 0.1, 0.01
ACTS = ("none", "lrelu", "relu", "tanh", "sigmoid")
ACT_ID = {"none": 0, "lrelu": 1, "relu": 2, "tanh": 3, "sigmoid": 4}
FWD_CEIL, GRAD_CEIL, CEIL_ATOL = 2e-4, 1e-3, 2e-5

# K per quantity (the table of the docstring)
K = {
    "fwd.mean": 4.0,
    "fwd.rstd": 6.0,
    "fwd.running_mean": 5.0,
    "fwd.running_var": 4.5,
    "fwd.out": 5.5,
    "bwd.dbeta": 3.5,
    "bwd.dgamma": 4.0,
    "bwd.dy": 10.0,
    "fin.mean|A": 4.0,
    "fin.rstd|A": 4.5,
    "fin.scale|A": 10.5,
    "fin.shift|A": 13.0,
    "fin.running_mean|A": 5.0,
    "fin.running_var|A": 4.5,
    "fin.mean|B": 7.5,
    "fin.rstd|B": 5.0,
    "fin.scale|B": 7.5,
    "fin.shift|B": 5.5,
    "fin.running_mean|B": 6.5,
    "fin.running_var|B": 4.5,
    "sfin.mean|B": 19.0,
    "sfin.rstd|B": 25.0,
    "sfin.scale|B": 25.0,
    "sfin.shift|B": 25.0,
    "sfin.running_mean|B": 17.0,
    "sfin.running_var|B": 16.0,
    "stats.sum": 36.5,
    "stats.sumsq": 40.5,
    "coef.dbeta|A": 4.0,
    "coef.dgamma|A": 4.0,
    "coef.coef|A": 4.0,
    "coef.dy|A": 10.5,
    "coef.dbeta|B": 6.5,
    "coef.dgamma|B": 6.5,
    "coef.dy|B": 7.5,
    "ssa.out": 4.0,
}
WORST = {}


# ---- float64 reference, from the definition ---------------------------------------------------------------------------------------
def act_fn(z, act, slope):
    if act == "lrelu":
        return torch.where(z > 0, z, z * slope)
    if act == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == "tanh":
        return torch.tanh(z)
    if act == "sigmoid":
        return torch.sigmoid(z)
    return z


def act_grad(z, act, slope):
    one = torch.ones_like(z)
    if act == "lrelu":
        return torch.where(z > 0, one, one * slope)
    if act == "relu":
        return torch.where(z > 0, one, 0 * one)
    if act == "tanh":
        return 1 - torch.tanh(z) ** 2
    if act == "sigmoid":
        s = torch.sigmoid(z)
        return s * (1 - s)
    return one


def ref_stats(y):
    """y float64 [rows][C] -> batch mean, biased variance, 1/sqrt(var + eps), unbiased variance (the biased one for rows == 1)."""
    rows = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + EPS), var * (rows / (rows - 1)) if rows > 1 else var


def ref_bwd(y, dout, gamma, beta, mean, rstd, act, slope):
    """dout [G][rows][C]; mean / rstd as saved.  -> dz, x_hat, dbeta [G][C], dgamma [G][C], dy, m1 = mean dz, m2 = mean dz x_hat."""
    xh = (y - mean) * rstd
    dz = dout * act_grad(xh * gamma + beta, act, slope)
    m1, m2 = dz.mean(1), (dz * xh).mean(1)
    dy = gamma * rstd * (dz - m1[:, None] - xh * m2[:, None])
    return dz, xh, dz.sum(1), (dz * xh).sum(1), dy, m1, m2


def draw(rows, c, base, far, kinked, make_z=None):
    """fp32 (y, gamma, beta) from manual_seed(base + attempt), redrawn while a pre-activation sits within 1e-5 of the kink."""
    for attempt in range(20):
        g = torch.Generator().manual_seed(base + attempt)
        y = torch.randn(rows, c, generator=g) + 8.0 if far else 2.0 * torch.randn(rows, c, generator=g) + 0.5
        gamma = 0.5 + torch.rand(c, generator=g)
        beta = 0.2 * torch.randn(c, generator=g)
        if not kinked:
            return y, gamma, beta, g
        if make_z is None:
            mean, _, rstd, _ = ref_stats(y.double())
            z = (y.double() - mean) * rstd * gamma.double() + beta.double()
        else:
            z = make_z(y, gamma, beta)
        if float(z.abs().min()) > 1e-5:
            return y, gamma, beta, g
    pytest.fail(f"no draw with min |z| > 1e-5 in 20 attempts from seed {base} at ({rows}, {c})")


# ---- GPU plumbing -------------------------------------------------------------------------------------------------------------------
class Buf:
    """An output between two guard zones; NaN inside unless `init`.  off: elements past a 16-byte boundary."""

    def __init__(self, shape, dev, init=None, off=0, dtype=torch.float32, guard=GUARD):
        n = 1
        for d in shape:
            n *= d
        self.lo = guard + off
        pat = PATTERN if dtype.is_floating_point else -0x123456789ABCDEF
        self.pat = torch.full((1,), pat, dtype=dtype)
        self.buf = torch.full((n + 2 * guard + off,), pat, dtype=dtype, device=dev)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if dtype == torch.float32:
            assert self.t.data_ptr() % 16 == 4 * (off % 4)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)
        self.start = self.t.cpu().clone()

    def ptr(self):
        return self.t.data_ptr()

    def guards_ok(self):
        n = self.t.numel()
        both = torch.cat([self.buf[:self.lo], self.buf[self.lo + n:]]).cpu()
        return bool((both == self.pat).all())

    def untouched(self):
        a, b = self.t.cpu(), self.start
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()) if a.dtype.is_floating_point else bool((a == b).all())


class Env:
    def __init__(self, lib, dev):
        self.L, self.lib, self.dev = lib, lib.load(), dev
        self.ws = lib.workspace(dev)
        self.outs, self.ins = [], []

    def out(self, shape, init=None, off=0, dtype=torch.float32, guard=GUARD):
        b = Buf(shape, self.dev, init, off, dtype, guard)
        self.outs.append(b)
        return b

    def inp(self, t, off=0):
        """t on the device (off: one float past a 16-byte boundary); compared with t after the call."""
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=self.dev)
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * off
        self.ins.append((v, t))
        return v

    def st(self):
        return self.L.stream_ptr(self.dev)

    def path(self):
        return self.lib.movae_bn_last_path().decode()

    def wsargs(self):
        return self.ws.data_ptr(), self.ws.numel()

    def done(self, what, written=True):
        """After a call: guards intact, nothing left NaN (or, for a refusal, nothing written at all), inputs and header unchanged."""
        torch.cuda.synchronize()
        for i, b in enumerate(self.outs):
            assert b.guards_ok(), f"{what}: a store outside output #{i} of shape {tuple(b.t.shape)}"
            if not written:
                assert b.untouched(), f"{what}: a refused call wrote to output #{i}"
        for i, (v, t) in enumerate(self.ins):
            assert torch.equal(v.cpu(), t), f"{what}: input #{i} of shape {tuple(t.shape)} was modified"
        assert not bool(self.ws[:4096].any()), f"{what}: the workspace header is no longer zero"
        self.outs, self.ins = [], []


@pytest.fixture(scope="module")
def E(gpu_device):
    knobs = sorted(k for k in os.environ if k.startswith("MOVAE_BN_"))
    if knobs:
        pytest.fail(f"{', '.join(knobs)} set in the environment: the paths this module asserts hold at the defaults only")
    import movae_amd
    import movae_amd._lib as lib

    movae_amd.load_library()
    yield Env(lib, gpu_device)
    print("\nworst |got - ref| / (2^-24 mag) per quantity, and K:")
    for q in K:
        if q in WORST:
            print(f"  {q:<24}{WORST[q]:10.3f}{K[q]:8.1f}")


def check(q, got, ref, mag, what, ceil=None, hard=None):
    """|got - ref| <= K[q] 2^-24 mag, and, with `ceil` (an rtol), also <= ceil |ref| + 2e-5 max |ref|, and also <= hard.  Records the
    worst ratio."""
    got = got.detach().double().cpu()
    ref = ref.double()
    assert got.shape == ref.shape, f"{what} {q}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what} {q}: {int((~torch.isfinite(got)).sum())} elements unwritten or not finite"
    mag = mag.double().expand_as(ref)
    err = (got - ref).abs()
    ratio = torch.where(mag > 0, err / (U * mag), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[q] = max(WORST.get(q, 0.0), worst)
    print(f"{what} {q}: worst ratio {worst:.3f} (K {K[q]})")
    tol = K[q] * U * mag
    if ceil is not None:
        tol = torch.minimum(tol, ceil * ref.abs() + CEIL_ATOL * float(ref.abs().max()))
    if hard is not None:
        tol = torch.minimum(tol, hard.double())
    bad = err > tol
    if bool(bad.any()):
        i = int((err - tol).flatten().argmax())
        pytest.fail(f"{what} {q}: {int(bad.sum())} of {bad.numel()} outside the bound; worst at flat index {i}: got {got.flatten()[i]:.9g}, "
                    f"ref {ref.flatten()[i]:.9g}, bound {tol.flatten()[i]:.3g}, ratio to 2^-24 mag {worst:.2f} (K {K[q]})")


def ptr_array(bufs):
    """HOST array of device pointers for dgamma / dbeta (None entries: null slots)."""
    return (C.c_void_p * len(bufs))(*[None if b is None else b.ptr() for b in bufs])


# ---- stand-alone forward -------------------------------------------------------------------------------------------------------------
KINK_MAX = 300_000  # elements up to which a draw with min |z| > 1e-5 exists in practice: P = exp(-2e-5 p(0) N), p(0) ~ 0.35


def run_fwd(E, rows, c, act, far, base, expect, off_y=0, off_p=0, running=True, what="", bwd=False):
    """One training-mode call, everything it writes checked.  -> the state the backward needs (bwd: one follows).  The forward is
    continuous across the kink (|act(a) - act(b)| <= |a - b|), so the one shape too large for the kink rule (1025 x 1028: a million
    draws always have one within 1e-5 of zero) runs forward without it, and its backward takes the smooth activations only."""
    what = what or f"fwd({rows},{c},{act},{'far' if far else 'usual'})"
    assert not (bwd and rows * c > KINK_MAX and act in ("lrelu", "relu")), "a backward over a kinked activation needs the kink rule"
    y, gamma, beta, g = draw(rows, c, base, far, act in ("lrelu", "relu") and rows * c <= KINK_MAX)
    rm0, rv0 = 0.3 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    yd, gd, bd = E.inp(y, off_y), E.inp(gamma, off_p), E.inp(beta, off_p)
    out, sm, sr = E.out((rows, c), off=off_y), E.out((c,)), E.out((c,))
    rm, rv = (E.out((c,), rm0), E.out((c,), rv0)) if running else (None, None)
    nbt = E.out((1,), torch.tensor([7]), dtype=torch.int64, guard=8) if running else None
    E.L.call("movae_bn_act_fwd", yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), sm.ptr(), sr.ptr(), rm and rm.ptr(), rv and rv.ptr(),
             nbt and nbt.ptr(), rows, c, EPS, MOM, 1, ACT_ID[act], SLOPE, *E.wsargs(), E.st())
    assert E.path() == expect, f"{what}: served by {E.path()}, the case was written for {expect}"
    E.done(what)
    y64, ga, be = y.double(), gamma.double(), beta.double()
    mean, var, rstd, unb = ref_stats(y64)
    std = var.sqrt()
    cap = None if far or rows <= 2 else FWD_CEIL
    # statistics: fp64 accumulation, so only the rounding of the results to fp32 -- relative to |mean| + std and to rstd
    check("fwd.mean", sm.t, mean, mean.abs() + std, what, cap)
    check("fwd.rstd", sr.t, rstd, rstd, what, cap)
    if running:
        # (1 - momentum) old + momentum new, formed in fp64 and rounded once
        check("fwd.running_mean", rm.t, (1 - MOM) * rm0.double() + MOM * mean, (1 - MOM) * rm0.double().abs() + MOM * (mean.abs() + std), what, cap)
        check("fwd.running_var", rv.t, (1 - MOM) * rv0.double() + MOM * unb, (1 - MOM) * rv0.double() + MOM * unb, what, cap)
        assert int(nbt.t.item()) == 8, f"{what}: num_batches_tracked {int(nbt.t.item())}, expected 7 + 1"
    xh = (y64 - mean) * rstd
    ref = act_fn(xh * ga + be, act, SLOPE)
    # (y - mean) * rstd * gamma + beta in fp32: y - mean carries the rounding of mean (|mean| 2^-24, times rstd), each product one more
    # rounding of |x_hat|, the sum one of |z| <= |gamma| |x_hat| + |beta|; the activations are 1-Lipschitz, tanhf / expf add a few ulp of |ref|
    check("fwd.out", out.t, ref, ga.abs() * (xh.abs() + mean.abs() * rstd + 1) + ref.abs(), what, cap)
    return dict(y=y, gamma=gamma, beta=beta, mean=sm.t.cpu().clone(), rstd=sr.t.cpu().clone(), g=g, off_y=off_y, off_p=off_p)


SMALL_SHAPES = [(r, c) for r in (1, 2, 255, 256, 257, 1023, 1024) for c in (4, 12, 36)]
FWD_CASES = (
    [(f"S{r}x{c}", r, c, 0, 0, "fwd_small") for r, c in SMALL_SHAPES] +
    [("V1025x32", 1025, 32, 0, 0, "fwd_stats4+apply_vec"),      # 9 partial blocks, the last holding one row
     ("V2100x12", 2100, 12, 0, 0, "fwd_stats4+apply_vec"),      # 3 quads on 4 column lanes: one idles
     ("V1025x260", 1025, 260, 0, 0, "fwd_stats4+apply_vec"),    # RG = 2
     ("V1025x1028", 1025, 1028, 0, 0, "fwd_stats4+apply_vec"),  # 257 quads: two column passes
     ("C1x3", 1, 3, 0, 0, "fwd_stats+apply_scalar"), ("C5x6", 5, 6, 0, 0, "fwd_stats+apply_scalar"),
     ("C1025x3", 1025, 3, 0, 0, "fwd_stats+apply_scalar"), ("C1500x6", 1500, 6, 0, 0, "fwd_stats+apply_scalar"),
     ("C1030x257", 1030, 257, 0, 0, "fwd_stats+apply_scalar"),  # two column passes
     ("M1_300x8_y", 300, 8, 1, 0, "fwd_stats+apply_scalar"),    # y / out one float off: scalar throughout although C % 4 == 0
     ("M2_300x8_p", 300, 8, 0, 1, "fwd_stats4+apply_scalar"),   # gamma / beta off: the one-launch kernel is refused
     ("M3_1500x8_p", 1500, 8, 0, 1, "fwd_stats4+apply_scalar")])
REGIMES = [pytest.param(False, id="usual"), pytest.param(True, id="far")]


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_fwd(E, case, far):
    name, rows, c, off_y, off_p, expect = case
    for i, act in enumerate(ACTS):
        run_fwd(E, rows, c, act, far, 1000 + 20 * i, expect, off_y, off_p, running=act != "tanh", what=f"{name}/{act}")


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("case", [("E300x8", 300, 8, 0, "fwd_eval+apply_vec"), ("E1500x8", 1500, 8, 0, "fwd_eval+apply_vec"),
                                  ("E300x6", 300, 6, 0, "fwd_eval+apply_scalar"), ("E300x8_y", 300, 8, 1, "fwd_eval+apply_scalar")],
                         ids=lambda c: c[0])
def test_fwd_eval(E, case, far):
    """Eval mode: the running statistics are read, not written; save_mean is their mean, save_rstd 1 / sqrt(running_var + eps)."""
    name, rows, c, off_y, expect = case
    for i, act in enumerate(ACTS):
        what = f"{name}/{act}"
        for attempt in range(20):
            g = torch.Generator().manual_seed(2000 + 20 * i + attempt)
            y = torch.randn(rows, c, generator=g) + 8.0 if far else 2.0 * torch.randn(rows, c, generator=g) + 0.5
            gamma, beta = 0.5 + torch.rand(c, generator=g), 0.2 * torch.randn(c, generator=g)
            rm0 = (8.0 if far else 0.5) + 0.3 * torch.randn(c, generator=g)
            rv0 = 0.5 + torch.rand(c, generator=g)
            rstd = 1.0 / torch.sqrt(rv0.double() + EPS)
            xh = (y.double() - rm0.double()) * rstd
            z = xh * gamma.double() + beta.double()
            if act not in ("lrelu", "relu") or float(z.abs().min()) > 1e-5:
                break
        else:
            pytest.fail(f"{what}: no draw with min |z| > 1e-5")
        yd, gd, bd = E.inp(y, off_y), E.inp(gamma), E.inp(beta)
        out, sm, sr = E.out((rows, c), off=off_y), E.out((c,)), E.out((c,))
        rm, rv = E.out((c,), rm0), E.out((c,), rv0)
        nbt = E.out((1,), torch.tensor([7]), dtype=torch.int64, guard=8)
        E.L.call("movae_bn_act_fwd", yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), sm.ptr(), sr.ptr(), rm.ptr(), rv.ptr(), nbt.ptr(),
                 rows, c, EPS, MOM, 0, ACT_ID[act], SLOPE, None, 0, E.st())  # (no workspace: eval mode needs none)
        assert E.path() == expect, f"{what}: served by {E.path()}, the case was written for {expect}"
        keep = (rm, rv, nbt)
        E.done(what)
        assert all(b.untouched() for b in keep), f"{what}: eval mode wrote to the running statistics or num_batches_tracked"
        assert torch.equal(sm.t.cpu(), rm0), f"{what}: save_mean is not the running mean"
        cap = None if far else FWD_CEIL
        check("fwd.rstd", sr.t, rstd, rstd, what, cap)
        ref = act_fn(z, act, SLOPE)
        check("fwd.out", out.t, ref, gamma.double() * (xh.abs() + rm0.double().abs() * rstd + 1) + ref.abs(), what, cap)


# ---- stand-alone backward -------------------------------------------------------------------------------------------------------------
def run_bwd(E, s, rows, c, act, far, G, acc, expect, null=None, what=""):
    """s: run_fwd's state.  null: None | a group index whose dgamma / dbeta slots are null | "all" (both arrays null)."""
    y, gamma, beta, mean, rstd = s["y"], s["gamma"], s["beta"], s["mean"], s["rstd"]
    g = torch.Generator().manual_seed(77 + 13 * G + acc)
    dout = torch.randn(G, rows, c, generator=g) * (1.0 + torch.arange(G, dtype=torch.float32))[:, None, None]  # a cotangent of its own per group
    init = torch.randn(2, G, c, generator=g) * 3.0
    yd, gd, bd = E.inp(y, s["off_y"]), E.inp(gamma, s["off_p"]), E.inp(beta, s["off_p"])
    md, rd, dd = E.inp(mean), E.inp(rstd), E.inp(dout, s["off_y"])
    dy = E.out((G, rows, c), off=s["off_y"])
    slots = [[None if null in ("all", i) else E.out((c,), init[k, i] if acc else None) for i in range(G)] for k in range(2)]
    tail = (rows, c, ACT_ID[act], SLOPE, acc, *E.wsargs(), E.st())
    if G == 1 and not acc and null is None:
        E.L.call("movae_bn_act_bwd", dd.data_ptr(), yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), md.data_ptr(), rd.data_ptr(), dy.ptr(),
                 slots[0][0].ptr(), slots[1][0].ptr(), *tail)
    else:
        arrs = (None, None) if null == "all" else (ptr_array(slots[0]), ptr_array(slots[1]))
        E.L.call("movae_bn_act_bwd_grouped", G, dd.data_ptr(), yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), md.data_ptr(), rd.data_ptr(), dy.ptr(),
                 arrs[0], arrs[1], *tail)
    assert E.path() == expect, f"{what}: served by {E.path()}, the case was written for {expect}"
    E.done(what)
    ga, m, r = gamma.double(), mean.double(), rstd.double()
    dz, xh, dbeta, dgamma, dyr, m1, m2 = ref_bwd(y.double(), dout.double(), ga, beta.double(), m, r, act, SLOPE)
    cap = None if far or rows <= 2 else GRAD_CEIL
    # dz = dout act'(z) in fp32: one rounding of |dz|; for tanh / sigmoid act' is formed from the rounded output o, whose error is that of
    # z (2^-24 |gamma| (|x_hat| + |mean| rstd + 1), as in the forward) through |act''| <= 1: e_dz = |dout| (1 + smooth zmag)
    smooth = 1.0 if act in ("tanh", "sigmoid") else 0.0
    e_dz = dout.double().abs() * (1 + smooth * ga * (xh.abs() + m.abs() * r + 1))
    add = init.double() if acc else torch.zeros(2, G, c, dtype=torch.float64)
    for i in range(G):
        if null in ("all", i):
            continue
        # the sums are accumulated in fp64 over fp32 terms: the terms' own errors add up, plus the rounding of the result (and of the add)
        check("bwd.dgamma", slots[0][i].t, add[0, i] + dgamma[i], (e_dz[i] * xh.abs()).sum(0) + dgamma[i].abs() + add[0, i].abs(), f"{what} g{i}", cap)
        check("bwd.dbeta", slots[1][i].t, add[1, i] + dbeta[i], e_dz[i].sum(0) + dbeta[i].abs() + add[1, i].abs(), f"{what} g{i}", cap)
    # gamma rstd (dz - m1 - x_hat m2) in fp32: every term rounded; m1 and m2 are means of rounded terms, so they carry the mean of the
    # terms' errors (mean e_dz, mean e_dz |x_hat|: more than 2^-24 |m1|, the means being small by cancellation)
    check("bwd.dy", dy.t, dyr, ga * r * (e_dz + e_dz.mean(1)[:, None] + xh.abs() * (e_dz * xh.abs()).mean(1)[:, None]), what, cap)


BWD_SHAPES = (
    [(f"S{r}x{c}", r, c, 0, 0, "fwd_small", "bwd_small") for r, c in SMALL_SHAPES] +
    [("V1025x32", 1025, 32, 0, 0, "fwd_stats4+apply_vec", "bwd_vec4"), ("V2100x12", 2100, 12, 0, 0, "fwd_stats4+apply_vec", "bwd_vec4"),
     ("V1025x260", 1025, 260, 0, 0, "fwd_stats4+apply_vec", "bwd_vec4"), ("V1025x1028", 1025, 1028, 0, 0, "fwd_stats4+apply_vec", "bwd_vec4"),
     ("V4100x8", 4100, 8, 0, 0, "fwd_stats4+apply_vec", "bwd_vec4"),
     ("C1x3", 1, 3, 0, 0, "fwd_stats+apply_scalar", "bwd_scalar"), ("C5x6", 5, 6, 0, 0, "fwd_stats+apply_scalar", "bwd_scalar"),
     ("C1025x3", 1025, 3, 0, 0, "fwd_stats+apply_scalar", "bwd_scalar"), ("C1500x6", 1500, 6, 0, 0, "fwd_stats+apply_scalar", "bwd_scalar"),
     ("C1030x257", 1030, 257, 0, 0, "fwd_stats+apply_scalar", "bwd_scalar"),
     ("M1_300x8_y", 300, 8, 1, 0, "fwd_stats+apply_scalar", "bwd_scalar"), ("M2_300x8_p", 300, 8, 0, 1, "fwd_stats4+apply_scalar", "bwd_scalar"),
     ("M3_1500x8_p", 1500, 8, 0, 1, "fwd_stats4+apply_scalar", "bwd_scalar")])
GROUPS = (1, 2, 3, 8)


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("idx", range(len(BWD_SHAPES)), ids=[c[0] for c in BWD_SHAPES])
def test_bwd_shapes(E, idx, far):
    """Every shape family of the forward, two (groups, accumulate, activation) combinations each, rotating with the case."""
    name, rows, c, off_y, off_p, fexp, bexp = BWD_SHAPES[idx]
    for j in range(2):
        i = 2 * idx + j
        act, acc, G = ACTS[i % 5], (i // 5 + j) % 2, GROUPS[(i // 2 + j) % 4]
        if rows * c > KINK_MAX and act in ("lrelu", "relu"):
            act = ("tanh", "sigmoid")[j]
        while G > 1 and G * rows * c > 1_100_000:
            G = GROUPS[GROUPS.index(G) - 1]
        s = run_fwd(E, rows, c, act, far, 3000 + 20 * i, fexp, off_y, off_p, what=f"{name}/fwd/{act}", bwd=True)
        run_bwd(E, s, rows, c, act, far, G, acc, bexp, what=f"{name}/{act}/G{G}/acc{acc}")


MATRIX = {"small": (257, 12, "fwd_small", "bwd_small"), "vec4": (1025, 32, "fwd_stats4+apply_vec", "bwd_vec4"),
          "scalar": (1025, 3, "fwd_stats+apply_scalar", "bwd_scalar")}


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("fam", list(MATRIX))
def test_bwd_matrix(E, fam, act, far):
    """One shape per path: every group count x accumulate x activation; a null slot for one group and both arrays null."""
    rows, c, fexp, bexp = MATRIX[fam]
    s = run_fwd(E, rows, c, act, far, 4000 + 20 * ACTS.index(act), fexp, what=f"{fam}/fwd/{act}", bwd=True)
    for G, acc in itertools.product(GROUPS, (0, 1)):
        run_bwd(E, s, rows, c, act, far, G, acc, bexp, what=f"{fam}/{act}/G{G}/acc{acc}")
    run_bwd(E, s, rows, c, act, far, 3, 1, bexp, null=1, what=f"{fam}/{act}/G3/null slot 1")
    run_bwd(E, s, rows, c, act, far, 2, 0, bexp, null="all", what=f"{fam}/{act}/G2/null arrays")
    run_bwd(E, s, rows, c, act, far, 1, 0, bexp, null=0, what=f"{fam}/{act}/G1/null slot 0")


def test_standalone_refusals(E):
    """groups out of range and a missing workspace are argument errors: nothing is launched, nothing written."""
    rows, c = 1025, 32
    y, gamma, beta, g = draw(rows, c, 5000, False, False)
    mean, _, rstd, _ = ref_stats(y.double())
    dout = torch.randn(9, rows, c, generator=g)
    for G, ws in ((0, True), (9, True), (2, False)):
        yd, gd, bd, md, rd, dd = E.inp(y), E.inp(gamma), E.inp(beta), E.inp(mean.float()), E.inp(rstd.float()), E.inp(dout)
        dy = E.out((9, rows, c))
        slots = [[E.out((c,)) for _ in range(9)] for _ in range(2)]
        with pytest.raises(RuntimeError):
            E.L.call("movae_bn_act_bwd_grouped", G, dd.data_ptr(), yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), md.data_ptr(), rd.data_ptr(), dy.ptr(),
                     ptr_array(slots[0]), ptr_array(slots[1]), rows, c, 1, SLOPE, 0, *(E.wsargs() if ws else (None, 0)), E.st())
        E.done(f"bwd refusal G={G} ws={ws}", written=False)
    yd, gd, bd = E.inp(y), E.inp(gamma), E.inp(beta)
    out, sm, sr = E.out((rows, c)), E.out((c,)), E.out((c,))
    with pytest.raises(RuntimeError):
        E.L.call("movae_bn_act_fwd", yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), sm.ptr(), sr.ptr(), None, None, None, rows, c, EPS, MOM, 1, 1,
                 SLOPE, None, 0, E.st())
    E.done("fwd refusal without a workspace", written=False)


@pytest.mark.parametrize("rows,c", [(300, 8), (1500, 8), (1025, 3)])
def test_workspace_of_the_stated_size(E, rows, c):
    """A workspace of exactly movae_bn_ws_bytes (4096 + groups x the rest for the grouped backward) is enough on the scalar path too:
    misaligned operands send C % 4 == 0 to the scalar kernels, whose split has more partial blocks than the 4-wide one
    (3 against 1 at (300, 8)).  The workspace lies between guards."""
    G = 2
    need = E.lib.movae_bn_ws_bytes(rows, c)
    need_g = 4096 + G * (need - 4096)
    y, gamma, beta, g = draw(rows, c, 5100, False, True)
    dout = torch.randn(G, rows, c, generator=g)
    ws = Buf((need_g // 4 + 1,), E.dev, torch.zeros(need_g // 4 + 1), guard=4096)
    yd, gd, bd = E.inp(y, 1), E.inp(gamma), E.inp(beta)
    out, sm, sr = E.out((rows, c), off=1), E.out((c,)), E.out((c,))
    E.L.call("movae_bn_act_fwd", yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), sm.ptr(), sr.ptr(), None, None, None, rows, c, EPS, MOM, 1, 1,
             SLOPE, ws.ptr(), need, E.st())
    assert E.path() == "fwd_stats+apply_scalar"
    dd, dy = E.inp(dout, 1), E.out((G, rows, c), off=1)
    slots = [[E.out((c,)) for _ in range(G)] for _ in range(2)]
    E.L.call("movae_bn_act_bwd_grouped", G, dd.data_ptr(), yd.data_ptr(), gd.data_ptr(), bd.data_ptr(), sm.ptr(), sr.ptr(), dy.ptr(),
             ptr_array(slots[0]), ptr_array(slots[1]), rows, c, 1, SLOPE, 0, ws.ptr(), need_g, E.st())
    assert E.path() == "bwd_scalar"
    E.done("exact workspace")
    assert ws.guards_ok(), "a store past the end of a workspace of movae_bn_ws_bytes"
    assert not bool(ws.t[:1024].any()), "the workspace header is no longer zero"
    mean, var, rstd, _ = ref_stats(y.double())
    check("fwd.mean", sm.t, mean, mean.abs() + var.sqrt(), "exact workspace", FWD_CEIL)
    _, _, dbeta, dgamma, dyr, _, _ = ref_bwd(y.double(), dout.double(), gamma.double(), beta.double(), sm.t.cpu().double(), sr.t.cpu().double(), "lrelu", SLOPE)
    assert torch.allclose(dy.t.cpu().double(), dyr, rtol=GRAD_CEIL, atol=CEIL_ATOL * float(dyr.abs().max()))
    assert torch.allclose(slots[0][1].t.cpu().double(), dgamma[1], rtol=GRAD_CEIL, atol=CEIL_ATOL * float(dgamma.abs().max()))
    assert torch.allclose(slots[1][1].t.cpu().double(), dbeta[1], rtol=GRAD_CEIL, atol=CEIL_ATOL * float(dbeta.abs().max()))


# ---- coefficient path: movae_bn_finalize ---------------------------------------------------------------------------------------------
def partials(values, P):
    """float64 [..., rows, C] -> [..., P, C]: row r goes to partial r mod P, empty partials stay zero."""
    rows = values.shape[-2]
    out = torch.zeros(*values.shape[:-2], P, values.shape[-1], dtype=torch.float64)
    return out.index_add_(-2, torch.arange(rows) % P, values)


def check_finalize(E, pbuf, cap, P, given, exact_abs, rows, c, y, gamma, beta, g, far, running, expect, what, tag="fin"):
    """movae_bn_finalize on the partials in pbuf ([P][2][C] at its start; the rest is room for a fold).  given: those partials as the
    kernel reads them (fp32 values, float64 tensor [P][2][C]); exact_abs: sum over the partials of |exact partial| per (k, C)."""
    rm0, rv0 = 0.3 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    gd, bd = E.inp(gamma), E.inp(beta)
    sm, sr, sc, sh = E.out((c,)), E.out((c,)), E.out((c,)), E.out((c,))
    rm, rv = (E.out((c,), rm0), E.out((c,), rv0)) if running else (None, None)
    nbt = E.out((1,), torch.tensor([7]), dtype=torch.int64, guard=8) if running else None
    E.outs.append(pbuf)
    E.L.call("movae_bn_finalize", pbuf.ptr(), cap, P, rows, c, gd.data_ptr(), bd.data_ptr(), EPS, MOM, sm.ptr(), sr.ptr(), sc.ptr(), sh.ptr(),
             rm and rm.ptr(), rv and rv.ptr(), nbt and nbt.ptr(), E.st())
    assert E.path() == expect, f"{what}: served by {E.path()}, the case was written for {expect}"
    E.done(what)
    fold = 1.0 if expect.startswith("fold") else 0.0
    if not fold:
        assert torch.equal(pbuf.t.cpu()[:P * 2 * c].double(), given.flatten()), f"{what}: the partials were modified without a fold"
    ga, be = gamma.double(), beta.double()
    if running:
        assert int(nbt.t.item()) == 8, f"{what}: num_batches_tracked {int(nbt.t.item())}, expected 7 + 1"
    # B: the definition on y.  The partials carry 2^-24 of their own size each: mean to 2^-24 sum |partial| / rows, the variance
    # q / rows - mean^2 to 2^-24 (E[y^2] + 2 |mean| E|y|) <= 3 2^-24 (var + mean^2), so 1 / sqrt(var + eps) to the relative
    # 2^-24 (1 + mean^2 / (var + eps)) -- the cancellation factor of test_fused_statistics_at_config_shapes (5e-7 = 8.4 x 2^-24 there)
    mean, var, rstd, unb = ref_stats(y.double())
    F = 1 + mean ** 2 / (var + EPS)
    e_mean, e_sq = exact_abs[0] / rows, exact_abs[1] / rows
    a = rstd * ga
    n1 = rows / (rows - 1) if rows > 1 else 1.0
    cap_ = None if far or rows <= 2 else FWD_CEIL
    # A: the same algebra in float64 on the partials as given: the outputs' own rounding (and, behind a fold, the fp32 fold's)
    s, q = given[:, 0].sum(0), given[:, 1].sum(0)
    mA = s / rows
    vA = (q / rows - mA * mA).clamp_min(0)
    rA = 1 / torch.sqrt(vA + EPS)
    m32, r32 = mA.float().double(), rA.float().double()
    aA = r32 * ga
    uA = vA * n1
    FA = 1 + mA ** 2 / (vA + EPS)
    check("fin.mean|A", sm.t, mA, mA.abs() + fold * e_mean, what)
    check("fin.rstd|A", sr.t, rA, rA * (1 + fold * FA), what)
    check("fin.scale|A", sc.t, aA, aA.abs() * (1 + fold * FA), what)
    check("fin.shift|A", sh.t, be - m32 * aA, ((m32 * aA).abs() + be.abs()) * (1 + fold * FA), what)
    # (whatever K says, the two statistics also stay within test_fused_statistics_at_config_shapes's bounds: 5e-7 (|mean| + std) and
    # 5e-7 (1 + mean^2 / var) relative)
    check(tag + ".mean|B", sm.t, mean, e_mean, what, cap_, hard=5e-7 * (mean.abs() + var.sqrt()))
    check(tag + ".rstd|B", sr.t, rstd, rstd * F, what, cap_, hard=5e-7 * F * rstd)
    check(tag + ".scale|B", sc.t, a, a.abs() * F, what, cap_)
    # shift = beta - mean scale: |mean| times the error of scale, |scale| times that of mean, and its own rounding
    check(tag + ".shift|B", sh.t, be - mean * a, (mean * a).abs() * F + a.abs() * e_mean + be.abs(), what, cap_)
    if running:
        r0, v0 = (1 - MOM) * rm0.double(), (1 - MOM) * rv0.double()
        check("fin.running_mean|A", rm.t, r0 + MOM * mA, r0.abs() + MOM * (mA.abs() + fold * e_mean), what)
        check("fin.running_var|A", rv.t, v0 + MOM * uA, v0 + MOM * n1 * (uA + fold * (e_sq + 2 * mA.abs() * e_mean)), what)
        check(tag + ".running_mean|B", rm.t, r0 + MOM * mean, r0.abs() + MOM * e_mean, what, cap_)
        check(tag + ".running_var|B", rv.t, v0 + MOM * unb, v0 + MOM * n1 * (e_sq + 2 * mean.abs() * e_mean), what, cap_)
    return sm, sr, sc, sh


FIN_P = [(1, 0, "finalize"), (3, 0, "finalize"), (255, 0, "finalize"), (256, 0, "finalize"), (257, 0, "finalize"), (2048, 64, "finalize"),
         (2049, 64, "fold+finalize"), (2500, 64, "fold+finalize"), (2049, 63, "finalize")]  # (partials, rows of room behind them, path)


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("c", [4, 12, 32, 260])
@pytest.mark.parametrize("pcase", FIN_P, ids=lambda p: f"P{p[0]}{'f' if p[2][0] == 'f' else 'n' if p[0] > 2048 else ''}")
def test_finalize(E, pcase, c, far):
    """Synthetic partials: float64 sums of (y, y^2) over the rows r = p mod P, rounded to fp32.  2049 partials with room for 63 folded
    rows only must fall back to the unfolded kernel and still be right."""
    P, room, expect = pcase
    rows = 300 if P <= 3 else P + 41
    y, gamma, beta, g = draw(rows, c, 6000 + P + c, far, False)
    y64 = torch.stack([y.double(), y.double() ** 2], -2)        # [rows][2][C]
    exact = partials(y64.reshape(rows, 2 * c), P).view(P, 2, c)
    cap = (P + room) * 2 * c
    pbuf = Buf((cap,), E.dev, torch.cat([exact.float().flatten(), torch.full((room * 2 * c,), float("nan"))]))
    check_finalize(E, pbuf, cap, P, exact.float().double(), exact.abs().sum(0), rows, c, y, gamma, beta, g, far, (P + c) % 8 != 0, expect,
                   f"finalize(P={P},C={c},{'far' if far else 'usual'})")


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("c", [4, 8, 32, 64, 128])
@pytest.mark.parametrize("rows", [1, 3, 255, 257, 1025, 4100])
def test_stats_then_finalize(E, rows, c, far):
    """movae_bn_stats's partials (fp32 sums of two rows per thread, folded over the block's row groups in fp32) against float64 sums of
    the same rows, then movae_bn_finalize on them."""
    what = f"stats({rows},{c},{'far' if far else 'usual'})"
    y, gamma, beta, g = draw(rows, c, 7000 + rows + c, far, False)
    rpb = 2 * (256 // (c // 4))  # rows per partial block (at most 1024 blocks: not reached below 2048 row groups)
    P = -(-rows // rpb)
    yd = E.inp(y)
    cap = (P + 64) * 2 * c
    pbuf = E.out((cap,))
    pout = C.c_int(-7)
    E.L.call("movae_bn_stats", yd.data_ptr(), rows, c, pbuf.ptr(), cap, C.byref(pout), E.st())
    assert pout.value == P, f"{what}: {pout.value} partials, expected {P} blocks of {rpb} rows"
    torch.cuda.synchronize()
    assert pbuf.guards_ok() and bool(torch.isnan(pbuf.t[P * 2 * c:]).all()), f"{what}: a store outside the {P} partials"
    E.outs.remove(pbuf)
    E.done(what)
    got = pbuf.t.cpu()[:P * 2 * c].view(P, 2, c)
    y64 = torch.stack([y.double(), y.double() ** 2], -2)
    pad = torch.zeros(P * rpb, 2, c, dtype=torch.float64)
    pad[:rows] = y64
    blocks = pad.view(P, rpb, 2, c)
    exact, mags = blocks.sum(1), blocks.abs().sum(1)
    # fp32 throughout: each block's sum to 2^-24 x its terms' magnitudes x the depth of the chain, which K takes up
    check("stats.sum", got[:, 0], exact[:, 0], mags[:, 0], what)
    check("stats.sumsq", got[:, 1], exact[:, 1], mags[:, 1], what)
    check_finalize(E, pbuf, cap, P, got.double(), mags.sum(0), rows, c, y, gamma, beta, g, far, True, "finalize", what, tag="sfin")


def test_stats_refusals(E):
    """C = 12 (256 % (C / 4) != 0) and a misaligned y: MOVAE_EUNSUPPORTED, the caller's int and the buffer untouched."""
    for rows, c, off in ((300, 12, 0), (300, 8, 1)):
        y = torch.randn(rows, c, generator=torch.Generator().manual_seed(8))
        yd, pbuf, pout = E.inp(y, off), E.out((1100 * 2 * c,)), C.c_int(-7)
        with pytest.raises(E.L.Unsupported):
            E.L.call("movae_bn_stats", yd.data_ptr(), rows, c, pbuf.ptr(), pbuf.t.numel(), C.byref(pout), E.st())
        assert pout.value == -7, "a refused movae_bn_stats wrote parts_out"
        E.done(f"stats refusal ({rows},{c},off {off})", written=False)


# ---- coefficient path: backward -------------------------------------------------------------------------------------------------------
def coef_data(rows, c, G, ppg, slope, far, base):
    """fp32 inputs of the coefficient backward, its synthetic partials, and both float64 references."""
    def make_z(y, gamma, beta):
        mean, _, rstd, _ = ref_stats(y.double())
        a = (rstd.float().double() * gamma.double()).float().double()
        b = (beta.double() - mean.float().double() * a).float().double()
        return y.double() * a + b
    y, gamma, beta, g = draw(rows, c, base, far, slope != 1.0, make_z)
    mean, _, rstd, _ = ref_stats(y.double())
    m32, r32 = mean.float(), rstd.float()            # the saved statistics the kernels are given
    a32 = (r32.double() * gamma.double()).float()
    b32 = (beta.double() - m32.double() * a32.double()).float()
    dout = torch.randn(G, rows, c, generator=g) * (1.0 + torch.arange(G, dtype=torch.float32))[:, None, None]
    y64, m, r, ga = y.double(), m32.double(), r32.double(), gamma.double()
    z = y64 * a32.double() + b32.double()  # (the kernels form it with one fma of the same fp32 operands: its sign is exact)
    d = dout.double() * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    exact = partials(torch.stack([d, d * y64], -2).reshape(G, rows, 2 * c), ppg).view(G, ppg, 2, c)
    part = exact.float()
    M = float(rows)
    # A: the kernels' algebra in float64 on the partials as given
    S1, S2 = part.double()[:, :, 0].sum(1), part.double()[:, :, 1].sum(1)
    dgam = r * (S2 - m * S1)
    k1 = (ga * r).expand(G, c)
    c2 = -k1 * r * dgam / M
    c3 = -k1 * S1 / M - c2 * m
    dyA = k1[:, None] * d + c2[:, None] * y64 + c3[:, None]
    # B: the definition
    xh = (y64 - m) * r
    dbB, dgB = d.sum(1), (d * xh).sum(1)
    dyB = ga * r * (d - d.mean(1)[:, None] - xh * (d * xh).mean(1)[:, None])
    E1, E2 = exact[:, :, 0].abs().sum(1), exact[:, :, 1].abs().sum(1)
    # the partials carry 2^-24 of their own size each: S1 to 2^-24 E1, S2 (sums of d y on the RAW y) to 2^-24 E2, and
    # dgamma = rstd (S2 - mean S1) to 2^-24 Edg, Edg = rstd (E2 + |mean| E1).  Far from zero |y| ~ |mean|, so Edg is about
    # (1 + |mean| rstd) x sum |d x_hat|: that is the far-mean factor of dgamma.  dy = k1 (d - S1 / M - x_hat dgamma / M) inherits
    # k1 (E1 + |x_hat| Edg) / M of it, and its fp32 evaluation k1 d + (c2 y + c3) rounds |c2 y| and |c3|, each about |mean| rstd / |x_hat|
    # times their sum: the far-mean factor of dy.
    Edg = r * (E2 + m.abs() * E1)
    arith = (k1[:, None] * d).abs() + (c2[:, None] * y64).abs() + c3.abs()[:, None]
    inherit = k1[:, None] * (E1[:, None] + xh.abs() * Edg[:, None]) / M
    coefA = torch.stack([k1, c2, c3], 1)
    coef_mag = torch.stack([k1, c2.abs(), (k1 * S1 / M).abs() + (c2 * m).abs()], 1)
    coef_inh = torch.stack([0 * k1, k1 * r * Edg / M, k1 * E1 / M + m.abs() * k1 * r * Edg / M], 1)
    return dict(y=y, gamma=gamma, m32=m32, r32=r32, a32=a32, b32=b32, dout=dout, part=part, g=g, S1=S1, dgam=dgam, dyA=dyA, dbB=dbB, dgB=dgB,
                dyB=dyB, E1=E1, Edg=Edg, arith=arith, inherit=inherit, coefA=coefA, coef_mag=coef_mag, coef_inh=coef_inh)


def run_coef(E, D, rows, c, G, ppg, slope, far, acc, room, expect, split=False, null=None, what=""):
    """movae_bn_bwd_finalize_apply (split: movae_bn_bwd_finalize, then movae_bn_bwd_apply, with coef itself checked)."""
    cap = G * (ppg + room) * 2 * c
    pbuf = E.out((cap,), torch.cat([D["part"].flatten(), torch.full((G * room * 2 * c,), float("nan"))]))
    yd, dd, gd = E.inp(D["y"]), E.inp(D["dout"]), E.inp(D["gamma"])
    md, rd, ad, bd = E.inp(D["m32"]), E.inp(D["r32"]), E.inp(D["a32"]), E.inp(D["b32"])
    dy, coef = E.out((G, rows, c)), E.out((G, 3, c))
    init = torch.randn(2, G, c, generator=D["g"]) * 3.0
    slots = [[None if null == i else E.out((c,), init[k, i] if acc else None) for i in range(G)] for k in range(2)]
    fin = (pbuf.ptr(), cap, ppg, G, rows, c, gd.data_ptr(), md.data_ptr(), rd.data_ptr(), ptr_array(slots[0]), ptr_array(slots[1]), coef.ptr(), acc)
    app = (dd.data_ptr(), yd.data_ptr(), ad.data_ptr(), bd.data_ptr(), slope)
    if split:
        E.L.call("movae_bn_bwd_finalize", *fin, E.st())
        assert E.path() == expect[0], f"{what}: served by {E.path()}, the case was written for {expect[0]}"
        E.L.call("movae_bn_bwd_apply", *app, coef.ptr(), dy.ptr(), G, rows, c, E.st())
        assert E.path() == "bwd_apply"
    else:
        if expect == "bwd_fused":
            E.outs.remove(coef)  # scratch that the one-launch form leaves alone
        E.L.call("movae_bn_bwd_finalize_apply", *fin, *app, dy.ptr(), E.st())
        assert E.path() == expect, f"{what}: served by {E.path()}, the case was written for {expect}"
    E.done(what)
    fold = 1.0 if "fold" in (expect[0] if split else expect) else 0.0
    cap_ = None if far or rows <= 2 else GRAD_CEIL
    add = init.double() if acc else torch.zeros(2, G, c, dtype=torch.float64)
    for i in range(G):
        if null == i:
            continue
        w = f"{what} g{i}"
        # A: fp64 sums of the given partials, rounded once (added to the destination in fp64 first); behind a fold the fp32 fold's share
        check("coef.dgamma|A", slots[0][i].t, add[0, i] + D["dgam"][i], (add[0, i] + D["dgam"][i]).abs() + fold * D["Edg"][i], w)
        check("coef.dbeta|A", slots[1][i].t, add[1, i] + D["S1"][i], (add[1, i] + D["S1"][i]).abs() + fold * D["E1"][i], w)
        check("coef.dgamma|B", slots[0][i].t, add[0, i] + D["dgB"][i], D["Edg"][i] + add[0, i].abs(), w, cap_)
        check("coef.dbeta|B", slots[1][i].t, add[1, i] + D["dbB"][i], D["E1"][i] + add[1, i].abs(), w, cap_)
    if split:
        check("coef.coef|A", coef.t, D["coefA"], D["coef_mag"] + fold * D["coef_inh"], what)
    check("coef.dy|A", dy.t, D["dyA"], D["arith"] + fold * D["inherit"], what)
    check("coef.dy|B", dy.t, D["dyB"], D["arith"] + D["inherit"], what, cap_)


COEF_ROWS, COEF_C = (1, 127, 128, 129, 300, 1000), (4, 12, 32, 36, 64, 260)
COEF_PPG = {1: "bwd_fused", 5: "bwd_fused", 64: "bwd_fused", 65: "bwd_fused", 256: "bwd_fused", 257: "bwd_finalize+apply",
            2049: "bwd_fold+finalize+apply"}
COEF_SHAPES = list(itertools.product(COEF_ROWS, COEF_C))


def fit_groups(G, rows, c, ppg, room):
    while G > 1 and max(G * rows * c, G * (ppg + room) * 2 * c) > 1_100_000:
        G = {8: 2, 2: 1}[G]
    return G


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("idx", range(len(COEF_SHAPES)), ids=[f"{r}x{c}" for r, c in COEF_SHAPES])
def test_coef_bwd(E, idx, far):
    """Every (rows, C) of the issue's grid: one to eight row chunks (128 rows at least each), a ragged last 32-channel slice at C = 36
    and 260.  Groups, partials per group, slope and accumulate rotate with the case so that every value meets every path; every third
    case calls the two entry points one by one as well."""
    rows, c = COEF_SHAPES[idx]
    ppg = list(COEF_PPG)[idx % 7]
    slope = (0.01, 0.0, 1.0)[(idx // 3) % 3]
    acc = (idx // 2) % 2
    room = 64 if ppg > 2048 else 0
    G = fit_groups((1, 2, 8)[idx % 3], rows, c, ppg, room)
    D = coef_data(rows, c, G, ppg, slope, far, 9000 + 20 * idx)
    what = f"coef({rows},{c},G{G},ppg{ppg},slope{slope},acc{acc})"
    run_coef(E, D, rows, c, G, ppg, slope, far, acc, room, COEF_PPG[ppg], null=1 if G == 8 else None, what=what)
    if idx % 3 == 0:
        first = "bwd_fold+finalize" if ppg > 2048 else "bwd_finalize"
        run_coef(E, D, rows, c, G, ppg, slope, far, acc, room, (first, "bwd_apply"), split=True, what=what + " split")


COEF_EXTRA = [  # (rows, C, G, ppg, slope, accumulate, room, path): what the rotation above may leave out
    (1000, 36, 2, 5, 0.01, 1, 0, "bwd_fused"),            # accumulate with 8 row chunks: dgamma / dbeta added exactly once
    (300, 64, 8, 256, 0.0, 1, 0, "bwd_fused"),            # the most partials the one launch takes, 8 groups, 3 chunks
    (300, 32, 8, 257, 0.01, 1, 0, "bwd_finalize+apply"),  # one partial more: two launches
    (129, 12, 8, 2049, 1.0, 1, 64, "bwd_fold+finalize+apply"),
    (300, 32, 2, 2049, 0.01, 0, 63, "bwd_finalize+apply"),  # no room for the fold: unfolded, and still right
    (1000, 260, 1, 65, 0.0, 0, 0, "bwd_fused"),
    # accumulate over hundreds of row chunks of one channel slice.  A kernel in which every chunk adds its sums shows only if some chunk
    # reads the destination after another wrote it; blocks that run at the same time all read the old value and store the same new one.
    # With 313 (63 x 2) chunks some always run late.
    (40000, 4, 1, 256, 0.01, 1, 0, "bwd_fused"),
    (8000, 12, 2, 64, 0.0, 1, 0, "bwd_fused"),
]


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("case", COEF_EXTRA, ids=lambda c: f"{c[0]}x{c[1]}G{c[2]}p{c[3]}")
def test_coef_bwd_extra(E, case, far):
    rows, c, G, ppg, slope, acc, room, expect = case
    D = coef_data(rows, c, G, ppg, slope, far, 9900 + rows + c)
    what = f"coef({rows},{c},G{G},ppg{ppg},slope{slope},acc{acc},room{room})"
    run_coef(E, D, rows, c, G, ppg, slope, far, acc, room, expect, what=what)
    first = "bwd_fold+finalize" if "fold" in expect else "bwd_finalize"
    run_coef(E, D, rows, c, G, ppg, slope, far, acc, room, (first, "bwd_apply"), split=True, what=what + " split")


SSA = [(4, 1), (4, 255), (4, 256), (4, 257), (4, 5000), (12, 1), (12, 85), (12, 86), (12, 1667), (64, 1), (64, 16), (64, 17), (64, 313)]


@pytest.mark.parametrize("far", REGIMES)
@pytest.mark.parametrize("c,rows", SSA)
def test_scale_shift_act(E, c, rows, far):
    """rows C / 4 = 1, 255, 256, 257 quads and counts past one grid stride (a launch has about a quarter as many threads as quads)."""
    for slope in (0.01, 0.0, 1.0):
        what = f"scale_shift_act({rows},{c},slope{slope},{'far' if far else 'usual'})"
        D = coef_data(rows, c, 1, 1, slope, far, 9500 + rows + c)
        y, a, b = D["y"], D["a32"], D["b32"]
        yd, ad, bd, out = E.inp(y), E.inp(a), E.inp(b), E.out((rows, c))
        E.L.call("movae_scale_shift_act", yd.data_ptr(), ad.data_ptr(), bd.data_ptr(), out.ptr(), rows, c, slope, E.st())
        assert E.path() == "scale_shift_act"
        E.done(what)
        z = y.double() * a.double() + b.double()
        # one fma: half an ulp of z; then the slope's product.  The far-mean loss is in the operands (|y a| and |b| against |z|), not here
        check("ssa.out", out.t, torch.where(z > 0, z, z * slope), z.abs(), what, None if far or rows <= 2 else FWD_CEIL)


def test_coef_refusals(E):
    """C % 4 != 0 or an operand off a 16-byte boundary: the three 4-wide-only entry points return an error and write nothing."""
    for c, off in ((6, 0), (8, 1)):
        rows, G, ppg = 130, 2, 3
        D = coef_data(rows, c, G, ppg, 0.01, False, 9700 + c)
        for name in ("movae_scale_shift_act", "movae_bn_bwd_apply", "movae_bn_bwd_finalize_apply"):
            yd, dd, gd = E.inp(D["y"], off), E.inp(D["dout"]), E.inp(D["gamma"])
            md, rd, ad, bd, pd = E.inp(D["m32"]), E.inp(D["r32"]), E.inp(D["a32"]), E.inp(D["b32"]), E.inp(D["part"])
            dy, coef, out = E.out((G, rows, c)), E.out((G, 3, c), torch.ones(G, 3, c)), E.out((rows, c), off=off)
            slots = [[E.out((c,)) for _ in range(G)] for _ in range(2)]
            with pytest.raises(RuntimeError):
                if name == "movae_scale_shift_act":
                    E.L.call(name, yd.data_ptr(), ad.data_ptr(), bd.data_ptr(), out.ptr(), rows, c, 0.01, E.st())
                elif name == "movae_bn_bwd_apply":
                    E.L.call(name, dd.data_ptr(), yd.data_ptr(), ad.data_ptr(), bd.data_ptr(), 0.01, coef.ptr(), dy.ptr(), G, rows, c, E.st())
                else:
                    E.L.call(name, pd.data_ptr(), pd.numel(), ppg, G, rows, c, gd.data_ptr(), md.data_ptr(), rd.data_ptr(), ptr_array(slots[0]),
                             ptr_array(slots[1]), coef.ptr(), 0, dd.data_ptr(), yd.data_ptr(), ad.data_ptr(), bd.data_ptr(), 0.01, dy.ptr(), E.st())
            E.done(f"{name} refusal (C={c}, off={off})", written=False)
