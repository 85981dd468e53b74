"""bf16-operand attention (csrc/attention.hip: attn_*_bf_k; include/movae.h: movae_set_compute_dtype; `--dtype bf16`).

The contract: every MFMA operand -- q and k after RoPE, v, dO, the probabilities after the dropout scaling, and dS with its 1/sqrt(hd)
-- is rounded to bf16 (RNE); accumulation, the logits' scale, the running max, the row sum (of the UNROUNDED probabilities), lse,
delta, dP - delta and the rotation back of dq / dk stay fp32.  `_emulated` below is that arithmetic on the CPU (float64 everywhere but
the rounding points) and is printed next to the kernel's error as the yardstick: its own error against float64 is 2.4e-3 .. 4.6e-3 on
out / dq / dk / dv for these shapes and for N = 256, hd = 64, with and without RoPE, so the bound

    1e-4 < rel-L2 error against float64 < 1e-2

(tests/test_hip_bf16.py's op-level bound) holds for the reference arithmetic with a factor >= 2 to spare, and its lower end shows that
the bf16 instances really ran (the fp32 instances sit near 3e-7).  GPU only."""
import ast
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, meta_of

pytestmark = pytest.mark.gpu
LO, HI = 1e-4, 1e-2


@pytest.fixture()
def bf16(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    prev = L.set_compute_dtype("bf16")
    yield L
    L.set_compute_dtype(prev)


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def _bf(t):
    return t.float().to(torch.bfloat16).double()


def _rope_ref(n, hd, dtype, base=10000.0):
    inv_freq = 1.0 / (base ** (torch.arange(0, hd, 2).float() / hd))  # the buffer is float32 in every precision
    freqs = torch.outer(torch.arange(n, dtype=torch.float32), inv_freq)
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def _attn_ref(qkv, heads, rope, dtype):
    """AttentionWithRoPE.forward without its two linears (restated from tests/test_sphere_encoder_vit.py) in `dtype`."""
    B, N, c3 = qkv.shape
    C = c3 // 3
    hd = C // heads
    q, k, v = qkv.to(dtype).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    if rope:
        cos, sin = _rope_ref(N, hd, dtype)

        def rotate(u):
            u1, u2 = u[..., 0::2], u[..., 1::2]
            return torch.stack([u1 * cos - u2 * sin, u1 * sin + u2 * cos], dim=-1).flatten(-2)

        q, k = rotate(q), rotate(k)
    attn = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, N, C)


def _emulated(q, k, v, do, rope=False, causal=False, keep=None, p=0.0):
    """The bf16 instances' arithmetic on [B, heads, L, hd] tensors: (out, dq, dk, dv), float64 except at the rounding points."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    n, hd = q.shape[-2:]
    cos, sin = _rope_ref(n, hd, torch.float64) if rope else (None, None)

    def rotate(u, sign=1.0):  # sign -1: the transpose rotation
        if not rope:
            return u
        u1, u2 = u[..., 0::2], u[..., 1::2]
        return torch.stack([u1 * cos - sign * u2 * sin, sign * u1 * sin + u2 * cos], dim=-1).flatten(-2)

    scale = 1.0 / math.sqrt(hd)
    qb, kb, vb, gb = _bf(rotate(q)), _bf(rotate(k)), _bf(v), _bf(do)
    s = (qb @ kb.transpose(-2, -1)) * scale
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(n, n, dtype=torch.bool)), float("-inf"))
    e = (s - s.amax(-1, keepdim=True)).exp()
    row = e.sum(-1, keepdim=True)  # the unrounded probabilities
    kp = 1.0 if keep is None else keep.reshape(s.shape).double() / (1.0 - p)
    out = (_bf(e * kp) @ vb) / row
    pn = e / row  # the backward's exp(s - lse)
    dv = _bf(pn * kp).transpose(-2, -1) @ gb
    dp = (gb @ vb.transpose(-2, -1)) * kp
    delta = (do * out).sum(-1, keepdim=True)
    ds = _bf(pn * (dp - delta) * scale)
    return out, rotate(ds @ kb, -1.0), rotate(ds.transpose(-2, -1) @ qb, -1.0), dv


def _heads_of(qkv, heads):
    """packed [B, L, 3C] -> q, k, v [B, heads, L, hd]"""
    B, n, c3 = qkv.shape
    return qkv.reshape(B, n, 3, heads, c3 // 3 // heads).permute(2, 0, 3, 1, 4)


def _packed(dq, dk, dv):
    """[B, heads, L, hd] x 3 -> [B, L, 3C]"""
    return torch.cat([t.transpose(1, 2).flatten(2) for t in (dq, dk, dv)], dim=-1)


def _run_bidir(qkv, cot, heads, rope, dev):
    from movae_amd import ops

    L_, hd = qkv.shape[1], qkv.shape[2] // 3 // heads
    xd = qkv.to(dev).requires_grad_(True)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    cs = ops.rope_tables(L_, inv_freq, dev) if rope else (None, None)
    o = ops.attention(xd, heads, *cs)
    return o.detach(), torch.autograd.grad(o, xd, cot.to(dev))[0]


def _check(name, got, yard, truth, lo=LO, hi=HI):
    e, ey = _rel(got, truth), _rel(yard, truth)
    print(f"{name}: rel-L2 against float64: kernel {e:.3e}, CPU composition with the same rounding points {ey:.3e}")
    assert lo < e < hi, (name, e, ey)


# ---- 1. the kernels against float64 -------------------------------------------------------------------------------------------
# one tile, exact and ragged 16-row tiles, a ragged 32-key step, more than one block of query tiles; head dims of every instance
BIDIR_CASES = [(3, 15, 16), (1, 16, 64), (3, 17, 64), (3, 40, 24), (1, 40, 6), (1, 33, 32), (2, 70, 64)]


def _bidir_case(heads, L_, hd, rope):
    B, C = 2, heads * hd
    g = torch.Generator().manual_seed(1000 * heads + 10 * L_ + hd)
    qkv = torch.randn(B, L_, 3 * C, generator=g)
    cot = torch.randn(B, L_, C, generator=g)
    x = qkv.double().requires_grad_(True)
    o = _attn_ref(x, heads, rope, torch.float64)
    truth = (o.detach(), torch.autograd.grad(o, x, cot.double())[0])
    eo, edq, edk, edv = _emulated(*_heads_of(qkv, heads), cot.reshape(B, L_, heads, hd).transpose(1, 2), rope=rope)
    return qkv, cot, truth, (eo.transpose(1, 2).flatten(2), _packed(edq, edk, edv))


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("heads,L_,hd", BIDIR_CASES)
def test_bf16_attention_against_float64(heads, L_, hd, rope, bf16, gpu_device):
    C = heads * hd
    qkv, cot, truth, yard = _bidir_case(heads, L_, hd, rope)
    o, d = _run_bidir(qkv, cot, heads, rope, gpu_device)
    tag = f"bf16 attn h={heads} L={L_} hd={hd} rope={rope}"
    _check(tag + " out", o, yard[0], truth[0])
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        _check(f"{tag} {nm}", d[..., sl], yard[1][..., sl], truth[1][..., sl])


@pytest.mark.parametrize("rope", [False, True])
def test_bf16_attention_single_key(rope, bf16, gpu_device):
    """L = 1: the softmax is constant, out = v and dv = dO up to their rounding, and dq = dk = 0 exactly in float64."""
    heads, L_, hd = 1, 1, 2
    qkv, cot, truth, yard = _bidir_case(heads, L_, hd, rope)
    o, d = _run_bidir(qkv, cot, heads, rope, gpu_device)
    _check(f"bf16 attn L=1 rope={rope} out", o, yard[0], truth[0])
    _check(f"bf16 attn L=1 rope={rope} dv", d[..., 2 * hd:], yard[1][..., 2 * hd:], truth[1][..., 2 * hd:])
    assert float(truth[1][..., :2 * hd].abs().max()) == 0.0
    lim = 1e-2 * float(truth[1].abs().max())
    for i, nm in enumerate(("dq", "dk")):
        e = float(d[..., i * hd:(i + 1) * hd].abs().max())
        print(f"bf16 attn L=1 rope={rope} {nm}: |max| {e:.3e} (truth 0, limit {lim:.3e})")
        assert e <= lim, (nm, e)


# ---- 2. exact key / query mapping -----------------------------------------------------------------------------------------------
def test_bf16_attention_one_hot_mapping_is_exact(bf16, gpu_device):
    """P is exactly one-hot at j = pi(i) (logit 512 there, 0 elsewhere): out[i] = v[pi(i)], dv[j] = dO[pi^-1(j)], dq = dk = 0, bit for
    bit -- a permuted k order inside a 32-deep MFMA step, which random data within 1e-2 can hide, breaks every row."""
    B, heads, L_, hd = 1, 2, 40, 64
    C = heads * hd
    pis = [torch.tensor([(7 * i + 3) % L_ for i in range(L_)]), torch.tensor([(11 * i + 5) % L_ for i in range(L_)])]
    qkv = torch.zeros(B, L_, 3, heads, hd)
    cot = torch.zeros(B, L_, heads, hd)
    i_, d_ = torch.arange(L_)[:, None], torch.arange(hd)[None, :]
    for h, pi in enumerate(pis):
        assert sorted(pi.tolist()) == list(range(L_)) and not torch.equal(pi[pi], torch.arange(L_)), "an asymmetric permutation"
        qkv[0, torch.arange(L_), 0, h, pi] = 64.0  # q[i] = 64 e_pi(i)
        qkv[0, torch.arange(L_), 1, h, torch.arange(L_)] = 64.0  # k[j] = 64 e_j
        qkv[0, :, 2, h] = ((37 * i_ + 11 * d_ + 5 * h) % 257 - 128).float()
        cot[0, :, h] = ((53 * i_ + 29 * d_ + 17 * h + 101) % 257 - 128).float()
    assert not torch.equal(pis[0], pis[1])
    v = qkv[0, :, 2].clone()  # [L, heads, hd]
    o, d = _run_bidir(qkv.reshape(B, L_, 3 * C), cot.reshape(B, L_, C), heads, False, gpu_device)
    o, d = o.cpu().reshape(L_, heads, hd), d.cpu().reshape(L_, 3, heads, hd)
    for h, pi in enumerate(pis):
        inv = torch.empty_like(pi)
        inv[pi] = torch.arange(L_)
        assert torch.equal(o[:, h], v[pi, h]), f"head {h}: out[i] != v[pi(i)]"
        assert torch.equal(d[:, 2, h], cot[0, inv, h]), f"head {h}: dv[j] != dO[pi^-1(j)]"
    assert float(d[:, :2].abs().max()) == 0.0, "dq / dk are not exactly zero"


# ---- 3. causal ----------------------------------------------------------------------------------------------------------------------
def _causal_ref(q, k, v, heads, keep=None, p=0.0):
    """CausalAttention2d.forward between the projections in float64 (restated from tests/test_pixelsnail.py): q, k, v [B, L, proj]
    (head h at channels h*hd ..) -> [B, L, proj] with (h, d) at channel d*heads + h."""
    B, n, proj = q.shape
    hd = proj // heads

    def split(t):
        return t.reshape(B, n, heads, hd).permute(0, 2, 1, 3)

    attn = torch.matmul(split(q), split(k).transpose(-2, -1)) / math.sqrt(hd)
    attn = attn.masked_fill(~torch.tril(torch.ones(n, n, dtype=torch.bool)), float("-inf")).softmax(-1)
    if keep is not None:
        attn = attn * keep.reshape(B, heads, n, n).to(attn.dtype) / (1.0 - p)
    return torch.matmul(attn, split(v)).permute(0, 2, 3, 1).reshape(B, n, proj)


def _run_causal(q, k, v, do, heads, dev, p, seed, draw):
    from movae_amd import ops

    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    o = ops.causal_attention(qd, kd, vd, heads, p, seed, draw)
    return (o.detach(),) + torch.autograd.grad(o, (qd, kd, vd), do.to(dev))


def _causal_inputs(B, heads, n, hd):
    g = torch.Generator().manual_seed(7 * n + hd)
    return tuple(torch.randn(B, n, heads * hd, generator=g) for _ in range(4))


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("hd", [16, 64])
def test_bf16_causal_attention_against_float64(hd, p, bf16, gpu_device):
    from movae_amd import ops

    B, heads, n, seed, draw = 2, 2, 40, 1234, 5
    q, k, v, do = _causal_inputs(B, heads, n, hd)
    keep = ops.causal_attention_dropout_mask(B * heads, n, p, seed, draw, gpu_device).cpu() if p > 0 else None
    if keep is not None:
        assert 0.6 < float(keep.float().mean()) < 0.9
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o = _causal_ref(qr, kr, vr, heads, keep, p)
    truth = (o.detach(),) + torch.autograd.grad(o, (qr, kr, vr), do.double())

    def split(t):
        return t.reshape(B, n, heads, hd).permute(0, 2, 1, 3)

    eo, edq, edk, edv = _emulated(split(q), split(k), split(v), do.reshape(B, n, hd, heads).permute(0, 3, 1, 2), causal=True, keep=keep, p=p)
    yard = (eo.permute(0, 2, 3, 1).reshape(B, n, heads * hd),) + tuple(t.transpose(1, 2).flatten(2) for t in (edq, edk, edv))
    got = _run_causal(q, k, v, do, heads, gpu_device, p, seed, draw)
    for nm, a, y, t in zip(("out", "dq", "dk", "dv"), got, yard, truth):
        _check(f"bf16 causal attn hd={hd} p={p} {nm}", a, y, t)


# ---- 4. the modes do not leak ---------------------------------------------------------------------------------------------------
def test_fp32_attention_is_unchanged_by_a_visit_to_bf16_and_reruns_are_identical(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    heads, L_, hd = 3, 40, 24
    qkv, cot, _, _ = _bidir_case(heads, L_, hd, True)
    cq = _causal_inputs(2, 2, 40, 16)

    def both():
        return _run_bidir(qkv, cot, heads, True, gpu_device) + _run_causal(*cq, 2, gpu_device, 0.25, 1234, 5)

    assert L.compute_dtype() == "fp32"
    before = both()
    prev = L.set_compute_dtype("bf16")
    try:
        assert L.compute_dtype() == "bf16"
        b1, b2 = both(), both()
    finally:
        L.set_compute_dtype(prev)
    after = both()
    for i, (x, y, z, w) in enumerate(zip(before, after, b1, b2)):
        assert torch.equal(x, y), f"tensor {i}: fp32 mode changed by a visit to bf16"
        assert torch.equal(z, w), f"tensor {i}: a bf16 rerun is not bit-identical"
        assert not torch.equal(x, z), f"tensor {i}: bf16 mode gave the fp32 result"


@pytest.mark.parametrize("fwd,bwd", [("fp32", "bf16"), ("bf16", "fp32")])
def test_backward_under_the_other_dtype_is_refused(fwd, bwd, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import ops

    x = torch.randn(1, 8, 3 * 16, device=gpu_device, requires_grad=True)
    q, k, v = (torch.randn(1, 8, 16, device=gpu_device, requires_grad=True) for _ in range(3))
    prev = L.set_compute_dtype(fwd)
    try:
        o, oc = ops.attention(x, 1), ops.causal_attention(q, k, v, 2)
        L.set_compute_dtype(bwd)
        for out, leaves in ((o, (x,)), (oc, (q, k, v))):
            with pytest.raises(RuntimeError) as ei:
                torch.autograd.grad(out, leaves, torch.ones_like(out), retain_graph=True)
            assert fwd in str(ei.value) and bwd in str(ei.value)
        L.set_compute_dtype(fwd)
        torch.autograd.grad(o, (x,), torch.ones_like(o))  # and the matching dtype goes through
    finally:
        L.set_compute_dtype(prev)


# ---- 5. model level -----------------------------------------------------------------------------------------------------------------
def test_bf16_vit_sum_step_against_the_fixture(bf16, gpu_device):
    """One `--agg sum` step of sphere_encoder_vit_tiny under bf16 mode against the fp32 fixture: at this size only attention changes
    arithmetic (the token linears are below the 128x128 tiles).  test_hip_bf16.py's step-level bounds: every loss within 2e-2 relative,
    the gradient over ALL parameters within 3e-2 rel-L2 of the sum of the fixture's Jacobian rows (the total loss adds its three
    objectives with weight 1 each: the lambdas are inside them)."""
    from movae_amd import train
    from movae_amd.models import SphereEncoderViT

    fx = load_golden("sphere_encoder_vit_tiny")
    m = meta_of(fx)
    torch.manual_seed(int(m["seed"]))
    net = SphereEncoderViT(use_perceptual=False, **ast.literal_eval(m["kwargs"]))
    net.load_state_dict({k[4:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sdw.")})
    net = net.to(gpu_device).train()
    net.noise_override = {"u": torch.from_numpy(fx["u"]).to(gpu_device), "e": torch.from_numpy(fx["e"]).to(gpu_device)}
    comps = [f[5:] for f in fx.files if f.startswith("loss.") and f != "loss.total_loss"]
    np.testing.assert_allclose(sum(float(fx["loss." + k]) for k in comps), float(fx["loss.total_loss"]), rtol=1e-6)
    x = torch.from_numpy(fx["x"]).to(gpu_device)
    ld = train.forward_backward(net, x, torch.optim.SGD(net.parameters(), lr=0.0), "sum")[0]
    for k, v in ld.items():
        got, want = v.detach().item(), float(fx["loss." + k])
        print(f"[bf16 vit sum step] loss {k}: {got:.6g} (fp32 fixture {want:.6g}, rel {abs(got - want) / abs(want):.2e})")
        np.testing.assert_allclose(got, want, rtol=2e-2, err_msg=f"loss {k}")
    got, want = [], []
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        got.append(p.grad.detach().double().cpu().flatten())
        want.append(sum(torch.from_numpy(fx[f"gloss.{i}.{n}"]).double() for i in range(len(comps))).flatten())
    e = _rel(torch.cat(got), torch.cat(want))
    print(f"[bf16 vit sum step] gradient over all parameters: rel-L2 {e:.3e}")
    assert e < 3e-2, e
