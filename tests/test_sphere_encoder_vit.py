"""The ViT Sphere Encoder (models/sphere_encoder_vit.py; csrc/attention.hip's bidirectional RoPE form, csrc/vit.hip) against golden vectors
recorded from the reference's own class (tests/golden/generate_sphere_encoder_vit.py) and against float64 restatements of its
expressions: constructor, init replay and the builder on the CPU; every kernel pair alone, the model's forward / losses / Jacobian rows /
step / eval / sampling, the aggregated step, the walker fallback, the in-kernel noise and graph replay on the GPU.

Kernel bound (as in test_sphere_encoder.py): the error against float64 may be MARGIN x the error of the float32 torch-CPU composition of
the same expression on the same inputs, plus a floor of FLOOR_ULP fp32 ulps of the output's largest magnitude."""
import ast
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, meta_of

TAGS = ["sphere_encoder_vit_tiny", "sphere_encoder_vit_tiny_mix"]
EPS32 = 2.0 ** -23
MARGIN, FLOOR_ULP = 4, 8


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def T(a):
    return torch.from_numpy(np.asarray(a))


def build(fx):
    import movae_amd  # noqa: F401
    from movae_amd.models import SphereEncoderViT

    m = meta_of(fx)
    torch.manual_seed(int(m["seed"]))
    return SphereEncoderViT(use_perceptual=False, **ast.literal_eval(m["kwargs"])), m


def assert_close(got, want, what, rtol=1e-3, atol=3e-6):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol * max(1.0, float(np.abs(want).max())), err_msg=what)


def _err(a, truth):
    return float((a.detach().double().cpu() - truth.detach()).abs().max())


def _bound(name, got, yard, truth, whole=None):
    """The kernel bound of the module docstring; prints the figures before it asserts.  `whole`: the float64 value of the whole tensor
    the op returns when `truth` is a slice of it -- the floor is taken from the output's largest magnitude, not the slice's."""
    t = truth.detach()
    e_ref, e_got = _err(yard, t), _err(got, t)
    mag = float((t if whole is None else whole.detach()).abs().max()) if t.numel() else 0.0
    lim = MARGIN * e_ref + FLOOR_ULP * EPS32 * mag
    print(f"{name}: kernel {e_got:.3g} reference-fp32 {e_ref:.3g} |max| {mag:.3g} ratio-to-bound {e_got / lim if lim else 0:.3g}")
    assert e_got <= lim, (name, e_got, e_ref, mag)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_are_the_references():
    import movae_amd  # noqa: F401
    from movae_amd.models import SphereEncoderViT

    got = {k: p.default for k, p in inspect.signature(SphereEncoderViT.__init__).parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == dict(img_size=32, patch_size=2, in_channels=3, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0, mixer_depth=2,
                       mixer_tokens_mlp_dim=256, mixer_channels_mlp_dim=2048, latent_channels=8, num_classes=0, sigma_max_angle_deg=80.0,
                       sigma_mix_prob=0.0, sigma_mix_angle_min_deg=None, sigma_mix_angle_max_deg=None, lambda_pix_recon=1.0,
                       lambda_pix_con=0.5, lambda_lat_con=0.1, pix_recon_smooth_l1_weight=1.0, pix_recon_perceptual_weight=1.0,
                       pix_con_smooth_l1_weight=0.5, pix_con_perceptual_weight=0.5, use_perceptual=True, dropout=0.0, device=None)
    assert list(got)[:3] == ["img_size", "patch_size", "in_channels"]


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_order_and_init_replay(tag):
    fx = load_golden(tag)
    net, m = build(fx)
    sd = net.state_dict()
    want = [f[4:] for f in fx.files if f.startswith("sd0.")]
    assert list(sd.keys()) == want
    assert "pos_embed_enc.pe" in want and "pos_embed_dec.pe" in want and "blocks_enc.0.attn.rotary.inv_freq" in want
    for k in want:
        assert sd[k].shape == fx["sd0." + k].shape and np.array_equal(sd[k].numpy(), fx["sd0." + k]), f"init replay {k}"
    assert net.features is None and list(net.objectives.keys()) == [str(s) for s in fx["objectives"]] == ["pix_recon", "pix_con", "lat_con"]
    assert net.graph_safe and net._jacobian_from_loss_op
    assert net.L == net.num_patches * 4 and net.radius == math.sqrt(net.L)
    assert net.sigma_max == math.tan(math.radians(net.sigma_max_angle_deg))


def test_perceptual_and_dropout_are_refused():
    import movae_amd  # noqa: F401
    from movae_amd.models import SphereEncoderViT

    kw = dict(img_size=8, embed_dim=16, depth=1, num_heads=1, mixer_depth=1, latent_channels=2)
    with pytest.raises(NotImplementedError, match="VGG16"):
        SphereEncoderViT(**kw)  # use_perceptual defaults to True, as in the reference
    with pytest.raises(NotImplementedError, match="dropout"):
        SphereEncoderViT(use_perceptual=False, dropout=0.1, **kw)


def test_builder_reads_the_flags_and_checks_divisibility():
    import movae_amd  # noqa: F401
    from movae_amd.models import build_sphere_encoder_vit

    a = Args(latent_dim=64, vit_embed_dim=16, vit_depth=1, vit_num_heads=2, vit_mixer_depth=1, sigma_mix_prob=0.1, lambda_pix_con=0.3,
             sigma_max_angle_deg=70.0, num_classes=0)
    net = build_sphere_encoder_vit(8, 3, a, None)
    assert (net.patch_size, net.num_patches, net.L) == (2, 16, 64) and net.latent_proj_enc.out_features == 4
    assert (net.sigma_mix_prob, net.lambda_pix_con, net.sigma_max_angle_deg, net.lambda_pix_recon, net.lambda_lat_con) == (0.1, 0.3, 70.0, 1.0, 0.1)
    assert len(net.blocks_enc) == len(net.blocks_dec) == 1 and len(net.mixer_enc.blocks) == 1 and net.blocks_enc[0].attn.num_heads == 2
    assert net.use_perceptual is False and net.img_size == 8 and net.in_channels == 3
    big = build_sphere_encoder_vit(64, 3, Args(latent_dim=128, vit_embed_dim=16, vit_depth=0, vit_num_heads=2, vit_mixer_depth=0), None)
    assert big.patch_size == 8 and big.num_patches == 64  # patch 8 above 32 pixels
    assert build_sphere_encoder_vit(8, 3, Args(latent_dim=32, patch_size=4, vit_embed_dim=16, vit_depth=0, vit_num_heads=2, vit_mixer_depth=0),
                                    None).num_patches == 4
    with pytest.raises(ValueError, match="divisible"):
        build_sphere_encoder_vit(8, 3, Args(latent_dim=65, vit_embed_dim=16, vit_depth=1, vit_num_heads=2, vit_mixer_depth=1), None)
    with pytest.raises(NotImplementedError):
        build_sphere_encoder_vit(8, 3, a, None, use_perceptual=True)


# ---- attention -------------------------------------------------------------------------------------------------------------------
def _rope_ref(n, hd, dtype, base=10000.0):
    inv_freq = 1.0 / (base ** (torch.arange(0, hd, 2).float() / hd))  # the buffer is float32 in every precision
    freqs = torch.outer(torch.arange(n, dtype=torch.float32), inv_freq)
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def _attn_ref(qkv, heads, rope, dtype):
    """AttentionWithRoPE.forward without its two linears (sphere_encoder_vit.py:157-166, apply_rotary_pos_emb :71-89) in `dtype`."""
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


# every padded head dim (2, 6 -> 8; 16; 24 -> 32; 64), one tile / exact tile / ragged tiles / several blocks' worth, one and three heads
ATTN_CASES = [(h, L, hd) for h, L, hd in
              [(1, 1, 2), (3, 1, 6), (1, 15, 6), (3, 15, 16), (1, 16, 2), (3, 16, 6), (1, 16, 16), (3, 16, 24), (1, 16, 64), (1, 17, 6),
               (3, 17, 16), (1, 17, 24), (3, 17, 64), (3, 40, 2), (1, 40, 6), (3, 40, 16), (3, 40, 24), (1, 40, 64), (3, 15, 64), (1, 1, 64)]]


@pytest.mark.gpu
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("heads,L,hd", ATTN_CASES)
def test_attention_against_float64(heads, L, hd, rope, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B, C = 2, heads * hd
    g = torch.Generator().manual_seed(1000 * heads + 10 * L + hd)
    qkv = torch.randn(B, L, 3 * C, generator=g)
    cot = torch.randn(B, L, C, generator=g)

    def run(dtype):
        x = qkv.to(dtype).requires_grad_(True)
        o = _attn_ref(x, heads, rope, dtype)
        return o.detach(), torch.autograd.grad(o, x, cot.to(dtype))[0]

    truth, yard = run(torch.float64), run(torch.float32)
    xd = qkv.to(gpu_device).requires_grad_(True)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    cs = ops.rope_tables(L, inv_freq, gpu_device) if rope else (None, None)
    o = ops.attention(xd, heads, *cs)
    assert o.shape == (B, L, C)
    d1 = torch.autograd.grad(o, xd, cot.to(gpu_device), retain_graph=True)[0]
    d2 = torch.autograd.grad(o, xd, cot.to(gpu_device))[0]
    assert torch.equal(d1, d2), "dqkv: a rerun is not bit-identical"
    assert torch.equal(o, ops.attention(xd, heads, *cs)), "out: a rerun is not bit-identical"
    tag = f"attn h={heads} L={L} hd={hd} rope={rope}"
    _bound(tag + " out", o, yard[0], truth[0])
    # The backward's output is ONE packed [B, L, 3C] tensor; its dq / dk / dv thirds are reported apart, each against its own fp32
    # yardstick, with the floor from the packed tensor's magnitude.  A third can be identically zero: with one key the softmax is
    # constant, so dq = dk = 0, which torch forms exactly (g - 1 * g) while the kernel subtracts two differently ordered fp32 sums of the
    # same products, dP - delta, and keeps a rounding residue (1.8e-7 measured at L = 1, hd = 6, where |dP| is about 2: one ulp of it).
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        _bound(f"{tag} {nm}", d1[..., sl], yard[1][..., sl], truth[1][..., sl], whole=truth[1])


@pytest.mark.gpu
def test_attention_layout_and_non_causality(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B, heads, L, hd = 2, 3, 17, 6
    C = heads * hd
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, L, 3 * C, generator=g)
    # constant-valued heads: v of head h is h + 1 everywhere, so the output of head h is h + 1 and sits at channels h*hd .. h*hd+hd-1
    qkv[..., 2 * C:] = (torch.arange(C) // hd + 1).float()
    o = ops.attention(qkv.to(gpu_device), heads).cpu()
    want = (torch.arange(C) // hd + 1).float().expand(B, L, C)
    np.testing.assert_allclose(o.numpy(), want.numpy(), rtol=1e-6)
    # bidirectional: the LAST key / value reaches the FIRST query
    a = torch.randn(B, L, 3 * C, generator=g)
    b = a.clone()
    b[:, -1, C:] += 1.0
    oa, ob = ops.attention(a.to(gpu_device), heads), ops.attention(b.to(gpu_device), heads)
    assert float((oa[:, 0] - ob[:, 0]).abs().max()) > 1e-3
    assert torch.equal(ops.attention(a.to(gpu_device), heads), oa)


@pytest.mark.gpu
def test_attention_refusals(gpu_device):
    import ctypes as C

    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import ops

    lib = L.load()
    buf = torch.zeros(1 << 16, device=gpu_device)
    p, st = buf.data_ptr(), L.stream_ptr(gpu_device)

    def fwd(hd, pdrop, rope):
        r = p if rope else None
        return lib.movae_attn_fwd(p, p, p, 3 * hd, r, r, p, p, 1, 1, 4, hd, C.c_float(pdrop), st)

    assert fwd(4, 0.0, True) == 0
    assert fwd(5, 0.0, False) == 0
    assert fwd(5, 0.0, True) == -1 and b"even" in lib.movae_last_error()
    assert fwd(4, 0.1, False) == -1 and b"dropout" in lib.movae_last_error()
    assert fwd(65, 0.0, False) == -1 and b"64" in lib.movae_last_error()
    ws = torch.zeros(lib.movae_attn_ws_bytes(1, 1, 4), dtype=torch.uint8, device=gpu_device)
    assert lib.movae_attn_bwd(p, p, p, 12, None, None, p, p, p, p, p, p, 1, 1, 4, 4, C.c_float(0.5), ws.data_ptr(), ws.numel(), st) == -1
    assert b"dropout" in lib.movae_last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.attention(torch.zeros(1, 4, 10, device=gpu_device), 1)


@pytest.mark.gpu
def test_causal_entry_points_are_bit_identical_to_the_parent(gpu_device):
    """movae_causal_attn_fwd / _bwd on two fixed inputs (one with dropout) against the outputs recorded from the parent commit's library
    (tests/golden/causal_attn_parent.npz)."""
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import ops

    fx = load_golden("causal_attn_parent")
    for tag in ("a", "b"):
        B, heads, n, hd, seed, draw = (int(v) for v in fx[tag + ".cfg"])
        p = float(fx[tag + ".p"])
        q, k, v, do = (T(fx[f"{tag}.{nm}"]).to(gpu_device) for nm in ("q", "k", "v", "dout"))
        o = torch.empty_like(q)
        lse = torch.empty(B * heads, n, device=gpu_device)
        L.call("movae_causal_attn_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), heads * hd, o.data_ptr(), lse.data_ptr(), B, heads, n, hd, p,
               seed, draw, L.stream_ptr(gpu_device))
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        ws = ops._ws_at_least(gpu_device, L.load().movae_causal_attn_ws_bytes(B, heads, n))
        L.call("movae_causal_attn_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), heads * hd, o.data_ptr(), do.data_ptr(), lse.data_ptr(),
               dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, heads, n, hd, p, seed, draw, ws.data_ptr(), ws.numel(), L.stream_ptr(gpu_device))
        for nm, t in (("out", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert np.array_equal(t.cpu().numpy(), fx[f"{tag}.{nm}"]), f"case {tag}: {nm} differs from the parent commit's"


# ---- row norm ----------------------------------------------------------------------------------------------------------------------
def _rownorm_ref(x, w, b, pos, mode, dtype):
    x = x.to(dtype)
    if mode == "layer":
        y = F.layer_norm(x, x.shape[-1:], None, None, 1e-5)
    else:
        y = x / (x.pow(2).mean(dim=-1, keepdim=True) + 1e-6).sqrt()  # rms_norm, models/sphere_encoder.py:23-26
    if w is not None:
        y = y * w
    if b is not None:
        y = y + b
    if pos is not None:
        y = (y.reshape(-1, *pos.shape) + pos.to(dtype)).reshape(x.shape)
    return y


ROWNORM_CASES = [(rows, D) for D in (1, 5, 32, 63, 64, 65, 1024) for rows in (1, 7, 300)]
#: (weight, bias -- LayerNorm only, pos): everything, the affine alone, weight without bias, pos without affine, nothing
ROWNORM_ARGS = [(True, True, True), (True, True, False), (True, False, False), (False, False, True), (False, False, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["layer", "rms"])
@pytest.mark.parametrize("rows,D", ROWNORM_CASES)
def test_rownorm_against_float64(rows, D, mode, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    g = torch.Generator().manual_seed(rows * 2000 + D)
    x = torch.randn(rows, D, generator=g) * 1.5 + 0.4
    cot = torch.randn(rows, D, generator=g)
    period = {1: 1, 7: 7, 300: 25}[rows]
    for affine, with_b, with_pos in ROWNORM_ARGS:
        if mode == "rms" and not with_b and (affine, True, with_pos) in ROWNORM_ARGS:
            continue  # (RMSNorm has no bias: the same call as the combination with one)
        w = torch.randn(D, generator=g) if affine else None
        b = torch.randn(D, generator=g) if with_b and mode == "layer" else None
        pos = torch.randn(period, D, generator=g) if with_pos else None

        def run(dtype, dev="cpu"):
            leaves = [t.to(device=dev, dtype=dtype).requires_grad_(True) if t is not None else None for t in (x, w, b)]
            if dev == "cpu":
                y = _rownorm_ref(leaves[0], leaves[1], leaves[2], pos, mode, dtype)
            else:
                pd = pos.to(dev) if pos is not None else None
                y = ops.layer_norm(leaves[0], leaves[1], leaves[2], pos=pd) if mode == "layer" else ops.rms_norm(leaves[0], leaves[1], pos=pd)
            live = [t for t in leaves if t is not None]
            grads = torch.autograd.grad(y, live, cot.to(device=dev, dtype=dtype))
            return [y.detach()] + list(grads)

        truth, yard = run(torch.float64), run(torch.float32)
        got, again = run(torch.float32, gpu_device), run(torch.float32, gpu_device)
        names = ["out", "dx"] + (["dweight"] if w is not None else []) + (["dbias"] if b is not None else [])
        for nm, a, a2, y, t in zip(names, got, again, yard, truth):
            assert torch.equal(a, a2), f"{nm}: a rerun is not bit-identical"
            _bound(f"rownorm {mode} rows={rows} D={D} weight={affine} bias={b is not None} pos={with_pos} {nm}", a, y, t)


# ---- bias + GELU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows,c,bias", [(1, 1, True), (7, 5, True), (300, 64, True), (33, 130, False)])
def test_bias_gelu_against_float64(rows, c, bias, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    g = torch.Generator().manual_seed(rows + c)
    x = torch.randn(rows, c, generator=g) * 3.0
    x.view(-1)[:: max(1, x.numel() // 16)] = torch.linspace(-8.0, 8.0, len(x.view(-1)[:: max(1, x.numel() // 16)]))  # the erf tails
    b = torch.randn(c, generator=g) * 0.5 if bias else None
    cot = torch.randn(rows, c, generator=g)

    def run(dtype, dev="cpu"):
        leaves = [t.to(device=dev, dtype=dtype).requires_grad_(True) if t is not None else None for t in (x, b)]
        if dev == "cpu":
            y = F.gelu(leaves[0] + leaves[1] if bias else leaves[0])
        else:
            y = ops.bias_gelu(leaves[0], leaves[1])
        return [y.detach()] + list(torch.autograd.grad(y, [t for t in leaves if t is not None], cot.to(device=dev, dtype=dtype)))

    truth, yard, got, again = run(torch.float64), run(torch.float32), run(torch.float32, gpu_device), run(torch.float32, gpu_device)
    for nm, a, a2, y, t in zip(["out", "dx", "dbias"], got, again, yard, truth):
        assert torch.equal(a, a2), f"{nm}: a rerun is not bit-identical"
        _bound(f"bias_gelu rows={rows} c={c} bias={bias} {nm}", a, y, t)


# ---- unpatchify + tanh, positional add -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("p", [1, 2, 4])
def test_unpatchify_act_against_float64(p, C, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B, size = 3, 8
    h = size // p
    g = torch.Generator().manual_seed(p * 10 + C)
    x = torch.randn(B, h * h, p * p * C, generator=g) * 1.5
    cot = torch.randn(B, C, size, size, generator=g)

    def ref(dtype):
        xx = x.to(dtype).requires_grad_(True)
        y = torch.tanh(xx.reshape(B, h, h, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, size, size))  # Unpatchify.forward, then Tanh
        return y.detach(), torch.autograd.grad(y, xx, cot.to(dtype))[0]

    truth, yard = ref(torch.float64), ref(torch.float32)
    xd = x.to(gpu_device).requires_grad_(True)
    y = ops.unpatchify_act(xd, size, size, C, p)
    assert y.shape == (B, size, size, C)
    dx = torch.autograd.grad(y, xd, cot.to(gpu_device).permute(0, 2, 3, 1).contiguous())[0]
    _bound(f"unpatchify p={p} C={C} out", y.permute(0, 3, 1, 2), yard[0], truth[0])
    _bound(f"unpatchify p={p} C={C} dx", dx, yard[1], truth[1])


@pytest.mark.gpu
def test_add_rows_bcast(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    g = torch.Generator().manual_seed(3)
    x, pos = torch.randn(3, 25, 12, generator=g), torch.randn(25, 12, generator=g)
    xd = x.to(gpu_device).requires_grad_(True)
    y = ops.add_rows_bcast(xd, pos.to(gpu_device))
    assert torch.equal(y.cpu(), x + pos)
    cot = torch.randn(3, 25, 12, generator=g).to(gpu_device)
    assert torch.equal(torch.autograd.grad(y, xd, cot)[0], cot)


# ---- the model against the fixtures ------------------------------------------------------------------------------------------------
def _gpu_net(fx, dev):
    net, m = build(fx)
    net.load_state_dict({k[4:]: T(fx[k]) for k in fx.files if k.startswith("sdw.")})  # the working state (the head scaled: see the generator)
    net = net.to(dev).train()
    net.noise_override = {"u": T(fx["u"]).to(dev), "e": T(fx["e"]).to(dev)}
    return net, m


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_forward_losses_jacobian_rows_sum_step(tag, gpu_device, monkeypatch):
    fx = load_golden(tag)
    net, m = _gpu_net(fx, gpu_device)
    x = T(fx["x"]).to(gpu_device)
    out = net(x)
    assert list(out.keys()) == [f[4:] for f in fx.files if f.startswith("out.")]
    for k in out:
        assert out[k].shape == fx["out." + k].shape, k
        assert_close(out[k], fx["out." + k], k, rtol=2e-4, atol=2e-5)
    assert out["x_recon_noisy_small_sg"].data_ptr() == out["recons"].data_ptr() and not out["x_recon_noisy_small_sg"].requires_grad
    ld = net.loss_function(x, args=out)
    assert list(ld.keys()) == [f[5:] for f in fx.files if f.startswith("loss.")]
    for k, v in ld.items():
        np.testing.assert_allclose(v.item(), fx["loss." + k], rtol=2e-5, atol=1e-7, err_msg=k)
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    comp = [v for k, v in ld.items() if k != "total_loss"]
    assert len(comp) == 3
    for i, v in enumerate(comp):  # the Jacobian rows: every objective reaches every parameter
        gs = torch.autograd.grad(v, params, retain_graph=True, allow_unused=True)
        for n, p, g in zip(names, params, gs):
            assert g is not None, f"row {i} leaves {n} without a gradient"
            assert_close(g, fx[f"gloss.{i}.{n}"], f"row {i} {n}", rtol=2e-3, atol=1e-5)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    ld["total_loss"].backward()
    for n, p in zip(names, params):
        assert_close(p.grad if p.grad is not None else torch.zeros_like(p), fx["gsum." + n], "grad " + n)
    opt.step()
    sd1 = net.state_dict()
    for k in [f[4:] for f in fx.files if f.startswith("sd1.")]:
        want = fx["sd1." + k]
        noise = ("gsum." + k) in fx.files and np.abs(fx["gsum." + k]).max() < 1e-6
        np.testing.assert_allclose(sd1[k].cpu().numpy(), want, rtol=2e-4, atol=2.1e-3 if noise else 3e-5, err_msg=k)
    ld2 = net.loss_function(x, args=net(x))
    for k, v in ld2.items():
        np.testing.assert_allclose(v.item(), fx["loss2." + k], rtol=1e-3, atol=2e-6, err_msg="loss2 " + k)
    net.eval()
    with torch.no_grad():
        oe = net(x)
        le = net.loss_function(x, args=oe)
    assert list(oe.keys()) == [f[5:] for f in fx.files if f.startswith("eval.")]
    for k in ("recons", "x_recon_NOISY"):
        assert_close(oe[k], fx["eval." + k], "eval " + k, rtol=2e-3, atol=5e-3)
    for k, v in le.items():
        np.testing.assert_allclose(v.item(), fx["eval_loss." + k], rtol=5e-2, atol=1e-4, err_msg="eval " + k)
    e = T(fx["sample.e"]).to(gpu_device)
    drawn = []
    monkeypatch.setattr(torch, "randn", lambda *a, **k: drawn.append(a) or e.clone())
    xs = net.sample(2, device=gpu_device, steps=3)
    monkeypatch.undo()
    assert drawn == [(2, net.L)]  # share_noise: one draw serves all three steps
    assert_close(xs, fx["sample.x"], "sample", rtol=2e-3, atol=5e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True])
def test_aggregated_step_and_the_walker_fallback(batched, gpu_device, monkeypatch):
    """train.forward_backward with upgrad equals the combination of the fixture's Jacobian rows under the weights the aggregator reports;
    with MOVAE_BATCHED_FULL_JACOBIAN=1 the walker refuses the new ops and the sequential form gives the same gradients."""
    import movae_amd  # noqa: F401
    from movae_amd import aggregation, autojac, train

    monkeypatch.setattr(autojac, "BATCHED_FULL_JACOBIAN", batched)
    tried = []
    real = autojac._batched_pullback

    def spy(*a, **k):
        tried.append(1)
        return real(*a, **k)

    monkeypatch.setattr(autojac, "_batched_pullback", spy)
    fx = load_golden("sphere_encoder_vit_tiny")
    net, m = _gpu_net(fx, gpu_device)
    names = [n for n, _ in net.named_parameters()]
    a = Args(aggregator="upgrad", agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None)
    A = aggregation.make_aggregator(a)
    seen = {}
    A.weighting.register_forward_hook(lambda mod, inp, out: seen.update(w=out.clone()))
    x = T(fx["x"]).to(gpu_device)
    train.forward_backward(net, x, torch.optim.SGD(net.parameters(), lr=0.0), A)
    assert len(tried) == (1 if batched else 0)  # the walker was entered once and fell back (NotImplementedError), or never
    w = seen["w"].double().cpu().numpy()
    assert w.shape == (3,) and np.isfinite(w).all()
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        want = sum(w[i] * fx[f"gloss.{i}.{n}"].astype(np.float64) for i in range(3))
        assert_close(p.grad, want.astype(np.float32), f"upgrad grad {n}", rtol=2e-3, atol=1e-5)
    assert set(names) == {n for n, _ in net.named_parameters()}


@pytest.mark.gpu
def test_in_kernel_noise_after_prepare_for_graph(gpu_device):
    fx = load_golden("sphere_encoder_vit_tiny_mix")
    net, _ = _gpu_net(fx, gpu_device)
    net.noise_override = None
    net.prepare_for_graph()
    assert net.noise_on_device
    x = T(fx["x"]).to(gpu_device)
    with torch.no_grad():
        o1, o2 = net(x), net(x)
    assert not torch.equal(o1["sigma"], o2["sigma"]) and not torch.equal(o1["v_noisy"], o2["v_noisy"])
    assert torch.equal(o1["v"], o2["v"])
    for o in (o1, o2):
        for k in ("v", "v_noisy", "v_noisy_small"):
            rms = o[k].double().pow(2).mean(dim=-1).sqrt()
            np.testing.assert_allclose(rms.cpu().numpy(), net.radius, rtol=1e-4)  # spherify: rms_norm(x) * radius
    assert net._noise_state_t.tolist()[1] == 2


@pytest.mark.gpu
def test_hipgraph_replay_matches_eager_steps(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import aggregation
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    fx = load_golden("sphere_encoder_vit_tiny")
    a = Args(aggregator="upgrad", agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None,
             optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None)
    x = T(fx["x"]).to(gpu_device)
    g = torch.Generator().manual_seed(11)
    batches = [x] + [(torch.rand(x.shape, generator=g) * 2 - 1).to(gpu_device) for _ in range(2)]
    net_e, _ = _gpu_net(fx, gpu_device)
    opt_e, agg_e = make_optimizer(net_e, a, capturable=True), aggregation.make_aggregator(a)
    eager = [train_step(net_e, b, opt_e, agg_e, a)[0]["total_loss"].item() for b in batches]
    net_g, _ = _gpu_net(fx, gpu_device)
    opt_g = make_optimizer(net_g, a, capturable=True)
    gs = GraphedTrainStep(net_g, opt_g, aggregation.make_aggregator(a), a, batches[0], preserve_state=True)
    graphed = [gs.step(b)[0]["total_loss"].item() for b in batches]
    np.testing.assert_allclose(graphed[0], float(fx["loss.total_loss"]), rtol=2e-5)  # preserve_state: the first replay is step 1
    np.testing.assert_allclose(graphed, eager, rtol=2e-5)
    for (n, p), (_, q) in zip(net_e.named_parameters(), net_g.named_parameters()):
        got, want = q.detach().cpu().numpy(), p.detach().cpu().numpy()
        # Adam turns rounding noise in a near-zero gradient into a step of up to +-lr: a handful of entries may differ by a fraction of one step
        bad = np.abs(got - want) > 2e-5 + 2e-3 * np.abs(want)
        assert bad.mean() <= 1e-3 and np.abs(got - want).max() < 5e-4, f"{n}: {int(bad.sum())} of {bad.size} off"

    # in-kernel noise: successive replays of the same batch draw fresh noise and stay finite
    net_r, _ = _gpu_net(fx, gpu_device)
    net_r.noise_override = None
    opt_r = make_optimizer(net_r, a, capturable=True)
    gr = GraphedTrainStep(net_r, opt_r, aggregation.make_aggregator(a), a, x, preserve_state=True)
    assert net_r.noise_on_device
    sig, tot = [], []
    for _ in range(3):
        ld, out = gr.step(x)
        sig.append(out["sigma"].detach().clone())
        tot.append(ld["total_loss"].item())
    assert not torch.equal(sig[0], sig[1]) and not torch.equal(sig[1], sig[2]) and len(set(tot)) == 3
    assert np.isfinite(tot).all() and all(bool(torch.isfinite(p).all()) for p in net_r.parameters())
    assert net_r._noise_state_t.tolist()[1] == 3


@pytest.mark.gpu
def test_train_step_and_evaluate(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import aggregation, train

    fx = load_golden("sphere_encoder_vit_tiny_mix")
    net, _ = _gpu_net(fx, gpu_device)
    net.noise_override = None
    a = Args(aggregator="upgrad", agg_norm_eps=1e-4, agg_reg_eps=1e-4, pref_weights=None, optimizer="adam", lr=1e-3, wd=0, momentum=0.9,
             max_grad_norm=1.0)
    opt, A = train.make_optimizer(net, a), aggregation.make_aggregator(a)
    x = T(fx["x"]).to(gpu_device)
    torch.manual_seed(0)
    l1 = train.train_step(net, x, opt, A, a)[0]
    l2 = train.train_step(net, x, opt, A, a)[0]
    assert list(l1.keys()) == ["pix_recon", "pix_con", "lat_con", "total_loss"]
    assert all(np.isfinite(v.item()) for v in list(l1.values()) + list(l2.values())) and l1["pix_con"].item() != l2["pix_con"].item()
    meters = train.evaluate(net, [(x.cpu(), None), (x.cpu(), None)], gpu_device, a)
    assert list(meters.keys()) == ["pix_recon", "pix_con", "lat_con", "total_loss"] and not net.training
    assert all(mt.count == 2 and np.isfinite(mt.avg) for mt in meters.values())
