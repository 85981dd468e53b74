"""The conv Sphere Encoder (models/sphere_encoder.py, csrc/sphere.hip) against golden vectors recorded from the reference's own class
(tests/golden/generate_sphere_encoder.py) and against float64 restatements of its formulas: constructor, init replay and the builder
on the CPU; the two kernel pairs alone, the model's forward / losses / Jacobian rows / step / eval / sampling, the aggregated step,
the in-kernel noise and graph replay on the GPU."""
import ast
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, meta_of

TAGS = ["sphere_encoder_tiny", "sphere_encoder_tiny_mix"]
EPS32 = 2.0 ** -23


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def T(a):
    return torch.from_numpy(np.asarray(a))


def build(fx):
    import movae_amd  # noqa: F401
    from movae_amd.models import SphereEncoder

    m = meta_of(fx)
    torch.manual_seed(int(m["seed"]))
    net = SphereEncoder(latent_dim=int(m["latent_dim"]), hidden_dims=ast.literal_eval(m["hidden_dims"]), input_size=int(m["input_size"]),
                        in_channels=3, recons_objective=m["objective"], recons_activation=None, lambda_weights=[1.0, 0.0],
                        use_perceptual=False, **ast.literal_eval(m["kwargs"]))
    return net, m


def assert_close(got, want, what, rtol=1e-3, atol=3e-6):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol * max(1.0, float(np.abs(want).max())), err_msg=what)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_constructor_state_dict_and_init_replay(tag):
    fx = load_golden(tag)
    net, m = build(fx)
    sd = net.state_dict()
    want = [f[4:] for f in fx.files if f.startswith("sd0.")]
    assert list(sd.keys()) == want
    assert want[-2:] == ["encoder_proj.weight", "encoder_proj.bias"] and not any(k.startswith(("mu.", "log_var.")) for k in want)
    for k in want:
        assert np.array_equal(sd[k].numpy(), fx["sd0." + k]), f"init replay {k}"
    assert net.features is None
    assert list(net.objectives.keys()) == [str(s) for s in fx["objectives"]] == ["pix_recon", "pix_con", "lat_con"]
    assert [f"{k}={v!r}" for k, v in net.lambda_weights.items()] == [str(s) for s in fx["lambda_weights"]]
    assert net.lambda_weights == {"reconstruction_loss": 1.0, "kld_loss": 0.0}
    assert net.graph_safe and net._jacobian_from_loss_op
    assert net.radius == math.sqrt(net.L) and net.sigma_max == math.tan(math.radians(net.sigma_max_angle_deg))


def test_constructor_defaults_are_the_references():
    import inspect

    import movae_amd  # noqa: F401
    from movae_amd.models import SphereEncoder

    got = {k: p.default for k, p in inspect.signature(SphereEncoder.__init__).parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == dict(latent_dim=2048, sigma_max_angle_deg=80.0, sigma_mix_prob=0.0, sigma_mix_angle_min_deg=None,
                       sigma_mix_angle_max_deg=None, lambda_pix_recon=1.0, lambda_pix_con=0.5, lambda_lat_con=0.1,
                       pix_recon_smooth_l1_weight=1.0, pix_recon_perceptual_weight=1.0, pix_con_smooth_l1_weight=0.5,
                       pix_con_perceptual_weight=0.5, use_perceptual=True)


def test_perceptual_term_is_refused():
    import movae_amd  # noqa: F401
    from movae_amd.models import SphereEncoder

    with pytest.raises(NotImplementedError, match="VGG16"):
        SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16)  # use_perceptual defaults to True, as in the reference
    with pytest.raises(NotImplementedError, match="VGG16"):
        SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16, use_perceptual=True)


def test_builder_reads_the_cli_flags(capsys):
    import movae_amd  # noqa: F401
    from movae_amd import train
    from movae_amd.models import build_sphere_encoder

    a = train.parse_args(["--sigma_mix_prob", "0.1", "--lambda_pix_con", "0.3", "--sigma_max_angle_deg", "70", "--latent_dim", "12",
                          "--hidden_dims", "4", "8"])
    net = build_sphere_encoder(16, 3, a, None)
    assert (net.sigma_mix_prob, net.lambda_pix_con, net.sigma_max_angle_deg) == (0.1, 0.3, 70.0)
    assert (net.lambda_pix_recon, net.lambda_lat_con, net.sigma_mix_angle_min_deg, net.sigma_mix_angle_max_deg) == (1.0, 0.1, None, None)
    assert net.L == 12 and net.hidden_dims == [4, 8] and net.use_perceptual is False
    assert net.sigma_max == math.tan(math.radians(70.0))
    with pytest.raises(NotImplementedError):
        build_sphere_encoder(16, 3, a, None, use_perceptual=True)


# ---- the latent kernel pair alone ----------------------------------------------------------------------------------------------
def _rms_norm(x, eps=1e-6):  # models/sphere_encoder.py:23-26
    return x / (x.pow(2).mean(dim=-1, keepdim=True) + eps).sqrt()


def _latents_ref(z, e, u, sched, radius, dtype):
    """The formulas of the issue / models/sphere_encoder.py:23-38, 196-220 in `dtype` on the CPU: float64 is the truth, float32 the
    reference's own expressions (the yardstick)."""
    z, e, u = z.to(dtype), e.to(dtype), u.to(dtype)
    angle_max, mix_prob, mix_min, mix_max = sched
    v = _rms_norm(z) * radius
    deg = u[:, 0:1] * angle_max
    if mix_prob > 0:
        deg = torch.where(u[:, 1:2] < mix_prob, mix_min + u[:, 2:3] * (mix_max - mix_min), deg)
    sigma = torch.tan(deg * (math.pi / 180.0))
    sigma_sub = (u[:, 3:4] * 0.5) * sigma
    vn = _rms_norm(v + sigma * e) * radius
    vs = _rms_norm(v + sigma_sub * e) * radius
    return v, vn, vs, sigma, sigma_sub


def _err(a, truth):
    return float((a.detach().double().cpu() - truth.detach()).abs().max())


LAT_SHAPES = [6, 130, 2048, 2051]  # wave per row (scalar tail), wave per row, block per row (16-byte accesses), block per row (tail)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("L", LAT_SHAPES)
def test_latents_kernel_against_float64(L, mix, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B = 5
    g = torch.Generator().manual_seed(100 + L)
    z = torch.randn(B, L, generator=g) * 1.7 + 0.3
    e = torch.randn(B, L, generator=g)
    u = torch.rand(B, 4, generator=g)
    u[:, 1] = torch.tensor([0.1, 0.9, 0.2, 0.8, 0.4])  # rows 0, 2, 4 come from the band at mix_prob 0.5
    u[0, 0], u[1, 0] = 0.999, 0.01                      # an angle at the top of the range and one near zero
    sched = (80.0, 0.5, 80.0, 85.0) if mix else (80.0, 0.0, 0.0, 0.0)
    radius = math.sqrt(L)
    names = ("v", "v_noisy", "v_noisy_small", "sigma", "sigma_sub")

    z64 = z.double().requires_grad_(True)
    z32 = z.clone().requires_grad_(True)
    truth = _latents_ref(z64, e, u, sched, radius, torch.float64)
    yard = _latents_ref(z32, e, u, sched, radius, torch.float32)
    zd = z.to(gpu_device).requires_grad_(True)
    got = ops.sphere_latents(zd, sched, radius, e=e.to(gpu_device), u=u.to(gpu_device))
    again = ops.sphere_latents(zd, sched, radius, e=e.to(gpu_device), u=u.to(gpu_device))
    # Bound per output: 4 x the error of the reference's fp32 expressions against float64 (the 4 is for the different summation order
    # over L) plus 4 ulp of the output's magnitude.  Yardsticks measured on the CPU, max over the eight cases (absolute): v 1.6e-5,
    # v_noisy 3.5e-5, v_noisy_small 2.9e-5 at |value| up to 186 (L = 2048); sigma 1.5e-5 at tan(84.9 deg) = 11.2 -- the fp32 rounding
    # of the angle in radians (6e-8 of 1.48) times sec^2 = 127, about 11 ulp of sigma, hence a bound of its own; sigma_sub 2.9e-6 at 3.7.
    for k, name in enumerate(names):
        t = truth[k].detach()
        e_ref, e_got = _err(yard[k].detach(), t), _err(got[k], t)
        print(f"L={L} mix={mix} {name}: kernel {e_got:.3g} reference-fp32 {e_ref:.3g} |max| {float(t.abs().max()):.3g}")
        assert e_got <= 4 * e_ref + 4 * EPS32 * float(t.abs().max()), (name, e_got, e_ref)
        assert torch.equal(got[k], again[k]), f"{name}: a rerun is not bit-identical"
    if mix:
        assert float(got[3][0]) > math.tan(math.radians(80.0)) > float(got[3][1])  # row 0 from the band, row 1 not

    cots = [torch.randn(B, L, generator=g) for _ in range(3)]
    for subset in itertools.chain.from_iterable(itertools.combinations(range(3), r) for r in (1, 2, 3)):
        def dz(outs, zz, conv):
            return torch.autograd.grad([outs[i] for i in subset], zz, [conv(cots[i]) for i in subset], retain_graph=True)[0]

        t = dz(truth, z64, lambda c: c.double())
        y = dz(yard, z32, lambda c: c)
        k1 = dz(got, zd, lambda c: c.to(gpu_device))
        k2 = dz(got, zd, lambda c: c.to(gpu_device))
        # yardstick of dz measured the same way: up to 3.0e-5 (absolute) at |dz| up to 184
        e_ref, e_got = _err(y, t), _err(k1, t)
        print(f"L={L} mix={mix} dz{subset}: kernel {e_got:.3g} reference-fp32 {e_ref:.3g} |max| {float(t.abs().max()):.3g}")
        assert e_got <= 4 * e_ref + 4 * EPS32 * float(t.abs().max()), (subset, e_got, e_ref)
        assert torch.equal(k1, k2), f"dz{subset}: a rerun is not bit-identical"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [6, 2048])
def test_spherify_clean_and_given_sigma_modes(L, gpu_device):
    """ops.spherify: the clean projection and the given-sigma mode (a scalar, one device value, a value per row) of the same kernels,
    forward and backward, held to the bound of test_latents_kernel_against_float64."""
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B, radius = 5, math.sqrt(L)
    g = torch.Generator().manual_seed(7 + L)
    z, e, cot = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    rows = torch.rand(B, 1, generator=g) * 5.0
    for sigma in (None, 5.671, torch.tensor(5.671), rows):
        def ref(dtype):
            zz = z.to(dtype).requires_grad_(True)
            v = _rms_norm(zz) * radius
            if sigma is not None:
                s = sigma.to(dtype) if isinstance(sigma, torch.Tensor) else sigma
                v = _rms_norm(v + s * e.to(dtype)) * radius
            return v.detach(), torch.autograd.grad(v, zz, cot.to(dtype))[0]

        t, y = ref(torch.float64), ref(torch.float32)
        zd = z.to(gpu_device).requires_grad_(True)
        sd = sigma.to(gpu_device) if isinstance(sigma, torch.Tensor) else sigma
        out = ops.spherify(zd, radius) if sigma is None else ops.spherify(zd, radius, sd, e.to(gpu_device))
        dz = torch.autograd.grad(out, zd, cot.to(gpu_device))[0]
        for name, a, k in (("v", out.detach(), 0), ("dz", dz, 1)):
            e_ref, e_got = _err(y[k], t[k]), _err(a, t[k])
            assert e_got <= 4 * e_ref + 4 * EPS32 * float(t[k].abs().max()), (name, sigma, e_got, e_ref)


# ---- the loss kernel pair alone --------------------------------------------------------------------------------------------------
def _losses_ref(r, x, xn, v, ve, lam, w, dtype):
    """models/sphere_encoder.py:249-283 without the perceptual term, in `dtype`."""
    r, x, xn, v, ve = (t.to(dtype) for t in (r, x, xn, v, ve))
    rec = lam[0] * (w[0] * F.smooth_l1_loss(r, x, reduction="mean"))
    con = lam[1] * (w[1] * F.smooth_l1_loss(xn, r.detach(), reduction="mean"))
    lat = lam[2] * (1 - F.cosine_similarity(v, ve, dim=-1)).mean()
    return rec, con, lat, rec + con + lat


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(3 * 16 * 16 * 4, 6), (3 * 16 * 16 * 4, 12), (2999, 6), (2999, 12)])
def test_losses_kernel_against_float64(n, L, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B = 4
    g = torch.Generator().manual_seed(n + L)
    x = torch.rand(n, generator=g)
    r = torch.tanh(torch.randn(n, generator=g) * 2)
    xn = torch.tanh(torch.randn(n, generator=g) * 2)
    assert 0.01 < float(((r - x).abs() >= 1).float().mean()) < 0.99 and 0.01 < float(((xn - r).abs() >= 1).float().mean()) < 0.99
    v = _rms_norm(torch.randn(B, L, generator=g)) * math.sqrt(L)
    ve = _rms_norm(v + 0.8 * torch.randn(B, L, generator=g)) * math.sqrt(L)
    lam, w = (0.8, 0.3, 0.2), (0.9, 0.4)
    names = ("pix_recon", "pix_con", "lat_con", "total_loss")

    def leaves(dtype, dev="cpu"):
        return [t.to(device=dev, dtype=dtype).requires_grad_(True) for t in (r, xn, v, ve)]

    l64, l32, ld = leaves(torch.float64), leaves(torch.float32), leaves(torch.float32, gpu_device)
    truth = _losses_ref(l64[0], x, l64[1], l64[2], l64[3], lam, w, torch.float64)
    yard = _losses_ref(l32[0], x, l32[1], l32[2], l32[3], lam, w, torch.float32)
    got = ops.sphere_losses(ld[0], x.to(gpu_device), ld[1], ld[2], ld[3], lam, w, sg=ld[0].detach())
    # the same bound as for the latent kernels: 4 x the reference's fp32 error + 4 ulp of the magnitude.  Yardsticks measured on the
    # CPU, max over the four cases: pix_recon 2.0e-8 at 0.32, pix_con 9.7e-9 at 0.065, lat_con 6.3e-9 at 0.011, total 2.3e-8 at 0.39;
    # drecons 3.2e-11 at 2.4e-4, dx_NOISY 6.3e-12 at 4e-5, dv 1.1e-9 at 2.3e-3, dv_enc_dec 9.9e-10 at 2.1e-3
    for k, name in enumerate(names):
        t = truth[k].detach()
        e_ref, e_got = _err(yard[k].detach(), t), _err(got[k].detach(), t)
        print(f"n={n} L={L} {name}: kernel {e_got:.3g} reference-fp32 {e_ref:.3g} value {float(t):.6g}")
        assert e_got <= 4 * e_ref + 4 * EPS32 * abs(float(t)), (name, e_got, e_ref)
    for k, name in enumerate(names):
        gt = torch.autograd.grad(truth[k], l64, retain_graph=True, allow_unused=True)
        gy = torch.autograd.grad(yard[k], l32, retain_graph=True, allow_unused=True)
        gk = torch.autograd.grad(got[k], ld, retain_graph=True, allow_unused=True)
        for what, a, y, t in zip(("drecons", "dx_NOISY", "dv", "dv_enc_dec"), gk, gy, gt):
            assert (a is None) == (t is None), f"{name} -> {what}: reached {a is not None}, expected {t is not None}"
            if t is None:
                continue
            e_ref, e_got = _err(y, t), _err(a, t)
            assert e_got <= 4 * e_ref + 4 * EPS32 * float(t.abs().max()), (name, what, e_got, e_ref)
    assert torch.autograd.grad(got[1], ld[0], retain_graph=True, allow_unused=True)[0] is None, "pix_con sends a gradient to recons"
    # a separate (non-aliasing) sg tensor takes the other read path and gives the same numbers
    other = ops.sphere_losses(ld[0], x.to(gpu_device), ld[1], ld[2], ld[3], lam, w, sg=ld[0].detach().clone())
    assert all(torch.equal(a, b) for a, b in zip(got, other))


# ---- the model against the fixtures ------------------------------------------------------------------------------------------------
def _gpu_net(fx, dev):
    net, m = build(fx)
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
        if k.endswith("num_batches_tracked"):  # one update per encoder / decoder call: two per module per step
            assert int(sd1[k].item()) == int(want) == 2, k
            continue
        noise = ("gsum." + k) in fx.files and np.abs(fx["gsum." + k]).max() < 1e-6
        np.testing.assert_allclose(sd1[k].cpu().numpy(), want, rtol=2e-4, atol=2.1e-3 if noise else 3e-5, err_msg=k)
    ld2 = net.loss_function(x, args=net(x))
    for k, v in ld2.items():
        np.testing.assert_allclose(v.item(), fx["loss2." + k], rtol=1e-3, atol=2e-6, err_msg="loss2 " + k)
    net.eval()
    with torch.no_grad():
        oe = net(x)  # (eval mode draws noise too: the override stands in for it)
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
@pytest.mark.parametrize("agg", ["upgrad", "mgda", "aligned_mtl"])
def test_aggregated_step_matches_oracle_on_fixture_jacobian(agg, batched, gpu_device, monkeypatch):
    import movae_amd  # noqa: F401
    from movae_amd import aggregation, autojac, train
    from oracle.aggregation import aggregate, make_weighting

    monkeypatch.setattr(autojac, "BATCHED_FULL_JACOBIAN", batched)  # MOVAE_BATCHED_FULL_JACOBIAN=1 / the sequential default
    walked = []
    real = autojac._batched_pullback
    monkeypatch.setattr(autojac, "_batched_pullback", lambda *a, **k: (real(*a, **k), walked.append(len(a[2])))[0])
    fx = load_golden("sphere_encoder_tiny")
    net, m = _gpu_net(fx, gpu_device)
    names = [n for n, _ in net.named_parameters()]
    K = len([f for f in fx.files if f.startswith("loss.")]) - 1
    J = torch.cat([torch.cat([T(fx[f"gloss.{i}.{n}"]).reshape(-1) for n in names]).reshape(1, -1) for i in range(K)]).double()
    losses = np.array([float(fx["loss." + k]) for k in [f[5:] for f in fx.files if f.startswith("loss.")] if k != "total_loss"])
    g_want, w_want, _ = aggregate(J, make_weighting(agg), losses)
    a = Args(aggregator=agg, agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None)
    A = aggregation.make_aggregator(a)
    seen = {}
    A.weighting.register_forward_hook(lambda mod, inp, out: seen.update(w=out.clone()))
    x = T(fx["x"]).to(gpu_device)
    train.forward_backward(net, x, torch.optim.SGD(net.parameters(), lr=0.0), A)
    assert walked == ([K] if batched else []), walked  # the batched form ran once over all K rows and did not fall back
    cond = agg != "upgrad"
    np.testing.assert_allclose(seen["w"].cpu().numpy(), w_want.numpy(), rtol=2e-2 if cond else 1e-3, atol=1e-4)
    off = 0
    for n, p in net.named_parameters():
        want = g_want[off: off + p.numel()].reshape(p.shape).float().numpy()
        off += p.numel()
        assert_close(p.grad if p.grad is not None else torch.zeros_like(p), want, f"{agg} grad {n}", rtol=3e-2 if cond else 2e-3,
                     atol=1e-4 if cond else 1e-5)


# ---- in-kernel noise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_in_kernel_noise(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B, L, p = 4096, 18, 0.3  # (L = 18: four full counter blocks and a partial one per row)
    sched, radius = (70.0, p, 80.0, 85.0), math.sqrt(L)
    z = torch.randn(B, L, generator=torch.Generator().manual_seed(1)).to(gpu_device).requires_grad_(True)
    state = torch.tensor([1234, 5], dtype=torch.int64, device=gpu_device)
    s0 = state.clone()
    out = ops.sphere_latents(z, sched, radius, state=state)
    v, vn, vs, sigma, sigma_sub, e, u = out
    assert state.tolist() == [1234, 6] and e.shape == (B, L) and u.shape == (B, 4) and not e.requires_grad and not sigma.requires_grad
    ed = e.double()
    n = B * L  # four standard errors of the mean and of the standard deviation of n standard normals
    assert abs(ed.mean().item()) < 4 / math.sqrt(n) and abs(ed.std().item() - 1) < 4 / math.sqrt(2 * n)
    assert abs((ed ** 3).mean().item()) < 4 * math.sqrt(15 / n) and abs((ed ** 4).mean().item() - 3) < 4 * math.sqrt(96 / n)
    assert abs(float((ed[:, :-1] * ed[:, 1:]).mean())) < 4 / math.sqrt(B * (L - 1))  # neighbours within a counter block are uncorrelated
    assert 0 <= float(u.min()) and float(u.max()) < 1
    for c in range(4):  # uniform: mean 1/2, variance 1/12
        assert abs(u[:, c].double().mean().item() - 0.5) < 4 * math.sqrt(1 / 12 / B)
    band = u[:, 1] < p
    assert abs(band.float().mean().item() - p) < 4 * math.sqrt(p * (1 - p) / B)  # four binomial standard errors
    sg = sigma[:, 0]
    hi = math.tan(math.radians(70.0)) * (1 + 1e-5)
    assert float(sg[~band].min()) >= 0 and float(sg[~band].max()) <= hi
    assert float(sg[band].min()) >= math.tan(math.radians(80.0)) * (1 - 1e-5) and float(sg[band].max()) <= math.tan(math.radians(85.0)) * (1 + 1e-5)
    assert float(sigma_sub.min()) >= 0 and bool((sigma_sub <= 0.5 * sigma).all())
    # the next draw number gives fresh draws; the same state gives the same ones
    out2 = ops.sphere_latents(z, sched, radius, state=state)
    assert state.tolist() == [1234, 7] and not torch.equal(out2[5], e) and not torch.equal(out2[6], u)
    assert abs(float((out2[5].double() * ed).mean())) < 4 / math.sqrt(n)
    same = ops.sphere_latents(z, sched, radius, state=s0)
    assert s0.tolist() == [1234, 6] and all(torch.equal(a, b) for a, b in zip(same, out))
    # forward and backward from the written-out draws equal the override path
    over = ops.sphere_latents(z, sched, radius, e=e, u=u)
    assert all(torch.equal(a, b) for a, b in zip(over[:5], out[:5]))
    cots = [torch.randn(B, L, generator=torch.Generator().manual_seed(2 + i)).to(gpu_device) for i in range(3)]
    dz_rng = torch.autograd.grad(out[:3], z, cots)[0]
    dz_over = torch.autograd.grad(over[:3], z, cots)[0]
    assert torch.equal(dz_rng, dz_over) and bool(torch.isfinite(dz_rng).all())


# ---- graph replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hipgraph_replay_matches_eager_steps(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import aggregation
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    fx = load_golden("sphere_encoder_tiny")
    a = Args(aggregator="upgrad", agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None,
             optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None)
    x = T(fx["x"]).to(gpu_device)
    g = torch.Generator().manual_seed(11)
    batches = [x] + [torch.rand(x.shape, generator=g).to(gpu_device) for _ in range(2)]
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
    for (n, p), (_, q) in zip(net_e.named_buffers(), net_g.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(p) == int(q) == 6, n  # three steps, two calls per module

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
    assert net_r._noise_state_t.tolist()[1] == 3  # preserve_state rewound the warm-up draws; three replays since


@pytest.mark.gpu
def test_train_step_and_evaluate(gpu_device):
    """train.train_step in eager mode with torch's own draws, and train.evaluate (eval mode draws noise too)."""
    import movae_amd  # noqa: F401
    from movae_amd import aggregation, train

    fx = load_golden("sphere_encoder_tiny_mix")
    net, _ = build(fx)
    net = net.to(gpu_device).train()
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
    np.testing.assert_allclose(meters["total_loss"].avg, sum(meters[k].avg for k in ("pix_recon", "pix_con", "lat_con")), rtol=1e-5)
