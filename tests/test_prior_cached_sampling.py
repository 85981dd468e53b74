"""Cached ancestral sampling for the PixelCNN priors (sampling.CachedPixelCNNSampler, csrc/prior_sample.hip): one launch per code.

The cached path is pinned position by position against quantities the suite already trusts: under teacher forcing a causal
network's step logits ARE the full forward's logits at every position, so they must match the reference's own vectors
(tests/golden/pixelcnn_tiny.npz) and forward_nhwc of the same model, at the tolerance test_prior.py uses for these logits; the
draw is checked as an inverse CDF against float64, and the Philox draw against the distribution it draws from."""
import numpy as np
import pytest
import torch

from conftest import load_golden, meta_of

TOL = dict(rtol=2e-4, atol=2e-5)  # test_prior.py's tolerance for the same logits against the reference's vectors


def _cfg(fx, hier):
    m = meta_of(fx)
    c = {k: int(m[k]) for k in ("num_embeddings", "embedding_dim", "hidden_channels", "num_layers")}
    c["hierarchical"] = hier
    return c, int(m["seed"])


def _build_hip(cfg, seed, device):
    """As test_prior.py::_build_hip."""
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelCNN, PixelCNN

    torch.manual_seed(seed)
    a = (cfg["num_embeddings"], cfg["embedding_dim"], cfg["hidden_channels"], cfg["num_layers"])
    return (HierarchicalPixelCNN(*a) if cfg["hierarchical"] else PixelCNN(*a)).to(device).train()


def _sampler(net):
    from movae_amd.sampling import CachedPixelCNNSampler

    return CachedPixelCNNSampler(net)


def _forced_logits(net, z, condition=None):
    """NCHW logits of the cached path under teacher forcing with the codes z; the returned codes must be the forced ones."""
    B, H, W = z.shape
    codes, lg = _sampler(net).run(B, H, W, condition=condition, forced=z, return_logits=True)
    assert codes.dtype == torch.int64 and torch.equal(codes, z)
    assert tuple(lg.shape) == (B, H, W, net.num_embeddings)
    return lg.permute(0, 3, 1, 2).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["flat", "hier"])
def test_teacher_forced_logits_equal_reference_vectors(tag, gpu_device):
    from movae_amd.models._base import nchw_view

    fx = load_golden("pixelcnn_tiny")
    cfg, seed = _cfg(fx, tag == "hier")
    net = _build_hip(cfg, seed, gpu_device)
    if tag == "flat":
        z = torch.from_numpy(fx["z"]).to(gpu_device)
        np.testing.assert_allclose(_forced_logits(net, z), fx["flat.logits"], **TOL)
        return
    zt, zb = torch.from_numpy(fx["z_top"]).to(gpu_device), torch.from_numpy(fx["z_bottom"]).to(gpu_device)
    np.testing.assert_allclose(_forced_logits(net.prior_top, zt), fx["hier.logits_top"], err_msg="top", **TOL)
    with torch.no_grad():
        cond = nchw_view(net._condition(zt))  # what HierarchicalPixelCNN.sample hands the bottom level
    np.testing.assert_allclose(_forced_logits(net.prior_bottom, zb, cond), fx["hier.logits_bottom"], err_msg="bottom", **TOL)


#: (B, H, W, K, D, hidden, layers, conv_in kernel, conditional channels)
SHAPES = {
    "ragged_5x7_K20": (3, 5, 7, 20, 8, 32, 2, 7, 0),  # non-square, H narrower than the 7-tap window, K and B multiples of nothing
    "real_widths": (2, 4, 4, 512, 64, 128, 3, 7, 0),
    "half_24": (5, 3, 9, 16, 4, 48, 1, 7, 0),  # C/2 = 24
    "no_blocks": (2, 4, 5, 16, 8, 32, 0, 7, 0),
    "kernel_3": (2, 5, 6, 16, 8, 32, 2, 3, 0),
    "kernel_5": (2, 5, 6, 16, 8, 32, 2, 5, 0),
    "conditional_6x6": (2, 6, 6, 16, 8, 32, 2, 7, 8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SHAPES))
def test_teacher_forced_logits_equal_full_forward(case, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops
    from movae_amd.models.pixelcnn_prior import PixelCNN

    B, H, W, K, D, hidden, layers, ks, cc = SHAPES[case]
    torch.manual_seed(11)
    net = PixelCNN(K, D, hidden, layers, kernel_size=ks, conditional_channels=cc).to(gpu_device).eval()
    g = torch.Generator().manual_seed(12)
    z = torch.randint(0, K, (B, H, W), generator=g).to(gpu_device)
    cond = torch.randn(B, cc, H, W, generator=g).to(gpu_device) if cc else None
    with torch.no_grad():
        want = net.forward_nhwc(z, ops.to_nhwc(cond) if cc else None).permute(0, 3, 1, 2).cpu().numpy()
    np.testing.assert_allclose(_forced_logits(net, z, cond), want, **TOL)


_FREE = {}


def _free_run(device, temperature):
    """One free run per temperature with given uniforms at (B 3, 6x6, K 16, hidden 32, L 2), shared by the tests below."""
    if temperature not in _FREE:
        import movae_amd  # noqa: F401
        from movae_amd.models.pixelcnn_prior import PixelCNN

        torch.manual_seed(21)
        net = PixelCNN(16, 8, 32, 2).to(device).eval()
        u = torch.rand(3, 6, 6, generator=torch.Generator().manual_seed(22))
        z, lg = _sampler(net).run(3, 6, 6, temperature=temperature, uniforms=u.to(device), return_logits=True)
        _FREE[temperature] = (net, u.numpy().astype(np.float64), z, lg)
    return _FREE[temperature]


@pytest.mark.gpu
def test_free_run_closes_on_itself(gpu_device):
    """One full forward over the sampled codes reproduces the logits the run saw: the caches were filled from those codes."""
    net, _, z, lg = _free_run(gpu_device, 1.0)
    assert z.dtype == torch.int64 and tuple(z.shape) == (3, 6, 6) and int(z.min()) >= 0 and int(z.max()) < 16
    assert len(torch.unique(z)) > 4  # (a run that ignored its draws would repeat one code)
    with torch.no_grad():
        want = net.forward_nhwc(z)
    np.testing.assert_allclose(lg.cpu().numpy(), want.cpu().numpy(), **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_draw_is_the_inverse_cdf(temperature, gpu_device):
    """code = the smallest k with u < cdf_k, clamped to K - 1, with cdf from the returned logits in float64.  Draws whose u lies
    within 1e-5 of a cdf boundary are left out; with K = 16 their expected share is <= 2e-5 * 16 = 3.2e-4, the condition is 1 %."""
    _, u, z, lg = _free_run(gpu_device, temperature)
    s = lg.cpu().numpy().astype(np.float64) / temperature
    p = np.exp(s - s.max(-1, keepdims=True))
    cdf = np.cumsum(p / p.sum(-1, keepdims=True), axis=-1)
    want = np.minimum((cdf <= u[..., None]).sum(-1), 15)
    near = np.abs(cdf - u[..., None]).min(-1) < 1e-5
    print(f"T={temperature}: {int(near.sum())} of {near.size} draws within 1e-5 of a boundary; "
          f"{int((z.cpu().numpy() != want)[~near].sum())} of the rest differ")
    assert near.mean() <= 0.01
    assert np.array_equal(z.cpu().numpy()[~near], want[~near])


@pytest.mark.gpu
def test_philox_draw_is_a_draw(gpu_device):
    """4096 one-pixel samples share one distribution p: every count lies within 5 sigma (+ 1) of B p_k; the same (seed, draw
    number) repeats the codes, another seed or another draw number does not."""
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import PixelCNN

    B, K = 4096, 8
    torch.manual_seed(31)
    net = PixelCNN(K, 4, 8, 1).to(gpu_device).eval()
    smp = _sampler(net)
    assert smp.draws == 0
    z, lg = smp.run(B, 1, 1, seed=1234, return_logits=True)
    assert smp.draws == 1
    lg = lg.reshape(B, K)
    assert torch.equal(lg, lg[:1].expand(B, K))  # no causal tap is inside a 1x1 grid: one distribution
    p = torch.softmax(lg[0].double(), 0).cpu().numpy()
    n = np.bincount(z.reshape(-1).cpu().numpy(), minlength=K)
    print("counts", n.tolist(), "expected", np.round(B * p, 1).tolist())
    assert n.sum() == B and np.all(np.abs(n - B * p) <= 5 * np.sqrt(B * p * (1 - p)) + 1), (n, B * p)
    smp.draws = 0
    assert torch.equal(smp.run(B, 1, 1, seed=1234), z)
    smp.draws = 0
    assert not torch.equal(smp.run(B, 1, 1, seed=1235), z)
    assert smp.draws == 1 and not torch.equal(smp.run(B, 1, 1, seed=1234), z)  # draw number 1


@pytest.mark.gpu
def test_a_sample_does_not_depend_on_its_batch(gpu_device, monkeypatch):
    """Same seed and draw number at B = 7 and B = 2 (4x5): the first two samples' codes and logits are bitwise equal (workgroup
    tail, absolute-index keying); so is a B = 7 run whose caches are split into chunks of 3 samples."""
    import movae_amd  # noqa: F401
    from movae_amd import sampling
    from movae_amd.models.pixelcnn_prior import PixelCNN

    torch.manual_seed(41)
    net = PixelCNN(16, 8, 32, 2).to(gpu_device).eval()
    z7, l7 = _sampler(net).run(7, 4, 5, seed=99, return_logits=True)
    z2, l2 = _sampler(net).run(2, 4, 5, seed=99, return_logits=True)
    assert torch.equal(z7[:2], z2) and torch.equal(l7[:2], l2)
    assert not torch.equal(z7[0], z7[1])
    per_sample = 4 * 4 * 5 * (8 + 2 * 16)
    monkeypatch.setattr(sampling, "MAX_CACHE_BYTES", 3 * per_sample)
    zc, lc = _sampler(net).run(7, 4, 5, seed=99, return_logits=True)
    assert torch.equal(zc, z7) and torch.equal(lc, l7)


def _stage_argv(arch, tmp_path):
    """The arguments of test_prior.py::test_prior_training_stage_on_vq_codes, with one prior epoch."""
    return ["--dataset", "synthetic_cifar10", "--arch", arch, "--embedding_dim", "8", "--num_embeddings", "16", "--hidden_dims", "16", "32",
            "--batch_size", "32", "--max_items", "128", "--epochs", "1", "--pixelcnn_epochs", "1", "--pixelcnn_hidden_channels", "16",
            "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3", "--save_path", str(tmp_path), "--seed", "1", "--device", "cuda:0",
            "--eval_freq", "0"]


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["vq_vae", "vq_vae2"])
def test_generate_samples_cached(arch, gpu_device, tmp_path):
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train
    from movae_amd.models import get_network

    args = train.parse_args(_stage_argv(arch, tmp_path))
    train.set_seed(args.seed)
    net = get_network(32, num_channels=3, args=args, device=gpu_device).to(gpu_device)
    prior = P.build_prior(net, args, gpu_device)
    full = P.generate_samples_vq_with_prior(net, prior, 2, gpu_device, 1.0, cached=False)
    imgs = P.generate_samples_vq_with_prior(net, prior, 2, gpu_device, 1.0, cached=True)
    assert imgs.shape == full.shape and imgs.shape[0] == 2 and torch.isfinite(imgs).all()
    if arch == "vq_vae2":
        assert prior.prior_top.cached_sampler().draws == 1 and prior.prior_bottom.cached_sampler().draws == 1
        return
    smp = prior.cached_sampler()
    assert smp.draws == 1
    smp.draws = 0  # the draw number of the call above, under the same torch.cuda.initial_seed()
    s = net.latent_spatial_dim
    z = smp.run(2, s, s)
    with torch.no_grad():
        want = net.decode(net.vq_layer.embed_code(z).permute(0, 3, 1, 2))
    assert torch.equal(imgs, want)


@pytest.mark.gpu
def test_hierarchical_pixelsnail_samples_its_bottom_cached(gpu_device):
    """cached=True: the PixelSNAIL top by full recompute (it has no cached sampler), the PixelCNN bottom through the cached one."""
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelSNAIL

    torch.manual_seed(51)
    net = HierarchicalPixelSNAIL(16, 8, hidden_channels=16, num_blocks_top=1, num_res_blocks_per_layer=1, num_heads=2,
                                 num_layers_bottom=1).to(gpu_device)
    zt, zb = net.sample(2, (2, 2), (4, 4), gpu_device, cached=True)
    assert tuple(zt.shape) == (2, 2, 2) and tuple(zb.shape) == (2, 4, 4) and zb.dtype == torch.int64
    assert 0 <= int(zb.min()) and int(zb.max()) < 16
    assert net.prior_bottom.cached_sampler().draws == 1 and "_cached_sampler" not in net.prior_top.__dict__


@pytest.mark.gpu
def test_prior_stage_with_cached_sampler(gpu_device, tmp_path):
    """--prior_sampler cached through train.main: the stage's visualisation samples come from the cached path."""
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train

    args = train.parse_args(_stage_argv("vq_vae", tmp_path) + ["--prior_sampler", "cached"])
    train.set_seed(args.seed)
    train.main(args)
    rec = P.LAST_RUN
    assert len(rec["epoch_losses"]) == 1
    assert rec["prior"].cached_sampler().draws == 1
    imgs = rec["samples"]
    assert tuple(imgs.shape) == (4, 3, 32, 32) and torch.isfinite(imgs).all()


def test_prior_sampler_flag_parses_and_defaults_to_full():
    import movae_amd  # noqa: F401
    from movae_amd import train

    base = ["--dataset", "synthetic_cifar10", "--arch", "vq_vae"]
    assert train.parse_args(base).prior_sampler == "full"
    assert train.parse_args(base + ["--prior_sampler", "cached"]).prior_sampler == "cached"
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--prior_sampler", "fast"])


def test_pixelsnail_refuses_cached_sampling():
    """Before any kernel is touched: the model lives on the CPU, where every op raises."""
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import PixelSNAIL

    net = PixelSNAIL(12, 6, hidden_channels=16, num_blocks=1, num_res_blocks_per_layer=1, num_heads=2)
    with pytest.raises(NotImplementedError, match="K/V cache"):
        net.sample(2, 3, 3, "cpu", cached=True)


def test_unsupported_shape_raises_value_error():
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import PixelCNN
    from movae_amd.sampling import CachedPixelCNNSampler

    net = PixelCNN(16, 8, hidden_channels=514, num_layers=1)
    with pytest.raises(ValueError, match="hidden_channels <= 256"):
        net.sample(2, 3, 3, "cpu", cached=True)
    with pytest.raises(ValueError, match="hidden_channels <= 256"):
        CachedPixelCNNSampler(net)
    with pytest.raises(ValueError, match="num_embeddings <= 2048"):
        CachedPixelCNNSampler(PixelCNN(4096, 8, hidden_channels=16, num_layers=1))
