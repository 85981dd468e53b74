"""Cached ancestral sampling for the PixelSNAIL priors (sampling.CachedPixelSNAILSampler, csrc/prior_sample.hip): one launch per
code over the cached conv1 outputs and the attention layers' K/V cache.

As in test_prior_cached_sampling.py the cached path is pinned position by position against quantities the suite already trusts:
under teacher forcing a causal network's step logits ARE the full forward's logits at every position, so they must match the
reference's own vectors (tests/golden/pixelsnail_tiny.npz) and forward_nhwc of the same model in eval mode, at the tolerance
test_pixelsnail.py uses for these logits; the draw is checked as an inverse CDF against float64, and a sample against the batch it
is drawn in, bitwise."""
import numpy as np
import pytest
import torch

from conftest import load_golden, meta_of

TOL = dict(rtol=2e-4, atol=2e-5)  # test_pixelsnail.py's tolerance for the same logits against the reference's vectors


def _build(tag, device):
    """As test_pixelsnail.py::_build (dropout 0 for flat / hier, the default 0.1 for eval)."""
    import movae_amd  # noqa: F401
    from movae_amd.models import HierarchicalPixelSNAIL, PixelSNAIL

    fx = load_golden("pixelsnail_tiny")
    m = {k: (float(v) if k == "lr" else int(v)) for k, v in meta_of(fx).items()}
    K, D, hid, nb, nr, nh = (m[k] for k in ("num_embeddings", "embedding_dim", "hidden_channels", "num_blocks",
                                            "num_res_blocks_per_layer", "num_heads"))
    torch.manual_seed(m["seed"] + (1 if tag == "eval" else 0))
    if tag == "hier":
        net = HierarchicalPixelSNAIL(K, D, hid, num_blocks_top=nb, num_res_blocks_per_layer=nr, num_heads=nh,
                                     num_layers_bottom=m["num_layers_bottom"], dropout=0.0)
    elif tag == "eval":
        net = PixelSNAIL(K, D, hid, num_blocks=nb, num_res_blocks_per_layer=nr, num_heads=nh)
    else:
        net = PixelSNAIL(K, D, hid, num_blocks=nb, num_res_blocks_per_layer=nr, num_heads=nh, dropout=0.0)
    return fx, net.to(device)


def _sampler(net):
    from movae_amd.sampling import CachedPixelSNAILSampler

    return CachedPixelSNAILSampler(net)


def _forced_logits(net, z, condition=None):
    """NCHW logits of the cached path under teacher forcing with the codes z; the returned codes must be the forced ones."""
    B, H, W = z.shape
    codes, lg = _sampler(net).run(B, H, W, condition=condition, forced=z, return_logits=True)
    assert codes.dtype == torch.int64 and torch.equal(codes, z)
    assert tuple(lg.shape) == (B, H, W, net.num_embeddings)
    return lg.permute(0, 3, 1, 2).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["flat", "eval", "hier"])
def test_teacher_forced_logits_equal_reference_vectors(tag, gpu_device):
    """flat.logits (3x6x7) and eval.logits of the flat models, hier.logits_top (2x4x4) of the hierarchical model's top.  The eval
    model carries the default dropout 0.1 and is left in training mode: the sampler is eval mode whatever the flag says."""
    fx, net = _build(tag, gpu_device)
    net.train()
    if tag == "hier":
        z = torch.from_numpy(fx["z_top"]).to(gpu_device)
        np.testing.assert_allclose(_forced_logits(net.prior_top, z), fx["hier.logits_top"], **TOL)
        return
    z = torch.from_numpy(fx["z"]).to(gpu_device)
    np.testing.assert_allclose(_forced_logits(net, z), fx[f"{tag}.logits"], **TOL)


#: (B, H, W, K, D, hidden, blocks, gated blocks per block, heads, conv_in kernel, conditional channels)
SHAPES = {
    "ragged_5x6_B3": (3, 5, 6, 20, 8, 32, 2, 1, 2, 7, 0),  # non-square, narrower than the 7-tap window, K a multiple of nothing
    "ragged_5x6_B5": (5, 5, 6, 20, 8, 32, 2, 1, 2, 7, 0),  # one full workgroup and a tail of one sample
    "keys_81": (2, 9, 9, 16, 8, 32, 1, 1, 2, 7, 0),  # more than 64 keys: the lanes' second round
    "keys_132": (2, 12, 11, 16, 8, 32, 1, 1, 2, 7, 0),  # more than 128 keys
    "head_dim_12": (2, 4, 5, 16, 4, 48, 1, 1, 4, 7, 0),  # C/2 = 24; head rows that are not 16-byte chunks of 16
    "head_dim_32": (2, 4, 5, 16, 8, 64, 1, 1, 2, 7, 0),  # two lanes per key
    "head_dim_64": (2, 4, 5, 16, 8, 128, 1, 1, 2, 7, 0),  # four lanes per key
    "head_dim_64_keys_81": (1, 9, 9, 16, 8, 128, 1, 0, 2, 3, 0),  # four lanes per key, 16 keys per round: six rounds
    "head_dim_40": (2, 4, 5, 16, 8, 80, 1, 1, 2, 7, 0),  # four lanes per key, the fourth owning no channel
    "one_head": (2, 4, 5, 16, 8, 16, 1, 1, 1, 7, 0),
    "head_dim_6": (2, 4, 5, 16, 8, 12, 1, 1, 2, 7, 0),  # head_dim not a multiple of 4: the scalar row loads
    "real_widths": (2, 4, 4, 512, 64, 128, 1, 2, 8, 7, 0),
    "no_gated_blocks": (2, 4, 5, 16, 8, 32, 2, 0, 2, 7, 0),
    "no_blocks": (2, 4, 5, 16, 8, 32, 0, 2, 2, 7, 0),
    "kernel_3": (2, 5, 6, 16, 8, 32, 1, 1, 2, 3, 0),
    "kernel_5": (2, 5, 6, 16, 8, 32, 1, 1, 2, 5, 0),
    "conditional_6x6": (2, 6, 6, 16, 8, 32, 1, 1, 2, 7, 8),
    "two_blocks_of_two": (2, 4, 5, 16, 8, 32, 2, 2, 2, 7, 0),  # the conv1 cache is indexed over all four gated blocks
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SHAPES))
def test_teacher_forced_logits_equal_full_forward(case, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops
    from movae_amd.models.pixelcnn_prior import PixelSNAIL

    B, H, W, K, D, hidden, nb, nr, heads, ks, cc = SHAPES[case]
    torch.manual_seed(11)
    net = PixelSNAIL(K, D, hidden, num_blocks=nb, num_res_blocks_per_layer=nr, num_heads=heads, kernel_size=ks,
                     conditional_channels=cc).to(gpu_device).eval()
    g = torch.Generator().manual_seed(12)
    z = torch.randint(0, K, (B, H, W), generator=g).to(gpu_device)
    cond = torch.randn(B, cc, H, W, generator=g).to(gpu_device) if cc else None
    with torch.no_grad():
        want = net.forward_nhwc(z, ops.to_nhwc(cond) if cc else None).permute(0, 3, 1, 2).cpu().numpy()
    got = _forced_logits(net, z, cond)
    print(f"{case}: max |cached - forward| = {np.abs(got - want).max():.3e}, max |logit| = {np.abs(want).max():.3f}")
    np.testing.assert_allclose(got, want, **TOL)


_FREE = {}


def _free_run(device, temperature):
    """One free run per temperature with given uniforms at (B 3, 6x6, K 16, hidden 32, 2 blocks x 1, 2 heads), shared by the tests
    below."""
    if temperature not in _FREE:
        import movae_amd  # noqa: F401
        from movae_amd.models.pixelcnn_prior import PixelSNAIL

        torch.manual_seed(21)
        net = PixelSNAIL(16, 8, 32, num_blocks=2, num_res_blocks_per_layer=1, num_heads=2).to(device).eval()
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
def test_a_sample_does_not_depend_on_its_batch(gpu_device, monkeypatch):
    """Same seed and draw number at B = 7 and B = 2 (4x5): the first two samples' codes and logits are bitwise equal (workgroup
    tail, absolute-index keying, the fixed order of the attention's partials); so is a B = 7 run whose caches are split into chunks
    of 3 samples.  Two samples of one run differ."""
    import movae_amd  # noqa: F401
    from movae_amd import sampling
    from movae_amd.models.pixelcnn_prior import PixelSNAIL

    torch.manual_seed(41)
    net = PixelSNAIL(16, 8, 32, num_blocks=2, num_res_blocks_per_layer=1, num_heads=2).to(gpu_device).eval()
    z7, l7 = _sampler(net).run(7, 4, 5, seed=99, return_logits=True)
    z2, l2 = _sampler(net).run(2, 4, 5, seed=99, return_logits=True)
    assert torch.equal(z7[:2], z2) and torch.equal(l7[:2], l2)
    assert not torch.equal(z7[0], z7[1])
    per_sample = 4 * 4 * 5 * ((8 + 2) + 2 * 16 + 2 * 2 * 32)  # 4 H W (D0 + n_gated C/2 + n_blocks 2P)
    monkeypatch.setattr(sampling, "MAX_CACHE_BYTES", 3 * per_sample)
    zc, lc = _sampler(net).run(7, 4, 5, seed=99, return_logits=True)
    assert torch.equal(zc, z7) and torch.equal(lc, l7)


@pytest.mark.gpu
def test_sample_surface(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelSNAIL, PixelSNAIL

    torch.manual_seed(51)
    net = PixelSNAIL(12, 6, hidden_channels=16, num_blocks=1, num_res_blocks_per_layer=1, num_heads=2).to(gpu_device)
    z = net.sample(2, 3, 3, gpu_device, cached="kv")
    assert z.dtype == torch.int64 and tuple(z.shape) == (2, 3, 3) and 0 <= int(z.min()) and int(z.max()) < 12
    assert net.cached_sampler().draws == 1
    hier = HierarchicalPixelSNAIL(16, 8, hidden_channels=16, num_blocks_top=1, num_res_blocks_per_layer=1, num_heads=2,
                                  num_layers_bottom=1).to(gpu_device)
    zt, zb = hier.sample(2, (2, 2), (4, 4), gpu_device, cached="kv")
    assert tuple(zt.shape) == (2, 2, 2) and tuple(zb.shape) == (2, 4, 4) and zt.dtype == zb.dtype == torch.int64
    assert 0 <= int(zt.min()) and int(zt.max()) < 16 and 0 <= int(zb.min()) and int(zb.max()) < 16
    assert hier.prior_top.cached_sampler().draws == 1 and hier.prior_bottom.cached_sampler().draws == 1


def _stage_argv(arch, tmp_path):
    """The arguments of test_pixelsnail.py::test_pixelsnail_prior_stage."""
    return ["--dataset", "synthetic_cifar10", "--arch", arch, "--embedding_dim", "8", "--num_embeddings", "16", "--hidden_dims", "16",
            "32", "--batch_size", "32", "--max_items", "128", "--epochs", "1", "--pixelcnn_epochs", "1", "--pixelcnn_hidden_channels",
            "16", "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3", "--save_path", str(tmp_path), "--seed", "1", "--device",
            "cuda:0", "--eval_freq", "0", "--pixelsnail_num_blocks", "2", "--pixelsnail_num_res_blocks", "1", "--pixelsnail_num_heads",
            "2"]


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["vq_vae", "vq_vae2"])
def test_generate_samples_kv_cached(arch, gpu_device, tmp_path):
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train
    from movae_amd.models import get_network
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelSNAIL, PixelSNAIL

    args = train.parse_args(_stage_argv(arch, tmp_path))
    train.set_seed(args.seed)
    net = get_network(32, num_channels=3, args=args, device=gpu_device).to(gpu_device)
    prior = P.build_pixelsnail_prior(net, args, gpu_device)
    imgs = P.generate_samples_vq_with_prior(net, prior, 2, gpu_device, 1.0, cached="kv")
    assert tuple(imgs.shape) == (2, 3, 32, 32) and torch.isfinite(imgs).all()
    if arch == "vq_vae2":
        assert type(prior) is HierarchicalPixelSNAIL
        assert prior.prior_top.cached_sampler().draws == 1 and prior.prior_bottom.cached_sampler().draws == 1
        return
    assert type(prior) is PixelSNAIL
    smp = prior.cached_sampler()
    assert smp.draws == 1
    smp.draws = 0  # the draw number of the call above, under the same torch.cuda.initial_seed()
    s = net.latent_spatial_dim
    z = smp.run(2, s, s)
    with torch.no_grad():
        want = net.decode(net.vq_layer.embed_code(z).permute(0, 3, 1, 2))
    assert torch.equal(imgs, want)


def test_prior_sampler_flag_takes_cached_kv():
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train

    base = ["--dataset", "synthetic_cifar10", "--arch", "vq_vae"]
    assert train.parse_args(base).prior_sampler == "full"
    assert train.parse_args(base + ["--prior_sampler", "cached_kv"]).prior_sampler == "cached_kv"
    assert P.PRIOR_SAMPLERS == {"full": False, "cached": True, "cached_kv": "kv"}


def test_sampler_refuses_what_it_cannot_sample():
    """Before any kernel is touched: the models live on the CPU, where every op raises."""
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import PixelCNN, PixelSNAIL
    from movae_amd.sampling import CachedPixelSNAILSampler

    with pytest.raises(TypeError, match="PixelSNAIL"):
        CachedPixelSNAILSampler(PixelCNN(16, 8, hidden_channels=16, num_layers=1))
    net = PixelSNAIL(16, 8, hidden_channels=512, num_blocks=1, num_res_blocks_per_layer=1, num_heads=8)
    with pytest.raises(ValueError, match="hidden_channels <= 256"):
        CachedPixelSNAILSampler(net)
    with pytest.raises(ValueError, match="hidden_channels <= 256"):
        net.sample(2, 3, 3, "cpu", cached="kv")
    with pytest.raises(ValueError, match="head_dim <= 64"):
        CachedPixelSNAILSampler(PixelSNAIL(16, 8, hidden_channels=128, num_blocks=1, num_res_blocks_per_layer=1, num_heads=1))
    with pytest.raises(ValueError, match="num_embeddings <= 2048"):
        CachedPixelSNAILSampler(PixelSNAIL(4096, 8, hidden_channels=16, num_blocks=1, num_res_blocks_per_layer=1, num_heads=2))
    ok = CachedPixelSNAILSampler(PixelSNAIL(16, 8, hidden_channels=16, num_blocks=1, num_res_blocks_per_layer=1, num_heads=2))
    assert ok.dims() == (10, 8, 16, 1, 1, 2, 8, 16, 7) and ok.draws == 0
