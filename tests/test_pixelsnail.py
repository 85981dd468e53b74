"""PixelSNAIL prior (reference models/pixelcnn_prior.py:95-259, :434-555; main.py:906-1048).

CPU: the constructor / state_dict surface and init replay against fixtures recorded from the reference's own classes, and the
prior-stage flag mapping.  GPU: the fused causal attention (csrc/attention.hip) against a float64 restatement of the reference's
expression, its dropout mask, the flat and hierarchical models against the fixtures through one optimizer step, and the prior stage
on tiny VQ models."""
import math
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, meta_of

SHAPES = [(2, 2, 64, 8), (2, 8, 256, 16), (1, 8, 1024, 16), (1, 2, 4096, 16), (3, 2, 35, 8), (2, 4, 36, 12), (2, 1, 1, 16)]


# ---------------------------------------------------------------------------------------------------------------------------
# float64 restatement of CausalAttention2d.forward between the projections (pixelcnn_prior.py:118-131)
def ref_attention(q, k, v, heads, keep=None, p=0.0):
    """q, k, v [B, L, proj] (head h at channels h*hd ..) -> [B, L, proj] with (h, d) at channel d*heads + h."""
    B, n, proj = q.shape
    hd = proj // heads

    def split(t):  # the reference's .view(B, heads, hd, L).permute(0, 1, 3, 2) of an NCHW conv output
        return t.reshape(B, n, heads, hd).permute(0, 2, 1, 3)

    attn = torch.matmul(split(q), split(k).transpose(-2, -1)) / math.sqrt(hd)
    mask = torch.tril(torch.ones(n, n, dtype=torch.bool))
    attn = attn.masked_fill(~mask, float("-inf")).softmax(-1)
    if keep is not None:
        attn = attn * keep.reshape(B, heads, n, n).to(attn.dtype) / (1.0 - p)
    out = torch.matmul(attn, split(v))  # [B, heads, L, hd]
    return out.permute(0, 2, 3, 1).reshape(B, n, proj)


def _inputs(B, heads, n, hd, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * n + hd)
    q, k, v = (torch.randn(B, n, heads * hd, generator=g) for _ in range(3))
    do = torch.randn(B, n, heads * hd, generator=g)
    return q, k, v, do


def _check(got, want, what, rtol=1e-4, atol_frac=2e-5):
    """fp32 against float64; the inputs are O(1), so the absolute floor is O(1) too (at L = 1 dQ and dK are exact zeros in float64
    and fp32 rounding of dP - D)."""
    want = want.detach().numpy()
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want, rtol=rtol,
                               atol=atol_frac * max(1.0, float(np.abs(want).max())), err_msg=what)


def _run_fused(q, k, v, do, heads, dev, p=0.0, seed=0, draw=0):
    from movae_amd import ops

    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    o = ops.causal_attention(qd, kd, vd, heads, p, seed, draw)
    o.backward(do.to(dev))
    torch.cuda.synchronize()
    return o.detach(), qd.grad, kd.grad, vd.grad


def _run_ref(q, k, v, do, heads, keep=None, p=0.0):
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o = ref_attention(qr, kr, vr, heads, keep, p)
    o.backward(do.double())
    return o.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.gpu
@pytest.mark.parametrize("B,heads,n,hd", SHAPES)
def test_fused_attention_matches_reference_expression(B, heads, n, hd, gpu_device):
    import movae_amd  # noqa: F401

    q, k, v, do = _inputs(B, heads, n, hd)
    got = _run_fused(q, k, v, do, heads, gpu_device)
    want = _run_ref(q, k, v, do, heads)
    for name, a, b in zip(("O", "dQ", "dK", "dV"), got, want):
        assert tuple(a.shape) == tuple(b.shape) == (B, n, heads * hd)
        _check(a, b, f"{name} {(B, heads, n, hd)}")
    again = _run_fused(q, k, v, do, heads, gpu_device)
    for name, a, b in zip(("O", "dQ", "dK", "dV"), got, again):
        assert torch.equal(a, b), f"{name} differs between two identical calls"


@pytest.mark.gpu
def test_output_channel_order_is_d_times_heads_plus_h(gpu_device):
    """With V constant per (head, dim), O is that constant wherever the row attends: channel d*heads + h must carry V's value
    of head h, dim d (the reference's permute(0, 2, 3, 1).reshape), not channel h*hd + d."""
    import movae_amd  # noqa: F401
    from movae_amd import ops

    B, heads, n, hd = 2, 2, 40, 8
    q, k, _, _ = _inputs(B, heads, n, hd)
    val = torch.arange(heads * hd, dtype=torch.float32)  # channel h*hd + d of V holds h*hd + d
    v = val.expand(B, n, heads * hd).contiguous()
    o = ops.causal_attention(q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), heads).cpu()
    for h in range(heads):
        for d in range(hd):
            torch.testing.assert_close(o[..., d * heads + h], torch.full((B, n), float(h * hd + d)), rtol=1e-6, atol=1e-5)


@pytest.mark.gpu
def test_head_dim_limit_is_named(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    q = torch.randn(1, 8, 65, device=gpu_device)
    with pytest.raises(RuntimeError, match="64"):
        ops.causal_attention(q, q, q, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,heads,n,hd", [(2, 2, 64, 8), (2, 4, 36, 12), (1, 8, 256, 16)])
def test_dropout_matches_reference_with_the_kernels_mask(B, heads, n, hd, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    p, seed, draw = 0.1, 1234, 5
    q, k, v, do = _inputs(B, heads, n, hd, seed=3)
    keep = ops.causal_attention_dropout_mask(B * heads, n, p, seed, draw, gpu_device).cpu()
    got = _run_fused(q, k, v, do, heads, gpu_device, p, seed, draw)
    want = _run_ref(q, k, v, do, heads, keep, p)
    for name, a, b in zip(("O", "dQ", "dK", "dV"), got, want):
        _check(a, b, f"dropout {name} {(B, heads, n, hd)}")
    again = _run_fused(q, k, v, do, heads, gpu_device, p, seed, draw)
    for name, a, b in zip(("O", "dQ", "dK", "dV"), got, again):
        assert torch.equal(a, b), name


@pytest.mark.gpu
def test_dropout_mask_statistics_and_reseeding(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    bh, n, p = 16, 256, 0.1
    m0 = ops.causal_attention_dropout_mask(bh, n, p, 42, 0, gpu_device)
    m1 = ops.causal_attention_dropout_mask(bh, n, p, 42, 1, gpu_device)
    total = bh * n * n
    frac = m0.double().mean().item()
    sd = math.sqrt(p * (1 - p) / total)
    assert abs(frac - (1 - p)) < 6 * sd, frac  # binomial bounds
    assert not torch.equal(m0, m1)  # consecutive draws differ
    assert torch.equal(m0, ops.causal_attention_dropout_mask(bh, n, p, 42, 0, gpu_device))  # re-seeding repeats
    assert not torch.equal(m0, ops.causal_attention_dropout_mask(bh, n, p, 43, 0, gpu_device))
    assert set(torch.unique(m0).tolist()) == {0, 1}
    assert torch.equal(ops.causal_attention_dropout_mask(bh, n, 0.0, 42, 0, gpu_device), torch.ones_like(m0))


# ---------------------------------------------------------------------------------------------------------------------------
# models against the reference's own classes (tests/golden/generate_pixelsnail.py)
def _meta():
    fx = load_golden("pixelsnail_tiny")
    m = {k: (float(v) if k == "lr" else int(v)) for k, v in meta_of(fx).items()}
    return fx, m


def _build(tag, device, dropout=0.0):
    import movae_amd  # noqa: F401
    from movae_amd.models import HierarchicalPixelSNAIL, PixelSNAIL

    fx, m = _meta()
    K, D, hid, nb, nr, nh = (m[k] for k in ("num_embeddings", "embedding_dim", "hidden_channels", "num_blocks",
                                            "num_res_blocks_per_layer", "num_heads"))
    torch.manual_seed(m["seed"] + (1 if tag == "eval" else 0))
    if tag == "hier":
        net = HierarchicalPixelSNAIL(K, D, hid, num_blocks_top=nb, num_res_blocks_per_layer=nr, num_heads=nh,
                                     num_layers_bottom=m["num_layers_bottom"], dropout=dropout)
    elif tag == "eval":
        net = PixelSNAIL(K, D, hid, num_blocks=nb, num_res_blocks_per_layer=nr, num_heads=nh)
    else:
        net = PixelSNAIL(K, D, hid, num_blocks=nb, num_res_blocks_per_layer=nr, num_heads=nh, dropout=dropout)
    return fx, m, net.to(device)


def _keys(fx, prefix):
    return [k[len(prefix):] for k in fx.files if k.startswith(prefix)]


@pytest.mark.parametrize("tag", ["flat", "hier", "eval"])
def test_state_dict_surface_and_init_replay(tag):
    """Constructor signatures, state_dict keys / order / shapes and the init RNG sequence (CPU: no kernel runs)."""
    fx, _, net = _build(tag, "cpu", dropout=0.1 if tag == "eval" else 0.0)
    keys = _keys(fx, f"{tag}.sd0.")
    sd = net.state_dict()
    assert list(sd.keys()) == keys
    for k in keys:
        want = fx[f"{tag}.sd0.{k}"]
        assert tuple(sd[k].shape) == want.shape and np.array_equal(sd[k].numpy(), want), k
    if tag != "eval":
        net.load_state_dict({k: torch.from_numpy(fx[f"{tag}.sd1.{k}"]) for k in keys})  # a reference checkpoint loads


def test_causal_attention_module_surface():
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import CausalAttention2d

    a = CausalAttention2d(128)
    assert (a.num_heads, a.head_dim, a.proj_dim, a.dropout.p) == (8, 16, 128, 0.1)
    assert [n for n, _ in a.named_children()] == ["q_proj", "k_proj", "v_proj", "out_proj", "dropout"]
    b = CausalAttention2d(10, num_heads=4, head_dim=6, dropout=0.0)
    assert (b.proj_dim, tuple(b.q_proj.weight.shape), tuple(b.out_proj.weight.shape)) == (24, (24, 10, 1, 1), (10, 24, 1, 1))
    with pytest.raises(AssertionError, match="divisible"):
        CausalAttention2d(10, num_heads=4)


def _snail_args(arch, **kw):
    a = dict(arch=arch, pixelcnn_hidden_channels=24, pixelcnn_num_layers=3, pixelsnail_num_blocks=3, pixelsnail_num_res_blocks=1,
             pixelsnail_num_heads=4, pixelsnail_dropout=0.25)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_build_pixelsnail_prior_maps_the_flags():
    """main.py:917-944: hidden channels, blocks, residual blocks, heads, dropout; the bottom PixelCNN's depth from
    --pixelcnn_num_layers; flat or hierarchical by arch."""
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd.models import HierarchicalPixelSNAIL, PixelCNN, PixelSNAIL

    vq = types.SimpleNamespace(num_embeddings=12, embedding_dim=6)
    flat = P.build_pixelsnail_prior(vq, _snail_args("vq_vae"), "cpu")
    assert type(flat) is PixelSNAIL and (flat.num_embeddings, flat.embedding_dim) == (12, 6)
    assert len(flat.blocks) == 3 and all(len(b.res_blocks) == 1 for b in flat.blocks)
    att = flat.blocks[0].attention
    assert (att.num_heads, att.head_dim, att.dropout.p) == (4, 6, 0.25)
    assert tuple(flat.conv_in.weight.shape) == (24, 6 + 2, 7, 7)
    for arch in ("vq_vae2", "gg_vq_vae2"):
        hier = P.build_pixelsnail_prior(vq, _snail_args(arch), "cpu")
        assert type(hier) is HierarchicalPixelSNAIL
        assert type(hier.prior_top) is PixelSNAIL and len(hier.prior_top.blocks) == 3
        assert type(hier.prior_bottom) is PixelCNN and len(hier.prior_bottom.res_blocks) == 3
        assert tuple(hier.prior_bottom.conv_in.weight.shape) == (24, 12, 7, 7)
    dflt = P.build_pixelsnail_prior(vq, types.SimpleNamespace(arch="vq_vae"), "cpu")  # the reference's defaults
    assert len(dflt.blocks) == 8 and len(dflt.blocks[0].res_blocks) == 2
    assert (dflt.blocks[0].attention.num_heads, dflt.blocks[0].attention.dropout.p) == (8, 0.1)


def test_build_prior_still_refuses_pixelsnail():
    import movae_amd  # noqa: F401
    from movae_amd import prior as P

    vq = types.SimpleNamespace(num_embeddings=12, embedding_dim=6)
    args = _snail_args("vq_vae", prior_type="pixelsnail")
    with pytest.raises(NotImplementedError):
        P.build_prior(vq, args, "cpu")  # the CLI switch stays off; the model is reached through build_pixelsnail_prior
    assert P.build_pixelsnail_prior(vq, args, "cpu").total_trainable_params() > 0


def _codes(fx, tag, dev):
    if tag == "hier":
        return torch.from_numpy(fx["z_top"]).to(dev), torch.from_numpy(fx["z_bottom"]).to(dev)
    return torch.from_numpy(fx["z"]).to(dev), None


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["flat", "hier"])
def test_hip_pixelsnail_forward_backward_and_step(tag, gpu_device):
    """The tolerances of test_prior.py::test_hip_prior_forward_backward_and_step."""
    from movae_amd.optim import FusedAdam, clip_grad_norm_

    fx, m, net = _build(tag, gpu_device)
    net.train()
    zt, zb = _codes(fx, tag, gpu_device)
    K = m["num_embeddings"]
    if tag == "hier":
        o = net(zt, zb)
        ld = net.loss_function(zt, zb)
        for k in ("logits_top", "logits_bottom"):
            assert tuple(o[k].shape) == fx[f"{tag}.{k}"].shape
            np.testing.assert_allclose(o[k].detach().cpu().numpy(), fx[f"{tag}.{k}"], rtol=2e-4, atol=2e-5, err_msg=k)
    else:
        logits = net(zt)
        assert tuple(logits.shape) == fx[f"{tag}.logits"].shape  # [B, K, 6, 7]
        np.testing.assert_allclose(logits.detach().cpu().numpy(), fx[f"{tag}.logits"], rtol=2e-4, atol=2e-5)
        ref_expr = torch.nn.functional.cross_entropy(logits.permute(0, 2, 3, 1).reshape(-1, K).detach(), zt.reshape(-1))
        ld = {"total_loss": net.loss(zt)}
        np.testing.assert_allclose(ld["total_loss"].item(), ref_expr.item(), rtol=1e-6)
    assert list(ld.keys()) == _keys(fx, f"{tag}.loss.")
    for k, v in ld.items():
        np.testing.assert_allclose(v.item(), fx[f"{tag}.loss.{k}"], rtol=2e-5, err_msg=k)
    opt = FusedAdam(net.parameters(), lr=m["lr"], weight_decay=0.0)
    opt.zero_grad()
    ld["total_loss"].backward()
    for n, p in net.named_parameters():
        want = fx[f"{tag}.g.{n}"]
        got = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-5 * max(1e-3, float(np.abs(want).max())), err_msg="grad " + n)
    gn = clip_grad_norm_(net.parameters(), max_norm=1.0)
    np.testing.assert_allclose(float(gn), float(fx[f"{tag}.gnorm"]), rtol=1e-4)
    opt.step()
    ld2 = net.loss_function(zt, zb) if tag == "hier" else {"total_loss": net.loss(zt)}
    for k, v in ld2.items():
        np.testing.assert_allclose(v.item(), fx[f"{tag}.loss2.{k}"], rtol=5e-5, err_msg="loss2 " + k)
    sd1 = net.state_dict()
    for k in _keys(fx, f"{tag}.sd1."):
        np.testing.assert_allclose(sd1[k].detach().cpu().numpy(), fx[f"{tag}.sd1.{k}"], rtol=2e-4, atol=2e-6, err_msg="sd1 " + k)


@pytest.mark.gpu
def test_eval_mode_uses_no_dropout(gpu_device):
    """A model built with the default dropout 0.1 gives the reference's eval-mode logits, and the same ones twice; in training
    mode its logits differ from call to call (fresh masks) and a re-seeded model repeats them."""
    fx, _, net = _build("eval", gpu_device)
    zt, _ = _codes(fx, "eval", gpu_device)
    net.eval()
    with torch.no_grad():
        a, b = net(zt), net(zt)
    np.testing.assert_allclose(a.cpu().numpy(), fx["eval.logits"], rtol=2e-4, atol=2e-5)
    assert torch.equal(a, b)
    net.train()
    with torch.no_grad():
        t1, t2 = net(zt).clone(), net(zt).clone()
    assert not torch.equal(t1, t2) and not torch.equal(t1, a)
    _, _, net2 = _build("eval", gpu_device)  # same torch.manual_seed: the same sequence of masks
    net2.train()
    with torch.no_grad():
        assert torch.equal(net2(zt), t1)


def _stage_argv(arch, tmp_path):
    return ["--dataset", "synthetic_cifar10", "--arch", arch, "--embedding_dim", "8", "--num_embeddings", "16", "--hidden_dims", "16",
            "32", "--batch_size", "32", "--max_items", "128", "--epochs", "1", "--pixelcnn_epochs", "6", "--pixelcnn_hidden_channels",
            "16", "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3", "--save_path", str(tmp_path), "--seed", "1", "--device",
            "cuda:0", "--eval_freq", "0", "--pixelsnail_num_blocks", "2", "--pixelsnail_num_res_blocks", "1", "--pixelsnail_num_heads",
            "2"]


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["vq_vae", "vq_vae2"])
def test_pixelsnail_prior_stage(arch, gpu_device, tmp_path):
    """main.py:890-1085 with a PixelSNAIL prior: codes of a (frozen) tiny VQ model, a few epochs (the loss falls), checkpoints
    under pixelsnail_prior/ with the reference's keys, and decoded samples."""
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train
    from movae_amd.models import get_network

    args = train.parse_args(_stage_argv(arch, tmp_path))
    train.set_seed(args.seed)
    train_ds, _, input_size = train.get_dataset(args.dataset, data_dir=args.data_dir, normalize=args.normalize_inputs,
                                                max_items=args.max_items)
    loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, shuffle=True)
    net = get_network(input_size, num_channels=3, args=args, device=gpu_device).to(gpu_device)  # a frozen, untrained VQ model
    prior = P.build_pixelsnail_prior(net, args, gpu_device)
    want_keys = list(prior.state_dict().keys())
    out = P.train_pixelcnn_prior(net, loader, gpu_device, args, str(tmp_path), prior=prior)
    assert out is prior and not prior.training
    rec = P.LAST_RUN
    assert rec["use_cache"] and rec["n_codes"] == 128 and len(rec["epoch_losses"]) == 6
    levels = 2 if arch == "vq_vae2" else 1  # the hierarchical loss is the sum of two cross-entropies
    assert rec["epoch_losses"][-1] < rec["epoch_losses"][0] < levels * np.log(16) * 1.2
    for name in ("best_prior.pth", "final_prior.pth"):
        ck = tmp_path / "pixelsnail_prior" / "checkpoints" / name
        assert ck.exists(), name
        assert list(torch.load(ck, map_location="cpu")["model_state_dict"].keys()) == want_keys
    assert not (tmp_path / "pixelcnn_prior").exists()
    imgs = rec["samples"]
    assert tuple(imgs.shape) == (4, 3, 32, 32) and torch.isfinite(imgs).all()
