"""Recursive-KL / cycle / recursive-cyclic VAEs (models/recursive_vaes.py) against golden vectors produced by the reference's own
modules (tests/golden/generate_recursive_vaes.py): factory and weight quirks, init replay, the CLI flag on the CPU; forward,
losses, Jacobian rows, the summed and the aggregated step, annealing and graph replay on the GPU."""
import ast

import numpy as np
import pytest
import torch

from conftest import load_golden, meta_of

TAGS = ["recursive_kl_vae_tiny", "cycle_vae_tiny", "rc_vae_tiny", "rc_vae_tiny_bce"]


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def T(a):
    return torch.from_numpy(np.asarray(a))


def _reset_counters():
    from movae_amd.models.recursive_vaes import RecursiveCyclicVAE, RecursiveKLVAE

    RecursiveKLVAE.num_iter = 0
    RecursiveCyclicVAE.num_iter = 0


def build(fx, device=None):
    import movae_amd  # noqa: F401
    from movae_amd.models import get_network

    m = meta_of(fx)
    args = Args(arch=m["arch"], batch_size=int(m["B"]), dataset_size=int(m["dataset_size"]), recons_objective=m["objective"],
                recons_activation=None, loss_weights=[float(v) for v in fx["loss_weights"]], latent_dim=int(m["latent_dim"]),
                hidden_dims=ast.literal_eval(m["hidden_dims"]), recursive_kld_anneal_steps=int(m["recursive_kld_anneal_steps"]))
    torch.manual_seed(int(m["seed"]))
    _reset_counters()
    return get_network(int(m["input_size"]), num_channels=3, args=args, device=device), m


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
    for k in want:
        assert np.array_equal(sd[k].numpy(), fx["sd0." + k]), f"init replay {k}"
    assert net.features is None
    assert list(net.objectives.keys()) == [str(s) for s in fx["objectives"]]
    assert [f"{k}={v!r}" for k, v in net.lambda_weights.items()] == [str(s) for s in fx["lambda_weights"]]
    assert getattr(net, "graph_safe", False)


def test_factory_and_weight_quirks_match_reference():
    import movae_amd  # noqa: F401
    from movae_amd.models import get_network

    q = load_golden("recursive_vaes_quirks")
    assert len(q["case"]) >= 15
    for case, want in zip(q["case"], q["result"]):
        arch, lw = ast.literal_eval(str(case))
        args = Args(arch=arch, batch_size=4, dataset_size=1000, recons_objective="mse", recons_activation=None, loss_weights=lw,
                    latent_dim=4, hidden_dims=[4, 8], recursive_kld_anneal_steps=10)
        try:
            net = get_network(16, num_channels=3, args=args, device=None)
            got = repr({"objectives": list(net.objectives.keys()), "lambda_weights": dict(net.lambda_weights), "features": net.features,
                        "anneal_steps": getattr(net, "anneal_steps", None)})
        except Exception as e:  # noqa: BLE001
            got = f"raises {type(e).__name__}"
        assert got == str(want), case


def test_sphere_encoders_stay_refused():
    import movae_amd  # noqa: F401
    from movae_amd.models import OUT_OF_SCOPE_ARCHS, get_network

    assert OUT_OF_SCOPE_ARCHS == {"sphere_encoder", "sphere_encoder_vit"}
    for arch in sorted(OUT_OF_SCOPE_ARCHS):
        with pytest.raises(NotImplementedError):
            get_network(32, 3, Args(arch=arch, batch_size=4, dataset_size=100, loss_weights=None), None)


def test_recursive_kld_anneal_steps_flag_is_live(capsys):
    import movae_amd  # noqa: F401
    from movae_amd import train
    from movae_amd.models import get_network

    a = train.parse_args(["--arch", "rc_vae", "--recursive_kld_anneal_steps", "7", "--loss_weights", "1.0", "0.00025", "0.00025"])
    assert a.recursive_kld_anneal_steps == 7 and "ignoring" not in capsys.readouterr().out
    a.dataset_size, a.hidden_dims, a.latent_dim = 1000, [4, 8], 4
    assert get_network(16, 3, a, None).anneal_steps == 7
    for arch in ("vae", "recursive_kl_vae", "cycle_vae"):  # parses for every arch; the default is the reference's
        assert train.parse_args(["--arch", arch]).recursive_kld_anneal_steps == 25000


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _gpu_net(fx, dev):
    net, m = build(fx)
    net = net.to(dev).train()
    net.eps_override = T(fx["eps"]).to(dev)
    if "z_prior" in fx.files:
        net.z_prior_override = T(fx["z_prior"]).to(dev)
    return net, m


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_forward_losses_jacobian_rows_sum_step(tag, gpu_device):
    fx = load_golden(tag)
    net, m = _gpu_net(fx, gpu_device)
    x = T(fx["x"]).to(gpu_device)
    out = net(x)
    assert sorted(out.keys()) == sorted(f[4:] for f in fx.files if f.startswith("out."))
    for k in out:
        assert_close(out[k], fx["out." + k], k, rtol=2e-4, atol=2e-5)
    ld = net.loss_function(x, args=out)
    assert list(ld.keys()) == [f[5:] for f in fx.files if f.startswith("loss.")]
    for k, v in ld.items():
        np.testing.assert_allclose(v.item(), fx["loss." + k], rtol=2e-5, atol=1e-7, err_msg=k)
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    comp = [v for k, v in ld.items() if k != "total_loss"]
    for i, v in enumerate(comp):  # the Jacobian rows: a parameter reached two or three times holds the sum of its uses
        gs = torch.autograd.grad(v, params, retain_graph=True, allow_unused=True)
        for n, p, g in zip(names, params, gs):
            assert_close(g if g is not None else torch.zeros_like(p), fx[f"gloss.{i}.{n}"], f"row {i} {n}", rtol=2e-3, atol=1e-5)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    ld["total_loss"].backward()
    for n, p in zip(names, params):
        assert_close(p.grad if p.grad is not None else torch.zeros_like(p), fx["gsum." + n], "grad " + n)
    opt.step()
    sd1 = net.state_dict()
    for k in [f[4:] for f in fx.files if f.startswith("sd1.")]:
        want = fx["sd1." + k]
        if k.endswith("num_batches_tracked"):  # one update per encoder / decoder call
            assert int(sd1[k].item()) == int(want), k
            continue
        noise = ("gsum." + k) in fx.files and np.abs(fx["gsum." + k]).max() < 1e-6
        np.testing.assert_allclose(sd1[k].cpu().numpy(), want, rtol=2e-4, atol=2.1e-3 if noise else 3e-5, err_msg=k)
    ld2 = net.loss_function(x, args=net(x))  # the annealing counter advanced once more
    for k, v in ld2.items():
        np.testing.assert_allclose(v.item(), fx["loss2." + k], rtol=1e-3, atol=2e-6, err_msg="loss2 " + k)
    net.eval()
    with torch.no_grad():
        oe = net(x)
        le = net.loss_function(x, args=oe)
    assert_close(oe["recons"], fx["eval.recons"], "eval recons", rtol=2e-3, atol=5e-3)
    for k, v in le.items():
        np.testing.assert_allclose(v.item(), fx["eval_loss." + k], rtol=5e-2, atol=1e-4, err_msg="eval " + k)


@pytest.mark.gpu
@pytest.mark.parametrize("agg", ["upgrad", "mgda", "aligned_mtl"])
def test_aggregated_step_matches_oracle_on_fixture_jacobian(agg, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import aggregation, train
    from oracle.aggregation import aggregate, make_weighting

    fx = load_golden("rc_vae_tiny")
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
    cond = agg != "upgrad"
    np.testing.assert_allclose(seen["w"].cpu().numpy(), w_want.numpy(), rtol=2e-2 if cond else 1e-3, atol=1e-4)
    off = 0
    for n, p in net.named_parameters():
        want = g_want[off: off + p.numel()].reshape(p.shape).float().numpy()
        off += p.numel()
        assert_close(p.grad if p.grad is not None else torch.zeros_like(p), want, f"{agg} grad {n}", rtol=3e-2 if cond else 2e-3,
                     atol=1e-4 if cond else 1e-5)


@pytest.mark.gpu
def test_device_prior_draw_shares_the_reparameterisation_launch(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    g = torch.Generator().manual_seed(0)
    mu, lv = torch.randn(64, 16, generator=g).to(gpu_device), torch.randn(64, 16, generator=g).to(gpu_device) * 0.1
    s1 = torch.tensor([1234, 5], dtype=torch.int64, device=gpu_device)
    s2 = s1.clone()
    z_ref = ops.reparameterize_rng(mu, lv, s1)
    z, zp = ops.reparameterize_prior_rng(mu, lv, s2, 4096)
    torch.cuda.synchronize()
    assert torch.equal(z, z_ref), "the prior draw changed the reparameterisation noise"
    assert s2.tolist() == [1234, 6] and s1.tolist() == [1234, 6]  # one counter advance for both draws
    assert zp.shape == (4096, 16) and not zp.requires_grad
    v = zp.double()
    assert abs(v.mean().item()) < 0.02 and abs(v.std().item() - 1.0) < 0.02
    eps = ((z_ref - mu) * torch.exp(-0.5 * lv))
    assert (v[:64] - eps).abs().max() > 0.1  # not the same numbers as eps
    _, zp2 = ops.reparameterize_prior_rng(mu, lv, s2, 4096)
    assert not torch.equal(zp, zp2)  # the next draw number gives fresh samples


@pytest.mark.gpu
def test_annealing_counter_eager_and_device(gpu_device):
    """Eager: the class counter advances per training-mode loss_function call (separately per class), eval uses 1.  Graph mode: the
    device counter, seeded from the class value, advances inside the loss kernel and gives the same losses."""
    from movae_amd.models.recursive_vaes import RecursiveCyclicVAE, RecursiveKLVAE

    fx = load_golden("rc_vae_tiny")
    x = T(fx["x"]).to(gpu_device)
    net, m = _gpu_net(fx, gpu_device)
    steps = int(m["recursive_kld_anneal_steps"])
    twin, _ = _gpu_net(fx, gpu_device)
    RecursiveKLVAE.num_iter = 100
    with torch.no_grad():
        out = net(x)
        base = net.loss_function(x, args=out)["recursive_kld_loss"].item()  # num_iter 1
        assert RecursiveCyclicVAE.num_iter == 1 and RecursiveKLVAE.num_iter == 100
        twin.prepare_for_graph()  # device counter from the class value (1)
        assert twin._iter_dev.item() == 1.0
        for it in range(2, steps + 3):
            want = base * steps * min(it / steps, 1.0)  # (base carries the factor 1 / steps)
            got_e = net.loss_function(x, args=out)["recursive_kld_loss"].item()
            got_d = twin.loss_function(x, args=out)["recursive_kld_loss"].item()
            np.testing.assert_allclose([got_e, got_d], [want, want], rtol=1e-5, err_msg=f"iter {it}")
        assert RecursiveCyclicVAE.num_iter == steps + 2 and twin._iter_dev.item() == steps + 2
        net.eval()
        ev = net.loss_function(x, args=out)["recursive_kld_loss"].item()
        assert RecursiveCyclicVAE.num_iter == steps + 2
    RecursiveKLVAE.num_iter = 0
    assert ev != 0.0


GRAPH_CASES = {"rc_vae": ([1.0, 0.05, 0.02], "upgrad"), "cycle_vae": ([1.0, 0.05], "mgda"), "recursive_kl_vae": ([1.0, 0.05], "aligned_mtl"),
               "rc_vae-sum": ([1.0, 0.05, 0.02], "sum")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GRAPH_CASES))
def test_hipgraph_replay_matches_eager_steps(case, gpu_device):
    """GraphedTrainStep captures the whole step (three encoder and two decoder passes, the K-row Jacobian over all parameters,
    Gram / solve / combine, Adam) and replays it like the eager loop, with the annealing counter on the device."""
    import movae_amd  # noqa: F401
    from movae_amd import aggregation
    from movae_amd.models import get_network
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    arch = case.split("-")[0]
    lw, agg = GRAPH_CASES[case]

    def make():
        a = Args(arch=arch, batch_size=16, dataset_size=1000, recons_objective="mse", recons_activation=None, loss_weights=list(lw),
                 latent_dim=8, hidden_dims=[16, 32], recursive_kld_anneal_steps=5, aggregator=agg, agg_norm_eps=1e-4, agg_reg_eps=1e-4,
                 mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None, optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None)
        torch.manual_seed(3)
        _reset_counters()
        net = get_network(32, 3, a, gpu_device).to(gpu_device).train()
        g = torch.Generator().manual_seed(5)
        net.eps_override = torch.randn(16, 8, generator=g).to(gpu_device)
        net.z_prior_override = torch.randn(16, 8, generator=g).to(gpu_device)
        return net, a

    g = torch.Generator().manual_seed(11)
    batches = [torch.rand(16, 3, 32, 32, generator=g).to(gpu_device) for _ in range(4)]
    net_e, a = make()
    opt_e = make_optimizer(net_e, a, capturable=True)
    agg_e = aggregation.make_aggregator(a)
    for _ in range(3):  # the graphed twin's warm-up steps
        train_step(net_e, batches[0], opt_e, agg_e, a)
    eager = [train_step(net_e, b, opt_e, agg_e, a)[0]["total_loss"].item() for b in batches]
    net_g, a2 = make()
    opt_g = make_optimizer(net_g, a2, capturable=True)
    gs = GraphedTrainStep(net_g, opt_g, aggregation.make_aggregator(a2), a2, batches[0])
    graphed = [gs.step(b)[0]["total_loss"].item() for b in batches]
    np.testing.assert_allclose(graphed, eager, rtol=2e-5)
    if arch != "cycle_vae":
        assert net_g._iter_dev.item() == 7.0  # 3 warm-up steps + 4 replays (the capture pass records, it does not run)
    for (n, p), (_, q) in zip(net_e.named_parameters(), net_g.named_parameters()):
        got, want = q.detach().cpu().numpy(), p.detach().cpu().numpy()
        # the annealing factor is fp32 on the device and a Python double in the eager loop; Adam turns rounding noise in a
        # near-zero gradient into a step of up to +-lr: a handful of entries may differ by a fraction of one step
        bad = np.abs(got - want) > 2e-5 + 2e-3 * np.abs(want)
        assert bad.mean() <= 1e-3 and np.abs(got - want).max() < 5e-4, f"{n}: {int(bad.sum())} of {bad.size} off"


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["off", "on"])
def test_cli_training_rc_vae(graph, gpu_device, tmp_path, capsys):
    import movae_amd  # noqa: F401
    from movae_amd import train

    argv = ["--dataset", "synthetic_cifar10", "--arch", "rc_vae", "--loss_weights", "1.0", "0.00025", "0.00025", "--agg", "upgrad",
            "--batch_size", "64", "--epochs", "2", "--max_items", "512", "--seed", "3", "--latent_dim", "16", "--hidden_dims", "16", "32",
            "64", "--recursive_kld_anneal_steps", "4", "--graph", graph, "--save_path", str(tmp_path), "--device", "cuda:0",
            "--max_fid_samples", "64"]
    hist = train.main(train.parse_args(argv))
    out = capsys.readouterr().out
    assert len(hist) == 2 and all(np.isfinite([v for k, v in h.items() if k != "kld_loss"]).all() for h in hist)
    assert list(hist[0].keys()) == ["reconstruction_loss", "kld_loss", "recursive_kld_loss", "cycle_loss", "total_loss"]
    assert hist[1]["reconstruction_loss"] < hist[0]["reconstruction_loss"]
    assert out.count("HV:") >= 2 and "final:" in out and "psnr" in out
    _reset_counters()


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["rc_vae", "recursive_kl_vae", "cycle_vae"])
def test_batched_jacobian_matches_sequential_passes(arch, gpu_device, monkeypatch):
    """autojac.backward_through with MOVAE_BATCHED_FULL_JACOBIAN=1 (the K loss cotangents of the loss kernel's inputs pulled back
    through the whole network in one traversal: recons is a root and an interior node of mu_hat's graph, the encoder is walked three times with per-group
    BatchNorm statistics, reused parameters sum their uses) fills the same Jacobian as one torch.autograd pass per loss."""
    import movae_amd  # noqa: F401
    from movae_amd import aggregation, autojac, train
    from movae_amd.models import get_network

    lw = {"rc_vae": [1.0, 0.3, 0.2], "recursive_kl_vae": [1.0, 0.3], "cycle_vae": [1.0, 0.2]}[arch]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(16, 3, 32, 32, generator=g).to(gpu_device)
    eps, zp = torch.randn(16, 16, generator=g).to(gpu_device), torch.randn(16, 16, generator=g).to(gpu_device)
    walked = []
    real = autojac._batched_pullback

    def spy(*a, **k):
        real(*a, **k)
        walked.append(len(a[2]))

    monkeypatch.setattr(autojac, "_batched_pullback", spy)
    rows, grads = {}, {}
    for batched in (True, False):
        monkeypatch.setattr(autojac, "BATCHED_FULL_JACOBIAN", batched)
        a = Args(arch=arch, batch_size=16, dataset_size=1000, recons_objective="mse", recons_activation=None, loss_weights=list(lw),
                 latent_dim=16, hidden_dims=[16, 32, 64], recursive_kld_anneal_steps=3)
        torch.manual_seed(4)
        _reset_counters()
        net = get_network(32, 3, a, gpu_device).to(gpu_device).train()
        net.eps_override, net.z_prior_override = eps, zp
        seen = {}
        A = aggregation.make_aggregator(Args(aggregator="upgrad", agg_norm_eps=1e-4, agg_reg_eps=1e-4, pref_weights=None))
        A.weighting.register_forward_hook(lambda mod, inp, o: seen.update(J=inp[0].clone()))
        train.forward_backward(net, x, torch.optim.SGD(net.parameters(), lr=0.0), A)
        rows[batched] = seen["J"].cpu()
        grads[batched] = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()
    assert walked == [len(lw)], walked  # the batched form ran (once, all K rows) and did not fall back
    assert rows[True].shape == rows[False].shape
    scale = float(rows[False].abs().max())
    np.testing.assert_allclose(rows[True].numpy(), rows[False].numpy(), rtol=1e-4, atol=1e-6 * max(scale, 1.0))
    np.testing.assert_allclose(grads[True].numpy(), grads[False].numpy(), rtol=1e-4, atol=1e-6 * float(grads[False].abs().max()))
    _reset_counters()
