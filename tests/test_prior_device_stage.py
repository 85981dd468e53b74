"""Prior stage on the device: movae_codes_batch exactly against store[idx].long(), prior.DeviceCodeLoader
against data.shard_indices, prior.GraphedPriorStep against the eager step on a twin, and the two new flags through train.main."""
import math

import numpy as np
import pytest
import torch

N = 37


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _store(shape, dtype, seed):
    """[N, *shape] codes over the whole non-negative range of `dtype`, its largest value included."""
    top = torch.iinfo(dtype).max
    t = torch.randint(0, top + 1, (N,) + shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    t[0, 0, 0], t[N - 1, -1, -1] = top, top
    return t.to(dtype)


def _dataset(hier, dtype=torch.int16):
    from movae_amd.prior import VQCodeDataset

    if hier:
        return VQCodeDataset((_store((4, 4), dtype, 1), _store((8, 8), dtype, 2)), True)
    return VQCodeDataset((_store((8, 8), dtype, 2),), False)


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------
def test_loader_indices_follow_shard_indices_and_len():
    import movae_amd  # noqa: F401
    from movae_amd.data import shard_indices
    from movae_amd.prior import DeviceCodeLoader

    ld = DeviceCodeLoader(_dataset(False), 8, "cuda:0", shuffle=True, seed=3)
    assert len(ld) == math.ceil(N / 8) == 5
    e1, e2 = ld.indices(1), ld.indices(2)
    assert e1 == shard_indices(N, True, 3, 1) and e2 == shard_indices(N, True, 3, 2)
    assert e1 != e2 and sorted(e1) == sorted(e2) == list(range(N))
    ld.set_epoch(2)
    assert ld.indices() == e2
    assert DeviceCodeLoader(_dataset(True), 8, "cuda:0", shuffle=False).indices(5) == list(range(N))


def test_flags_parse_with_defaults_and_reject_other_values():
    import movae_amd  # noqa: F401
    from movae_amd import train

    base = ["--dataset", "synthetic_cifar10", "--arch", "vq_vae"]
    a = train.parse_args(base)
    assert (a.prior_loader, a.prior_step) == ("host", "eager")
    a = train.parse_args(base + ["--prior_loader", "device", "--prior_step", "graph"])
    assert (a.prior_loader, a.prior_step) == ("device", "graph")
    for bad in (["--prior_loader", "gpu"], ["--prior_step", "replay"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)


def test_row_outside_the_store_is_refused_on_the_host(monkeypatch):
    import movae_amd  # noqa: F401
    from movae_amd import ops
    from movae_amd.prior import DeviceCodeLoader

    def no_launch(*a, **k):
        raise AssertionError("a launch was attempted")

    monkeypatch.setattr(ops, "_call", no_launch)
    store = _store((4, 4), torch.int16, 1)
    for rows in ([0, N], [3, -1], torch.tensor([N + 5], dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.codes_batch(store, rows)
    ld = DeviceCodeLoader(_dataset(False), 8, "cuda:0")
    monkeypatch.setattr(ld, "indices", lambda epoch=None: [0, 1, N])
    with pytest.raises(ValueError):
        next(iter(ld))


def test_bare_namespace_selects_host_and_eager():
    import movae_amd  # noqa: F401
    from movae_amd.prior import prior_modes

    assert prior_modes(Args(batch_size=8)) == ("host", "eager")
    assert prior_modes(Args(prior_loader="device", prior_step="graph")) == ("device", "graph")
    with pytest.raises(ValueError):
        prior_modes(Args(prior_loader="gpu"))


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
ROWS = {
    "b8": [0, N - 1, 5, 5, 20, 5, N - 1, 0],   # repeats, rows 0 and N - 1
    "b5": [N - 1, 30, 17, 4, 0],               # descending
}


@pytest.mark.gpu
@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("dtype", [torch.int16, torch.int32], ids=["int16", "int32"])
@pytest.mark.parametrize("grids", [((4, 4),), ((8, 8),), ((3, 5),), ((4, 4), (8, 8)), ((3, 5), (8, 8))],
                         ids=["4x4", "8x8", "3x5", "4x4+8x8", "3x5+8x8"])
def test_codes_batch_equals_indexing(grids, dtype, rows, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    stores = [_store(g, dtype, 7 + i).to(gpu_device) for i, g in enumerate(grids)]
    idx = torch.tensor(ROWS[rows], dtype=torch.int32, device=gpu_device)
    want = [s[idx.long()].long() for s in stores]
    got = ops.codes_batch(stores[0], idx, stores[1] if len(stores) == 2 else None)
    got = list(got) if len(stores) == 2 else [got]
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and g.shape == w.shape and torch.equal(g, w)
    assert int(want[0].max()) == torch.iinfo(dtype).max  # (the largest code of the width went through)
    # caller-supplied buffers are written in place
    bufs = [torch.full_like(w, -1) for w in want]
    ptrs = [b.data_ptr() for b in bufs]
    out = ops.codes_batch(stores[0], idx, stores[1] if len(stores) == 2 else None, out_top=bufs[0],
                          out_bottom=bufs[1] if len(stores) == 2 else None)
    out = list(out) if len(stores) == 2 else [out]
    for o, b, p, w in zip(out, bufs, ptrs, want):
        assert o is b and o.data_ptr() == p and torch.equal(b, w)
    # a host row list is checked, uploaded and gives the same batch
    assert torch.equal(ops.codes_batch(stores[0], ROWS[rows]), want[0])


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hier", [False, True], ids=["flat", "hier"])
def test_loader_visits_every_grid_once_in_index_order(hier, gpu_device, monkeypatch):
    import movae_amd  # noqa: F401
    from movae_amd import ops
    from movae_amd.prior import DeviceCodeLoader

    ds = _dataset(hier)
    ld = DeviceCodeLoader(ds, 8, gpu_device, shuffle=True, seed=4)
    launches = []
    real = ops.codes_batch
    monkeypatch.setattr(ops, "codes_batch", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    for epoch in (1, 2):
        ld.set_epoch(epoch)
        batches = list(ld)
        assert len(batches) == len(ld) == 5 and len(launches) == 5 * epoch
        order = torch.tensor(ld.indices(epoch))
        levels = list(zip(*batches)) if hier else [batches]
        for store, parts in zip((ds.z_top, ds.z_bottom) if hier else (ds.z,), levels):
            assert [p.size(0) for p in parts] == [8, 8, 8, 8, 5] and all(p.dtype == torch.int64 and p.is_cuda for p in parts)
            got = torch.cat(parts).cpu()
            assert torch.equal(got, store[order].long())  # the batches follow indices(e) in order
            flat = lambda t: sorted(map(tuple, t.reshape(t.size(0), -1).tolist()))  # noqa: E731
            assert flat(got) == flat(store.long())  # a permutation of the store: every grid exactly once


@pytest.mark.gpu
def test_extract_codes_on_device_keeps_the_dataset_contract(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd.prior import extract_codes

    class Net(torch.nn.Module):
        num_embeddings = 16

        def get_code_indices(self, images):
            return (images[:, 0, :4, :4] * 15.99).long()

    imgs = torch.rand(20, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    loader = [(imgs[:8], 0), (imgs[8:16], 0), (imgs[16:], 0)]
    host = extract_codes(Net(), loader, gpu_device, False)
    dev = extract_codes(Net(), loader, gpu_device, False, on_device=True)
    assert not host.z.is_cuda and dev.z.is_cuda and dev.z.dtype == host.z.dtype == torch.int16
    assert len(dev) == len(host) == 20 and torch.equal(dev.z.cpu(), host.z)
    item = dev[7]
    assert item.is_cuda and item.dtype == torch.int64 and torch.equal(item.cpu(), host[7])
    with pytest.raises(IndexError):
        dev[20]


# ---- the captured step ---------------------------------------------------------------------------------------------------------------
def _twin(hier, device):
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelCNN, PixelCNN
    from movae_amd.optim import FusedAdam

    torch.manual_seed(3)
    net = (HierarchicalPixelCNN(16, 8, 16, 2) if hier else PixelCNN(16, 8, hidden_channels=16, num_layers=2)).to(device).train()
    return net, FusedAdam(net.parameters(), lr=3e-3, weight_decay=0.0, device_step=True)


def _batches(hier, device):
    g = torch.Generator().manual_seed(11)
    mk = lambda b: tuple(torch.randint(0, 16, (b, s, s), generator=g).to(device) for s in ((4, 8) if hier else (8,)))  # noqa: E731
    return [mk(16) for _ in range(4)] + [mk(5)]


def _assert_params_agree(net_e, net_g):
    for (n, p), (_, q) in zip(net_e.named_parameters(), net_g.named_parameters()):
        np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().cpu().numpy(), rtol=1e-4, atol=2e-6, err_msg=n)


@pytest.mark.gpu
@pytest.mark.parametrize("hier", [False, True], ids=["flat", "hier"])
def test_graphed_prior_step_matches_eager_twin(hier, gpu_device):
    """Four full batches replay, the learning rate changes after step 2, a ragged fifth batch takes the eager branch; the first
    replay equals the eager twin's first step from the initial state (the warm-up was rewound)."""
    import movae_amd  # noqa: F401
    from movae_amd.prior import GraphedPriorStep, _one_step

    batches = _batches(hier, gpu_device)
    net_e, opt_e = _twin(hier, gpu_device)
    net_g, opt_g = _twin(hier, gpu_device)
    gs = GraphedPriorStep(net_g, opt_g, *batches[0])
    for (n, p), (_, q) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(p, q), f"warm-up not rewound: {n}"
    eager, graph, worst = [], [], 0.0
    for i, b in enumerate(batches):
        le, lg = _one_step(net_e, opt_e, *b), gs.step(*b)
        eager.append(le.item())
        graph.append(lg.item())
        if i == 0:  # step 1 of both twins, from the same initial state
            np.testing.assert_allclose(graph[0], eager[0], rtol=2e-5)
            _assert_params_agree(net_e, net_g)
        if i == 1:
            for opt in (opt_e, opt_g):
                opt.param_groups[0]["lr"] = 1e-3
                opt.sync_hyper()
        worst = max([worst] + [(p - q).abs().max().item() for p, q in zip(net_e.parameters(), net_g.parameters())])
    print(f"hier={hier}: worst loss diff {max(abs(a - b) for a, b in zip(eager, graph)):.3e}, worst parameter diff {worst:.3e}")
    assert (gs.replayed_steps, gs.eager_steps) == (4, 1)
    assert len(set(graph)) == 5  # every step handed out its own scalar
    np.testing.assert_allclose(graph, eager, rtol=2e-5)
    _assert_params_agree(net_e, net_g)
    assert float(opt_g.state[next(net_g.parameters())]["step"]) == 5.0 == float(opt_e.state[next(net_e.parameters())]["step"])


@pytest.mark.gpu
def test_graphed_prior_step_skips_the_copy_for_bound_batches(gpu_device, monkeypatch):
    """A loader bound to the static inputs hands out those very buffers; step() then replays without a copy_."""
    import movae_amd  # noqa: F401
    from movae_amd.prior import DeviceCodeLoader, GraphedPriorStep, VQCodeDataset

    z = torch.randint(0, 16, (N, 8, 8), generator=torch.Generator().manual_seed(2)).to(torch.int16)
    ld = DeviceCodeLoader(VQCodeDataset((z,), False), 16, gpu_device, shuffle=True, seed=0)
    net, opt = _twin(False, gpu_device)
    first = next(iter(ld))
    gs = GraphedPriorStep(net, opt, first)
    ld.bind(gs.static_top)
    copies = []
    real = torch.Tensor.copy_
    static = gs.static_top.data_ptr()  # (only copies into the static input count: the eager branch's optimizer may copy a gradient)
    monkeypatch.setattr(torch.Tensor, "copy_",
                        lambda self, *a, **k: (copies.append(1) if self.data_ptr() == static else None, real(self, *a, **k))[1])
    order = torch.tensor(ld.indices())
    for i, b in enumerate(ld):
        if b.size(0) == 16:
            assert b.data_ptr() == gs.static_top.data_ptr() and torch.equal(b.cpu(), z[order[16 * i:16 * i + 16]].long())
        gs.step(b)
    assert (gs.replayed_steps, gs.eager_steps) == (2, 1) and copies == []
    gs.step(first)  # a batch from elsewhere: one copy_ into the static input
    assert copies == [1]


@pytest.mark.gpu
def test_graphed_prior_step_refuses_pixelsnail(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd.models.pixelcnn_prior import PixelSNAIL
    from movae_amd.optim import FusedAdam
    from movae_amd.prior import GraphedPriorStep

    net = PixelSNAIL(16, 8, hidden_channels=16, num_blocks=1, num_res_blocks_per_layer=1, num_heads=2).to(gpu_device)
    opt = FusedAdam(net.parameters(), lr=1e-3, device_step=True)
    with pytest.raises(NotImplementedError):
        GraphedPriorStep(net, opt, torch.zeros(4, 8, 8, dtype=torch.long, device=gpu_device))


# ---- the stage -----------------------------------------------------------------------------------------------------------------------
def _stage_argv(tmp_path, *extra):
    return ["--dataset", "synthetic_cifar10", "--arch", "vq_vae", "--embedding_dim", "8", "--num_embeddings", "16", "--hidden_dims", "16", "32",
            "--batch_size", "32", "--max_items", "128", "--epochs", "1", "--pixelcnn_epochs", "2", "--pixelcnn_hidden_channels", "16",
            "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3", "--save_path", str(tmp_path), "--seed", "1", "--device", "cuda:0",
            "--eval_freq", "0", "--prior_loader", "device", *extra]


@pytest.mark.gpu
def test_stage_on_the_device_eager_and_graph_agree(gpu_device, tmp_path):
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train

    runs = {}
    for mode in ("eager", "graph"):
        root = tmp_path / mode
        args = train.parse_args(_stage_argv(root, "--prior_step", mode))
        train.set_seed(args.seed)
        assert len(train.main(args)) == 1
        rec = dict(P.LAST_RUN)
        assert rec["use_cache"] and rec["n_codes"] == 128 and rec["loader"] == "device" and rec["step_mode"] == mode
        assert rec["replayed_steps"] + rec["eager_steps"] == 2 * 4
        assert rec["replayed_steps"] == (8 if mode == "graph" else 0)
        losses = rec["epoch_losses"]
        assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0] < np.log(16) * 1.2
        assert len(list(root.rglob("final_prior.pth"))) == 1 and list(root.rglob("best_prior.pth"))
        assert tuple(rec["samples"].shape) == (4, 3, 32, 32) and torch.isfinite(rec["samples"]).all()
        runs[mode] = losses
    print("epoch losses", runs)
    np.testing.assert_allclose(runs["graph"], runs["eager"], rtol=2e-5)


@pytest.mark.gpu
def test_stage_trains_pixelsnail_eagerly_under_prior_step_graph(gpu_device, tmp_path, capsys):
    import movae_amd  # noqa: F401
    from movae_amd import prior as P
    from movae_amd import train
    from movae_amd.models import get_network

    args = train.parse_args(_stage_argv(tmp_path, "--prior_step", "graph", "--pixelsnail_num_blocks", "1", "--pixelsnail_num_res_blocks",
                                        "1", "--pixelsnail_num_heads", "2"))
    train.set_seed(args.seed)
    train_ds, _, input_size = train.get_dataset(args.dataset, data_dir=args.data_dir, normalize=args.normalize_inputs,
                                                max_items=args.max_items)
    loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, shuffle=True)
    net = get_network(input_size, num_channels=3, args=args, device=gpu_device).to(gpu_device)
    prior = P.build_pixelsnail_prior(net, args, gpu_device)
    P.train_pixelcnn_prior(net, loader, gpu_device, args, str(tmp_path), prior=prior)
    rec = P.LAST_RUN
    assert rec["step_mode"] == "eager" and rec["loader"] == "device" and (rec["replayed_steps"], rec["eager_steps"]) == (0, 8)
    assert np.isfinite(rec["epoch_losses"]).all()
    assert capsys.readouterr().out.count("taking the eager step") == 1
