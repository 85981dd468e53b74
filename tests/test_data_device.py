"""Device side of the real-dataset path: movae_batch_u8 bit for bit against the restated transforms and flip rule, 64-bit offsets, the
epoch semantics of data.DeviceBatchLoader, its agreement with the host path, the residency refusal, the zero-copy input layout, and
train.cli on a tiny CIFAR-10 written into tmp_path."""
import numpy as np
import pytest
import torch

import data_yardstick as Y

pytestmark = pytest.mark.gpu

SEED = Y.SEED
IDX = [10, 0, 3, 3, 7]  # out of order and repeated; at (SEED, 0) and at (SEED, 1) some of these rows flip and some do not


@pytest.fixture(scope="module")
def M(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import data, ops, train

    return data, ops, train


def _nchw(out_nhwc):
    return out_nhwc.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("h,w", [(8, 8), (6, 10), (5, 4)])  # (6, 10): w is no multiple of 4 (the per-element path) and H != W
def test_kernel_is_exact(M, gpu_device, h, w, c, normalize):
    data, ops, _ = M
    u8 = Y.images(11, h, w, c, seed=h * 100 + w * 10 + c)
    store = torch.from_numpy(u8).to(gpu_device)
    # the table restated: ToTensor's u / 255, then Normalize's (x - 0.5) / 0.5
    table = torch.arange(256, dtype=torch.float32).div(255).repeat(c, 1)
    if normalize:
        table = table.sub(0.5).div(0.5)
    assert torch.equal(data.value_table(c, normalize), table)
    lut = table.to(gpu_device)
    seen = set()
    for idx in (IDX, [4]):
        rows = torch.tensor(idx, dtype=torch.int32, device=gpu_device)
        for flip in (False, True):
            for epoch in Y.EPOCHS:
                out = ops.batch_u8(store, rows, lut, flip=flip, seed=SEED, epoch=epoch)
                assert out.dtype == torch.float32 and tuple(out.shape) == (len(idx), h, w, c) and out.is_contiguous()
                assert torch.equal(_nchw(out), Y.expected_batch(u8, idx, normalize, flip, SEED, epoch)), (idx, flip, epoch)
                if flip:
                    seen.update(Y.flip_rule(idx, SEED, epoch).tolist())
    assert seen == {False, True}, "both flipped and unflipped rows must have occurred"
    # a 64-bit seed and epoch reach the counter and the key whole
    big_seed, big_epoch = (3 << 32) | 9, (1 << 32) | 2
    rows = torch.arange(11, dtype=torch.int32, device=gpu_device)
    out = ops.batch_u8(store, rows, lut, flip=True, seed=big_seed, epoch=big_epoch)
    assert torch.equal(_nchw(out), Y.expected_batch(u8, list(range(11)), normalize, True, big_seed, big_epoch))


def test_offsets_are_64_bit(M, gpu_device):
    """A store of more than 2^31 bytes (11 000 images of 256 x 256 x 3, uninitialised but for the first and the last image)."""
    data, ops, _ = M
    n, s = 11000, 256
    store = torch.empty((n, s, s, 3), dtype=torch.uint8, device=gpu_device)
    assert store.numel() > 2 ** 31
    ends = Y.images(2, s, s, 3, seed=4)
    store[0].copy_(torch.from_numpy(ends[0]))
    store[n - 1].copy_(torch.from_numpy(ends[1]))
    lut = data.value_table(3, True).to(gpu_device)
    idx = [n - 1, 0]
    out = ops.batch_u8(store, torch.tensor(idx, dtype=torch.int32, device=gpu_device), lut, flip=True, seed=SEED, epoch=0)
    fl = Y.flip_rule(idx, SEED, 0)
    want = torch.stack([Y.transform(ends[1], True, bool(fl[0])), Y.transform(ends[0], True, bool(fl[1]))])
    assert torch.equal(_nchw(out), want)
    del store


def test_bad_arguments_are_refused(M, gpu_device):
    import movae_amd._lib as L

    data, _, _ = M
    lib = L.load()
    store = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=gpu_device)
    idx = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    lut = data.value_table(3, False).to(gpu_device)
    out = torch.full((2, 4, 4, 3), 7.0, device=gpu_device)
    st = L.stream_ptr(gpu_device)
    good = dict(store=store.data_ptr(), idx=idx.data_ptr(), b=2, h=4, w=4, c=3, lut=lut.data_ptr(), out=out.data_ptr())

    def rc(**kw):
        a = dict(good, **kw)
        return lib.movae_batch_u8(a["store"], a["idx"], a["b"], a["h"], a["w"], a["c"], a["lut"], 1, 0, 0, a["out"], st)

    for bad in (dict(store=None), dict(idx=None), dict(lut=None), dict(out=None), dict(b=0), dict(b=-1), dict(h=0), dict(w=0), dict(w=-4),
                dict(c=2), dict(c=4), dict(c=0)):
        assert rc(**bad) == -1, bad
        assert b"movae_batch_u8" in lib.movae_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call launches nothing"
    assert rc() == 0
    torch.cuda.synchronize()
    assert (out == 0.0).all()


@pytest.fixture(scope="module")
def epoch_set():
    return Y.images(37, 8, 8, 3, seed=21)


def _epoch(loader, epoch):
    loader.set_epoch(epoch)
    return [(x, y) for x, y in loader]


def test_one_epoch(M, gpu_device, epoch_set):
    data, _, _ = M
    u8 = epoch_set
    ds = data.ResidentImages(u8, True, train=True, seed=SEED)
    loader = data.DeviceBatchLoader(ds, 8, gpu_device, shuffle=True, seed=3)
    assert len(loader) == 5
    runs = {}
    for epoch in (0, 1):
        batches = _epoch(loader, epoch)
        assert [x.size(0) for x, _ in batches] == [8, 8, 8, 8, 5]
        order = loader.indices()
        assert sorted(order) == list(range(37))
        for k, (x, y) in enumerate(batches):
            assert tuple(x.shape) == (x.size(0), 3, 8, 8) and x.is_cuda and x.permute(0, 2, 3, 1).is_contiguous()  # logical NCHW over NHWC
            assert y.dtype == torch.long and tuple(y.shape) == (x.size(0),) and not y.any()
            assert torch.equal(x.cpu(), Y.expected_batch(u8, order[8 * k:8 * k + 8], True, True, SEED, epoch)), (epoch, k)
        assert len({x.data_ptr() for x, _ in batches}) == 5, "output buffers are not reused"
        runs[epoch] = (order, torch.cat([x for x, _ in batches]).cpu())
    assert runs[0][0] != runs[1][0] and not torch.equal(runs[0][1], runs[1][1])
    # the same seeds reproduce both epochs, in a fresh loader and in the old one
    again = data.DeviceBatchLoader(data.ResidentImages(u8, True, train=True, seed=SEED), 8, gpu_device, shuffle=True, seed=3)
    for epoch in (1, 0):
        for ld in (again, loader):
            assert torch.equal(torch.cat([x for x, _ in _epoch(ld, epoch)]).cpu(), runs[epoch][1])
    # without a shuffle the images come in store order; an evaluation set (train=False) is never flipped
    plain = data.DeviceBatchLoader(data.ResidentImages(u8, True, train=False, seed=SEED), 8, gpu_device, shuffle=False)
    got = torch.cat([x for x, _ in _epoch(plain, 1)]).cpu()
    assert torch.equal(got, Y.expected_batch(u8, list(range(37)), True, False, SEED, 1))


def test_host_and_device_paths_agree(M, gpu_device, epoch_set):
    data, _, _ = M
    ds = data.ResidentImages(epoch_set, False, train=True, seed=SEED)
    loader = data.DeviceBatchLoader(ds, 8, gpu_device, shuffle=True, seed=1)
    for epoch in (0, 1):
        ds.set_epoch(epoch)
        loader.set_epoch(epoch)
        host = torch.utils.data.DataLoader(ds, batch_size=8, sampler=loader.indices(), drop_last=False)
        dev = list(loader)
        assert len(host) == len(dev) == 5
        for (hx, hy), (dx, dy) in zip(host, dev):
            assert torch.equal(hx, dx.cpu()) and torch.equal(hy, dy.cpu())


def test_loaders_of_one_array_share_the_store(M, gpu_device, epoch_set):
    """The train loader, the prior stage's loader and AFHQ's test set (its train file) read one device copy."""
    data, _, _ = M
    tr, te = data.ResidentImages(epoch_set, False, train=True), data.ResidentImages(epoch_set, False, train=False)
    a, b, c = (data.DeviceBatchLoader(ds, 8, gpu_device, shuffle=False) for ds in (tr, tr, te))
    other = data.DeviceBatchLoader(data.ResidentImages(epoch_set[:30], False, train=False), 8, gpu_device, shuffle=False)
    firsts = [next(iter(ld))[0] for ld in (a, b, c, other)]
    assert a._store.data_ptr() == b._store.data_ptr() == c._store.data_ptr() != other._store.data_ptr()
    assert torch.equal(firsts[0], firsts[1]) and torch.equal(firsts[2], firsts[3])  # (a, b flip; c and other, evaluation sets, do not)
    assert torch.equal(torch.cat([x for x, _ in c]).cpu(), Y.expected_batch(epoch_set, list(range(37)), False, False, 0, 0))


def test_set_that_does_not_fit_is_refused(M, gpu_device, monkeypatch):
    data, ops, _ = M
    ds = data.ResidentImages(Y.images(200, 32, 32, 3, seed=2), False, train=True)  # 614 400 bytes > half of 1 MB
    loader = data.DeviceBatchLoader(ds, 8, gpu_device, shuffle=True)
    launches = []
    monkeypatch.setattr(ops, "batch_u8", lambda *a, **k: launches.append(a))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 288 << 30))
    with pytest.raises(RuntimeError) as e:
        next(iter(loader))
    assert "--data_loader host" in str(e.value) and str(1 << 20) in str(e.value) and str(ds.u8.nbytes + 3 * 256 * 4) in str(e.value)
    assert loader._store is None and not launches, "refused before any upload"


def test_loader_view_needs_no_layout_pass(M, gpu_device, monkeypatch):
    """The loader's batch is a logical-NCHW view of an NHWC buffer: ops.to_nhwc of it is zero-copy, so the step's 3-channel input
    transpose (ops.NchwToNhwc) is not launched, and the step computes bit for bit what it computes on the contiguous NCHW copy."""
    data, ops, train = M
    from movae_amd import aggregation
    from movae_amd.models import get_network
    from movae_amd.optim import FusedAdam

    class A:
        pass

    a = A()
    a.arch, a.batch_size, a.dataset_size = "vae", 8, 1000
    a.latent_dim, a.hidden_dims = 8, [8, 16]
    a.recons_objective, a.recons_activation, a.loss_weights = "mse", None, None
    torch.manual_seed(0)
    net = get_network(8, 3, a, gpu_device).to(gpu_device).train()
    net.eps_override = torch.randn(8, 8, generator=torch.Generator().manual_seed(2)).to(gpu_device)
    opt = FusedAdam(net.parameters(), lr=1e-3, weight_decay=0)
    ds = data.ResidentImages(Y.images(8, 8, 8, 3, seed=6), False, train=True, seed=SEED)
    x, _ = next(iter(data.DeviceBatchLoader(ds, 8, gpu_device, shuffle=True)))
    assert not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()
    assert ops.to_nhwc(x).data_ptr() == x.data_ptr()

    calls = []
    real = ops.NchwToNhwc

    class Counting:
        @staticmethod
        def apply(*args):
            calls.append(tuple(args[0].shape))
            return real.apply(*args)

        def __getattr__(self, name):
            return getattr(real, name)

    monkeypatch.setattr(ops, "NchwToNhwc", Counting())

    def run(images):
        ld, _ = train.forward_backward(net, images, opt, aggregation.UPGrad())
        torch.cuda.synchronize()
        return ({k: v.detach().clone() for k, v in ld.items()},
                {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})

    # hidden_dims [8, 16] on 8 x 8 leave a 2 x 2 latent grid, so the decoder's nn.Unflatten goes through the same op once per step
    # (the other layout pass); the image batch itself must not
    losses_v, grads_v = run(x)
    assert calls and set(calls) == {(8, 16, 2, 2)}, f"only the latent grid is transposed, never the loader's view: {calls}"
    del calls[:]
    losses_c, grads_c = run(x.contiguous())
    assert calls.count((8, 3, 8, 8)) == 1, f"the contiguous NCHW copy does take the input transpose (the counter works): {calls}"
    assert losses_v.keys() == losses_c.keys() and grads_v.keys() == grads_c.keys() and grads_v
    for k in losses_v:
        assert torch.equal(losses_v[k], losses_c[k]), k
    for n in grads_v:
        assert torch.equal(grads_v[n], grads_c[n]), n


def _tiny_cifar10(root):
    Y.write_cifar10(str(root), per_file=40, seed=8)  # 5 x 40 train images, 40 test images
    return str(root)


@pytest.mark.parametrize("mode", ["graph_off", "graph_on", "host"])
def test_cli_trains_on_cifar10_files(M, gpu_device, tmp_path, capsys, monkeypatch, mode):
    _, ops, train = M
    launches = []
    real = ops.batch_u8
    monkeypatch.setattr(ops, "batch_u8", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    argv = ["--dataset", "CIFAR10", "--data_dir", _tiny_cifar10(tmp_path / "data"), "--arch", "vae", "--agg", "upgrad", "--batch_size", "16",
            "--epochs", "2", "--latent_dim", "16", "--hidden_dims", "16", "32", "--max_fid_samples", "40", "--seed", "3",
            "--save_path", str(tmp_path / "logs"), "--device", "cuda:0", "--graph", "on" if mode == "graph_on" else "off"]
    if mode == "host":
        argv += ["--data_loader", "host"]
    hist = train.cli(argv)
    out = capsys.readouterr().out
    assert len(hist) == 2 and all(np.isfinite(list(h.values())).all() for h in hist)
    final = [line for line in out.splitlines() if line.startswith("final:")]
    assert len(final) == 1 and "eval_total_loss" in final[0] and "psnr" in final[0]
    assert all(np.isfinite(v) for v in train.LAST_FINAL["losses"].values()) and np.isfinite(train.LAST_FINAL["recon"]["psnr"])
    # 13 train batches per epoch, 3 test batches per evaluation (two epochs' and the final one)
    assert len(launches) == (0 if mode == "host" else 2 * 13 + 3 * 3)


def test_cli_prior_stage_on_cifar10_files(M, gpu_device, tmp_path):
    """A VQ-VAE run with the prior stage (the shape of tests/test_prior.py): the prior's loader comes from the same helper."""
    _, _, train = M
    from movae_amd import prior as P

    argv = ["--dataset", "CIFAR10", "--data_dir", _tiny_cifar10(tmp_path / "data"), "--arch", "vq_vae", "--embedding_dim", "8",
            "--num_embeddings", "16", "--hidden_dims", "16", "32", "--batch_size", "32", "--max_items", "128", "--epochs", "1",
            "--pixelcnn_epochs", "2", "--pixelcnn_hidden_channels", "16", "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3",
            "--save_path", str(tmp_path / "logs"), "--seed", "1", "--device", "cuda:0", "--eval_freq", "0", "--max_fid_samples", "0"]
    args = train.parse_args(argv)
    train.set_seed(args.seed)
    hist = train.main(args)
    assert len(hist) == 1 and np.isfinite(list(hist[0].values())).all()
    rec = P.LAST_RUN
    assert rec["use_cache"] and rec["n_codes"] == 128 and len(rec["epoch_losses"]) == 2 and np.isfinite(rec["epoch_losses"]).all()
    assert list((tmp_path / "logs").rglob("final_prior.pth"))
