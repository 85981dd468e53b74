"""Device side of the RandomResizedCrop path: movae_batch_rrc_u8 bit for bit against Pillow's recorded outputs (tests/golden/rrc_tiny.npz),
the kernel's fp64 coefficient routine against the restated table, 64-bit offsets, the refusals, data.RaggedBatchLoader against the host
items and the sampler's shards, the residency refusal, the zero-copy input layout, and train.cli on a tiny prepared
oxford-flower-102."""
import collections

import numpy as np
import pytest
import torch

import data_yardstick as Y
import rrc_yardstick as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

SEED = Y.SEED


@pytest.fixture(scope="module")
def M(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import data, ops, train

    return data, ops, train


def _nchw(out_nhwc):
    return out_nhwc.permute(0, 3, 1, 2).cpu()


def _kmax(sides, s):
    return max(R.ksize(int(v), s) for v in sides)


def _dev(gpu_device, blob, index, boxes):
    return (torch.from_numpy(blob).to(gpu_device), torch.from_numpy(np.ascontiguousarray(index[:, 0])).to(gpu_device),
            torch.from_numpy(index[:, 1:].astype(np.int32)).to(gpu_device), torch.from_numpy(np.asarray(boxes, dtype=np.int32)).to(gpu_device))


def test_kernel_equals_pillow_on_the_fixture(M, gpu_device):
    """Every case, through the value table, normalise on / off, flip on / off; one launch takes the cases of one (s, c), in lists that
    are out of order, repeated and of length one.  The blob starts one byte in, so images begin at odd and even bytes alike."""
    data, ops, _ = M
    groups = collections.defaultdict(list)
    for c in R.load_cases(load_golden("rrc_tiny")):
        groups[(c["s"], c["src"].shape[2])].append(c)
    assert {s for s, _ in groups} >= {4, 8, 16, 32, 40} and {c for _, c in groups} == {1, 3}
    seen, odd = set(), 0
    for (s, ch), cs in sorted(groups.items()):
        n = len(cs)
        blob, index = R.pack([c["src"] for c in cs], lead=1)
        odd += int((index[:, 0] % 2 == 1).sum())
        boxes = np.array([c["box"] for c in cs], dtype=np.int32)
        store, offsets, dims, dboxes = _dev(gpu_device, blob, index, boxes)
        kmax = _kmax(boxes[:, 2:].reshape(-1), s)
        assert 5 <= kmax <= 33
        lists = [list(range(n))[::-1] + [0, n - 1, 0], [n // 2]]
        for normalize in (False, True):
            lut = data.value_table(ch, normalize).to(gpu_device)
            for idx in lists:
                rows = torch.tensor(idx, dtype=torch.int32, device=gpu_device)
                for flip in (False, True):
                    for epoch in Y.EPOCHS:
                        out = ops.batch_rrc_u8(store, offsets, dims, dboxes, rows, s, ch, kmax, lut, flip=flip, seed=SEED, epoch=epoch)
                        assert out.dtype == torch.float32 and tuple(out.shape) == (len(idx), s, s, ch) and out.is_contiguous()
                        fl = Y.flip_rule(idx, SEED, epoch) if flip else np.zeros(len(idx), dtype=bool)
                        want = torch.stack([Y.transform(cs[i]["out"], normalize, bool(f)) for i, f in zip(idx, fl)])
                        got = _nchw(out)
                        for j, i in enumerate(idx):
                            assert torch.equal(got[j], want[j]), (s, ch, normalize, flip, epoch, i, cs[i]["box"])
                        if flip:
                            seen.update(fl.tolist())
    assert seen == {False, True}, "both flipped and unflipped rows must have occurred"
    assert odd > 5, "images at odd byte offsets must have occurred"


def _check_tables(ops, gpu_device, sizes, out, kmax):
    k, b = ops.resample_coeffs(torch.tensor(sizes, dtype=torch.int32, device=gpu_device), out, kmax)
    assert k.dtype == torch.int32 and tuple(k.shape) == (len(sizes), out, kmax) and tuple(b.shape) == (len(sizes), out, 2)
    k, b = k.cpu().numpy(), b.cpu().numpy()
    for q, n in enumerate(sizes):
        kk, bb = R.coeffs(n, out, kmax)
        assert np.array_equal(b[q], bb), (n, out)
        assert np.array_equal(k[q], kk), (n, out, np.argwhere(k[q] != kk)[:3])


@pytest.mark.parametrize("out", [4, 8, 16])
def test_coefficient_tables_small(M, gpu_device, out):
    """Every input size 1 .. 64 (64 -> 4 is a filter scale of 16: 65 taps, past what the batch kernel stages, not past this entry)."""
    _, ops, _ = M
    _check_tables(ops, gpu_device, list(range(1, 65)), out, R.ksize(64, out))


def test_coefficient_tables_at_256(M, gpu_device):
    """200 input sizes in 65 .. 2048 at the dataset's output side, among them the identity, its two neighbours and the 8 x cap."""
    _, ops, _ = M
    rng = np.random.default_rng(8)
    sizes = [256, 255, 257, 2048] + [int(v) for v in rng.integers(65, 2049, size=196)]
    _check_tables(ops, gpu_device, sizes, 256, 33)


def test_offsets_are_64_bit(M, gpu_device):
    """A blob of 2.2e9 bytes, uninitialised but for a first and a last image."""
    data, ops, _ = M
    total = 2_200_000_001
    blob = torch.empty(total, dtype=torch.uint8, device=gpu_device)
    ends = [Y.images(1, 20, 27, 3, seed=4)[0], Y.images(1, 31, 18, 3, seed=5)[0]]
    index = np.array([[0, 20, 27], [total - ends[1].size, 31, 18]], dtype=np.int64)
    assert index[1, 0] > 2 ** 31
    for (off, _, _), im in zip(index, ends):
        blob[int(off):int(off) + im.size].copy_(torch.from_numpy(im.reshape(-1)))
    boxes = np.array([[1, 2, 17, 24], [3, 0, 28, 18]], dtype=np.int32)
    lut = data.value_table(3, True).to(gpu_device)
    idx = [1, 0]
    out = ops.batch_rrc_u8(blob, torch.from_numpy(np.ascontiguousarray(index[:, 0])).to(gpu_device),
                           torch.from_numpy(index[:, 1:].astype(np.int32)).to(gpu_device), torch.from_numpy(boxes).to(gpu_device),
                           torch.tensor(idx, dtype=torch.int32, device=gpu_device), 16, 3, _kmax(boxes[:, 2:].reshape(-1), 16), lut,
                           flip=True, seed=SEED, epoch=0)
    fl = Y.flip_rule(idx, SEED, 0)
    want = torch.stack([R.item(ends[i], boxes[i], 16, True, bool(f)) for i, f in zip(idx, fl)])
    assert torch.equal(_nchw(out), want)
    del blob


def test_bad_arguments_are_refused(M, gpu_device):
    import movae_amd._lib as L

    data, _, _ = M
    lib = L.load()
    img = Y.images(2, 6, 5, 3, seed=1)
    blob, index = R.pack(list(img))
    boxes = np.array([[0, 0, 6, 5], [1, 1, 4, 3]], dtype=np.int32)
    store, offsets, dims, dboxes = _dev(gpu_device, blob, index, boxes)
    idx = torch.tensor([1, 0], dtype=torch.int32, device=gpu_device)
    lut = data.value_table(3, False).to(gpu_device)
    out = torch.full((2, 4, 4, 3), 7.0, device=gpu_device)
    st = L.stream_ptr(gpu_device)
    good = dict(blob=store.data_ptr(), offsets=offsets.data_ptr(), dims=dims.data_ptr(), boxes=dboxes.data_ptr(), idx=idx.data_ptr(), b=2, s=4,
                c=3, kmax=5, lut=lut.data_ptr(), out=out.data_ptr())

    def rc(**kw):
        a = dict(good, **kw)
        return lib.movae_batch_rrc_u8(a["blob"], a["offsets"], a["dims"], a["boxes"], a["idx"], a["b"], a["s"], a["c"], a["kmax"], a["lut"],
                                      1, 0, 0, a["out"], st)

    for bad in (dict(blob=None), dict(offsets=None), dict(dims=None), dict(boxes=None), dict(idx=None), dict(lut=None), dict(out=None),
                dict(b=0), dict(b=-1), dict(s=0), dict(s=-4), dict(c=2), dict(c=4), dict(c=0), dict(kmax=3), dict(kmax=4), dict(kmax=6),
                dict(kmax=32), dict(kmax=35), dict(kmax=-5), dict(out=out.data_ptr() + 4)):
        assert rc(**bad) == -1, bad
        assert b"movae_batch_rrc_u8" in lib.movae_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call launches nothing"
    assert rc() == 0 and rc(kmax=33) == 0
    torch.cuda.synchronize()
    want = torch.stack([R.item(img[i], boxes[i], 4, False, bool(f)) for i, f in zip([1, 0], Y.flip_rule([1, 0], 0, 0))])
    assert torch.equal(_nchw(out), want)
    # the table entry refuses the same way
    sizes = torch.tensor([7], dtype=torch.int32, device=gpu_device)
    k, b = torch.full((1, 4, 5), 9, dtype=torch.int32, device=gpu_device), torch.full((1, 4, 2), 9, dtype=torch.int32, device=gpu_device)
    for args in ((None, 1, 4, 5, k.data_ptr(), b.data_ptr()), (sizes.data_ptr(), 1, 4, 5, None, b.data_ptr()),
                 (sizes.data_ptr(), 1, 4, 5, k.data_ptr(), None), (sizes.data_ptr(), 0, 4, 5, k.data_ptr(), b.data_ptr()),
                 (sizes.data_ptr(), 1, 0, 5, k.data_ptr(), b.data_ptr()), (sizes.data_ptr(), 1, 4, 4, k.data_ptr(), b.data_ptr()),
                 (sizes.data_ptr(), 1, 4, 3, k.data_ptr(), b.data_ptr())):
        assert lib.movae_resample_coeffs(*args, st) == -1, args
        assert b"movae_resample_coeffs" in lib.movae_last_error()
    torch.cuda.synchronize()
    assert (k == 9).all() and (b == 9).all()


@pytest.fixture(scope="module")
def epoch_set():
    """37 images of mixed sizes, 5 .. 128 a side (up to 8 x the output side 16), packed one byte in."""
    rng = np.random.default_rng(21)
    dims = rng.integers(5, 129, size=(37, 2))
    dims[0], dims[1] = (128, 128), (5, 128)
    imgs = [rng.integers(0, 256, size=(int(h), int(w), 3), dtype=np.uint8) for h, w in dims]
    blob, index = R.pack(imgs, lead=1)
    return imgs, blob, index


def _epoch(loader, epoch):
    loader.set_epoch(epoch)
    return [(x, y) for x, y in loader]


def test_loader_equals_the_host_items(M, gpu_device, epoch_set):
    data, _, _ = M
    imgs, blob, index = epoch_set
    ds = data.RaggedImages(blob, index, 16, True, train=True, seed=SEED)
    assert ds.kmax == 33
    loader = data.RaggedBatchLoader(ds, 8, gpu_device, shuffle=True, seed=3)
    assert len(loader) == 5
    runs = {}
    for epoch in (0, 1):
        ds.set_epoch(epoch)
        batches = _epoch(loader, epoch)
        assert [x.size(0) for x, _ in batches] == [8, 8, 8, 8, 5]
        order = loader.indices()
        assert order == data.shard_indices(37, True, 3, epoch) and sorted(order) == list(range(37))
        host = torch.utils.data.DataLoader(ds, batch_size=8, sampler=order, drop_last=False)
        for k, ((x, y), (hx, hy)) in enumerate(zip(batches, host)):
            assert tuple(x.shape) == (x.size(0), 3, 16, 16) and x.is_cuda and x.permute(0, 2, 3, 1).is_contiguous()
            assert y.dtype == torch.long and tuple(y.shape) == (x.size(0),) and not y.any()
            assert torch.equal(x.cpu(), hx) and torch.equal(y.cpu(), hy), (epoch, k)
        assert len({x.data_ptr() for x, _ in batches}) == 5, "output buffers are not reused"
        runs[epoch] = (order, torch.cat([x for x, _ in batches]).cpu())
    assert runs[0][0] != runs[1][0] and not torch.equal(runs[0][1], runs[1][1])
    # and the host items are the restated pipeline (one epoch, every image)
    boxes, fl = R.boxes(index[:, 1:], SEED, 1), Y.flip_rule(np.arange(37), SEED, 1)
    by_index = dict(zip(runs[1][0], runs[1][1]))
    for i in range(37):
        assert torch.equal(by_index[i], R.item(imgs[i], boxes[i], 16, True, bool(fl[i]))), i
    # the same seeds reproduce an epoch; an evaluation set is the whole image, never flipped, in store order
    assert torch.equal(torch.cat([x for x, _ in _epoch(loader, 0)]).cpu(), runs[0][1])
    plain = data.RaggedBatchLoader(data.RaggedImages(blob, index, 16, True, train=False, seed=SEED), 8, gpu_device, shuffle=False)
    got = torch.cat([x for x, _ in _epoch(plain, 1)]).cpu()
    assert torch.equal(got, torch.stack([Y.transform(R.resize(im, 16), True, False) for im in imgs]))


def test_loader_shards_by_rank(M, gpu_device, epoch_set):
    data, _, _ = M
    imgs, blob, index = epoch_set
    ds = data.RaggedImages(blob, index, 16, False, train=True, seed=SEED)
    whole = data.RaggedBatchLoader(ds, 8, gpu_device, shuffle=True, seed=3)
    rank1 = data.RaggedBatchLoader(ds, 8, gpu_device, shuffle=True, rank=1, world_size=2, seed=3)
    assert whole._store is None
    by_index = dict(zip(whole.indices(0), torch.cat([x for x, _ in _epoch(whole, 0)]).cpu()))
    shard = data.shard_indices(37, True, 3, 0, rank=1, world_size=2)
    assert rank1.indices(0) == shard and len(shard) == 19 and len(rank1) == 3
    got = torch.cat([x for x, _ in _epoch(rank1, 0)]).cpu()
    assert torch.equal(got, torch.stack([by_index[i] for i in shard]))
    assert rank1._store.data_ptr() == whole._store.data_ptr(), "loaders of one blob share one device copy"


def test_set_that_does_not_fit_is_refused(M, gpu_device, monkeypatch, epoch_set):
    data, ops, _ = M
    _, blob, index = epoch_set
    big = np.concatenate([blob, np.zeros(600_000, np.uint8)])  # more than half of 1 MB
    ds = data.RaggedImages(big, index, 16, False, train=True)
    loader = data.RaggedBatchLoader(ds, 8, gpu_device, shuffle=True)
    launches = []
    monkeypatch.setattr(ops, "batch_rrc_u8", lambda *a, **k: launches.append(a))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 288 << 30))
    with pytest.raises(RuntimeError) as e:
        next(iter(loader))
    assert "--data_loader host" in str(e.value) and str(1 << 20) in str(e.value)
    assert loader._store is None and not launches, "refused before any upload"


def test_loader_view_needs_no_layout_pass(M, gpu_device, epoch_set):
    data, ops, _ = M
    _, blob, index = epoch_set
    ds = data.RaggedImages(blob, index, 16, False, train=True, seed=SEED)
    x, _ = next(iter(data.RaggedBatchLoader(ds, 8, gpu_device, shuffle=True)))
    assert not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()
    assert ops.to_nhwc(x).data_ptr() == x.data_ptr()


@pytest.mark.parametrize("graph", ["off", "auto"])
def test_cli_trains_on_prepared_files(M, gpu_device, tmp_path, capsys, monkeypatch, graph):
    """8 train images of 40 .. 60 px a side and 2 test images in the prepared on-disk form; the image side is the dataset's 256."""
    _, ops, train = M
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, size=(int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(40, 61, size=(8, 2))]
    blob, index = R.pack(imgs)
    root = tmp_path / "data"
    root.mkdir()
    np.save(root / "oxford-flower-102_train_ragged_u8.npy", blob)
    np.save(root / "oxford-flower-102_train_ragged_index.npy", index)
    np.save(root / "oxford-flower-102_test_u8.npy", Y.images(2, 256, 256, 3, seed=9))
    launches = []
    real = ops.batch_rrc_u8
    monkeypatch.setattr(ops, "batch_rrc_u8", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    argv = ["--dataset", "oxford-flower-102", "--data_dir", str(root), "--arch", "vae", "--agg", "upgrad", "--batch_size", "4", "--epochs", "1",
            "--latent_dim", "16", "--hidden_dims", "8", "16", "32", "32", "64", "--max_fid_samples", "2", "--seed", "3",
            "--save_path", str(tmp_path / "logs"), "--device", "cuda:0", "--graph", graph]
    hist = train.cli(argv)
    out = capsys.readouterr().out
    assert len(hist) == 1 and np.isfinite(list(hist[0].values())).all()
    final = [line for line in out.splitlines() if line.startswith("final:")]
    assert len(final) == 1 and "eval_total_loss" in final[0] and "psnr" in final[0]
    assert len(launches) == 2, "two train batches, one launch each (the test set is a ResidentImages)"
