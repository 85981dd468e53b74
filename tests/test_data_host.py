"""Host side of the real-dataset path (no GPU): the readers of train.get_dataset, the index rule of data.DeviceBatchLoader against
torch's own DistributedSampler, ResidentImages.__getitem__ against the restated transforms and flip rule, tools/prepare_images.py
against the PIL calls.  Every dataset is written into tmp_path from seeded numpy uint8."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

import data_yardstick as Y
from conftest import ROOT


@pytest.fixture(scope="module")
def train():
    import movae_amd  # noqa: F401
    from movae_amd import train

    return train


def _planar_check(ds, rows, size=32):
    """pixel (y, x, ch) of image k == rows[k][ch * size * size + y * size + x]."""
    assert ds.u8.dtype == np.uint8 and ds.u8.shape == (len(rows), size, size, 3)
    want = rows.reshape(len(rows), 3, size, size)
    for k in range(len(rows)):
        for ch in range(3):
            assert np.array_equal(ds.u8[k][:, :, ch], want[k, ch]), (k, ch)
    assert ds.u8[len(rows) - 1][5, 7, 2] == rows[len(rows) - 1][2 * size * size + 5 * size + 7]


def test_cifar10_reader(train, tmp_path):
    from movae_amd.data import ResidentImages

    tr_rows, te_rows = Y.write_cifar10(str(tmp_path))
    for name in ("CIFAR10", "cifar10"):
        tr, te, size = train.get_dataset(name, data_dir=str(tmp_path), normalize=False)
        assert size == 32 and isinstance(tr, ResidentImages) and isinstance(te, ResidentImages)
        assert len(tr) == 40 and len(te) == 8 and tr.train and not te.train
        _planar_check(tr, tr_rows)
        _planar_check(te, te_rows)
    x, label = te[3]
    assert label == 0 and x.dtype == torch.float32 and tuple(x.shape) == (3, 32, 32)


def test_cifar100_reader(train, tmp_path):
    tr_rows, te_rows = Y.write_cifar100(str(tmp_path))
    tr, te, size = train.get_dataset("CIFAR100", data_dir=str(tmp_path))
    assert size == 32 and len(tr) == 12 and len(te) == 5
    _planar_check(tr, tr_rows)
    _planar_check(te, te_rows)


@pytest.mark.parametrize("name,file_key,size", [("celeba", "celeba", 64), ("CelebA-128", "celeba-128", 128), ("celeba-hq", "celeba-hq", 256),
                                                ("afhq", "afhq", 256), ("animal-face", "afhq", 256)])
def test_npy_readers(train, tmp_path, name, file_key, size):
    tr_u8, te_u8 = Y.images(3, size, size, 3, 1), Y.images(2, size, size, 3, 2)
    np.save(tmp_path / f"{file_key}_train_u8.npy", tr_u8)
    if file_key != "afhq":
        np.save(tmp_path / f"{file_key}_test_u8.npy", te_u8)
    tr, te, got_size = train.get_dataset(name, data_dir=str(tmp_path), normalize=True)
    assert got_size == size and tr.train and not te.train and tr.normalize and te.normalize
    assert np.array_equal(tr.u8, tr_u8)
    assert np.array_equal(te.u8, tr_u8 if file_key == "afhq" else te_u8)  # AFHQ: the test set is the train file


def test_reader_errors_and_limits(train, tmp_path):
    # a missing file names its path and says that nothing is downloaded
    with pytest.raises(FileNotFoundError) as e:
        train.get_dataset("cifar10", data_dir=str(tmp_path))
    assert os.path.join(str(tmp_path), "cifar-10-batches-py", "data_batch_1") in str(e.value) and "download" in str(e.value)
    Y.write_cifar10(str(tmp_path))
    os.remove(tmp_path / "cifar-10-batches-py" / "data_batch_4")  # all five train files are required
    with pytest.raises(FileNotFoundError, match="data_batch_4"):
        train.get_dataset("cifar10", data_dir=str(tmp_path))
    with pytest.raises(FileNotFoundError) as e:
        train.get_dataset("celeba", data_dir=str(tmp_path))
    assert str(tmp_path / "celeba_train_u8.npy") in str(e.value)
    np.save(tmp_path / "celeba_train_u8.npy", Y.images(20, 64, 64, 3, 0))
    with pytest.raises(FileNotFoundError, match="celeba_test_u8.npy"):
        train.get_dataset("celeba", data_dir=str(tmp_path))
    # float or wrongly shaped arrays
    np.save(tmp_path / "celeba_test_u8.npy", np.zeros((2, 64, 64, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="float32"):
        train.get_dataset("celeba", data_dir=str(tmp_path))
    np.save(tmp_path / "celeba_test_u8.npy", np.zeros((2, 32, 64, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        train.get_dataset("celeba", data_dir=str(tmp_path))
    np.save(tmp_path / "celeba_test_u8.npy", np.zeros((2, 3, 64, 64), dtype=np.uint8))
    with pytest.raises(ValueError):
        train.get_dataset("celeba", data_dir=str(tmp_path))
    # max_items: the first max_items train images, the first max(1, max_items // 10) test images
    te_u8 = Y.images(7, 64, 64, 3, 3)
    np.save(tmp_path / "celeba_test_u8.npy", te_u8)
    tr, te, _ = train.get_dataset("celeba", data_dir=str(tmp_path), max_items=12)
    assert len(tr) == 12 and len(te) == 1 and np.array_equal(tr.u8, Y.images(20, 64, 64, 3, 0)[:12]) and np.array_equal(te.u8, te_u8[:1])
    tr, te, _ = train.get_dataset("celeba", data_dir=str(tmp_path), max_items=50)
    assert len(tr) == 20 and len(te) == 5
    Y.write_cifar100(str(tmp_path))
    tr, te, _ = train.get_dataset("cifar100", data_dir=str(tmp_path), max_items=5)
    assert len(tr) == 5 and len(te) == 1
    # the two sets that stay out say why; an unknown name is refused; the synthetic names are untouched
    with pytest.raises(NotImplementedError, match="252 GB"):
        train.get_dataset("imagenet", data_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="RandomResizedCrop"):
        train.get_dataset("oxford-flower-102", data_dir=str(tmp_path))
    with pytest.raises(NotImplementedError):
        train.get_dataset("mnist", data_dir=str(tmp_path))
    s_tr, s_te, s_size = train.get_dataset("synthetic_cifar10", max_items=100)
    assert isinstance(s_tr, train.SyntheticImages) and len(s_tr) == 100 and len(s_te) == 10 and s_size == 32


def test_resident_images_refuses_other_arrays(train):
    from movae_amd.data import ResidentImages

    for bad in (np.zeros((2, 4, 4, 3), np.float32), np.zeros((2, 4, 4), np.uint8), np.zeros((2, 4, 4, 2), np.uint8),
                np.zeros((0, 4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            ResidentImages(bad, False, True)


@pytest.mark.parametrize("n", [37, 64])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_index_rule_is_the_distributed_samplers(train, n, world):
    """No GPU is touched: the loader exposes its index list on the host."""
    from movae_amd.data import DeviceBatchLoader, ResidentImages

    ds = ResidentImages(Y.images(n, 2, 2, 3, 0), False, True)
    for seed in (0, 11):
        for rank in range(world):
            loader = DeviceBatchLoader(ds, 8, "cuda:0", shuffle=True, rank=rank, world_size=world, seed=seed)
            sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=seed)
            assert len(loader) == -(-len(sampler) // 8)
            for epoch in (0, 1):
                sampler.set_epoch(epoch)
                loader.set_epoch(epoch)
                assert loader.indices() == list(sampler), (n, world, rank, seed, epoch)
            assert loader.indices(0) != loader.indices(1)
    plain = DeviceBatchLoader(ds, 8, "cuda:0", shuffle=False)
    assert plain.indices() == list(range(n)) and len(plain) == -(-n // 8)


def test_flip_rule_is_balanced():
    """The restated rule alone, at the tests' seed: between 45 % and 55 % of the indices 0 .. 4095 are flipped, in both epochs."""
    for epoch in Y.EPOCHS:
        share = Y.flip_rule(np.arange(4096), Y.SEED, epoch).mean()
        assert 0.45 < share < 0.55, (epoch, share)
    assert not np.array_equal(Y.flip_rule(np.arange(4096), Y.SEED, 0), Y.flip_rule(np.arange(4096), Y.SEED, 1))
    assert not np.array_equal(Y.flip_rule(np.arange(4096), Y.SEED, 0), Y.flip_rule(np.arange(4096), Y.SEED + 1, 0))


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("normalize", [False, True])
def test_getitem_is_the_restated_transform(train, channels, normalize):
    from movae_amd.data import ResidentImages

    n = 24
    u8 = Y.images(n, 6, 10, channels, 7)
    u8[0, 0, :, 0] = np.arange(10) * 25  # a line that differs from its mirror image, and both ends of the byte range
    u8[1].reshape(-1)[:2] = (0, 255)
    tr, te = ResidentImages(u8, normalize, train=True, seed=Y.SEED), ResidentImages(u8, normalize, train=False, seed=Y.SEED)
    for epoch in Y.EPOCHS:
        tr.set_epoch(epoch)
        te.set_epoch(epoch)
        fl = Y.flip_rule(np.arange(n), Y.SEED, epoch)
        assert 0 < fl.sum() < n
        for i in range(n):
            x, label = tr[i]
            assert label == 0 and x.dtype == torch.float32 and tuple(x.shape) == (channels, 6, 10)
            assert torch.equal(x, Y.transform(u8[i], normalize, bool(fl[i]))), (epoch, i)
            assert torch.equal(te[i][0], Y.transform(u8[i], normalize, False)), (epoch, i)  # only a training set flips
    lo, hi = (-1.0, 1.0) if normalize else (0.0, 1.0)
    assert te[1][0].min().item() == lo and te[1][0].max().item() == hi
    with pytest.raises(IndexError):
        tr[n]


def test_getitem_from_a_memory_map(train, tmp_path):
    from movae_amd.data import ResidentImages

    u8 = Y.images(5, 4, 4, 3, 9)
    np.save(tmp_path / "a.npy", u8)
    ds = ResidentImages(np.load(tmp_path / "a.npy", mmap_mode="r"), True, train=True, seed=Y.SEED)
    fl = Y.flip_rule(np.arange(5), Y.SEED, 0)
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=5, shuffle=False)))[0]
    assert torch.equal(batch, torch.stack([Y.transform(u8[i], True, bool(fl[i])) for i in range(5)]))


@pytest.mark.parametrize("workers", [0, 2])
def test_host_loader_flips_follow_the_epoch(train, workers):
    """`--data_loader host` through train.make_loader, with and without worker processes: a worker holds a copy of the set, so the
    epoch set in the main process must still reach the items of every later epoch."""
    from movae_amd.data import ResidentImages

    n = 24
    u8 = Y.images(n, 4, 6, 3, 13)
    ds = ResidentImages(u8, False, train=True, seed=Y.SEED)
    a = train.parse_args(["--data_loader", "host", "--num_workers", str(workers)])
    loader = train.make_loader(ds, 8, torch.device("cpu"), a, shuffle=False)
    assert isinstance(loader, torch.utils.data.DataLoader) and loader.num_workers == workers
    flips = {e: Y.flip_rule(np.arange(n), Y.SEED, e) for e in (1, 2, 3)}
    assert not np.array_equal(flips[1], flips[2]) and not np.array_equal(flips[2], flips[3])
    for epoch in (1, 2, 3):
        ds.set_epoch(epoch)  # what train.main does per epoch on this path
        got = torch.cat([x for x, _ in loader])
        want = torch.stack([Y.transform(u8[i], False, bool(flips[epoch][i])) for i in range(n)])
        assert torch.equal(got, want), (workers, epoch)


def test_data_loader_flag(train):
    a = train.parse_args(["--dataset", "CIFAR10"])
    assert a.data_loader == "auto"
    assert train.parse_args(["--data_loader", "host"]).data_loader == "host"
    with pytest.raises(SystemExit):
        train.parse_args(["--data_loader", "nope"])
    # auto leaves the synthetic path on the DataLoader; device refuses it
    ds, _, _ = train.get_dataset("synthetic_cifar10", max_items=64)
    a.num_workers, a.seed = 0, None
    loader = train.make_loader(ds, 16, torch.device("cpu"), a, shuffle=False)
    assert isinstance(loader, torch.utils.data.DataLoader) and len(loader) == 4
    a.data_loader = "device"
    with pytest.raises(ValueError, match="uint8"):
        train.make_loader(ds, 16, torch.device("cpu"), a, shuffle=False)


def test_prepare_images(tmp_path):
    """tools/prepare_images.py on six PNGs of 20 x 24, centre crop 16, S = 8: equal to the PIL calls restated here."""
    from PIL import Image

    spec = importlib.util.spec_from_file_location("prepare_images", os.path.join(ROOT, "tools", "prepare_images.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = tmp_path / "src"
    src.mkdir()
    rng = np.random.default_rng(3)
    names = ["f.png", "b.png", "a.png", "e.png", "c.png", "d.png"]  # written out of order: the tool sorts
    raw = {}
    for n in names:
        raw[n] = rng.integers(0, 256, size=(24, 20, 3), dtype=np.uint8)  # 20 wide, 24 high
        Image.fromarray(raw[n]).save(src / n)
    (src / "notes.txt").write_text("not an image")

    def want(n):
        img = Image.open(src / n).convert("RGB")
        assert img.size == (20, 24)
        return np.asarray(img.crop((2, 4, 18, 20)).resize((8, 8), Image.BICUBIC))

    tool.main(["--src", str(src), "--out", str(tmp_path / "out"), "--name", "celeba", "--size", "8", "--center_crop", "16", "--split", "0.67"])
    tr, te = np.load(tmp_path / "out" / "celeba_train_u8.npy"), np.load(tmp_path / "out" / "celeba_test_u8.npy")
    assert tr.dtype == np.uint8 and tr.shape == (4, 8, 8, 3) and te.shape == (2, 8, 8, 3)
    order = sorted(names)
    for k, n in enumerate(order[:4]):
        assert np.array_equal(tr[k], want(n)), n
    for k, n in enumerate(order[4:]):
        assert np.array_equal(te[k], want(n)), n
    # a list of train names instead of a fraction; without a crop the whole image is resized
    lst = tmp_path / "train.txt"
    lst.write_text("e.png\nb.png\n")
    paths = tool.convert(str(src), str(tmp_path / "out2"), "afhq", 8, None, None, ["e.png", "b.png"])
    assert [os.path.basename(p) for p in paths] == ["afhq_train_u8.npy", "afhq_test_u8.npy"]
    tr2 = np.load(paths[0])
    assert tr2.shape == (2, 8, 8, 3) and np.load(paths[1]).shape == (4, 8, 8, 3)
    assert np.array_equal(tr2[0], np.asarray(Image.open(src / "b.png").convert("RGB").resize((8, 8), Image.BICUBIC)))
    with pytest.raises(ValueError):
        tool.split_names(order, split_list=["zz.png"])
