"""Host side of the streamed path (no GPU): data.ShardedImages against data.ResidentImages over the concatenated array, locate and gather,
the imagenet reader of train.get_dataset on shards written into tmp_path with every refusal, the loader make_loader picks under the four
--data_loader modes for each kind of set, and tools/prepare_images.py --shard_images --recursive."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import data_yardstick as Y
from conftest import ROOT

SIZES = (37, 41, 5)  # images per shard; the set has 83


@pytest.fixture(scope="module")
def M():
    import movae_amd  # noqa: F401
    from movae_amd import data, train

    return data, train


def _shards(h, w, c, seed):
    whole = Y.images(sum(SIZES), h, w, c, seed)
    edges = np.cumsum((0,) + SIZES)
    return whole, [whole[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("h,w,c", [(6, 10, 3), (5, 4, 1)])
def test_sharded_items_are_the_resident_items(M, h, w, c):
    data, _ = M
    whole, shards = _shards(h, w, c, seed=31)
    flips = set()
    for train_set in (True, False):
        for normalize in (False, True):
            sh = data.ShardedImages(shards, normalize, train=train_set, seed=Y.SEED)
            re = data.ResidentImages(whole, normalize, train=train_set, seed=Y.SEED)
            assert len(sh) == len(re) == 83 and sh.normalize == re.normalize and sh.train == re.train and sh.seed == re.seed == Y.SEED
            assert torch.equal(sh.table, re.table) and sh.epoch == re.epoch == 0
            for epoch in Y.EPOCHS:
                sh.set_epoch(epoch)
                re.set_epoch(epoch)
                assert sh.epoch == epoch
                fl = Y.flip_rule(np.arange(83), Y.SEED, epoch)
                for i in range(83):
                    (x, label), (want, _) = sh[i], re[i]
                    assert label == 0 and x.dtype == torch.float32 and tuple(x.shape) == (c, h, w)
                    assert torch.equal(x, want), (train_set, normalize, epoch, i)
                    assert sh.flipped(i) == re.flipped(i) == (bool(fl[i]) and train_set)
                    if normalize:  # once per (set, epoch) is enough for the yardstick's own transform
                        assert torch.equal(x, Y.transform(whole[i], True, bool(fl[i]) and train_set))
                    if train_set:
                        flips.add(sh.flipped(i))
            with pytest.raises(IndexError):
                sh[83]
            with pytest.raises(IndexError):
                sh[-1]
    assert flips == {False, True}


def test_locate_at_every_shard_edge(M):
    data, _ = M
    _, shards = _shards(6, 10, 3, seed=1)
    sh = data.ShardedImages(shards, False, train=True)
    assert [sh.locate(i) for i in (0, 36, 37, 38, 77, 78, 82)] == [(0, 0), (0, 36), (1, 0), (1, 1), (1, 40), (2, 0), (2, 4)]
    assert sh.locate(np.int64(78)) == (2, 0) and all(isinstance(v, int) for v in sh.locate(np.int64(78)))
    for bad in (-1, 83, 1000):
        with pytest.raises(IndexError):
            sh.locate(bad)
    one = data.ResidentImages(shards[0], False, train=True)
    assert one.locate(0) == (0, 0) and one.locate(36) == (0, 36)
    with pytest.raises(IndexError):
        one.locate(37)


def test_gather(M, tmp_path):
    data, _ = M
    whole, shards = _shards(6, 10, 3, seed=2)
    order = [82, 0, 37, 36, 36, 78, 5, 77, 38, 0]  # out of order, repeated, every shard and both sides of both edges
    for k, s in enumerate(shards):  # from maps, as the reader opens them
        np.save(tmp_path / f"s{k}.npy", s)
    maps = [np.load(tmp_path / f"s{k}.npy", mmap_mode="r") for k in range(3)]
    for ds in (data.ShardedImages(shards, True, train=True), data.ShardedImages(maps, False, train=False),
               data.ResidentImages(whole, False, train=True)):
        for idx in (order, np.array(order, dtype=np.int32), torch.tensor(order, dtype=torch.int32).numpy()[2:7], []):
            out = np.full((len(idx), 6, 10, 3), 7, dtype=np.uint8)
            assert ds.gather(idx, out) is out
            assert np.array_equal(out, whole[np.asarray(idx, dtype=np.int64)])  # as stored: neither flipped nor converted
        buf = np.zeros((4, 3, 6, 10, 3), dtype=np.uint8)  # a slice of a larger buffer, like a slot of the loader's ring
        ds.gather([81, 80], buf[2][:2])
        assert np.array_equal(buf[2][:2], whole[[81, 80]]) and not buf[2][2].any() and not buf[1].any() and not buf[3].any()
        for bad in ([0, 83], [-1], [5, 2 ** 31]):
            with pytest.raises(IndexError):
                ds.gather(bad, np.zeros((len(bad), 6, 10, 3), dtype=np.uint8))
        for out in (np.zeros((2, 6, 10, 3), dtype=np.uint8), np.zeros((3, 6, 10, 3), dtype=np.float32), np.zeros((3, 10, 6, 3), dtype=np.uint8),
                    torch.zeros((3, 6, 10, 3), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                ds.gather([1, 2, 3], out)


def test_sharded_images_refuses_other_shards(M):
    data, _ = M
    good = Y.images(2, 4, 4, 3, 0)
    data.ShardedImages([good, good[:1]], False, True)
    for bad in ([], [good, np.zeros((2, 4, 5, 3), np.uint8)], [good, np.zeros((2, 4, 4, 1), np.uint8)], [good, np.zeros((0, 4, 4, 3), np.uint8)],
                [good, good.astype(np.float32)], [np.zeros((2, 4, 4, 2), np.uint8)], [good, torch.zeros(2, 4, 4, 3, dtype=torch.uint8)]):
        with pytest.raises(ValueError):
            data.ShardedImages(bad, False, True)


def _imagenet(root, seed=0):
    """2 train shards of 3 + 2 images and one test file of 2, side 256 -> (train images [5], test images [2])."""
    os.makedirs(root, exist_ok=True)
    tr, te = Y.images(5, 256, 256, 3, seed), Y.images(2, 256, 256, 3, seed + 1)
    np.save(os.path.join(root, "imagenet_train_u8_00000.npy"), tr[:3])
    np.save(os.path.join(root, "imagenet_train_u8_00001.npy"), tr[3:])
    np.save(os.path.join(root, "imagenet_test_u8.npy"), te)
    return tr, te


@pytest.mark.parametrize("normalize", [False, True])
def test_imagenet_reader(M, tmp_path, normalize):
    data, train = M
    tr_u8, te_u8 = _imagenet(str(tmp_path))
    for name in ("imagenet", "ImageNet"):
        tr, te, size = train.get_dataset(name, data_dir=str(tmp_path), normalize=normalize)
        assert size == 256 and type(tr) is data.ShardedImages and type(te) is data.ResidentImages
        assert len(tr) == 5 and len(te) == 2 and tr.train and not te.train and tr.normalize == te.normalize == normalize
        assert [s.shape[0] for s in tr.shards] == [3, 2] and all(isinstance(s, np.memmap) for s in tr.shards)
        assert np.array_equal(te.u8, te_u8)
    out = np.zeros((5, 256, 256, 3), dtype=np.uint8)
    assert np.array_equal(tr.gather(range(5), out), tr_u8)
    tr.seed = Y.SEED
    tr.set_epoch(1)
    fl = Y.flip_rule(np.arange(5), Y.SEED, 1)
    for i in (2, 3):  # the last image of shard 0, the first of shard 1
        assert torch.equal(tr[i][0], Y.transform(tr_u8[i], normalize, bool(fl[i])))
    # max_items: the first 4 train images, over the shard boundary; the first max(1, 4 // 10) test image
    tr, te, _ = train.get_dataset("imagenet", data_dir=str(tmp_path), normalize=normalize, max_items=4)
    assert type(tr) is data.ShardedImages and len(tr) == 4 and [s.shape[0] for s in tr.shards] == [3, 1] and len(te) == 1
    assert np.array_equal(tr.gather(range(4), out[:4]), tr_u8[:4]) and np.array_equal(te.u8, te_u8[:1])
    tr, te, _ = train.get_dataset("imagenet", data_dir=str(tmp_path), max_items=2)  # inside the first shard: the form on disk decides
    assert type(tr) is data.ShardedImages and len(tr) == 2 and len(tr.shards) == 1 and np.array_equal(tr.shards[0], tr_u8[:2])
    tr, te, _ = train.get_dataset("imagenet", data_dir=str(tmp_path), max_items=50)
    assert len(tr) == 5 and len(te) == 2


def test_imagenet_as_single_files_and_sharded_test_split(M, tmp_path):
    data, train = M
    tr_u8, te_u8 = Y.images(3, 256, 256, 3, 5), Y.images(3, 256, 256, 3, 6)
    np.save(tmp_path / "imagenet_train_u8.npy", tr_u8)
    np.save(tmp_path / "imagenet_test_u8_00000.npy", te_u8[:1])
    np.save(tmp_path / "imagenet_test_u8_00001.npy", te_u8[1:])
    tr, te, size = train.get_dataset("imagenet", data_dir=str(tmp_path))
    assert size == 256 and type(tr) is data.ResidentImages and type(te) is data.ShardedImages
    assert np.array_equal(tr.u8, tr_u8) and len(te) == 3 and not te.train
    assert np.array_equal(te.gather([2, 0, 1], np.zeros((3, 256, 256, 3), np.uint8)), te_u8[[2, 0, 1]])


def test_imagenet_refusals(M, tmp_path):
    data, train = M
    root = str(tmp_path / "d")
    # without the train files: the refusal older callers know, now with the remedy
    for where in (root, str(tmp_path)):  # a folder that does not exist, and an empty one
        with pytest.raises(NotImplementedError) as e:
            train.get_dataset("imagenet", data_dir=where)
        msg = str(e.value)
        assert "252 GB" in msg and os.path.join(where, "imagenet_train_u8_00000.npy") in msg and "--shard_images" in msg
        assert "tools/prepare_images.py" in msg and "nothing is downloaded" in msg
    _imagenet(root)
    train.get_dataset("imagenet", data_dir=root)
    # the test split missing: a missing file like any other set's
    os.rename(os.path.join(root, "imagenet_test_u8.npy"), os.path.join(root, "aside.npy"))
    with pytest.raises(FileNotFoundError, match="imagenet_test_u8.npy"):
        train.get_dataset("imagenet", data_dir=root)
    os.rename(os.path.join(root, "aside.npy"), os.path.join(root, "imagenet_test_u8.npy"))
    # both forms of one split
    np.save(os.path.join(root, "imagenet_train_u8.npy"), Y.images(1, 256, 256, 3, 0))
    with pytest.raises(ValueError, match="imagenet_train_u8.npy"):
        train.get_dataset("imagenet", data_dir=root)
    os.remove(os.path.join(root, "imagenet_train_u8.npy"))
    np.save(os.path.join(root, "imagenet_test_u8_00000.npy"), Y.images(1, 256, 256, 3, 0))
    with pytest.raises(ValueError, match="imagenet_test_u8.npy"):
        train.get_dataset("imagenet", data_dir=root)
    os.remove(os.path.join(root, "imagenet_test_u8_00000.npy"))
    # a gap in the numbering names the file that is missing: in the middle, and at the start
    np.save(os.path.join(root, "imagenet_train_u8_00003.npy"), Y.images(1, 256, 256, 3, 0))
    with pytest.raises(ValueError, match="imagenet_train_u8_00002.npy"):
        train.get_dataset("imagenet", data_dir=root)
    os.remove(os.path.join(root, "imagenet_train_u8_00003.npy"))
    os.rename(os.path.join(root, "imagenet_train_u8_00000.npy"), os.path.join(root, "aside.npy"))
    with pytest.raises(ValueError, match="imagenet_train_u8_00000.npy"):
        train.get_dataset("imagenet", data_dir=root)
    os.rename(os.path.join(root, "aside.npy"), os.path.join(root, "imagenet_train_u8_00000.npy"))
    # a wrong dtype, and shapes that differ between shards or from [.][256][256][3]: the file is named
    last = os.path.join(root, "imagenet_train_u8_00001.npy")
    for bad in (np.zeros((2, 256, 256, 3), np.float32), np.zeros((2, 128, 128, 3), np.uint8), np.zeros((2, 256, 256, 1), np.uint8),
                np.zeros((2, 3, 256, 256), np.uint8), np.zeros((0, 256, 256, 3), np.uint8), np.zeros((256, 256, 3), np.uint8)):
        np.save(last, bad)
        with pytest.raises(ValueError, match="imagenet_train_u8_00001.npy"):
            train.get_dataset("imagenet", data_dir=root)
    np.save(last, Y.images(2, 256, 256, 3, 0))
    train.get_dataset("imagenet", data_dir=root)
    # names that only look like shards are not shards
    np.save(os.path.join(root, "imagenet_train_u8_0002.npy"), np.zeros(3))
    np.save(os.path.join(root, "imagenet_train_u8_00002.npy.bak.npy"), np.zeros(3))
    assert len(train.get_dataset("imagenet", data_dir=root)[0]) == 5


def test_other_npy_sets_may_be_sharded(M, tmp_path):
    """The shard form is the reader's, not imagenet's alone; the one-file form of the other sets is tests/test_data_host.py's."""
    data, train = M
    tr_u8, te_u8 = Y.images(5, 64, 64, 3, 1), Y.images(2, 64, 64, 3, 2)
    np.save(tmp_path / "celeba_train_u8_00000.npy", tr_u8[:2])
    np.save(tmp_path / "celeba_train_u8_00001.npy", tr_u8[2:])
    np.save(tmp_path / "celeba_test_u8.npy", te_u8)
    tr, te, size = train.get_dataset("celeba", data_dir=str(tmp_path))
    assert size == 64 and type(tr) is data.ShardedImages and type(te) is data.ResidentImages and len(tr) == 5
    assert np.array_equal(tr.gather([4, 1], np.zeros((2, 64, 64, 3), np.uint8)), tr_u8[[4, 1]])


def _args(train, mode, workers=0):
    a = train.parse_args(["--data_loader", mode, "--num_workers", str(workers)])
    a.seed = 3
    return a


def test_loader_selection(M):
    data, train = M
    cpu = torch.device("cpu")  # no loader touches its device before the first batch
    resident = data.ResidentImages(Y.images(9, 4, 4, 3, 0), False, train=True)
    sharded = data.ShardedImages([Y.images(5, 4, 4, 3, 1), Y.images(4, 4, 4, 3, 2)], False, train=True)
    blob = Y.images(1, 8, 8, 3, 3).reshape(-1)
    ragged = data.RaggedImages(blob, np.array([[0, 8, 8]], dtype=np.int64), 4, False, train=True)
    synthetic, _, _ = train.get_dataset("synthetic_cifar10", max_items=16)
    want = {  # (set, mode) -> loader class, or the words of the refusal
        ("resident", "auto"): data.DeviceBatchLoader, ("resident", "device"): data.DeviceBatchLoader,
        ("resident", "stream"): data.StreamedBatchLoader, ("resident", "host"): torch.utils.data.DataLoader,
        ("sharded", "auto"): data.StreamedBatchLoader, ("sharded", "device"): "--data_loader stream or host",
        ("sharded", "stream"): data.StreamedBatchLoader, ("sharded", "host"): torch.utils.data.DataLoader,
        ("ragged", "auto"): data.RaggedBatchLoader, ("ragged", "device"): data.RaggedBatchLoader,
        ("ragged", "stream"): "RaggedImages", ("ragged", "host"): torch.utils.data.DataLoader,
        ("synthetic", "auto"): torch.utils.data.DataLoader, ("synthetic", "device"): "uint8",
        ("synthetic", "stream"): "uint8", ("synthetic", "host"): torch.utils.data.DataLoader,
    }
    sets = dict(resident=resident, sharded=sharded, ragged=ragged, synthetic=synthetic)
    for (kind, mode), expected in want.items():
        a, ds = _args(train, mode), sets[kind]
        if isinstance(expected, str):
            for fn in (lambda: train.make_loader(ds, 4, cpu, a, shuffle=True), lambda: train.uses_device_loader(ds, a)):
                with pytest.raises(ValueError, match=expected):
                    fn()
            continue
        loader = train.make_loader(ds, 4, cpu, a, shuffle=True)
        assert type(loader) is expected, (kind, mode)
        assert train.uses_device_loader(ds, a) == (expected is not torch.utils.data.DataLoader), (kind, mode)
        assert loader.dataset is ds
        if isinstance(loader, data.ResidentLoader):
            assert loader.seed == 3 and loader.shuffle and (loader.rank, loader.world_size) == (0, 1)

    class Dp:
        rank, world_size = 1, 2

    streamed = train.make_loader(sharded, 4, cpu, _args(train, "auto", workers=4), shuffle=True, dp=Dp())
    assert (streamed.rank, streamed.world_size, streamed.workers, streamed.depth, streamed.timeout) == (1, 2, 4, 3, 600.0)
    assert len(streamed) == 2 and streamed.indices(1) == data.shard_indices(9, True, 3, 1, 1, 2) and streamed.streamed == 0
    # --num_workers sizes the gather pool: at least one thread, at most eight
    assert [train.make_loader(sharded, 4, cpu, _args(train, "stream", w), shuffle=False).workers for w in (0, 1, 5, 8, 64)] == [1, 1, 5, 8, 8]
    with pytest.raises(TypeError):
        data.StreamedBatchLoader(ragged, 4, cpu, shuffle=True)
    with pytest.raises(TypeError):
        data.DeviceBatchLoader(sharded, 4, cpu, shuffle=True)
    # the host DataLoader over a ShardedImages: the item contract, the epoch set on the set (what train.main does on this path)
    host = train.make_loader(sharded, 4, cpu, _args(train, "host"), shuffle=False)
    sharded.seed = Y.SEED
    whole = np.concatenate(sharded.shards)
    for epoch in Y.EPOCHS:
        sharded.set_epoch(epoch)
        got = torch.cat([x for x, _ in host])
        assert torch.equal(got, Y.expected_batch(whole, list(range(9)), False, True, Y.SEED, epoch))


def test_parser_accepts_stream(M):
    _, train = M
    assert train.parse_args(["--data_loader", "stream"]).data_loader == "stream"
    assert train.parse_args([]).data_loader == "auto"
    with pytest.raises(SystemExit):
        train.parse_args(["--data_loader", "streamed"])


def test_prepare_images_shards(tmp_path):
    """--shard_images 2 --recursive on a tree of class folders: shards of at most 2 images in the order of the relative paths; the same
    data without the flag gives the single file, with equal bytes."""
    from PIL import Image

    spec = importlib.util.spec_from_file_location("prepare_images", os.path.join(ROOT, "tools", "prepare_images.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = tmp_path / "src"
    rng = np.random.default_rng(4)
    rel = ["n02/b.png", "n01/z.png", "n01/a.png", "top.png", "n03/deep/c.png", "n02/a.png", "n01/m.png"]  # written out of order
    for r in rel:
        (src / r).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, size=(12, 10, 3), dtype=np.uint8)).save(src / r)
    (src / "n01" / "notes.txt").write_text("not an image")
    order = sorted(os.path.join(*r.split("/")) for r in rel)
    assert tool.list_images(str(src), recursive=True) == order and tool.list_images(str(src)) == ["top.png"]

    def want(r):
        return np.asarray(Image.open(src / r).convert("RGB").resize((8, 8), Image.BICUBIC))

    common = ["--src", str(src), "--name", "imagenet", "--size", "8", "--split", "0.72", "--recursive"]  # int(7 * 0.72) = 5 train, 2 test
    tool.main(common + ["--out", str(tmp_path / "sharded"), "--shard_images", "2"])
    tool.main(common + ["--out", str(tmp_path / "whole")])
    assert sorted(os.listdir(tmp_path / "sharded")) == ["imagenet_test_u8_00000.npy", "imagenet_train_u8_00000.npy",
                                                        "imagenet_train_u8_00001.npy", "imagenet_train_u8_00002.npy"]
    assert sorted(os.listdir(tmp_path / "whole")) == ["imagenet_test_u8.npy", "imagenet_train_u8.npy"]
    shards = [np.load(tmp_path / "sharded" / f"imagenet_train_u8_0000{k}.npy") for k in range(3)]
    assert [s.shape for s in shards] == [(2, 8, 8, 3), (2, 8, 8, 3), (1, 8, 8, 3)] and all(s.dtype == np.uint8 for s in shards)
    train_whole, test_whole = np.load(tmp_path / "whole" / "imagenet_train_u8.npy"), np.load(tmp_path / "whole" / "imagenet_test_u8.npy")
    assert np.concatenate(shards).tobytes() == train_whole.tobytes()
    assert np.load(tmp_path / "sharded" / "imagenet_test_u8_00000.npy").tobytes() == test_whole.tobytes()
    for k, r in enumerate(order[:5]):
        assert np.array_equal(train_whole[k], want(r)), r
    for k, r in enumerate(order[5:]):
        assert np.array_equal(test_whole[k], want(r)), r
    # the shards are what the reader takes (side 8 is not imagenet's: read them as the arrays they are)
    import movae_amd  # noqa: F401
    from movae_amd import data

    ds = data.ShardedImages([np.load(tmp_path / "sharded" / f"imagenet_train_u8_0000{k}.npy", mmap_mode="r") for k in range(3)], False, True)
    assert np.array_equal(ds.gather(range(5), np.zeros((5, 8, 8, 3), np.uint8)), train_whole)
    # without --recursive the sub-folders are not entered, and a shard size below 1 is refused
    with pytest.raises(ValueError):
        tool.convert(str(src), str(tmp_path / "bad"), "imagenet", 8, shard_images=0, recursive=True)
    paths = tool.convert(str(src), str(tmp_path / "flat"), "imagenet", 8)
    assert [os.path.basename(p) for p in paths] == ["imagenet_train_u8.npy"] and np.load(paths[0]).shape == (1, 8, 8, 3)
