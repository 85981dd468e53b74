"""Host side of the RandomResizedCrop path (no GPU): data.resize_u8 against Pillow's recorded outputs (tests/golden/rrc_tiny.npz) and
against Pillow itself, data.rrc_boxes against torchvision's rule restated on the Philox streams, tools/prepare_images.py --ragged, the
oxford-flower-102 reader, RaggedImages.__getitem__ against the restated pipeline, and the host loader over two epochs."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import data_yardstick as Y
import rrc_yardstick as R
from conftest import ROOT, load_golden

SEED = Y.SEED
BIG = ((3 << 32) | 9, (1 << 32) | 2)  # a 64-bit (seed, epoch)


@pytest.fixture(scope="module")
def M():
    import movae_amd  # noqa: F401
    from movae_amd import data, train

    return data, train


@pytest.fixture(scope="module")
def cases():
    return R.load_cases(load_golden("rrc_tiny"))


def _crop(c):
    top, left, bh, bw = c["box"]
    return c["src"][top:top + bh, left:left + bw]


def test_resize_equals_the_fixture(M, cases):
    data, _ = M
    assert len(cases) >= 40
    for k, c in enumerate(cases):
        got = data.resize_u8(_crop(c), c["s"])
        assert got.dtype == np.uint8 and np.array_equal(got, c["out"]), (k, c["box"], c["s"])
        assert np.array_equal(R.resize(_crop(c), c["s"]), c["out"]), k  # and so does the yardstick the other tests lean on


def test_resize_equals_pillow_on_fresh_cases(M):
    Image = pytest.importorskip("PIL.Image")
    data, _ = M
    rng = np.random.default_rng(77)
    for k in range(30):
        s = int(rng.choice([4, 8, 16, 32, 40]))
        h, w = (int(v) for v in rng.integers(1, min(8 * s, 90) + 1, size=2))
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        if k % 5 == 0:
            a = (rng.integers(0, 2, size=a.shape) * 255).astype(np.uint8)
        bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        top, left = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        want = np.asarray(Image.fromarray(a).crop((left, top, left + bw, top + bh)).resize((s, s), Image.BICUBIC))
        assert np.array_equal(data.resize_u8(a[top:top + bh, left:left + bw], s), want), (k, h, w, (top, left, bh, bw), s)


def test_boxes_follow_the_restated_rule(M):
    data, _ = M
    rng = np.random.default_rng(3)
    dims = np.stack([rng.integers(1, 900, 200), rng.integers(1, 900, 200)], 1)
    for seed, epoch in ((SEED, 0), BIG):
        got = data.rrc_boxes(dims, seed, epoch)
        assert got.dtype == np.int32 and got.shape == (200, 4)
        assert np.array_equal(got, R.boxes(dims, seed, epoch)), (seed, epoch)
        top, left, bh, bw = (got[:, k].astype(np.int64) for k in range(4))
        h, w = dims[:, 0], dims[:, 1]
        assert (top >= 0).all() and (left >= 0).all() and (bh >= 1).all() and (bw >= 1).all()
        assert (top + bh <= h).all() and (left + bw <= w).all()
        # area share in [0.7, 1] and aspect in [3/4, 4/3] up to the rounding of the sides (each side moves by at most a half)
        tried = (np.minimum(h, w) >= 8) & (np.maximum(h, w) * 3 <= np.minimum(h, w) * 4)  # (no fallback: the ratio already fits)
        assert tried.sum() > 20
        for i in np.flatnonzero(tried):
            lo_a, hi_a = (bh[i] - .5) * (bw[i] - .5) / (h[i] * w[i]), (bh[i] + .5) * (bw[i] + .5) / (h[i] * w[i])
            assert hi_a >= 0.7 and lo_a <= 1.0, (i, dims[i], got[i])
            assert (bw[i] + .5) / (bh[i] - .5) >= 3 / 4 and (bw[i] - .5) / (bh[i] + .5) <= 4 / 3, (i, dims[i], got[i])
    assert not np.array_equal(data.rrc_boxes(dims, SEED, 0), data.rrc_boxes(dims, SEED, 1))
    assert not np.array_equal(data.rrc_boxes(dims, SEED, 0), data.rrc_boxes(dims, SEED + 1, 0))


def test_fallback_is_the_central_crop(M):
    data, _ = M
    for seed, epoch in ((SEED, 0), (SEED, 1), BIG):  # whatever is drawn: no try fits such an image
        got = data.rrc_boxes(np.array([[10, 100], [100, 10]]), seed, epoch)
        assert got[0].tolist() == [0, 43, 10, 13] and got[1].tolist() == [43, 0, 13, 10]  # central 10 x 13 and 13 x 10


def test_box_depends_on_seed_epoch_index_only(M):
    """Not on the other images of the set, nor on their number; the flip bit is data.flip_bits' (stream 0), untouched by the crops."""
    data, _ = M
    dims = np.array([[60, 80]] * 9)
    whole = data.rrc_boxes(dims, SEED, 1)
    assert len({tuple(b) for b in whole.tolist()}) > 1, "same size, different index: different boxes"
    other = dims.copy()
    other[:4] = (300, 200)
    assert np.array_equal(data.rrc_boxes(other, SEED, 1)[4:], whole[4:])
    assert np.array_equal(data.rrc_boxes(dims[:5], SEED, 1), whole[:5])
    blob, index = R.pack([Y.images(1, 6, 8, 3, k)[0] for k in range(24)])
    ds = data.RaggedImages(blob, index, 4, False, train=True, seed=SEED)
    for epoch in Y.EPOCHS:
        ds.set_epoch(epoch)
        fl = Y.flip_rule(np.arange(24), SEED, epoch)
        assert np.array_equal(data.flip_bits(np.arange(24), SEED, epoch), fl) and np.array_equal(ds._draws()[1], fl)


def _tool():
    spec = importlib.util.spec_from_file_location("prepare_images", os.path.join(ROOT, "tools", "prepare_images.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _write_pngs(src, sizes, seed=3):
    from PIL import Image

    src.mkdir()
    rng = np.random.default_rng(seed)
    raw = {}
    for k, (h, w) in enumerate(sizes):
        raw[f"im{k:02d}.png"] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        Image.fromarray(raw[f"im{k:02d}.png"]).save(src / f"im{k:02d}.png")
    return raw


SIZES = [(9, 14), (12, 12), (17, 11), (8, 20), (13, 9), (10, 10), (15, 16)]


def test_prepare_images_ragged(tmp_path):
    """Seven PNGs of different sizes -> the prepared oxford-flower-102 files at S = 256; the first five are the train part."""
    from PIL import Image

    raw = _write_pngs(tmp_path / "src", SIZES)
    names = sorted(raw)
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(names[:5]) + "\n")
    out = tmp_path / "data"
    _tool().main(["--src", str(tmp_path / "src"), "--out", str(out), "--name", "oxford-flower-102", "--size", "256", "--ragged",
                  "--split_list", str(lst)])
    train_raw, test_raw = [raw[n] for n in names[:5]], [raw[n] for n in names[5:]]
    assert sorted(os.listdir(out)) == ["oxford-flower-102_test_u8.npy", "oxford-flower-102_train_ragged_index.npy",
                                       "oxford-flower-102_train_ragged_u8.npy"]
    blob = np.load(out / "oxford-flower-102_train_ragged_u8.npy", allow_pickle=False)
    index = np.load(out / "oxford-flower-102_train_ragged_index.npy", allow_pickle=False)
    assert blob.dtype == np.uint8 and blob.ndim == 1 and index.dtype == np.int64 and index.shape == (5, 3)
    want_blob, want_index = R.pack(train_raw)
    assert np.array_equal(index, want_index) and np.array_equal(blob, want_blob)  # own sizes, no resampling, back to back
    test = np.load(out / "oxford-flower-102_test_u8.npy", allow_pickle=False)
    assert test.shape == (2, 256, 256, 3)
    for k, a in enumerate(test_raw):
        assert np.array_equal(test[k], np.asarray(Image.fromarray(a).resize((256, 256), Image.BICUBIC)))


def test_reader_and_items(M, tmp_path):
    """The three files in their on-disk form, written with numpy alone: the reader needs no Pillow."""
    data, train = M
    rng = np.random.default_rng(3)
    train_raw = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SIZES[:5]]
    blob, index = R.pack(train_raw)
    out = tmp_path / "data"
    out.mkdir()
    np.save(out / "oxford-flower-102_train_ragged_u8.npy", blob)
    np.save(out / "oxford-flower-102_train_ragged_index.npy", index)
    test_u8 = Y.images(2, 256, 256, 3, seed=9)
    np.save(out / "oxford-flower-102_test_u8.npy", test_u8)
    for normalize in (False, True):
        tr, te, size = train.get_dataset("oxford-flower-102", data_dir=str(out), normalize=normalize)
        assert isinstance(tr, data.RaggedImages) and isinstance(te, data.ResidentImages) and size == 256
        assert len(tr) == 5 and len(te) == 2 and tr.train and not te.train and tr.kmax == 5
        assert np.array_equal(te.u8, test_u8) and tr.normalize == te.normalize == normalize
    tr.seed = SEED
    dims = np.array([a.shape[:2] for a in train_raw])
    seen = set()
    for epoch in Y.EPOCHS:
        tr.set_epoch(epoch)
        boxes, fl = R.boxes(dims, SEED, epoch), Y.flip_rule(np.arange(5), SEED, epoch)
        seen.update(fl.tolist())
        for i in range(5):
            x, label = tr[i]
            assert label == 0 and x.dtype == torch.float32 and tuple(x.shape) == (3, 256, 256)
            assert torch.equal(x, R.item(train_raw[i], boxes[i], 256, True, bool(fl[i]))), (epoch, i)
    assert seen == {False, True}
    tr2, te2, _ = train.get_dataset("Oxford-Flower-102", data_dir=str(out), max_items=3)
    assert len(tr2) == 3 and len(te2) == 1 and np.array_equal(tr2.dims, dims[:3])
    assert tr2.blob.shape[0] == index[3, 0], "max_items keeps the blob up to the end of the last image kept, no further"
    tr2.seed = SEED
    assert torch.equal(tr2[2][0], R.item(train_raw[2], R.boxes(dims[:3], SEED, 0)[2], 256, False, bool(Y.flip_rule([2], SEED, 0)[0])))
    with pytest.raises(IndexError):
        tr[5]
    # without the prepared files the set stays "not available": type and wording as before, plus where the files come from
    with pytest.raises(NotImplementedError, match="RandomResizedCrop") as e:
        train.get_dataset("oxford-flower-102", data_dir=str(out / "nowhere"))
    msg = str(e.value)
    assert os.path.join(str(out / "nowhere"), "oxford-flower-102_train_ragged_u8.npy") in msg
    assert "prepare_images.py --ragged" in msg and "download" in msg
    with pytest.raises(NotImplementedError, match="252 GB"):
        train.get_dataset("imagenet", data_dir=str(out))


def test_items_at_a_small_side(M):
    """The same rule at s = 16 over images up to 8 x the side, both channel tables; an evaluation set resizes the whole image."""
    data, _ = M
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, size=(int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(5, 129, size=(12, 2))]
    blob, index = R.pack(imgs, lead=1)
    for normalize in (False, True):
        tr = data.RaggedImages(blob, index, 16, normalize, train=True, seed=SEED)
        te = data.RaggedImages(blob, index, 16, normalize, train=False, seed=SEED)
        assert tr.kmax == 2 * math.ceil(2 * max(1.0, index[:, 1:].max() / 16)) + 1
        tr.set_epoch(1)
        boxes, fl = R.boxes(index[:, 1:], SEED, 1), Y.flip_rule(np.arange(12), SEED, 1)
        for i in range(12):
            assert torch.equal(tr[i][0], R.item(imgs[i], boxes[i], 16, normalize, bool(fl[i]))), i
            assert torch.equal(te[i][0], Y.transform(R.resize(imgs[i], 16), normalize, False)), i


def test_bad_index_and_oversized_image_are_refused(M):
    data, _ = M
    blob = np.zeros(3 * (4 * 5 + 6 * 2), np.uint8)
    good = np.array([[0, 4, 5], [60, 6, 2]], dtype=np.int64)
    data.RaggedImages(blob, good, 8, False, True)
    for bad, word in ((np.array([[0, 4, 5], [61, 6, 2]]), "row 1 spans"),     # runs past the blob
                      (np.array([[-1, 4, 5], [60, 6, 2]]), "row 0 spans"),    # negative offset
                      (np.array([[0, 4, 5], [59, 6, 2]]), "overlap"),         # one byte into its neighbour
                      (np.array([[0, 0, 5], [60, 6, 2]]), "row 0 has h, w"),  # h = 0
                      (np.array([[0, 4, 5], [60, 6, -2]]), "row 1 has h, w")):
        with pytest.raises(ValueError, match=word):
            data.RaggedImages(blob, bad.astype(np.int64), 8, False, True)
    for bad in (good.astype(np.float64), good[:, :2], good[:0]):
        with pytest.raises(ValueError, match="index"):
            data.RaggedImages(blob, bad, 8, False, True)
    with pytest.raises(ValueError, match="blob"):
        data.RaggedImages(blob.astype(np.int8), good, 8, False, True)
    # the cap: a side of more than 8 x the output side, named with its row
    wide = np.zeros(3 * (4 * 5 + 1 * 33), np.uint8)
    with pytest.raises(ValueError, match=r"row 1 is an image of 1 x 33.*at most 8 x the output side 4 = 32"):
        data.RaggedImages(wide, np.array([[0, 4, 5], [60, 1, 33]], dtype=np.int64), 4, False, True)
    data.RaggedImages(wide, np.array([[0, 4, 5], [60, 1, 32]], dtype=np.int64), 4, False, True)  # exactly 8 x is inside


@pytest.mark.parametrize("workers", [0, 2])
def test_host_loader_crops_follow_the_epoch(M, workers):
    """`--data_loader host` through train.make_loader: the same items with and without worker processes over two epochs (a worker holds
    a copy of the set, so it must be a fresh one per epoch), and other crops in the second epoch."""
    data, train = M
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, size=(int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(12, 40, size=(10, 2))]
    blob, index = R.pack(imgs)
    ds = data.RaggedImages(blob, index, 8, False, train=True, seed=SEED)
    a = train.parse_args(["--data_loader", "host", "--num_workers", str(workers)])
    assert not train.uses_device_loader(ds, a)
    loader = train.make_loader(ds, 4, torch.device("cpu"), a, shuffle=False)
    assert isinstance(loader, torch.utils.data.DataLoader) and loader.num_workers == workers
    for mode in ("auto", "device"):
        assert train.uses_device_loader(ds, train.parse_args(["--data_loader", mode]))
    boxes = {e: R.boxes(index[:, 1:], SEED, e) for e in (1, 2)}
    assert not np.array_equal(boxes[1], boxes[2])
    for epoch in (1, 2):
        ds.set_epoch(epoch)
        got = torch.cat([x for x, _ in loader])
        fl = Y.flip_rule(np.arange(10), SEED, epoch)
        want = torch.stack([R.item(imgs[i], boxes[epoch][i], 8, False, bool(fl[i])) for i in range(10)])
        assert torch.equal(got, want), (workers, epoch)
