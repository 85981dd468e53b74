"""Real image sets from disk, resident on the device as uint8, batches assembled by one HIP kernel.

The reference's pipeline is a per-item transform on PIL images (utils/utils.py:180-422: RandomHorizontalFlip -> ToTensor -> optional
Normalize(0.5, 0.5)).  Here the whole set is one uint8 array [N][H][W][C]; ToTensor / Normalize become a 256-entry table per channel,
computed once with the reference's own torch expressions, and the flip of image i in epoch e is bit 31 of word 0 of
Philox4x32-10(counter = (i, e), key = seed) -- a pure function of (seed, epoch, dataset index), the same on the host
(ResidentImages.__getitem__) and on the device (DeviceBatchLoader -> ops.batch_u8 -> movae_batch_u8).  Nothing is downloaded: the
readers take the files a user already has (the CIFAR pickles torchvision unpacks; .npy arrays written by tools/prepare_images.py)."""
import math
import os
import pickle
import weakref

import numpy as np
import torch

from . import ops

_M32 = np.uint64(0xFFFFFFFF)


def philox_word0(counter_lo, counter_hi, key):
    """Word 0 of Philox4x32-10 for the 64-bit counters (counter_lo, counter_hi) under the 64-bit key, vectorised over counter_lo
    (csrc/common.h: philox4x32_10 with c = (lo low word, lo high word, hi low word, hi high word), k = (key low word, key high word))."""
    lo = np.atleast_1d(np.asarray(counter_lo)).astype(np.uint64)
    hi, key = int(counter_hi) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1)
    c0, c1 = lo & _M32, lo >> np.uint64(32)
    c2 = np.full_like(c0, hi & 0xFFFFFFFF)
    c3 = np.full_like(c0, hi >> 32)
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    m0, m1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def flip_bits(indices, seed, epoch):
    """bool[len(indices)]: which dataset indices are flipped in `epoch` under `seed`."""
    return (philox_word0(indices, epoch, seed) >> np.uint64(31)).astype(bool)


def value_table(channels, normalize):
    """float32 [channels][256]: the value of every byte.  u / 255 is ToTensor's `.to(float32).div(255)`; with `normalize`,
    `.sub(0.5).div(0.5)` is Normalize's `sub_(mean).div_(std)` with the 0.5s every set of the reference uses."""
    t = torch.arange(256, dtype=torch.float32).div(255)
    t = t.repeat(channels, 1)
    if normalize:
        mean, std = torch.full((channels, 1), 0.5), torch.full((channels, 1), 0.5)
        t = t.sub(mean).div(std)
    return t.contiguous()


class ResidentImages(torch.utils.data.Dataset):
    """A uint8 image set [N][H][W][C] (C in {1, 3}; a numpy array or an np.load(mmap_mode="r") map) with the reference's transforms as
    a table.  Item i is (CHW float tensor, 0): the host form of what DeviceBatchLoader assembles on the device, bit for bit, for the
    same (index, epoch) -- flipped only when `train`."""

    def __init__(self, u8, normalize, train, seed=0):
        if not isinstance(u8, np.ndarray) or u8.dtype != np.uint8 or u8.ndim != 4 or u8.shape[3] not in (1, 3) or 0 in u8.shape:
            raise ValueError(f"ResidentImages: a non-empty uint8 array [N][H][W][C] with C in (1, 3), got "
                             f"{getattr(u8, 'dtype', type(u8))} {getattr(u8, 'shape', None)}")
        self.u8, self.normalize, self.train, self.seed, self.epoch = u8, bool(normalize), bool(train), int(seed), 0
        self.table = value_table(u8.shape[3], normalize)
        self._chan = torch.arange(u8.shape[3]).reshape(-1, 1, 1)
        self._flips = (None, None)  # ((seed, epoch), bool[N])

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.u8.shape[0]

    def flipped(self, i):
        if not self.train:
            return False
        if self._flips[0] != (self.seed, self.epoch):  # the whole epoch's bits at once: one vectorised Philox pass
            self._flips = ((self.seed, self.epoch), flip_bits(np.arange(len(self)), self.seed, self.epoch))
        return bool(self._flips[1][i])

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        img = np.array(self.u8[i])  # HWC (a copy: a read-only map stays untouched)
        if self.flipped(i):
            img = img[:, ::-1]
        codes = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).long()
        return self.table[self._chan, codes], 0


def shard_indices(n, shuffle, seed, epoch, rank=0, world_size=1):
    """The epoch's index list of one rank: torch.utils.data.distributed.DistributedSampler(shuffle=shuffle, seed=seed,
    drop_last=False) after set_epoch(epoch), restated (world_size == 1 is the same rule: the whole permutation)."""
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} outside world of {world_size}")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = math.ceil(n / world_size) * world_size
    pad = total - n
    if pad:
        idx += (idx * math.ceil(pad / n))[:pad]
    return idx[rank:total:world_size]


def refuse_if_too_big(need, device, what, advice):
    """The residency rule of every store kept on the device, checked before its upload: at most half of the memory free there."""
    free, _ = torch.cuda.mem_get_info(device)
    if need > free // 2:
        raise RuntimeError(f"{what} {need} bytes on {device}, more than half of the {free} bytes free there; {advice}")


class ResidentLoader:
    """Iterable over the batches of a set whose rows are resident on the device: the epoch's index list of this rank (shard_indices)
    is range-checked on the host and uploaded once per epoch as int32, the set itself on first use, and every batch is one
    self._batch(rows) over a slice of `batch_size` row numbers.  drop_last=False: the last batch is ragged."""

    # what a subclass gives --
    # noun: what a row is, for the messages
    # _upload(): make the set resident (called once, on first use); refuses a set that does not fit (refuse_if_too_big)
    # _batch(rows): the batch of the device int32 row numbers `rows` -- what the iteration yields
    # _checked(idx): the host index list as a CPU int32 tensor, refused unless every entry is a row of the set
    noun = "rows"

    def __init__(self, ds, batch_size, device, shuffle=True, rank=0, world_size=1, seed=0):
        if batch_size <= 0:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if len(ds) >= 2 ** 31:
            raise ValueError(f"{len(ds)} {self.noun}: row numbers are int32")
        self.dataset, self.batch_size, self.device = ds, int(batch_size), torch.device(device)
        self.shuffle, self.rank, self.world_size, self.seed, self.epoch = bool(shuffle), int(rank), int(world_size), int(seed), 0
        self._uploaded = False
        self._idx = (None, None)  # (epoch, device int32 list)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self, epoch=None):
        """This rank's index list of `epoch` (default: the current one), on the host; no device is touched."""
        return shard_indices(len(self.dataset), self.shuffle, self.seed, self.epoch if epoch is None else int(epoch), self.rank,
                             self.world_size)

    def __len__(self):
        per_rank = math.ceil(len(self.dataset) / self.world_size)
        return math.ceil(per_rank / self.batch_size)

    def _device_indices(self):
        if self._idx[0] != self.epoch:
            rows = self._checked(self.indices())  # on the host: a bad list is refused before anything reaches the device
            if not self._uploaded:  # (and a set that does not fit before the list's upload)
                self._upload()
                self._uploaded = True
            self._idx = (self.epoch, rows.to(self.device))
        return self._idx[1]

    def __iter__(self):
        idx = self._device_indices()
        for s in range(0, idx.numel(), self.batch_size):
            yield self._batch(idx[s:s + self.batch_size])


#: (address, shape, strides of the host array, device) -> its uint8 copy on the device, while any loader holds it
_STORES = weakref.WeakValueDictionary()


class DeviceBatchLoader(ResidentLoader):
    """ResidentLoader over the (images, labels) batches of a ResidentImages: the uint8 set and its table are uploaded on first use,
    and every batch is ONE movae_batch_u8 launch into a fresh NHWC buffer, handed out as its logical-NCHW view (ops.to_nhwc of it is
    zero-copy).  Labels are zeros, like item[1]."""

    noun = "images"

    def __init__(self, ds, batch_size, device, shuffle, rank=0, world_size=1, seed=0):
        if not isinstance(ds, ResidentImages):
            raise TypeError(f"DeviceBatchLoader needs a ResidentImages, got {type(ds).__name__}")
        super().__init__(ds, batch_size, device, shuffle, rank, world_size, seed)
        self._store = self._lut = self._zeros = None

    def _upload(self):
        u8 = self.dataset.u8
        # loaders over the same host array on the same device share ONE store (the train and the prior loader of a run; AFHQ's train
        # and test set): the entry lives as long as a loader holds the store, and so no longer than the array whose address names it
        key = (u8.__array_interface__["data"][0], u8.shape, u8.strides, str(self.device))
        store = _STORES.get(key)
        if store is None:
            refuse_if_too_big(int(u8.nbytes) + self.dataset.table.numel() * 4, self.device, "the image set needs",
                              "keep it on the host with --data_loader host")
            store = torch.empty(u8.shape, dtype=torch.uint8, device=self.device)
            rows = max(1, (256 << 20) // max(1, int(u8[0].nbytes)))  # staged through <= 256 MB of host memory (the array may be a map)
            for s in range(0, u8.shape[0], rows):
                store[s:s + rows].copy_(torch.from_numpy(np.array(u8[s:s + rows])))
            _STORES[key] = store
        self._store = store
        self._lut = self.dataset.table.to(self.device)
        self._zeros = torch.zeros(self.batch_size, dtype=torch.long, device=self.device)

    def _checked(self, idx):
        if idx and not 0 <= min(idx) <= max(idx) < len(self.dataset):
            raise RuntimeError("DeviceBatchLoader: index list outside the store")
        return torch.tensor(idx, dtype=torch.int32)  # (an empty list gives an empty iteration)

    def _batch(self, rows):
        ds = self.dataset
        out = ops.batch_u8(self._store, rows, self._lut, flip=ds.train, seed=ds.seed, epoch=self.epoch)
        return out.permute(0, 3, 1, 2), self._zeros[:rows.numel()]


# ---- readers -----------------------------------------------------------------------------------------------------------------------
#: name -> image side of the .npy sets: <data_dir>/<name>_train_u8.npy and <name>_test_u8.npy, uint8 [N][S][S][3]
NPY_SETS = {"celeba": 64, "celeba-128": 128, "celeba-hq": 256, "afhq": 256}
ALIASES = {"animal-face": "afhq"}
REFUSED = {
    "imagenet": "1.28 M images of 256 x 256 are 252 GB as uint8: they do not fit one device and would have to stream from host memory",
    "oxford-flower-102": "its training transform is RandomResizedCrop, a per-item resample that the table-and-flip kernel does not do",
}


def _need(path):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} is missing: datasets are read from files already on disk, nothing is downloaded")
    return path


def _cifar_rows(path):
    with open(_need(path), "rb") as f:
        d = pickle.load(f, encoding="latin1")
    data = d.get("data") if isinstance(d, dict) else None
    if data is None and isinstance(d, dict):
        data = d.get(b"data")
    data = np.asarray(data) if data is not None else None
    if data is None or data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != 3072:
        raise ValueError(f"{path}: expected key 'data' as uint8 [N][3072], got "
                         f"{None if data is None else (data.dtype, data.shape)}")
    return data


def _cifar(files_train, files_test):
    """Planar R, G, B rows [N][3072] -> HWC [N][32][32][3], transposed once."""
    hwc = lambda files: np.ascontiguousarray(  # noqa: E731
        np.concatenate([_cifar_rows(p) for p in files]).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
    return hwc(files_train), hwc(files_test)


def _npy(path, size):
    a = np.load(_need(path), mmap_mode="r", allow_pickle=False)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[0] == 0 or tuple(a.shape[1:]) != (size, size, 3):
        raise ValueError(f"{path}: expected uint8 [N][{size}][{size}][3], got {a.dtype} {a.shape}")
    return a


def get_real_dataset(name, data_dir="./data", normalize=False, max_items=None):
    """-> (train ResidentImages, test ResidentImages, image side) for a real dataset name of the reference (case-insensitive), or None
    for a name this module does not know.  `max_items` keeps the first max_items train and the first max(1, max_items // 10) test images."""
    key = name.lower()
    key = ALIASES.get(key, key)
    if key in REFUSED:
        raise NotImplementedError(f"dataset {name!r}: {REFUSED[key]}")
    if key == "cifar10":
        root = os.path.join(data_dir, "cifar-10-batches-py")
        train, test = _cifar([os.path.join(root, f"data_batch_{i}") for i in range(1, 6)], [os.path.join(root, "test_batch")])
        size = 32
    elif key == "cifar100":
        root = os.path.join(data_dir, "cifar-100-python")
        train, test = _cifar([os.path.join(root, "train")], [os.path.join(root, "test")])
        size = 32
    elif key in NPY_SETS:
        size = NPY_SETS[key]
        train = _npy(os.path.join(data_dir, f"{key}_train_u8.npy"), size)
        # AFHQ has one split in the reference (utils/utils.py:420-422): the train images serve as the test set too
        test = train if key == "afhq" else _npy(os.path.join(data_dir, f"{key}_test_u8.npy"), size)
    else:
        return None
    if max_items:
        train, test = train[:max_items], test[:max(1, max_items // 10)]
    return ResidentImages(train, normalize, train=True), ResidentImages(test, normalize, train=False), size
