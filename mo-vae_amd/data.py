"""Real image sets from disk, resident on the device as uint8, batches assembled by one HIP kernel.

The reference's pipeline is a per-item transform on PIL images (utils/utils.py:180-422: RandomHorizontalFlip -> ToTensor -> optional
Normalize(0.5, 0.5)).  Here the whole set is one uint8 array [N][H][W][C]; ToTensor / Normalize become a 256-entry table per channel,
computed once with the reference's own torch expressions, and the flip of image i in epoch e is bit 31 of word 0 of
Philox4x32-10(counter = (i, e), key = seed) -- a pure function of (seed, epoch, dataset index), the same on the host
(ResidentImages.__getitem__) and on the device (DeviceBatchLoader -> ops.batch_u8 -> movae_batch_u8).  Nothing is downloaded: the
readers take the files a user already has (the CIFAR pickles torchvision unpacks; .npy arrays written by tools/prepare_images.py).

A set whose pipeline starts with RandomResizedCrop (oxford-flower-102, utils/utils.py:367-397) is kept RAGGED instead: the images at
their own sizes back to back in one uint8 blob (RaggedImages), the epoch's crop boxes drawn on the host from further Philox streams
of the same counter (rrc_boxes), and the crop, PIL's 8-bit bicubic resample restated bit for bit (resize_u8), the flip and the table
done per batch by one launch (RaggedBatchLoader -> ops.batch_rrc_u8 -> movae_batch_rrc_u8).

A set that does not fit the device (imagenet) STREAMS from host memory instead: its shards stay np.load maps (ShardedImages), pool
threads gather each batch's rows into page-locked slots, and the device step is one copy and one launch (StreamedBatchLoader ->
ops.batch_u8_staged -> movae_batch_u8_staged), the same pixels for the same (seed, epoch, dataset index)."""
import math
import os
import pickle
import re
import weakref

import numpy as np
import torch

from . import ops

_M32 = np.uint64(0xFFFFFFFF)


def philox_word0(counter_lo, counter_hi, key):
    """Word 0 of philox_words."""
    return philox_words(counter_lo, counter_hi, key)[0]


def philox_words(counter_lo, counter_hi, key):
    """The four words of Philox4x32-10 for the 64-bit counters (counter_lo, counter_hi) under the 64-bit key, vectorised over counter_lo
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
    return c0, c1, c2, c3


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


def _is_u8_images(u8):
    return isinstance(u8, np.ndarray) and u8.dtype == np.uint8 and u8.ndim == 4 and u8.shape[3] in (1, 3) and 0 not in u8.shape


class _TableImages(torch.utils.data.Dataset):
    """What ResidentImages and ShardedImages share: a uint8 set [N][H][W][C] held as `shards` (arrays [n_k][H][W][C], in order) with
    the reference's transforms as a table and the Philox flip rule.  Item i of the set is row `i - starts[k]` of shard k (locate)."""

    def _setup(self, normalize, train, seed):
        channels = self.shards[0].shape[3]
        self.normalize, self.train, self.seed, self.epoch = bool(normalize), bool(train), int(seed), 0
        self.table = value_table(channels, normalize)
        self._chan = torch.arange(channels).reshape(-1, 1, 1)
        self._flips = (None, None)  # ((seed, epoch), bool[N])

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    @property
    def image_shape(self):
        """(H, W, C) of every image."""
        return tuple(self.shards[0].shape[1:])

    def locate(self, i):
        """-> (shard number, row in that shard) of image i."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        k = int(np.searchsorted(self.starts, i, side="right")) - 1
        return k, i - int(self.starts[k])

    def gather(self, indices, out):
        """Fills the numpy uint8 array out[j] ([len(indices)][H][W][C]) with image indices[j] as it is stored (no flip, no table), in the
        order given; any order, repeats allowed.  IndexError for an index outside the set.  Host memory only: this is the one function
        StreamedBatchLoader's pool threads call."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and not 0 <= idx.min() <= idx.max() < len(self):
            raise IndexError(f"gather: index outside the set of {len(self)} images")
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or tuple(out.shape) != (idx.size, *self.image_shape):
            raise ValueError(f"gather: out is a numpy uint8 array {(idx.size, *self.image_shape)}, got "
                             f"{getattr(out, 'dtype', type(out))} {getattr(out, 'shape', None)}")
        starts, shards = self.starts, self.shards
        ks = np.searchsorted(starts, idx, side="right") - 1
        rows = idx - starts[ks]
        for j in range(idx.size):  # one copy per image, straight from the array or the map into `out`: no intermediate batch
            out[j] = shards[ks[j]][rows[j]]
        return out

    def flipped(self, i):
        if not self.train:
            return False
        if self._flips[0] != (self.seed, self.epoch):  # the whole epoch's bits at once: one vectorised Philox pass
            self._flips = ((self.seed, self.epoch), flip_bits(np.arange(len(self)), self.seed, self.epoch))
        return bool(self._flips[1][i])

    def __getitem__(self, i):
        i = int(i)
        k, row = self.locate(i)  # (IndexError outside the set)
        img = np.array(self.shards[k][row])  # HWC (a copy: a read-only map stays untouched)
        if self.flipped(i):
            img = img[:, ::-1]
        codes = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).long()
        return self.table[self._chan, codes], 0


class ResidentImages(_TableImages):
    """A uint8 image set [N][H][W][C] (C in {1, 3}; a numpy array or an np.load(mmap_mode="r") map) with the reference's transforms as
    a table.  Item i is (CHW float tensor, 0): the host form of what DeviceBatchLoader assembles on the device, bit for bit, for the
    same (index, epoch) -- flipped only when `train`."""

    def __init__(self, u8, normalize, train, seed=0):
        if not _is_u8_images(u8):
            raise ValueError(f"ResidentImages: a non-empty uint8 array [N][H][W][C] with C in (1, 3), got "
                             f"{getattr(u8, 'dtype', type(u8))} {getattr(u8, 'shape', None)}")
        self.u8 = u8
        self._setup(normalize, train, seed)

    # one shard: the array itself (read from self.u8 at every use, so the set is whatever self.u8 is)
    @property
    def shards(self):
        return (self.u8,)

    @property
    def starts(self):
        return np.array([0, self.u8.shape[0]], dtype=np.int64)

    def locate(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return 0, i

    def __len__(self):
        return self.u8.shape[0]


class ShardedImages(_TableImages):
    """A uint8 image set split over `shards`, arrays (or np.load(mmap_mode="r") maps) [n_k][H][W][C] of one image shape: ResidentImages'
    item contract and attributes over their concatenation, which is never made.  The set for StreamedBatchLoader, for a set too large
    for the device (imagenet) or for host memory (the maps are read through the page cache)."""

    def __init__(self, shards, normalize, train, seed=0):
        shards = list(shards)
        if not shards:
            raise ValueError("ShardedImages: no shards")
        for k, s in enumerate(shards):
            if not _is_u8_images(s) or s.shape[1:] != shards[0].shape[1:]:
                raise ValueError(f"ShardedImages: shard {k} is not a non-empty uint8 array [n][H][W][C] with C in (1, 3) of shard 0's image "
                                 f"shape {getattr(shards[0], 'shape', (None,))[1:]}: got {getattr(s, 'dtype', type(s))} "
                                 f"{getattr(s, 'shape', None)}")
        self.shards = shards
        self.starts = np.concatenate([[0], np.cumsum([s.shape[0] for s in shards])]).astype(np.int64)
        self._setup(normalize, train, seed)

    def __len__(self):
        return int(self.starts[-1])


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
    # _upload(): make the set resident (called once, on first use); refuses a set that does not fit (refuse_if_too_big).  The streamed
    #            loader, whose set stays on the host, allocates its ring of host slots and its device staging buffer here instead
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
                              "keep it on the host with --data_loader host, or stream it with --data_loader stream")
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


class StreamedBatchLoader(ResidentLoader):
    """ResidentLoader's index rule over a ResidentImages or ShardedImages that STAYS IN HOST MEMORY: yields
    what DeviceBatchLoader yields, bit for bit, but the set is never uploaded.  Batch k of the epoch is gathered by a pool thread
    (ds.gather, numpy only) into slot k % depth of a ring of page-locked host buffers; next(), in the main thread and on the current
    stream, waits for it, copies the slot into the ONE device staging buffer, records an event and launches ops.batch_u8_staged with
    the batch's dataset indices.  A slot is handed to a worker again only after its copy event has been synchronised.  A pool thread
    makes no HIP and no torch-device call, which is what keeps a hipGraph capture in the main thread legal while the pool runs.

    num_workers sizes the pool (1 .. 8 threads); `timeout` (seconds) bounds the wait for one batch.  `streamed` counts the batches
    handed out."""

    noun = "images"
    depth = 3

    def __init__(self, ds, batch_size, device, shuffle, rank=0, world_size=1, seed=0, num_workers=1, timeout=600.0):
        if not isinstance(ds, (ResidentImages, ShardedImages)):
            raise TypeError(f"StreamedBatchLoader needs a ResidentImages or a ShardedImages, got {type(ds).__name__}")
        super().__init__(ds, batch_size, device, shuffle, rank, world_size, seed)
        self.workers, self.timeout, self.streamed = max(1, min(int(num_workers), 8)), float(timeout), 0
        self._slots = self._slots_np = self._stage = self._lut = self._zeros = self._host_rows = None
        self._active = None  # weak reference to the generator of the epoch under way

    def _upload(self):  # (nothing of the set goes up: the ring, the staging buffer, the table)
        shape = (self.batch_size, *self.dataset.image_shape)
        self._slots = torch.empty((self.depth, *shape), dtype=torch.uint8, pin_memory=True)
        self._slots_np = self._slots.numpy()
        self._stage = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._lut = self.dataset.table.to(self.device)
        self._zeros = torch.zeros(self.batch_size, dtype=torch.long, device=self.device)

    def _checked(self, idx):
        if idx and not 0 <= min(idx) <= max(idx) < len(self.dataset):
            raise RuntimeError("StreamedBatchLoader: index list outside the set")
        rows = torch.tensor(idx, dtype=torch.int32)
        self._host_rows = rows.numpy()  # the same list, for the gathers (replaced with the device list, once per epoch)
        return rows

    def _convert(self, stage, ids):
        ds = self.dataset
        out = ops.batch_u8_staged(stage, ids, self._lut, flip=ds.train, seed=ds.seed, epoch=self.epoch)
        return out.permute(0, 3, 1, 2), self._zeros[:ids.numel()]

    def _batch(self, rows):
        """The batch of ANY device row list, outside an epoch's iteration (visual.first_items): gathered here, in the caller's
        thread, through a pageable buffer of its own, so the ring of an epoch under way is not touched."""
        host = np.empty((rows.numel(), *self.dataset.image_shape), dtype=np.uint8)
        self.dataset.gather(rows.cpu().numpy(), host)
        return self._convert(torch.from_numpy(host).to(self.device), rows.contiguous())

    def __iter__(self):
        prev = self._active() if self._active is not None else None
        if prev is not None:
            prev.close()  # an epoch abandoned half-way gives up its pool and the ring before the next one starts
        gen = self._epoch_batches()
        self._active = weakref.ref(gen)
        return gen

    def _epoch_batches(self):
        from concurrent.futures import ThreadPoolExecutor
        from concurrent.futures import TimeoutError as FutureTimeout

        idx = self._device_indices()
        host, bs, depth = self._host_rows, self.batch_size, self.depth
        starts = range(0, host.shape[0], bs)
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="movae-stream")
        futures, copied, wait = {}, [None] * depth, True

        def submit(k):
            rows = host[starts[k]:starts[k] + bs]
            futures[k] = pool.submit(self.dataset.gather, rows, self._slots_np[k % depth][:rows.shape[0]])

        try:
            for k in range(min(depth, len(starts))):
                submit(k)
            for k, s in enumerate(starts):
                if k >= 1 and k - 1 + depth < len(starts):  # the slot of batch k - 1 is free once its copy has left the host
                    copied[(k - 1) % depth].synchronize()
                    submit(k - 1 + depth)
                try:
                    futures.pop(k).result(self.timeout)  # (a worker's exception is raised here)
                except FutureTimeout as e:
                    wait = False  # the worker may never come back: do not wait for it below
                    raise RuntimeError(f"StreamedBatchLoader: batch {k} of epoch {self.epoch} was not gathered within "
                                       f"{self.timeout:g} s ({self.workers} workers)") from e
                ids = idx[s:s + bs]
                stage = self._stage[:ids.numel()]  # (the ragged last batch: the first rows of slot and stage)
                stage.copy_(self._slots[k % depth][:ids.numel()], non_blocking=True)
                copied[k % depth] = torch.cuda.Event()
                copied[k % depth].record()
                batch = self._convert(stage, ids)
                self.streamed += 1
                yield batch
        finally:  # the epoch's end, an abandoned epoch (the generator is closed or collected), an exception in the consumer
            pool.shutdown(wait=wait, cancel_futures=True)


# ---- ragged sets: RandomResizedCrop -----------------------------------------------------------------------
#: RandomResizedCrop(size, scale=(0.7, 1.0), ratio=(3/4, 4/3)) of the reference's oxford-flower-102 pipeline (utils/utils.py:367-397)
RRC_SCALE, RRC_RATIO, RRC_TRIES = (0.7, 1.0), (3.0 / 4.0, 4.0 / 3.0), 10
#: a crop side may be at most RRC_MAX_SCALE times the output side: the filter scale is then at most 8 and a sample has at most 33 taps,
#: which is what movae_batch_rrc_u8 sizes its LDS for
RRC_MAX_SCALE = 8


def rrc_boxes(dims, seed, epoch):
    """int32 [N][4] = (top, left, bh, bw): the epoch's crop of every image of dims [N][2] = (h, w), torchvision's
    RandomResizedCrop.get_params restated on Philox draws.  Try t = 0 .. 9 of index i reads the four words of counter
    (i + ((t + 1) << 32), epoch) under key seed (stream t + 1 in the counter's second word; stream 0 is the flip's), as
    u = (word + 0.5) / 2^32 in float64: area = h w (0.7 + 0.3 u0), ratio = exp(log 3/4 + u1 (log 4/3 - log 3/4)),
    bw = rint(sqrt(area ratio)), bh = rint(sqrt(area / ratio)) (half to even, Python's round); the first try that fits the image is
    taken, with top = (word2 (h - bh + 1)) >> 32 and left = (word3 (w - bw + 1)) >> 32.  Without one, the central crop at the nearest
    allowed ratio.  A function of (seed, epoch, index, h, w) alone."""
    dims = np.asarray(dims, dtype=np.int64).reshape(-1, 2)
    n = dims.shape[0]
    h, w = dims[:, 0], dims[:, 1]
    idx = np.arange(n, dtype=np.uint64)
    done = np.zeros(n, dtype=bool)
    out = np.zeros((n, 4), dtype=np.int64)
    log_lo, log_hi = math.log(RRC_RATIO[0]), math.log(RRC_RATIO[1])
    for t in range(RRC_TRIES):
        w0, w1, w2, w3 = philox_words(idx + (np.uint64(t + 1) << np.uint64(32)), epoch, seed)
        u0, u1 = (w0.astype(np.float64) + 0.5) / 2.0 ** 32, (w1.astype(np.float64) + 0.5) / 2.0 ** 32
        area = (h * w).astype(np.float64) * (RRC_SCALE[0] + (RRC_SCALE[1] - RRC_SCALE[0]) * u0)
        ratio = np.exp(log_lo + u1 * (log_hi - log_lo))
        bw, bh = np.rint(np.sqrt(area * ratio)).astype(np.int64), np.rint(np.sqrt(area / ratio)).astype(np.int64)
        ok = ~done & (0 < bw) & (bw <= w) & (0 < bh) & (bh <= h)
        # (word * span) >> 32 with span < 2^31: exact in uint64
        top = ((w2 * np.maximum(h - bh + 1, 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        left = ((w3 * np.maximum(w - bw + 1, 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        out[ok] = np.stack([top, left, bh, bw], 1)[ok]
        done |= ok
    if not done.all():
        in_ratio = w.astype(np.float64) / h.astype(np.float64)
        bw = np.where(in_ratio > RRC_RATIO[1], np.rint(h * RRC_RATIO[1]).astype(np.int64), w)
        bh = np.where(in_ratio < RRC_RATIO[0], np.rint(w / RRC_RATIO[0]).astype(np.int64), h)
        central = np.stack([(h - bh) // 2, (w - bw) // 2, bh, bw], 1)
        out[~done] = central[~done]
    return out.astype(np.int32)


def _cubic(x):
    """Keys' cubic, a = -0.5 (PIL's BICUBIC), in the operation order of PIL's C."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resample_table(in_size, out_size):
    """PIL's 8-bit coefficient table of one axis -> (k int32 [out][kmax], zero past the last tap; xmin int [out]; taps int [out]).
    float64 throughout, the weights summed in tap order, then k = int(w / sum * 2^22 +- 0.5)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    kmax = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # the cast truncates toward zero, like C's
    count = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(kmax)[None, :]
    live = taps < count[:, None]
    wt = np.where(live, _cubic(((taps + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size)
    for t in range(kmax):  # in tap order: numpy's own sum is pairwise
        ww = ww + wt[:, t]
    wt = np.where((ww != 0.0)[:, None], wt / np.where(ww != 0.0, ww, 1.0)[:, None], wt)
    k = np.where(wt < 0, -0.5 + wt * (1 << 22), 0.5 + wt * (1 << 22)).astype(np.int64)  # truncation toward zero
    return np.where(live, k, 0).astype(np.int32), xmin, count


def _resample_axis1(img, out_size):
    """uint8 [R][in][C] -> uint8 [R][out][C] along axis 1: clamp((2^21 + sum pixel * k) >> 22, 0, 255) in int32; unchanged where
    in == out (PIL skips that pass)."""
    if img.shape[1] == out_size:
        return img
    k, xmin, count = resample_table(img.shape[1], out_size)
    acc = np.full((img.shape[0], out_size, img.shape[2]), 1 << 21, dtype=np.int32)
    last = img.shape[1] - 1
    for t in range(int(count.max())):  # (a tap past an output's window has weight 0: its clamped read adds nothing)
        acc += img[:, np.minimum(xmin + t, last), :].astype(np.int32) * k[None, :, t, None]
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize_u8(crop_hwc, size):
    """uint8 [h][w][C] -> uint8 [size][size][C]: PIL's Image.resize((size, size), BICUBIC) of an 8-bit image, bit for bit.  The
    horizontal pass first, rounded to uint8, then the vertical pass over it.  The host path's transform and the yardstick of
    movae_batch_rrc_u8."""
    crop = np.asarray(crop_hwc)
    if crop.dtype != np.uint8 or crop.ndim != 3 or 0 in crop.shape:
        raise ValueError(f"resize_u8: a non-empty uint8 [h][w][C] image, got {crop.dtype} {crop.shape}")
    t = _resample_axis1(crop, size)
    return np.ascontiguousarray(_resample_axis1(t.transpose(1, 0, 2), size).transpose(1, 0, 2))


def rrc_kmax(max_side, size):
    """The tap bound movae_batch_rrc_u8 takes for a set whose largest image side is max_side: 2 ceil(2 max(1, max_side / size)) + 1."""
    return 2 * int(math.ceil(2.0 * max(1.0, max_side / size))) + 1


class RaggedImages(torch.utils.data.Dataset):
    """RGB images of their own sizes, back to back in HWC order in one flat uint8 `blob` (an array or a map), `index` int64 [N][3] =
    (byte offset, h, w), with the reference's RandomResizedCrop(size, BICUBIC) -> RandomHorizontalFlip -> ToTensor -> Normalize
    pipeline.  Item i is (CHW float32 [3][size][size], 0): the host form of what RaggedBatchLoader assembles on the device, bit for
    bit, for the same (seed, epoch, index).  An evaluation set (train=False) resizes the whole image and never flips."""

    channels = 3

    def __init__(self, blob, index, size, normalize, train, seed=0):
        index = np.asarray(index)
        if index.ndim != 2 or index.shape[1] != 3 or index.shape[0] == 0 or index.dtype.kind not in "iu":
            raise ValueError(f"RaggedImages: the index is a non-empty integer array [N][3] of (byte offset, h, w), got "
                             f"{index.dtype} {index.shape}")
        if not isinstance(blob, np.ndarray) or blob.dtype != np.uint8 or blob.ndim != 1:
            raise ValueError(f"RaggedImages: the blob is a flat uint8 array, got {getattr(blob, 'dtype', type(blob))} "
                             f"{getattr(blob, 'shape', None)}")
        index = index.astype(np.int64)
        off, h, w = index[:, 0], index[:, 1], index[:, 2]
        bad = np.flatnonzero((h < 1) | (w < 1))
        if bad.size:
            raise ValueError(f"RaggedImages: index row {bad[0]} has h, w = {h[bad[0]]}, {w[bad[0]]}; both must be at least 1")
        size = int(size)
        over = np.flatnonzero(np.maximum(h, w) > RRC_MAX_SCALE * size)
        if over.size:
            r = over[0]
            raise ValueError(f"RaggedImages: index row {r} is an image of {h[r]} x {w[r]}; a side may be at most {RRC_MAX_SCALE} x the "
                             f"output side {size} = {RRC_MAX_SCALE * size} (the resample kernel holds at most 33 taps per sample)")
        end = off + h * w * self.channels
        bad = np.flatnonzero((off < 0) | (end > blob.shape[0]))
        if bad.size:
            raise ValueError(f"RaggedImages: index row {bad[0]} spans bytes {off[bad[0]]} .. {end[bad[0]]}, outside the blob's "
                             f"{blob.shape[0]}")
        order = np.argsort(off, kind="stable")
        clash = np.flatnonzero(end[order][:-1] > off[order][1:])
        if clash.size:
            raise ValueError(f"RaggedImages: index rows {order[clash[0]]} and {order[clash[0] + 1]} overlap in the blob")
        self.blob, self.offsets, self.dims = blob, np.ascontiguousarray(off), np.ascontiguousarray(index[:, 1:3]).astype(np.int32)
        self.size, self.normalize, self.train, self.seed, self.epoch = size, bool(normalize), bool(train), int(seed), 0
        self.kmax = rrc_kmax(int(self.dims.max()), size)
        self.table = value_table(self.channels, normalize)
        self._chan = torch.arange(self.channels).reshape(-1, 1, 1)
        self._drawn = (None, None, None)  # ((seed, epoch), boxes, flips)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.dims.shape[0]

    def boxes(self, epoch=None):
        """int32 [N][4]: the crops of `epoch` (default: the current one); the whole image for an evaluation set."""
        epoch = self.epoch if epoch is None else int(epoch)
        if not self.train:
            return np.concatenate([np.zeros_like(self.dims), self.dims], 1)
        return rrc_boxes(self.dims, self.seed, epoch)

    def _draws(self):
        if self._drawn[0] != (self.seed, self.epoch):  # the whole epoch's boxes and bits at once: vectorised Philox passes
            flips = flip_bits(np.arange(len(self)), self.seed, self.epoch) if self.train else np.zeros(len(self), dtype=bool)
            self._drawn = ((self.seed, self.epoch), self.boxes(), flips)
        return self._drawn[1], self._drawn[2]

    def image(self, i):
        """uint8 [h][w][3] of row i (a view of the blob)."""
        h, w = self.dims[i]
        o = int(self.offsets[i])
        return self.blob[o:o + int(h) * int(w) * self.channels].reshape(int(h), int(w), self.channels)

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        boxes, flips = self._draws()
        top, left, bh, bw = (int(v) for v in boxes[i])
        img = resize_u8(np.array(self.image(i)[top:top + bh, left:left + bw]), self.size)
        if flips[i]:
            img = img[:, ::-1]  # after the crop and the resize: the OUTPUT columns
        codes = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).long()
        return self.table[self._chan, codes], 0


class RaggedBatchLoader(ResidentLoader):
    """ResidentLoader over the (images, labels) batches of a RaggedImages: the blob, its offsets and dims and the table are uploaded on
    first use, the epoch's boxes with the epoch's index list, and every batch is ONE movae_batch_rrc_u8 launch into a fresh NHWC
    buffer, handed out as its logical-NCHW view.  Labels are zeros, like item[1]."""

    noun = "images"

    def __init__(self, ds, batch_size, device, shuffle, rank=0, world_size=1, seed=0):
        if not isinstance(ds, RaggedImages):
            raise TypeError(f"RaggedBatchLoader needs a RaggedImages, got {type(ds).__name__}")
        super().__init__(ds, batch_size, device, shuffle, rank, world_size, seed)
        self._store = self._offsets = self._dims = self._boxes = self._lut = self._zeros = None

    def _upload(self):
        ds, blob = self.dataset, self.dataset.blob
        key = (blob.__array_interface__["data"][0], blob.shape, blob.strides, str(self.device))  # (one copy per host blob: _STORES)
        store = _STORES.get(key)
        if store is None:
            refuse_if_too_big(int(blob.nbytes) + len(ds) * 32 + ds.table.numel() * 4, self.device, "the image set needs",
                              "keep it on the host with --data_loader host")
            store = torch.empty(blob.shape, dtype=torch.uint8, device=self.device)
            step = 256 << 20  # staged through <= 256 MB of host memory (the blob may be a map)
            for s in range(0, blob.shape[0], step):
                store[s:s + step].copy_(torch.from_numpy(np.array(blob[s:s + step])))
            _STORES[key] = store
        self._store = store
        self._offsets = torch.from_numpy(ds.offsets).to(self.device)
        self._dims = torch.from_numpy(ds.dims).to(self.device)
        self._lut = ds.table.to(self.device)
        self._zeros = torch.zeros(self.batch_size, dtype=torch.long, device=self.device)

    def _checked(self, idx):
        if idx and not 0 <= min(idx) <= max(idx) < len(self.dataset):
            raise RuntimeError("RaggedBatchLoader: index list outside the set")
        return torch.tensor(idx, dtype=torch.int32)

    def _device_indices(self):
        if self._idx[0] != self.epoch:  # the epoch's crops go up with its index list, checked on the host like it
            ds = self.dataset
            boxes = ds.boxes(self.epoch)
            top, left, bh, bw = boxes.T
            if not ((top >= 0) & (left >= 0) & (bh >= 1) & (bw >= 1) & (top + bh <= ds.dims[:, 0]) & (left + bw <= ds.dims[:, 1])).all():
                raise RuntimeError("RaggedBatchLoader: a crop box outside its image")
            rows = super()._device_indices()
            self._boxes = torch.from_numpy(boxes).to(self.device)
            return rows
        return self._idx[1]

    def _batch(self, rows):
        ds = self.dataset
        out = ops.batch_rrc_u8(self._store, self._offsets, self._dims, self._boxes, rows, ds.size, ds.channels, ds.kmax, self._lut,
                               flip=ds.train, seed=ds.seed, epoch=self.epoch)
        return out.permute(0, 3, 1, 2), self._zeros[:rows.numel()]


# ---- readers -----------------------------------------------------------------------------------------------------------------------
#: name -> image side of the .npy sets: <data_dir>/<name>_train_u8.npy and <name>_test_u8.npy, uint8 [N][S][S][3]; either part may
#: instead be split over shards <name>_<part>_u8_00000.npy, _00001.npy, ... of that form (a ShardedImages, which streams)
NPY_SETS = {"celeba": 64, "celeba-128": 128, "celeba-hq": 256, "afhq": 256, "imagenet": 256}
ALIASES = {"animal-face": "afhq"}
#: sets whose missing train files are a NotImplementedError with this reason (tests/test_data_host.py pins type and the words 252 GB,
#: as _ragged's does for RandomResizedCrop): without its prepared files such a set is still "not available" to an older caller
UNPREPARED = {
    "imagenet": "1.28 M images of 256 x 256 are 252 GB as uint8: they do not fit one device and stream from host memory",
}
#: name -> image side of the ragged sets: <data_dir>/<name>_train_ragged_u8.npy + <name>_train_ragged_index.npy (the images at their
#: own sizes, cropped and resampled per item) and <name>_test_u8.npy, uint8 [N][S][S][3]; written by tools/prepare_images.py --ragged
RAGGED_SETS = {"oxford-flower-102": 256}


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


def _split_files(data_dir, key, part):
    """-> (path of the one-file form, paths of the shards in order) of one split as they lie in data_dir; either may be absent.
    ValueError for both forms at once and for a gap in the shard numbers."""
    whole = os.path.join(data_dir, f"{key}_{part}_u8.npy")
    pattern = re.compile(re.escape(f"{key}_{part}_u8_") + r"(\d{5})\.npy")
    found = sorted(f for f in (os.listdir(data_dir) if os.path.isdir(data_dir) else ()) if pattern.fullmatch(f))
    if found and os.path.isfile(whole):
        raise ValueError(f"{whole} and the shards {found[0]} .. lie side by side: keep one form of the {part} split")
    for k, f in enumerate(found):
        want = f"{key}_{part}_u8_{k:05d}.npy"
        if f != want:
            raise ValueError(f"{os.path.join(data_dir, want)} is missing: shard numbers are consecutive from 00000, but {f} is there")
    return whole, [os.path.join(data_dir, f) for f in found]


def _split(data_dir, key, part, size):
    """One split of an .npy set: its array (the one-file form) or the list of its shards' arrays, all maps."""
    whole, shards = _split_files(data_dir, key, part)
    return [_npy(p, size) for p in shards] if shards else _npy(whole, size)


def _head(split, n):
    """The first n images of a split (an array, or a list of shards: across a shard boundary if need be)."""
    if not isinstance(split, list):
        return split[:n]
    kept = []
    for s in split:
        if n <= 0:
            break
        kept.append(s[:n])
        n -= kept[-1].shape[0]
    return kept


def _images(split, normalize, train):
    return (ShardedImages if isinstance(split, list) else ResidentImages)(split, normalize, train=train)


def _ragged(name, key, data_dir, normalize, max_items):
    size = RAGGED_SETS[key]
    blob_path, index_path = (os.path.join(data_dir, f"{key}_train_ragged_{part}.npy") for part in ("u8", "index"))
    for path in (blob_path, index_path):
        if not os.path.isfile(path):
            # NotImplementedError, not FileNotFoundError: without its prepared files this set is still "not available" to a caller
            # written before the ragged path existed (tests/test_data_host.py pins type and the word RandomResizedCrop)
            raise NotImplementedError(
                f"dataset {name!r}: its RandomResizedCrop pipeline reads {path}, written by tools/prepare_images.py --ragged from the "
                f"images on disk; that file is missing, and nothing is downloaded")
    blob = np.load(blob_path, mmap_mode="r", allow_pickle=False)
    index = np.load(index_path, allow_pickle=False)
    if blob.dtype != np.uint8 or blob.ndim != 1:
        raise ValueError(f"{blob_path}: expected a flat uint8 array, got {blob.dtype} {blob.shape}")
    if index.dtype != np.int64 or index.ndim != 2 or index.shape[1] != 3 or index.shape[0] == 0:
        raise ValueError(f"{index_path}: expected int64 [N][3] of (byte offset, h, w), got {index.dtype} {index.shape}")
    test = _npy(os.path.join(data_dir, f"{key}_test_u8.npy"), size)
    if max_items:
        index, test = index[:max_items], test[:max(1, max_items // 10)]
        # the blob up to the farthest end of a kept image (a view of the map): the device loader then checks the free memory for,
        # and uploads, what the run can read, not the whole file
        blob = blob[:max(0, int((index[:, 0] + 3 * index[:, 1] * index[:, 2]).max()))]
    return RaggedImages(blob, index, size, normalize, train=True), ResidentImages(test, normalize, train=False), size


def get_real_dataset(name, data_dir="./data", normalize=False, max_items=None):
    """-> (train set, test set, image side) for a real dataset name of the reference (case-insensitive), or None for a name this
    module does not know.  A set is a ResidentImages; a ShardedImages where the split lies on disk as shards; the train set a
    RaggedImages for a set whose pipeline is RandomResizedCrop.
    `max_items` keeps the first max_items train and the first max(1, max_items // 10) test images."""
    key = name.lower()
    key = ALIASES.get(key, key)
    if key in UNPREPARED:
        whole, shards = _split_files(data_dir, key, "train")
        if not shards and not os.path.isfile(whole):
            first = os.path.join(data_dir, f"{key}_train_u8_00000.npy")
            raise NotImplementedError(
                f"dataset {name!r}: {UNPREPARED[key]}.  Its train images are read from {first}, _00001.npy, ... (or from {whole}), "
                f"written by tools/prepare_images.py --shard_images from the images on disk; {first} is missing, and nothing is "
                f"downloaded")
    if key in RAGGED_SETS:
        return _ragged(name, key, data_dir, normalize, max_items)
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
        train = _split(data_dir, key, "train", size)
        # AFHQ has one split in the reference (utils/utils.py:420-422): the train images serve as the test set too
        test = train if key == "afhq" else _split(data_dir, key, "test", size)
    else:
        return None
    if max_items:
        train, test = _head(train, max_items), _head(test, max(1, max_items // 10))
    return _images(train, normalize, True), _images(test, normalize, False), size
