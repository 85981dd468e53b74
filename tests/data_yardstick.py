"""Yardsticks of tests/test_data_host.py and tests/test_data_device.py, restated here and never imported from movae_amd.data: the torch
expressions of the reference's transforms (ToTensor, Normalize(0.5, 0.5), flip(-1)), a numpy Philox4x32-10 for the flip bit, and
writers of tiny datasets in the on-disk formats the readers take."""
import os
import pickle

import numpy as np
import torch

SEED, EPOCHS = 5, (0, 1)  # the (seed, epoch) pairs of the tests: (SEED, 0) and (SEED, 1)


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on numpy: c [n, 4] counter words, k (k0, k1) -> [n, 4] words."""
    c = [c[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k[0]), np.uint64(k[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1)


def flip_rule(indices, seed, epoch):
    """bool per dataset index: bit 31 of word 0 of Philox(counter = (i lo, i hi, epoch lo, epoch hi), key = (seed lo, seed hi))."""
    i = np.asarray(indices, dtype=np.uint64)
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    ctr = np.stack([i & m32, i >> s32, np.full_like(i, epoch & 0xFFFFFFFF), np.full_like(i, epoch >> 32)], 1)
    return (philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[:, 0] >> np.uint64(31)).astype(bool)


def transform(img_hwc, normalize, flip):
    """The reference's per-item pipeline on one uint8 HWC image -> CHW float32: [flip] -> ToTensor -> [Normalize(0.5, 0.5)].
    (The flip of a PIL image mirrors the columns: flip(-1) of the CHW tensor.)"""
    x = torch.from_numpy(np.ascontiguousarray(img_hwc)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)  # ToTensor
    if flip:
        x = x.flip(-1)
    if normalize:
        c = x.shape[0]
        mean, std = torch.tensor([0.5] * c).view(-1, 1, 1), torch.tensor([0.5] * c).view(-1, 1, 1)
        x = x.clone().sub_(mean).div_(std)  # Normalize
    return x


def expected_batch(u8, indices, normalize, flip, seed, epoch):
    """[B, C, H, W] float32 for the dataset indices, flipped where the rule says (and `flip` is on)."""
    fl = flip_rule(indices, seed, epoch) if flip else np.zeros(len(indices), dtype=bool)
    return torch.stack([transform(u8[i], normalize, bool(f)) for i, f in zip(indices, fl)])


def images(n, h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, c), dtype=np.uint8)


def write_cifar10(root, per_file=8, seed=0):
    """<root>/cifar-10-batches-py/data_batch_1..5 and test_batch of `per_file` planar rows each -> (train rows, test rows)."""
    d = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, 256, size=(per_file, 3072), dtype=np.uint8) for _ in range(6)]
    for name, r in zip([f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"], rows):
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({"data": r, "labels": [0] * per_file}, f)
    return np.concatenate(rows[:5]), rows[5]


def write_cifar100(root, n_train=12, n_test=5, seed=1):
    d = os.path.join(root, "cifar-100-python")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    tr, te = rng.integers(0, 256, size=(n_train, 3072), dtype=np.uint8), rng.integers(0, 256, size=(n_test, 3072), dtype=np.uint8)
    for name, r in (("train", tr), ("test", te)):
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({"data": r, "fine_labels": [0] * len(r)}, f)
    return tr, te
