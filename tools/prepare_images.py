"""Image folder -> the uint8 .npy sets that train.get_dataset reads (<name>_train_u8.npy / <name>_test_u8.npy, [N][S][S][3]).

    python tools/prepare_images.py --src img_align_celeba --out data --name celeba --size 64 --center_crop 148 --split 0.9

Per image: RGB, an optional centre crop, then Image.resize((S, S), Image.BICUBIC) -- what the reference's CenterCrop + Resize(BICUBIC,
antialias=True) do to a PIL image (utils/utils.py:262-274).  Files are taken in sorted order.  --split F sends the first F of them to
the train file and the rest to the test file; --split_list FILE names the TRAIN files, one per line (the others are the test set).

    python tools/prepare_images.py --src jpg --out data --name oxford-flower-102 --size 256 --ragged --split_list trnval.txt

--ragged is for a set whose training pipeline is RandomResizedCrop (oxford-flower-102: train + validation images as the train part).
The TRAIN images are not resampled: <name>_train_ragged_u8.npy holds them back to back as RGB bytes in HWC order, one flat uint8
array, and <name>_train_ragged_index.npy int64 [N][3] = (byte offset, h, w); the crop and the resample happen per item at training
time.  The test part is written as always (the reference's Resize((S, S)) of the whole image).

    python tools/prepare_images.py --src ILSVRC --out data --name imagenet --size 256 --recursive --shard_images 50000 --split_list train.txt

--shard_images N writes each part as shards <name>_<part>_u8_00000.npy, _00001.npy, ... of at most N images instead of one file: the
form of a set that stays in host memory and streams (imagenet; data.ShardedImages).  --recursive takes the images of sub-folders too
(ImageNet's train/<class>/ and val/ folders under one --src), sorted by their path relative to --src; a --split_list then names
relative paths (here: every file under train/).  The Hugging Face arrow / parquet cache is not read.
Pure host code; nothing is downloaded."""
import argparse
import os

import numpy as np
from PIL import Image

EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".webp")


def load_image(path, size, center_crop=None):
    """-> uint8 [size][size][3]."""
    img = Image.open(path).convert("RGB")
    if center_crop:
        w, h = img.size
        # torchvision's CenterCrop: the window's corner is round((side - crop) / 2) (transforms/functional.py: center_crop)
        left, top = int(round((w - center_crop) / 2.0)), int(round((h - center_crop) / 2.0))
        img = img.crop((left, top, left + center_crop, top + center_crop))
    return np.asarray(img.resize((size, size), Image.BICUBIC), dtype=np.uint8)


def list_images(src, recursive=False):
    """The image files of `src`, sorted; with `recursive` those of its sub-folders too (ImageNet's class folders), as paths relative
    to `src`, sorted by that path."""
    if not recursive:
        return sorted(f for f in os.listdir(src) if f.lower().endswith(EXTENSIONS))
    return sorted(os.path.relpath(os.path.join(root, f), src) for root, _, files in os.walk(src) for f in files
                  if f.lower().endswith(EXTENSIONS))


def split_names(names, split=None, split_list=None):
    """-> (train names, test names), each in sorted order."""
    if split_list is not None:
        chosen = set(split_list)
        missing = sorted(chosen - set(names))
        if missing:
            raise ValueError(f"{len(missing)} names of the split list are not in the folder, e.g. {missing[:3]}")
        return [n for n in names if n in chosen], [n for n in names if n not in chosen]
    if split is None:
        return list(names), []
    if not 0.0 < split <= 1.0:
        raise ValueError(f"--split is the train fraction in (0, 1], got {split}")
    k = int(len(names) * split)
    return names[:k], names[k:]


def convert(src, out, name, size, center_crop=None, split=None, split_list=None, shard_images=None, recursive=False):
    """Writes <out>/<name>_train_u8.npy and, when the split leaves any, <out>/<name>_test_u8.npy; with `shard_images` N each part as
    shards <name>_<part>_u8_00000.npy, _00001.npy, ... of at most N images, the same images in the same order.  -> the paths written."""
    if shard_images is not None and shard_images < 1:
        raise ValueError(f"--shard_images is the largest number of images in a shard, at least 1 (got {shard_images})")
    names = list_images(src, recursive)
    if not names:
        raise FileNotFoundError(f"no images ({', '.join(EXTENSIONS)}) in {src}")
    os.makedirs(out, exist_ok=True)
    written = []
    for part, chosen in zip(("train", "test"), split_names(names, split, split_list)):
        if not chosen:
            continue
        stem = os.path.join(out, f"{name}_{part}_u8")
        pieces = [(stem + ".npy", chosen)] if shard_images is None else \
            [(f"{stem}_{k:05d}.npy", chosen[s:s + shard_images]) for k, s in enumerate(range(0, len(chosen), shard_images))]
        for path, piece in pieces:
            arr = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=(len(piece), size, size, 3))
            for i, n in enumerate(piece):
                arr[i] = load_image(os.path.join(src, n), size, center_crop)
            arr.flush()
            del arr
            written.append(path)
    return written


def convert_ragged(src, out, name, size, split=None, split_list=None):
    """Writes <out>/<name>_train_ragged_u8.npy and <name>_train_ragged_index.npy (the train images at their own sizes) and, when the
    split leaves any, <out>/<name>_test_u8.npy (the test images resized whole).  -> the paths written."""
    names = list_images(src)
    if not names:
        raise FileNotFoundError(f"no images ({', '.join(EXTENSIONS)}) in {src}")
    os.makedirs(out, exist_ok=True)
    train, test = split_names(names, split, split_list)
    if not train:
        raise ValueError("the split leaves no train images")
    index = np.zeros((len(train), 3), dtype=np.int64)
    for i, n in enumerate(train):  # a first pass over the headers alone: the sizes give the offsets
        with Image.open(os.path.join(src, n)) as img:
            w, h = img.size
        index[i] = (index[i - 1, 0] + 3 * index[i - 1, 1] * index[i - 1, 2] if i else 0, h, w)
    total = int(index[-1, 0] + 3 * index[-1, 1] * index[-1, 2])
    blob_path, index_path = (os.path.join(out, f"{name}_train_ragged_{part}.npy") for part in ("u8", "index"))
    blob = np.lib.format.open_memmap(blob_path, mode="w+", dtype=np.uint8, shape=(total,))
    for (off, h, w), n in zip(index, train):
        px = np.asarray(Image.open(os.path.join(src, n)).convert("RGB"), dtype=np.uint8)
        assert px.shape == (h, w, 3), (n, px.shape, h, w)
        blob[off:off + 3 * h * w] = px.reshape(-1)
    blob.flush()
    del blob
    np.save(index_path, index, allow_pickle=False)
    written = [blob_path, index_path]
    if test:
        path = os.path.join(out, f"{name}_test_u8.npy")
        arr = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=(len(test), size, size, 3))
        for i, n in enumerate(test):
            arr[i] = load_image(os.path.join(src, n), size)
        arr.flush()
        del arr
        written.append(path)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--src", required=True, help="folder of images")
    p.add_argument("--out", required=True, help="the --data_dir of training")
    p.add_argument("--name", required=True, help="celeba | celeba-128 | celeba-hq | afhq | imagenet | oxford-flower-102 (with --ragged)")
    p.add_argument("--size", type=int, required=True, help="S: 64 / 128 / 256")
    p.add_argument("--center_crop", type=int, default=None, help="148 (celeba), 178 (celeba-128)")
    p.add_argument("--split", type=float, default=None, help="fraction of the sorted files that goes to the train file")
    p.add_argument("--split_list", type=str, default=None, help="text file naming the train files, one per line")
    p.add_argument("--ragged", action="store_true", help="keep the train images at their own sizes (a RandomResizedCrop set)")
    p.add_argument("--shard_images", type=int, default=None,
                   help="write each part as shards <name>_<part>_u8_00000.npy, ... of at most this many images (a set that streams "
                        "from host memory: imagenet)")
    p.add_argument("--recursive", action="store_true", help="take the images of sub-folders too (class folders), sorted by relative path")
    a = p.parse_args(argv)
    listed = None
    if a.split_list:
        with open(a.split_list) as f:
            listed = [line.strip() for line in f if line.strip()]
    if a.ragged and a.center_crop:
        p.error("--ragged keeps whole images: it takes no --center_crop")
    if a.ragged and (a.shard_images is not None or a.recursive):
        p.error("--ragged writes one blob from one folder: it takes neither --shard_images nor --recursive")
    paths = convert_ragged(a.src, a.out, a.name, a.size, a.split, listed) if a.ragged else \
        convert(a.src, a.out, a.name, a.size, a.center_crop, a.split, listed, a.shard_images, a.recursive)
    for path in paths:
        print(path)


if __name__ == "__main__":
    main()
