"""Device side of the streamed path: movae_batch_u8_staged bit for bit against movae_batch_u8 and the restated transforms, its refusals,
data.StreamedBatchLoader against data.DeviceBatchLoader over the same images (ring reuse, ragged last batch, ranks, workers, slow
producer and consumer, which thread does what, abandoned epochs, a failing and a stuck gather), and train.cli on a tiny ImageNet in
tmp_path against the same images as one resident file."""
import gc
import threading
import time
import traceback

import numpy as np
import pytest
import torch

import data_yardstick as Y

pytestmark = pytest.mark.gpu

SEED = Y.SEED
IDX = [10, 0, 3, 3, 7]  # out of order and repeated; at (SEED, 0) and at (SEED, 1) some of these rows flip and some do not
SIZES = (37, 41, 5)


@pytest.fixture(scope="module")
def M(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import data, ops, train

    return data, ops, train


def _nchw(out_nhwc):
    return out_nhwc.permute(0, 3, 1, 2).cpu()


def _pool_threads():
    return [t for t in threading.enumerate() if t.name.startswith("movae-stream")]


def _no_pool_thread_left():
    for t in _pool_threads():
        t.join(10)
    return not _pool_threads()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("h,w,c", [(8, 8, 3), (6, 10, 3), (5, 4, 1), (6, 12, 1)])
def test_kernel_is_exact(M, gpu_device, h, w, c, normalize):
    data, ops, _ = M
    u8 = Y.images(40, h, w, c, seed=h * 100 + w * 10 + c)
    store = torch.from_numpy(u8).to(gpu_device)
    lut = data.value_table(c, normalize).to(gpu_device)
    seen = set()
    cases = [(IDX, SEED, e) for e in Y.EPOCHS] + [([4], SEED, e) for e in Y.EPOCHS]
    cases.append((np.random.default_rng(1).permutation(40)[:37].tolist(), SEED, 1))  # b = 37: more than one block at 8 x 8 x 3
    cases.append((list(range(11)), (3 << 32) | 9, (1 << 32) | 2))  # a 64-bit seed and epoch reach the counter and the key whole
    for idx, seed, epoch in cases:
        ids = torch.tensor(idx, dtype=torch.int32, device=gpu_device)
        stage = store[ids.long()].contiguous()
        odd = torch.empty(stage.numel() + 1, dtype=torch.uint8, device=gpu_device)[1:].view(stage.shape)  # 1 byte into its buffer
        odd.copy_(stage)
        assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
        for flip in (False, True):
            want = Y.expected_batch(u8, idx, normalize, flip, seed, epoch)
            resident = ops.batch_u8(store, ids, lut, flip=flip, seed=seed, epoch=epoch)
            for st in (stage, odd):  # aligned: the 4-pixel path where w % 4 == 0; the view: always the per-element path
                out = ops.batch_u8_staged(st, ids, lut, flip=flip, seed=seed, epoch=epoch)
                assert out.dtype == torch.float32 and tuple(out.shape) == (len(idx), h, w, c) and out.is_contiguous()
                assert torch.equal(out, resident), (idx, flip, epoch)
                assert torch.equal(_nchw(out), want), (idx, flip, epoch)
            if flip and seed == SEED:
                seen.update(Y.flip_rule(idx, seed, epoch).tolist())
    assert seen == {False, True}, "both flipped and unflipped rows must have occurred"


def test_flip_key_is_the_dataset_index_not_the_row(M, gpu_device):
    """ids past 2^16 with a stage of 6 rows: the source row is j, the key ids[j]; against a resident store that has those rows."""
    data, ops, _ = M
    idx = [70000, 2, 65536, 65537, 99999, 70000]
    u8 = Y.images(len(idx), 5, 4, 1, seed=12)
    u8[5] = u8[0]  # (the same dataset index twice is the same image twice)
    fl = {e: Y.flip_rule(idx, SEED, e) for e in Y.EPOCHS}
    assert any(0 < f.sum() < len(idx) for f in fl.values())
    assert any(not np.array_equal(f, Y.flip_rule(list(range(len(idx))), SEED, e)) for e, f in fl.items()), "keys that rows would not give"
    store = torch.zeros((100000, 5, 4, 1), dtype=torch.uint8, device=gpu_device)
    ids = torch.tensor(idx, dtype=torch.int32, device=gpu_device)
    stage = torch.from_numpy(u8).to(gpu_device)
    store[ids.long()] = stage
    lut = data.value_table(1, True).to(gpu_device)
    for epoch in Y.EPOCHS:
        out = ops.batch_u8_staged(stage, ids, lut, flip=True, seed=SEED, epoch=epoch)
        want = torch.stack([Y.transform(u8[j], True, bool(fl[epoch][j])) for j in range(len(idx))])
        assert torch.equal(_nchw(out), want)
        assert torch.equal(out, ops.batch_u8(store, ids, lut, flip=True, seed=SEED, epoch=epoch))


def test_bad_arguments_are_refused(M, gpu_device):
    import movae_amd._lib as L

    data, _, _ = M
    lib = L.load()
    stage = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=gpu_device)
    ids = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    lut = data.value_table(3, False).to(gpu_device)
    out = torch.full((2 * 4 * 4 * 3 + 4,), 7.0, device=gpu_device)
    st = L.stream_ptr(gpu_device)
    good = dict(stage=stage.data_ptr(), ids=ids.data_ptr(), b=2, h=4, w=4, c=3, lut=lut.data_ptr(), out=out.data_ptr())

    def rc(**kw):
        a = dict(good, **kw)
        return lib.movae_batch_u8_staged(a["stage"], a["ids"], a["b"], a["h"], a["w"], a["c"], a["lut"], 1, 0, 0, a["out"], st)

    for bad in (dict(stage=None), dict(ids=None), dict(lut=None), dict(out=None), dict(b=0), dict(b=-1), dict(h=0), dict(w=0), dict(w=-4),
                dict(c=2), dict(c=4), dict(c=0), dict(out=out.data_ptr() + 4)):
        assert rc(**bad) == -1, bad
        assert b"movae_batch_u8_staged" in lib.movae_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call launches nothing"
    assert rc() == 0
    torch.cuda.synchronize()
    assert (out[:96] == 0.0).all() and (out[96:] == 7.0).all()


# ---- the loader ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(M):
    """(the images [83][8][12][3], their shards 37 + 41 + 5): one array for every loader test, never written to."""
    whole = Y.images(sum(SIZES), 8, 12, 3, seed=21)
    edges = np.cumsum((0,) + SIZES)
    return whole, [whole[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.fixture(scope="module")
def resident_epochs(M, gpu_device, sets):
    """(shuffle, rank, world, epoch) -> the batches of data.DeviceBatchLoader over the concatenated images, on the host; computed once."""
    data, _, _ = M
    whole, _ = sets
    ds = data.ResidentImages(whole, True, train=True, seed=SEED)
    ref = {}
    for shuffle in (True, False):
        for rank, world in ((0, 1), (0, 2), (1, 2)):
            loader = data.DeviceBatchLoader(ds, 16, gpu_device, shuffle, rank=rank, world_size=world, seed=3)
            for epoch in (0, 1):
                loader.set_epoch(epoch)
                ref[shuffle, rank, world, epoch] = [(x.cpu(), y.cpu()) for x, y in loader]
    return ref


def _same(got, want):
    assert len(got) == len(want)
    for k, ((x, y), (wx, wy)) in enumerate(zip(got, want)):
        assert torch.equal(x.cpu(), wx) and torch.equal(y.cpu(), wy), k


@pytest.mark.parametrize("workers", [1, 4])
def test_loader_equals_the_resident_loader(M, gpu_device, sets, resident_epochs, workers):
    data, _, _ = M
    _, shards = sets
    ds = data.ShardedImages(shards, True, train=True, seed=SEED)
    for shuffle in (True, False):
        for rank, world in ((0, 1), (0, 2), (1, 2)):
            loader = data.StreamedBatchLoader(ds, 16, gpu_device, shuffle, rank=rank, world_size=world, seed=3, num_workers=workers)
            assert loader.workers == workers and len(loader) == (6 if world == 1 else 3)
            for epoch in (0, 1, 0):
                loader.set_epoch(epoch)
                batches = list(loader)
                if world == 1:  # 6 batches over a ring of 3: every slot is used twice, and the last batch is ragged
                    assert [x.size(0) for x, _ in batches] == [16, 16, 16, 16, 16, 3]
                for x, y in batches:
                    assert tuple(x.shape) == (x.size(0), 3, 8, 12) and x.is_cuda and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()
                    assert y.dtype == torch.long and tuple(y.shape) == (x.size(0),) and not y.any() and y.is_cuda
                assert len({x.data_ptr() for x, _ in batches}) == len(batches), "output buffers are not reused"
                _same(batches, resident_epochs[shuffle, rank, world, epoch])
            assert loader.streamed == 3 * len(loader)
    assert _no_pool_thread_left()


def test_streaming_a_resident_set_and_an_evaluation_set(M, gpu_device, sets, resident_epochs):
    """`--data_loader stream` over one array, and a set that never flips."""
    data, _, _ = M
    whole, shards = sets
    loader = data.StreamedBatchLoader(data.ResidentImages(whole, True, train=True, seed=SEED), 16, gpu_device, True, seed=3, num_workers=2)
    loader.set_epoch(1)
    _same(list(loader), resident_epochs[True, 0, 1, 1])
    plain = data.StreamedBatchLoader(data.ShardedImages(shards, True, train=False, seed=SEED), 16, gpu_device, shuffle=False)
    plain.set_epoch(1)
    got = torch.cat([x for x, _ in plain]).cpu()
    assert torch.equal(got, Y.expected_batch(whole, list(range(83)), True, False, SEED, 1))
    # the rows visual.first_items asks for, outside an epoch
    from movae_amd import visual

    first = visual.first_items(loader, 5, gpu_device)
    assert torch.equal(first.cpu(), Y.expected_batch(whole, list(range(5)), True, True, SEED, 1))


def test_slow_producer_and_slow_consumer(M, gpu_device, sets, resident_epochs):
    data, _, _ = M
    _, shards = sets
    ds = data.ShardedImages(shards, True, train=True, seed=SEED)
    real = ds.gather

    def slow_gather(indices, out):
        time.sleep(0.05)
        return real(indices, out)

    ds.gather = slow_gather
    for workers in (1, 4):
        loader = data.StreamedBatchLoader(ds, 16, gpu_device, True, seed=3, num_workers=workers)
        _same(list(loader), resident_epochs[True, 0, 1, 0])
    del ds.gather
    loader = data.StreamedBatchLoader(ds, 16, gpu_device, True, seed=3, num_workers=4)
    loader.set_epoch(1)
    got = []
    for batch in loader:  # the producers run ahead: the ring must hold them back, not overwrite a slot that has not been copied
        time.sleep(0.02)
        got.append(batch)
    _same(got, resident_epochs[True, 0, 1, 1])


def test_who_runs_where(M, gpu_device, sets, monkeypatch):
    data, ops, _ = M
    _, shards = sets
    ds = data.ShardedImages(shards, True, train=True, seed=SEED)
    gathers, launches = [], []
    real_gather, real_launch = ds.gather, ops.batch_u8_staged
    ds.gather = lambda i, o: (gathers.append(threading.current_thread()), real_gather(i, o))[1]
    monkeypatch.setattr(ops, "batch_u8_staged", lambda *a, **k: (launches.append(threading.current_thread()), real_launch(*a, **k))[1])
    for workers in (1, 4):
        for _ in data.StreamedBatchLoader(ds, 16, gpu_device, True, num_workers=workers):
            pass
    main = threading.main_thread()
    assert len(gathers) == len(launches) == 12
    assert all(t is not main and t.name.startswith("movae-stream") for t in gathers), "gather runs on pool threads only"
    assert all(t is main for t in launches), "the launch is the main thread's"
    assert _no_pool_thread_left()


def test_abandoned_epochs_leave_no_thread(M, gpu_device, sets, resident_epochs):
    data, _, _ = M
    _, shards = sets
    ds = data.ShardedImages(shards, True, train=True, seed=SEED)
    loader = data.StreamedBatchLoader(ds, 16, gpu_device, True, seed=3, num_workers=4)
    it = iter(loader)
    two = [next(it), next(it)]
    assert _pool_threads(), "the pool lives while the epoch is under way"
    again = list(loader)  # a second iter() starts the epoch again; the abandoned one gives up its pool
    _same(two, resident_epochs[True, 0, 1, 0][:2])
    _same(again, resident_epochs[True, 0, 1, 0])
    with pytest.raises(StopIteration):
        next(it)
    assert not _pool_threads()
    for batch in loader:  # leaving the loop, and an exception in the step
        break
    assert not _pool_threads()
    with pytest.raises(ZeroDivisionError):
        for batch in loader:
            1 / 0
    gc.collect()
    assert not _pool_threads()
    it = iter(loader)
    next(it)
    assert _pool_threads()
    del it, loader
    gc.collect()
    assert not _pool_threads(), "deleting the loader leaves no thread behind"


def test_a_failing_and_a_stuck_gather(M, gpu_device, sets):
    data, _, _ = M
    _, shards = sets
    ds = data.ShardedImages(shards, True, train=True, seed=SEED)
    real, calls = ds.gather, []

    def failing_gather(indices, out):
        calls.append(1)
        if len(calls) == 2:
            raise KeyError("the second batch cannot be read")
        return real(indices, out)

    ds.gather = failing_gather
    it = iter(data.StreamedBatchLoader(ds, 16, gpu_device, True, seed=3, num_workers=1))
    next(it)
    with pytest.raises(KeyError, match="the second batch cannot be read") as e:
        next(it)
    assert "failing_gather" in "".join(traceback.format_exception(type(e.value), e.value, e.value.__traceback__)), "the worker's own frames"
    with pytest.raises(StopIteration):
        next(it)
    assert not _pool_threads()

    release = threading.Event()

    def stuck_gather(indices, out):
        release.wait(30)
        return real(indices, out)

    ds.gather = stuck_gather
    loader = data.StreamedBatchLoader(ds, 16, gpu_device, True, seed=3, num_workers=2, timeout=0.2)
    try:
        with pytest.raises(RuntimeError, match="batch 0 ") as e:
            next(iter(loader))
        assert "0.2 s" in str(e.value)
    finally:
        release.set()
    assert _no_pool_thread_left()
    del ds.gather
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_imagenet(tmp_path_factory):
    """12 train images in shards of 7 + 5 and 2 test images, side 256; and the same images as ONE train file in a second folder."""
    root = tmp_path_factory.mktemp("imagenet")
    tr, te = Y.images(12, 256, 256, 3, seed=40), Y.images(2, 256, 256, 3, seed=41)
    (root / "sharded").mkdir()
    (root / "whole").mkdir()
    np.save(root / "sharded" / "imagenet_train_u8_00000.npy", tr[:7])
    np.save(root / "sharded" / "imagenet_train_u8_00001.npy", tr[7:])
    np.save(root / "whole" / "imagenet_train_u8.npy", tr)
    for d in ("sharded", "whole"):
        np.save(root / d / "imagenet_test_u8.npy", te)
    return root


@pytest.mark.parametrize("graph", ["off", "auto"])
def test_cli_trains_on_imagenet_shards(M, gpu_device, tiny_imagenet, tmp_path, capsys, monkeypatch, graph):
    data, ops, train = M
    staged, captures = [], []
    real = ops.batch_u8_staged
    monkeypatch.setattr(ops, "batch_u8_staged", lambda *a, **k: (staged.append(1), real(*a, **k))[1])
    real_step = train.GraphedTrainStep

    class Watched(real_step):
        def __init__(self, *a, **k):
            captures.append(len(_pool_threads()))
            super().__init__(*a, **k)

    monkeypatch.setattr(train, "GraphedTrainStep", Watched)

    def run(folder, loader):
        argv = ["--dataset", "imagenet", "--data_dir", str(tiny_imagenet / folder), "--arch", "vq_vae", "--hidden_dims", "8", "16",
                "--embedding_dim", "8", "--num_embeddings", "16", "--agg", "upgrad", "--batch_size", "4", "--epochs", "2", "--skip_pixelcnn",
                "--seed", "3", "--graph", graph, "--data_loader", loader, "--num_workers", "2", "--max_fid_samples", "0",
                "--save_path", str(tmp_path / f"{folder}_{loader}"), "--device", "cuda:0"]
        hist = train.cli(argv)
        params = {k: v.detach().clone() for k, v in train.LAST_RUN["net"].state_dict().items()}
        return hist, params, capsys.readouterr().out

    hist_s, params_s, out_s = run("sharded", "auto")
    assert len(staged) == 2 * 3, "three streamed train batches per epoch (the one-file test set is resident)"
    assert "[movae] streamed 6 batches of the training set from host memory (2 gather threads)" in out_s
    assert "hipGraph capture" not in out_s
    if graph == "auto":
        assert len(captures) == 1 and captures[0] >= 1, f"one capture, made while the gather pool is alive: {captures}"
    else:
        assert not captures
    assert _no_pool_thread_left()
    del captures[:]
    hist_r, params_r, out_r = run("whole", "device")
    assert len(staged) == 6 and "streamed" not in out_r and captures == ([0] if graph == "auto" else [])
    assert len(hist_s) == len(hist_r) == 2 and all(np.isfinite(list(h.values())).all() for h in hist_s)
    assert hist_s == hist_r, "the epoch histories are bit-equal"
    assert params_s.keys() == params_r.keys() and params_s
    for k in params_s:
        assert torch.equal(params_s[k], params_r[k]), k
