"""The shared halves of the two captured steps and the two resident loaders: data.ResidentLoader on a stub without a device,
capture.recording without a launch, and on the GPU capture.snapshot / restore on a small PixelCNN and capture.capturing around two
launches."""
import pytest
import torch

N = 37


# ---- data.ResidentLoader, without a GPU ----------------------------------------------------------------------------------------------
def _stub(n=N, batch_size=8, **kw):
    import movae_amd  # noqa: F401
    from movae_amd.data import ResidentLoader

    class Rows:
        def __len__(self):
            return n  # (nothing is allocated: the base class asks for the length only)

    class Stub(ResidentLoader):
        noun = "things"

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.uploads = self.asked = 0

        def indices(self, epoch=None):
            self.asked += epoch is None
            return super().indices(epoch)

        def _upload(self):
            self.uploads += 1

        def _checked(self, idx):
            return torch.tensor(idx, dtype=torch.int32)

        def _batch(self, rows):
            return rows

    return Stub(Rows(), batch_size, "cpu", **kw)


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "in_order"])
def test_resident_loader_slices_the_epoch_list(shuffle):
    from movae_amd.data import shard_indices

    ld = _stub(shuffle=shuffle, seed=3)
    assert len(ld) == 5
    for epoch in (1, 2):
        ld.set_epoch(epoch)
        batches = list(ld)
        assert [b.numel() for b in batches] == [8, 8, 8, 8, 5] and all(b.dtype == torch.int32 for b in batches)
        assert torch.cat(batches).tolist() == shard_indices(N, shuffle, 3, epoch) == ld.indices(epoch)
    assert ld.uploads == 1, "the set is uploaded on first use, once"


def test_resident_loader_takes_its_rank_shard():
    from movae_amd.data import shard_indices

    ld = _stub(shuffle=True, seed=3, rank=1, world_size=2)
    assert len(ld) == 3  # ceil(37 / 2) = 19 rows per rank, in batches of 8
    ld.set_epoch(1)
    batches = list(ld)
    assert [b.numel() for b in batches] == [8, 8, 3]
    assert torch.cat(batches).tolist() == shard_indices(N, True, 3, 1, rank=1, world_size=2)
    assert torch.cat(batches).tolist() != shard_indices(N, True, 3, 1, rank=0, world_size=2)


def test_resident_loader_builds_the_index_list_once_per_epoch():
    ld = _stub(shuffle=True)
    first, again = list(ld), list(ld)
    assert ld.asked == 1 and torch.equal(torch.cat(first), torch.cat(again))
    ld.set_epoch(1)
    later = list(ld)
    assert ld.asked == 2 and not torch.equal(torch.cat(later), torch.cat(first))
    list(ld)
    assert ld.asked == 2


def test_resident_loader_refuses_bad_sizes():
    with pytest.raises(ValueError, match="batch_size must be positive"):
        _stub(batch_size=0)
    with pytest.raises(ValueError, match=f"{2 ** 31} things: row numbers are int32"):
        _stub(n=2 ** 31)
    assert len(_stub(n=2 ** 31 - 1, batch_size=2 ** 30)) == 2


# ---- capture.recording, without a GPU ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """_lib.call with the library stubbed out: the trace hook runs, nothing is launched."""
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    class Lib:
        def __getattr__(self, name):
            return lambda *args: 0

    monkeypatch.setattr(L, "load", lambda: Lib())
    monkeypatch.setattr(L, "TRACE", None)
    return L


def test_recording_traces_calls_and_always_resets(no_library):
    L = no_library
    from movae_amd import capture

    calls = []
    with capture.recording(calls):
        assert L.TRACE is not None
        L.call("movae_add", 1, 2, 3)
    assert calls == [("movae_add", (1, 2, 3))] and L.TRACE is None
    L.call("movae_add", 4)
    assert len(calls) == 1, "nothing is recorded outside the block"
    with pytest.raises(KeyError):
        with capture.recording(calls):
            L.call("movae_mul", 5)
            raise KeyError("the body failed")
    assert L.TRACE is None and [c[0] for c in calls] == ["movae_add", "movae_mul"]


def test_recording_none_leaves_the_trace_alone(no_library):
    L = no_library
    from movae_amd import capture

    seen = []
    outer = lambda name, cargs: seen.append(name)  # noqa: E731
    L.TRACE = outer
    with capture.recording(None):
        assert L.TRACE is outer
        L.call("movae_add", 1)
    assert L.TRACE is outer and seen == ["movae_add"]


# ---- capture.snapshot / restore ------------------------------------------------------------------------------------------------------
def _twin(device):
    from movae_amd.models.pixelcnn_prior import PixelCNN
    from movae_amd.optim import FusedAdam

    torch.manual_seed(3)
    net = PixelCNN(16, 8, hidden_channels=16, num_layers=2).to(device).train()
    return net, FusedAdam(net.parameters(), lr=3e-3, weight_decay=0.0, device_step=True)


def _state(net, opt):
    """name -> tensor of everything the step changes: parameters, buffers, optimizer state tensors."""
    out = {f"param {n}": p for n, p in net.named_parameters()}
    out.update({f"buffer {n}": b for n, b in net.named_buffers()})
    names = {id(p): n for n, p in net.named_parameters()}
    for p, st in opt.state.items():
        out.update({f"state {names[id(p)]}.{k}": v for k, v in st.items() if torch.is_tensor(v)})
    return out


@pytest.mark.gpu
def test_restore_rewinds_a_trained_twin_in_place(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import capture
    from movae_amd.prior import _one_step

    z = torch.randint(0, 16, (4, 8, 8), generator=torch.Generator().manual_seed(11)).to(gpu_device)
    net, opt = _twin(gpu_device)
    _one_step(net, opt, z)
    snap = capture.snapshot(net, opt, gpu_device)
    want = {k: v.detach().clone() for k, v in _state(net, opt).items()}
    assert any(k.startswith("state ") for k in want) and float(opt.state[next(net.parameters())]["step"]) == 1.0
    rng = torch.cuda.get_rng_state(gpu_device), torch.get_rng_state()
    for _ in range(3):
        _one_step(net, opt, z)
    torch.rand(3, device=gpu_device), torch.rand(3)  # both streams move on
    assert not torch.equal(torch.cuda.get_rng_state(gpu_device), rng[0]) and not torch.equal(torch.get_rng_state(), rng[1])
    before = _state(net, opt)
    ptrs = {k: v.data_ptr() for k, v in before.items()}
    assert any(not torch.equal(before[k], want[k]) for k in want if k.startswith("param "))
    capture.restore(snap, net, opt, gpu_device)
    after = _state(net, opt)
    assert after.keys() == want.keys()
    for k, v in after.items():
        assert v.data_ptr() == ptrs[k], f"{k} moved"
        assert torch.equal(v, want[k]), f"{k} differs from its value at the snapshot"
    assert torch.equal(torch.cuda.get_rng_state(gpu_device), rng[0]) and torch.equal(torch.get_rng_state(), rng[1])


@pytest.mark.gpu
def test_restore_to_the_initial_state_zeroes_what_the_warm_up_created(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import capture
    from movae_amd.prior import _one_step

    z = torch.randint(0, 16, (4, 8, 8), generator=torch.Generator().manual_seed(11)).to(gpu_device)
    net, opt = _twin(gpu_device)
    ref, ref_opt = _twin(gpu_device)
    snap = capture.snapshot(net, opt, gpu_device)
    assert len(opt.state) == 0
    for _ in range(3):
        _one_step(net, opt, z)
    ptrs = {k: v.data_ptr() for k, v in _state(net, opt).items()}
    capture.restore(snap, net, opt, gpu_device)
    after = _state(net, opt)
    born = [k for k in after if k.startswith("state ")]
    assert born and all(not after[k].any() for k in born), "state tensors born during the warm-up are zero"
    assert all(after[k].data_ptr() == ptrs[k] for k in after)
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.equal(p, q), f"{n} is not back at its initial value"
    loss, ref_loss = _one_step(net, opt, z), _one_step(ref, ref_opt, z)
    assert torch.equal(loss, ref_loss)
    got, want = _state(net, opt), _state(ref, ref_opt)
    assert got.keys() == want.keys()
    for k in got:
        assert torch.equal(got[k], want[k]), f"{k}: the step after the restore is not the untouched twin's first step"


# ---- capture.capturing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capturing_forgets_the_layout_conversion_and_replays_exactly(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import capture, ops

    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(2, 3, 8, 8, generator=g).to(gpu_device), torch.randn(2, 8, 8, 3, generator=g).to(gpu_device)
    ops.forget_nhwc()
    eager = ops.add(ops.to_nhwc(x), y).clone()
    L.workspace(gpu_device)
    torch.cuda.synchronize()
    calls, graph = [], torch.cuda.CUDAGraph()
    with capture.recording(calls):
        assert ops.to_nhwc(x) is ops.to_nhwc(x) and calls == [], "the eager conversion is remembered"
        with capture.capturing(graph):
            out = ops.add(ops.to_nhwc(x), y)
        assert [c[0] for c in calls] == ["movae_nchw_to_nhwc", "movae_add"], "the graph holds a conversion of its own"
        assert ops._LAST_NHWC[0] is None, "no graph-pool tensor is remembered past the block"
        ops.to_nhwc(x)
        assert [c[0] for c in calls][2:] == ["movae_nchw_to_nhwc"], "after the block the conversion is launched again"
    assert L.TRACE is None
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(torch.randn(2, 3, 8, 8, generator=g))  # the replay reads the static input
    graph.replay()
    assert torch.equal(out, ops.add(x.permute(0, 2, 3, 1).contiguous(), y))
