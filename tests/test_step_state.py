"""The host-side state a step carries from one call to the next is owned by what uses it ("Step state"):
the persistent Jacobian arena and the persistent zero gradient hang on the parameters they describe, and a LazyDict computes on
every read.  No GPU: JacobianBuffer.persistent and ops._sink_zeros only allocate, on whatever device the parameters are."""
import gc
import weakref

import pytest
import torch

import movae_amd  # noqa: F401
from movae_amd import autojac, ops
from movae_amd.models._base import LazyDict

CPU = torch.device("cpu")


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*shape, generator=g)) for shape in ((3, 5), (7,), (2, 3, 2, 2))]


def test_arena_is_found_again_however_many_models_are_alive():
    lists = [_params(i) for i in range(6)]
    arenas = [autojac.JacobianBuffer.persistent(ps, 2, CPU) for ps in lists]
    ptrs = [jb.buf.data_ptr() for jb in arenas]
    assert len({id(jb) for jb in arenas}) == 6 and len(set(ptrs)) == 6
    again = autojac.JacobianBuffer.persistent(lists[0], 2, CPU)
    assert again is arenas[0] and again.buf.data_ptr() == ptrs[0]
    for ps, jb in zip(lists, arenas):  # ... and every other one
        assert autojac.JacobianBuffer.persistent(ps, 2, CPU) is jb
    assert again.buf.shape == (2, 48) and again.m == 46 and not again.buf.any()


def test_arena_matches_parameter_objects_not_their_sizes():
    ps = _params(0)
    jb = autojac.JacobianBuffer.persistent(ps, 2, CPU)
    twin = [ps[0]] + _params(1)[1:]  # same first parameter, same sizes, other objects
    other = autojac.JacobianBuffer.persistent(twin, 2, CPU)
    assert other is not jb and other.buf.data_ptr() != jb.buf.data_ptr()
    assert autojac.JacobianBuffer.persistent(ps, 2, CPU) is jb
    assert autojac.JacobianBuffer.persistent(twin, 2, CPU) is other
    assert autojac.JacobianBuffer.persistent(ps[:2], 2, CPU) is not jb  # a prefix is another parameter list


def test_arena_and_parameters_are_released_with_the_model():
    ps = _params(0)
    jb = autojac.JacobianBuffer.persistent(ps, 3, CPU)
    jb.buf[1].fill_(1.0)
    refs = [weakref.ref(jb.buf), weakref.ref(jb), weakref.ref(ps[0]), weakref.ref(ps[2])]
    del jb, ps
    gc.collect()
    assert [r() for r in refs] == [None] * 4


def test_same_parameters_with_another_k_get_another_arena():
    ps = _params(0)
    two = autojac.JacobianBuffer.persistent(ps, 2, CPU)
    three = autojac.JacobianBuffer.persistent(ps, 3, CPU)
    assert two is not three and two.buf.shape[0] == 2 and three.buf.shape[0] == 3
    two.buf.fill_(2.0)
    three.buf.fill_(3.0)
    assert autojac.JacobianBuffer.persistent(ps, 2, CPU) is two and autojac.JacobianBuffer.persistent(ps, 3, CPU) is three
    assert bool((two.buf == 2.0).all()) and bool((three.buf == 3.0).all())


def test_persistent_resets_the_per_call_logs():
    ps = _params(0)
    jb = autojac.JacobianBuffer.persistent(ps, 2, CPU)
    jb.copied.add(1)
    ops.SINK_LOG.append(1)
    ops.SINK_ZERO_LOG.append(2)
    assert autojac.JacobianBuffer.persistent(ps, 2, CPU) is jb
    assert jb.copied == set() and ops.SINK_LOG == [] and ops.SINK_ZERO_LOG == []


def test_persistent_j_off_gives_a_fresh_zero_filled_buffer_per_call(monkeypatch):
    monkeypatch.setattr(autojac, "PERSISTENT_J", False)
    ps = _params(0)
    a = autojac.JacobianBuffer.persistent(ps, 2, CPU)
    a.buf.fill_(1.0)
    b = autojac.JacobianBuffer.persistent(ps, 2, CPU)
    assert b is not a and b.buf.data_ptr() != a.buf.data_ptr() and not b.buf.any() and b.dirty is None
    assert not hasattr(ps[0], "_movae_j_arenas")


def test_zero_gradient_lives_and_dies_with_its_parameter():
    p = _params(0)[2]
    z = ops._sink_zeros(0, p, p.shape)
    assert z.shape == p.shape and z.dtype == p.dtype and z.device == p.device and not z.any()
    assert ops._sink_zeros(0, p, p.shape).data_ptr() == z.data_ptr()  # one tensor for life: no allocation after the first step
    q = _params(0)[2]
    assert ops._sink_zeros(0, q, q.shape).data_ptr() != z.data_ptr()
    refs = [weakref.ref(p._movae_zero_grad), weakref.ref(p)]
    del p, z
    gc.collect()
    assert [r() for r in refs] == [None, None]


def test_zero_gradient_is_validated_against_its_parameter():
    p = _params(0)[1]
    z = ops._sink_zeros(0, p, p.shape)
    p.data = torch.zeros(9, dtype=torch.float64)
    z2 = ops._sink_zeros(0, p, p.shape)
    assert z2.shape == (9,) and z2.dtype == torch.float64 and z2.data_ptr() != z.data_ptr()


# ---- LazyDict -------------------------------------------------------------------------------------------------------------------
def _lazy():
    a, b = torch.tensor(1.0), torch.tensor(2.0)
    return a, b, LazyDict({"plain": a, "sum": lambda: a + b, "n": 3})


def test_lazydict_recomputes_on_every_read():
    a, b, d = _lazy()
    assert float(d["sum"]) == 3.0
    a.fill_(5.0)  # what a graph replay does to the tensors the lambda closes over
    assert float(d["sum"]) == 7.0 and float(d.get("sum")) == 7.0
    b.fill_(-5.0)
    assert float(dict(d)["sum"]) == 0.0


def test_lazydict_never_hands_out_a_function():
    a, b, d = _lazy()
    views = {"dict()": dict(d), "{**d}": {**d}, "copy()": d.copy(), "items()": dict(d.items()), "values()": dict(zip(d.keys(), d.values())),
             "get()": {k: d.get(k) for k in d}, "[]": {k: d[k] for k in d}}
    for how, got in views.items():
        assert list(got) == ["plain", "sum", "n"], how
        assert not any(callable(v) for v in got.values()), how
        assert got["plain"] is a and isinstance(got["sum"], torch.Tensor) and float(got["sum"]) == 3.0 and got["n"] == 3, how
    assert type(d.copy()) is dict
    assert d.get("absent") is None and d.get("absent", 4) == 4
    with pytest.raises(KeyError):
        d["absent"]


def test_lazydict_computes_nothing_until_read():
    calls = []
    d = LazyDict({"sum": lambda: calls.append(1) or torch.tensor(0.0)})
    assert calls == [] and callable(dict.__getitem__(d, "sum"))
    d["sum"], d["sum"]
    assert len(calls) == 2 and callable(dict.__getitem__(d, "sum"))  # the dict still stores the lambda: nothing was written back
