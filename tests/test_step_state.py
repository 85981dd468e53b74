"""The host-side state a step carries from one call to the next is owned by what uses it ("Step state"):
the persistent Jacobian arena and the persistent zero gradient hang on the parameters they describe, a LazyDict computes on
every read, and where one autograd call's gradients go is an ops.Destinations that the caller builds, installs and reads.  No GPU:
JacobianBuffer.persistent and ops.Destinations only allocate and look up, on whatever device the parameters are."""
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
    d = jb.destinations([0, 1], engine=False)
    d.sink(1, ps[0], ps[0].shape)
    d.zeros(0, ps[1], ps[1].shape)
    assert jb.written == [jb.buf[1].data_ptr()] and d.zeroed == [jb.buf[0][15:].data_ptr()]
    assert autojac.JacobianBuffer.persistent(ps, 2, CPU) is jb
    assert jb.copied == set() and jb.written == []
    assert jb.destinations([0], engine=True).written == []  # ... and what the arena hands out next starts from the empty record


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
    z = ops.Destinations(True).zeros(0, p, p.shape)
    assert z.shape == p.shape and z.dtype == p.dtype and z.device == p.device and not z.any()
    assert ops.Destinations(True).zeros(0, p, p.shape).data_ptr() == z.data_ptr()  # one tensor for life: no allocation after the first step
    q = _params(0)[2]
    assert ops.Destinations(True).zeros(0, q, q.shape).data_ptr() != z.data_ptr()
    refs = [weakref.ref(p._movae_zero_grad), weakref.ref(p)]
    del p, z
    gc.collect()
    assert [r() for r in refs] == [None, None]


def test_zero_gradient_is_validated_against_its_parameter():
    p = _params(0)[1]
    z = ops.Destinations(True).zeros(0, p, p.shape)
    p.data = torch.zeros(9, dtype=torch.float64)
    z2 = ops.Destinations(True).zeros(0, p, p.shape)
    assert z2.shape == (9,) and z2.dtype == torch.float64 and z2.data_ptr() != z.data_ptr()


# ---- ops.Destinations -----------------------------------------------------------------------------------------------------------
def _slices(ps, extra=0):
    """One flat zero slice per parameter (of numel + extra elements), and the {param data_ptr: slice} row made of them."""
    sl = [torch.zeros(p.numel() + extra) for p in ps]
    return sl, {p.data_ptr(): t for p, t in zip(ps, sl)}


def _fresh(t, *others):
    """`t` shares memory with none of `others`."""
    return all(t.untyped_storage().data_ptr() != o.untyped_storage().data_ptr() for o in others)


@pytest.mark.parametrize("engine", [True, False])
def test_sink_is_consumed_once(engine):
    ps = _params(0)
    sl, row = _slices(ps)
    d = ops.Destinations(engine, [row])
    p = ps[2]
    a = d.sink(0, p, (2, 2, 2, 3))
    assert a.data_ptr() == sl[2].data_ptr() and a.shape == (2, 2, 2, 3) and d.written == [sl[2].data_ptr()]
    a.fill_(1.0)
    assert bool((sl[2] == 1.0).all())  # a view: the kernel's writes land in the registered slice
    b = d.sink(0, p, (2, 2, 2, 3))
    assert _fresh(b, *sl) and b.shape == (2, 2, 2, 3) and b.dtype == p.dtype and d.written == [sl[2].data_ptr()]
    assert d.zeroed == [] and d.taken == set()


def test_sink_of_the_wrong_size_is_ignored_and_not_recorded():
    ps = _params(0)
    sl, row = _slices(ps, extra=1)
    d = ops.Destinations(False, [dict(row), dict(row)])
    for g in (0, 1):
        assert _fresh(d.sink(g, ps[0], ps[0].shape), *sl) and _fresh(d.zeros(g, ps[1], ps[1].shape), *sl)
    got, all_sunk = d.sinks(2, ps[2], ps[2].shape)
    assert all(_fresh(t, *sl) for t in got) and not all_sunk
    assert d.written == [] and d.zeroed == []


def test_sinks_says_whether_every_group_had_one():
    ps = _params(0)
    (s0, r0), (s1, r1) = _slices(ps), _slices(ps)
    del r1[ps[1].data_ptr()]
    d = ops.Destinations(False, [r0, r1])
    got, all_sunk = d.sinks(2, ps[0], ps[0].shape)
    assert all_sunk and [t.data_ptr() for t in got] == [s0[0].data_ptr(), s1[0].data_ptr()] == d.written
    got, all_sunk = d.sinks(2, ps[1], ps[1].shape)
    assert not all_sunk and got[0].data_ptr() == s0[1].data_ptr() and _fresh(got[1], *s0, *s1)
    got, all_sunk = d.sinks(2, ps[0], ps[0].shape)  # consumed above
    assert not all_sunk and all(_fresh(t, *s0, *s1) for t in got) and len(d.written) == 3


@pytest.mark.parametrize("engine", [True, False])
def test_zeros_hands_a_registered_slice_out_untouched(engine):
    ps = _params(0)
    sl, row = _slices(ps)
    d = ops.Destinations(engine, [row])
    z = d.zeros(0, ps[1], ps[1].shape)
    assert z.data_ptr() == sl[1].data_ptr() and not z.any() and d.zeroed == [sl[1].data_ptr()] and d.written == []


def test_zeros_without_a_sink():
    p = _params(0)[0]
    w = ops.Destinations(False, [{}])
    a, b = w.zeros(0, p, p.shape), w.zeros(0, p, p.shape)
    assert a.data_ptr() != b.data_ptr() and a.shape == p.shape and not a.any() and not b.any()
    assert not hasattr(p, "_movae_zero_grad")  # the walker's form keeps nothing
    e = ops.Destinations(True, [{}])
    z = e.zeros(0, p, p.shape)
    assert z.data_ptr() == p._movae_zero_grad.data_ptr() == e.zeros(0, p, p.shape).data_ptr() and not z.any()
    assert w.zeroed == e.zeroed == [] and w.written == e.written == []


def _grads(ps):
    w = ps[2]  # [2, 3, 2, 2]
    gw = torch.zeros(w.shape).contiguous(memory_format=torch.channels_last)
    gb = torch.zeros(ps[1].shape)
    return w, ps[1], gw, gb


def test_accum_targets_takes_both_or_neither():
    w, b, gw, gb = _grads(_params(0))
    d = ops.Destinations(True, accum={w.data_ptr(): gw})
    assert d.accum_targets(w, b, True) == (None, None) and d.taken == set() and list(d.accum) == [w.data_ptr()]
    d = ops.Destinations(True, accum={w.data_ptr(): gw, b.data_ptr(): gb})
    v, got_b = d.accum_targets(w, b, True)
    assert v.data_ptr() == gw.data_ptr() and v.shape == (2, 2, 2, 3) and v.is_contiguous() and got_b is gb
    assert d.taken == {w.data_ptr(), b.data_ptr()} and d.accum == {}
    assert d.accum_targets(w, b, True) == (None, None)  # consumed
    d = ops.Destinations(True, accum={w.data_ptr(): gw, b.data_ptr(): gb})
    v, got_b = d.accum_targets(w, b, False)  # the bias gradient is not wanted: the weight's alone
    assert v.data_ptr() == gw.data_ptr() and got_b is None and d.taken == {w.data_ptr()} and list(d.accum) == [b.data_ptr()]


def test_accum_targets_checks_memory_order_and_shape():
    w, b, gw, gb = _grads(_params(0))
    d = ops.Destinations(True, accum={w.data_ptr(): torch.zeros(w.shape), b.data_ptr(): gb})  # NCHW-contiguous: not the kernels' order
    assert d.accum_targets(w, b, True) == (None, None)
    d = ops.Destinations(True, accum={w.data_ptr(): gw.permute(1, 0, 2, 3).contiguous(), b.data_ptr(): gb})  # another shape
    assert d.accum_targets(w, b, True) == (None, None)
    assert d.taken == set() and len(d.accum) == 2


def test_accum_targets_is_the_engines_alone():
    w, b, gw, gb = _grads(_params(0))
    d = ops.Destinations(False, [{}], accum={w.data_ptr(): gw, b.data_ptr(): gb})
    assert d.accum_targets(w, b, True) == (None, None) and d.taken == set() and len(d.accum) == 2


def test_cotangent():
    like = torch.zeros(2, 3, 4, 5)  # what the op computes on: NHWC, contiguous
    same = torch.zeros(2, 3, 4, 5)
    feat = like.permute(0, 3, 1, 2)  # the feature: a logical-NCHW view of that memory
    perm = torch.empty_strided(feat.shape, feat.stride())  # its slice, allocated with the feature's strides
    d = ops.Destinations(True, cot={1: same, 2: perm, 3: torch.zeros(2, 3, 4, 5, dtype=torch.float64), 4: torch.zeros(2, 3, 4, 6)})
    assert d.cotangent(1, like) is same
    v = d.cotangent(2, like)
    assert v.data_ptr() == perm.data_ptr() and v.shape == like.shape and v.stride() == like.stride()
    v.copy_(torch.arange(120.0).view(2, 3, 4, 5))
    assert torch.equal(perm, torch.arange(120.0).view(2, 3, 4, 5).permute(0, 3, 1, 2))  # the same memory, seen both ways
    for key in (3, 4, 5):  # wrong dtype, wrong numel, not registered
        t = d.cotangent(key, like)
        assert _fresh(t, same, perm) and t.shape == like.shape and t.dtype == like.dtype
    assert d.cot == {}
    assert _fresh(d.cotangent(1, like), same)  # consumed on first use
    assert d.written == [] and d.zeroed == [] and d.taken == set()


def test_scopes_nest_and_unwind():
    e, e2, w = ops.Destinations(True), ops.Destinations(True), ops.Destinations(False)
    none_e, none_w = ops.installed(True), ops.installed(False)
    assert none_e is not e and none_e.engine is True and none_w.engine is False
    with e:
        assert ops.installed(True) is e
        with e2:
            assert ops.installed(True) is e2
            with w:
                assert ops.installed(False) is w and ops.installed(True) is none_e
            assert ops.installed(True) is e2
        assert ops.installed(True) is e and ops.installed(False) is none_w
    with pytest.raises(KeyError):
        with w:
            with e:
                raise KeyError("inside")
    assert ops.installed(True) is none_e and ops.installed(False) is none_w


def test_each_kind_sees_only_its_own_instance():
    ps = _params(0)
    p = ps[0]
    sl, row = _slices(ps)
    w = ops.Destinations(False, [row, dict(row)], accum={p.data_ptr(): torch.zeros(p.shape)}, cot={7: torch.zeros(3)})
    with w:  # the walker calls Function.backward per group on a node that has no backward_batched: no sink, not row 0's
        e = ops.installed(True)
        assert _fresh(e.sink(0, p, p.shape), *sl) and _fresh(e.cotangent(7, torch.zeros(3)), w.cot[7])
        assert e.zeros(0, p, p.shape).data_ptr() == p._movae_zero_grad.data_ptr()
        assert (e.written, e.zeroed, e.taken) == ([], [], set())
    assert (w.written, w.zeroed, w.taken) == ([], [], set()) and len(w.rows[0]) == 3 and len(w.cot) == 1
    e = ops.Destinations(True, [row])
    with e:
        wd = ops.installed(False)
        assert all(_fresh(t, *sl) for g in range(3) for t in (wd.sink(g, p, p.shape), wd.zeros(g, p, p.shape)))
        assert (wd.written, wd.zeroed) == ([], [])
    assert (e.written, e.zeroed) == ([], []) and len(row) == 3


def test_nothing_installed_records_nothing_anywhere():
    p = _params(0)[0]
    for engine in (True, False):
        d = ops.installed(engine)
        d.sink(0, p, p.shape), d.sinks(2, p, p.shape), d.zeros(1, p, p.shape), d.accum_targets(p, None, False), d.cotangent(1, p.data)
        assert (d.written, d.zeroed, d.taken, d.accum, d.cot) == ([], [], set(), {}, {}) and not d.rows


def _held(*modules):
    """Number of entries of every container reachable from the modules' globals through containers and the modules' own objects."""
    seen, total, stack = {}, 0, [vars(m) for m in modules]  # (seen keeps what it visited alive: an id is not reused meanwhile)
    names = {m.__name__ for m in modules}
    while stack:
        o = stack.pop()
        if id(o) in seen:
            continue
        seen[id(o)] = o
        if isinstance(o, dict):
            total += len(o)
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set, frozenset)):
            total += len(o)
            stack.extend(o)
        elif isinstance(o, type) and o.__module__ in names:  # a class of theirs: its attributes
            stack.append(dict(vars(o)))
        elif type(o).__module__ in names:  # an object of theirs: its attributes, slots included
            stack.append(getattr(o, "__dict__", {}))
            stack.extend(getattr(o, s) for c in type(o).__mro__ for s in getattr(c, "__slots__", ()) if hasattr(o, s))
    return total


def test_a_non_persistent_arena_leaves_nothing_behind(monkeypatch):
    monkeypatch.setattr(autojac, "PERSISTENT_J", False)
    ps = _params(0)

    def step():
        jb = autojac.JacobianBuffer.persistent(ps, 2, CPU)
        with jb.destinations([0, 1], engine=False):
            for g in (0, 1):
                ops.installed(False).sink(g, ps[0], ps[0].shape)
                ops.installed(False).zeros(g, ps[1], ps[1].shape)
        with jb.destinations([1], engine=True):
            ops.installed(True).sink(0, ps[2], ps[2].shape)
        assert len(jb.written) == 3
        jb.settle()

    step()
    before = _held(ops, autojac)
    for _ in range(300):
        step()
    assert _held(ops, autojac) == before
    assert ops.installed(True).written == [] and ops.installed(False).written == []


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
