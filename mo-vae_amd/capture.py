"""What surrounds the capture of an optimisation step into a hipGraph -- the one copy of the protocol that train.GraphedTrainStep and
prior.GraphedPriorStep follow (DESIGN.md sections 3.4 and 3.21)."""
#     snap = snapshot(module, optimizer, device)      # the warm-up steps are real optimisation steps ...
#     warm_up(step_fn, n, device)                     # workspace outside the capture, n steps on a side stream, synchronise
#     optimizer.zero_grad(set_to_none=True)
#     with recording(calls), capturing(graph):        # forget_nhwc / torch.cuda.graph / forget_nhwc; L.TRACE reset on every exit
#         ... the step ...
#     restore(snap, module, optimizer, device)        # ... rewound, so the first replay is step 1 of the run
import contextlib

import torch

from . import _lib as L
from . import ops


def _state_tensors(module):
    # BetaTC's device-side step counter; the in-kernel noise generator's {seed, draws} (models/_base.py)
    extra = [t for t in (getattr(module, "_iter_dev", None), getattr(module, "_noise_state_t", None)) if isinstance(t, torch.Tensor)]
    return list(module.parameters()) + list(module.buffers()) + extra


def snapshot(module, optimizer, device):
    """Everything a step changes: parameters, buffers, the device-side counters, optimizer state tensors and both RNG streams."""
    return {"tensors": [t.detach().clone() for t in _state_tensors(module)],
            "opt": {id(p): {k: v.detach().clone() for k, v in st.items() if torch.is_tensor(v)} for p, st in optimizer.state.items()},
            "cuda_rng": torch.cuda.get_rng_state(device), "cpu_rng": torch.get_rng_state()}


@torch.no_grad()
def restore(snap, module, optimizer, device):
    """Rewind to `snap` in place; a state tensor born after the snapshot (by the warm-up) is zeroed."""
    torch.cuda.synchronize(device)
    for t, s in zip(_state_tensors(module), snap["tensors"]):
        t.copy_(s)
    for p, st in optimizer.state.items():  # the state tensors keep their addresses (the captured graph points at them)
        old = snap["opt"].get(id(p), {})
        for k, v in st.items():
            if torch.is_tensor(v):
                if k in old:
                    v.copy_(old[k])
                else:
                    v.zero_()
    torch.cuda.set_rng_state(snap["cuda_rng"], device)
    torch.set_rng_state(snap["cpu_rng"])


def warm_up(step_fn, n, device):
    """`n` calls of step_fn() on a side stream, as a capture needs them: they create the optimizer state and load the code objects."""
    L.workspace(device)  # allocate the scratch arena outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(n):
            step_fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


@contextlib.contextmanager
def capturing(graph, **graph_kwargs):
    """torch.cuda.graph(graph, **graph_kwargs) between two ops.forget_nhwc(): a conversion produced eagerly must not stand in for a
    launch the graph has to contain, and graph-pool memory must not leak into eager code -- after a failed capture either."""
    ops.forget_nhwc()
    try:
        with torch.cuda.graph(graph, **graph_kwargs):
            yield graph
    finally:
        ops.forget_nhwc()


@contextlib.contextmanager
def recording(calls):
    """While active, every C-ABI launch appends (name, args) to the list `calls`; None records nothing and leaves L.TRACE alone."""
    if calls is None:
        yield
        return
    L.TRACE = lambda name, cargs: calls.append((name, cargs))
    try:
        yield
    finally:
        L.TRACE = None
