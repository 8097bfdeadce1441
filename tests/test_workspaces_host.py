"""CPU-only tests of who owns the library's device scratch (_ops.Workspaces): each captured graph owns a set that nothing else hands out,
replaces or frees, while eager launches share one set per stream handle.  PyTorch hands its side streams out from a pool of 32 per
device, so stream handles repeat: 40 owners on handles i % 32 stand in for 40 captures.  The sets live on the CPU here; no compute call
touches a GPU."""
import threading
import weakref

import pytest
import torch

from q_learning_with_hjb_amd import _ops

CPU = torch.device("cpu")
N_OWNERS, N_HANDLES = 40, 32
NEED = 3000                              # bytes of parameter-gradient scratch each "capture" asks for
BIG = (64 << 20) + (64 << 10)           # more than 4 NEED + 64 MiB: an eager set gives it back once NEED is asked for again


@pytest.fixture
def handle(monkeypatch):
    """The stream lookup of _ops, pointed at a settable handle; a private table of eager sets."""
    h = [0]
    monkeypatch.setattr(_ops, "_stream", lambda: h[0])
    monkeypatch.setattr(_ops, "_eager", {})
    return h


def _buffers():
    """What one step requests, the way hjb_residual, the rollout kernel and value_loss_adam do."""
    got = _ops._workspaces(CPU)
    return got, [got.reduce(), _ops._rollout_workspace(CPU), got.grad(NEED)]


def test_owned_sets_survive_aliased_stream_handles_and_release(handle):
    owners, bufs = [], []
    for i in range(N_OWNERS):
        handle[0] = i % N_HANDLES
        ws = _ops.Workspaces(CPU)
        with _ops.using_workspaces(ws):
            got, b = _buffers()
        assert got is ws
        owners.append(ws)
        bufs.append(b)
    eager = {}
    for h in range(N_HANDLES):
        handle[0] = h
        eager[h], eager_bufs = _buffers()
        assert not eager[h].owned and all(eager[h] is not o for o in owners)
        bufs.append(eager_bufs)
    every = [t for b in bufs for t in b]
    assert len({t.data_ptr() for t in every}) == len(every), "a buffer is shared between two sets"

    # half the owners die; then every eager set, and those of one aliased handle once more, are released
    survivors = [(ws, b, [t.data_ptr() for t in b]) for ws, b in zip(owners[1::2], bufs[1:N_OWNERS:2])]
    dead = [weakref.ref(t) for b in bufs[0:N_OWNERS:2] for t in b]
    del owners, bufs, every
    assert all(r() is None for r in dead), "a dead owner's buffers are still referenced"
    _ops.release_workspaces()
    handle[0] = 7
    fresh, fresh_bufs = _buffers()
    assert fresh is not eager[7]
    _ops.release_workspaces(7)
    assert _ops._workspaces(CPU) is not fresh
    for ws, b, ptrs in survivors:
        now = [ws.reduce(), ws.rollout(), ws.grad(NEED)]
        assert all(x is y for x, y in zip(now, b)) and [t.data_ptr() for t in now] == ptrs
        assert not now[0].any() and not now[1].any(), "tickets / flags must stay zero (include/hjbx.h)"
        with _ops.using_workspaces(ws):
            assert _ops._workspaces(CPU) is ws
    live = [t for _, b, _ in survivors for t in b] + fresh_bufs
    assert len({t.data_ptr() for t in live}) == len(live)


def test_eager_sets_are_shared_per_handle_and_give_scratch_back(handle):
    handle[0] = 3
    a, b = _ops._workspaces(CPU), _ops._workspaces(CPU)
    assert a is b and a.reduce() is b.reduce() and a.rollout() is b.rollout()
    handle[0] = 4
    assert _ops._workspaces(CPU) is not a
    big = a.grad(BIG)
    assert a.grad(BIG // 4) is big             # within 4x + 64 MiB of the request: kept
    ref = weakref.ref(big)
    del big
    small = a.grad(NEED)
    assert NEED <= small.numel() < BIG and ref() is None, "the eager set did not give its large scratch back"
    assert a.grad(2 * NEED).numel() >= 2 * NEED


def test_owned_set_never_drops_a_buffer_it_handed_out(handle):
    ws = _ops.Workspaces(CPU)
    first = ws.grad(BIG)
    ptr, ref = first.data_ptr(), weakref.ref(first)
    del first
    assert ws.grad(NEED) is ref()               # no give-back for an owner
    larger = ws.grad(BIG + 4096)
    assert larger is not ref() and larger.numel() >= BIG + 4096
    assert ref() is not None and ref().data_ptr() == ptr, "an owned set freed a buffer a graph may replay into"


def test_activation_is_per_thread_and_restored(handle):
    ws = _ops.Workspaces(CPU)
    seen = []
    with _ops.using_workspaces(ws):
        t = threading.Thread(target=lambda: seen.append(_ops._workspaces(CPU)))
        t.start()
        t.join()
        inner = _ops.Workspaces(CPU)
        with _ops.using_workspaces(inner):
            assert _ops._workspaces(CPU) is inner
        assert _ops._workspaces(CPU) is ws
    assert seen[0] is not ws and not seen[0].owned
    assert _ops._workspaces(CPU) is seen[0]
