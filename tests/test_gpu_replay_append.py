"""hjbx_replay_append_* / ReplayBuffer.extend_rollout on the device: a rollout log appended to the replay ring trajectory by trajectory
(reference controller/vhjb.py:304-308 on the deque(maxlen) of :62-73).

The comparator is ReplayBuffer._extend_rollout_torch, the torch expression train() and warm_start() used before (transposed copy of the
log, boolean-mask compaction, ReplayBuffer.extend); tests/test_replay_append_host.py holds it against a Python deque.  Records are copied,
never computed, so every comparison here is on raw bits: there is no tolerance."""
import numpy as np
import pytest
import torch

from conftest import make_dynamics, make_vhjb_config
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.controller.vhjb import ReplayBuffer, VHJBController

pytestmark = pytest.mark.gpu

INT = {torch.float32: torch.int32, torch.float64: torch.int64}
SENTINEL = {torch.float32: 0x7FC0DEAD, torch.float64: 0x7FF8DEADBEEF0000}      # NaNs with a payload no computation produces


def _bits(t):
    return t.view(INT[t.dtype])


def _ring(n, capacity, dtype, head, size):
    rb = ReplayBuffer(n, capacity, dtype, "cuda")
    for t in (rb.x, rb.cost, rb.done):
        _bits(t).fill_(SENTINEL[dtype])
    rb.head, rb.size = head, size
    return rb


def _same_ring(a, b):
    return (torch.equal(_bits(a.x), _bits(b.x)) and torch.equal(_bits(a.cost), _bits(b.cost)) and torch.equal(_bits(a.done), _bits(b.done))
            and a.head == b.head and a.size == b.size)


def _log(gen, T, B, n, dtype):
    """random log, random done_step in [0, T] with forced 0s and Ts, NaN in every entry past done_step"""
    done_step = torch.randint(0, T + 1, (B,), generator=gen, device="cuda", dtype=torch.int32)
    if B >= 2:
        done_step[0], done_step[-1] = 0, T
    if B >= 7:
        done_step[3], done_step[B // 2] = T, 0
    traj = torch.randn((T + 1, B, n), generator=gen, device="cuda", dtype=dtype)
    cost = torch.randn((T + 1, B), generator=gen, device="cuda", dtype=dtype)
    past = torch.arange(T + 1, device="cuda")[:, None] > done_step[None, :]
    traj[past] = float("nan")
    cost[past] = float("nan")
    return traj, cost, done_step


@pytest.mark.parametrize("n", [2, 4, 6, 10])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_device_append_is_bit_equal_to_the_torch_expression(dtype, n):
    gen = torch.Generator(device="cuda").manual_seed(100 * n + (dtype == torch.float64))
    regimes = set()
    for B in (1, 7, 64, 1000, 4099):
        for T in (1, 25, 200):
            traj, cost, done_step = _log(gen, T, B, n, dtype)
            K, max_L = int((done_step.long() + 1).sum()), int(done_step.max()) + 1
            capacities = {"K < capacity": K + 5, "K == capacity": K, "K > capacity": max(1, K // 2), "capacity < max L": max(1, max_L // 2)}
            for regime, capacity in capacities.items():
                if regime == "K > capacity" and not K > capacity or regime == "capacity < max L" and not capacity < max_L:
                    continue                                                      # (B = 1, T = 1 with a single record)
                regimes.add(regime)
                starts = {"empty": (0, 0), "half full": (capacity // 2, capacity // 2), "wrapped": (min(capacity - 1, capacity // 3 + 1), capacity)}
                for start, (head, size) in starts.items():
                    dev, ref = _ring(n, capacity, dtype, head, size), _ring(n, capacity, dtype, head, size)
                    k_dev = dev.extend_rollout(traj, cost, done_step)
                    k_ref = ref._extend_rollout_torch(traj, cost, done_step)
                    assert k_dev == k_ref == K, (B, T, regime, start)
                    assert _same_ring(dev, ref), (B, T, regime, start)
                    assert dev.head == (head + min(K, capacity)) % capacity and dev.size == min(capacity, size + min(K, capacity))
    assert regimes == {"K < capacity", "K == capacity", "K > capacity", "capacity < max L"}


@pytest.mark.parametrize("n", [1, 3, 5, 7, 8, 9])
def test_device_append_other_state_dimensions_and_unaligned_views(n):
    """Records whose size is not a multiple of 8 bytes (float32, odd n) move in 4-byte words; so does an even-n log that starts 4 bytes off
    an 8-byte boundary, and a log of 16-byte records 8 bytes off a 16-byte boundary moves in 8-byte words."""
    gen = torch.Generator(device="cuda").manual_seed(n)
    for dtype in (torch.float32, torch.float64):
        traj, cost, done_step = _log(gen, 37, 333, n, dtype)
        K = int((done_step.long() + 1).sum())
        for capacity in (K + 3, K // 3):
            dev, ref = _ring(n, capacity, dtype, capacity // 5, capacity // 5), _ring(n, capacity, dtype, capacity // 5, capacity // 5)
            assert dev.extend_rollout(traj, cost, done_step) == ref._extend_rollout_torch(traj, cost, done_step) == K
            assert _same_ring(dev, ref)
    traj, cost, done_step = _log(gen, 20, 130, 6, torch.float32)
    shifted = torch.empty(traj.numel() + 1, device="cuda")[1:].view(traj.shape).copy_(traj)
    assert shifted.data_ptr() % 8 == 4 and shifted.is_contiguous()
    dev, ref = _ring(6, 500, torch.float32, 17, 17), _ring(6, 500, torch.float32, 17, 17)
    dev.extend_rollout(shifted, cost, done_step)
    ref._extend_rollout_torch(traj, cost, done_step)
    assert _same_ring(dev, ref)
    traj, cost, done_step = _log(gen, 20, 130, 4, torch.float32)
    shifted = torch.empty(traj.numel() + 2, device="cuda")[2:].view(traj.shape).copy_(traj)
    assert shifted.data_ptr() % 16 == 8
    dev, ref = _ring(4, 500, torch.float32, 499, 500), _ring(4, 500, torch.float32, 499, 500)
    dev.extend_rollout(shifted, cost, done_step)
    ref._extend_rollout_torch(traj, cost, done_step)
    assert _same_ring(dev, ref)


def test_header_reports_records_dropped_and_bad_entries():
    gen = torch.Generator(device="cuda").manual_seed(9)
    traj, cost, done_step = _log(gen, 30, 500, 4, torch.float32)
    K = int((done_step.long() + 1).sum())
    rb = _ring(4, 1000, torch.float32, 0, 0)
    assert K > 1000
    assert _ops.replay_append(traj, cost, done_step, rb.x, rb.cost, rb.done, 0).tolist() == [K, K - 1000, 0, 0]
    big = _ring(4, K + 1, torch.float32, 0, 0)
    assert _ops.replay_append(traj, cost, done_step, big.x, big.cost, big.done, 5).tolist() == [K, 0, 0, 0]
    # B == 0: nothing launched, the header zeroed
    header = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    none = torch.empty((31, 0, 4), device="cuda")
    rc = _abi.lib().hjbx_replay_append_f32(traj.data_ptr(), cost.data_ptr(), done_step.data_ptr(), 30, 0, 4, rb.x.data_ptr(), rb.cost.data_ptr(),
                                           rb.done.data_ptr(), 1000, 0, header.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == _abi.OK and header.tolist() == [0, 0, 0, 0]
    before = _ring(4, 1000, torch.float32, 3, 3)
    assert before.extend_rollout(none, none[:, :, 0].contiguous(), done_step[:0]) == 0 and before.head == 3 and before.size == 3
    assert (_bits(before.x) == SENTINEL[torch.float32]).all()
    # shape / dtype / device checks of the wrapper
    with pytest.raises(TypeError):
        _ops.replay_append(traj.double(), cost, done_step, rb.x, rb.cost, rb.done, 0)
    with pytest.raises(ValueError):
        _ops.replay_append(traj.transpose(0, 1), cost, done_step, rb.x, rb.cost, rb.done, 0)
    with pytest.raises(ValueError):
        _ops.replay_append(traj, cost, done_step, rb.x, rb.cost, rb.done, 1000)           # head outside the ring


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("bad", [-1, "T + 1"])
def test_bad_done_step_raises_and_leaves_the_ring_untouched(bad, dtype):
    """Validation, not a provoked fault: the kernels read no log entry and write no slot for an out-of-range done_step."""
    gen = torch.Generator(device="cuda").manual_seed(2)
    T = 12
    traj, cost, done_step = _log(gen, T, 300, 6, dtype)
    done_step[77] = T + 1 if bad == "T + 1" else bad
    done_step[299] = T + 1 if bad == "T + 1" else bad
    rb, ref = _ring(6, 700, dtype, 650, 700), _ring(6, 700, dtype, 650, 700)
    with pytest.raises(ValueError, match="2 done_step entries outside"):
        rb.extend_rollout(traj, cost, done_step)
    assert _same_ring(rb, ref)


@pytest.mark.parametrize("name", ["cartpole", "nearhover"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fused-f32", "stepwise-f64"])
def test_rollout_done_flags_are_the_terminal_tuple(name, dtype):
    """The premise of writing `done` from done_step alone: on valid tuples the rollout's own done array is 1 exactly at t == done_step."""
    T, B = 40, 3000
    d = make_dynamics(name)
    ctl = VHJBController(d, make_vhjb_config(name, maximum_step=T), dtype=dtype)
    assert ctl.fused_value_grad == (dtype == torch.float32)
    rng = np.random.default_rng(11)
    cfg = make_vhjb_config(name)
    box = np.asarray(cfg.obs_max, np.float64).clip(max=3.0)
    x0 = np.asarray(cfg.xf, np.float64) + rng.uniform(-1, 1, (B, d.state_dim)) * box * 1.05      # some start outside the box, some stay to T
    out = ctl.rollout_batch(ctl._dev(x0))
    ds = out["done_step"].long()
    assert 0 <= int(ds.min()) < int(ds.max()) <= T                      # trajectories of several lengths
    steps = torch.arange(T + 1, device="cuda")[:, None]
    valid = steps <= ds[None, :]
    assert torch.equal(out["done"][valid], (steps == ds[None, :]).to(dtype)[valid])
    # and so the device append of this log equals the expression train() used to evaluate on it, out["done"] included
    rb, ref = _ring(d.state_dim, 5000, dtype, 0, 0), _ring(d.state_dim, 5000, dtype, 0, 0)
    vm = valid.t().reshape(-1)
    ref.extend(out["traj"].transpose(0, 1).reshape(-1, d.state_dim)[vm], out["cost"].t().reshape(-1)[vm], out["done"].t().reshape(-1)[vm])
    assert rb.extend_rollout(out["traj"], out["cost"], out["done_step"]) == int(vm.sum())
    assert _same_ring(rb, ref)


def _train_twice(name, dtype, capacity, **ctor):
    kw = dict(epochs=5, num_of_trajectories_per_epoch=12, maximum_step=30, batch_size=64, maximum_buffer_size=capacity,
              regularization_warmup_steps_per_cycle=4, regularization_total_steps_per_cycle=9, regularization_num_of_cycles=2, regularization_peak_value=1e-2)
    runs = []
    for device_append in (True, False):
        d = make_dynamics(name)
        ctl = VHJBController(d, make_vhjb_config(name, **kw), dtype=dtype, device_replay_append=device_append, **ctor)
        assert ctl.device_replay_append == device_append
        runs.append((ctl, ctl.train()))
    return runs


@pytest.mark.parametrize("name,dtype,capacity", [("cartpole", torch.float32, 900), ("nearhover", torch.float32, 100), ("cartpole", torch.float64, 900)],
                         ids=["cartpole-f32", "nearhover-f32", "cartpole-f64"])
def test_train_is_identical_with_and_without_the_device_append(name, dtype, capacity):
    """(the untrained near-hover policy leaves the observation box within a few steps: its ring is smaller, so that it wraps as well)"""
    (a, lists_a), (b, lists_b) = _train_twice(name, dtype, capacity)
    assert a.fused_value_grad == (dtype == torch.float32)
    ra, rb = a.replay_buffer, b.replay_buffer
    assert ra.size == ra.capacity == capacity and sum(lists_a[2]) * 12 > capacity      # more tuples emitted than the ring holds: it did wrap
    assert _same_ring(ra, rb)
    assert a.update_counter == b.update_counter > 0 and a.regularization == b.regularization
    assert len(lists_a) == 6 and all(len(x) == 5 for x in lists_a[:3])
    for la, lb in zip(lists_a, lists_b):
        assert la == lb                                                     # the six returned lists, float for float
    for wa, wb in zip(a.value_function_approximator.weights, b.value_function_approximator.weights):
        assert torch.equal(wa, wb)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_warm_start_is_identical_with_and_without_the_device_append(dtype):
    from q_learning_with_hjb_amd.controller.cartpole_energy_shaping import CartpoleEnergyShapingController
    results = []
    for device_append in (True, False):
        d = make_dynamics("cartpole")
        ctl = VHJBController(d, make_vhjb_config("cartpole", maximum_buffer_size=200, maximum_step=60), dtype=dtype, device_replay_append=device_append)
        es = CartpoleEnergyShapingController(d)
        x0 = np.random.default_rng(4).uniform(-1, 1, (50, 4)) * np.array([1.0, np.pi, 1.0, 1.0])
        results.append((ctl, ctl.warm_start(es, 50, x0=x0)))
    (a, ra), (b, rb) = results
    assert ra["records"] == rb["records"] == int((ra["done_step"].long() + 1).sum()) >= 50
    assert ra["average_trajectory_cost"] == rb["average_trajectory_cost"] and ra["average_trajectory_length"] == rb["average_trajectory_length"]
    assert torch.equal(ra["done_step"], rb["done_step"])
    qa, qb = a.replay_buffer, b.replay_buffer
    print(f"warm start: {ra['records']} records, ring {qa.size} / {qa.capacity}, head {qa.head}")
    assert qa.size == qb.size == 200 and qa.head == qb.head            # full (its unwritten slots would be uninitialised memory)
    assert _same_ring(qa, qb)


# ---- full size ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_log():
    """Storage for the near-hover log at B = 2^20 (n = 10, T = 200: 8.4 GB), allocated once"""
    T, n, B = 200, 10, 1 << 20
    store = dict(traj=torch.empty((T + 1) * B * n, device="cuda"), cost=torch.empty((T + 1) * B, device="cuda"))
    yield store
    store.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("log2_B", [17, 20])
def test_full_size_append_lands_the_last_million_records_in_order(big_log, log2_B):
    T, n, B, capacity = 200, 10, 1 << log2_B, 10 ** 6
    traj = big_log["traj"][:(T + 1) * B * n].view(T + 1, B, n)
    cost = big_log["cost"][:(T + 1) * B].view(T + 1, B)
    env = torch.arange(B, device="cuda")
    steps = torch.arange(T + 1, device="cuda")
    traj[:, :, 0] = env.float()[None, :]                                   # x[t, b, 0] = b, x[t, b, 1] = t: exact in float32 below 2^24
    traj[:, :, 1] = steps.float()[:, None]
    cost.copy_(((env % 4096) * 256)[None, :] + steps[:, None])              # < 2^21: exact as well
    gen = torch.Generator(device="cuda").manual_seed(log2_B)
    done_step = torch.randint(0, T + 1, (B,), generator=gen, device="cuda", dtype=torch.int32)
    K = int((done_step.long() + 1).sum())
    assert K > capacity
    rb = _ring(n, capacity, torch.float32, 123457, 500000)
    workspace = _abi.lib().hjbx_replay_append_workspace_bytes(B)
    assert workspace <= B // 64 * 12 + 64
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    assert rb.extend_rollout(traj, cost, done_step) == K                   # the header's K
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"B = 2^{log2_B}: K = {K}, peak device memory rose by {rise} bytes during the append (workspace {workspace} bytes)")
    assert rise <= workspace + (1 << 20)                                   # no copy of the log (8.4 GB at 2^20) was made
    assert rb.size == capacity and rb.head == 123457                       # a full turn
    idx = (rb.head + torch.arange(capacity, device="cuda")) % capacity
    x, c, dn = rb.x[idx], rb.cost[idx], rb.done[idx]
    assert not torch.isnan(x[:, :2]).any() and not torch.isnan(c).any() and not torch.isnan(dn).any()       # every slot was written
    b, t = x[:, 0].long(), x[:, 1].long()
    assert torch.equal(x[:, 0], b.float()) and torch.equal(x[:, 1], t.float())
    ds = done_step.long()
    last = t == ds[b]
    assert torch.equal(dn, last.float())                                   # done == 1 exactly where t == done_step[b]
    assert torch.equal(c, ((b % 4096) * 256 + t).float())
    # each slot is one step further along the trajectory-major order than the one before it
    nb, nt = b[1:], t[1:]
    assert torch.equal(nb, torch.where(last[:-1], b[:-1] + 1, b[:-1])) and torch.equal(nt, torch.where(last[:-1], torch.zeros_like(nt), t[:-1] + 1))
    assert int(b[-1]) == B - 1 and int(t[-1]) == int(ds[B - 1])
    # and it starts where the records that no longer fit end: running index K - capacity
    off = torch.cumsum(ds + 1, 0) - (ds + 1)
    assert int(off[b[0]] + t[0]) == K - capacity


def test_full_size_cartpole_shape_lands_the_rows_of_the_log(big_log):
    """n = 4, B = 2^20, T = 200 (16-byte records, each workgroup striding over several time tiles), random data: every slot of the ring against
    the row of the log its running index names, gathered by plain indexing.  (Not against the torch expression: on a log of this size, 3.4 GB,
    its masked transposed copy was observed to deliver all-zero states on the MI355X; up to B = 4 * 10^5 the two agree bit for bit.)"""
    T, n, B, capacity, head = 200, 4, 1 << 20, 10 ** 6, 999999
    traj = big_log["traj"][:(T + 1) * B * n].view(T + 1, B, n)
    cost = big_log["cost"][:(T + 1) * B].view(T + 1, B)
    gen = torch.Generator(device="cuda").manual_seed(4)
    traj.normal_(generator=gen)
    cost.normal_(generator=gen)
    done_step = torch.randint(0, T + 1, (B,), generator=gen, device="cuda", dtype=torch.int32)
    rb = _ring(n, capacity, torch.float32, head, capacity)
    L = done_step.long() + 1
    K = rb.extend_rollout(traj, cost, done_step)
    assert K == int(L.sum()) > capacity and rb.head == head and rb.size == capacity
    off = torch.cumsum(L, 0) - L
    j = (torch.arange(capacity, device="cuda") - head) % capacity + (K - capacity)       # the running index that lands in each slot
    b = torch.searchsorted(off, j, right=True) - 1
    t = j - off[b]
    assert int(t.min()) >= 0 and bool((t < L[b]).all())
    assert torch.equal(_bits(rb.x), _bits(traj[t, b])) and torch.equal(_bits(rb.cost), _bits(cost[t, b]))
    assert torch.equal(rb.done, (t == done_step[b]).float())
