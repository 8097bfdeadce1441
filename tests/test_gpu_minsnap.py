"""The min-snap planner on the device: hjbx_minsnap_reference_* and hjbx_rollout_minsnap_tracking_* against the golden fixture of
tools/gen_golden_minsnap.py (the reference's NumPy planner; a tracking loop composed of reference pieces) and the restatement
tests/minsnap_ref.py, which tests/test_minsnap_host.py pins on the CPU.

Shapes: B in {1, 65, 257} (a lone lane, a partial second wave, a partial second workgroup of 256), S in {1, 3} (plan 2 has one segment), the
fixture's grids (39 - 359 steps: every segment change and the hover tail are crossed).  Environment b starts from the golden start b % 4.
Bounds: float64 against golden 1e-12 x component scale (reference generator) and 1e-9 x scale (closed loops), the project's levels;
float32: max error per component <= 2 x the error of the float32 restatement against the same golden, floor 2^-24 x scale (DESIGN.md
section 6)."""
import numpy as np
import pytest
import torch

import minsnap_ref as M
from conftest import make_dynamics
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller.quadrotors_model_based_controller import Quadrotors2DTrackingController, Quadrotors2DWaypointsPlanner
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D

pytestmark = pytest.mark.gpu

BATCHES = (1, 65, 257)
PLANS = (0, 1, 2, 3)            # S = 3, 3, 1, 3
TORCH = {"f32": torch.float32, "f64": torch.float64}
INT = {torch.float32: torch.int32, torch.float64: torch.int64}
SENTINEL = {torch.float32: 0x7FC0DEAD, torch.float64: 0x7FF8DEADBEEF0000}      # NaNs with a payload no computation produces


def _bits(t):
    return t.view(INT[t.dtype])


@pytest.fixture(scope="module")
def gold():
    return M.golden()


@pytest.fixture(scope="module")
def quad():
    return make_dynamics("quad2d")


@pytest.fixture(scope="module")
def plans(gold):
    return [M.plan_of(gold, i) for i in PLANS]


@pytest.fixture(scope="module")
def yard(gold, plans):
    """computed once, never modified: per plan the float32 restatement of update(t_k) and of the four Euler loops, and the float64 RK4 loops"""
    out = []
    for p in plans:
        steps = len(p["t"])
        args = (gold["K"], gold["Q"], gold["R"], gold["umin"], gold["umax"], gold["params"])
        loops32 = [M.tracking_loop(p, p["x0"][b], steps, *args, dtype=np.float32) for b in range(4)]
        rk4 = [M.tracking_loop(p, p["x0"][b], steps, *args, rk4=True) for b in range(4)]
        out.append(dict(ref32=M.reference_grid(p, gold["params"], steps, dtype=np.float32),
                        loop32={k: np.stack([l[k] for l in loops32]) for k in ("traj", "u", "cost")},
                        rk4={k: np.stack([l[k] for l in rk4]) for k in ("traj", "u", "cost")}))
    return out


def _device_plan(p, dtype):
    """(coeff (1, 2, S, 8), cum_t (1, S + 1) float64, end_pt (1, 2)) of one golden plan: the golden coefficients themselves"""
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda", dt)
    return up(p["coeff"][None], dtype), up(p["cumulated_t"][None], torch.float64), up(p["waypoints"][-1][None], dtype)


def _ctrl_task(gold):
    ctrl = _abi.make_controller(_abi.CTRL_LINEAR_FEEDBACK, 6, 2, gold["K"])
    task = _abi.make_task(6, 2, gold["Q"], gold["R"], None, np.zeros(6), np.zeros(2), None, None, 0.0)
    return ctrl, task


def _starts(p, B, dtype):
    return torch.from_numpy(p["x0"][np.arange(B) % 4]).to("cuda", dtype).contiguous()


def _rollout(quad, gold, p, B, dtype, integrator=_abi.EULER, **kw):
    ctrl, task = _ctrl_task(gold)
    kw = dict(dict(task=task, log_cost=True, log_reference=True), **kw)
    out = _ops.rollout_minsnap_tracking(quad.system, ctrl, *_device_plan(p, dtype), _starts(p, B, dtype), len(p["t"]), integrator=integrator, **kw)
    torch.cuda.synchronize()
    return out


def _by_start(a, B):
    """time-major device log (T, B, ...) -> numpy (B, T, ...)"""
    return np.moveaxis(a.cpu().numpy().astype(np.float64), 1, 0)


def _comp_err(a, ref):
    """max |a - ref| per component of the last axis"""
    d = np.abs(np.asarray(a, np.float64) - ref)
    return d.reshape(-1, d.shape[-1]).max(axis=0)


# ---- the reference generator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("i", PLANS)
def test_reference_f64_matches_golden(quad, plans, i, B):
    p = plans[i]
    xr, ur = _ops.minsnap_reference(quad.system, *_device_plan(p, torch.float64), len(p["t"]), B=B)
    assert xr.shape == (len(p["t"]), B, 6) and ur.shape == (len(p["t"]), B, 2)
    for a, ref, name in ((xr, p["x_ref"], "x_ref"), (ur, p["u_ref"], "u_ref")):
        a = _by_start(a, B)
        err = (_comp_err(a, ref[None]) / M.scale(ref)).max()
        print(f"plan {i} B {B}: {name} f64 vs golden {err:.2e} of the component scale")
        assert err <= 1e-12
        assert (a == a[:1]).all()                     # every environment of a shared plan gets the same bits


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("i", PLANS)
def test_reference_f32_within_twice_the_float32_restatement(quad, plans, yard, i, B):
    p = plans[i]
    assert np.abs(p["t"][:, None] - p["cumulated_t"][None, 1:]).min() >= 1e-3     # a float32 implementation picks the same segments
    xr, ur = _ops.minsnap_reference(quad.system, *_device_plan(p, torch.float32), len(p["t"]), B=B)
    for a, ref, y, name in ((xr, p["x_ref"], yard[i]["ref32"][0], "x_ref"), (ur, p["u_ref"], yard[i]["ref32"][1], "u_ref")):
        err, yerr = _comp_err(_by_start(a, B), ref[None]), _comp_err(y, ref)
        bound = np.maximum(2 * yerr, 2.0 ** -24 * M.scale(ref))
        print(f"plan {i} B {B}: {name} f32 kernel err {err}, restatement err {yerr}, worst ratio to the bound {(err / bound).max():.2f}")
        assert (err <= bound).all()


# ---- the tracking rollout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("i", PLANS)
def test_tracking_f64_euler_matches_the_golden_closed_loop(quad, gold, plans, i, B):
    p = plans[i]
    out = _rollout(quad, gold, p, B, torch.float64)
    idx = np.arange(B) % 4
    for key in ("traj", "u"):
        err = (_comp_err(_by_start(out[key], B), p[key][idx]) / M.scale(p[key])).max()
        print(f"plan {i} B {B}: {key} f64 vs golden {err:.2e} of the component scale")
        assert err <= 1e-9
    cost = out["cost"].cpu().numpy()
    err = np.abs(cost.T - p["cost"][idx]).max() / np.abs(p["cost"]).max()
    print(f"plan {i} B {B}: cost f64 vs golden {err:.2e} of the scale")
    assert err <= 1e-9
    # total_cost is the sum of the logged step costs in time order, and x_final the last row of traj
    assert np.array_equal(out["total_cost"].cpu().numpy(), np.cumsum(cost, axis=0)[-1])
    assert torch.equal(out["x_final"], out["traj"][-1])
    assert torch.equal(out["traj"][0], _starts(p, B, torch.float64))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("i", PLANS)
def test_tracking_f32_euler_within_twice_the_float32_restatement(quad, gold, plans, yard, i, B):
    p = plans[i]
    out = _rollout(quad, gold, p, B, torch.float32)
    idx = np.arange(B) % 4
    for key in ("traj", "u", "cost"):
        a, ref, y = _by_start(out[key], B), p[key], yard[i]["loop32"][key]
        if key == "cost":
            a, ref, y = a[..., None], ref[..., None], y[..., None]
        err, yerr = _comp_err(a, ref[idx]), _comp_err(y, ref)
        bound = np.maximum(2 * yerr, 2.0 ** -24 * M.scale(ref))
        print(f"plan {i} B {B}: {key} f32 kernel err {err}, restatement err {yerr}, worst ratio to the bound {(err / bound).max():.2f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("B", (1, 257))
@pytest.mark.parametrize("i", PLANS)
def test_tracking_f64_rk4_matches_the_restatement(quad, gold, plans, yard, i, B):
    p = plans[i]
    out = _rollout(quad, gold, p, B, torch.float64, integrator=_abi.RK4)
    idx = np.arange(B) % 4
    for key in ("traj", "u"):
        err = (_comp_err(_by_start(out[key], B), yard[i]["rk4"][key][idx]) / M.scale(p[key])).max()
        print(f"plan {i} B {B}: {key} f64 RK4 vs restatement {err:.2e} of the component scale")
        assert err <= 1e-9
    err = np.abs(out["cost"].cpu().numpy().T - yard[i]["rk4"]["cost"][idx]).max() / np.abs(p["cost"]).max()
    assert err <= 1e-9
    # RK4 is not Euler: the two loops differ by far more than the bound
    assert np.abs(yard[i]["rk4"]["traj"] - p["traj"]).max() > 1e-4


@pytest.mark.parametrize("integrator", (_abi.EULER, _abi.RK4))
def test_per_step_identity_from_the_kernels_own_logs(quad, gold, plans, integrator):
    """u_log[k] == clip(u_ref_log[k] - K wrap(traj[k] - x_ref_log[k])) to 1e-12, float64"""
    p = plans[0]
    out = _rollout(quad, gold, p, 65, torch.float64, integrator=integrator)
    traj, u, xr, ur = (out[k].cpu().numpy() for k in ("traj", "u", "x_ref", "u_ref"))
    e = traj[:-1] - xr
    e[..., 2] = np.remainder(e[..., 2] + np.pi, 2 * np.pi) - np.pi
    want = np.clip(ur - e @ gold["K"].T, gold["umin"], gold["umax"])
    assert np.abs(u - want).max() <= 1e-12 * M.scale(p["u"]).max()


@pytest.mark.parametrize("sfx", ("f32", "f64"))
@pytest.mark.parametrize("i", (0, 2))
def test_reference_logs_are_bit_equal_to_the_reference_generator(quad, gold, plans, sfx, i):
    """the two kernels call one device function"""
    p, B = plans[i], 257
    out = _rollout(quad, gold, p, B, TORCH[sfx])
    xr, ur = _ops.minsnap_reference(quad.system, *_device_plan(p, TORCH[sfx]), len(p["t"]), B=B)
    assert torch.equal(_bits(out["x_ref"]), _bits(xr)) and torch.equal(_bits(out["u_ref"]), _bits(ur))


def test_saturating_controls(gold, plans, quad):
    """umax lowered to 6 (the golden loop of plan 0 asks for up to 7.3) and umin raised to 4: controls sit at both limits, and the float64
    kernel still follows the restatement with the same limits"""
    p, B = plans[0], 65
    tight = Quadrotors2D(D.quadrotors2d_dynamics_config(umin=[4.0, 4.0], umax=[6.0, 6.0]))
    ctrl, task = _ctrl_task(gold)
    out = _ops.rollout_minsnap_tracking(tight.system, ctrl, *_device_plan(p, torch.float64), _starts(p, B, torch.float64), len(p["t"]), task=task,
                                        log_cost=True)
    want = [M.tracking_loop(p, p["x0"][b], len(p["t"]), gold["K"], gold["Q"], gold["R"], [4.0, 4.0], [6.0, 6.0], gold["params"]) for b in range(4)]
    idx = np.arange(B) % 4
    u = _by_start(out["u"], B)
    assert (u == 6.0).sum() > B and (u == 4.0).sum() > B and ((u > 4.0) & (u < 6.0)).sum() > B
    for key in ("traj", "u"):
        ref = np.stack([w[key] for w in want])
        assert (_comp_err(_by_start(out[key], B), ref[idx]) / M.scale(ref)).max() <= 1e-9
    ref = np.stack([w["cost"] for w in want])
    assert np.abs(out["cost"].cpu().numpy().T - ref[idx]).max() <= 1e-9 * np.abs(ref).max()


# ---- plan layout ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ("f32", "f64"))
def test_shared_plan_equals_copies_of_it(quad, gold, plans, sfx):
    p, B, dtype = plans[3], 257, TORCH[sfx]
    shared = _rollout(quad, gold, p, B, dtype)
    coeff, cum_t, end_pt = _device_plan(p, dtype)
    ctrl, task = _ctrl_task(gold)
    copies = _ops.rollout_minsnap_tracking(quad.system, ctrl, coeff.repeat(B, 1, 1, 1), cum_t.repeat(B, 1), end_pt.repeat(B, 1), _starts(p, B, dtype),
                                           len(p["t"]), task=task, log_cost=True, log_reference=True)
    for key in shared:
        assert torch.equal(_bits(shared[key]), _bits(copies[key])), key
    a = _ops.minsnap_reference(quad.system, coeff, cum_t, end_pt, len(p["t"]), B=B)
    b = _ops.minsnap_reference(quad.system, coeff.repeat(B, 1, 1, 1), cum_t.repeat(B, 1), end_pt.repeat(B, 1), len(p["t"]))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("B", (65, 257))
def test_one_plan_per_environment(quad, gold, plans, B):
    """environment b flies plan (0, 3, 1)[b % 3] (distinct waypoints and speeds, all S = 3) from that plan's golden start b % 4, for the
    steps of the shortest grid: each matches its own golden loop, and the product's stacked planner gives the same device plan"""
    ids = np.array([0, 3, 1])[np.arange(B) % 3]
    steps = min(len(plans[i]["t"]) for i in (0, 3, 1))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda", dt)
    coeff = up(np.stack([plans[i]["coeff"] for i in ids]), torch.float64)
    cum_t = up(np.stack([plans[i]["cumulated_t"] for i in ids]), torch.float64)
    end_pt = up(np.stack([plans[i]["waypoints"][-1] for i in ids]), torch.float64)
    x0 = up(np.stack([plans[i]["x0"][b % 4] for b, i in enumerate(ids)]), torch.float64)
    ctrl, task = _ctrl_task(gold)
    out = _ops.rollout_minsnap_tracking(quad.system, ctrl, coeff, cum_t, end_pt, x0, steps, task=task, log_cost=True, log_reference=True)
    xr, ur = _ops.minsnap_reference(quad.system, coeff, cum_t, end_pt, steps)
    assert torch.equal(_bits(out["x_ref"]), _bits(xr)) and torch.equal(_bits(out["u_ref"]), _bits(ur))
    traj, u, xr = _by_start(out["traj"], B), _by_start(out["u"], B), _by_start(xr, B)
    for b, i in enumerate(ids):
        p = plans[i]
        assert (np.abs(xr[b] - p["x_ref"][:steps]) <= 1e-12 * M.scale(p["x_ref"])).all()
        assert (np.abs(traj[b] - p["traj"][b % 4][:steps + 1]) <= 1e-9 * M.scale(p["traj"])).all()
        assert (np.abs(u[b] - p["u"][b % 4][:steps]) <= 1e-9 * M.scale(p["u"])).all()


def test_every_optional_output_may_be_null(quad, gold, plans):
    p, B, T = plans[2], 65, len(plans[2]["t"])
    full = _rollout(quad, gold, p, B, torch.float64)
    coeff, cum_t, end_pt = _device_plan(p, torch.float64)
    ctrl, task = _ctrl_task(gold)
    x0 = _starts(p, B, torch.float64)
    fn, L = _abi.lib().hjbx_rollout_minsnap_tracking_f64, T
    outs = dict(traj=(T + 1, B, 6), u=(T, B, 2), cost=(T, B), total_cost=(B,), x_final=(B, 6), x_ref=(T, B, 6), u_ref=(T, B, 2))
    order = ("traj", "u", "cost", "total_cost", "x_final", "x_ref", "u_ref")
    for only in order + (None,):                    # one output at a time, then none at all
        bufs = {k: (torch.empty(outs[k], dtype=torch.float64, device="cuda") if k == only else None) for k in order}
        t = _abi.ref(task) if only in ("cost", "total_cost") else None
        rc = fn(quad.system.ptr, t, _abi.ref(ctrl), _abi.EULER, coeff.data_ptr(), cum_t.data_ptr(), end_pt.data_ptr(), 1, 1, 0.0, L, x0.data_ptr(),
                *[None if bufs[k] is None else bufs[k].data_ptr() for k in order], B, None)
        torch.cuda.synchronize()
        assert rc == _abi.OK, _abi.last_error()
        if only is not None:
            assert torch.equal(_bits(bufs[only]), _bits(full[only])), only
    xr, _ = _ops.minsnap_reference(quad.system, coeff, cum_t, end_pt, L, B=B)
    only_x = torch.empty_like(xr)
    assert _abi.lib().hjbx_minsnap_reference_f64(quad.system.ptr, coeff.data_ptr(), cum_t.data_ptr(), end_pt.data_ptr(), 1, 1, 0.0, L, only_x.data_ptr(), None,
                                                 B, None) == _abi.OK
    torch.cuda.synchronize()
    assert torch.equal(_bits(only_x), _bits(xr))


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ("f32", "f64"))
def test_argument_errors_launch_nothing(quad, gold, plans, sfx):
    p, B, dtype, T = plans[0], 65, TORCH[sfx], 5
    coeff, cum_t, end_pt = _device_plan(p, dtype)
    ctrl, task = _ctrl_task(gold)
    x0 = _starts(p, B, dtype)
    traj = torch.empty((T + 1, B, 6), dtype=dtype, device="cuda")
    xr = torch.empty((T, B, 6), dtype=dtype, device="cuda")
    _bits(traj).fill_(SENTINEL[dtype]); _bits(xr).fill_(SENTINEL[dtype])
    other = make_dynamics("nearhover")
    L = _abi.lib()

    def track(**kw):
        a = dict(sys=quad.system.ptr, ctrl=_abi.ref(ctrl), integ=_abi.EULER, coeff=coeff.data_ptr(), cum_t=cum_t.data_ptr(), end_pt=end_pt.data_ptr(), S=3,
                 n_plans=1, t0=0.0, T=T, x0=x0.data_ptr(), B=B)
        a.update(kw)
        return getattr(L, f"hjbx_rollout_minsnap_tracking_{sfx}")(a["sys"], _abi.ref(task), a["ctrl"], a["integ"], a["coeff"], a["cum_t"], a["end_pt"], a["S"],
                                                                a["n_plans"], a["t0"], a["T"], a["x0"], traj.data_ptr(), None, None, None, None,
                                                                xr.data_ptr(), None, a["B"], None)

    def reference(**kw):
        a = dict(sys=quad.system.ptr, coeff=coeff.data_ptr(), cum_t=cum_t.data_ptr(), end_pt=end_pt.data_ptr(), S=3, n_plans=1, t0=0.0, T=T, B=B)
        a.update(kw)
        return getattr(L, f"hjbx_minsnap_reference_{sfx}")(a["sys"], a["coeff"], a["cum_t"], a["end_pt"], a["S"], a["n_plans"], a["t0"], a["T"],
                                                          xr.data_ptr(), None, a["B"], None)

    bad = [dict(sys=other.system.ptr), dict(S=0), dict(t0=-1.0), dict(T=-1), dict(n_plans=2), dict(n_plans=B + 1), dict(coeff=None), dict(cum_t=None),
           dict(end_pt=None)]
    for kw in bad:
        assert track(**kw) == _abi.EINVAL and reference(**kw) == _abi.EINVAL, kw
    for kw in (dict(x0=None), dict(ctrl=None), dict(integ=_abi.ZOH)):
        assert track(**kw) == _abi.EINVAL, kw
    torch.cuda.synchronize()
    assert (_bits(traj) == SENTINEL[dtype]).all() and (_bits(xr) == SENTINEL[dtype]).all()      # nothing was launched
    assert track() == _abi.OK and reference() == _abi.OK                                        # the same calls, valid: they do write
    torch.cuda.synchronize()
    assert not (_bits(traj) == SENTINEL[dtype]).any() and not (_bits(xr) == SENTINEL[dtype]).any()


# ---- the public classes ---------------------------------------------------------------------------------------------------------------------
def test_planner_reference_and_tracking_controller(quad, gold, plans):
    p = plans[0]
    steps = len(p["t"])
    pl = Quadrotors2DWaypointsPlanner(p["waypoints"], quad, avg_speed=1.0)
    xr, ur = pl.reference(steps, dtype=torch.float64)
    assert xr.is_cuda and xr.shape == (steps, 1, 6) and ur.shape == (steps, 1, 2)
    assert (np.abs(xr[:, 0].cpu().numpy() - p["x_ref"]) <= 1e-9 * M.scale(p["x_ref"])).all()      # (the planner's own solve: cond(A) 2^-53 ~ 1e-11)
    assert (np.abs(ur[:, 0].cpu().numpy() - p["u_ref"]) <= 1e-9 * M.scale(p["u_ref"])).all()
    assert pl.reference(7)[0].dtype == torch.float32
    tc = Quadrotors2DTrackingController(quad, pl, gold["Q"], gold["R"])
    out = tc.rollout(p["x0"], steps, log_cost=True, log_reference=True)                           # numpy in -> numpy out
    assert all(isinstance(out[k], np.ndarray) for k in ("traj", "u", "cost", "total_cost", "x_final", "x_ref", "u_ref"))
    assert out["traj"].shape == (steps + 1, 4, 6) and out["u"].shape == (steps, 4, 2) and out["cost"].shape == (steps, 4)
    assert (np.abs(np.moveaxis(out["traj"], 1, 0) - p["traj"]) <= 1e-8 * M.scale(p["traj"])).all()
    assert (np.abs(np.moveaxis(out["u"], 1, 0) - p["u"]) <= 1e-8 * M.scale(p["u"])).all()
    # the law at one time, for one state and for a batch; a rollout that starts at t0 continues the same plan
    k = 30
    u1 = tc.get_control_efforts(out["traj"][k, 2], p["t"][k])
    assert u1.shape == (2,) and np.array_equal(u1, out["u"][k, 2])
    assert np.array_equal(tc.get_control_efforts(out["traj"][k], p["t"][k]), out["u"][k])
    tail = tc.rollout(out["traj"][k], steps - k, t0=p["t"][k])
    assert np.abs(tail["traj"] - out["traj"][k:]).max() <= 1e-12 and np.abs(tail["u"] - out["u"][k:]).max() <= 1e-11      # (t0 + j dt vs (k + j) dt: an ulp of t)
    dev = tc.rollout(torch.from_numpy(p["x0"]).cuda(), 5, log_traj=False, log_u=False)
    assert dev["traj"] is None and dev["u"] is None and dev["x_final"].is_cuda and dev["total_cost"].shape == (4,)
    # stacked plans: one per environment
    stacked = Quadrotors2DWaypointsPlanner(np.stack([plans[0]["waypoints"], plans[3]["waypoints"]]), quad, avg_speed=1.0)
    xs, _ = stacked.reference(20, dtype=torch.float64)
    assert xs.shape == (20, 2, 6) and (np.abs(xs[:, 1].cpu().numpy() - plans[3]["x_ref"][:20]) <= 1e-9 * M.scale(plans[3]["x_ref"])).all()
    two = Quadrotors2DTrackingController(quad, stacked, gold["Q"], gold["R"]).rollout(np.stack([plans[0]["x0"][1], plans[3]["x0"][2]]), 20)
    assert (np.abs(two["traj"][:, 1] - plans[3]["traj"][2][:21]) <= 1e-8 * M.scale(plans[3]["traj"])).all()
    with pytest.raises(ValueError):
        Quadrotors2DTrackingController(quad, stacked, gold["Q"], gold["R"]).rollout(plans[0]["x0"][:3], 5)       # 2 plans, 3 environments
