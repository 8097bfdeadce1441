"""The min-snap waypoint planner of Quadrotors2D on the host (no GPU): the golden fixture of tools/gen_golden_minsnap.py (the reference's own
NumPy planner and a tracking loop composed of reference pieces) pins the test-side restatement tests/minsnap_ref.py and the product's
Quadrotors2DWaypointsPlanner; the C entry points' argument checks; the ISA audit of csrc/hjbx_track.hip."""
import os
import re
import subprocess

import numpy as np
import pytest

import minsnap_ref as M
from conftest import ROOT, make_dynamics
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.controller.quadrotors_model_based_controller import (Quadrotors2DHoveringController, Quadrotors2DTrackingController,
                                                                                  Quadrotors2DWaypointsPlanner)

EPS64 = 2.0 ** -53
N_PLANS = 4


@pytest.fixture(scope="module")
def gold():
    return M.golden()


@pytest.fixture(scope="module")
def quad():
    return make_dynamics("quad2d")


def _rel(err, ref):
    """max over components of (max |err| / component scale of the golden array)"""
    return float((np.abs(err).reshape(-1, err.shape[-1]).max(axis=0) / M.scale(ref)).max())


# ---- the fixture and the restatement -------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_issue_asks_for(gold):
    assert int(gold["n_plans"]) == N_PLANS and float(gold["dt"]) == 0.05 and float(gold["t0"]) == 0.0
    w0 = [[0, 0], [1, 0.5], [1.5, -0.5], [0, 1]]
    assert np.array_equal(gold["p0_waypoints"], w0) and float(gold["p0_avg_speed"]) == 1.0
    assert np.array_equal(gold["p1_waypoints"], w0) and float(gold["p1_avg_speed"]) == 0.25
    assert np.array_equal(gold["p2_waypoints"], [[0, 0], [1, 1]]) and float(gold["p2_avg_speed"]) == 1.0
    assert gold["p3_waypoints"].shape == (4, 2) and float(gold["p3_avg_speed"]) == 1.0
    for i in range(N_PLANS):
        p = M.plan_of(gold, i)
        S = p["waypoints"].shape[0] - 1
        steps = int(np.ceil(p["cumulated_t"][-1] / 0.05)) + 10
        assert p["coeff"].shape == (2, S, 8) and p["interval_t"].shape == (S,) and p["cumulated_t"].shape == (S + 1,)
        assert np.array_equal(p["t"], [0.0 + k * 0.05 for k in range(steps)])          # t_k = t0 + k dt, not accumulated
        assert p["t"][-1] > p["cumulated_t"][-1] + 0.4                                     # the hover tail is on the grid
        assert p["x_ref"].shape == (steps, 6) and p["u_ref"].shape == (steps, 2)
        assert p["x0"].shape == (4, 6) and p["traj"].shape == (4, steps + 1, 6) and p["u"].shape == (4, steps, 2) and p["cost"].shape == (4, steps)
        assert np.abs(p["t"][:, None] - p["cumulated_t"][None, 1:]).min() >= 1e-3          # no grid time within 1e-3 s of a segment boundary
        assert np.abs(p["x0"][:, :2] - p["waypoints"][0]).max() <= 0.3 and np.abs(p["x0"][:, 2:]).max() <= 0.3
        assert np.abs(p["u"]).max() < 20.0                                                 # no control of the golden loops saturates
    assert os.path.getsize(M.GOLDEN) < 400 * 1024


@pytest.mark.parametrize("i", range(N_PLANS))
def test_restatement_reproduces_the_golden_update(gold, i):
    """float64 restatement (Horner, same formulas) == the reference's update(t_k) to 1e-12 x component scale (measured: 4e-14)."""
    p = M.plan_of(gold, i)
    xr, ur = M.reference_grid(p, gold["params"], len(p["t"]))
    ex, eu = _rel(xr - p["x_ref"], p["x_ref"]), _rel(ur - p["u_ref"], p["u_ref"])
    print(f"plan {i}: update(t) restatement vs golden: x_ref {ex:.2e}, u_ref {eu:.2e} of the component scale")
    assert ex <= 1e-12 and eu <= 1e-12


@pytest.mark.parametrize("i", range(N_PLANS))
def test_restatement_reproduces_the_golden_closed_loop(gold, i):
    """float64 restatement of the Euler tracking loop == the loop composed of reference pieces to 1e-12 x component scale (measured: 6e-14)."""
    p = M.plan_of(gold, i)
    for b in range(4):
        o = M.tracking_loop(p, p["x0"][b], len(p["t"]), gold["K"], gold["Q"], gold["R"], gold["umin"], gold["umax"], gold["params"])
        et, eu = _rel(o["traj"] - p["traj"][b], p["traj"]), _rel(o["u"] - p["u"][b], p["u"])
        ec = float(np.abs(o["cost"] - p["cost"][b]).max() / np.abs(p["cost"]).max())
        print(f"plan {i} start {b}: loop restatement vs golden: traj {et:.2e}, u {eu:.2e}, cost {ec:.2e} of the scale")
        assert et <= 1e-12 and eu <= 1e-12 and ec <= 1e-12


def test_restatement_rk4_converges_on_euler_with_a_small_step(gold):
    """the RK4 loop of the restatement (the yardstick of the RK4 kernel) is a 4th-order step: one RK4 step == 64 Euler steps of dt / 64
    under a constant control, to O(dt^2 / 64)"""
    params, dt = gold["params"], np.float64
    x = np.array([0.1, -0.2, 0.3, 0.4, -0.5, 0.6])
    u = np.array([5.5, 4.5])
    xe = x.copy()
    for _ in range(4096):
        xe = M.step(xe, u, params, dt(0.05 / 4096), dt, rk4=False)
    xr = M.step(x, u, params, dt(0.05), dt, rk4=True)
    assert np.abs(xr - xe).max() < 2e-5 and np.abs(M.step(x, u, params, dt(0.05), dt, rk4=False) - xe).max() > 1e-3


# ---- the product planner --------------------------------------------------------------------------------------------------------------------
def _check_plan(planner_attrs, p, bound, tag):
    interval_t, cumulated_t, coeff = planner_attrs
    assert np.abs(interval_t - p["interval_t"]).max() <= 4 * EPS64 * np.abs(p["interval_t"]).max()
    assert np.abs(cumulated_t - p["cumulated_t"]).max() <= 4 * EPS64 * np.abs(p["cumulated_t"]).max()
    err = float(np.abs(coeff - p["coeff"]).max() / np.abs(p["coeff"]).max())
    print(f"{tag}: coeff vs golden {err:.2e} relative (bound {bound:.2e})")
    assert coeff.shape == p["coeff"].shape and err <= bound


@pytest.mark.parametrize("i", range(N_PLANS))
def test_planner_reproduces_the_golden_plan(gold, quad, i):
    """bound: 100 cond(A) 2^-53 relative, cond(A) from the restatement's own A (a backward-stable solve of the same system in another row order)"""
    p = M.plan_of(gold, i)
    A = M.assemble(p["waypoints"], float(p["avg_speed"]))[2]
    bound = 100 * np.linalg.cond(A) * EPS64
    pl = Quadrotors2DWaypointsPlanner(p["waypoints"], quad, avg_speed=float(p["avg_speed"]))
    assert pl.points_num == p["waypoints"].shape[0] and np.array_equal(pl.points, p["waypoints"]) and pl.dim == 2
    _check_plan((pl.interval_t, pl.cumulated_t, pl.coeff), p, bound, f"plan {i}")
    out = [pl.update(t) for t in p["t"]]
    xr, ur = np.array([o[0] for o in out]), np.array([o[1] for o in out])
    ex, eu = _rel(xr - p["x_ref"], p["x_ref"]), _rel(ur - p["u_ref"], p["u_ref"])
    print(f"plan {i}: host update(t) vs golden: x_ref {ex:.2e}, u_ref {eu:.2e} of the component scale (bound {bound:.2e})")
    assert ex <= bound and eu <= bound
    # the polynomial term of upstream's get_polynomial_term
    assert np.array_equal(pl.get_polynomial_term(2.0, 0), 2.0 ** np.arange(8))
    assert np.array_equal(pl.get_polynomial_term(0.0, 2), [0, 0, 2, 0, 0, 0, 0, 0])
    assert np.array_equal(pl.get_polynomial_term(2.0, 3), [0, 0, 0, 6, 48, 240, 960, 3360])
    assert np.array_equal(pl.get_polynomial_term(3.0, 1, order=3), [0, 1, 6, 27])


def test_stacked_planner_reproduces_each_golden_plan(gold, quad):
    """(Bp, P, 2) waypoints: one stacked solve, every attribute with a leading plan axis, each plan as the single planner gives it"""
    ids = [0, 3, 0]                                  # the two four-waypoint plans at avg_speed 1.0 (one twice)
    plans = [M.plan_of(gold, i) for i in ids]
    pl = Quadrotors2DWaypointsPlanner(np.stack([p["waypoints"] for p in plans]), quad, avg_speed=1.0)
    assert pl.coeff.shape == (3, 2, 3, 8) and pl.interval_t.shape == (3, 3) and pl.cumulated_t.shape == (3, 4) and pl.points_num == 4
    for b, p in enumerate(plans):
        bound = 100 * np.linalg.cond(M.assemble(p["waypoints"], 1.0)[2]) * EPS64
        _check_plan((pl.interval_t[b], pl.cumulated_t[b], pl.coeff[b]), p, bound, f"stacked plan {b}")
    assert np.array_equal(pl.coeff[0], pl.coeff[2])
    for k in (0, 17, 40, len(plans[1]["t"]) - 1):    # inside segments and in plan 3's hover tail
        x, u = pl.update(plans[1]["t"][k])
        assert x.shape == (3, 6) and u.shape == (3, 2)
        for b, p in enumerate(plans):
            bound = 100 * np.linalg.cond(M.assemble(p["waypoints"], 1.0)[2]) * EPS64
            assert (np.abs(x[b] - p["x_ref"][k]) <= bound * M.scale(p["x_ref"])).all() and (np.abs(u[b] - p["u_ref"][k]) <= bound * M.scale(p["u_ref"])).all()


def test_hover_tail_and_exact_zero_branch(gold, quad):
    """past the last waypoint: the end point, zero rates, u = m g / 2 each (the sin(theta) == 0 branch)"""
    p = M.plan_of(gold, 0)
    pl = Quadrotors2DWaypointsPlanner(p["waypoints"], quad, avg_speed=1.0)
    x, u = pl.update(p["cumulated_t"][-1] + 0.3)
    assert np.array_equal(x, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]) and np.array_equal(u, [quad.m * quad.g / 2] * 2)
    x, u = pl.update(p["cumulated_t"][-1])           # t == the last boundary: already the hover (t >= cumulated_t[-1])
    assert np.array_equal(x, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    x, u = pl.update(0.0)                            # rest at the first waypoint: x_ddot = 0 exactly, the same branch with a snap != 0
    assert x[2] == 0 and np.allclose(x, 0, atol=1e-12) and abs(u.sum() - quad.m * quad.g) <= 1e-12 and abs(u[0] - u[1]) > 0.1


def test_three_dimensional_waypoints_and_bad_shapes(quad):
    w3 = np.array([[0, 0, 0], [1, 0.5, 0.2], [1.5, -0.5, 0.4]], float)
    pl = Quadrotors2DWaypointsPlanner(w3, quad, avg_speed=0.5)
    assert pl.dim == 3 and pl.coeff.shape == (3, 2, 8) and np.isfinite(pl.coeff).all()
    # the solved polynomials pass through the waypoints
    for s in range(2):
        assert np.allclose(pl.coeff[:, s, 0], w3[s], atol=1e-12)
        assert np.allclose(pl.coeff[:, s] @ pl.get_polynomial_term(pl.interval_t[s], 0), w3[s + 1], atol=1e-9)
    with pytest.raises(NotImplementedError):
        pl.update(0.1)
    with pytest.raises(NotImplementedError):
        pl.device_plan(None, None)
    for bad in (np.zeros((3, 4)), np.zeros((3,)), np.zeros((2, 3, 4)), np.zeros((1, 2)), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError):
            Quadrotors2DWaypointsPlanner(bad, quad)
    with pytest.raises(ValueError):
        Quadrotors2DWaypointsPlanner(np.array([[0.0, 0], [1, 1]]), quad, avg_speed=0.0)


def test_tracking_controller_has_the_hover_gain(gold, quad):
    p = M.plan_of(gold, 0)
    pl = Quadrotors2DWaypointsPlanner(p["waypoints"], quad, avg_speed=1.0)
    tc = Quadrotors2DTrackingController(quad, pl, np.eye(6), np.eye(2))
    hover = Quadrotors2DHoveringController(quad, np.zeros(6), np.eye(6), np.eye(2))
    assert np.array_equal(tc.K, hover.K) and np.array_equal(tc.P, hover.P)
    assert np.abs(tc.K - gold["K"]).max() <= 1e-12 * np.abs(gold["K"]).max()          # the reference controller's gain
    d = tc._descriptor()
    assert d.kind == _abi.CTRL_LINEAR_FEEDBACK and np.array_equal(np.array(d.K[:12]).reshape(2, 6), tc.K)


def test_device_calls_need_a_device(gold, quad):
    import torch
    if torch.cuda.is_available():
        return                                       # (with a device the same calls are tested in test_gpu_minsnap.py)
    p = M.plan_of(gold, 0)
    pl = Quadrotors2DWaypointsPlanner(p["waypoints"], quad, avg_speed=1.0)
    tc = Quadrotors2DTrackingController(quad, pl, np.eye(6), np.eye(2))
    with pytest.raises(RuntimeError, match="no HIP device"):
        pl.reference(10)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tc.rollout(p["x0"], 10)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tc.get_control_efforts(p["x0"][0], 0.1)


# ---- the C surface --------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("hjbx_minsnap_reference_f32", "hjbx_minsnap_reference_f64", "hjbx_rollout_minsnap_tracking_f32", "hjbx_rollout_minsnap_tracking_f64")


def test_new_symbols_are_declared_exported_and_built():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    L = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name)
        decl = re.search(r"/\* \((.*)\) \*/\nint " + name + r"\(", hdr)
        assert decl and "quadrotors_model_based_controller.py:" in decl.group(1), f"{name}: the declaration cites the reference lines it replaces"
    assert hdr.index("#undef HJBX_DECLARE") < hdr.index("int hjbx_minsnap_reference_f32(")     # plain declarations, outside the typed macro
    assert re.search(r"#define HJBX_VERSION 112\b", hdr) and L.hjbx_version() == 112
    assert ("hjbx_track.hip", (), "hjbx_track.o") in _abi._UNITS and "hjbx_minsnap.hpp" in _abi._HEADERS


def _args(sfx, quad, **kw):
    """arguments of the two entry points with dummy (non-NULL, aligned, never dereferenced) pointers except where `kw` says otherwise"""
    ctrl = _abi.make_controller(_abi.CTRL_LINEAR_FEEDBACK, 6, 2, np.zeros((2, 6)))
    task = _abi.make_task(6, 2, np.eye(6), np.eye(2), None, np.zeros(6), np.zeros(2), None, None, 0.0)
    a = dict(sys=quad.system.ptr, task=_abi.ref(task), ctrl=_abi.ref(ctrl), integrator=_abi.EULER, coeff=0x10000, cum_t=0x20000, end_pt=0x30000, S=3,
             n_plans=1, t0=0.0, T_steps=5, x0=0x40000, traj=0x50000, u_log=0x60000, cost=0x70000, total_cost=0x80000, x_final=0x90000,
             x_ref=0xa0000, u_ref=0xb0000, B=7, stream=None, _keep=(ctrl, task))
    a.update(kw)
    return a


def _reference(sfx, quad, **kw):
    a = _args(sfx, quad, **kw)
    return getattr(_abi.lib(), f"hjbx_minsnap_reference_{sfx}")(a["sys"], a["coeff"], a["cum_t"], a["end_pt"], a["S"], a["n_plans"], a["t0"], a["T_steps"],
                                                               a["x_ref"], a["u_ref"], a["B"], a["stream"])


def _tracking(sfx, quad, **kw):
    a = _args(sfx, quad, **kw)
    return getattr(_abi.lib(), f"hjbx_rollout_minsnap_tracking_{sfx}")(a["sys"], a["task"], a["ctrl"], a["integrator"], a["coeff"], a["cum_t"], a["end_pt"],
                                                                      a["S"], a["n_plans"], a["t0"], a["T_steps"], a["x0"], a["traj"], a["u_log"], a["cost"],
                                                                      a["total_cost"], a["x_final"], a["x_ref"], a["u_ref"], a["B"], a["stream"])


BAD_PLAN = [dict(sys=None), dict(S=0), dict(S=-1), dict(t0=-0.05), dict(t0=float("nan")), dict(T_steps=-1), dict(n_plans=2), dict(n_plans=0), dict(B=-1),
            dict(coeff=None), dict(cum_t=None), dict(end_pt=None), dict(coeff=0x10004), dict(cum_t=0x20004)]


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_entry_points_refuse_bad_arguments_before_any_launch(quad, sfx):
    """every refusal is HJBX_EINVAL from the host-side checks: with the dummy pointers of _args, a launch would fault (or, here, fail for
    want of a device) instead"""
    for bad in BAD_PLAN:
        assert _reference(sfx, quad, **bad) == _abi.EINVAL, bad
        assert _tracking(sfx, quad, **bad) == _abi.EINVAL, bad
    other = make_dynamics("cartpole")
    assert _reference(sfx, quad, sys=other.system.ptr) == _abi.EINVAL and "QUAD2D" in _abi.last_error()
    assert _tracking(sfx, quad, sys=other.system.ptr) == _abi.EINVAL and "QUAD2D" in _abi.last_error()
    assert _reference(sfx, quad, x_ref=0xa0004) == _abi.EINVAL
    energy = _abi.make_controller(_abi.CTRL_CARTPOLE_ENERGY, 6, 2, np.zeros((2, 6)))
    for bad in (dict(x0=None), dict(x0=0x40004), dict(ctrl=None), dict(ctrl=_abi.ref(energy)), dict(integrator=_abi.ZOH), dict(integrator=7), dict(task=None),
                dict(task=None, cost=None), dict(traj=0x50004), dict(u_log=0x60004), dict(x_ref=0xa0004)):
        assert _tracking(sfx, quad, **bad) == _abi.EINVAL, bad
    # nothing to do: HJBX_OK without a launch
    assert _reference(sfx, quad, B=0, n_plans=1) == _abi.OK and _reference(sfx, quad, T_steps=0) == _abi.OK
    assert _reference(sfx, quad, x_ref=None, u_ref=None) == _abi.OK
    assert _tracking(sfx, quad, B=0, n_plans=1) == _abi.OK


# ---- ISA audit ------------------------------------------------------------------------------------------------------------------------------
def test_tracking_kernels_use_no_scratch(tmp_path):
    """Every kernel of hjbx_track.hip (reference generator x 2 dtypes, tracking rollout x 2 integrators x 2 dtypes) compiles for gfx950 with a
    private segment of 0 bytes, no spilled VGPR and no scratch instruction."""
    asm = tmp_path / "track.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only", "-o", str(asm),
                    os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc", "hjbx_track.hip")], check=True, stderr=subprocess.DEVNULL)
    text = asm.read_text()
    meta = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
    kernels = meta.findall(text)
    assert sum("k_minsnap_reference" in k[0] for k in kernels) == 2 and sum("k_rollout_minsnap_tracking" in k[0] for k in kernels) == 4
    assert len(kernels) == 6
    for name, private, _sgpr_spill, vgpr_spill in kernels:
        assert int(private) == 0 and int(vgpr_spill) == 0, f"{name}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
    assert not re.search(r"^\s+scratch_(load|store)", text, flags=re.M) and "Folded Spill" not in text
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)
    assert len(lds) == 6 and all(int(v) == 0 for v in lds)                  # streaming family: no LDS
    # the row vector stores of RowIO: a 6-float state row leaves as dwordx2 stores, a 6-double row as dwordx4
    assert "global_store_dwordx2" in text and "global_store_dwordx4" in text
