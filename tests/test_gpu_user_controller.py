"""User-defined control laws on the device (DeviceController, hjbx_user_controller_*: csrc/hjbx_user_controller_kernels.hpp compiled at run
time around the law's snippet).  Run on the MI355X box with `-m gpu`.

The yardstick of most tests is the library's own built-in kernel: the four fixed controller kinds restated as snippets (tests/user_laws.py,
expression for expression from controller_eval) must give the SAME BITS as hjbx_rollout_feedback_* / hjbx_controller_* with the built-in
descriptor -- both sides are the same expressions under the same compiler flags, so no tolerance is needed.  The golden closed loops use
the bounds of test_gpu_parity.py::test_controller_gains_and_golden_closed_loop (the reference's own trajectories); the laws of time use
1 ulp of t0 + k dt and the float64 tolerance of test_gpu_parity.py (DT["f64"])."""
import itertools

import numpy as np
import pytest
import torch

import user_laws as UL
from conftest import ANGLE_IDX, load_golden, make_dynamics, make_vhjb_config, orc_system, wrapped_diff
from oracle import oracle as O
from parity_util import abs_err, check
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.configs import defaults as D
from test_gpu_parity import DT, TRAJ, _ctrl_objects, _double_integrator, dev
from test_gpu_user_system import UserQuad2D

pytestmark = pytest.mark.gpu

BS, TS = (1, 63, 257, 3001), (0, 1, 60)
KEYS = ("traj", "u", "cost", "total_cost", "x_final")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _assert_same(got, want, label):
    for k in KEYS:
        assert (got[k] is None) == (want[k] is None), (label, k)
        if want[k] is not None:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{label}: {k} differs in {(got[k] != want[k]).sum().item()} elements"
    assert torch.equal(got["done_step"], want["done_step"]), f"{label}: done_step differs"


class _Described:
    """a built-in linear-feedback law given by its descriptor"""

    def __init__(self, dynamics, desc):
        self.dynamics, self._desc = dynamics, desc

    def _descriptor(self):
        return self._desc


def _twin_case(case):
    """-> (dynamics, built-in controller, its DeviceController twin, config name, stop_at_target)"""
    if case == "di_bangbang":
        from q_learning_with_hjb_amd.controller.time_optimal import DoubleIntegratorTimeOptimalController
        d = _double_integrator()
        c = DoubleIntegratorTimeOptimalController(d)
        return d, c, UL.twin_of(c), "linear", True
    if case == "cartpole_feedback_wrap":       # linear feedback about the upright with the wrapped error, gain of the energy shaper's LQR branch
        d, es = _ctrl_objects("cartpole")
        c = _Described(d, _abi.make_controller(_abi.CTRL_LINEAR_FEEDBACK, 4, 1, es.get_lqr_term()[0], xf=es.xf, uf=[0.25], wrap_error=True))
        return d, c, UL.twin_of(c), "cartpole", False
    name = {"linear_feedback_nowrap": "linear", "cartpole_es": "cartpole", "acrobot_es": "acrobot"}[case]
    d, c = _ctrl_objects(name)
    return d, c, UL.twin_of(c), name, False


def _starts(cfg, xf, n, B, seed=21):
    """the start states of test_rollout_feedback_vs_oracle, every other row pushed out of the observation box"""
    rng = np.random.default_rng(seed)
    x0 = np.asarray(xf, np.float64) + rng.uniform(-1, 1, (B, n)) * np.asarray(cfg.obs_max, np.float64).clip(max=3.0) * 0.9
    x0[1::2] += np.sign(x0[1::2] - np.asarray(xf, np.float64)) * np.asarray(cfg.obs_max, np.float64).clip(max=3.0) * 0.4 * (rng.uniform(size=(B // 2, n)) < 0.3)
    return x0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["linear_feedback_nowrap", "cartpole_feedback_wrap", "cartpole_es", "acrobot_es", "di_bangbang"])
def test_twins_are_bit_identical_to_the_builtin_kernels(case, prec):
    """1. the four fixed kinds as snippets == the built-in kernels, bit for bit: every B x T, both integrators, terminate on and off"""
    tdt = DT[prec][0]
    d, c, twin, cfgname, stop = _twin_case(case)
    cfg = make_vhjb_config(cfgname)
    n, m = d.get_dimension()
    xf = np.asarray(c.xf if hasattr(c, "xf") else cfg.xf, np.float64)
    task = _abi.make_task(n, m, cfg.Q, cfg.R, np.eye(n) * 2.0, xf, getattr(c, "uf", cfg.uf), cfg.obs_min, cfg.obs_max, cfg.epsilon)
    x_all = dev(_starts(cfg, xf, n, max(BS)), tdt)
    desc = c._descriptor()
    for B in BS:
        x0 = x_all[:B].contiguous()
        assert torch.equal(_bits(_ops.user_controller_eval(twin.handle, x0)), _bits(_ops.controller(d.system, desc, x0))), (case, prec, B)
        for T, integ, terminate in itertools.product(TS, (_abi.EULER, _abi.RK4), (False, True)):
            kw = dict(task=task, integrator=integ, terminate=terminate, log_u=True, log_cost=True, stop_at_target=stop)
            want = _ops.rollout_feedback(d.system, desc, x0, T, **kw)
            got = _ops.user_controller_rollout(twin.handle, x0, T, **kw)
            _assert_same(got, want, f"{case} {prec} B={B} T={T} integrator={integ} terminate={terminate}")
    # the comparison saw every branch: environments that ended early and environments that ran the whole horizon
    ds = want["done_step"].cpu().numpy()
    assert (ds < 60).any() and ((ds == 60).any() or stop)
    # without a task: no cost outputs, the same states and controls
    want = _ops.rollout_feedback(d.system, desc, x_all[:257].contiguous(), 60, log_u=True, stop_at_target=stop)
    got = _ops.user_controller_rollout(twin.handle, x_all[:257].contiguous(), 60, log_u=True, stop_at_target=stop)
    _assert_same(got, want, f"{case} {prec} no task")


@pytest.mark.parametrize("name", ["cartpole", "acrobot"])
def test_golden_closed_loop(name):
    """2. the energy-shaping twins against the reference's own trajectories: the assertions and bounds of
    test_gpu_parity.py::test_controller_gains_and_golden_closed_loop"""
    g = load_golden(TRAJ[name])
    d, c = _ctrl_objects(name)
    twin = UL.twin_of(c)
    T = g["US"].shape[0]
    out = twin.rollout(g["XS"][0][None, :], T)           # numpy f64 in -> f64 kernels
    dd = np.abs(wrapped_diff(out["traj"][:, 0], g["XS"], ANGLE_IDX[name]))
    du = np.abs(out["u"][:, 0] - g["US"].reshape(T, -1))
    print(f"    {name}: first 150 steps traj {dd[:150].max():.2e} u {du[:150].max():.2e}; whole loop traj {dd.max():.2e}")
    assert dd[:150].max() < 1e-7 and du[:150].max() < 2e-6 and dd.max() < 1e-3
    assert int(out["done_step"][0]) == T
    u0 = twin.get_control_efforts(g["XS"][0])
    np.testing.assert_allclose(np.atleast_1d(u0), g["US"][0].reshape(-1), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_user_system_with_user_law(prec):
    """3. UserQuad2D + a hover-LQR snippet.

    FINDING: against built-in Quadrotors2D + Quadrotors2DHoveringController the pair is NOT bit-identical, in either precision, and the law
    has no part in it: the two SYSTEM structs round differently.  Quad2D::xdot writes f2 u out as `over_m(-s) * u[0] + over_m(-s) * u[1]`
    (float32: times the stored 1 / m) where the user system's generic xdot accumulates f2[i][j] * u[j] from zero and QUAD2D_SRC divides by
    p[0]; the library's own hjbx_rollout_feedback_* on the two handles therefore differs in the same last bits: the snippet's kernel on
    UserQuad2D is bit-equal to the built-in kernel on UserQuad2D (asserted below) and differed from the built-in kernel on Quadrotors2D
    (float64, B = 1, T = 60: in 127 of 366 trajectory elements; test_gpu_user_system.py compares the pair at 1e-12 / 1e-9, not bitwise).
    So, as the issue prescribes for a twin that is not bit-equal (DESIGN.md 4.8a states the cause):
      * the law and the new rollout body are checked bit for bit where both sides run the SAME system struct: the snippet on UserQuad2D ==
        hjbx_rollout_feedback_* with the built-in linear-feedback descriptor on UserQuad2D (its streaming code object);
      * the pair is compared through parity_util.check against the float64 oracle run with the built-in descriptor at the tolerances
        test_gpu_parity.py uses for this kernel: DT[prec] per closed-loop step (the law, one step from every start state), and for the
        60-step loop the bounds of test_rollout_feedback_vs_oracle (f64: 1e-9 of the environment's scale over the 12-step prefix and 1e-5
        over the horizon; f32: the median prefix error within DT["f32"])."""
    tdt, ndt, tol = DT[prec]
    d, c = _ctrl_objects("quad2d")
    uq = UserQuad2D(D.quadrotors2d_dynamics_config())
    twin = UL.twin_of(c, uq)
    cfg = make_vhjb_config("quad2d")
    task = _abi.make_task(6, 2, cfg.Q, cfg.R, np.eye(6) * 2.0, c.xf, c.uf, cfg.obs_min, cfg.obs_max, cfg.epsilon)
    x_all = dev(_starts(cfg, c.xf, 6, 3001), tdt)
    desc = c._descriptor()
    for B, T in ((1, 60), (63, 1), (257, 60), (3001, 60), (257, 0)):
        x0 = x_all[:B].contiguous()
        assert torch.equal(_bits(_ops.user_controller_eval(twin.handle, x0)), _bits(_ops.controller(uq.system, desc, x0)))
        for integ, terminate in itertools.product((_abi.EULER, _abi.RK4), (False, True)):
            kw = dict(task=task, integrator=integ, terminate=terminate, log_u=True, log_cost=True)
            _assert_same(_ops.user_controller_rollout(twin.handle, x0, T, **kw), _ops.rollout_feedback(uq.system, desc, x0, T, **kw),
                         f"user quad2d {prec} B={B} T={T} integrator={integ} terminate={terminate}")
    # the pair against the float64 oracle of the built-in system and descriptor
    s = orc_system("quad2d")
    x0r = x_all.cpu().numpy().astype(np.float64)
    umax = np.abs(d.umax).astype(np.float64)[None, :]
    S_u = umax + np.abs(x0r - c.xf) @ np.abs(np.asarray(c.K, np.float64)).T          # |terms| of u_j = uf_j - sum_i K_ji e_i, and its range
    check(_ops.user_controller_eval(twin.handle, x_all), O.controller(s, desc, x0r), tol, S_u)
    fmax = max(1.0 / float(d.m), float(d.r) / float(d.I))                              # largest |f2| entry
    for integ in (_abi.EULER, _abi.RK4):
        kw = dict(task=task, integrator=integ, terminate=True)
        one, want1 = _ops.user_controller_rollout(twin.handle, x_all, 1, log_u=True, log_cost=True, **kw), O.rollout_feedback(s, desc, x0r, 1, **kw)
        assert np.array_equal(one["done_step"].cpu().numpy(), want1["done_step"])
        # x'_k = wrap(x_k + dt (f1_k + sum_j f2_kj u_j)): |terms|, with what the control's allowed error contributes through dt |f2|
        S1 = np.abs(x0r) + float(d.dt) * (np.abs(x0r).max(axis=1, keepdims=True) + float(d.g) + fmax * S_u.sum(axis=1, keepdims=True))
        S1[:, ANGLE_IDX["quad2d"]] += np.pi
        r1 = check(one["traj"][1], want1["traj"][1], tol, S1, angle_idx=ANGLE_IDX["quad2d"])
        got, want = _ops.user_controller_rollout(twin.handle, x_all, 60, log_u=True, log_cost=True, **kw), O.rollout_feedback(s, desc, x0r, 60, **kw)
        gs, ws = got["done_step"].cpu().numpy(), want["done_step"]
        keep = gs == ws
        assert keep.all() if prec == "f64" else (keep.mean() > 0.99 and np.abs(gs - ws).max() <= 1)
        P, km = 12, torch.as_tensor(keep)
        S_env = np.abs(want["traj"][:P]).max(axis=(0, 2))[None, :, None] + np.zeros((1, 1, 6))
        S_env[..., ANGLE_IDX["quad2d"]] += np.pi
        if prec == "f64":
            rp = check(got["traj"][:P, km], want["traj"][:P, keep], 1e-9, S_env[:, keep], angle_idx=ANGLE_IDX["quad2d"])
            S_all = np.abs(want["traj"]).max(axis=(0, 2))[None, :, None] + np.zeros((1, 1, 6))
            S_all[..., ANGLE_IDX["quad2d"]] += np.pi
            rh = check(got["traj"], want["traj"], 1e-5, S_all, angle_idx=ANGLE_IDX["quad2d"])
            print(f"    f64 integrator={integ}: one step {r1:.3f} of 1e-12, 12-step prefix {rp:.3f} of 1e-9, horizon {rh:.3g} of 1e-5")
        else:
            eg = abs_err(got["traj"][:P].cpu().numpy()[:, keep], want["traj"][:P, keep], ANGLE_IDX["quad2d"]) / np.broadcast_to(S_env, want["traj"][:P].shape)[:, keep]
            print(f"    f32 integrator={integ}: one step {r1:.3f} of 1e-5, 12-step prefix median err / scale {np.median(eg):.2e} (bound {tol:g})")
            assert np.median(eg) <= tol


def _wide_integrator(dt=0.01):
    from q_learning_with_hjb_amd.dynamics.linear import LinearDynamics
    return LinearDynamics(D.linear_dynamics_config(dt=dt, umin=[-100.0], umax=[100.0]))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("t0", [0.0, 0.37])
def test_the_law_sees_the_time_of_the_step(prec, t0):
    """4a. u[0] = t on Linear(2, 1): u_log[k] within 1 ulp of t0 + k dt evaluated in float64"""
    tdt, ndt, _ = DT[prec]
    d = _wide_integrator()
    law = UL.SourceLaw(d, UL.TIME_SRC)
    for integ in (_abi.EULER, _abi.RK4):
        d.integrator = integ
        out = law.rollout(torch.zeros((63, 2), dtype=tdt, device="cuda"), 60, t0=t0)
        u = out["u"][:, :, 0].cpu().numpy()
        want = t0 + np.arange(60, dtype=np.float64) * float(d.dt)
        ulp = np.spacing(np.abs(want).astype(ndt)).astype(np.float64)
        err = np.abs(u.astype(np.float64) - want[:, None]) / ulp[:, None]
        print(f"    {prec} t0={t0} integrator={integ}: max |u_log[k] - (t0 + k dt)| = {err.max():.3f} ulp")
        assert err.max() <= 1.0
        assert (u == u[:, :1]).all()
    ev = law.get_control_efforts(np.zeros((5, 2), ndt), t=1.25)
    assert ev.dtype == ndt and np.array_equal(ev, np.full((5, 1), 1.25, ndt))


def test_time_varying_law_against_a_numpy_restatement():
    """4b. u[0] = q0 sin(q1 t), float64, Euler, T = 60, against the closed loop written out in NumPy float64"""
    d = _wide_integrator()
    q0, q1, t0, T = 1.7, 2.3, 0.37, 60
    law = UL.SourceLaw(d, UL.SINE_SRC, [q0, q1])
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (257, 2))
    out = law.rollout(x0, T, t0=t0)
    A, Bm = np.asarray(d.A, np.float64), np.asarray(d.B, np.float64)
    x, traj, us = x0.copy(), [x0.copy()], []
    for k in range(T):
        u = np.full((x.shape[0], 1), q0 * np.sin(q1 * (t0 + k * float(d.dt))))
        x = x + (x @ A.T + u @ Bm.T) * float(d.dt)
        traj.append(x.copy()); us.append(u)
    tol = DT["f64"][2]
    print(f"    sine law: traj {check(out['traj'], np.stack(traj), tol):.3f} u {check(out['u'], np.stack(us), tol):.3f} of the bound (rtol = atol = {tol:g})")
    assert (out["done_step"] == T).all()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_per_environment_parameters(prec):
    """5. linear feedback about w[0..n): three targets round-robin over B = 257 == three built-in runs, one per target, row by row"""
    tdt = DT[prec][0]
    d, es = _ctrl_objects("cartpole")
    K = np.asarray(es.get_lqr_term()[0], np.float64).reshape(1, 4)
    targets = np.array([[0.0, np.pi, 0.0, 0.0], [0.5, np.pi - 0.3, 0.0, 0.1], [-1.0, 2.5, 0.2, 0.0]])
    B, T = 257, 60
    law = UL.SourceLaw(d, UL.ENV_TARGET_SRC, UL.linear_feedback_params(K, None, [0.25], True), env_params=4)
    cfg = make_vhjb_config("cartpole")
    x0 = dev(_starts(cfg, cfg.xf, 4, B, seed=5), tdt)
    w = dev(targets[np.arange(B) % 3], tdt)
    task = _abi.make_task(4, 1, cfg.Q, cfg.R, np.eye(4) * 2.0, cfg.xf, cfg.uf, cfg.obs_min, cfg.obs_max, cfg.epsilon)
    for integ, terminate in ((_abi.EULER, True), (_abi.RK4, False)):
        kw = dict(task=task, integrator=integ, terminate=terminate, log_u=True, log_cost=True)
        got = _ops.user_controller_rollout(law.handle, x0, T, w=w, **kw)
        ue = _ops.user_controller_eval(law.handle, x0, w=w)
        for j in range(3):
            desc = _abi.make_controller(_abi.CTRL_LINEAR_FEEDBACK, 4, 1, K, xf=targets[j], uf=[0.25], wrap_error=True)
            want = _ops.rollout_feedback(d.system, desc, x0, T, **kw)
            rows = torch.arange(j, B, 3, device="cuda")
            for k in ("traj", "u", "cost"):
                assert torch.equal(_bits(got[k][:, rows]), _bits(want[k][:, rows])), (prec, j, k)
            for k in ("total_cost", "x_final", "done_step"):
                assert torch.equal(got[k][rows], want[k][rows]), (prec, j, k)
            assert torch.equal(_bits(ue[rows]), _bits(_ops.controller(d.system, desc, x0)[rows]))
    with pytest.raises(ValueError, match="per-environment"):
        _ops.user_controller_rollout(law.handle, x0, T)
    # the public methods take the values as env_params, numpy in -> numpy out
    out = law.rollout(x0.cpu().numpy(), 5, env_params=w.cpu().numpy())
    same = _ops.user_controller_rollout(law.handle, x0, 5, w=w, log_u=True)
    assert isinstance(out["traj"], np.ndarray) and np.array_equal(out["traj"], same["traj"].cpu().numpy()) and np.array_equal(out["u"], same["u"].cpu().numpy())


def test_set_params_changes_the_law_without_a_new_code_object():
    """6. set_params(K2) == a freshly built controller with K2, bit for bit; the code object stays the one compiled at first use"""
    d, c = _ctrl_objects("quad2d")
    K2 = c.K * 0.5 + 0.01
    a = UL.SourceLaw(d, UL.LINEAR_FEEDBACK_SRC, UL.linear_feedback_params(c.K, c.xf, c.uf, True))
    fresh = UL.SourceLaw(d, UL.LINEAR_FEEDBACK_SRC, UL.linear_feedback_params(K2, c.xf, c.uf, True))
    cfg = make_vhjb_config("quad2d")
    x0 = dev(_starts(cfg, c.xf, 6, 257), torch.float32)
    before, code = _ops.user_controller_rollout(a.handle, x0, 60, log_u=True), a.code_object()
    handle = a.handle
    a.set_params(UL.linear_feedback_params(K2, c.xf, c.uf, True))
    assert a.handle is handle and a.code_object() == code == fresh.code_object()
    after, want = _ops.user_controller_rollout(a.handle, x0, 60, log_u=True), _ops.user_controller_rollout(fresh.handle, x0, 60, log_u=True)
    _assert_same(after, want, "set_params")
    assert not torch.equal(after["u"], before["u"])
    assert torch.equal(_bits(_ops.user_controller_eval(a.handle, x0)), _bits(_ops.user_controller_eval(fresh.handle, x0)))
    with pytest.raises(ValueError, match="compiled for"):
        a.set_params([1.0, 2.0])


@pytest.mark.parametrize("device_collection", [False, True])
def test_warm_start_takes_a_device_controller(device_collection):
    """7. VHJBController.warm_start with the cart-pole twin == with CartpoleEnergyShapingController: the same ring, records and averages"""
    from q_learning_with_hjb_amd.controller.cartpole_energy_shaping import CartpoleEnergyShapingController
    from q_learning_with_hjb_amd.controller.vhjb import VHJBController
    results = []
    for use_twin in (True, False):
        d = make_dynamics("cartpole")
        ctl = VHJBController(d, make_vhjb_config("cartpole", maximum_buffer_size=200, maximum_step=60), dtype=torch.float32, device_collection=device_collection)
        es = CartpoleEnergyShapingController(d)
        x0 = np.random.default_rng(4).uniform(-1, 1, (50, 4)) * np.array([1.0, np.pi, 1.0, 1.0])
        results.append((ctl, ctl.warm_start(UL.twin_of(es) if use_twin else es, 50, x0=x0)))
    (a, ra), (b, rb) = results
    assert ra["records"] == rb["records"] == int((ra["done_step"].long() + 1).sum()) >= 50
    assert ra["average_trajectory_cost"] == rb["average_trajectory_cost"] and ra["average_trajectory_length"] == rb["average_trajectory_length"]
    assert torch.equal(ra["done_step"], rb["done_step"])
    qa, qb = a.replay_buffer, b.replay_buffer
    assert qa.size == qb.size == 200 and qa.head == qb.head            # full (its unwritten slots would be uninitialised memory)
    assert torch.equal(_bits(qa.x), _bits(qb.x)) and torch.equal(_bits(qa.cost), _bits(qb.cost)) and torch.equal(_bits(qa.done), _bits(qb.done))


def test_every_output_is_optional():
    """8. every subset of the six outputs set to NULL leaves the others bit-equal to the all-outputs run, and the bytes after each buffer intact"""
    d, c = _ctrl_objects("cartpole")
    twin = UL.twin_of(c)
    cfg = make_vhjb_config("cartpole")
    task = _abi.make_task(4, 1, cfg.Q, cfg.R, np.eye(4) * 2.0, c.xf, cfg.uf, cfg.obs_min, cfg.obs_max, cfg.epsilon)
    B, T, GUARD = 257, 7, 64
    x0 = dev(_starts(cfg, c.xf, 4, B), torch.float32)
    sizes = dict(traj=(T + 1) * B * 4, u_log=T * B, cost=(T + 1) * B, done_step=B, total_cost=B, x_final=B * 4)
    fn = _abi.lib().hjbx_user_controller_rollout_f32

    def run(names):
        bufs = {}
        for k in names:
            if k == "done_step":
                bufs[k] = torch.full((sizes[k] + GUARD,), -77, dtype=torch.int32, device="cuda")
            else:
                bufs[k] = torch.full((sizes[k] + GUARD,), -77.0, dtype=torch.float32, device="cuda")
        p = {k: (bufs[k].data_ptr() if k in bufs else None) for k in sizes}
        _abi.check(fn(twin.handle.ptr, _abi.ref(task), _abi.RK4, _abi.ROLLOUT_TERMINATE, 0.0, T, x0.data_ptr(), None, p["traj"], p["u_log"], p["cost"],
                      p["done_step"], p["total_cost"], p["x_final"], B, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return bufs

    full = run(list(sizes))
    for k, b in full.items():
        assert (b[sizes[k]:] == -77).all() and not (b[:sizes[k]] == -77).all(), k
    names = list(sizes)
    for r in range(len(names)):                                  # every proper subset, the empty one included
        for keep in itertools.combinations(names, r):
            got = run(keep)
            for k in keep:
                assert torch.equal(got[k].view(torch.int32), full[k].view(torch.int32)), (keep, k)   # the values AND the guard elements
