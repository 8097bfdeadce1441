"""CPU-only tests of user-defined control laws (hjbx_user_controller_*, DeviceController, csrc/hjbx_user_controller_kernels.hpp): the C
surface and its registration, the run-time compile of twin laws for a built-in, a linear and a user-defined system and what the code
objects hold, compile errors, every refusal of the entry points before any launch, and the lifetime of a controller whose system handle
is destroyed first.  No compute call touches a GPU."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import user_laws as UL
from conftest import ROOT, make_dynamics
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller import DeviceController
from q_learning_with_hjb_amd.controller.controller_basic import Controller
from q_learning_with_hjb_amd.controller.time_optimal import DoubleIntegratorTimeOptimalController
from test_gpu_parity import _ctrl_objects
from test_gpu_user_system import UserQuad2D

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
META = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                  r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
KERNELS = sorted(f"hjbx_uc_{k}_{s}" for k in ("control", "rollout_i0", "rollout_i1") for s in ("f32", "f64"))
NEW_SYMBOLS = ("hjbx_user_controller_create", "hjbx_user_controller_destroy", "hjbx_user_controller_set_params", "hjbx_user_controller_code_object",
               "hjbx_user_controller_eval_f32", "hjbx_user_controller_eval_f64", "hjbx_user_controller_rollout_f32", "hjbx_user_controller_rollout_f64")


def kernel_metadata(code, tmp_path, tag):
    assert code[:4] == b"\x7fELF"
    path = tmp_path / f"{tag}.co"
    path.write_bytes(code)
    notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    return META.findall(notes)


def test_new_symbols_are_declared_exported_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    L = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None
        decl = re.search(r"/\* \((.*)\) \*/\n(?:int|void|size_t) " + name + r"\(", hdr)
        assert decl and "controller/controller_basic.py:1-5" in decl.group(1), f"{name}: the declaration cites the reference lines it replaces"
        if "rollout" in name:
            assert "controller/vhjb.py:171-193" in decl.group(1)
        assert hdr.index("#undef HJBX_DECLARE") < decl.start()                                  # plain declarations, outside the typed macro
    assert re.search(r"#define HJBX_VERSION 112\b", hdr) and L.hjbx_version() == 112
    assert re.search(r"#define HJBX_HAS_USER_CONTROLLER 1\b", hdr)
    assert "typedef struct hjbx_user_controller hjbx_user_controller;" in hdr
    # the device unit is embedded into hjbx_user.hip (whose host code compiles it) and is a dependency of the build
    assert "hjbx_user_controller_kernels.hpp" in _abi._HEADERS and any(u[0] == "hjbx_user.hip" for u in _abi._UNITS)
    user = open(os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc", "hjbx_user.hip")).read()
    assert 'X(hjbx_src_user_controller, "hjbx_user_controller_kernels.hpp", "hjbx_user_controller_kernels.hpp")' in user
    assert user.count("int compile_unit(") == 1                                                # widened, not copied
    assert (_abi.LAW_MAX_PARAMS, _abi.LAW_MAX_ENV_PARAMS) == (128, 32)
    assert issubclass(DeviceController, Controller)


def _twins():
    dq, cq = _ctrl_objects("quad2d")
    return {"cartpole": lambda: UL.twin_of(_ctrl_objects("cartpole")[1]),
            "linear21": lambda: UL.twin_of(_ctrl_objects("linear")[1]),
            "user_quad2d": lambda: UL.twin_of(cq, UserQuad2D(D.quadrotors2d_dynamics_config()))}


@pytest.mark.parametrize("name", ["cartpole", "linear21", "user_quad2d"])
def test_twin_laws_compile_without_a_device(name, tmp_path):
    """the code object is an ELF with exactly the six hjbx_uc_* kernels, none with scratch or spilled VGPRs; code_object() does not compile twice"""
    twin = _twins()[name]()
    assert twin._handle is None                                                 # built at first use
    t0 = time.perf_counter()
    code = twin.code_object()
    t_compile = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert twin.code_object() == code and time.perf_counter() - t0 < 0.1
    kernels = kernel_metadata(code, tmp_path, name)
    assert sorted(k[0] for k in kernels) == KERNELS
    for kname, private, sgpr_spill, vgprs, vgpr_spill in kernels:
        print(f"    {name} {kname}: {vgprs} VGPRs, {sgpr_spill} spilled SGPRs, {private} bytes of scratch")
        assert int(private) == 0 and int(vgpr_spill) == 0, f"{kname}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
    print(f"    {name}: compiled in {t_compile:.2f} s, {len(code)} bytes")
    if name == "user_quad2d":                                                   # a code object of its own: the system's streaming object is untouched
        stream = kernel_metadata(twin.dynamics.system.code_object("streaming"), tmp_path, "streaming")
        assert len(stream) == 32 and all(k[0].startswith("hjbx_u_") for k in stream)
    # parameters can be replaced without a recompile; their number is part of the compiled struct
    handle = twin.handle
    twin.set_params(np.asarray(handle.params) * 0.5)
    assert twin.handle is handle and twin.code_object() == code
    with pytest.raises(ValueError, match="compiled for"):
        twin.set_params([1.0])


def test_compile_errors_and_what_survives_them():
    d = make_dynamics("cartpole")
    good = UL.twin_of(_ctrl_objects("cartpole")[1], d)
    code = good.code_object()
    bad = UL.SourceLaw(d, "HJBX_DEV void control(const S& sys, const Limits<T, S::M>& lim, const T* x, const T* w, T t, T* u) const { u[0] = undeclared_gain * x[0]; }\n")
    with pytest.raises(ValueError, match="undeclared_gain") as e:
        bad.code_object()
    assert "compiler log" in str(e.value) and "undeclared_gain" in _abi.compile_log()
    # the dynamics handle and the controller built before keep working
    n, m = C.c_int(), C.c_int()
    assert _abi.lib().hjbx_dims(d.system.ptr, C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (4, 1)
    assert good.code_object() == code
    good.set_params(good.handle.params)
    assert UL.twin_of(_ctrl_objects("cartpole")[1], d).code_object() == code   # the same source compiles to the same bytes
    # a law without `reached` asked to stop at the target; a law that says reached=True without defining it
    with pytest.raises(ValueError, match="reached"):
        good.rollout(np.zeros((3, 4)), 5, stop_at_target=True)
    with pytest.raises(ValueError, match="reached"):
        UL.SourceLaw(d, UL.CARTPOLE_ES_SRC, np.zeros(13), reached=True).code_object()
    # a controller without a law
    with pytest.raises(NotImplementedError, match="device_source"):
        DeviceController(d).code_object()
    with pytest.raises(NotImplementedError, match="device_source"):
        DeviceController(d).get_control_efforts(np.zeros(4))
    # the limits of the argument structs
    with pytest.raises(ValueError, match="0..128"):
        UL.SourceLaw(d, UL.TIME_SRC, np.zeros(129)).code_object()
    with pytest.raises(ValueError, match="0..32"):
        UL.SourceLaw(d, UL.TIME_SRC, env_params=33).code_object()
    assert UL.SourceLaw(d, UL.TIME_SRC, np.zeros(128), env_params=32).code_object()[:4] == b"\x7fELF"
    # a LINEAR handle whose (n, m) the library has no kernels for
    lin = _abi.SystemHandle(_abi.SYS_LINEAR, 3, 1, 0.02, [-1], [1], np.zeros(12))
    h = C.c_void_p()
    rc = _abi.lib().hjbx_user_controller_create(lin.ptr, UL.TIME_SRC.encode(), None, 0, 0, 0, C.byref(h))
    assert rc == _abi.EUNSUPPORTED and not h.value
    assert _abi.lib().hjbx_user_controller_create(None, UL.TIME_SRC.encode(), None, 0, 0, 0, C.byref(h)) == _abi.EINVAL
    assert _abi.lib().hjbx_user_controller_create(d.system.ptr, None, None, 0, 0, 0, C.byref(h)) == _abi.EINVAL


def _args(handle, n, m, **kw):
    """arguments of the rollout entry points with dummy (non-NULL, aligned, never dereferenced) pointers except where `kw` says otherwise"""
    task = _abi.make_task(n, m, np.eye(n), np.eye(m), None, np.zeros(n), np.zeros(m), None, None, 0.0)
    a = dict(ctl=handle.ptr, task=_abi.ref(task), integrator=_abi.EULER, flags=0, t0=0.0, T_steps=5, x0=0x40000, w=0x50000, traj=0x60000, u_log=0x70000,
             cost=0x80000, done_step=0x90000, total_cost=0xa0000, x_final=0xb0000, B=7, stream=None, _keep=task)
    a.update(kw)
    return a


def _rollout(sfx, handle, n, m, **kw):
    a = _args(handle, n, m, **kw)
    return getattr(_abi.lib(), f"hjbx_user_controller_rollout_{sfx}")(a["ctl"], a["task"], a["integrator"], a["flags"], a["t0"], a["T_steps"], a["x0"], a["w"],
                                                                      a["traj"], a["u_log"], a["cost"], a["done_step"], a["total_cost"], a["x_final"], a["B"],
                                                                      a["stream"])


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_entry_points_refuse_bad_arguments_before_any_launch(sfx):
    """every refusal comes from the host-side checks: with the dummy pointers of _args a launch would fault (or, here, fail for want of a
    device) instead"""
    d = make_dynamics("quad2d")                                                # n = 6, m = 2: rows of 24 / 8 bytes (f32), 48 / 16 (f64)
    K = np.zeros((2, 6))
    plain = UL.SourceLaw(d, UL.LINEAR_FEEDBACK_SRC, UL.linear_feedback_params(K)).handle
    env = UL.SourceLaw(d, UL.ENV_TARGET_SRC, UL.linear_feedback_params(K), env_params=6).handle
    eval_fn = getattr(_abi.lib(), f"hjbx_user_controller_eval_{sfx}")
    for ctl, w in ((plain, None), (env, 0x50000)):
        bad = [dict(ctl=None), dict(B=-1), dict(x0=None), dict(x0=0x40004), dict(traj=0x60004), dict(u_log=0x70004), dict(x_final=0xb0004),
               dict(flags=_abi.ROLLOUT_STOP_AT_TARGET), dict(flags=4), dict(integrator=7), dict(integrator=-1), dict(task=None, flags=_abi.ROLLOUT_TERMINATE),
               dict(task=None), dict(task=None, cost=None), dict(task=None, total_cost=None), dict(T_steps=-1)]
        for kw in bad:
            assert _rollout(sfx, ctl, 6, 2, **dict(dict(w=w), **kw)) == _abi.EINVAL, kw
        assert _rollout(sfx, ctl, 6, 2, w=w, integrator=_abi.ZOH) == _abi.EUNSUPPORTED and "HJBX_ZOH" in _abi.last_error()
        assert _rollout(sfx, ctl, 6, 2, w=w, B=0) == _abi.OK                   # nothing to do: HJBX_OK without a launch
        assert eval_fn(ctl.ptr, 0x40000, w, 0.0, 0x70000, 0, None) == _abi.OK
        for x, u, B in ((None, 0x70000, 3), (0x40000, None, 3), (0x40004, 0x70000, 3), (0x40000, 0x70004, 3), (0x40000, 0x70000, -1)):
            assert eval_fn(ctl.ptr, x, w, 0.0, u, B, None) == _abi.EINVAL
        assert eval_fn(None, 0x40000, w, 0.0, 0x70000, 3, None) == _abi.EINVAL
    # w: NULL if and only if the law reads no per-environment values; aligned like every row
    assert _rollout(sfx, env, 6, 2, w=None) == _abi.EINVAL and "per-environment" in _abi.last_error()
    assert _rollout(sfx, env, 6, 2, w=0x50004) == _abi.EINVAL
    assert eval_fn(env.ptr, 0x40000, None, 0.0, 0x70000, 3, None) == _abi.EINVAL
    bad_task = _abi.make_task(6, 2, np.eye(6), np.eye(2), None, np.zeros(6), np.zeros(2), None, None, 0.0, law=9)
    assert _rollout(sfx, plain, 6, 2, w=None, task=_abi.ref(bad_task)) == _abi.EINVAL
    # the bang-bang twin defines `reached`: the flag passes the checks (and the call then ends for want of a device, or launches on one)
    import torch
    if not torch.cuda.is_available():
        di = UL.twin_of(DoubleIntegratorTimeOptimalController(make_dynamics("linear")))
        assert _rollout(sfx, di.handle, 2, 1, w=None, flags=_abi.ROLLOUT_STOP_AT_TARGET) == _abi.ENODEVICE


def test_compute_calls_need_a_device():
    import torch
    if torch.cuda.is_available():
        return                                       # (with a device the same calls are tested in test_gpu_user_controller.py)
    twin = UL.twin_of(_ctrl_objects("cartpole")[1])
    with pytest.raises(RuntimeError, match="no HIP device"):
        twin.get_control_efforts(np.zeros(4))
    with pytest.raises(RuntimeError, match="no HIP device"):
        twin.rollout(np.zeros((3, 4)), 10)
    rc = _rollout("f32", twin.handle, 4, 1, w=None)
    assert rc == _abi.ENODEVICE and "no HIP device" in _abi.last_error()
    with pytest.raises(RuntimeError, match="no HIP device"):
        _abi.check(rc)


def test_the_controller_outlives_its_system_handle():
    """the library copies what the law needs from the system handle (include/hjbx.h): destroying the system first, then using and destroying
    the controller, touches no freed memory (the same sequence runs under AddressSanitizer as a stand-alone C program)"""
    L = _abi.lib()
    for make in (lambda: UserQuad2D(D.quadrotors2d_dynamics_config()), lambda: make_dynamics("quad2d")):
        d = make()
        c = UL.SourceLaw(d, UL.LINEAR_FEEDBACK_SRC, UL.linear_feedback_params(np.ones((2, 6))))
        handle, code = c.handle, c.code_object()
        sysh = d.system
        L.hjbx_system_destroy(sysh.ptr)
        sysh._h = None                               # (the Python owner must not free it a second time)
        assert c.code_object() == code
        c.set_params(handle.params * 2)
        assert _rollout("f64", handle, 6, 2, w=None, x0=0x40008) == _abi.EINVAL      # the checks read the controller's copy of n, m
        assert _rollout("f64", handle, 6, 2, w=None, B=0) == _abi.OK
        L.hjbx_user_controller_destroy(handle.ptr)
        handle._h = None
