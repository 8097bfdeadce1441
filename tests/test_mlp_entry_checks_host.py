"""CPU-only record of the argument checks of the six C entry points that launch the value network's matrix-core kernels:
hjbx_value_grad_f32 / hjbx_softpd_value_grad_f32, hjbx_vhjb_rollout_f32 / hjbx_softpd_rollout_f32 and hjbx_value_loss_grad_f32 /
hjbx_value_loss_adam_f32.  One table of faults serves both heads; every call carries exactly ONE fault (or B == 0) and must come back with
the status and the message below BEFORE the device is touched: the pointers are made-up integers, none of these calls may reach a launch.
The table therefore holds no case that would pass validation."""
import numpy as np
import pytest

from q_learning_with_hjb_amd import _abi

OK, EINVAL, EUNSUPPORTED = _abi.OK, _abi.EINVAL, _abi.EUNSUPPORTED
PTR = 0x7F0000100000                    # made-up "device" addresses, 64 KiB apart: aligned to everything the checks ask for (256 bytes)
NAMES = ("x", "V", "g", "traj", "u_log", "cost", "done", "resid", "done_step", "x_out", "ws", "flat",
         "W1", "b1", "W2", "b2", "W3", "b3", "w4", "b4")
ADDR = {name: PTR + 0x10000 * k for k, name in enumerate(NAMES)}

# (kind of entry point, head) -> name; the two loss entry points take the PD descriptor
ENTRY = {("vg", "pd"): "hjbx_value_grad_f32", ("vg", "soft"): "hjbx_softpd_value_grad_f32",
         ("ro", "pd"): "hjbx_vhjb_rollout_f32", ("ro", "soft"): "hjbx_softpd_rollout_f32",
         ("vlg", "pd"): "hjbx_value_loss_grad_f32", ("vla", "pd"): "hjbx_value_loss_adam_f32"}

_systems = {}


def _system(name):
    if name not in _systems:
        kind, n, m, npar = {"lin4": (_abi.SYS_LINEAR, 4, 1, 20), "lin6": (_abi.SYS_LINEAR, 6, 2, 48), "cartpole": (_abi.SYS_CARTPOLE, 4, 1, 4)}[name]
        _systems[name] = _abi.SystemHandle(kind, n, m, 0.02, -np.ones(m), np.ones(m), np.ones(npar))
    return _systems[name]


def _mlp(head, n):
    d = _abi.HjbxMlp() if head == "pd" else _abi.HjbxSoftpdMlp()
    for f in ("W1", "W2", "W3") + (("b1", "b2", "b3", "w4", "b4") if head == "soft" else ()):
        setattr(d, f, ADDR[f])
    d.h1, d.h2, d.h3, d.activation = 128, 128, 64, _abi.ACT_TANH
    for k in range(n):
        d.std[k] = 1.0
    return d


def _call(kind, head, system="lin4", edit_mlp=None, edit_task=None, **over):
    """One call of ENTRY[kind, head] with valid made-up arguments, except what `edit_mlp` / `edit_task` (functions that edit the descriptor) and
    `over` (argument name -> value) change.  -> (status, message)"""
    sys_h = _system(system)
    a = dict(ADDR, sys=sys_h.ptr, B=64, integrator=_abi.RK4, mode=_abi.RESIDUAL_NORMALISED, mlp_d=_mlp(head, sys_h.n),
             task_d=_abi.make_task(sys_h.n, sys_h.m, np.eye(sys_h.n), np.eye(sys_h.m), None, np.zeros(sys_h.n), np.zeros(sys_h.m), None, None, 0.1))
    if edit_mlp:
        edit_mlp(a["mlp_d"])
    if edit_task:
        edit_task(a["task_d"])
    a["mlp"], a["task"] = _abi.ref(a["mlp_d"]), _abi.ref(a["task_d"])
    a.update(over)
    L = _abi.lib()
    fn = getattr(L, ENTRY[kind, head])
    if kind == "vg":
        rc = fn(a["sys"], a["mlp"], a["x"], a["V"], a["g"], a["B"], None)
    elif kind == "ro":
        rc = fn(a["sys"], a["task"], a["mlp"], a["integrator"], 0, 4, 4, a["x"], a["traj"], a["u_log"], a["cost"], a["done"], a["resid"],
                a["done_step"], a["x_out"], None, a["B"], a["ws"], None)
    elif kind == "vlg":
        rc = fn(a["sys"], a["task"], a["mlp"], a["mode"], a["x"], a["cost"], a["done"], a["flat"], a["ws"], a["B"], None)
    else:
        rc = fn(a["sys"], a["task"], a["mlp"], a["mode"], a["x"], a["cost"], a["done"], None, 0.0, 1e-8, None, None, None, None, None, a["ws"],
                a["B"], None)
    return rc, _abi.last_error()


def _set(**fields):
    return lambda d: [setattr(d, k, v) for k, v in fields.items()]


def _std_zero(d):
    d.std[3] = 0.0


def _bangbang(t):
    t.law, t.target_r2 = _abi.LAW_BANGBANG, -1.0


NULLS = "x, cost, done, workspace and the weights must be non-NULL"
# (fault, keyword arguments of _call, {entry points: (status, fragment of the message)}); keys of the last dict: a kind ("vg", "ro", "vlg",
# "vla"; several joined by "+") for both heads, or "<kind>.<head>" where the heads' messages differ
FAULTS = [
    ("NULL system", dict(sys=None), {"vg": (EINVAL, "NULL system or mlp descriptor"), "ro+vlg+vla": (EINVAL, "NULL system, task or mlp descriptor")}),
    ("NULL network", dict(mlp=None), {"vg": (EINVAL, "NULL system or mlp descriptor"), "ro+vlg+vla": (EINVAL, "NULL system, task or mlp descriptor")}),
    ("NULL task", dict(task=None), {"ro+vlg+vla": (EINVAL, "NULL system, task or mlp descriptor")}),
    ("negative B", dict(B=-1), {"vg+vlg+vla": (EINVAL, "negative batch size"), "ro": (EINVAL, "negative size or step index")}),
    ("NULL x", dict(x=None), {"vg.pd": (EINVAL, "NULL x or weight pointer"), "vg.soft": (EINVAL, "NULL x"),
                              "ro.pd": (EINVAL, "x, cost, done, done_step and the weights must be non-NULL"),
                              "ro.soft": (EINVAL, "x, cost, done and done_step must be non-NULL"), "vlg+vla": (EINVAL, NULLS)}),
    ("NULL W2", dict(edit_mlp=_set(W2=None)), {"vg.pd": (EINVAL, "NULL x or weight pointer"), "vg.soft+ro.soft": (EINVAL, "NULL weight or bias pointer"),
                                          "ro.pd": (EINVAL, "x, cost, done, done_step and the weights must be non-NULL"), "vlg+vla": (EINVAL, NULLS)}),
    ("NULL b3", dict(edit_mlp=_set(b3=None)), {"vg.soft+ro.soft": (EINVAL, "NULL weight or bias pointer")}),
    ("NULL w4", dict(edit_mlp=_set(w4=None)), {"vg.soft+ro.soft": (EINVAL, "NULL weight or bias pointer")}),
    ("features", dict(edit_mlp=_set(h2=64)), {"vg+ro+vlg+vla": (EUNSUPPORTED, "features must be [128,128,64], got [128,64,64]")}),
    ("activation 7", dict(edit_mlp=_set(activation=7)), {"vg+ro+vlg+vla": (EINVAL, "unknown activation 7")}),
    ("std[3] = 0", dict(edit_mlp=_std_zero), {"vg+ro+vlg+vla": (EINVAL, "normalization_std[3] is zero")}),
    # rows of n = 4 floats are 16-byte vectors, rows of n = 6 floats 8-byte ones; u_log rows of m = 1: 4 bytes, of m = 2: 8 bytes
    ("x off 16 (n=4)", dict(x=ADDR["x"] + 8), {"vg": (EINVAL, "x / gradV must be aligned to their row vector width"),
                                               "ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width"),
                                               "vlg+vla": (EINVAL, "x must be aligned to its row vector width and workspace to 256 bytes")}),
    ("x off 8 (n=6)", dict(system="lin6", x=ADDR["x"] + 4), {"vg": (EINVAL, "x / gradV must be aligned to their row vector width"),
                                                            "ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width"),
                                                            "vlg+vla": (EINVAL, "x must be aligned to its row vector width and workspace to 256 bytes")}),
    ("gradV off 16 (n=4)", dict(g=ADDR["g"] + 8), {"vg": (EINVAL, "x / gradV must be aligned to their row vector width")}),
    ("gradV off 8 (n=6)", dict(system="lin6", g=ADDR["g"] + 4), {"vg": (EINVAL, "x / gradV must be aligned to their row vector width")}),
    ("traj off 16 (n=4)", dict(traj=ADDR["traj"] + 8), {"ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width")}),
    ("traj off 8 (n=6)", dict(system="lin6", traj=ADDR["traj"] + 4), {"ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width")}),
    ("x_out off 16 (n=4)", dict(x_out=ADDR["x_out"] + 8), {"ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width")}),
    ("u_log off 4 (m=1)", dict(u_log=ADDR["u_log"] + 2), {"ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width")}),
    ("u_log off 8 (m=2)", dict(system="lin6", u_log=ADDR["u_log"] + 4), {"ro": (EINVAL, "x / traj / x_out / u_log must be aligned to their row vector width")}),
    ("NULL workspace", dict(ws=None), {"ro": (EINVAL, "workspace must be a 16-byte aligned device buffer"), "vlg+vla": (EINVAL, NULLS)}),
    ("workspace off", dict(ws=ADDR["ws"] + 8), {"ro": (EINVAL, "workspace must be a 16-byte aligned device buffer"),
                                                "vlg+vla": (EINVAL, "x must be aligned to its row vector width and workspace to 256 bytes")}),
    ("workspace off 256", dict(ws=ADDR["ws"] + 128), {"vlg+vla": (EINVAL, "x must be aligned to its row vector width and workspace to 256 bytes")}),
    ("integrator 9", dict(integrator=9), {"ro": (EINVAL, "unknown integrator 9")}),
    ("ZOH, cart-pole", dict(system="cartpole", integrator=_abi.ZOH), {"ro": (EUNSUPPORTED, "HJBX_ZOH exists for LINEAR systems only")}),
    # (check_task's messages are the one exception to "starts with the entry point's name": they name the law, for every caller)
    ("bang-bang, target_r2 < 0", dict(edit_task=_bangbang), {"ro+vlg+vla": (EINVAL, "bang-bang law: target_r2 must be >= 0, got -1")}),
]


def _cases():
    out = []
    for fault, kw, expect in FAULTS:
        for keys, (status, fragment) in expect.items():
            for key in keys.split("+"):
                kind, _, head = key.partition(".")
                for h in ((head,) if head else ("pd", "soft")):
                    if (kind, h) in ENTRY:
                        out.append(pytest.param(kind, h, kw, status, fragment, id=f"{ENTRY[kind, h]}-{fault}"))
    return out


CASES = _cases()


def test_the_table_covers_every_entry_point_and_holds_one_case_per_fault():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for name in ENTRY.values():
        assert sum(i.startswith(name + "-") for i in ids) >= 12, name


@pytest.mark.parametrize("kind, head, kw, status, fragment", CASES)
def test_fault_is_rejected_before_the_device(kind, head, kw, status, fragment):
    rc, msg = _call(kind, head, **kw)
    assert rc == status, (rc, msg)
    who = ENTRY[kind, head]
    assert msg.startswith(fragment if fragment.startswith("bang-bang law") else who + ": "), msg
    assert fragment in msg, msg


@pytest.mark.parametrize("kind, head", [k for k in ENTRY if k[0] in ("vg", "ro")])
def test_empty_batch_is_ok(kind, head):
    rc, msg = _call(kind, head, B=0)
    assert rc == OK, msg
