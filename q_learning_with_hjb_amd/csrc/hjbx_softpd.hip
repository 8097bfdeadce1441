// hjbx_softpd.hip -- the soft-PD value network of the notebooks (SoftPDValueApproximator: examples/cartpole_balancing.ipynb cells 6, 11-12,
// drone_hovering.ipynb, double_integrator_optimal_time.ipynb, 10D_quadcopte.ipynb) on the matrix cores:
//
//   e = wrap(x - xf); z = (e - mean)/std; h1 = act(z W1 + b1); h2 = act(h1 W2 + b2); h3 = act(h2 W3 + b3)
//   V = h3 . w4 + b4
//   dV/dx = ((((w4 . act'(a3)) W3') . act'(a2)) W2' . act'(a1)) W1' / std
//
// The kernels are those of hjbx_mlp.hip (hjbx_mlp_kernels.hpp) with the soft-PD head (MlpHeadSoft): the same three MFMA chains forward and
// backward, the biases initialise the accumulators, b1 / b2 / b3 / w4 / b4 sit in LDS next to the weights.  float32 MFMA only
// (HJBX_OPT_MLP_ARITHMETIC does not apply).  Compiled once per activation (-DHJBX_SOFTPD_ACT = hjbx_activation: 0 relu, 1 tanh, 2 sin); the
// relu object also carries the two C entry points, which validate and hand over to the object of the requested activation.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"
#include "hjbx_host.hpp"
#include "hjbx_mlp_kernels.hpp"
#include "hjbx_mlp_host.hpp"

using namespace hjbx;

#ifndef HJBX_SOFTPD_ACT
#error "compile hjbx_softpd.hip with -DHJBX_SOFTPD_ACT=0 (relu + the C entry points), =1 (tanh) and =2 (sin)"
#endif
static constexpr int kAct = HJBX_SOFTPD_ACT;
static_assert(kAct == HJBX_ACT_RELU || kAct == HJBX_ACT_TANH || kAct == HJBX_ACT_SIN, "soft-PD kernels exist for relu, tanh and sin");
#define HJBX_SOFTPD_CAT2(a, b) a##b
#define HJBX_SOFTPD_CAT(a, b) HJBX_SOFTPD_CAT2(a, b)
#define HJBX_SOFTPD_SYM(name) HJBX_SOFTPD_CAT(name, HJBX_SOFTPD_ACT)
#define HJBX_HIDDEN __attribute__((visibility("hidden")))
static constexpr int kWaves = 8;   // launch shape of hjbx_mlp.hip: one tile of 32 environments per wave, 8 waves per workgroup, one per CU

#define HJBX_SOFTPD_VG_ARGS const hjbx_system*, const hjbx_softpd_mlp*, const float*, float*, float*, int64_t, void*
#define HJBX_SOFTPD_RO_ARGS                                                                                                                 \
    const hjbx_system*, const hjbx_task*, const hjbx_softpd_mlp*, int, int, int, int, const float*, float*, float*, float*, float*, float*, \
        int32_t*, float*, const int32_t*, int64_t, void*, void*
HJBX_HIDDEN int hjbx_softpd_value_grad_act0(HJBX_SOFTPD_VG_ARGS);
HJBX_HIDDEN int hjbx_softpd_value_grad_act1(HJBX_SOFTPD_VG_ARGS);
HJBX_HIDDEN int hjbx_softpd_value_grad_act2(HJBX_SOFTPD_VG_ARGS);
HJBX_HIDDEN int hjbx_softpd_rollout_act0(HJBX_SOFTPD_RO_ARGS);
HJBX_HIDDEN int hjbx_softpd_rollout_act1(HJBX_SOFTPD_RO_ARGS);
HJBX_HIDDEN int hjbx_softpd_rollout_act2(HJBX_SOFTPD_RO_ARGS);

template <int N> static MlpP<N> softpd_params(const hjbx_softpd_mlp* mlp) {
    return make_mlp_params<N>(mlp->mean, mlp->std, mlp->xf, 0.0);   // (no eps |e|^2 term in this network)
}

static MlpHeadSoft softpd_head(const hjbx_softpd_mlp* mlp) {
    return MlpHeadSoft{(const float*)mlp->b1, (const float*)mlp->b2, (const float*)mlp->b3, (const float*)mlp->w4, (const float*)mlp->b4};
}

template <typename S>
static int launch_softpd_value_grad(S sys, const hjbx_softpd_mlp* mlp, const float* x, float* V, float* g, int64_t B, void* st) {
    constexpr int N = S::N;
    int64_t ngroups = 0, grid = 0;
    if (int rc = mlp_value_grad_grid(B, 1, &ngroups, &grid, "hjbx_softpd_value_grad_f32")) return rc;
    hipLaunchKernelGGL((k_value_grad_mfma<S, 1, kWaves, kAct, 0, MlpHeadSoft>), dim3((unsigned)grid), dim3(kWaves * 64), 0, (hipStream_t)st, sys,
                       softpd_params<N>(mlp), (const float*)mlp->W1, (const float*)mlp->W2, (const float*)mlp->W3, x, V, g, B, ngroups,
                       softpd_head(mlp));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "hjbx_softpd_value_grad_f32: %s", hipGetErrorString(e));
    return HJBX_OK;
}

// system kind -> instantiation of this object's activation (the same seven as hjbx_value_grad_f32: V does not depend on m)
int HJBX_SOFTPD_SYM(hjbx_softpd_value_grad_act)(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* V, float* g, int64_t B,
                                                void* stream) {
    switch (sys->kind) {
    case HJBX_SYS_LINEAR:
        if (sys->n == 2) { Linear<float, 2, 1> l{}; return launch_softpd_value_grad(l, mlp, x, V, g, B, stream); }
        if (sys->n == 4) { Linear<float, 4, 1> l{}; return launch_softpd_value_grad(l, mlp, x, V, g, B, stream); }
        if (sys->n == 6) { Linear<float, 6, 2> l{}; return launch_softpd_value_grad(l, mlp, x, V, g, B, stream); }
        break;
    case HJBX_SYS_CARTPOLE: { Cartpole<float> c{}; return launch_softpd_value_grad(c, mlp, x, V, g, B, stream); }
    case HJBX_SYS_ACROBOT: { Acrobot<float> a{}; return launch_softpd_value_grad(a, mlp, x, V, g, B, stream); }
    case HJBX_SYS_QUAD2D: { Quad2D<float> q{}; return launch_softpd_value_grad(q, mlp, x, V, g, B, stream); }
    case HJBX_SYS_NEARHOVER: { NearHover<float> q{}; return launch_softpd_value_grad(q, mlp, x, V, g, B, stream); }
    }
    return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_softpd_value_grad_f32: no kernel for system kind %d with n=%d", sys->kind, sys->n);
}

template <typename S>
static int launch_softpd_rollout(const hjbx_system* sysh, S sys, const hjbx_task* task, const hjbx_softpd_mlp* mlp, int integrator, int t_first,
                                 int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                                 int32_t* done_step, float* x_out, const int32_t* order, int64_t B, void* workspace, void* st) {
    constexpr int N = S::N, M = S::M;
    const MlpP<N> p = softpd_params<N>(mlp);
    const auto tk = make_task<float, N, M>(task);
    const auto lim = make_limits<float, M>(sysh);
    RolloutOut<N, M> o{traj, u_log, cost, done, resid, done_step, x_out};
    int64_t ngroups = 0, grid = 0;   // as hjbx_vhjb_rollout_f32, schedule and test hook included
    int sched = 0;
    if (int rc = mlp_rollout_grid(B, &ngroups, &grid, &sched, "hjbx_softpd_rollout_f32")) return rc;
    const float *W1 = (const float*)mlp->W1, *W2 = (const float*)mlp->W2, *W3 = (const float*)mlp->W3;
    auto launch = [&](auto integ) {
        hipLaunchKernelGGL((k_vhjb_rollout_mfma<decltype(integ)::value, S, kWaves, kAct, 0, MlpHeadSoft>), dim3((unsigned)grid), dim3(kWaves * 64), 0,
                           (hipStream_t)st, sys, p, tk, lim, W1, W2, W3, t_first, n_steps, T_max, x, order, o, B, ngroups, (unsigned*)workspace, sched,
                           softpd_head(mlp));
    };
    if (integrator == HJBX_EULER) launch(std::integral_constant<int, 0>{});
    else if (integrator == HJBX_RK4) launch(std::integral_constant<int, 1>{});
    else if constexpr (S::kHasZoh) launch(std::integral_constant<int, 2>{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "hjbx_softpd_rollout_f32: %s", hipGetErrorString(e));
    return HJBX_OK;
}

int HJBX_SOFTPD_SYM(hjbx_softpd_rollout_act)(const hjbx_system* sys, const hjbx_task* task, const hjbx_softpd_mlp* mlp, int integrator, int t_first,
                                             int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                                             int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace, void* stream) {
    int rc = HJBX_EUNSUPPORTED;
    const bool ok = with_system<float>(sys, [&](auto S) {
        using SS = decltype(S);
        if constexpr (SS::N % 2 == 0)
            rc = launch_softpd_rollout<SS>(sys, S, task, mlp, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out,
                                           env_order, B, workspace, stream);
    });
    if (!ok || rc == HJBX_EUNSUPPORTED)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_softpd_rollout_f32: no kernel for system kind %d with n=%d m=%d", sys->kind, sys->n, sys->m);
    return rc;
}

#if HJBX_SOFTPD_ACT == 0
static hjbx_user_net user_net(const hjbx_softpd_mlp* mlp) {
    return hjbx_user_net{1, mlp->activation, mlp->mean, mlp->std, mlp->xf, 0.0, (const float*)mlp->W1, (const float*)mlp->W2, (const float*)mlp->W3,
                         (const float*)mlp->b1, (const float*)mlp->b2, (const float*)mlp->b3, (const float*)mlp->w4, (const float*)mlp->b4};
}

// the checks both entry points share: descriptor, features, activation, normalisation, and the handle (built-in systems, and user-defined
// ones that asked for the matrix-core kernels: hjbx_system_enable_matrix_cores)
static int check_softpd(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const char* who) {
    if (!mlp->W1 || !mlp->b1 || !mlp->W2 || !mlp->b2 || !mlp->W3 || !mlp->b3 || !mlp->w4 || !mlp->b4)
        return hjbx_set_error(HJBX_EINVAL, "%s: NULL weight or bias pointer", who);
    if (sys->kind == HJBX_SYS_USER && !hjbx_user_matrix_cores(sys))
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the matrix-core kernels exist for the built-in systems only", who);
    if (mlp->h1 != kH1 || mlp->h2 != kH2 || mlp->h3 != kH3)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: features must be [128,128,64], got [%d,%d,%d]", who, mlp->h1, mlp->h2, mlp->h3);
    if (mlp->activation != HJBX_ACT_RELU && mlp->activation != HJBX_ACT_TANH && mlp->activation != HJBX_ACT_SIN)
        return hjbx_set_error(HJBX_EINVAL, "%s: unknown activation %d", who, mlp->activation);
    for (int k = 0; k < sys->n; ++k)
        if (!(mlp->std[k] != 0.0)) return hjbx_set_error(HJBX_EINVAL, "%s: normalization_std[%d] is zero", who, k);
    return HJBX_OK;
}

extern "C" int hjbx_softpd_value_grad_f32(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* V, float* g, int64_t B,
                                          void* stream) {
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_value_grad_f32: NULL system or mlp descriptor");
    if (B < 0) return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_value_grad_f32: negative batch size");
    if (B == 0 || (!V && !g)) return HJBX_OK;
    if (!x) return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_value_grad_f32: NULL x");
    if (int rc = check_softpd(sys, mlp, "hjbx_softpd_value_grad_f32")) return rc;
    const size_t row = (size_t)sys->n * sizeof(float);
    const uintptr_t am = (row % 16 == 0) ? 15u : 7u;
    if ((reinterpret_cast<uintptr_t>(x) & am) || (g && (reinterpret_cast<uintptr_t>(g) & am)))
        return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_value_grad_f32: x / gradV must be aligned to their row vector width");
    if (sys->kind == HJBX_SYS_USER) {
        const hjbx_user_net net = user_net(mlp);
        return hjbx_user_value_grad(sys, &net, x, V, g, B, stream, "hjbx_softpd_value_grad_f32");
    }
    auto* fn = mlp->activation == HJBX_ACT_TANH ? hjbx_softpd_value_grad_act1 : mlp->activation == HJBX_ACT_SIN ? hjbx_softpd_value_grad_act2
                                                                                                               : hjbx_softpd_value_grad_act0;
    return fn(sys, mlp, x, V, g, B, stream);
}

extern "C" int hjbx_softpd_rollout_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_softpd_mlp* mlp, int integrator, int t_first,
                                       int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                                       int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace, void* stream) {
    if (!sys || !task || !mlp) return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_rollout_f32: NULL system, task or mlp descriptor");
    if (int rc = check_task(task)) return rc;
    if (B < 0 || n_steps < 0 || t_first < 0 || T_max < 0) return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_rollout_f32: negative size or step index");
    if (int rc = check_integrator(sys, integrator, "hjbx_softpd_rollout_f32")) return rc;
    if (B == 0) return HJBX_OK;
    if (!x || !cost || !done || !done_step)
        return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_rollout_f32: x, cost, done and done_step must be non-NULL");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_rollout_f32: workspace must be a 16-byte aligned device buffer of hjbx_rollout_workspace_bytes() zero-filled bytes");
    if (int rc = check_softpd(sys, mlp, "hjbx_softpd_rollout_f32")) return rc;
    const size_t row = (size_t)sys->n * sizeof(float);
    const uintptr_t am = (row % 16 == 0) ? 15u : 7u;
    const size_t urow = (size_t)sys->m * sizeof(float);
    const uintptr_t um = (urow % 16 == 0) ? 15u : (urow % 8 == 0) ? 7u : 3u;
    if ((reinterpret_cast<uintptr_t>(x) & am) || (traj && (reinterpret_cast<uintptr_t>(traj) & am)) ||
        (x_out && (reinterpret_cast<uintptr_t>(x_out) & am)) || (u_log && (reinterpret_cast<uintptr_t>(u_log) & um)))
        return hjbx_set_error(HJBX_EINVAL, "hjbx_softpd_rollout_f32: x / traj / x_out / u_log must be aligned to their row vector width");
    if (sys->kind == HJBX_SYS_USER) {
        const hjbx_user_net net = user_net(mlp);
        return hjbx_user_rollout(sys, task, &net, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B,
                                 workspace, stream, "hjbx_softpd_rollout_f32");
    }
    auto* fn = mlp->activation == HJBX_ACT_TANH ? hjbx_softpd_rollout_act1 : mlp->activation == HJBX_ACT_SIN ? hjbx_softpd_rollout_act2
                                                                                                            : hjbx_softpd_rollout_act0;
    return fn(sys, task, mlp, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B, workspace, stream);
}
#endif
