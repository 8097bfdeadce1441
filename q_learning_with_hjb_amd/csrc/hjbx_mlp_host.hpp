// hjbx_mlp_host.hpp -- the one host path between a C entry point and a launch of the value network's matrix-core kernels (hjbx_mlp.hip,
// hjbx_softpd.hip, hjbx_hessian.hip, hjbx_softpd_hessian.hip, hjbx_train.hip, hjbx_train_coop.hip, and hjbx_user.hip for a user-defined
// system): the network of either head as one
// descriptor (hjbx_net), the argument checks of the entry points, the normalisation constants as the kernels take them, the persistent
// grids, and -- templated on the head -- one launcher and one system dispatcher per kernel.  Not part of the ABI.
#pragma once
#include <type_traits>

#include "hjbx_host.hpp"
#include "hjbx_mlp_kernels.hpp"
#include "hjbx_hessian_kernels.hpp"

// ---- the network descriptor --------------------------------------------------------------------------------------------------------
inline hjbx_net make_net(const hjbx_mlp* mlp) {
    return hjbx_net{0, mlp->activation, mlp->h1, mlp->h2, mlp->h3, mlp->mean, mlp->std, mlp->xf, mlp->eps_scalar, (const float*)mlp->W1,
                    (const float*)mlp->W2, (const float*)mlp->W3, nullptr, nullptr, nullptr, nullptr, nullptr};
}
inline hjbx_net make_net(const hjbx_softpd_mlp* mlp) {   // (no eps |e|^2 term in this network)
    return hjbx_net{1, mlp->activation, mlp->h1, mlp->h2, mlp->h3, mlp->mean, mlp->std, mlp->xf, 0.0, (const float*)mlp->W1, (const float*)mlp->W2,
                    (const float*)mlp->W3, (const float*)mlp->b1, (const float*)mlp->b2, (const float*)mlp->b3, (const float*)mlp->w4, (const float*)mlp->b4};
}

// mean, 1/std, xf and eps_scalar of a network descriptor, rounded to float once per call
template <int N> inline MlpP<N> make_mlp_params(const hjbx_net& net) {
    MlpP<N> p;
    for (int k = 0; k < N; ++k) { p.mean[k] = (float)net.mean[k]; p.istd[k] = (float)(1.0 / net.std[k]); p.xf[k] = (float)net.xf[k]; }
    p.eps_s = (float)net.eps_scalar;
    return p;
}

// the head's by-value kernel argument
template <typename Head> inline Head make_head(const hjbx_net& net) {
    if constexpr (std::is_same<Head, MlpHeadSoft>::value) return MlpHeadSoft{net.b1, net.b2, net.b3, net.w4, net.b4};
    else return MlpHeadPd{};
}

// ---- argument checks ---------------------------------------------------------------------------------------------------------------
// The order of the checks is that of the PD entry points (hjbx_value_grad_f32, hjbx_vhjb_rollout_f32); the messages are each head's own.
static constexpr int kEmptyCall = 1;   // returned by the entry-point checks for a call with nothing to compute: the caller returns HJBX_OK

inline int check_features(const char* who, const hjbx_net& net) {
    if (net.h1 != kH1 || net.h2 != kH2 || net.h3 != kH3)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: features must be [128,128,64], got [%d,%d,%d]", who, net.h1, net.h2, net.h3);
    if (net.activation != HJBX_ACT_RELU && net.activation != HJBX_ACT_TANH && net.activation != HJBX_ACT_SIN)
        return hjbx_set_error(HJBX_EINVAL, "%s: unknown activation %d", who, net.activation);
    return HJBX_OK;
}
inline int check_std(const char* who, const hjbx_net& net, int n) {
    for (int k = 0; k < n; ++k)
        if (!(net.std[k] != 0.0)) return hjbx_set_error(HJBX_EINVAL, "%s: normalization_std[%d] is zero", who, k);
    return HJBX_OK;
}
// state rows (x, gradV, traj, x_out) are read in pairs of floats at least; control rows (u_log) may be single floats
inline bool state_rows_aligned(const void* p, const hjbx_system* sys) { return aligned_rows(p, (size_t)sys->n * sizeof(float), 7u); }
// soft-PD head: its five extra pointers, and a user handle must have asked for the kernels; then features and activation for both heads
inline int check_net(const char* who, const hjbx_system* sys, const hjbx_net& net) {
    if (net.soft) {
        if (!net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3 || !net.w4 || !net.b4)
            return hjbx_set_error(HJBX_EINVAL, "%s: NULL weight or bias pointer", who);
        if (sys->kind == HJBX_SYS_USER && !hjbx_user_matrix_cores(sys))
            return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the matrix-core kernels exist for the built-in systems only", who);
    }
    return check_features(who, net);
}

// hjbx_value_grad_f32 / hjbx_softpd_value_grad_f32 after their NULL-descriptor check
inline int check_value_grad(const char* who, const hjbx_system* sys, const hjbx_net& net, const float* x, const float* V, const float* g, int64_t B) {
    if (B < 0) return hjbx_set_error(HJBX_EINVAL, "%s: negative batch size", who);
    if (B == 0 || (!V && !g)) return kEmptyCall;
    if (net.soft ? !x : (!x || !net.W1 || !net.W2 || !net.W3))
        return hjbx_set_error(HJBX_EINVAL, net.soft ? "%s: NULL x" : "%s: NULL x or weight pointer", who);
    if (int rc = check_net(who, sys, net)) return rc;
    if (!state_rows_aligned(x, sys) || (g && !state_rows_aligned(g, sys)))
        return hjbx_set_error(HJBX_EINVAL, "%s: x / gradV must be aligned to their row vector width", who);
    return check_std(who, net, sys->n);
}

// hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 after their NULL-descriptor check: the checks of check_value_grad in its order, for
// these entry points' outputs (dy = dy_dx, PD head only: the soft-PD entry point passes NULL); a user-defined system has a kernel only when
// its handle asked for the matrix-core kernels (hjbx_user_value_hessian of hjbx_user.hip compiles it at the first call)
inline int check_value_hessian(const char* who, const hjbx_system* sys, const hjbx_net& net, const float* x, const float* H, const float* dy, int64_t B) {
    if (B < 0) return hjbx_set_error(HJBX_EINVAL, "%s: negative batch size", who);
    if (B == 0 || (!H && !dy)) return kEmptyCall;
    if (!x || !net.W1 || !net.W2 || !net.W3 || (net.soft && (!net.b1 || !net.b2 || !net.b3 || !net.w4 || !net.b4)))
        return hjbx_set_error(HJBX_EINVAL, net.soft ? "%s: NULL x, weight or bias pointer" : "%s: NULL x or weight pointer", who);
    if (sys->kind == HJBX_SYS_USER && !hjbx_user_matrix_cores(sys))
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: user-defined systems are not supported unless the handle has asked for the matrix-core kernels "
                                                 "(hjbx_system_enable_matrix_cores)", who);
    if (int rc = check_features(who, net)) return rc;
    if (!state_rows_aligned(x, sys) || (reinterpret_cast<uintptr_t>(H) & 15u) || (reinterpret_cast<uintptr_t>(dy) & 15u))
        return hjbx_set_error(HJBX_EINVAL, net.soft ? "%s: x must be aligned to its row vector width, H to 16 bytes"
                                                    : "%s: x must be aligned to its row vector width, H and dy_dx to 16 bytes", who);
    return check_std(who, net, sys->n);
}

// hjbx_vhjb_rollout_f32 / hjbx_softpd_rollout_f32 after their NULL-descriptor check
inline int check_rollout(const char* who, const hjbx_system* sys, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& a) {
    if (int rc = check_task(task)) return rc;
    if (a.B < 0 || a.n_steps < 0 || a.t_first < 0 || a.T_max < 0) return hjbx_set_error(HJBX_EINVAL, "%s: negative size or step index", who);
    if (int rc = check_integrator(sys, a.integrator, who)) return rc;
    if (a.B == 0) return kEmptyCall;
    if (!a.x || !a.cost || !a.done || !a.done_step || (!net.soft && (!net.W1 || !net.W2 || !net.W3)))
        return hjbx_set_error(HJBX_EINVAL, net.soft ? "%s: x, cost, done and done_step must be non-NULL" : "%s: x, cost, done, done_step and the weights must be non-NULL", who);
    if (!a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 15u))
        return hjbx_set_error(HJBX_EINVAL, "%s: workspace must be a 16-byte aligned device buffer of hjbx_rollout_workspace_bytes() zero-filled bytes", who);
    if (int rc = check_net(who, sys, net)) return rc;
    if (!state_rows_aligned(a.x, sys) || (a.traj && !state_rows_aligned(a.traj, sys)) || (a.x_out && !state_rows_aligned(a.x_out, sys)) ||
        (a.u_log && !aligned_rows(a.u_log, (size_t)sys->m * sizeof(float))))
        return hjbx_set_error(HJBX_EINVAL, "%s: x / traj / x_out / u_log must be aligned to their row vector width", who);
    return check_std(who, net, sys->n);
}

// ---- grids -------------------------------------------------------------------------------------------------------------------------
// tile groups of `per_group` samples (value gradient: 32 * TL environments; Hessian: 32 / n samples, n columns each); one resident workgroup
// per CU (106 KB of LDS each); small batches are spread one tile group per CU rather than packed eight to a workgroup, so up to n_cu matrix
// pipes work on them
inline int mlp_persistent_grid(int64_t B, int per_group, int64_t* ngroups, int64_t* grid, const char* who) {
    *ngroups = (B + per_group - 1) / per_group;
    const int n_cu = hjbx_device_cus();
    if (n_cu <= 0) return hjbx_set_error(HJBX_ENODEVICE, "%s: no HIP device", who);
    *grid = *ngroups < n_cu ? *ngroups : n_cu;
    return HJBX_OK;
}

// rollout: as above with one tile of 32 environments per wave, plus the schedule and the test hook for workgroups that cannot be resident before others finish
inline int mlp_rollout_grid(int64_t B, int64_t* ngroups, int64_t* grid, int* sched, const char* who) {
    if (int rc = mlp_persistent_grid(B, 32, ngroups, grid, who)) return rc;
    *sched = hjbx_option_value(HJBX_OPT_ROLLOUT_SCHEDULE);
    *grid += hjbx_option_value(HJBX_OPT_ROLLOUT_EXTRA_WORKGROUPS);
    if (*grid > kMaxGrid) *grid = kMaxGrid;
    return HJBX_OK;
}

// ---- the launchers of the built-in systems (arguments already validated by the C entry point) ------------------------------------------
// launch shape: TL tiles of 32 environments per wave, WAVES waves per workgroup (one workgroup per CU).
//   (TL, WAVES) = (1, 8): two waves per SIMD, 256 VGPRs each.   (2, 4): one wave per SIMD, 512 VGPRs.
template <typename S, int TL, int WAVES, int ACT, int ARITH, typename Head>
int launch_value_grad(S sys, const hjbx_net& net, const float* x, float* V, float* g, int64_t B, void* st, const char* who) {
    const MlpP<S::N> p = make_mlp_params<S::N>(net);
    int64_t ngroups = 0, grid = 0;
    if (int rc = mlp_persistent_grid(B, 32 * TL, &ngroups, &grid, who)) return rc;
    hipLaunchKernelGGL((k_value_grad_mfma<S, TL, WAVES, ACT, ARITH, Head>), dim3((unsigned)grid), dim3(WAVES * 64), 0, (hipStream_t)st, sys, p, net.W1,
                       net.W2, net.W3, x, V, g, B, ngroups, make_head<Head>(net));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

// Hessian: 32 / n samples per tile, kHessWaves waves per workgroup (design: top of hjbx_hessian.hip); dy = NULL for the soft-PD head
template <typename S, int ACT, typename Head>
int launch_value_hessian(S sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* st, const char* who) {
    const MlpP<S::N> p = make_mlp_params<S::N>(net);
    int64_t ngroups = 0, grid = 0;
    if (int rc = mlp_persistent_grid(B, 32 / S::N, &ngroups, &grid, who)) return rc;
    hipLaunchKernelGGL((k_value_hessian<S, kHessWaves, ACT, Head>), dim3((unsigned)grid), dim3(kHessWaves * 64), 0, (hipStream_t)st, sys, p, net.W1,
                       net.W2, net.W3, x, H, dy, B, ngroups, make_head<Head>(net));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

template <typename S, int WAVES, int ACT, int ARITH, typename Head>
int launch_rollout(const hjbx_system* sysh, S sys, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& a, const char* who) {
    constexpr int N = S::N, M = S::M;
    const MlpP<N> p = make_mlp_params<N>(net);
    const auto tk = make_task<float, N, M>(task);
    const auto lim = make_limits<float, M>(sysh);
    RolloutOut<N, M> o{a.traj, a.u_log, a.cost, a.done, a.resid, a.done_step, a.x_out};
    int64_t ngroups = 0, grid = 0;
    int sched = 0;
    if (int rc = mlp_rollout_grid(a.B, &ngroups, &grid, &sched, who)) return rc;
    auto launch = [&](auto integ) {
        hipLaunchKernelGGL((k_vhjb_rollout_mfma<decltype(integ)::value, S, WAVES, ACT, ARITH, Head>), dim3((unsigned)grid), dim3(WAVES * 64), 0,
                           (hipStream_t)a.stream, sys, p, tk, lim, net.W1, net.W2, net.W3, a.t_first, a.n_steps, a.T_max, a.x, a.env_order, o, a.B, ngroups,
                           (unsigned*)a.workspace, sched, make_head<Head>(net));
    };
    if (a.integrator == HJBX_EULER) launch(std::integral_constant<int, 0>{});
    else if (a.integrator == HJBX_RK4) launch(std::integral_constant<int, 1>{});
    else if constexpr (S::kHasZoh) launch(std::integral_constant<int, 2>{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

// ---- system kind -> instantiation --------------------------------------------------------------------------------------------------
// Development builds (-DHJBX_MLP_DEV: 30 instantiations take a minute per variant) narrow the two lists below to the cart-pole, with
// -DHJBX_MLP_DEV_QUAD2D the planar quadrotor's value gradient (and with it the Hessian) as well; what they keep is launched as in the product.
// Value gradient and Hessian: seven cases (V does not depend on m; wrap is all the kernels take from the system, so its parameters stay
// unset).  go(system) launches one instantiation.
template <typename Go> int dispatch_value_system(const hjbx_system* sys, const char* who, Go go) {
    switch (sys->kind) {
    case HJBX_SYS_CARTPOLE: return go(Cartpole<float>{});
#if !defined(HJBX_MLP_DEV) || defined(HJBX_MLP_DEV_QUAD2D)
    case HJBX_SYS_QUAD2D: return go(Quad2D<float>{});
#endif
#ifndef HJBX_MLP_DEV
    case HJBX_SYS_LINEAR:
        if (sys->n == 2) return go(Linear<float, 2, 1>{});
        if (sys->n == 4) return go(Linear<float, 4, 1>{});
        if (sys->n == 6) return go(Linear<float, 6, 2>{});
        break;
    case HJBX_SYS_ACROBOT: return go(Acrobot<float>{});
    case HJBX_SYS_NEARHOVER: return go(NearHover<float>{});
#endif
    }
    return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no kernel for system kind %d with n=%d", who, sys->kind, sys->n);
}
template <int TL, int WAVES, int ACT, int ARITH, typename Head>
int dispatch_value_grad(const hjbx_system* sys, const hjbx_net& net, const float* x, float* V, float* g, int64_t B, void* st, const char* who) {
    return dispatch_value_system(sys, who, [&](auto s) { return launch_value_grad<decltype(s), TL, WAVES, ACT, ARITH, Head>(s, net, x, V, g, B, st, who); });
}
template <int ACT, typename Head>
int dispatch_value_hessian(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* st, const char* who) {
    return dispatch_value_system(sys, who, [&](auto s) { return launch_value_hessian<decltype(s), ACT, Head>(s, net, x, H, dy, B, st, who); });
}

// Rollout: every built-in system of even state dimension (with_system), each with the integrators it has.
template <int WAVES, int ACT, int ARITH, typename Head>
int dispatch_rollout(const hjbx_system* sys, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& a, const char* who) {
    int rc = HJBX_EUNSUPPORTED;
    const bool ok = with_system<float>(sys, [&](auto S) {
        using SS = decltype(S);
#ifdef HJBX_MLP_DEV
        if constexpr (std::is_same<SS, Cartpole<float>>::value)
#else
        if constexpr (SS::N % 2 == 0)
#endif
            rc = launch_rollout<SS, WAVES, ACT, ARITH, Head>(sys, S, task, net, a, who);
    });
    if (!ok || rc == HJBX_EUNSUPPORTED) return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no kernel for system kind %d with n=%d m=%d", who, sys->kind, sys->n, sys->m);
    return rc;
}

// ---- the hidden per-object symbols -------------------------------------------------------------------------------------------------
// hjbx_mlp.hip and hjbx_softpd.hip are compiled once per variant; object v defines <prefix>_value_grad_act<v> and <prefix>_rollout_act<v>
// (the two dispatchers above for its activation and arithmetic), and the object with the C entry points calls the one it selects.
// hjbx_hessian.hip and hjbx_softpd_hessian.hip do the same with <prefix>_value_hessian_act<v>, v = hjbx_activation.
using mlp_value_grad_fn = int(const hjbx_system* sys, const hjbx_net& net, const float* x, float* V, float* g, int64_t B, void* stream, const char* who);
using mlp_rollout_fn = int(const hjbx_system* sys, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& a, const char* who);
using mlp_value_hessian_fn = int(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* stream, const char* who);
#define HJBX_MLP_SYM2(prefix, name, v) prefix##name##v
#define HJBX_MLP_SYM(prefix, name, v) HJBX_MLP_SYM2(prefix, name, v)
#define HJBX_MLP_DECLARE_VARIANT(prefix, v)                                                          \
    __attribute__((visibility("hidden"))) mlp_value_grad_fn HJBX_MLP_SYM(prefix, _value_grad_act, v); \
    __attribute__((visibility("hidden"))) mlp_rollout_fn HJBX_MLP_SYM(prefix, _rollout_act, v);
#define HJBX_MLP_DEFINE_VARIANT(prefix, v, TL, WAVES, ACT, ARITH, Head)                                                                            \
    int HJBX_MLP_SYM(prefix, _value_grad_act, v)(const hjbx_system* sys, const hjbx_net& net, const float* x, float* V, float* g, int64_t B,        \
                                                 void* stream, const char* who) {                                                                  \
        return dispatch_value_grad<TL, WAVES, ACT, ARITH, Head>(sys, net, x, V, g, B, stream, who);                                                \
    }                                                                                                                                              \
    int HJBX_MLP_SYM(prefix, _rollout_act, v)(const hjbx_system* sys, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& a,       \
                                              const char* who) {                                                                                   \
        return dispatch_rollout<WAVES, ACT, ARITH, Head>(sys, task, net, a, who);                                                                  \
    }
#define HJBX_HESS_DECLARE_VARIANT(prefix, v) __attribute__((visibility("hidden"))) mlp_value_hessian_fn HJBX_MLP_SYM(prefix, _value_hessian_act, v);
#define HJBX_HESS_DEFINE_VARIANT(prefix, v, ACT, Head)                                                                                              \
    int HJBX_MLP_SYM(prefix, _value_hessian_act, v)(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B,    \
                                                    void* stream, const char* who) {                                                               \
        return dispatch_value_hessian<ACT, Head>(sys, net, x, H, dy, B, stream, who);                                                              \
    }
