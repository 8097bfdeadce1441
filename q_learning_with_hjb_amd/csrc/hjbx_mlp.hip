// hjbx_mlp.hip -- ValueFunctionApproximator forward + input gradient (reference controller/vhjb.py:17-60
// and get_v_gradient :201-202) fused into one gfx950 kernel on the matrix cores: this file holds the two kernels and the float32-MFMA
// arithmetic described below; the same kernels instantiate the 16-bit split-operand arithmetics of hjbx_mlp_x3.hpp (bf16 x 3) and
// hjbx_mlp_h2.hpp (f16 x 2; both opt-in, HJBX_OPT_MLP_ARITHMETIC) through the AR template parameter.
//
//   e = wrap(x - xf); z = (e - mean)/std; h1 = act(z W1); h2 = act(h1 W2); y = h2 W3        (act = relu | tanh | sin)
//   V = |y|^2 + eps_s |e|^2
//   dV/dx = ((((2y) W3') . act'(h2)) W2' . act'(h1)) W1' / std + 2 eps_s e
//
// Design (CDNA4):
//  * v_mfma_f32_32x32x2_f32 (exact f32, 157 TFLOP/s dense peak) -- the network is float32 in the reference.
//  * Everything is computed TRANSPOSED (features x environments): a wave owns TL tiles of 32 environments
//    (the MFMA column index = lane & 31) and the accumulator registers of one layer ARE the B operands of
//    the next one, forward and backward, with no cross-lane movement and no LDS round trip: accumulator
//    register s of lane-half h holds feature perm(s) + 4h, and the weight (A) operand for k-step s is
//    simply fetched for that same feature.
//  * All three weight matrices live in LDS once per workgroup (106 KB, one copy serves W and W'): rows
//    padded to an ODD stride (129 / 65 floats) so that both the row walk of the forward pass and the
//    column walk of the backward pass hit 32 distinct banks per ds_read_b32 lane group.
//  * A VALU-category instruction issued between two MFMAs costs matrix-pipe time (~4 cycles each, tools/ubench/mfma_mix.hip;
//    LDS reads and s_waitcnt issue beside the MFMAs for free), so a chain is ONLY ds_read / s_waitcnt / MFMA: weight
//    operands are prefetched by inline-asm ds_reads two k-steps ahead and retired by counted s_waitcnt; the element-wise
//    work (activation, its derivative, |y|^2, 2y) runs in place on the accumulators in VALU-only passes between the
//    chains, where it overlaps the SIMD partner's MFMAs; activation derivatives are taken from the activations (nothing
//    extra is stored; layer 1 is recomputed for the last one); the last backward product (only n useful rows) runs on the
//    VALU.  The activation is a template parameter: ReLU (one integer max) or tanh (exp2 + rcp).
//  * Persistent grid, one workgroup per CU (2 waves per SIMD); waves pull tile groups from an LDS counter so SIMD
//    partners finish together.  In the rollout kernel the per-environment constants (system, task, limits) are staged
//    in LDS too: as kernel-argument SGPRs they spilled into v_readlane / v_writelane inside the chains.
// Per environment: 4(128 n + 128*128 + 128*64) flop; algorithmic HBM traffic 4(2n+1) bytes -> MFMA bound.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstddef>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"
#include "hjbx_host.hpp"
#include "hjbx_mlp_core.hpp"
#include "hjbx_mlp_x3.hpp"
#include "hjbx_mlp_h2.hpp"
#include "hjbx_mlp_kernels.hpp"
#include "hjbx_mlp_host.hpp"

using namespace hjbx;

// launch shape: TL tiles of 32 environments per wave, WAVES waves per workgroup (one workgroup per CU).
//   (TL, WAVES) = (1, 8): two waves per SIMD, 256 VGPRs each.   (2, 4): one wave per SIMD, 512 VGPRs.
// This file is compiled once per variant (-DHJBX_MLP_ACT=0 relu, =1 tanh, =2 relu with the bf16x3-split arithmetic of hjbx_mlp_x3.hpp,
// =3 relu with the f16x2-split arithmetic of hjbx_mlp_h2.hpp, =4 sin: 30 kernel instantiations each, side by side); the relu object also
// carries the two C entry points, which validate and hand over to the object of the requested variant.
#ifndef HJBX_MLP_ACT
#error "compile hjbx_mlp.hip with -DHJBX_MLP_ACT=0 (relu + the C entry points), =1 (tanh), =2 (relu, bf16x3-split MFMA), =3 (relu, f16x2-split MFMA) and =4 (sin)"
#endif
static constexpr int kArith = HJBX_MLP_ACT == 2 ? 1 : HJBX_MLP_ACT == 3 ? 2 : 0;  // 0 = f32 MFMA, 1 = bf16x3, 2 = f16x2 (HJBX_OPT_MLP_ARITHMETIC)
static constexpr int kAct = kArith ? HJBX_ACT_RELU : HJBX_MLP_ACT == 4 ? HJBX_ACT_SIN : HJBX_MLP_ACT;
static_assert(kAct == HJBX_ACT_RELU || kAct == HJBX_ACT_TANH || kAct == HJBX_ACT_SIN, "fused kernels exist for relu, tanh and sin");
#define HJBX_MLP_CAT2(a, b) a##b
#define HJBX_MLP_CAT(a, b) HJBX_MLP_CAT2(a, b)
#define HJBX_MLP_SYM(name) HJBX_MLP_CAT(name, HJBX_MLP_ACT)
#define HJBX_HIDDEN __attribute__((visibility("hidden")))
// per-activation dispatchers (system kind -> kernel instantiation), one pair per object file
HJBX_HIDDEN int hjbx_mlp_value_grad_act0(const hjbx_system*, const hjbx_mlp*, const float*, float*, float*, int64_t, void*);
HJBX_HIDDEN int hjbx_mlp_value_grad_act1(const hjbx_system*, const hjbx_mlp*, const float*, float*, float*, int64_t, void*);
HJBX_HIDDEN int hjbx_mlp_value_grad_act2(const hjbx_system*, const hjbx_mlp*, const float*, float*, float*, int64_t, void*);
HJBX_HIDDEN int hjbx_mlp_value_grad_act3(const hjbx_system*, const hjbx_mlp*, const float*, float*, float*, int64_t, void*);
HJBX_HIDDEN int hjbx_mlp_value_grad_act4(const hjbx_system*, const hjbx_mlp*, const float*, float*, float*, int64_t, void*);
HJBX_HIDDEN int hjbx_mlp_rollout_act3(const hjbx_system*, const hjbx_task*, const hjbx_mlp*, int, int, int, int, const float*, float*, float*, float*,
                                      float*, float*, int32_t*, float*, const int32_t*, int64_t, void*, void*);
HJBX_HIDDEN int hjbx_mlp_rollout_act2(const hjbx_system*, const hjbx_task*, const hjbx_mlp*, int, int, int, int, const float*, float*, float*, float*,
                                      float*, float*, int32_t*, float*, const int32_t*, int64_t, void*, void*);
HJBX_HIDDEN int hjbx_mlp_rollout_act0(const hjbx_system*, const hjbx_task*, const hjbx_mlp*, int, int, int, int, const float*, float*, float*, float*,
                                      float*, float*, int32_t*, float*, const int32_t*, int64_t, void*, void*);
HJBX_HIDDEN int hjbx_mlp_rollout_act1(const hjbx_system*, const hjbx_task*, const hjbx_mlp*, int, int, int, int, const float*, float*, float*, float*,
                                      float*, float*, int32_t*, float*, const int32_t*, int64_t, void*, void*);
HJBX_HIDDEN int hjbx_mlp_rollout_act4(const hjbx_system*, const hjbx_task*, const hjbx_mlp*, int, int, int, int, const float*, float*, float*, float*,
                                      float*, float*, int32_t*, float*, const int32_t*, int64_t, void*, void*);

#ifndef HJBX_MLP_TL
#define HJBX_MLP_TL 1
#endif
#ifndef HJBX_MLP_WAVES
#define HJBX_MLP_WAVES 8
#endif
// kernel 1 (k_value_grad_mfma: V and dV/dx for a batch of states) and kernel 2 (k_vhjb_rollout_mfma: the whole VHJB closed loop for n_steps
// steps in one launch) are in hjbx_mlp_kernels.hpp, instantiated here with the PD head (MlpHeadPd)


#if HJBX_MLP_ACT == 0
extern "C" size_t hjbx_rollout_workspace_bytes(void) { return (size_t)kWsWords * sizeof(unsigned); }
static int check_activation(const hjbx_mlp* mlp, const char* who) {
    if (mlp->activation == HJBX_ACT_RELU || mlp->activation == HJBX_ACT_TANH || mlp->activation == HJBX_ACT_SIN) return HJBX_OK;
    return hjbx_set_error(HJBX_EINVAL, "%s: unknown activation %d", who, mlp->activation);
}
// a user-defined system that asked for the matrix-core kernels (hjbx_system_enable_matrix_cores) gets them compiled at run time, in the
// float32 MFMA arithmetic only
static int check_user_arithmetic(const char* who) {
    if (hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC) == 0) return HJBX_OK;
    return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: HJBX_OPT_MLP_ARITHMETIC=%d (split-operand MFMA) is not compiled for user-defined systems; set it to 0", who,
                          hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC));
}
static hjbx_user_net user_net(const hjbx_mlp* mlp) {
    return hjbx_user_net{0, mlp->activation, mlp->mean, mlp->std, mlp->xf, mlp->eps_scalar, (const float*)mlp->W1, (const float*)mlp->W2,
                         (const float*)mlp->W3, nullptr, nullptr, nullptr, nullptr, nullptr};
}
#endif

template <typename S> static int launch_value_grad(S sys, const hjbx_mlp* mlp, const float* x, float* V, float* g, int64_t B, void* st) {
    constexpr int N = S::N;
    constexpr int TL = HJBX_MLP_TL, WAVES = HJBX_MLP_WAVES;
    const MlpP<N> p = make_mlp_params<N>(mlp->mean, mlp->std, mlp->xf, mlp->eps_scalar);
    int64_t ngroups = 0, grid = 0;   // one resident workgroup per CU, small batches one tile group per CU (hjbx_mlp_host.hpp)
    if (int rc = mlp_value_grad_grid(B, TL, &ngroups, &grid, "hjbx_value_grad_f32")) return rc;
    hipLaunchKernelGGL((k_value_grad_mfma<S, TL, WAVES, kAct, kArith>), dim3((unsigned)grid), dim3(WAVES * 64), 0, (hipStream_t)st, sys, p,
                       (const float*)mlp->W1, (const float*)mlp->W2, (const float*)mlp->W3, x, V, g, B, ngroups, MlpHeadPd{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "hjbx_value_grad_f32: %s", hipGetErrorString(e));
    return HJBX_OK;
}

// system kind -> instantiation of this object's activation (arguments already validated by the C entry point)
int HJBX_MLP_SYM(hjbx_mlp_value_grad_act)(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* V, float* g, int64_t B, void* stream) {
#ifdef HJBX_MLP_DEV  // development builds: cartpole only (30 instantiations take a minute per variant)
    if (sys->kind == HJBX_SYS_CARTPOLE) { Cartpole<float> c{}; return launch_value_grad(c, mlp, x, V, g, B, stream); }
#ifdef HJBX_MLP_DEV_QUAD2D
    if (sys->kind == HJBX_SYS_QUAD2D) { Quad2D<float> q{}; return launch_value_grad(q, mlp, x, V, g, B, stream); }
#endif
    return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_value_grad_f32: development build (cartpole only)");
#else
    switch (sys->kind) {
    case HJBX_SYS_LINEAR:
        if (sys->n == 2) {
            Linear<float, 2, 1> l{};  // wrap is the identity; A, B unused here
            return launch_value_grad(l, mlp, x, V, g, B, stream);
        }
        if (sys->n == 4) { Linear<float, 4, 1> l{}; return launch_value_grad(l, mlp, x, V, g, B, stream); }
        if (sys->n == 6) { Linear<float, 6, 2> l{}; return launch_value_grad(l, mlp, x, V, g, B, stream); }
        break;
    case HJBX_SYS_CARTPOLE: { Cartpole<float> c{}; return launch_value_grad(c, mlp, x, V, g, B, stream); }
    case HJBX_SYS_ACROBOT: { Acrobot<float> a{}; return launch_value_grad(a, mlp, x, V, g, B, stream); }
    case HJBX_SYS_QUAD2D: { Quad2D<float> q{}; return launch_value_grad(q, mlp, x, V, g, B, stream); }
    case HJBX_SYS_NEARHOVER: { NearHover<float> q{}; return launch_value_grad(q, mlp, x, V, g, B, stream); }
    }
    return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_value_grad_f32: no kernel for system kind %d with n=%d", sys->kind, sys->n);
#endif
}


#if HJBX_MLP_ACT == 0
extern "C" int hjbx_value_grad_f32(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* V, float* g, int64_t B,
                                   void* stream) {
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "hjbx_value_grad_f32: NULL system or mlp descriptor");
    if (B < 0) return hjbx_set_error(HJBX_EINVAL, "hjbx_value_grad_f32: negative batch size");
    if (B == 0 || (!V && !g)) return HJBX_OK;
    if (!x || !mlp->W1 || !mlp->W2 || !mlp->W3) return hjbx_set_error(HJBX_EINVAL, "hjbx_value_grad_f32: NULL x or weight pointer");
    if (mlp->h1 != kH1 || mlp->h2 != kH2 || mlp->h3 != kH3)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_value_grad_f32: features must be [128,128,64], got [%d,%d,%d]", mlp->h1, mlp->h2,
                              mlp->h3);
    if (int rc = check_activation(mlp, "hjbx_value_grad_f32")) return rc;
    const size_t row = (size_t)sys->n * sizeof(float);
    const uintptr_t am = (row % 16 == 0) ? 15u : 7u;
    if ((reinterpret_cast<uintptr_t>(x) & am) || (g && (reinterpret_cast<uintptr_t>(g) & am)))
        return hjbx_set_error(HJBX_EINVAL, "hjbx_value_grad_f32: x / gradV must be aligned to their row vector width");
    for (int k = 0; k < sys->n; ++k)
        if (!(mlp->std[k] != 0.0)) return hjbx_set_error(HJBX_EINVAL, "hjbx_value_grad_f32: normalization_std[%d] is zero", k);
    if (hjbx_user_matrix_cores(sys)) {
        if (int rc = check_user_arithmetic("hjbx_value_grad_f32")) return rc;
        const hjbx_user_net net = user_net(mlp);
        return hjbx_user_value_grad(sys, &net, x, V, g, B, stream, "hjbx_value_grad_f32");
    }
    if (mlp->activation == HJBX_ACT_TANH) return hjbx_mlp_value_grad_act1(sys, mlp, x, V, g, B, stream);
    if (mlp->activation == HJBX_ACT_SIN) return hjbx_mlp_value_grad_act4(sys, mlp, x, V, g, B, stream);
    const int arith = hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC);
    return arith == 1 ? hjbx_mlp_value_grad_act2(sys, mlp, x, V, g, B, stream)
         : arith == 2 ? hjbx_mlp_value_grad_act3(sys, mlp, x, V, g, B, stream)
                      : hjbx_mlp_value_grad_act0(sys, mlp, x, V, g, B, stream);
}
#endif

template <typename S>
static int launch_vhjb_rollout(const hjbx_system* sysh, S sys, const hjbx_task* task, const hjbx_mlp* mlp, int integrator, int t_first,
                               int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                               int32_t* done_step, float* x_out, const int32_t* order, int64_t B, void* workspace, void* st) {
    constexpr int N = S::N, M = S::M;
    constexpr int WAVES = HJBX_MLP_WAVES;
    const MlpP<N> p = make_mlp_params<N>(mlp->mean, mlp->std, mlp->xf, mlp->eps_scalar);
    const auto tk = make_task<float, N, M>(task);
    const auto lim = make_limits<float, M>(sysh);
    RolloutOut<N, M> o{traj, u_log, cost, done, resid, done_step, x_out};
    int64_t ngroups = 0, grid = 0;   // as in launch_value_grad, plus the schedule and the test hook (hjbx_mlp_host.hpp)
    int sched = 0;
    if (int rc = mlp_rollout_grid(B, &ngroups, &grid, &sched, "hjbx_vhjb_rollout_f32")) return rc;
    const float *W1 = (const float*)mlp->W1, *W2 = (const float*)mlp->W2, *W3 = (const float*)mlp->W3;
    auto launch = [&](auto integ) {
        hipLaunchKernelGGL((k_vhjb_rollout_mfma<decltype(integ)::value, S, WAVES, kAct, kArith>), dim3((unsigned)grid), dim3(WAVES * 64), 0,
                           (hipStream_t)st, sys, p, tk, lim, W1, W2, W3, t_first, n_steps, T_max, x, order, o, B, ngroups, (unsigned*)workspace, sched, MlpHeadPd{});
    };
    if (integrator == HJBX_EULER) launch(std::integral_constant<int, 0>{});
    else if (integrator == HJBX_RK4) launch(std::integral_constant<int, 1>{});
    else if constexpr (S::kHasZoh) launch(std::integral_constant<int, 2>{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "hjbx_vhjb_rollout_f32: %s", hipGetErrorString(e));
    return HJBX_OK;
}

int HJBX_MLP_SYM(hjbx_mlp_rollout_act)(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int integrator, int t_first, int n_steps,
                                       int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                                       int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace, void* stream) {
    int rc = HJBX_EUNSUPPORTED;
#ifdef HJBX_MLP_DEV
    if (sys->kind == HJBX_SYS_CARTPOLE && integrator == HJBX_EULER) {
        Cartpole<float> S{(float)sys->p[0], (float)sys->p[1], (float)sys->p[2], (float)sys->p[3]};
        constexpr int WAVES = HJBX_MLP_WAVES;
        MlpP<4> p;
        for (int k = 0; k < 4; ++k) { p.mean[k] = (float)mlp->mean[k]; p.istd[k] = (float)(1.0 / mlp->std[k]); p.xf[k] = (float)mlp->xf[k]; }
        p.eps_s = (float)mlp->eps_scalar;
        RolloutOut<4, 1> o{traj, u_log, cost, done, resid, done_step, x_out};
        const int64_t ngroups = (B + 31) / 32;
        int64_t grid = ngroups < 256 ? ngroups : 256;
        hipLaunchKernelGGL((k_vhjb_rollout_mfma<0, Cartpole<float>, WAVES, kAct, kArith>), dim3((unsigned)grid), dim3(WAVES * 64), 0, (hipStream_t)stream, S, p,
                           make_task<float, 4, 1>(task), make_limits<float, 1>(sys), (const float*)mlp->W1, (const float*)mlp->W2, (const float*)mlp->W3, t_first,
                           n_steps, T_max, x, env_order, o, B, ngroups, (unsigned*)workspace, hjbx_option_value(HJBX_OPT_ROLLOUT_SCHEDULE), MlpHeadPd{});
        return hipGetLastError() == hipSuccess ? HJBX_OK : hjbx_set_error(HJBX_EHIP, "launch");
    }
    return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_vhjb_rollout_f32: development build (cartpole, Euler only)");
#else
    const bool ok = with_system<float>(sys, [&](auto S) {
        using SS = decltype(S);
        if constexpr (SS::N % 2 == 0)
            rc = launch_vhjb_rollout<SS>(sys, S, task, mlp, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step,
                                         x_out, env_order, B, workspace, stream);
    });
    if (!ok || rc == HJBX_EUNSUPPORTED)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_vhjb_rollout_f32: no kernel for system kind %d with n=%d m=%d", sys->kind, sys->n, sys->m);
    return rc;
#endif
}

#if HJBX_MLP_ACT == 0
extern "C" int hjbx_vhjb_rollout_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int integrator, int t_first,
                                     int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done,
                                     float* resid, int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace,
                                     void* stream) {
    if (!sys || !task || !mlp) return hjbx_set_error(HJBX_EINVAL, "hjbx_vhjb_rollout_f32: NULL system, task or mlp descriptor");
    if (int rc = check_task(task)) return rc;
    if (B < 0 || n_steps < 0 || t_first < 0 || T_max < 0) return hjbx_set_error(HJBX_EINVAL, "hjbx_vhjb_rollout_f32: negative size or step index");
    if (int rc = check_integrator(sys, integrator, "hjbx_vhjb_rollout_f32")) return rc;
    if (B == 0) return HJBX_OK;
    if (!x || !cost || !done || !done_step || !mlp->W1 || !mlp->W2 || !mlp->W3)
        return hjbx_set_error(HJBX_EINVAL, "hjbx_vhjb_rollout_f32: x, cost, done, done_step and the weights must be non-NULL");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return hjbx_set_error(HJBX_EINVAL, "hjbx_vhjb_rollout_f32: workspace must be a 16-byte aligned device buffer of hjbx_rollout_workspace_bytes() zero-filled bytes");
    if (mlp->h1 != kH1 || mlp->h2 != kH2 || mlp->h3 != kH3)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_vhjb_rollout_f32: features must be [128,128,64], got [%d,%d,%d]", mlp->h1, mlp->h2,
                              mlp->h3);
    if (int rc = check_activation(mlp, "hjbx_vhjb_rollout_f32")) return rc;
    const size_t row = (size_t)sys->n * sizeof(float);
    const uintptr_t am = (row % 16 == 0) ? 15u : 7u;
    const size_t urow = (size_t)sys->m * sizeof(float);
    const uintptr_t um = (urow % 16 == 0) ? 15u : (urow % 8 == 0) ? 7u : 3u;
    if ((reinterpret_cast<uintptr_t>(x) & am) || (traj && (reinterpret_cast<uintptr_t>(traj) & am)) ||
        (x_out && (reinterpret_cast<uintptr_t>(x_out) & am)) || (u_log && (reinterpret_cast<uintptr_t>(u_log) & um)))
        return hjbx_set_error(HJBX_EINVAL, "hjbx_vhjb_rollout_f32: x / traj / x_out / u_log must be aligned to their row vector width");
    for (int k = 0; k < sys->n; ++k)
        if (!(mlp->std[k] != 0.0)) return hjbx_set_error(HJBX_EINVAL, "hjbx_vhjb_rollout_f32: normalization_std[%d] is zero", k);
    if (hjbx_user_matrix_cores(sys)) {
        if (int rc = check_user_arithmetic("hjbx_vhjb_rollout_f32")) return rc;
        const hjbx_user_net net = user_net(mlp);
        return hjbx_user_rollout(sys, task, &net, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B,
                                 workspace, stream, "hjbx_vhjb_rollout_f32");
    }
    if (mlp->activation == HJBX_ACT_TANH)
        return hjbx_mlp_rollout_act1(sys, task, mlp, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B, workspace, stream);
    if (mlp->activation == HJBX_ACT_SIN)
        return hjbx_mlp_rollout_act4(sys, task, mlp, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B, workspace, stream);
    const int arith = hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC);
    return (arith == 1 ? hjbx_mlp_rollout_act2 : arith == 2 ? hjbx_mlp_rollout_act3 : hjbx_mlp_rollout_act0)(
        sys, task, mlp, integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B, workspace, stream);
}
#endif
