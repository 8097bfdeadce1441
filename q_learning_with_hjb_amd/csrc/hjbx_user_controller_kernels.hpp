// hjbx_user_controller_kernels.hpp -- the translation unit hiprtc compiles for ONE (system, user-defined control law) pair
// (hjbx_user_controller_create, include/hjbx.h): the reference's second plugin surface, "anything with get_control_efforts(x)"
// (controller/controller_basic.py:1-5), inside the closed loop of controller/vhjb.py:171-193.  A subclass of the reference's `Controller`
// hands its law over as a device-code snippet and gets two kinds of kernels for it: the law alone (the counterpart of k_controller_body)
// and the whole closed loop in one launch (the counterpart of k_rollout_feedback_body, hjbx_stream_kernels.hpp).
//
// Defined by the host before this file is compiled:
//   HJBX_LAW_SYSTEM       hjbx_system_kind of the system the law drives: 0 Linear<T, HJBX_USER_N, HJBX_USER_M>, 1 Cartpole, 2 Acrobot, 3 Quad2D,
//                         4 NearHover, 5 UserSystem<T> (hjbx_user_kernels.hpp around the system's own snippet "hjbx_user_snippet.hpp", with
//                         HJBX_USER_N / _M / _NP / _KIND exactly as for the system's streaming unit)
//   HJBX_LAW_NQ           number of law parameters q[0..NQ-1] (at least 1: a law without parameters gets one unused value), <= 128
//   HJBX_LAW_NW           number of per-environment values w[0..NW-1], 0..32
//   HJBX_LAW_HAS_REACHED  1 when the snippet defines `reached`
// and the in-memory header "hjbx_user_law_snippet.hpp" = the member functions of UserLaw below, written for a scalar type `T` (float and
// double are both instantiated) and a system struct `S`:
//   required   HJBX_DEV void control(const S& sys, const Limits<T, S::M>& lim, const T* x, const T* w, T t, T* u) const
//                  writes the RAW control u[0..M); the kernels clip it to [umin, umax] afterwards (clip_u, as controller_eval does).
//                  w = this environment's NW values (never to be dereferenced when NW = 0), t = the time of the step.
//   optional   HJBX_DEV bool reached(const S& sys, const T* x, const T* w, T t) const
//                  (HJBX_LAW_HAS_REACHED) the stop test behind HJBX_ROLLOUT_STOP_AT_TARGET.
// The snippet may use q[i], T, S::N, S::M, the public members of the system struct (sys.mc, sys.l, ... of a built-in system; sys.p[i] and
// the system snippet's own functions of a user-defined one), everything in hjbx_systems.hpp (sincos_t, wrap_angle, quad_form, clamp_t,
// sys.wrap, sys.affine, sys.energy, ...) and plain C++.  Index q, x, w and u with compile-time constants (or in loops of constant trip
// count, which are unrolled): a private array indexed by a run-time value lives in scratch memory, not in registers.
// A law keeps no state between steps.
#pragma once
#define HJBX_USER_CONTROLLER_UNIT 1   // (also keeps hjbx_user_kernels.hpp from emitting the 32 streaming kernels a second time)
#if HJBX_LAW_SYSTEM == 5
#include "hjbx_user_kernels.hpp"
#else
#include "hjbx_stream_kernels.hpp"
#endif

#if HJBX_LAW_NQ < 1 || HJBX_LAW_NQ > 128 || HJBX_LAW_NW < 0 || HJBX_LAW_NW > 32
#error "a user-defined control law takes 1..128 parameters and 0..32 per-environment values"
#endif

namespace hjbx {

template <typename T, typename S> struct UserLaw {
    T q[HJBX_LAW_NQ];   // the ONLY data member: the host builds this struct as a plain array of HJBX_LAW_NQ values

#include "hjbx_user_law_snippet.hpp"
};

#if HJBX_LAW_SYSTEM == 0
template <typename T> using LawSystem = Linear<T, HJBX_USER_N, HJBX_USER_M>;
#elif HJBX_LAW_SYSTEM == 1
template <typename T> using LawSystem = Cartpole<T>;
#elif HJBX_LAW_SYSTEM == 2
template <typename T> using LawSystem = Acrobot<T>;
#elif HJBX_LAW_SYSTEM == 3
template <typename T> using LawSystem = Quad2D<T>;
#elif HJBX_LAW_SYSTEM == 4
template <typename T> using LawSystem = NearHover<T>;
#elif HJBX_LAW_SYSTEM == 5
template <typename T> using LawSystem = UserSystem<T>;
#else
#error "HJBX_LAW_SYSTEM: unknown hjbx_system_kind"
#endif

static constexpr int kLawNW = HJBX_LAW_NW;
static constexpr int kLawNWRegs = HJBX_LAW_NW > 0 ? HJBX_LAW_NW : 1;   // (no zero-length array; never read when NW = 0)

// Controller.get_control_efforts for one row per thread: the counterpart of k_controller_body
template <typename S, typename T>
HJBX_DEV void k_user_control_body(S sys, UserLaw<T, S> law, Limits<T, S::M> lim, T t, const T* __restrict__ x, const T* __restrict__ w,
                                  T* __restrict__ u, int64_t B) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    T xs[S::N], ws[kLawNWRegs], ur[S::M], uo[S::M];
    RowIO<T, S::N>::load(x, i, xs);
    if constexpr (kLawNW > 0) RowIO<T, kLawNWRegs>::load(w, i, ws);
    law.control(sys, lim, xs, ws, t, ur);
    clip_u<T, S::M>(lim, ur, uo);
    RowIO<T, S::M>::store(u, i, uo);
}

// The whole closed loop in one launch: k_rollout_feedback_body (hjbx_stream_kernels.hpp) line for line -- one lane per environment; state,
// w row and running total in registers for all T steps; RowIO vector accesses; time-major logs; every output optional; the same
// done_step / terminal tuple / total_cost / x_final and HJBX_ROLLOUT_TERMINATE -- except that (1) the control is law.control then clip_u,
// (2) HJBX_ROLLOUT_STOP_AT_TARGET consults law.reached, (3) both are given the time of the step, t0 + k dt.
template <int INTEG, typename S, typename T>
HJBX_DEV void k_user_rollout_body(S sys, UserLaw<T, S> law, TaskP<T, S::N, S::M> tk, Limits<T, S::M> lim, uint32_t flags, int has_task,
                                  int T_steps, T t0, const T* __restrict__ x0, const T* __restrict__ w, T* __restrict__ traj,
                                  T* __restrict__ u_log, T* __restrict__ cost, int32_t* __restrict__ done_step, T* __restrict__ total_cost,
                                  T* __restrict__ x_final, int64_t B) {
    constexpr int N = S::N, M = S::M;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    T x[N], xn[N], u[M], ws[kLawNWRegs];
    RowIO<T, N>::load(x0, i, x);
    if constexpr (kLawNW > 0) RowIO<T, kLawNWRegs>::load(w, i, ws);
    const bool term = (flags & kRolloutTerminate) != 0;
    const bool stop_at_target = (flags & kRolloutStopAtTarget) != 0;
    int ds = -1;
    T tot = T(0);
    for (int t = 0; t <= T_steps; ++t) {
        if (traj) RowIO<T, N>::store(traj + (int64_t)t * B * N, i, x);
        T cst = T(0);
#pragma unroll
        for (int j = 0; j < M; ++j) u[j] = T(0);
        if (ds < 0) {
            const T time = T(t0) + T(t) * lim.dt;
            T e[N];
            bool oob = false;
            if (has_task) {
                error_coords(sys, tk.xf, x, e);
                oob = term && out_of_box<S, T>(tk, e);
            }
            bool reached = false;
#if HJBX_LAW_HAS_REACHED
            if (stop_at_target) reached = law.reached(sys, x, ws, time);
#else
            (void)stop_at_target;   // (the host refuses the flag for a law without `reached`)
#endif
            if (t == T_steps || oob || reached) {
                if (has_task && term && !reached) cst = quad_form<N>(tk.P, e);
                ds = t;
            } else {
                T ur[M];
                law.control(sys, lim, x, ws, time, ur);
                clip_u<T, M>(lim, ur, u);
                if (has_task) cst = running_cost_e<S, T>(tk, e, u) * lim.dt;
                integrate<INTEG>(sys, lim.dt, x, u, xn);
#pragma unroll
                for (int k = 0; k < N; ++k) x[k] = xn[k];
            }
        }
        tot += cst;
        if (cost) cost[(int64_t)t * B + i] = cst;
        if (u_log && t < T_steps) RowIO<T, M>::store(u_log + (int64_t)t * B * M, i, u);
    }
    if (done_step) done_step[i] = ds;
    if (total_cost) total_cost[i] = tot;
    if (x_final) RowIO<T, N>::store(x_final, i, x);
}

// HIP passes at most 4 KB of kernel arguments: the by-value structs of the float64 rollout kernel (the largest) plus its 13 scalar and pointer
// arguments (8 bytes each at most) stay below that.  NQ <= 128 and NW <= 32 are chosen so that this holds up to n = 10, m = 3.
static_assert(sizeof(LawSystem<double>) + sizeof(UserLaw<double, LawSystem<double>>) + sizeof(TaskP<double, LawSystem<double>::N, LawSystem<double>::M>) +
                      sizeof(Limits<double, LawSystem<double>::M>) + 13 * 8 <= 4096,
              "the kernel arguments of hjbx_uc_rollout_*_f64 exceed HIP's 4 KB limit");

}  // namespace hjbx

using namespace hjbx;

// extern "C" kernels (names are looked up by hjbx_user.hip): one row per thread, the integrator in the name
#define HJBX_UC_KERNELS(T, SFX)                                                                                                             \
    using UC_##SFX = LawSystem<T>;                                                                                                          \
    extern "C" __global__ __launch_bounds__(kBlock) void hjbx_uc_control_##SFX(UC_##SFX s, UserLaw<T, UC_##SFX> law,                        \
                                                                              Limits<T, UC_##SFX::M> lim, T t, const T* x, const T* w,     \
                                                                              T* u, int64_t B) {                                           \
        k_user_control_body<UC_##SFX, T>(s, law, lim, t, x, w, u, B);                                                                       \
    }                                                                                                                                       \
    extern "C" __global__ __launch_bounds__(kBlock) void hjbx_uc_rollout_i0_##SFX(                                                          \
        UC_##SFX s, UserLaw<T, UC_##SFX> law, TaskP<T, UC_##SFX::N, UC_##SFX::M> tk, Limits<T, UC_##SFX::M> lim, uint32_t flags,            \
        int has_task, int T_steps, T t0, const T* x0, const T* w, T* traj, T* u_log, T* cost, int32_t* done_step, T* total_cost,            \
        T* x_final, int64_t B) {                                                                                                            \
        k_user_rollout_body<0, UC_##SFX, T>(s, law, tk, lim, flags, has_task, T_steps, t0, x0, w, traj, u_log, cost, done_step, total_cost, \
                                            x_final, B);                                                                                   \
    }                                                                                                                                       \
    extern "C" __global__ __launch_bounds__(kBlock) void hjbx_uc_rollout_i1_##SFX(                                                          \
        UC_##SFX s, UserLaw<T, UC_##SFX> law, TaskP<T, UC_##SFX::N, UC_##SFX::M> tk, Limits<T, UC_##SFX::M> lim, uint32_t flags,            \
        int has_task, int T_steps, T t0, const T* x0, const T* w, T* traj, T* u_log, T* cost, int32_t* done_step, T* total_cost,            \
        T* x_final, int64_t B) {                                                                                                            \
        k_user_rollout_body<1, UC_##SFX, T>(s, law, tk, lim, flags, has_task, T_steps, t0, x0, w, traj, u_log, cost, done_step, total_cost, \
                                            x_final, B);                                                                                   \
    }

HJBX_UC_KERNELS(float, f32)
HJBX_UC_KERNELS(double, f64)
