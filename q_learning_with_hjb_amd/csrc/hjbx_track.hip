// hjbx_track.hip -- the min-snap waypoint planner of Quadrotors2D on the device (reference
// controller/quadrotors_model_based_controller.py:77-233): the reference generator and the tracking closed loop of hjbx_minsnap.hpp as
// gfx950 kernels, and their four C entry points (include/hjbx.h).  Streaming family: one lane per environment, wave64, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hjbx_internal.hpp"
#include "hjbx_host.hpp"
#include "hjbx_minsnap.hpp"

using namespace hjbx;

namespace {

template <typename T>
__global__ __launch_bounds__(kBlock) void k_minsnap_reference(Quad2D<T> sys, MinsnapPlan<T> plan, double t0, double dt, int64_t rows,
                                                              T* __restrict__ x_ref, T* __restrict__ u_ref, int64_t B) {
    k_minsnap_reference_body<T>(sys, plan, t0, dt, rows, x_ref, u_ref, B);
}

template <int INTEG, typename T>
__global__ __launch_bounds__(kBlock) void k_rollout_minsnap_tracking(Quad2D<T> sys, MinsnapPlan<T> plan, TrackP<T> tp, Limits<T, 2> lim, int want_cost,
                                                                     int T_steps, double t0, double dt, const T* __restrict__ x0, T* __restrict__ traj,
                                                                     T* __restrict__ u_log, T* __restrict__ cost, T* __restrict__ total_cost,
                                                                     T* __restrict__ x_final, T* __restrict__ x_ref_log, T* __restrict__ u_ref_log,
                                                                     int64_t B) {
    k_rollout_minsnap_tracking_body<INTEG, T>(sys, plan, tp, lim, want_cost, T_steps, t0, dt, x0, traj, u_log, cost, total_cost, x_final, x_ref_log,
                                              u_ref_log, B);
}

#define HJBX_REQUIRE(cond, ...)                                       \
    do {                                                              \
        if (!(cond)) return hjbx_set_error(HJBX_EINVAL, __VA_ARGS__); \
    } while (0)

int check_launch(const char* who) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

constexpr int64_t kMaxGrid = 0x7fffffff;

// the checks both entry points share: the system, the plan and its layout.  Run before any launch.
template <typename T>
int check_plan(const char* who, const hjbx_system* sys, const T* coeff, const double* cum_t, const T* end_pt, int S, int64_t n_plans, double t0,
               int T_steps, int64_t B) {
    HJBX_REQUIRE(sys != nullptr, "%s: system handle is NULL", who);
    HJBX_REQUIRE(sys->kind == HJBX_SYS_QUAD2D, "%s: the min-snap planner exists for HJBX_SYS_QUAD2D only (system kind %d)", who, sys->kind);
    HJBX_REQUIRE(B >= 0, "%s: negative batch size %lld", who, (long long)B);
    HJBX_REQUIRE(S >= 1, "%s: a plan has at least one segment, got S = %d", who, S);
    HJBX_REQUIRE(t0 >= 0.0, "%s: t0 must be >= 0, got %g", who, t0);
    HJBX_REQUIRE(T_steps >= 0, "%s: negative horizon %d", who, T_steps);
    HJBX_REQUIRE(n_plans == 1 || n_plans == B, "%s: n_plans must be 1 (shared) or B = %lld (one per environment), got %lld", who, (long long)B,
                 (long long)n_plans);
    HJBX_REQUIRE(coeff != nullptr && aligned_rows(coeff, kMinsnapTerms * sizeof(T)), "%s: coeff must be a non-NULL device pointer aligned to 16 bytes", who);
    HJBX_REQUIRE(cum_t != nullptr && (reinterpret_cast<uintptr_t>(cum_t) & 7u) == 0, "%s: cum_t must be a non-NULL device pointer aligned to 8 bytes", who);
    HJBX_REQUIRE(end_pt != nullptr && aligned_rows(end_pt, 2 * sizeof(T)), "%s: end_pt must be a non-NULL device pointer aligned to its row", who);
    return HJBX_OK;
}

template <typename T> MinsnapPlan<T> make_plan(const T* coeff, const double* cum_t, const T* end_pt, int S, int64_t n_plans, int64_t B) {
    return MinsnapPlan<T>{coeff, cum_t, end_pt, n_plans == 1 ? int64_t(0) : int64_t(1), S};
}

template <typename T> Quad2D<T> make_quad(const hjbx_system* s) { return Quad2D<T>{(T)s->p[0], (T)s->p[1], (T)s->p[2], (T)s->p[3]}; }

template <typename T>
int minsnap_reference_impl(const hjbx_system* sys, const T* coeff, const double* cum_t, const T* end_pt, int S, int64_t n_plans, double t0, int T_steps,
                           T* x_ref, T* u_ref, int64_t B, void* st) {
    const char* who = "hjbx_minsnap_reference";
    if (int rc = check_plan<T>(who, sys, coeff, cum_t, end_pt, S, n_plans, t0, T_steps, B)) return rc;
    HJBX_REQUIRE(x_ref == nullptr || aligned_rows(x_ref, 6 * sizeof(T)), "%s: x_ref must be aligned to its row vector width", who);
    HJBX_REQUIRE(u_ref == nullptr || aligned_rows(u_ref, 2 * sizeof(T)), "%s: u_ref must be aligned to its row vector width", who);
    const int64_t rows = B * (int64_t)T_steps;
    if (rows == 0 || (!x_ref && !u_ref)) return HJBX_OK;
    const int64_t grid = (rows + kBlock - 1) / kBlock;
    HJBX_REQUIRE(grid <= kMaxGrid, "%s: B x T_steps = %lld rows exceed one launch", who, (long long)rows);
    hipLaunchKernelGGL((k_minsnap_reference<T>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)st, make_quad<T>(sys),
                       make_plan<T>(coeff, cum_t, end_pt, S, n_plans, B), t0, sys->dt, rows, x_ref, u_ref, B);
    return check_launch(who);
}

template <typename T>
int rollout_minsnap_tracking_impl(const hjbx_system* sys, const hjbx_task* task, const hjbx_controller* c, int integ, const T* coeff, const double* cum_t,
                                  const T* end_pt, int S, int64_t n_plans, double t0, int T_steps, const T* x0, T* traj, T* u_log, T* cost,
                                  T* total_cost, T* x_final, T* x_ref_log, T* u_ref_log, int64_t B, void* st) {
    const char* who = "hjbx_rollout_minsnap_tracking";
    if (int rc = check_plan<T>(who, sys, coeff, cum_t, end_pt, S, n_plans, t0, T_steps, B)) return rc;
    HJBX_REQUIRE(c != nullptr, "%s: controller is NULL", who);
    HJBX_REQUIRE(c->kind == HJBX_CTRL_LINEAR_FEEDBACK, "%s: the tracking law takes a linear feedback gain (controller kind %d)", who, c->kind);
    HJBX_REQUIRE(integ == HJBX_EULER || integ == HJBX_RK4, "%s: integrator must be HJBX_EULER or HJBX_RK4, got %d", who, integ);
    HJBX_REQUIRE(task != nullptr || (!cost && !total_cost), "%s: cost outputs need a task (Q, R)", who);
    HJBX_REQUIRE(x0 != nullptr && aligned_rows(x0, 6 * sizeof(T)), "%s: x0 must be a non-NULL device pointer aligned to its row vector width", who);
    HJBX_REQUIRE((traj == nullptr || aligned_rows(traj, 6 * sizeof(T))) && (x_final == nullptr || aligned_rows(x_final, 6 * sizeof(T))) &&
                     (x_ref_log == nullptr || aligned_rows(x_ref_log, 6 * sizeof(T))),
                 "%s: traj, x_final and x_ref_log must be aligned to their row vector width", who);
    HJBX_REQUIRE((u_log == nullptr || aligned_rows(u_log, 2 * sizeof(T))) && (u_ref_log == nullptr || aligned_rows(u_ref_log, 2 * sizeof(T))) &&
                     (cost == nullptr || aligned_rows(cost, sizeof(T))) && (total_cost == nullptr || aligned_rows(total_cost, sizeof(T))),
                 "%s: u_log, u_ref_log, cost and total_cost must be aligned to their row vector width", who);
    if (B == 0) return HJBX_OK;
    const int64_t grid = (B + kBlock - 1) / kBlock;
    HJBX_REQUIRE(grid <= kMaxGrid, "%s: B = %lld exceeds one launch", who, (long long)B);
    TrackP<T> tp;
    for (int i = 0; i < 12; ++i) tp.K[i] = (T)c->K[i];
    for (int i = 0; i < 36; ++i) tp.Q[i] = task ? (T)task->Q[i] : T(0);
    for (int i = 0; i < 4; ++i) tp.R[i] = task ? (T)task->R[i] : T(0);
    const int want_cost = (cost || total_cost) ? 1 : 0;
    const auto sysd = make_quad<T>(sys);
    const auto plan = make_plan<T>(coeff, cum_t, end_pt, S, n_plans, B);
    const auto lim = make_limits<T, 2>(sys);
    if (integ == HJBX_RK4)
        hipLaunchKernelGGL((k_rollout_minsnap_tracking<1, T>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)st, sysd, plan, tp, lim, want_cost,
                           T_steps, t0, sys->dt, x0, traj, u_log, cost, total_cost, x_final, x_ref_log, u_ref_log, B);
    else
        hipLaunchKernelGGL((k_rollout_minsnap_tracking<0, T>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)st, sysd, plan, tp, lim, want_cost,
                           T_steps, t0, sys->dt, x0, traj, u_log, cost, total_cost, x_final, x_ref_log, u_ref_log, B);
    return check_launch(who);
}

}  // namespace

extern "C" {

int hjbx_minsnap_reference_f32(const hjbx_system* sys, const float* coeff, const double* cum_t, const float* end_pt, int S, int64_t n_plans, double t0,
                               int T_steps, float* x_ref, float* u_ref, int64_t B, void* stream) {
    return minsnap_reference_impl<float>(sys, coeff, cum_t, end_pt, S, n_plans, t0, T_steps, x_ref, u_ref, B, stream);
}
int hjbx_minsnap_reference_f64(const hjbx_system* sys, const double* coeff, const double* cum_t, const double* end_pt, int S, int64_t n_plans, double t0,
                               int T_steps, double* x_ref, double* u_ref, int64_t B, void* stream) {
    return minsnap_reference_impl<double>(sys, coeff, cum_t, end_pt, S, n_plans, t0, T_steps, x_ref, u_ref, B, stream);
}
int hjbx_rollout_minsnap_tracking_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_controller* ctrl, int integrator, const float* coeff,
                                      const double* cum_t, const float* end_pt, int S, int64_t n_plans, double t0, int T_steps, const float* x0,
                                      float* traj, float* u_log, float* cost, float* total_cost, float* x_final, float* x_ref_log, float* u_ref_log,
                                      int64_t B, void* stream) {
    return rollout_minsnap_tracking_impl<float>(sys, task, ctrl, integrator, coeff, cum_t, end_pt, S, n_plans, t0, T_steps, x0, traj, u_log, cost,
                                                total_cost, x_final, x_ref_log, u_ref_log, B, stream);
}
int hjbx_rollout_minsnap_tracking_f64(const hjbx_system* sys, const hjbx_task* task, const hjbx_controller* ctrl, int integrator, const double* coeff,
                                      const double* cum_t, const double* end_pt, int S, int64_t n_plans, double t0, int T_steps, const double* x0,
                                      double* traj, double* u_log, double* cost, double* total_cost, double* x_final, double* x_ref_log,
                                      double* u_ref_log, int64_t B, void* stream) {
    return rollout_minsnap_tracking_impl<double>(sys, task, ctrl, integrator, coeff, cum_t, end_pt, S, n_plans, t0, T_steps, x0, traj, u_log, cost,
                                                 total_cost, x_final, x_ref_log, u_ref_log, B, stream);
}

}  // extern "C"
