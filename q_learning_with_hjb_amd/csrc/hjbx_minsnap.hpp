// hjbx_minsnap.hpp -- device side of the min-snap waypoint planner of Quadrotors2D (reference
// controller/quadrotors_model_based_controller.py:77-233) and of the tracking closed loop built on it.  One lane = one environment.
//
// The host solves the coefficients (float64 NumPy, quadrotors_model_based_controller.py of this package); the device evaluates
// `update(t)`: segment selection (:218-228), derivatives 0..4 of the two 7th-order polynomials (:161-176, :189-198) and the differential
// flatness map to [x, y, theta, xd, yd, thetad] and the two rotor thrusts (:200-214).  The formulas are the reference's, statement by
// statement, INCLUDING its theta_ddot expression, whose last term is not the exact second derivative of theta: u_ref
// is the reference's feedforward, not an exact one.
//
// Two kernels call the one device function minsnap_eval, so the reference logs of a tracking rollout are bit-equal to the reference generator:
//   k_minsnap_reference<T>               threads over environment x step -> x_ref (T, B, 6), u_ref (T, B, 2)
//   k_rollout_minsnap_tracking<INTEG, T>  one thread per environment, state in registers, u = clip(u_ref - K wrap(x - x_ref)), time-major logs
// No host code in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjbx_systems.hpp"
#include "hjbx_stream_kernels.hpp"

namespace hjbx {

HJBX_DEV float atan2_t(float y, float x) { return atan2f(y, x); }
HJBX_DEV double atan2_t(double y, double x) { return atan2(y, x); }

static constexpr int kMinsnapTerms = 8;   // a 7th-order polynomial per axis and segment

// The plans on the device, in the reference's layout: coeff (n_plans, 2, S, 8) ascending powers, cum_t (n_plans, S + 1) = cumulated_t,
// end_pt (n_plans, 2) = points[-1].  Times stay double in both precisions: the segment and the local time t - cum_t[i] are found exactly
// as the float64 planner finds them, and only the local time is rounded to T.  stride = 0: one plan shared by every environment, 1: one each.
template <typename T> struct MinsnapPlan {
    const T* coeff;
    const double* cum_t;
    const T* end_pt;
    int64_t stride;
    int S;
};

// the segment a lane is in: its time interval [t_lo, t_hi) and the 16 coefficients (hover: the end point and zeros, local time 0)
template <typename T> struct MinsnapSegment {
    double t_lo = 1.0, t_hi = 0.0;   // empty: the first minsnap_eval selects
    T c[2][kMinsnapTerms];
    bool hover;
};

// :218-228.  index = the last i with t >= cumulated_t[i], found by a scan whose result lies in [0, S] whatever cum_t holds (a NaN or
// unsorted plan cannot send a load outside coeff); index == S is the hover past the last waypoint.  Nothing is read while t stays inside
// the interval selected last (cumulated_t is a cumulative sum of non-negative durations: the scan would return the same index).
template <typename T> HJBX_DEV void minsnap_select(const MinsnapPlan<T>& plan, int64_t env, double t, MinsnapSegment<T>& seg) {
    if (t >= seg.t_lo && t < seg.t_hi) return;
    const int S = plan.S;
    const int64_t p = env * plan.stride;
    const double* ct = plan.cum_t + p * (S + 1);
    int idx = 0;
    double lo = ct[0];
    for (int i = 1; i <= S; ++i) {
        const double v = ct[i];
        if (t >= v) { idx = i; lo = v; }
    }
    seg.t_lo = lo;
    seg.hover = idx == S;
    if (seg.hover) {
        seg.t_hi = __builtin_huge_val();
        T end[2];
        RowIO<T, 2>::load(plan.end_pt, p, end);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            seg.c[d][0] = end[d];
#pragma unroll
            for (int k = 1; k < kMinsnapTerms; ++k) seg.c[d][k] = T(0);
        }
    } else {
        seg.t_hi = ct[idx + 1];
        RowIO<T, kMinsnapTerms>::load(plan.coeff, (p * 2 + 0) * S + idx, seg.c[0]);
        RowIO<T, kMinsnapTerms>::load(plan.coeff, (p * 2 + 1) * S + idx, seg.c[1]);
    }
}

// get_polynomial_term (:161-176) folded into Horner's rule: the D-th derivative of sum_i c_i tau^i is sum_{i >= D} c_i i!/(i-D)! tau^(i-D)
constexpr int minsnap_falling(int i, int D) { return D == 0 ? 1 : i * minsnap_falling(i - 1, D - 1); }
template <int D, typename T> HJBX_DEV T minsnap_poly(const T* c, T tau) {
    T acc = c[kMinsnapTerms - 1] * T(minsnap_falling(kMinsnapTerms - 1, D));
#pragma unroll
    for (int i = kMinsnapTerms - 2; i >= D; --i) acc = acc * tau + c[i] * T(minsnap_falling(i, D));
    return acc;
}

// flat_output_to_full_states_and_inputs_2D (:178-216), in the reference's operation order
template <typename T> HJBX_DEV void minsnap_flat_to_state(const Quad2D<T>& sys, const MinsnapSegment<T>& seg, T tau, T* x_ref, T* u_ref) {
    const T x0 = minsnap_poly<0>(seg.c[0], tau), y0 = minsnap_poly<0>(seg.c[1], tau);
    const T x1 = minsnap_poly<1>(seg.c[0], tau), y1 = minsnap_poly<1>(seg.c[1], tau);
    const T x2 = minsnap_poly<2>(seg.c[0], tau), y2 = minsnap_poly<2>(seg.c[1], tau);
    const T x3 = minsnap_poly<3>(seg.c[0], tau), y3 = minsnap_poly<3>(seg.c[1], tau);
    const T x4 = minsnap_poly<4>(seg.c[0], tau), y4 = minsnap_poly<4>(seg.c[1], tau);
    const T den = y2 + sys.g;
    const T den2 = den * den, den3 = den2 * den;
    const T ratio = x2 / den;
    const T one_r2 = T(1) + ratio * ratio;
    const T w = x3 / den - x2 * y3 / den2;
    const T theta = -atan2_t(x2, den);
    const T theta_dot = T(-1) / one_r2 * w;
    const T theta_ddot = T(2) * x2 / den / (one_r2 * one_r2) * (w * w) -
                         T(1) / one_r2 * (x4 / den - x3 * y3 / den2 - x3 * y3 / den2 - x2 * y4 / den2 + T(2) * x2 * y3 / den3);
    x_ref[0] = x0; x_ref[1] = y0; x_ref[2] = theta; x_ref[3] = x1; x_ref[4] = y1; x_ref[5] = theta_dot;
    T s, c;
    sincos_t(theta, &s, &c);
    const T torque = sys.I / sys.r * theta_ddot, ntorque = -sys.I / sys.r * theta_ddot;
    T lift;
    if (!(s == T(0))) lift = -(sys.m / s * x2);       // :207-209 (taken wherever x_ddot != 0)
    else lift = sys.m / c * (y2 + sys.g);             // :211-212 (the hover tail, and any instant with x_ddot == 0)
    u_ref[0] = (torque + lift) / T(2);
    u_ref[1] = (ntorque + lift) / T(2);
}

// update(t) (:218-233) for environment `env`
template <typename T>
HJBX_DEV void minsnap_eval(const Quad2D<T>& sys, const MinsnapPlan<T>& plan, int64_t env, double t, MinsnapSegment<T>& seg, T* x_ref, T* u_ref) {
    minsnap_select(plan, env, t, seg);
    const T tau = seg.hover ? T(0) : (T)(t - seg.t_lo);
    minsnap_flat_to_state(sys, seg, tau, x_ref, u_ref);
}

// the tracking law's constants: K of the hover LQR (2, 6), Q (6, 6) and R (2, 2) of the step cost
template <typename T> struct TrackP { T K[2 * 6], Q[6 * 6], R[2 * 2]; };

// ----------------------------------------------------------------------------------------------
// x_ref (T_steps, B, 6), u_ref (T_steps, B, 2) at t_k = t0 + k dt (formed in double, never accumulated); row = k B + env
// ----------------------------------------------------------------------------------------------
template <typename T>
HJBX_DEV void k_minsnap_reference_body(Quad2D<T> sys, MinsnapPlan<T> plan, double t0, double dt, int64_t rows, T* __restrict__ x_ref,
                                       T* __restrict__ u_ref, int64_t B) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    const int64_t k = row / B, env = row - k * B;
    MinsnapSegment<T> seg;
    T xr[6], ur[2];
    minsnap_eval(sys, plan, env, t0 + (double)k * dt, seg, xr, ur);
    if (x_ref) RowIO<T, 6>::store(x_ref, row, xr);
    if (u_ref) RowIO<T, 2>::store(u_ref, row, ur);
}

// ----------------------------------------------------------------------------------------------
// the tracking closed loop: for k < T_steps: (x_ref, u_ref) = update(t0 + k dt); e = wrap(x - x_ref); u = clip(u_ref - K e);
// cost_k = (e'Qe + (u - u_ref)'R(u - u_ref)) dt; x = simulate(x, u).  Logs are time-major, every output may be NULL:
// traj (T_steps + 1, B, 6), u_log (T_steps, B, 2), cost (T_steps, B), total_cost (B), x_final (B, 6), x_ref_log / u_ref_log as above.
// ----------------------------------------------------------------------------------------------
template <int INTEG, typename T>
HJBX_DEV void k_rollout_minsnap_tracking_body(Quad2D<T> sys, MinsnapPlan<T> plan, TrackP<T> tp, Limits<T, 2> lim, int want_cost, int T_steps,
                                              double t0, double dt, const T* __restrict__ x0, T* __restrict__ traj, T* __restrict__ u_log,
                                              T* __restrict__ cost, T* __restrict__ total_cost, T* __restrict__ x_final,
                                              T* __restrict__ x_ref_log, T* __restrict__ u_ref_log, int64_t B) {
    constexpr int N = 6, M = 2;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    T x[N], xn[N], xr[N], ur[M], e[N], u[M];
    RowIO<T, N>::load(x0, i, x);
    MinsnapSegment<T> seg;
    T tot = T(0);
    for (int k = 0; k < T_steps; ++k) {
        const int64_t row = (int64_t)k * B + i;
        if (traj) RowIO<T, N>::store(traj, row, x);
        minsnap_eval(sys, plan, i, t0 + (double)k * dt, seg, xr, ur);
        error_coords(sys, xr, x, e);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            T acc = T(0);
#pragma unroll
            for (int q = 0; q < N; ++q) acc += tp.K[j * N + q] * e[q];
            u[j] = clamp_t(ur[j] - acc, lim.umin[j], lim.umax[j]);
        }
        if (want_cost) {
            T du[M];
#pragma unroll
            for (int j = 0; j < M; ++j) du[j] = u[j] - ur[j];
            const T c = (quad_form<N>(tp.Q, e) + quad_form<M>(tp.R, du)) * lim.dt;
            tot += c;
            if (cost) cost[row] = c;
        }
        if (u_log) RowIO<T, M>::store(u_log, row, u);
        if (x_ref_log) RowIO<T, N>::store(x_ref_log, row, xr);
        if (u_ref_log) RowIO<T, M>::store(u_ref_log, row, ur);
        integrate<INTEG>(sys, lim.dt, x, u, xn);
#pragma unroll
        for (int q = 0; q < N; ++q) x[q] = xn[q];
    }
    if (traj) RowIO<T, N>::store(traj, (int64_t)T_steps * B + i, x);
    if (total_cost) total_cost[i] = tot;
    if (x_final) RowIO<T, N>::store(x_final, i, x);
}

}  // namespace hjbx
