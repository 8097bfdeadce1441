// hjbx_hessian.hip -- the Hessian of the PD value network with respect to the state, d2V/dx2, and the Jacobian dy/de of its last layer
// (hjbx_value_hessian_f32), on the matrix cores.  The counterpart of jax.hessian / jax.jacobian over the value function in the reference's
// utils/debug_helper.py:7-38 and :40-59 (and the landscape plots of utils/debug_plots.py:145-172).
//
//   e = wrap(x - xf); z = (e - mean)/std; a1 = z W1; h1 = act(a1); a2 = h1 W2; h2 = act(a2); y = h2 W3; V = |y|^2 + eps_s |e|^2
//   reverse sweep:  r2 = 2y W3'; d2 = r2 . act'(a2); r1 = d2 W2'; d1 = r1 . act'(a1); dV/dz = d1 W1'
//   tangent along z_j:  a1. = W1[j,:]; h1. = act'(a1) . a1.; a2. = h1. W2; h2. = act'(a2) . a2.; y. = h2. W3   (row j of dy/dz)
//                       r2. = 2 y. W3'; d2. = r2. . act'(a2) + r2 . act''(a2) . a2.; r1. = d2. W2'; d1. = r1. . act'(a1) + r1 . act''(a1) . a1.
//                       H_z[:,j] = d1. W1'
//   H_x = diag(1/std) H_z diag(1/std) + 2 eps_s I;    dy/de_j = y. / std_j.        (the wrap is data: d wrap = I)
//
// Formulation: the 32 MFMA columns of a tile are (sample, direction) pairs -- C = 32 / n samples, n columns each; the 32 - C n columns left
// over (two for n = 6 and n = 10) compute on the target state and store nothing.  Every column carries its sample's forward and reverse sweep
// (redundantly within the sample) and then the tangent sweep above for its direction j on the SAME five chains as the value gradient
// (mfma_chain with the OffW2F / OffW3F / OffW3B / OffW2B walks of hjbx_mlp_core.hpp over one MlpLds image per workgroup): an accumulator
// register of one product is the B operand of the next, nothing crosses lanes, and the column ends up with column j of its sample's H_z
// (the last product, n useful rows, runs on the VALU as in mlp_value_grad) and row j of dy/dz.  a1. comes from the layer-1 chain with the unit
// vector e_j as its B operand (products with 0 and 1: exact).  H is therefore computed column by column and need not be bitwise symmetric.
// ReLU has act'' = 0: its Hessian is 2 J J' of the active paths and the sample's reverse sweep is not computed at all.
//
// Registers: 64 per 128-wide quantity of a column.  The tangent runs forward first and the sample's reverse sweep only then, so the peak
// (h2, q2 = r2 . act''(a2) . a2., 2 y., r2 . act'(a2) and r1 during the r1 chain; sin keeps cos(a2) next to sin(a2)) is 288 / 352 of the 512 a
// wave of a four-wave workgroup has; layer 1 is recomputed where its activation is needed again (n / 2 x 4 MFMAs) instead of kept.
// LDS: the 106 KB weight image plus the tile counter, one workgroup per CU.  No scratch, no workspace, no communication between workgroups.
// Per sample: n columns x 2 x the value gradient's flop = 8 n (128 n + 128*128 + 128*64) (tanh, sin; ReLU runs 7 of the 10 chains).
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstddef>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"
#include "hjbx_host.hpp"
#include "hjbx_mlp_core.hpp"
#include "hjbx_hessian_kernels.hpp"
#include "hjbx_mlp_host.hpp"

using namespace hjbx;

// Compiled once per activation (-DHJBX_HESS_ACT=0 relu + the C entry point, =1 tanh, =2 sin): seven instantiations each, side by side, of
// k_value_hessian (hjbx_hessian_kernels.hpp, next to mlp_value_hessian: one column of a tile) with the PD head (MlpHeadPd); the checks, the
// launcher and the dispatcher are in hjbx_mlp_host.hpp, shared with hjbx_softpd_hessian.hip.
#ifndef HJBX_HESS_ACT
#error "compile hjbx_hessian.hip with -DHJBX_HESS_ACT=0 (relu + the C entry point), =1 (tanh) and =2 (sin)"
#endif
static constexpr int kAct = HJBX_HESS_ACT;
static_assert(kAct == HJBX_ACT_RELU || kAct == HJBX_ACT_TANH || kAct == HJBX_ACT_SIN, "the Hessian kernel exists for relu, tanh and sin");

#define HJBX_HESS_VARIANTS(X) X(hjbx, 0) X(hjbx, 1) X(hjbx, 2)
HJBX_HESS_VARIANTS(HJBX_HESS_DECLARE_VARIANT)
HJBX_HESS_DEFINE_VARIANT(hjbx, HJBX_HESS_ACT, kAct, MlpHeadPd)

#if HJBX_HESS_ACT == 0
// (variant = hjbx_activation: the checks have refused anything else)
extern "C" int hjbx_value_hessian_f32(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* H, float* dy_dx, int64_t B, void* stream) {
    const char* who = "hjbx_value_hessian_f32";
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    if (const int rc = check_value_hessian(who, sys, net, x, H, dy_dx, B)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (hjbx_user_matrix_cores(sys)) return hjbx_user_value_hessian(sys, net, x, H, dy_dx, B, stream, who);   // (compiled at its first use)
#define HJBX_HESS_ENTRY(prefix, v) prefix##_value_hessian_act##v,
    static mlp_value_hessian_fn* const variants[] = {HJBX_HESS_VARIANTS(HJBX_HESS_ENTRY)};
#undef HJBX_HESS_ENTRY
    return variants[net.activation](sys, net, x, H, dy_dx, B, stream, who);
}
#endif
