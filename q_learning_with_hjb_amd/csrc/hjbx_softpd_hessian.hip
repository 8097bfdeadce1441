// hjbx_softpd_hessian.hip -- the Hessian of the soft-PD value network of the notebooks (SoftPDValueApproximator) with respect to the state,
// d2V/dx2 (hjbx_softpd_value_hessian_f32), on the matrix cores: jax.hessian over the value function in the reference's
// utils/debug_helper.py:40-59, applied to the network of examples/cartpole_balancing.ipynb cell 6.
//
//   e = wrap(x - xf); z = (e - mean)/std; a1 = z W1 + b1; h1 = act(a1); a2 = h1 W2 + b2; h2 = act(a2); a3 = h2 W3 + b3; V = act(a3) . w4 + b4
//   reverse sweep:  d3 = w4 . act'(a3); r2 = d3 W3'; d2 = r2 . act'(a2); r1 = d2 W2'; d1 = r1 . act'(a1); dV/dz = d1 W1'
//   tangent along z_j:  a1. = W1[j,:]; h1. = act'(a1) . a1.; a2. = h1. W2; h2. = act'(a2) . a2.; a3. = h2. W3
//                       d3. = w4 . act''(a3) . a3.; r2. = d3. W3'; d2. = r2. . act'(a2) + r2 . act''(a2) . a2.; r1. = d2. W2'
//                       d1. = r1. . act'(a1) + r1 . act''(a1) . a1.;  H_z[:,j] = d1. W1'
//   H_x = diag(1/std) H_z diag(1/std)                                  (no eps term in this network; the wrap is data: d wrap = I)
//
// The formulation, the ten chains, the LDS walks and the work distribution are those of hjbx_hessian.hip (one column of a tile = one
// (sample, direction) pair, C = 32 / n samples per tile): the same kernel, k_value_hessian of hjbx_hessian_kernels.hpp, with the soft-PD head
// (MlpHeadSoft; mlp_value_hessian with SOFT set): d3 and d3. take the places of 2y and 2y., the accumulators of a1, a2 and a3 start from the
// biases (MlpLdsSoft: the 385 floats of MlpBias next to the weight image), and a3 is a 32-register transient where the PD head holds y.  H is
// the only output.  Per sample: 8 n (128 n + 128*128 + 128*64) flop.  The checks, the launcher and the dispatcher are in hjbx_mlp_host.hpp.
// ReLU has act'' = 0: a scalar piecewise-linear network has H = 0 wherever it is defined, so no ReLU kernel exists and the entry point fills H
// with zeros on the stream.  Compiled once per smooth activation (-DHJBX_SOFTPD_HESS_ACT=1 tanh + the C entry point, =2 sin): seven
// instantiations each; one that needed scratch or spilled a VGPR would fail tests/test_softpd_hessian_host.py.
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

#ifndef HJBX_SOFTPD_HESS_ACT
#error "compile hjbx_softpd_hessian.hip with -DHJBX_SOFTPD_HESS_ACT=1 (tanh + the C entry point) and =2 (sin)"
#endif
static constexpr int kAct = HJBX_SOFTPD_HESS_ACT;
static_assert(kAct == HJBX_ACT_TANH || kAct == HJBX_ACT_SIN, "the soft-PD Hessian kernel exists for tanh and sin (relu: H = 0, filled by the entry point)");

#define HJBX_SOFTPD_HESS_VARIANTS(X) X(hjbx_softpd, 1) X(hjbx_softpd, 2)
HJBX_SOFTPD_HESS_VARIANTS(HJBX_HESS_DECLARE_VARIANT)
HJBX_HESS_DEFINE_VARIANT(hjbx_softpd, HJBX_SOFTPD_HESS_ACT, kAct, MlpHeadSoft)

#if HJBX_SOFTPD_HESS_ACT == 1
extern "C" int hjbx_softpd_value_hessian_f32(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* H, int64_t B, void* stream) {
    const char* who = "hjbx_softpd_value_hessian_f32";
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    if (const int rc = check_value_hessian(who, sys, net, x, H, nullptr, B)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (net.activation == HJBX_ACT_RELU) {   // act'' = 0: H = 0 wherever it is defined (see the top of this file)
        const hipError_t e = hipMemsetAsync(H, 0, sizeof(float) * (size_t)B * (size_t)sys->n * (size_t)sys->n, (hipStream_t)stream);
        if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
        return HJBX_OK;
    }
    if (hjbx_user_matrix_cores(sys)) return hjbx_user_value_hessian(sys, net, x, H, nullptr, B, stream, who);   // (compiled at its first use)
#define HJBX_SOFTPD_HESS_ENTRY(prefix, v) prefix##_value_hessian_act##v,
    static mlp_value_hessian_fn* const variants[] = {nullptr, HJBX_SOFTPD_HESS_VARIANTS(HJBX_SOFTPD_HESS_ENTRY)};   // (variant = hjbx_activation)
#undef HJBX_SOFTPD_HESS_ENTRY
    return variants[net.activation](sys, net, x, H, nullptr, B, stream, who);
}
#endif
