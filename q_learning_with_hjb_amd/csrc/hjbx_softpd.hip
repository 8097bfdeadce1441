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
static constexpr int kWaves = 8;   // launch shape of hjbx_mlp.hip: one tile of 32 environments per wave, 8 waves per workgroup, one per CU

#define HJBX_SOFTPD_VARIANTS(X) X(hjbx_softpd, 0) X(hjbx_softpd, 1) X(hjbx_softpd, 2)
HJBX_SOFTPD_VARIANTS(HJBX_MLP_DECLARE_VARIANT)
HJBX_MLP_DEFINE_VARIANT(hjbx_softpd, HJBX_SOFTPD_ACT, 1, kWaves, kAct, 0, MlpHeadSoft)

#if HJBX_SOFTPD_ACT == 0
// (variant = hjbx_activation: the checks have refused anything else)
extern "C" int hjbx_softpd_value_grad_f32(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* V, float* g, int64_t B,
                                          void* stream) {
    const char* who = "hjbx_softpd_value_grad_f32";
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    if (const int rc = check_value_grad(who, sys, net, x, V, g, B)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (hjbx_user_matrix_cores(sys)) return hjbx_user_value_grad(sys, net, x, V, g, B, stream, who);
#define HJBX_SOFTPD_ENTRY(prefix, v) prefix##_value_grad_act##v,
    static mlp_value_grad_fn* const variants[] = {HJBX_SOFTPD_VARIANTS(HJBX_SOFTPD_ENTRY)};
#undef HJBX_SOFTPD_ENTRY
    return variants[net.activation](sys, net, x, V, g, B, stream, who);
}

extern "C" int hjbx_softpd_rollout_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_softpd_mlp* mlp, int integrator, int t_first,
                                       int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                                       int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace, void* stream) {
    const char* who = "hjbx_softpd_rollout_f32";
    if (!sys || !task || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system, task or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    const hjbx_rollout_args a{integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B, workspace, stream};
    if (const int rc = check_rollout(who, sys, task, net, a)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (hjbx_user_matrix_cores(sys)) return hjbx_user_rollout(sys, task, net, a, who);
#define HJBX_SOFTPD_ENTRY(prefix, v) prefix##_rollout_act##v,
    static mlp_rollout_fn* const variants[] = {HJBX_SOFTPD_VARIANTS(HJBX_SOFTPD_ENTRY)};
#undef HJBX_SOFTPD_ENTRY
    return variants[net.activation](sys, task, net, a, who);
}
#endif
