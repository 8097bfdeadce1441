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
//    VALU, its W1' rows fetched in groups by the same kind of asm read and counted wait (left to the compiler it was one
//    exposed LDS latency per feature pair; the chains' own prologues, by contrast, cost nothing measurable: DESIGN 4.2).
//    The activation is a template parameter: ReLU (one integer max) or tanh (exp2 + rcp).
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

// This file is compiled once per variant (-DHJBX_MLP_ACT=0 relu, =1 tanh, =2 relu with the bf16x3-split arithmetic of hjbx_mlp_x3.hpp,
// =3 relu with the f16x2-split arithmetic of hjbx_mlp_h2.hpp, =4 sin: 30 kernel instantiations each, side by side); the relu object also
// carries the two C entry points, which validate and hand over to the object of the requested variant.  The kernels (k_value_grad_mfma: V
// and dV/dx for a batch of states; k_vhjb_rollout_mfma: the whole VHJB closed loop for n_steps steps in one launch) are in
// hjbx_mlp_kernels.hpp, the checks, launchers and dispatchers in hjbx_mlp_host.hpp, instantiated here with the PD head (MlpHeadPd).
#ifndef HJBX_MLP_ACT
#error "compile hjbx_mlp.hip with -DHJBX_MLP_ACT=0 (relu + the C entry points), =1 (tanh), =2 (relu, bf16x3-split MFMA), =3 (relu, f16x2-split MFMA) and =4 (sin)"
#endif
static constexpr int kArith = HJBX_MLP_ACT == 2 ? 1 : HJBX_MLP_ACT == 3 ? 2 : 0;  // 0 = f32 MFMA, 1 = bf16x3, 2 = f16x2 (HJBX_OPT_MLP_ARITHMETIC)
static constexpr int kAct = kArith ? HJBX_ACT_RELU : HJBX_MLP_ACT == 4 ? HJBX_ACT_SIN : HJBX_MLP_ACT;
static_assert(kAct == HJBX_ACT_RELU || kAct == HJBX_ACT_TANH || kAct == HJBX_ACT_SIN, "fused kernels exist for relu, tanh and sin");
#ifndef HJBX_MLP_TL
#define HJBX_MLP_TL 1
#endif
#ifndef HJBX_MLP_WAVES
#define HJBX_MLP_WAVES 8
#endif

#define HJBX_MLP_VARIANTS(X) X(hjbx_mlp, 0) X(hjbx_mlp, 1) X(hjbx_mlp, 2) X(hjbx_mlp, 3) X(hjbx_mlp, 4)
HJBX_MLP_VARIANTS(HJBX_MLP_DECLARE_VARIANT)
HJBX_MLP_DEFINE_VARIANT(hjbx_mlp, HJBX_MLP_ACT, HJBX_MLP_TL, HJBX_MLP_WAVES, kAct, kArith, MlpHeadPd)

#if HJBX_MLP_ACT == 0
extern "C" size_t hjbx_rollout_workspace_bytes(void) { return (size_t)kWsWords * sizeof(unsigned); }

// a user-defined system that asked for the matrix-core kernels (hjbx_system_enable_matrix_cores) gets them compiled at run time, in the
// float32 MFMA arithmetic only
static int check_user_arithmetic(const char* who) {
    if (hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC) == 0) return HJBX_OK;
    return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: HJBX_OPT_MLP_ARITHMETIC=%d (split-operand MFMA) is not compiled for user-defined systems; set it to 0", who,
                          hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC));
}
// the object that serves a network: tanh and sin in float32, relu in the arithmetic of HJBX_OPT_MLP_ARITHMETIC
static int variant_of(const hjbx_net& net) {
    if (net.activation == HJBX_ACT_TANH) return 1;
    if (net.activation == HJBX_ACT_SIN) return 4;
    const int arith = hjbx_option_value(HJBX_OPT_MLP_ARITHMETIC);
    return arith == 1 ? 2 : arith == 2 ? 3 : 0;
}

extern "C" int hjbx_value_grad_f32(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* V, float* g, int64_t B,
                                   void* stream) {
    const char* who = "hjbx_value_grad_f32";
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    if (const int rc = check_value_grad(who, sys, net, x, V, g, B)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (hjbx_user_matrix_cores(sys)) {
        if (int rc = check_user_arithmetic(who)) return rc;
        return hjbx_user_value_grad(sys, net, x, V, g, B, stream, who);
    }
#define HJBX_MLP_ENTRY(prefix, v) prefix##_value_grad_act##v,
    static mlp_value_grad_fn* const variants[] = {HJBX_MLP_VARIANTS(HJBX_MLP_ENTRY)};
#undef HJBX_MLP_ENTRY
    return variants[variant_of(net)](sys, net, x, V, g, B, stream, who);
}

extern "C" int hjbx_vhjb_rollout_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int integrator, int t_first,
                                     int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done,
                                     float* resid, int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace,
                                     void* stream) {
    const char* who = "hjbx_vhjb_rollout_f32";
    if (!sys || !task || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system, task or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    const hjbx_rollout_args a{integrator, t_first, n_steps, T_max, x, traj, u_log, cost, done, resid, done_step, x_out, env_order, B, workspace, stream};
    if (const int rc = check_rollout(who, sys, task, net, a)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (hjbx_user_matrix_cores(sys)) {
        if (int rc = check_user_arithmetic(who)) return rc;
        return hjbx_user_rollout(sys, task, net, a, who);
    }
#define HJBX_MLP_ENTRY(prefix, v) prefix##_rollout_act##v,
    static mlp_rollout_fn* const variants[] = {HJBX_MLP_VARIANTS(HJBX_MLP_ENTRY)};
#undef HJBX_MLP_ENTRY
    return variants[variant_of(net)](sys, task, net, a, who);
}
#endif
