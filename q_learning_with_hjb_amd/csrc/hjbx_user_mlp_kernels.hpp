// hjbx_user_mlp_kernels.hpp -- the SECOND translation unit hiprtc compiles for a user-defined system, on demand: the two persistent
// matrix-core kernels of the value network (hjbx_mlp_kernels.hpp: k_value_grad_mfma, k_vhjb_rollout_mfma -- the very templates the five
// built-in systems run) instantiated for the user's struct, for ONE head and ONE activation.  A handle asks for it with
// hjbx_system_enable_matrix_cores (include/hjbx.h); the first hjbx_value_grad_f32 / hjbx_vhjb_rollout_f32 / hjbx_softpd_value_grad_f32 /
// hjbx_softpd_rollout_f32 call with that head and activation compiles it (hjbx_user.hip), later calls launch it.  Device code only.
//
// Defined by the host before this file is compiled: what hjbx_user_kernels.hpp needs (HJBX_USER_N / _M / _NP / _KIND and the in-memory
// header "hjbx_user_snippet.hpp"), plus
//   HJBX_USER_MLP_ACT   hjbx_activation of the network: 0 relu, 1 tanh, 2 sin
//   HJBX_USER_MLP_SOFT  0 = PD head (controller/vhjb.py:17-60), 1 = soft-PD head of the notebooks
// Defined HERE for the snippet to see: HJBX_USER_MATRIX_CORE_UNIT.  A snippet may test it to give the matrix-core unit other code than
// the streaming unit (the two must still compute the same function: the fused rollout is bit-identical to value_grad + vhjb_step only
// if vhjb_step_env sees the same expressions in both).
//
// The three kernels of the unit -- value gradient (one tile per wave, eight waves, f32 MFMA), Euler rollout, RK4 rollout -- are explicit
// instantiations; the host finds their symbols through hiprtc's name expressions (HJBX_UM_VALUE_GRAD / HJBX_UM_ROLLOUT_EULER / _RK4 below are those
// expressions, so the host and an offline hipcc -S of this file name the same functions).  The system struct of a user system is the
// opaque array p[HJBX_USER_NP]: the rollout kernel stages it in LDS like every built-in system struct (sys_s), so a p[i] inside the
// user's code is an LDS broadcast read at its point of use and costs no SGPR across the MFMA chains.
#pragma once
#define HJBX_USER_MATRIX_CORE_UNIT 1   // (also keeps hjbx_user_kernels.hpp from emitting the 32 streaming kernels a second time)
#ifndef HJBX_USER_MLP_ACT
#error "compile hjbx_user_mlp_kernels.hpp with -DHJBX_USER_MLP_ACT=0 (relu), 1 (tanh) or 2 (sin)"
#endif
#ifndef HJBX_USER_MLP_SOFT
#error "compile hjbx_user_mlp_kernels.hpp with -DHJBX_USER_MLP_SOFT=0 (PD head) or 1 (soft-PD head)"
#endif
#include "hjbx_user_kernels.hpp"
#include "hjbx_mlp_kernels.hpp"

static_assert(HJBX_USER_N % 2 == 0, "the matrix-core kernels take an even state dimension (k-steps of 2)");
static_assert(HJBX_USER_MLP_ACT == HJBX_ACT_RELU || HJBX_USER_MLP_ACT == HJBX_ACT_TANH || HJBX_USER_MLP_ACT == HJBX_ACT_SIN,
              "fused kernels exist for relu, tanh and sin");

using HjbxUmSys = UserSystem<float>;
#if HJBX_USER_MLP_SOFT
using HjbxUmHead = MlpHeadSoft;
#else
using HjbxUmHead = MlpHeadPd;
#endif
static constexpr int kUmWaves = 8;   // the launch shape of hjbx_mlp.hip: one tile of 32 environments per wave, 8 waves, one workgroup per CU

#define HJBX_UM_VALUE_GRAD k_value_grad_mfma<HjbxUmSys, 1, kUmWaves, HJBX_USER_MLP_ACT, 0, HjbxUmHead>
#define HJBX_UM_ROLLOUT_EULER k_vhjb_rollout_mfma<0, HjbxUmSys, kUmWaves, HJBX_USER_MLP_ACT, 0, HjbxUmHead>
#define HJBX_UM_ROLLOUT_RK4 k_vhjb_rollout_mfma<1, HjbxUmSys, kUmWaves, HJBX_USER_MLP_ACT, 0, HjbxUmHead>

template __global__ void HJBX_UM_VALUE_GRAD(HjbxUmSys, MlpP<HjbxUmSys::N>, const float*, const float*, const float*, const float*, float*,
                                            float*, int64_t, int64_t, HjbxUmHead);
template __global__ void HJBX_UM_ROLLOUT_EULER(HjbxUmSys, MlpP<HjbxUmSys::N>, TaskP<float, HjbxUmSys::N, HjbxUmSys::M>, Limits<float, HjbxUmSys::M>,
                                            const float*, const float*, const float*, int, int, int, const float*, const int32_t*,
                                            RolloutOut<HjbxUmSys::N, HjbxUmSys::M>, int64_t, int64_t, unsigned*, int, HjbxUmHead);
template __global__ void HJBX_UM_ROLLOUT_RK4(HjbxUmSys, MlpP<HjbxUmSys::N>, TaskP<float, HjbxUmSys::N, HjbxUmSys::M>, Limits<float, HjbxUmSys::M>,
                                            const float*, const float*, const float*, int, int, int, const float*, const int32_t*,
                                            RolloutOut<HjbxUmSys::N, HjbxUmSys::M>, int64_t, int64_t, unsigned*, int, HjbxUmHead);
