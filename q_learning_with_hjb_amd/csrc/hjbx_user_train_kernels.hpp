// hjbx_user_train_kernels.hpp -- the THIRD translation unit hiprtc compiles for a user-defined system, on demand: the cooperative
// parameter-gradient kernel of the value-learning step (hjbx_train_coop_kernels.hpp: k_train_coop -- the very template the five built-in
// systems run; reference controller/vhjb.py:227-253, 282-284) instantiated for the user's struct, for ONE activation.  PD head only (the
// soft-PD network trains through autograd).  A handle that asked for the matrix-core kernels (hjbx_system_enable_matrix_cores,
// include/hjbx.h) gets it at the first hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 call with that activation (hjbx_user.hip);
// later calls launch it.  Device code only.
//
// Defined by the host before this file is compiled: what hjbx_user_kernels.hpp needs (HJBX_USER_N / _M / _NP / _KIND and the in-memory
// header "hjbx_user_snippet.hpp"), plus
//   HJBX_USER_MLP_ACT   hjbx_activation of the network: 0 relu, 1 tanh, 2 sin (sin: n <= 4, as for the built-in systems)
// Defined HERE for the snippet to see: HJBX_USER_MATRIX_CORE_UNIT (as in hjbx_user_mlp_kernels.hpp) and HJBX_USER_TRAIN_UNIT.
//
// The four kernels of the unit -- residual mode 0 / 1 x PS 1 (large batch: one workgroup per tile) / 4 (minibatch: four workgroups per
// tile) -- are explicit instantiations; the host finds their symbols through hiprtc's name expressions (the HJBX_UT_* macros below ARE those
// expressions, so the host and an offline hipcc -S of this file name the same functions).  One wave per SIMD, 512 registers: a kernel
// that does not fit them spills to scratch, and the host refuses the whole unit (hjbx_user.hip).  The reduce / update epilogues depend on N
// only and are launched from the library.
#pragma once
#define HJBX_USER_MATRIX_CORE_UNIT 1   // (also keeps hjbx_user_kernels.hpp from emitting the 32 streaming kernels a second time)
#define HJBX_USER_TRAIN_UNIT 1
#ifndef HJBX_USER_MLP_ACT
#error "compile hjbx_user_train_kernels.hpp with -DHJBX_USER_MLP_ACT=0 (relu), 1 (tanh) or 2 (sin)"
#endif
#include "hjbx_user_kernels.hpp"
#include "hjbx_train_coop_kernels.hpp"

static_assert(HJBX_USER_N % 2 == 0, "the matrix-core kernels take an even state dimension (k-steps of 2)");
static_assert(HJBX_USER_MLP_ACT == HJBX_ACT_RELU || HJBX_USER_MLP_ACT == HJBX_ACT_TANH || HJBX_USER_MLP_ACT == HJBX_ACT_SIN,
              "fused kernels exist for relu, tanh and sin");
static_assert(HJBX_USER_MLP_ACT != HJBX_ACT_SIN || HJBX_USER_N <= 4, "the sin network's fused parameter gradient exists for n <= 4");

using HjbxUtSys = UserSystem<float>;

#define HJBX_UT_M0_PS1 k_train_coop<0, HJBX_USER_MLP_ACT, 1, HjbxUtSys>
#define HJBX_UT_M0_PS4 k_train_coop<0, HJBX_USER_MLP_ACT, 4, HjbxUtSys>
#define HJBX_UT_M1_PS1 k_train_coop<1, HJBX_USER_MLP_ACT, 1, HjbxUtSys>
#define HJBX_UT_M1_PS4 k_train_coop<1, HJBX_USER_MLP_ACT, 4, HjbxUtSys>

#define HJBX_UT_ARGS                                                                                                                      \
    (HjbxUtSys, MlpP<HjbxUtSys::N>, TaskP<float, HjbxUtSys::N, HjbxUtSys::M>, Limits<float, HjbxUtSys::M>, const float*, const float*,  \
     const float*, const float*, const float*, const float*, float, float*, float*, double*, int64_t, int64_t)
template __global__ void HJBX_UT_M0_PS1 HJBX_UT_ARGS;
template __global__ void HJBX_UT_M0_PS4 HJBX_UT_ARGS;
template __global__ void HJBX_UT_M1_PS1 HJBX_UT_ARGS;
template __global__ void HJBX_UT_M1_PS4 HJBX_UT_ARGS;
