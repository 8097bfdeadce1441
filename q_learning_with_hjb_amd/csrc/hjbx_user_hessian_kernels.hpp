// hjbx_user_hessian_kernels.hpp -- the FOURTH translation unit hiprtc compiles for a user-defined system, on demand: the Hessian kernel of
// the value network (hjbx_hessian_kernels.hpp: k_value_hessian -- the very template the built-in systems run; reference
// utils/debug_helper.py:40-59, jax.hessian over the value function) instantiated for the user's struct, for ONE head and ONE activation.  A
// handle that asked for the matrix-core kernels (hjbx_system_enable_matrix_cores, include/hjbx.h) gets it at the first
// hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 call with that head and activation (hjbx_user.hip); later calls launch it.
// Device code only.
//
// Defined by the host before this file is compiled: what hjbx_user_kernels.hpp needs (HJBX_USER_N / _M / _NP / _KIND and the in-memory
// header "hjbx_user_snippet.hpp"), plus
//   HJBX_USER_MLP_ACT   hjbx_activation of the network: 0 relu, 1 tanh, 2 sin
//   HJBX_USER_MLP_SOFT  0 = PD head (controller/vhjb.py:17-60), 1 = soft-PD head of the notebooks (tanh and sin: a soft-PD ReLU network has
//                       H = 0 and no kernel, the entry point fills H with zeros)
// Defined HERE for the snippet to see: HJBX_USER_MATRIX_CORE_UNIT (as in hjbx_user_mlp_kernels.hpp) and HJBX_USER_HESSIAN_UNIT.
//
// The one kernel of the unit is an explicit instantiation; the host finds its symbol through hiprtc's name expression (HJBX_UH_VALUE_HESSIAN
// below IS that expression, so the host and an offline hipcc -S of this file name the same function).  The kernel takes S::N and S::wrap
// from the system and nothing else.  One wave per SIMD, 512 registers: a kernel that does not fit them spills to scratch, and the host
// refuses the unit (hjbx_user.hip).  A unit of its own: the matrix-core unit keeps its three kernels and the train unit its four.
#pragma once
#define HJBX_USER_MATRIX_CORE_UNIT 1   // (also keeps hjbx_user_kernels.hpp from emitting the 32 streaming kernels a second time)
#define HJBX_USER_HESSIAN_UNIT 1
#ifndef HJBX_USER_MLP_ACT
#error "compile hjbx_user_hessian_kernels.hpp with -DHJBX_USER_MLP_ACT=0 (relu), 1 (tanh) or 2 (sin)"
#endif
#ifndef HJBX_USER_MLP_SOFT
#error "compile hjbx_user_hessian_kernels.hpp with -DHJBX_USER_MLP_SOFT=0 (PD head) or 1 (soft-PD head)"
#endif
#include "hjbx_user_kernels.hpp"
#include "hjbx_hessian_kernels.hpp"

static_assert(HJBX_USER_N % 2 == 0, "the matrix-core kernels take an even state dimension (k-steps of 2)");
static_assert(HJBX_USER_MLP_ACT == HJBX_ACT_RELU || HJBX_USER_MLP_ACT == HJBX_ACT_TANH || HJBX_USER_MLP_ACT == HJBX_ACT_SIN,
              "the Hessian kernel exists for relu, tanh and sin");
static_assert(!(HJBX_USER_MLP_SOFT && HJBX_USER_MLP_ACT == HJBX_ACT_RELU),
              "the soft-PD Hessian of a ReLU network is identically zero: there is no soft-PD ReLU unit");

using HjbxUhSys = UserSystem<float>;
#if HJBX_USER_MLP_SOFT
using HjbxUhHead = MlpHeadSoft;
#else
using HjbxUhHead = MlpHeadPd;
#endif

#define HJBX_UH_VALUE_HESSIAN k_value_hessian<HjbxUhSys, kHessWaves, HJBX_USER_MLP_ACT, HjbxUhHead>

template __global__ void HJBX_UH_VALUE_HESSIAN(HjbxUhSys, MlpP<HjbxUhSys::N>, const float*, const float*, const float*, const float*, float*,
                                               float*, int64_t, int64_t, HjbxUhHead);
