// hjbx_internal.hpp -- definitions shared by the translation units of libhjbx.so (not part of the ABI)
#pragma once
#include "../../include/hjbx.h"

// the opaque handle of include/hjbx.h: what Dynamics.__init__ stores (dynamics_basic.py:17-26)
struct hjbx_system {
    int kind, n, m;
    double dt;
    double umin[HJBX_MAX_M], umax[HJBX_MAX_M];
    double p[2 * (HJBX_MAX_N * HJBX_MAX_N + HJBX_MAX_N * HJBX_MAX_M)];  // packing documented at hjbx_system_kind
    int n_params;
    void* user;   // HJBX_SYS_USER: the run-time compiled program (hjbx_user.hip); NULL otherwise
};

// HJBX_SYS_USER (hjbx_user.hip): launch an extern "C" kernel of the handle's code object (args[0] points at the system blob), and free it
int hjbx_user_launch(const hjbx_system* s, const char* kernel, unsigned grid, void** args, void* stream);
void hjbx_user_release(void* user_program);

// The value network of either head as every launcher of the two matrix-core kernels takes it (hjbx_mlp_host.hpp: make_net converts the ABI's
// hjbx_mlp / hjbx_softpd_mlp, the shared argument checks and the launchers of the built-in systems read it; hjbx_user.hip: the launchers
// of a user-defined system).
struct hjbx_net {
    int soft, activation;                     // 0 = PD head (hjbx_mlp), 1 = soft-PD head (hjbx_softpd_mlp); hjbx_activation
    int h1, h2, h3;                           // features
    const double *mean, *std, *xf;            // (n) each
    double eps_scalar;                        // PD head only (0 for the soft-PD head)
    const float *W1, *W2, *W3;                // device pointers
    const float *b1, *b2, *b3, *w4, *b4;      // soft-PD head only
};
// what a fused rollout takes after the descriptors, in the order of hjbx_vhjb_rollout_f32 / hjbx_softpd_rollout_f32
struct hjbx_rollout_args {
    int integrator, t_first, n_steps, T_max;
    const float* x;
    float *traj, *u_log, *cost, *done, *resid;
    int32_t* done_step;
    float* x_out;
    const int32_t* env_order;
    int64_t B;
    void *workspace, *stream;
};

// HJBX_SYS_USER handles that asked for the matrix-core kernels (hjbx_system_enable_matrix_cores): the two launchers of hjbx_user.hip --
// called by the four C entry points of hjbx_mlp.hip / hjbx_softpd.hip AFTER their argument checks; the first call for a (head, activation)
// compiles the kernels.  `who` names the entry point in messages.
bool hjbx_user_matrix_cores(const hjbx_system* s);
int hjbx_user_value_grad(const hjbx_system* s, const hjbx_net& net, const float* x, float* V, float* g, int64_t B, void* stream, const char* who);
int hjbx_user_rollout(const hjbx_system* s, const hjbx_task* task, const hjbx_net& net, const hjbx_rollout_args& a, const char* who);
// The Hessian of the value network for such a handle: called by hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 AFTER
// check_value_hessian (and after the soft-PD entry point's ReLU memset: no soft-PD ReLU unit exists).  The first call for a (head, activation)
// compiles the handle's Hessian unit (hjbx_user_hessian_kernels.hpp: k_value_hessian<UserSystem<float>, kHessWaves, activation, head>);
// HJBX_EUNSUPPORTED when the kernel needs scratch (the refusal is remembered, nothing is launched), HJBX_EINVAL when the source does not
// compile there.  dy = NULL for the soft-PD head.
int hjbx_user_value_hessian(const hjbx_system* s, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* stream, const char* who);

// The parameter gradient of such a handle (hjbx_train_coop.hip calls both after the entry points' argument checks).  hjbx_user_train_unit:
// the handle's train unit for `activation` (hjbx_user_train_kernels.hpp: k_train_coop<0|1, activation, 1|4, UserSystem<float>>), compiled now
// if this is the first request; HJBX_EUNSUPPORTED when the handle is not enabled or one of the four kernels needs scratch (the whole unit is
// refused and the refusal remembered), HJBX_EINVAL when the source does not compile there.  hjbx_user_train_launch: enqueue the kernel for
// (mode 0 | 1, psplit 1 | 4) with `grid` workgroups of 256 threads; args = pointers to the kernel's arguments in order (args[0] points at the
// system blob, as for hjbx_user_launch).
int hjbx_user_train_unit(const hjbx_system* s, int activation, const char* who);
int hjbx_user_train_launch(const hjbx_system* s, int activation, int mode, int psplit, unsigned grid, void** args, void* stream, const char* who);

// records the calling thread's error message and returns `code`
int hjbx_set_error(int code, const char* fmt, ...);

// current value of a hjbx_option (hjbx_set_option), 0 for an unknown one
int hjbx_option_value(int option);

// the cooperative single-kernel parameter gradient (hjbx_train_coop.hip), called by hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 after
// argument validation.  fuse == NULL: the partial sums are reduced into `flat`; fuse != NULL (hjbx_adam.hpp): reduced, mixed and applied to the
// weights by Adam in the same epilogue kernel, `flat` unused
struct FuseArgs;
int hjbx_train_coop(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int mode, const float* x, const float* cost, const float* done,
                    float* flat, void* workspace, int64_t B, void* stream, const FuseArgs* fuse);
size_t hjbx_train_coop_workspace_bytes(int64_t B, int n);
