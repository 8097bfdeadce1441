/*
 * hjbx.h -- C ABI of libhjbx.so: MI355X (gfx950) batched control-affine rollouts + HJB residuals.
 *
 * This is the drop-in boundary for the hot path of HaoxiangYou/Q_Learning_with_HJB (SURVEY.md
 * section 8b).  The reference has no FFI: its "operator API" is two Python base classes
 * (dynamics/dynamics_basic.py:7-122 `Dynamics`, controller/controller_basic.py:1-5 `Controller`)
 * plus the math inside controller/vhjb.py.  Each entry point below names the reference statement(s)
 * it replaces; q_learning_with_hjb_amd/_abi.py is the ctypes binding a maintainer would add
 * (INTEGRATION.md shows the reference-side patch).
 *
 * Conventions
 *  - Every array argument is a raw DEVICE pointer (hipMalloc / torch.Tensor.data_ptr()) to a
 *    contiguous row-major buffer; `hjbx_task` / `hjbx_controller` / `hjbx_mlp` descriptors are
 *    HOST structs read during the call (copied into kernel arguments).  No torch types cross.
 *  - State batches are (B, n) row-major ("batch_size, state_dim": dynamics_basic.py:58-60),
 *    controls (B, m), f2 (B, n, m).  Trajectory slabs are time-major: (T+1, B, n).
 *  - `_f32` entry points take float buffers, `_f64` double buffers.  Descriptor fields are double
 *    and are rounded to float once per call for `_f32`.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are enqueued and
 *    the call returns; nothing here synchronises, allocates device memory or copies to the host.
 *  - Return value: HJBX_OK (0) or a negative hjbx_status.  hjbx_last_error() gives the message of
 *    the calling thread's last failure.  No C++ exception crosses this boundary.
 *  - Handles are immutable after creation and may be shared between host threads.
 */
#ifndef HJBX_H
#define HJBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HJBX_VERSION 112 /* major*100 + minor */
#define HJBX_HAS_REPLAY_APPEND 1 /* hjbx_replay_append_f32 / _f64 exist (added without a version step: an addition, nothing else changed) */
#define HJBX_HAS_USER_MATRIX_CORES 1 /* hjbx_system_enable_matrix_cores / hjbx_system_matrix_cores / hjbx_system_code_object exist (an addition) */
#define HJBX_HAS_USER_TRAIN 1 /* hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 take an enabled user-defined system; HJBX_CODE_TRAIN exists (an addition) */
#define HJBX_HAS_USER_VALUE_HESSIAN 1 /* hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 take an enabled user-defined system; HJBX_CODE_HESSIAN exists (an addition) */
#define HJBX_MAX_N 10    /* largest state dimension (NearHoverQuadcopter) */
#define HJBX_MAX_M 3     /* largest control dimension */

typedef enum hjbx_status {
    HJBX_OK = 0,
    HJBX_EINVAL = -1,       /* bad argument (NULL pointer, bad size, bad enum) */
    HJBX_EUNSUPPORTED = -2, /* valid request this build has no kernel for */
    HJBX_EHIP = -3,         /* HIP runtime error (message carries hipGetErrorString) */
    HJBX_ENODEVICE = -4     /* no usable gfx950 device */
} hjbx_status;

/* Which dynamics class of the reference the handle stands for. */
typedef enum hjbx_system_kind {
    HJBX_SYS_LINEAR = 0,    /* dynamics/linear.py:7-22      params = A (n*n row-major), B (n*m) [, Ad (n*n), Bd (n*m) for HJBX_ZOH] */
    HJBX_SYS_CARTPOLE = 1,  /* dynamics/cartpole.py:10-64   params = mc, mp, l, g                    */
    HJBX_SYS_ACROBOT = 2,   /* dynamics/acrobot.py:19-81    params = m1, m2, l1, l2, I1, I2, g       */
    HJBX_SYS_QUAD2D = 3,    /* dynamics/quadrotors.py:9-70  params = m, r, I, g                      */
    HJBX_SYS_NEARHOVER = 4, /* dynamics/quadrotors.py:102-170 params = g, m, kT, n0                  */
    HJBX_SYS_USER = 5       /* a user-defined Dynamics subclass: created by hjbx_system_create_from_source only */
} hjbx_system_kind;

/* What a user-defined system supplies (hjbx_system_create_from_source). */
typedef enum hjbx_user_kind {
    HJBX_USER_AFFINE = 0,      /* the subclass overrides get_control_affine_matrix (like dynamics/linear.py:20-22, quadrotors.py:17-46):
                                  the source defines wrap(x) and affine(x, f1, f2) */
    HJBX_USER_MANIPULATOR = 1  /* the subclass defines get_M / get_C / get_G / get_B and inherits the generic manipulator form
                                  f1 = [dq; -inv(M)(C dq + G)], f2 = [0; inv(M) B] (dynamics/dynamics_basic.py:64-94): the source
                                  defines wrap(x), get_M, get_C, get_G, get_B; n even, q = x[:n/2] */
} hjbx_user_kind;
#define HJBX_USER_MAX_PARAMS 16

typedef enum hjbx_integrator {
    HJBX_EULER = 0, /* x' = wrap(x + dt*xdot): the reference's integrator, dynamics_basic.py:120 (parity mode) */
    HJBX_RK4 = 1,   /* classic RK4 with zero-order-hold control, wrap applied once at the end (new mode)         */
    HJBX_ZOH = 2    /* LINEAR systems only: exact zero-order-hold step x' = Ad x + Bd u, the discretisation the
                       reference's LQR / time-optimal notebooks use (scipy.signal.cont2discrete:
                       examples/double_integrator_optimal_time.ipynb cell 4); needs Ad, Bd in the handle          */
} hjbx_integrator;

typedef enum hjbx_residual_mode {
    HJBX_RESIDUAL_NORMALISED = 0, /* |gradV.xdot/(l+eps) + 1| (1-done): controller/vhjb.py:233       */
    HJBX_RESIDUAL_RAW = 1         /* |gradV.xdot + l| (1-done): examples/cartpole_balancing.ipynb cell 11; with
                                     HJBX_LAW_BANGBANG and done = 0 this is pd_hjb_loss of the time-optimal notebook (cell 11) */
} hjbx_residual_mode;

/* How u is obtained from gradV, and which running cost goes with it (hjbx_task.law). */
typedef enum hjbx_control_law {
    HJBX_LAW_QUADRATIC = 0, /* u = clip(-Rinv f2' gradV / 2 + uf), l = e'Qe + (u-uf)'R(u-uf): controller/vhjb.py:162-165, 218-220 */
    HJBX_LAW_BANGBANG = 1   /* time-optimal learning (examples/double_integrator_optimal_time.ipynb cells 7, 9, 11):
                               u_j = umax_j if (f2' gradV)_j < 0, umin_j if > 0, 0 if == 0  (= -sign(gradV @ B) for +-1 limits);
                               l = 1 outside the target ball e'e > target_r2, 0 inside; rollouts end inside the ball
                               (terminal tuple, cost e'Pe) as well as outside the observation box; d u / d gradV = 0 */
} hjbx_control_law;

typedef enum hjbx_controller_kind {
    HJBX_CTRL_LINEAR_FEEDBACK = 0, /* u = clip(-K e + uf): controller/lqr.py:25-26, quadrotors_model_based_controller.py:36-38, 73-75 */
    HJBX_CTRL_CARTPOLE_ENERGY = 1, /* controller/cartpole_energy_shaping.py:65-110 */
    HJBX_CTRL_ACROBOT_ENERGY = 2,  /* controller/acrobot_energy_shaping.py:74-121  */
    HJBX_CTRL_DI_TIME_OPTIMAL = 3  /* double integrator (LINEAR n=2, m=1), analytic bang-bang law with its switching curve:
                                      get_analytical_control, examples/double_integrator_optimal_time.ipynb cell 18;
                                      u = 0 inside the target ball e'e <= eps_region, else +-umax */
} hjbx_controller_kind;

/* rollout flags */
#define HJBX_ROLLOUT_TERMINATE 1u /* stop an environment when wrap(x-xf) leaves [obs_min, obs_max] (vhjb.py:176-181) */
#define HJBX_ROLLOUT_STOP_AT_TARGET 2u /* stop an environment once e'e <= ctrl.eps_region, e = x - ctrl.xf, checked before
                                          the control of each step (time-to-origin loops of the time-optimal notebook,
                                          cell 9); done_step = index of that step */

/* Process-wide tuning / test knobs (hjbx_set_option; a negative value queries).  Options 0-2 do not change results. */
typedef enum hjbx_option {
    HJBX_OPT_ROLLOUT_SCHEDULE = 0,         /* work distribution of hjbx_vhjb_rollout_f32: 0 (default) = equal static shares per workgroup, with
                                              the shares of workgroups that have not started taken over by the waves that finish first;
                                              1 = device-wide tile queue (one atomic per 32-environment tile) */
    HJBX_OPT_ROLLOUT_EXTRA_WORKGROUPS = 1, /* TEST HOOK: launch this many workgroups more than there are CUs (they cannot be resident until
                                              others finish -- the situation the take-over above exists for); default 0 */
    HJBX_OPT_STREAM_ROWS = 2,              /* TUNING: rows per thread of the float32 streaming kernels (simulate, vhjb_step, hjb_residual):
                                              1, 2 or 4; 0 (default) = the library's choice */
    HJBX_OPT_MLP_ARITHMETIC = 3            /* arithmetic of the ReLU value network inside hjbx_value_grad_f32 / hjbx_vhjb_rollout_f32 and of the eight
                                              128 / 64-wide products of hjbx_value_loss_grad_f32 (mode 1 runs those on the f32 MFMA) (THE ONE KNOB
                                              THAT CHANGES RESULTS, within float32 rounding; inputs, outputs, accumulation, layer 1 and everything
                                              outside the network are float32 in every mode; tanh and sin networks always run mode 0):
                                              0 (DEFAULT) = float32 MFMA, bitwise an fmaf chain: the arithmetic of the reference's float32 network
                                                  (controller/vhjb.py:17-60);
                                              1 = OPT-IN bf16x3: every float32 operand split EXACTLY into three bfloat16 pieces, the six largest piece
                                                  products on the bf16 matrix cores (dropped products <= 2^-23 of each term);
                                              2 = OPT-IN f16x2: every operand scaled by a power of two (ONE exponent per weight matrix; one per
                                                  environment and product for the activations) and rounded to two float16 pieces, the three
                                                  largest piece products on the f16 matrix cores.  An operand within 2^16 of its scaling maximum
                                                  keeps 22 significant bits (perturbation <= 3 x 2^-22 = 7e-7 of its term); a smaller one loses
                                                  low bits of its lo piece (float16 subnormals), i.e. the error bound is ABSOLUTE: 2^-39 of the
                                                  matrix's largest |weight| (of the environment's largest activation) per operand, so one outlier
                                                  weight 2^17 above the rest degrades every other entry of its matrix.
                                              Modes 1 and 2 are faster and narrower than the reference's arithmetic: never the default.
                                              tests/test_gpu_f32_parity.py runs every test in every mode against the same bounds, and
                                              test_fused_value_grad_split_arithmetics_stay_within_their_stated_bound checks modes 1 / 2 against
                                              mode 0 on the device. */,
    HJBX_OPT_TRAIN_KERNEL = 4              /* implementation of hjbx_value_loss_grad_f32 in the float32 arithmetic (results agree to float32 summation
                                              order): 0 (default) = the cooperative single kernel (no scratch in HBM, a tile's chains split over the four
                                              waves of a workgroup; ReLU, tanh, sin); 1 = the round-2 pair of kernels (chains + outer products through a
                                              5-KB-per-sample scratch; ReLU only) -- kept for A/B measurements and for the f16x2 arithmetic */
} hjbx_option;

typedef struct hjbx_system hjbx_system; /* opaque */

/* Task = the cost / target / observation-box part of VHJBControllerConfig
 * (configs/controller/vhjb_controller_config.py:47-55) plus P from vhjb.py:156-160. Row-major,
 * only the leading n*n / m*m / n / m entries are read. */
typedef struct hjbx_task {
    double Q[HJBX_MAX_N * HJBX_MAX_N];
    double R[HJBX_MAX_M * HJBX_MAX_M];
    double Rinv[HJBX_MAX_M * HJBX_MAX_M];
    double P[HJBX_MAX_N * HJBX_MAX_N]; /* terminal cost e'Pe, vhjb.py:167-169 */
    double xf[HJBX_MAX_N];
    double uf[HJBX_MAX_M];
    double obs_min[HJBX_MAX_N]; /* bounds on the error coordinates wrap(x-xf), strict compares */
    double obs_max[HJBX_MAX_N];
    double eps;                 /* VHJBControllerConfig.epsilon */
    int32_t law;                /* hjbx_control_law; 0 = the reference's VHJBController */
    int32_t _pad;
    double target_r2;           /* HJBX_LAW_BANGBANG: squared radius of the target ball ("metric", notebook cell 7) */
} hjbx_task;

/* Closed-form feedback laws. */
typedef struct hjbx_controller {
    int32_t kind;       /* hjbx_controller_kind */
    int32_t wrap_error; /* LINEAR_FEEDBACK: e = wrap_error ? wrap(x-xf) : x-xf */
    double K[HJBX_MAX_M * HJBX_MAX_N]; /* (m, n) row-major state-feedback gain */
    double xf[HJBX_MAX_N];
    double uf[HJBX_MAX_M];
    double P[HJBX_MAX_N * HJBX_MAX_N]; /* ACROBOT_ENERGY: LQR region is e'Pe < eps_region */
    double Kes[3];      /* energy-shaping gains (cartpole [4,4,10], acrobot [1,2,1]) */
    double eps_energy;  /* CARTPOLE_ENERGY: |E-E(xf)| < eps_energy ... */
    double eps_state;   /* ... and ||(dtheta_err, dtheta_dot)|| < eps_state selects the LQR branch */
    double eps_region;  /* ACROBOT_ENERGY: LQR region; DI_TIME_OPTIMAL / STOP_AT_TARGET: squared radius of the target ball */
} hjbx_controller;

typedef enum hjbx_activation {
    HJBX_ACT_RELU = 0, /* controller/vhjb.py:52,56 and examples/drone_hovering.ipynb, 10D_quadcopte.ipynb */
    HJBX_ACT_TANH = 1, /* examples/cartpole_balancing.ipynb cell 6 */
    HJBX_ACT_SIN = 2   /* examples/double_integrator_optimal_time.ipynb cell 5 (sin and cos evaluated to 1e-7 absolute for pre-activations
                          |a| <= 1e3, bounded by 1 for every finite one: see hjbx_activation_probe_f32) */
} hjbx_activation;

/* Value network of controller/vhjb.py:17-60 (no bias, BatchNorm off): device weight pointers,
 * Flax Dense layout (in, out) row-major, y = x @ W. */
typedef struct hjbx_mlp {
    const void* W1; /* (n,  h1) */
    const void* W2; /* (h1, h2) */
    const void* W3; /* (h2, h3) */
    int32_t h1, h2, h3;
    int32_t activation;      /* hjbx_activation between the Dense layers */
    double mean[HJBX_MAX_N]; /* normalization_mean */
    double std[HJBX_MAX_N];  /* normalization_std  */
    double xf[HJBX_MAX_N];
    double eps_scalar;       /* epsilon_scalar */
} hjbx_mlp;

/* Soft-PD value network of the notebooks (SoftPDValueApproximator: examples/cartpole_balancing.ipynb cell 6, drone_hovering.ipynb cell 6,
 * double_integrator_optimal_time.ipynb cell 5, 10D_quadcopte.ipynb cell 6): Dense layers WITH biases and a scalar output,
 *   h1 = act(z W1 + b1), h2 = act(h1 W2 + b2), h3 = act(h2 W3 + b3), V = h3 . w4 + b4,   z = (wrap(x - xf) - mean) / std
 * (no eps |e|^2 term; positivity is only encouraged by the training loss).  Device pointers, Flax Dense layout (in, out) row-major. */
typedef struct hjbx_softpd_mlp {
    const void* W1; /* (n,  h1) */
    const void* b1; /* (h1) */
    const void* W2; /* (h1, h2) */
    const void* b2; /* (h2) */
    const void* W3; /* (h2, h3) */
    const void* b3; /* (h3) */
    const void* w4; /* (h3, 1) */
    const void* b4; /* (1) */
    int32_t h1, h2, h3;
    int32_t activation;      /* hjbx_activation, applied after each of the three hidden layers */
    double mean[HJBX_MAX_N]; /* normalization_mean */
    double std[HJBX_MAX_N];  /* normalization_std  */
    double xf[HJBX_MAX_N];
} hjbx_softpd_mlp;

/* ---- library / handles --------------------------------------------------------------------- */
int hjbx_version(void);
/* Copies the calling thread's last error message (NUL terminated) into buf; returns its length. */
size_t hjbx_last_error(char* buf, size_t buflen);
/* Number of visible HIP devices whose arch is gfx950 (0 when there is none / no driver). */
int hjbx_device_count(void);
/* Sets a hjbx_option and returns its previous value (value < 0: query only); HJBX_EINVAL for an unknown option. */
int hjbx_set_option(int option, int value);

/* Replaces Dynamics.__init__ + subclass __init__ (dynamics_basic.py:17-26 etc.). */
int hjbx_system_create(int kind, int n, int m, double dt, const double* umin, const double* umax,
                       const double* params, int n_params, hjbx_system** out);
void hjbx_system_destroy(hjbx_system* sys);
/* The OPEN half of the reference's plugin surface: "any subclass of Dynamics" (dynamics/dynamics_basic.py:7-122).  `device_source` is the text
 * of the subclass's per-state methods as device code (member functions of a struct template on the scalar type T with the parameters in
 * p[0..n_params-1]; the exact contract is at the top of csrc/hjbx_user_kernels.hpp).  It is compiled at run time (hiprtc, gfx950, the
 * library's own build flags) INTO THE LIBRARY'S OWN STREAMING KERNELS, float32 and float64: the returned handle works with every
 * hjbx_*_f32 / _f64 entry point of the HJBX_DECLARE block below (wrap, affine, dynamics_step, simulate with HJBX_EULER / HJBX_RK4,
 * initial_state, costs, control_from_grad, hjb_residual, vhjb_step, controller and rollout_feedback with HJBX_CTRL_LINEAR_FEEDBACK; any other law: hjbx_user_controller_create below).
 * The matrix-core entry points (hjbx_value_grad_f32, hjbx_vhjb_rollout_f32, the two hjbx_softpd_* ones, hjbx_value_loss_grad_f32) return
 * HJBX_EUNSUPPORTED for such a handle unless it asked for them (hjbx_system_enable_matrix_cores below).  Compilation needs no GPU.  HJBX_EINVAL when the source does not compile
 * (hjbx_last_compile_log returns the compiler's messages for the calling thread's last call), HJBX_EUNSUPPORTED when libhiprtc.so
 * is not available. */
int hjbx_system_create_from_source(int user_kind, const char* device_source, int n, int m, double dt, const double* umin,
                                   const double* umax, const double* params, int n_params, hjbx_system** out);
size_t hjbx_last_compile_log(char* buf, size_t buflen);
/* The value network on the matrix cores for a user-defined system: the subclass of Dynamics (dynamics_basic.py:64-94) under the reference's
 * VHJBController (controller/vhjb.py:17-60 the network, :201-202 its input gradient, :162-193 the closed loop).  Marks a HJBX_SYS_USER
 * handle as wanting the two persistent matrix-core kernels: from then on hjbx_value_grad_f32, hjbx_vhjb_rollout_f32,
 * hjbx_softpd_value_grad_f32 and hjbx_softpd_rollout_f32 accept it, with the arguments, workspace, chunking and env_order contract they
 * have for the built-in systems (HJBX_EULER / HJBX_RK4; the fused rollout is bit-identical to value_grad + hjbx_vhjb_step_f32 per step).
 * Nothing is compiled here: the first of those calls for a (head, activation) compiles the user's source into the kernels of
 * csrc/hjbx_user_mlp_kernels.hpp (hiprtc, seconds, once per handle; a source that does not compile there: HJBX_EINVAL +
 * hjbx_last_compile_log; kernels that would spill registers to scratch: HJBX_EUNSUPPORTED; either way the handle keeps working with the
 * streaming entry points and the refusal is remembered).  float32 MFMA arithmetic only: with HJBX_OPT_MLP_ARITHMETIC != 0 the PD entry
 * points return HJBX_EUNSUPPORTED for such a handle.  The same call opens hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 to the handle
 * (a third unit, compiled at their first call: see there).  Call it before the handle is shared between threads.
 * HJBX_EUNSUPPORTED when n is odd (the kernels walk the state in k-steps of 2); HJBX_EINVAL for a built-in handle. */
int hjbx_system_enable_matrix_cores(hjbx_system* sys);
/* 1 when the handle is a user-defined system with the matrix-core kernels enabled, 0 otherwise (built-in systems included). */
int hjbx_system_matrix_cores(const hjbx_system* sys);
/* The gfx950 code objects (ELF) a user-defined system runs (dynamics_basic.py:64-94 compiled; vhjb.py:17-60, 162-193, 201-202 for the
 * matrix-core units), for inspection: copies up to `len` bytes into buf (may be NULL) and returns the object's size.  `which` =
 * HJBX_CODE_STREAMING, HJBX_CODE_MATRIX_CORES(head, activation) with head 0 = hjbx_mlp, 1 = hjbx_softpd_mlp, or HJBX_CODE_TRAIN(activation):
 * the parameter-gradient unit of hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 (four kernels), or HJBX_CODE_HESSIAN(head, activation):
 * the value-Hessian unit of hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 (one kernel; HJBX_EUNSUPPORTED for head 1 with
 * HJBX_ACT_RELU: that H is identically zero and has no kernel) -- compiled now if it has not been yet.  Returns 0 on failure
 * (hjbx_last_error; hjbx_last_compile_log when the compiler refused the source). */
#define HJBX_CODE_STREAMING 0
#define HJBX_CODE_MATRIX_CORES(head, activation) (1 + 3 * (head) + (activation))
#define HJBX_CODE_TRAIN(activation) (7 + (activation))
#define HJBX_CODE_HESSIAN(head, activation) (10 + 3 * (head) + (activation))
size_t hjbx_system_code_object(const hjbx_system* sys, int which, void* buf, size_t len);
/* Dynamics.get_dimension, dynamics_basic.py:31-36 */
int hjbx_dims(const hjbx_system* sys, int* n, int* m);
/* Bytes of device scratch the reducing entry points need (hjb_residual, termination_residual).  The workspace holds the
 * per-workgroup partial sums and the arrival counters of the in-kernel final reduction: it must be 16-byte aligned and ZERO-FILLED
 * ONCE after allocation (hipMemset); every call leaves the counters at zero again, so no per-call memset is needed.  One
 * workspace serves one stream at a time (calls on the same stream may share it; concurrent streams need one each). */
size_t hjbx_reduce_workspace_bytes(void);

#define HJBX_DECLARE(T, SFX)                                                                          \
    /* Dynamics.get_control_affine_matrix (dynamics_basic.py:64-94, linear.py:20-22,                 \
       quadrotors.py:17-46, 118-149): f1 (B,n), f2 (B,n,m). */                                       \
    int hjbx_affine_##SFX(const hjbx_system* sys, const T* x, T* f1, T* f2, int64_t B, void* stream); \
    /* Dynamics.states_wrap (cartpole.py:52-64, acrobot.py:72-81, quadrotors.py:48-70, 151-170);     \
       out may alias x (the NumPy branch of the reference wraps in place). */                        \
    int hjbx_wrap_##SFX(const hjbx_system* sys, const T* x, T* out, int64_t B, void* stream);         \
    /* Dynamics.dynamics_step (dynamics_basic.py:96-105): xdot = f1 + f2 u, u NOT clipped. */         \
    int hjbx_dynamics_step_##SFX(const hjbx_system* sys, const T* x, const T* u, T* xdot, int64_t B,  \
                                 void* stream);                                                       \
    /* Dynamics.simulate (dynamics_basic.py:107-122): u clipped to [umin,umax], one integrator step, \
       wrap.  x_next may alias x. */                                                                  \
    int hjbx_simulate_##SFX(const hjbx_system* sys, int integrator, const T* x, const T* u,           \
                            T* x_next, int64_t B, void* stream);                                      \
    /* Dynamics.get_initial_state (dynamics_basic.py:28-29) for B environments:                      \
       x0 = wrap(-x0_std + 2 x0_std * u01 + x0_mean); u01 (B,n) are caller-supplied uniforms so the   \
       RNG stays with the caller (the reference uses NumPy's global MT19937). */                      \
    int hjbx_initial_state_##SFX(const hjbx_system* sys, const double* x0_mean, const double* x0_std, \
                                 const T* u01, T* x0, int64_t B, void* stream);                       \
    /* VHJBController.running_cost (vhjb.py:162-165): cost (B,) = e'Qe + (u-uf)'R(u-uf). */           \
    int hjbx_running_cost_##SFX(const hjbx_system* sys, const hjbx_task* task, const T* x,            \
                                const T* u, T* cost, int64_t B, void* stream);                        \
    /* VHJBController.termination_cost (vhjb.py:167-169): cost (B,) = e'Pe. */                        \
    int hjbx_termination_cost_##SFX(const hjbx_system* sys, const hjbx_task* task, const T* x,        \
                                    T* cost, int64_t B, void* stream);                                \
    /* Control law of get_control_efforts_with_additional_term (vhjb.py:218-220):                    \
       u = clip(-Rinv f2' gradV / 2 + uf, umin, umax). */                                             \
    int hjbx_control_from_grad_##SFX(const hjbx_system* sys, const hjbx_task* task, const T* x,       \
                                     const T* gradV, T* u, int64_t B, void* stream);                  \
    /* hjb_loss body (vhjb.py:227-241) forward + analytic d(loss_i)/d(gradV).           \
       done (B,) is the 0/1 mask as T.  loss_i (B,) and dloss_dgrad (B,n) may be NULL.                \
       sums[0..2] = {sum loss_i, sum (1-done), sum done}, reduced deterministically (fixed order, no  \
       float atomics) inside the same launch through the caller's workspace (see                      \
       hjbx_reduce_workspace_bytes()); sums may be NULL. */                    \
    int hjbx_hjb_residual_##SFX(const hjbx_system* sys, const hjbx_task* task, int mode, const T* x,  \
                                const T* gradV, const T* done, T* loss_i, T* dloss_dgrad, T* sums,    \
                                void* workspace, int64_t B, void* stream);                            \
    /* termination_loss body (vhjb.py:243-253): loss_i = |V/(cost+eps) - 1| done,                    \
       dloss_dV = sign(.) done/(cost+eps); sums as above. */                                          \
    int hjbx_termination_residual_##SFX(double eps, const T* V, const T* cost, const T* done,         \
                                        T* loss_i, T* dloss_dV, T* sums, void* workspace, int64_t B,  \
                                        void* stream);                                                \
    /* One iteration of rollout_trajectory's loop (vhjb.py:175-191) for B environments, given the    \
       value gradient of the current states.  step t in [0,T]: environments with done_step<0 are     \
       live.  A live env outside the observation box (or t==T) emits (cost=e'Pe, done=1), latches    \
       done_step=t and holds its state; otherwise u from gradV, cost=l(x,u)*dt, done=0, x_next=       \
       simulate(x,u).  Dead envs emit cost=0, done=0 and hold.  done_step (B,) int32 must be          \
       initialised to -1 before t=0.  u_out may be NULL.  resid_t (B,) may be NULL; when given it     \
       receives the normalised HJB residual gradV.xdot/(l+eps) + 1 (vhjb.py:233, signed, before the   \
       abs) of every live, non-terminating environment at its current state and 0 elsewhere -- the    \
       residual comes for free here because u, xdot and l are already in registers. */                \
    int hjbx_vhjb_step_##SFX(const hjbx_system* sys, const hjbx_task* task, int integrator, int t,    \
                             int T_max, const T* x, const T* gradV, T* x_next, T* u_out, T* cost_t,   \
                             T* done_t, int32_t* done_step, T* resid_t, int64_t B, void* stream);     \
    /* Controller.get_control_efforts for the closed-form controllers, u (B,m). */      \
    int hjbx_controller_##SFX(const hjbx_system* sys, const hjbx_controller* ctrl, const T* x, T* u,  \
                              int64_t B, void* stream);                                               \
    /* Whole closed loop in one kernel: for t in 0..T-1: u=ctrl(x); log; x=simulate(x,u)              \
       (scripts/test_vhjb_policy.py:143-151, cartpole_energy_shaping.py:123-125).  With              \
       HJBX_ROLLOUT_TERMINATE it follows rollout_trajectory (vhjb.py:171-193) with `task`:            \
       per-step cost l*dt, terminal e'Pe, done_step.  Outputs (any may be NULL):                      \
       traj (T+1,B,n) time-major states, u_log (T,B,m), cost (T+1,B), done_step (B,) int32,           \
       total_cost (B,) sum of the emitted costs (get_trajectory_cost, vhjb.py:195-199).               \
       task may be NULL when neither cost nor TERMINATE is requested. */                              \
    int hjbx_rollout_feedback_##SFX(const hjbx_system* sys, const hjbx_task* task,                    \
                                    const hjbx_controller* ctrl, int integrator, uint32_t flags,      \
                                    int T_steps, const T* x0, T* traj, T* u_log, T* cost,             \
                                    int32_t* done_step, T* total_cost, T* x_final, int64_t B,         \
                                    void* stream);

HJBX_DECLARE(float, f32)
HJBX_DECLARE(double, f64)
#undef HJBX_DECLARE

/* ValueFunctionApproximator.__call__ + get_v_gradient (vhjb.py:17-60, 201-202) fused on the matrix
 * cores: V (B,) and gradV (B,n) = dV/dx in one pass, weights staged in LDS.  f32 only (the JAX side
 * of the reference is float32).  V or gradV may be NULL. */
int hjbx_value_grad_f32(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* V,
                        float* gradV, int64_t B, void* stream);

/* rollout_trajectory (vhjb.py:171-193) for B environments, `n_steps` consecutive iterations t = t_first ..
 * t_first+n_steps-1 of its loop in ONE launch: per step the value gradient (as hjbx_value_grad_f32, weights staged
 * in LDS once per launch) followed by exactly hjbx_vhjb_step_f32's per-environment code; the state stays in
 * registers between steps.  Bit-identical to calling those two entry points n_steps times.
 *   x (B,n): states at step t_first.            done_step (B,) int32 in/out (-1 = live), as hjbx_vhjb_step.
 *   traj (n_steps+1,B,n) or NULL: slab k = state at step t_first+k (slab 0 = x).     x_out (B,n) or NULL: final state.
 *   cost, done (n_steps,B): the tuples emitted at each step.   resid (n_steps,B) or NULL.   u_log (n_steps,B,m) or NULL.
 * A whole reference rollout is t_first = 0, n_steps = T_max + 1 (the last iteration emits the forced terminal tuple).
 *   env_order (B,) int32 or NULL: a permutation of 0..B-1 = the order in which environments are packed into the 32-wide
 *   tiles of the kernel (all arrays stay indexed by environment).  A tile whose environments have all finished skips the
 *   value network and only writes its log rows, so listing the live environments first (a stable sort by done_step >= 0,
 *   refreshed between launches) makes a batch in which most environments have terminated cost what its live part
 *   costs.  Results do not depend on the order.
 *   x may be the same buffer as slab 0 of traj (each row is written back with the value just read).
 *   workspace: hjbx_rollout_workspace_bytes() bytes of 16-byte aligned device memory, ZERO-FILLED ONCE after allocation; the
 *   kernel keeps its work-distribution words there and leaves them zeroed.  One workspace per stream in flight. */
size_t hjbx_rollout_workspace_bytes(void);
int hjbx_vhjb_rollout_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int integrator, int t_first,
                          int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done,
                          float* resid, int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace,
                          void* stream);

/* The soft-PD network (hjbx_softpd_mlp) in the two fused kernels above: V (B,) and gradV (B,n) as hjbx_value_grad_f32 (V or gradV may be NULL),
 * and the closed loop with exactly the arguments, chunking (t_first, n_steps), in-place done_step, logs, x_out, env_order and rollout
 * workspace of hjbx_vhjb_rollout_f32 (bit-identical to hjbx_softpd_value_grad_f32 + hjbx_vhjb_step_f32 per step).  Always the float32 MFMA
 * arithmetic: HJBX_OPT_MLP_ARITHMETIC does not apply.  Features [128,128,64]; built-in systems, and user-defined ones after
 * hjbx_system_enable_matrix_cores (HJBX_EUNSUPPORTED otherwise).  There is no fused parameter gradient for this network: it is trained through autograd. */
int hjbx_softpd_value_grad_f32(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* V, float* gradV, int64_t B,
                               void* stream);
int hjbx_softpd_rollout_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_softpd_mlp* mlp, int integrator, int t_first,
                            int n_steps, int T_max, const float* x, float* traj, float* u_log, float* cost, float* done, float* resid,
                            int32_t* done_step, float* x_out, const int32_t* env_order, int64_t B, void* workspace, void* stream);

/* The Hessian of the PD value network (hjbx_mlp) with respect to the state, and the Jacobian of its last layer: what the reference takes
 * from jax.hessian / jax.jacobian in utils/debug_helper.py:40-59 (local_optimal_x) and :7-38 (the equivalent linear map of a ReLU network),
 * and what the landscape plots of utils/debug_plots.py:145-172 are drawn from.
 *   H (B,n,n) or NULL:      H[b,i,j] = d2V / dx_i dx_j at x_b = diag(1/std) H_z diag(1/std) + 2 eps_scalar I, with
 *                           H_z = 2 J_z J_z' + A2. diag(r2 . act''(a2)) A2.' + A1. diag(r1 . act''(a1)) A1.'  (J_z = dy/dz, A1. = da1/dz, A2. = da2/dz,
 *                           r2, r1 the reverse sweep of hjbx_value_grad_f32; act'' = 0 for relu, -2h(1-h^2) for tanh, -h for sin).
 *   dy_dx (B,n,h3) or NULL: dy_dx[b,i,:] = dy / de_i, y the output of the last layer, e = wrap(x - xf) the error coordinates.
 * The wrap is data (d wrap = I), as in hjbx_value_grad_f32.  For relu H is piecewise constant and both outputs jump where a hidden unit
 * crosses zero.  H is computed column by column (each column is one tangent sweep through the network): it is symmetric up to rounding and
 * NOT bitwise symmetric.  Results are deterministic: two calls on the same input agree bit for bit.
 * Always the float32 MFMA arithmetic (HJBX_OPT_MLP_ARITHMETIC does not apply).  Features [128,128,64]; relu, tanh and sin; the built-in
 * systems hjbx_value_grad_f32 dispatches, and a user-defined system (HJBX_SYS_USER) whose handle asked for the matrix-core kernels
 * (hjbx_system_enable_matrix_cores): the first call for an activation compiles the same kernel for the user's struct
 * (csrc/hjbx_user_hessian_kernels.hpp: hiprtc, seconds, once per handle; HJBX_CODE_HESSIAN(0, activation) returns the code object).  A
 * kernel that would need scratch is never launched: HJBX_EUNSUPPORTED, the refusal is remembered and the handle keeps its other kernels;
 * HJBX_EINVAL + hjbx_last_compile_log when the source does not compile there.  A user-defined system that has not asked returns
 * HJBX_EUNSUPPORTED.  No workspace.
 * x must be aligned to its row vector width, H and dy_dx to 16 bytes.  B == 0 or both outputs NULL: HJBX_OK, nothing is launched. */
#define HJBX_HAS_VALUE_HESSIAN 1 /* the entry point below exists (an addition, nothing else changed) */
int hjbx_value_hessian_f32(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* H /* (B,n,n) or NULL */,
                           float* dy_dx /* (B,n,h3) or NULL */, int64_t B, void* stream);

/* The Hessian of the soft-PD value network (hjbx_softpd_mlp) with respect to the state: what jax.hessian over the value function gives in
 * the reference's utils/debug_helper.py:40-59 (local_optimal_x) when the controller carries the notebooks' SoftPDValueApproximator.
 *   e = wrap(x - xf); z = (e - mean)/std; a1 = z W1 + b1; h1 = act(a1); a2 = h1 W2 + b2; h2 = act(a2); a3 = h2 W3 + b3; V = act(a3) . w4 + b4
 *   reverse sweep:  d3 = w4 . act'(a3); r2 = d3 W3'; d2 = r2 . act'(a2); r1 = d2 W2'; d1 = r1 . act'(a1); dV/dz = d1 W1'
 *   tangent along z_j:  a1. = W1[j,:]; h1. = act'(a1) . a1.; a2. = h1. W2; h2. = act'(a2) . a2.; a3. = h2. W3
 *                       d3. = w4 . act''(a3) . a3.; r2. = d3. W3'; d2. = r2. . act'(a2) + r2 . act''(a2) . a2.; r1. = d2. W2'
 *                       d1. = r1. . act'(a1) + r1 . act''(a1) . a1.;  H_z[:,j] = d1. W1'
 *   H (B,n,n):  H[b,i,j] = d2V / dx_i dx_j at x_b = diag(1/std) H_z diag(1/std)   (no eps term in this network), in closed form
 *               H_z = A3 diag(w4 . act''(a3)) A3' + A2 diag(r2 . act''(a2)) A2' + A1 diag(r1 . act''(a1)) A1',
 *               A1 = W1, A2 = (A1 . act'(a1)) W2, A3 = (A2 . act'(a2)) W3.
 * The wrap is data (d wrap = I).  H is computed column by column: it is symmetric up to rounding, not bitwise.  Two calls on the same input
 * agree bit for bit.  ReLU has act'' = 0, so the scalar piecewise-linear network has H = 0 wherever it is defined: there is no ReLU kernel,
 * the entry point fills H with zeros on the stream.  tanh and sin run on the matrix cores (float32 MFMA; HJBX_OPT_MLP_ARITHMETIC does not
 * apply) for the built-in systems hjbx_softpd_value_grad_f32 dispatches; a (system, activation) pair whose kernel would need scratch is
 * refused with HJBX_EUNSUPPORTED and a message that names it (none at present).  A user-defined system whose handle asked for the
 * matrix-core kernels (hjbx_system_enable_matrix_cores) runs the same kernel, compiled for its struct at the first call for an activation
 * (HJBX_CODE_HESSIAN(1, activation); scratch and compile failures as for hjbx_value_hessian_f32; relu compiles nothing, H is zero-filled);
 * one that has not asked returns HJBX_EUNSUPPORTED.
 * Features [128,128,64].  No workspace.  x must be aligned to its row vector width, H to 16 bytes.  B == 0 or H == NULL: HJBX_OK, nothing
 * is launched. */
#define HJBX_HAS_SOFTPD_VALUE_HESSIAN 1 /* the entry point below exists (an addition, nothing else changed) */
int hjbx_softpd_value_hessian_f32(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* H /* (B,n,n) */, int64_t B,
                                  void* stream);

/* The parameter gradient of one value-learning step (vhjb.py:227-253 and the jax.grad calls of :282-284) for a minibatch of B samples
 * (x (B,n), cost (B,), done (B,) as 0/1 floats), fused on the matrix cores:
 *   flat = [ d(sum_b hjb_loss_b)/dW1 (n,h1) | /dW2 (h1,h2) | /dW3 (h2,h3) | d(sum_b termination_loss_b)/dW1 | /dW2 | /dW3 |
 *            sum_b hjb_loss_b, sum_b termination_loss_b, sum_b (1-done_b), sum_b done_b ]                  (2P + 4 floats)
 * i.e. the gradients of the loss SUMS (the caller divides by the counts, vhjb.py:241, 253, and mixes with the regularisation weight,
 * :284) -- the buffer a data-parallel step all-reduces once.  hjb_loss is a function of dV/dx, so its gradient is a second-order
 * reverse sweep; both are evaluated in closed form (no autograd graph).  `mode` = hjbx_residual_mode.  Deterministic: no float atomics,
 * fixed summation order (the order depends on B and the device's CU count only).  ReLU, tanh and (state dimension <= 4) sin networks with features [128,128,64]
 * (HJBX_EUNSUPPORTED otherwise: the PyTorch autograd path remains); W1, W2, W3 16-byte aligned.  workspace: hjbx_value_loss_grad_workspace_bytes(B) bytes (it depends on
 * HJBX_OPT_MLP_ARITHMETIC / HJBX_OPT_TRAIN_KERNEL: ask again after changing them), 256-byte aligned, need not be initialised.
 * User-defined systems (hjbx_system_create_from_source) after hjbx_system_enable_matrix_cores: the same arguments, workspace and results.
 * All argument checks run first; then the first call for an activation compiles the cooperative kernel for the user's struct (hiprtc, seconds,
 * at most once per handle; csrc/hjbx_user_train_kernels.hpp: residual mode 0 / 1 x large batch / minibatch = four kernels, PD network only).
 * HJBX_EUNSUPPORTED -- nothing launched, the handle's streaming and rollout kernels keep working, the PyTorch autograd path remains -- when
 * the handle has not been enabled, n is odd, the network is sin and n > 4, HJBX_OPT_MLP_ARITHMETIC != 0 or HJBX_OPT_TRAIN_KERNEL != 0 (float32
 * MFMA arithmetic, cooperative kernel only; the message names the option), or when ANY of the four kernels needs scratch: the whole unit is
 * refused, the message names the kernel and its bytes, and the refusal is remembered (a second call returns it at once).  HJBX_EINVAL +
 * hjbx_last_compile_log when the source does not compile there. */
size_t hjbx_value_loss_grad_workspace_bytes(int64_t B);
int hjbx_value_loss_grad_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int mode, const float* x,
                             const float* cost, const float* done, float* flat, void* workspace, int64_t B, void* stream);

/* The step between that buffer (after the all-reduce, if any) and Adam: mixed[k] = flat[k] / (#interior + eps) + reg * flat[P + k] / (#done + eps)
 * for the P = n_params parameter entries (vhjb.py:241, 253, 284) and losses[0..2] = {hjb + reg termination, hjb, termination} (vhjb.py:285-288;
 * losses may be NULL).  reg is read from reg_dev[0] when reg_dev is non-NULL (a device scalar survives hipGraph replay), else from `reg`.
 * loss_accum (3 floats, may be NULL): the three losses are ADDED to it -- `total_losses += ...` of train (vhjb.py:320-322) on the device;
 * step_counter (one int32, may be NULL): incremented by one -- `update_counter += 1` (vhjb.py:323). */
int hjbx_mix_gradients_f32(const float* flat, int64_t n_params, const float* reg_dev, double reg, double eps, float* mixed, float* losses,
                           float* loss_accum, int32_t* step_counter, void* stream);

/* The same step with optax.adam (vhjb.py:120, 262-263: b1, b2, eps as given, eps_root 0) applied in the same launch, the mixed gradient never
 * materialised:  g as above;  m <- m + (1 - b1)(g - m);  v <- b2 v + (1 - b2) g^2;  t <- t + 1;
 *                w <- w - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 * param / exp_avg / exp_avg_sq: the three weight matrices W1, W2, W3 (row-major, numel[i] entries, in the order of `flat`) and Adam's moments,
 * all updated in place; step[i]: device scalar holding t as float32, one per tensor (the layout torch.optim.Adam(fused / capturable) keeps, so
 * its state tensors can be handed over as they are; t is read from step[0], t + 1 written to all three, which may alias); ticket: one zero-initialised device word for the kernel's use, left zero. */
typedef struct hjbx_adam_state {
    float* param[3];
    float* exp_avg[3];
    float* exp_avg_sq[3];
    int64_t numel[3];
    float* step[3];
    unsigned int* ticket;
    double lr, beta1, beta2, eps;
} hjbx_adam_state;
int hjbx_mix_adam_f32(const float* flat, const float* reg_dev, double reg, double eps, const hjbx_adam_state* adam, float* losses, float* loss_accum,
                      int32_t* step_counter, void* stream);

/* params_update (vhjb.py:255-288) in ONE call for a single process: hjbx_value_loss_grad_f32 followed by hjbx_mix_adam_f32, with the flat
 * buffer never materialised on the default (cooperative) path -- the reduction of the per-workgroup partial sums, the division by the counts,
 * the mix, the losses and Adam's update run in one epilogue kernel, i.e. two launches per update.  Arguments as in those two entry points;
 * adam->param[] must be the network's W1, W2, W3.  workspace: hjbx_value_loss_adam_workspace_bytes(B) bytes, 256-byte aligned, need not be
 * initialised.  (A data-parallel step needs the flat buffer for its all-reduce: hjbx_value_loss_grad_f32, all-reduce, hjbx_mix_adam_f32.)
 * The Adam state's shapes are checked before anything is launched: an HJBX_EINVAL leaves no kernel behind.
 * User-defined systems after hjbx_system_enable_matrix_cores: as for hjbx_value_loss_grad_f32 -- the same run-time compiled unit, the same
 * refusals (not enabled, odd n, sin with n > 4, HJBX_OPT_MLP_ARITHMETIC != 0, HJBX_OPT_TRAIN_KERNEL != 0, a kernel that needs scratch), all of
 * them before the first launch -- followed by the library's own epilogue kernel. */
size_t hjbx_value_loss_adam_workspace_bytes(int64_t B);
/* optional last duty of that call: assemble the NEXT update's minibatch (what hjbx_replay_gather_f32 would do for index step_counter + 1, same
 * arguments and bounds behaviour) inside the epilogue kernel, so that a captured fit-phase update is two launches.  reg_out may be the buffer
 * reg_dev points to (it is written after every read of this update). */
typedef struct hjbx_next_minibatch {
    const float* buf_x; const float* buf_cost; const float* buf_done;
    int64_t capacity; int n;
    const int32_t* perm; int64_t perm_len;
    const float* reg_table; int64_t table_len;
    int64_t batch;
    float* xs; float* costs; float* dones; float* reg_out;
} hjbx_next_minibatch;
int hjbx_value_loss_adam_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int mode, const float* x, const float* cost,
                             const float* done, const float* reg_dev, double reg, double eps, const hjbx_adam_state* adam, float* losses,
                             float* loss_accum, int32_t* step_counter, const hjbx_next_minibatch* next, void* workspace, int64_t B, void* stream);

/* The minibatch of one update, assembled on the device: DataLoader(batch_size, shuffle=True, drop_last=True) + np_collate of the reference
 * (vhjb.py:151-154, 314; utils/utils.py:7-14) for a device-resident replay buffer (buf_x (capacity, n), buf_cost, buf_done (capacity,)):
 *   xs[s] = buf_x[perm[k * batch + s]] (likewise costs, dones), s = 0..batch-1, with k = step_dev[0] read ON THE DEVICE (NULL: k = 0), and
 *   reg_out[0] = reg_table[k] when reg_out is non-NULL (the regularisation weight of update k of the epoch, vhjb.py:323-324).
 * perm: perm_len int32 row indices < capacity (one random permutation of the buffer per epoch); reg_table: table_len floats.  A counter
 * beyond the permutation or the table, or an index outside the buffer, gathers nothing (no out-of-bounds access) and sets reg_out to NaN.
 * With step_dev = the counter hjbx_mix_gradients_f32 / hjbx_mix_adam_f32 increment, a captured hipGraph of gather ->
 * hjbx_value_loss_grad_f32 -> mix + Adam replays with no host-side work between two updates. */
int hjbx_replay_gather_f32(const float* buf_x, const float* buf_cost, const float* buf_done, int64_t capacity, int n, const int32_t* perm,
                           int64_t perm_len, const int32_t* step_dev, const float* reg_table, int64_t table_len, int64_t batch, float* xs,
                           float* costs, float* dones, float* reg_out, void* stream);

/* A rollout log appended to the device-resident replay ring, trajectory by trajectory: `trajectory = rollout_trajectory();
 * replay_buffer.xs.extend(trajectory)` of the reference (vhjb.py:304-308) on its deque(maxlen) (vhjb.py:62-73), for B closed loops at once and
 * without leaving the log's time-major layout.
 *   traj (T+1, B, n), cost (T+1, B): the log; done_step (B,) int32: index of each environment's terminal tuple;
 *   buf_x (capacity, n), buf_cost, buf_done (capacity,): the ring; head: its next write slot, in [0, capacity).
 * Environment b emits L_b = done_step[b] + 1 records (t = 0 .. done_step[b], in time order), environments in order of b.  With off_b the
 * exclusive prefix sum of L, K = sum L_b and drop = max(0, K - capacity), record (b, t) has the running index j = off_b + t; it is written
 * iff j >= drop, to slot (head + j - drop) mod capacity: x and cost copied bit for bit, done = 1 for t == done_step[b], else 0.  Nothing
 * beyond done_step[b] is read, no other slot is written, and the work is proportional to the min(K, capacity) records that land, not to
 * B (T+1).  The caller advances head by min(K, capacity) mod capacity.
 * A done_step entry outside [0, T] makes the call append NOTHING (no out-of-bounds access for any content of done_step).
 *   header: int64[4] in device memory = { K (over the valid entries), drop, number of out-of-range done_step entries, 0 }.
 *   workspace: hjbx_replay_append_workspace_bytes(B) bytes, 8-byte aligned, need not be initialised (slice sums and offsets of this call).
 * HJBX_EINVAL before any launch: a NULL or misaligned buffer, n outside [1, HJBX_MAX_N], B < 0, T < 0, capacity < 1, head outside
 * [0, capacity).  B == 0: HJBX_OK, nothing launched, the header zeroed. */
size_t hjbx_replay_append_workspace_bytes(int64_t B);
/* (vhjb.py:304-308 for float32 logs) */
int hjbx_replay_append_f32(const float* traj, const float* cost, const int32_t* done_step, int64_t T, int64_t B, int n, float* buf_x,
                           float* buf_cost, float* buf_done, int64_t capacity, int64_t head, int64_t* header, void* workspace, void* stream);
/* (vhjb.py:304-308 for float64 logs) */
int hjbx_replay_append_f64(const double* traj, const double* cost, const int32_t* done_step, int64_t T, int64_t B, int n, double* buf_x,
                           double* buf_cost, double* buf_done, int64_t capacity, int64_t head, int64_t* header, void* workspace, void* stream);

/* Dynamics.get_initial_state (dynamics_basic.py:28-29) with the uniforms drawn on the device: x0[i] = wrap(-x0_std + 2 x0_std u(i) + x0_mean),
 * the statement (and the code) of hjbx_initial_state_*, where the n uniforms of row r = first_row + i come from Philox4x32-10 (round
 * multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) under key (lo32(seed), hi32(seed)) at counter
 * (lo32(r), hi32(r), g, 0):
 *   float32: component k takes word k % 4 of group g = k / 4,                      u = float(w >> 8) 2^-24;
 *   float64: component k takes words a = 2 (k % 2), b = a + 1 of group g = k / 2,  u = ((w_a >> 5) 2^26 + (w_b >> 6)) 2^-53.
 * A row depends on (seed, r) only: batch size, grid, the split of a batch into calls, rank and call order have no effect, so disjoint row
 * ranges of one seed are disjoint parts of one stream.  No u01 buffer, no generator state in memory, no atomics.  Built-in systems run one
 * fused kernel; for a HJBX_SYS_USER handle the library writes the same uniforms into a (B, n) temporary of its own (stream-ordered) and
 * runs the handle's hjbx_initial_state_* kernel on it: the same bits.
 * HJBX_EINVAL before anything is enqueued: a NULL handle, x0_mean, x0_std or x0, a misaligned x0, B < 0.  B == 0: HJBX_OK, nothing launched. */
#define HJBX_HAS_DEVICE_COLLECTION 1 /* the four entry points below exist (an addition, nothing else changed) */
int hjbx_initial_state_philox_f32(const hjbx_system* sys, const double* x0_mean, const double* x0_std, uint64_t seed, uint64_t first_row,
                                  float* x0, int64_t B, void* stream);
int hjbx_initial_state_philox_f64(const hjbx_system* sys, const double* x0_mean, const double* x0_std, uint64_t seed, uint64_t first_row,
                                  double* x0, int64_t B, void* stream);

/* The statistics of an epoch's rollouts (vhjb.py:302-307: the trajectories; :326-329: mean and np.var(...)**0.5 of their costs, mean length)
 * from the contiguous time-major (S, B) cost log of hjbx_rollout_feedback_* / the fused rollouts.  Tuple t of environment b counts iff
 * t <= done_step[b]; entries past it are never read (a NaN there is not seen), and a done_step outside [0, S-1] is held to that range
 * (a negative one counts no tuple), so no content of done_step leads outside the log.
 *   traj_cost (B,) or NULL: the float64 sum of cost[0..done_step[b], b] in time order (one sequential chain per environment).
 *   stats[4] = { sum_b c_b, sum_b (c_b - mean)^2 with mean = stats[0] / B, sum_b (done_step[b] + 1), B }: summed over b in a fixed order
 *              without float atomics, bit-identical from call to call.  Mean, population standard deviation and mean length follow on the host.
 *   workspace: hjbx_reduce_workspace_bytes() bytes under that function's contract (zero-filled once, left zeroed, one stream at a time).
 * Two launches, no host synchronisation.  HJBX_EINVAL before anything is enqueued: NULL cost, done_step, stats or workspace, a misaligned
 * buffer, S < 1, B < 0.  B == 0: HJBX_OK, nothing launched, stats untouched. */
int hjbx_rollout_cost_stats_f32(const float* cost, const int32_t* done_step, int64_t S, int64_t B, double* traj_cost, double* stats,
                                void* workspace, void* stream);
int hjbx_rollout_cost_stats_f64(const double* cost, const int32_t* done_step, int64_t S, int64_t B, double* traj_cost, double* stats,
                                void* workspace, void* stream);

/* TEST INFRASTRUCTURE (like HJBX_OPT_ROLLOUT_EXTRA_WORKGROUPS): the element-wise activation functions that the matrix-core kernels inline,
 * evaluated over a plain device array by the same device code, so that a test can sweep the whole float32 range against a float64 reference:
 *   h[i] = act(a[i])                     (hjbx_activation: relu, tanh, sin)
 *   s[i] = the factor act'(a[i]) in the form the kernels use: [h > 0] (relu) and 1 - h^2 (tanh), both taken from h; cos(a[i]) for sin.
 * What the functions guarantee (asserted by tests/test_gpu_smooth_activations.py over every normal binade):
 *   relu: exact, -0 and negative inputs give +0, NaN passes through (s = 0 for it);
 *   tanh: relative error <= 6 x 2^-24 down to the smallest normal (<= 2 x 2^-24 for |a| < 0.625), odd bit for bit, +-1 exactly where the
 *         float32 rounding of tanh is +-1, NaN for NaN;
 *   sin / cos: absolute error <= 1e-7 for |a| <= 1e3 (sin relatively accurate as a -> 0); beyond that the accuracy decays (the argument
 *         reduction uses two float32 constants) and is gone by |a| ~ 1e6, but every finite input gives |h|, |s| <= 1; NaN for NaN and +-inf.
 * h or s may be NULL (not written).  One grid-stride launch on `stream`, no workspace.  HJBX_EINVAL before anything is enqueued: an unknown
 * activation, N < 0, NULL a, a misaligned buffer.  N == 0 or both outputs NULL: HJBX_OK, nothing launched. */
#define HJBX_HAS_ACTIVATION_PROBE 1 /* the entry point below exists (an addition, nothing else changed) */
int hjbx_activation_probe_f32(int activation, const float* a, float* h, float* s, int64_t N, void* stream);

/* The min-snap waypoint planner of Quadrotors2D on the device (quadrotors_model_based_controller.py:77-233).  The host solves the 7th-order
 * polynomials through the waypoints (solve_minimum_snap_coefficient, :99-159, float64); these entry points evaluate `update(t)` (:218-233):
 * the segment = the last i with t >= cumulated_t[i], the local time t - cumulated_t[i], derivatives 0..4 of both polynomials (:161-176) and the
 * differential flatness map to [x, y, theta, xd, yd, thetad] and the two rotor thrusts (:178-216), in the reference's formulas -- its theta_ddot
 * expression included, which is not the exact second derivative of theta (u_ref is not an exact feedforward).  Past the
 * last waypoint the reference is a hover at end_pt with local time 0 (:220-225).
 *   sys: a HJBX_SYS_QUAD2D handle (m, r, I, g, dt and the control limits are read from it).
 *   coeff (n_plans, 2, S, 8): ascending powers, the reference's layout (axis, segment, power); cum_t (n_plans, S + 1) = cumulated_t, ALWAYS
 *   double: segment and local time are found in float64 in both precisions, only the local time is rounded; end_pt (n_plans, 2) = points[-1].
 *   n_plans = 1: one plan shared by the B environments; n_plans = B: plan b belongs to environment b.
 *   t_k = t0 + k dt, formed in double for every k (never accumulated).
 * hjbx_minsnap_reference_*: x_ref (T_steps, B, 6), u_ref (T_steps, B, 2) = update(t_k) for k < T_steps, time-major; either may be NULL.
 * The segment index is held to [0, S] whatever cum_t contains: no plan leads a load outside coeff.
 * HJBX_EINVAL before any launch: a NULL handle or one that is not HJBX_SYS_QUAD2D, S < 1, t0 < 0 (or NaN), T_steps < 0, B < 0, n_plans other
 * than 1 or B, NULL or misaligned coeff (16 bytes), cum_t (8 bytes) or end_pt (its row), a misaligned output.  B == 0 or T_steps == 0:
 * HJBX_OK, nothing launched. */
#define HJBX_HAS_MINSNAP 1 /* the four entry points below exist (an addition, nothing else changed) */
/* (quadrotors_model_based_controller.py:218-233 and :178-216 in float32) */
int hjbx_minsnap_reference_f32(const hjbx_system* sys, const float* coeff, const double* cum_t, const float* end_pt, int S, int64_t n_plans,
                               double t0, int T_steps, float* x_ref, float* u_ref, int64_t B, void* stream);
/* (quadrotors_model_based_controller.py:218-233 and :178-216 in float64) */
int hjbx_minsnap_reference_f64(const hjbx_system* sys, const double* coeff, const double* cum_t, const double* end_pt, int S, int64_t n_plans,
                               double t0, int T_steps, double* x_ref, double* u_ref, int64_t B, void* stream);

/* The tracking closed loop on a plan, one kernel launch: for k < T_steps
 *   (x_ref, u_ref) = update(t_k);  e = states_wrap(x_k - x_ref);  u_k = clip(u_ref - K e, umin, umax)      (the law of :36-38 about a moving reference)
 *   cost_k = (e'Qe + (u_k - u_ref)'R(u_k - u_ref)) dt;  x_{k+1} = Dynamics.simulate(x_k, u_k)              (dynamics_basic.py:107-122; HJBX_RK4: u held)
 *   ctrl: HJBX_CTRL_LINEAR_FEEDBACK, only K (2, 6) is read; task: Q and R of the step cost, NULL when neither cost output is asked for.
 *   x0 (B, 6).  Outputs, time-major, each may be NULL: traj (T_steps + 1, B, 6), u_log (T_steps, B, 2), cost (T_steps, B),
 *   total_cost (B,) = the sum of cost_k in time order, x_final (B, 6), x_ref_log (T_steps, B, 6), u_ref_log (T_steps, B, 2): the two
 *   reference logs are bit-equal to hjbx_minsnap_reference_* on the same plan (one device function).
 * HJBX_EINVAL before any launch: everything hjbx_minsnap_reference_* refuses, a NULL controller or one of another kind, an integrator other
 * than HJBX_EULER / HJBX_RK4, a cost output without a task, NULL or misaligned x0, a misaligned output.  B == 0: HJBX_OK, nothing launched. */
/* (quadrotors_model_based_controller.py:36-38 about update(t) of :218-233, float32) */
int hjbx_rollout_minsnap_tracking_f32(const hjbx_system* sys, const hjbx_task* task, const hjbx_controller* ctrl, int integrator,
                                      const float* coeff, const double* cum_t, const float* end_pt, int S, int64_t n_plans, double t0, int T_steps,
                                      const float* x0, float* traj, float* u_log, float* cost, float* total_cost, float* x_final,
                                      float* x_ref_log, float* u_ref_log, int64_t B, void* stream);
/* (quadrotors_model_based_controller.py:36-38 about update(t) of :218-233, float64) */
int hjbx_rollout_minsnap_tracking_f64(const hjbx_system* sys, const hjbx_task* task, const hjbx_controller* ctrl, int integrator,
                                      const double* coeff, const double* cum_t, const double* end_pt, int S, int64_t n_plans, double t0,
                                      int T_steps, const double* x0, double* traj, double* u_log, double* cost, double* total_cost,
                                      double* x_final, double* x_ref_log, double* u_ref_log, int64_t B, void* stream);

/* User-defined control laws: the OPEN half of the reference's second plugin surface, "anything with get_control_efforts(x)"
 * (controller/controller_basic.py:1-5), compiled into the closed-loop rollout kernel (controller/vhjb.py:171-193; the four fixed kinds of
 * hjbx_controller stay what they are).  `law_source` is the text of the law as device code: member functions of
 *   template <typename T, typename S> struct UserLaw { T q[n_q]; ... };
 * `control` (required: the RAW control of one state, clipped to [umin, umax] by the library afterwards) and `reached` (optional, has_reached != 0:
 * the stop test of HJBX_ROLLOUT_STOP_AT_TARGET); the exact contract is at the top of csrc/hjbx_user_controller_kernels.hpp.  It is compiled
 * at run time (hiprtc, gfx950, the library's own build flags) for the system `sys` -- one of the five built-in systems or a user-defined one,
 * whose own source is compiled along -- into a code object of its own with six kernels: the law alone and the whole closed loop with
 * HJBX_EULER / HJBX_RK4, in float32 and float64.  The law reads n_q parameters q (<= HJBX_LAW_MAX_PARAMS, shared by all environments,
 * replaceable without a recompile), n_w values per environment (<= HJBX_LAW_MAX_ENV_PARAMS, a (B, n_w) buffer per call) and the time of the step.
 * The controller COPIES what it needs from `sys` (kind, dimensions, parameters, control limits, dt, a user-defined system's source): it holds
 * no reference to the handle, which may be destroyed first.  One controller may be used from several threads; its module is loaded per
 * device at the first launch.
 * hjbx_user_controller_create compiles eagerly and needs no GPU.  HJBX_EINVAL: NULL arguments, n_q or n_w out of range, a law that does
 * not compile (hjbx_last_compile_log returns the compiler's messages; after a successful create it lists the kernels that need scratch
 * memory, which are slow, not wrong: scratch is reported, not refused).  HJBX_EUNSUPPORTED: libhiprtc.so is not available, or a
 * HJBX_SYS_LINEAR handle whose (n, m) has no kernels.
 * hjbx_user_controller_set_params replaces q (n_q must be the value given at creation).  hjbx_user_controller_code_object copies up to `len`
 * bytes of the gfx950 ELF into buf (may be NULL) and returns its size.
 * hjbx_user_controller_eval_*: u (B, m) = clip(control(x, w, t)) for x (B, n); w (B, n_w), NULL if and only if n_w == 0.
 * hjbx_user_controller_rollout_*: hjbx_rollout_feedback_* with the law in place of the descriptor, the same outputs (any may be NULL), flags,
 * task and termination rules; the law and `reached` see t_k = t0 + k dt at step k.  Refused with HJBX_EINVAL before any launch: a NULL
 * controller, B < 0, T_steps < 0, an unknown integrator or flag, NULL or misaligned x0, w NULL with n_w > 0 or misaligned, a misaligned output,
 * HJBX_ROLLOUT_STOP_AT_TARGET for a law without `reached`, HJBX_ROLLOUT_TERMINATE or a cost output without a task; HJBX_ZOH:
 * HJBX_EUNSUPPORTED (not built).  B == 0: HJBX_OK, nothing launched. */
#define HJBX_HAS_USER_CONTROLLER 1 /* the entry points below exist (an addition, nothing else changed) */
#define HJBX_LAW_MAX_PARAMS 128
#define HJBX_LAW_MAX_ENV_PARAMS 32
typedef struct hjbx_user_controller hjbx_user_controller; /* opaque */
/* (controller/controller_basic.py:1-5: a Controller subclass's __init__, compiled) */
int hjbx_user_controller_create(const hjbx_system* sys, const char* law_source, const double* q, int n_q, int n_w, int has_reached,
                                hjbx_user_controller** out);
/* (controller/controller_basic.py:1-5: the end of the controller object) */
void hjbx_user_controller_destroy(hjbx_user_controller* ctl);
/* (controller/controller_basic.py:1-5: assigning the subclass's gains; no recompile) */
int hjbx_user_controller_set_params(hjbx_user_controller* ctl, const double* q, int n_q);
/* (controller/controller_basic.py:1-5 compiled; the closed loop controller/vhjb.py:171-193 around it) */
size_t hjbx_user_controller_code_object(const hjbx_user_controller* ctl, void* buf, size_t len);
/* (controller/controller_basic.py:1-5: get_control_efforts, float32) */
int hjbx_user_controller_eval_f32(hjbx_user_controller* ctl, const float* x, const float* w, double t, float* u, int64_t B, void* stream);
/* (controller/controller_basic.py:1-5: get_control_efforts, float64) */
int hjbx_user_controller_eval_f64(hjbx_user_controller* ctl, const double* x, const double* w, double t, double* u, int64_t B, void* stream);
/* (controller/controller_basic.py:1-5 inside the closed loop controller/vhjb.py:171-193, float32) */
int hjbx_user_controller_rollout_f32(hjbx_user_controller* ctl, const hjbx_task* task, int integrator, uint32_t flags, double t0, int T_steps,
                                     const float* x0, const float* w, float* traj, float* u_log, float* cost, int32_t* done_step,
                                     float* total_cost, float* x_final, int64_t B, void* stream);
/* (controller/controller_basic.py:1-5 inside the closed loop controller/vhjb.py:171-193, float64) */
int hjbx_user_controller_rollout_f64(hjbx_user_controller* ctl, const hjbx_task* task, int integrator, uint32_t flags, double t0, int T_steps,
                                     const double* x0, const double* w, double* traj, double* u_log, double* cost, int32_t* done_step,
                                     double* total_cost, double* x_final, int64_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HJBX_H */
