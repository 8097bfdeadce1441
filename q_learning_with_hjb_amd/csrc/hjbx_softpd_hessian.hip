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
// (sample, direction) pair, C = 32 / n samples per tile, mlp_value_hessian of hjbx_hessian_kernels.hpp with SOFT set): d3 and d3. take the
// places of 2y and 2y., the accumulators of a1, a2 and a3 start from the biases (MlpLdsSoft: the 385 floats of MlpBias next to the weight
// image), and a3 is a 32-register transient where the PD kernel holds y.  H is the only output.  Per sample: 8 n (128 n + 128*128 + 128*64) flop.
// ReLU has act'' = 0: a scalar piecewise-linear network has H = 0 wherever it is defined, so no ReLU kernel exists and the entry point fills H
// with zeros on the stream.  Compiled once per smooth activation (-DHJBX_SOFTPD_HESS_ACT=1 tanh + the C entry point, =2 sin).
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
static constexpr int kHessWaves = 4;   // one wave per SIMD: up to 512 registers each

// ---- the shipped (system, activation) pairs ------------------------------------------------------------------------------------------
// ONE table: the dispatcher below instantiates and launches exactly these, and tests/test_softpd_hessian_host.py reads the same lines to know
// how many kernels each unit must hold.  A pair is shipped only if its kernel needs no scratch and spills no VGPR; a pair taken out of the
// table is refused with HJBX_EUNSUPPORTED (the Python layer then takes the torch closed form) and listed in DESIGN.md 4.12.
//   X(system, activation)   system: one of the seven cases hjbx_softpd_value_grad_f32 dispatches; activation: 1 tanh, 2 sin
#define HJBX_SOFTPD_HESS_SHIPPED(X) \
    X(cartpole, 1) X(cartpole, 2)   \
    X(quad2d, 1) X(quad2d, 2)       \
    X(linear2, 1) X(linear2, 2)     \
    X(linear4, 1) X(linear4, 2)     \
    X(linear6, 1) X(linear6, 2)     \
    X(acrobot, 1) X(acrobot, 2)     \
    X(nearhover, 1) X(nearhover, 2)

enum SoftHessSys { cartpole, quad2d, linear2, linear4, linear6, acrobot, nearhover };
static constexpr const char* kSoftHessSysName[] = {"cartpole", "quad2d", "linear (n=2)", "linear (n=4)", "linear (n=6)", "acrobot", "nearhover"};
constexpr bool softpd_hessian_shipped(int system, int act) {
    bool yes = false;
#define HJBX_SOFTPD_HESS_ROW(s, a) yes = yes || (system == s && act == a);
    HJBX_SOFTPD_HESS_SHIPPED(HJBX_SOFTPD_HESS_ROW)
#undef HJBX_SOFTPD_HESS_ROW
    return yes;
}

// H (B,n,n) for a batch of states.  Tile group g = the samples g C .. g C + C - 1; work distribution and LDS staging exactly as in
// k_value_hessian (a contiguous range of groups per workgroup, pulled by its waves from an LDS counter; idle columns compute on the target
// state and store nothing).
template <typename S, int WAVES, int ACT>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void k_softpd_value_hessian(S sys, MlpP<S::N> p, const float* __restrict__ W1g,
                                                                              const float* __restrict__ W2g, const float* __restrict__ W3g,
                                                                              MlpHeadSoft head, const float* __restrict__ x,
                                                                              float* __restrict__ Hout, int64_t B, int64_t ngroups) {
    constexpr int N = S::N;
    constexpr int C = 32 / N;   // samples per tile
    static_assert(N % 2 == 0 && C >= 1, "state dimension must be even (k-steps of 2) and at most 32");
    __shared__ __attribute__((aligned(256))) MlpLdsSoft<N> L;
    const int tid = threadIdx.x;
    if (tid == 0) L.next = WAVES;  // groups 0..WAVES-1 of the range are taken statically
    mlp_fill_lds<N, WAVES * 64>(L, W1g, W2g, W3g, tid);
    mlp_fill_bias<WAVES * 64>(L.bias, head.b1, head.b2, head.b3, head.w4, head.b4, tid);
    __syncthreads();
    // (the wave index through readfirstlane: the tile group then lives in SGPRs, see k_vhjb_rollout_mfma)
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const auto c = [&] { return mlp_ctx<N>(L, lane); }();
    const int i = c.i, h = c.h;
    const bool busy = i < C * N;             // an idle column computes on the target state and stores nothing
    const int cs = busy ? i / N : 0;         // sample of the tile
    const int j = busy ? i - cs * N : 0;     // direction
    float sj = p.istd[0];
#pragma unroll
    for (int k = 1; k < N; ++k) sj = (j == k) ? p.istd[k] : sj;

    const int64_t groups_per_wg = (ngroups + gridDim.x - 1) / gridDim.x;
    const int64_t g_begin = (int64_t)blockIdx.x * groups_per_wg;
    const int64_t g_end = (g_begin + groups_per_wg < ngroups) ? g_begin + groups_per_wg : ngroups;

    // (no prefetch of the next tile's rows: see k_value_hessian)
    for (int64_t grp = g_begin + wave; grp < g_end;) {
        // the weights are loop invariant: without this barrier LICM hoists LDS reads out of the tile loop
        asm volatile("" ::: "memory");
        const int64_t env = grp * C + cs;
        const bool live = busy && env < B;
        float xs[N], Hcol[N];
        load_sample<N>(x, p, env, live, xs);
        mlp_value_hessian<S, ACT, true>(sys, p, c, xs, j, sj, true, nullptr, Hcol, &L.bias);
        if (live && h == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k) Hout[(env * N + k) * N + j] = Hcol[k];
        }
        int nxt = 0;
        if (lane == 0) nxt = atomicAdd(&L.next, 1);
        grp = g_begin + __builtin_amdgcn_readfirstlane(nxt);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
template <typename S, int ACT>
static int launch_softpd_value_hessian(S sys, const hjbx_net& net, const float* x, float* H, int64_t B, void* st, const char* who) {
    constexpr int C = 32 / S::N;
    const MlpP<S::N> p = make_mlp_params<S::N>(net);
    const int64_t ngroups = (B + C - 1) / C;
    const int n_cu = hjbx_device_cus();
    if (n_cu <= 0) return hjbx_set_error(HJBX_ENODEVICE, "%s: no HIP device", who);
    const int64_t grid = ngroups < n_cu ? ngroups : n_cu;
    hipLaunchKernelGGL((k_softpd_value_hessian<S, kHessWaves, ACT>), dim3((unsigned)grid), dim3(kHessWaves * 64), 0, (hipStream_t)st, sys, p, net.W1,
                       net.W2, net.W3, make_head<MlpHeadSoft>(net), x, H, B, ngroups);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

// the systems hjbx_softpd_value_grad_f32 dispatches, each if the table ships it for this unit's activation (wrap is all the kernel takes from
// the system, so its parameters stay unset)
template <int ACT>
static int dispatch_softpd_value_hessian(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, int64_t B, void* st, const char* who) {
    auto go = [&](auto tag, auto s) {
        constexpr int kSys = decltype(tag)::value;
        if constexpr (softpd_hessian_shipped(kSys, ACT)) return launch_softpd_value_hessian<decltype(s), ACT>(s, net, x, H, B, st, who);
        else
            return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no kernel for the pair (%s, %s): it does not fit the register file without scratch", who,
                                  kSoftHessSysName[kSys], ACT == HJBX_ACT_TANH ? "tanh" : "sin");
    };
    switch (sys->kind) {
    case HJBX_SYS_CARTPOLE: return go(std::integral_constant<int, cartpole>{}, Cartpole<float>{});
    case HJBX_SYS_QUAD2D: return go(std::integral_constant<int, quad2d>{}, Quad2D<float>{});
    case HJBX_SYS_LINEAR:
        if (sys->n == 2) return go(std::integral_constant<int, linear2>{}, Linear<float, 2, 1>{});
        if (sys->n == 4) return go(std::integral_constant<int, linear4>{}, Linear<float, 4, 1>{});
        if (sys->n == 6) return go(std::integral_constant<int, linear6>{}, Linear<float, 6, 2>{});
        break;
    case HJBX_SYS_ACROBOT: return go(std::integral_constant<int, acrobot>{}, Acrobot<float>{});
    case HJBX_SYS_NEARHOVER: return go(std::integral_constant<int, nearhover>{}, NearHover<float>{});
    }
    return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no kernel for system kind %d with n=%d", who, sys->kind, sys->n);
}

using softpd_value_hessian_fn = int(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, int64_t B, void* stream, const char* who);
#define HJBX_SOFTPD_HESS_VARIANTS(X) X(1) X(2)
#define HJBX_SOFTPD_HESS_DECLARE(v) __attribute__((visibility("hidden"))) softpd_value_hessian_fn HJBX_MLP_SYM(hjbx_softpd_value_hessian, _act, v);
HJBX_SOFTPD_HESS_VARIANTS(HJBX_SOFTPD_HESS_DECLARE)
int HJBX_MLP_SYM(hjbx_softpd_value_hessian, _act, HJBX_SOFTPD_HESS_ACT)(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, int64_t B,
                                                                        void* stream, const char* who) {
    return dispatch_softpd_value_hessian<kAct>(sys, net, x, H, B, stream, who);
}

#if HJBX_SOFTPD_HESS_ACT == 1
// the checks of hjbx_value_hessian_f32 (check_value_hessian), in its order, for this head's pointers and its one output
static int check_softpd_value_hessian(const char* who, const hjbx_system* sys, const hjbx_net& net, const float* x, const float* H, int64_t B) {
    if (B < 0) return hjbx_set_error(HJBX_EINVAL, "%s: negative batch size", who);
    if (B == 0 || !H) return kEmptyCall;
    if (!x || !net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3 || !net.w4 || !net.b4)
        return hjbx_set_error(HJBX_EINVAL, "%s: NULL x, weight or bias pointer", who);
    if (sys->kind == HJBX_SYS_USER)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: user-defined systems are not supported, the kernel exists for the built-in systems only", who);
    if (int rc = check_features(who, net)) return rc;
    if (!state_rows_aligned(x, sys) || (reinterpret_cast<uintptr_t>(H) & 15u))
        return hjbx_set_error(HJBX_EINVAL, "%s: x must be aligned to its row vector width, H to 16 bytes", who);
    return check_std(who, net, sys->n);
}

extern "C" int hjbx_softpd_value_hessian_f32(const hjbx_system* sys, const hjbx_softpd_mlp* mlp, const float* x, float* H, int64_t B, void* stream) {
    const char* who = "hjbx_softpd_value_hessian_f32";
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    if (const int rc = check_softpd_value_hessian(who, sys, net, x, H, B)) return rc == kEmptyCall ? HJBX_OK : rc;
    if (net.activation == HJBX_ACT_RELU) {   // act'' = 0: H = 0 wherever it is defined (see the top of this file)
        const hipError_t e = hipMemsetAsync(H, 0, sizeof(float) * (size_t)B * (size_t)sys->n * (size_t)sys->n, (hipStream_t)stream);
        if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
        return HJBX_OK;
    }
#define HJBX_SOFTPD_HESS_ENTRY(v) hjbx_softpd_value_hessian_act##v,
    static softpd_value_hessian_fn* const variants[] = {nullptr, HJBX_SOFTPD_HESS_VARIANTS(HJBX_SOFTPD_HESS_ENTRY)};
#undef HJBX_SOFTPD_HESS_ENTRY
    return variants[net.activation](sys, net, x, H, B, stream, who);
}
#endif
