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
#include "hjbx_hessian_kernels.hpp"   // mlp_value_hessian: one column of a tile (shared with hjbx_softpd_hessian.hip)
#include "hjbx_mlp_host.hpp"

using namespace hjbx;

// Compiled once per activation (-DHJBX_HESS_ACT=0 relu + the C entry point, =1 tanh, =2 sin): seven instantiations each, side by side.
#ifndef HJBX_HESS_ACT
#error "compile hjbx_hessian.hip with -DHJBX_HESS_ACT=0 (relu + the C entry point), =1 (tanh) and =2 (sin)"
#endif
static constexpr int kAct = HJBX_HESS_ACT;
static_assert(kAct == HJBX_ACT_RELU || kAct == HJBX_ACT_TANH || kAct == HJBX_ACT_SIN, "the Hessian kernel exists for relu, tanh and sin");
static constexpr int kHessWaves = 4;   // one wave per SIMD: up to 512 registers each

// H (B,n,n) and dy_dx (B,n,64) for a batch of states.  Tile group g = the samples g C .. g C + C - 1; work distribution and LDS staging as in
// k_value_grad_mfma (a contiguous range of groups per workgroup, pulled by its waves from an LDS counter).
template <typename S, int WAVES, int ACT>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void k_value_hessian(S sys, MlpP<S::N> p, const float* __restrict__ W1g,
                                                                       const float* __restrict__ W2g, const float* __restrict__ W3g,
                                                                       const float* __restrict__ x, float* __restrict__ Hout,
                                                                       float* __restrict__ dyout, int64_t B, int64_t ngroups) {
    constexpr int N = S::N;
    constexpr int C = 32 / N;   // samples per tile
    static_assert(N % 2 == 0 && C >= 1, "state dimension must be even (k-steps of 2) and at most 32");
    __shared__ __attribute__((aligned(256))) MlpLds<N> L;
    const int tid = threadIdx.x;
    if (tid == 0) L.next = WAVES;  // groups 0..WAVES-1 of the range are taken statically
    mlp_fill_lds<N, WAVES * 64>(L, W1g, W2g, W3g, tid);
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

    // No prefetch of the next tile's rows, unlike k_value_grad_mfma: a tile is ~1600 MFMAs (40 us), the exposed load a few per cent of it,
    // and n more registers held through every chain are what the sin instantiation for n = 10 has not got.
    for (int64_t grp = g_begin + wave; grp < g_end;) {
        // the weights are loop invariant: without this barrier LICM hoists LDS reads out of the tile loop
        asm volatile("" ::: "memory");
        const int64_t env = grp * C + cs;
        const bool live = busy && env < B;
        float xs[N], Hcol[N];
        load_sample<N>(x, p, env, live, xs);
        float* dyp = (dyout && live) ? dyout + (env * N + j) * kH3 + 4 * h : nullptr;
        mlp_value_hessian<S, ACT>(sys, p, c, xs, j, sj, Hout != nullptr, dyp, Hcol);
        if (Hout && live && h == 0) {
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
static int launch_value_hessian(S sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* st, const char* who) {
    constexpr int C = 32 / S::N;
    const MlpP<S::N> p = make_mlp_params<S::N>(net);
    const int64_t ngroups = (B + C - 1) / C;
    const int n_cu = hjbx_device_cus();
    if (n_cu <= 0) return hjbx_set_error(HJBX_ENODEVICE, "%s: no HIP device", who);
    const int64_t grid = ngroups < n_cu ? ngroups : n_cu;
    hipLaunchKernelGGL((k_value_hessian<S, kHessWaves, ACT>), dim3((unsigned)grid), dim3(kHessWaves * 64), 0, (hipStream_t)st, sys, p, net.W1, net.W2,
                       net.W3, x, H, dy, B, ngroups);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

// the systems hjbx_value_grad_f32 dispatches (wrap is all the kernel takes from the system, so its parameters stay unset)
template <int ACT>
static int dispatch_value_hessian(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* st, const char* who) {
    auto go = [&](auto s) { return launch_value_hessian<decltype(s), ACT>(s, net, x, H, dy, B, st, who); };
    switch (sys->kind) {
    case HJBX_SYS_CARTPOLE: return go(Cartpole<float>{});
    case HJBX_SYS_QUAD2D: return go(Quad2D<float>{});
    case HJBX_SYS_LINEAR:
        if (sys->n == 2) return go(Linear<float, 2, 1>{});
        if (sys->n == 4) return go(Linear<float, 4, 1>{});
        if (sys->n == 6) return go(Linear<float, 6, 2>{});
        break;
    case HJBX_SYS_ACROBOT: return go(Acrobot<float>{});
    case HJBX_SYS_NEARHOVER: return go(NearHover<float>{});
    }
    return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no kernel for system kind %d with n=%d", who, sys->kind, sys->n);
}

using value_hessian_fn = int(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B, void* stream, const char* who);
#define HJBX_HESS_VARIANTS(X) X(0) X(1) X(2)
#define HJBX_HESS_DECLARE(v) __attribute__((visibility("hidden"))) value_hessian_fn HJBX_MLP_SYM(hjbx_value_hessian, _act, v);
HJBX_HESS_VARIANTS(HJBX_HESS_DECLARE)
int HJBX_MLP_SYM(hjbx_value_hessian, _act, HJBX_HESS_ACT)(const hjbx_system* sys, const hjbx_net& net, const float* x, float* H, float* dy, int64_t B,
                                                          void* stream, const char* who) {
    return dispatch_value_hessian<kAct>(sys, net, x, H, dy, B, stream, who);
}

#if HJBX_HESS_ACT == 0
// the checks of hjbx_value_grad_f32 (check_value_grad), in its order, for this entry point's outputs
static int check_value_hessian(const char* who, const hjbx_system* sys, const hjbx_net& net, const float* x, const float* H, const float* dy, int64_t B) {
    if (B < 0) return hjbx_set_error(HJBX_EINVAL, "%s: negative batch size", who);
    if (B == 0 || (!H && !dy)) return kEmptyCall;
    if (!x || !net.W1 || !net.W2 || !net.W3) return hjbx_set_error(HJBX_EINVAL, "%s: NULL x or weight pointer", who);
    if (sys->kind == HJBX_SYS_USER)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: user-defined systems are not supported, the kernel exists for the built-in systems only", who);
    if (int rc = check_features(who, net)) return rc;
    if (!state_rows_aligned(x, sys) || (reinterpret_cast<uintptr_t>(H) & 15u) || (reinterpret_cast<uintptr_t>(dy) & 15u))
        return hjbx_set_error(HJBX_EINVAL, "%s: x must be aligned to its row vector width, H and dy_dx to 16 bytes", who);
    return check_std(who, net, sys->n);
}

extern "C" int hjbx_value_hessian_f32(const hjbx_system* sys, const hjbx_mlp* mlp, const float* x, float* H, float* dy_dx, int64_t B, void* stream) {
    const char* who = "hjbx_value_hessian_f32";
    if (!sys || !mlp) return hjbx_set_error(HJBX_EINVAL, "%s: NULL system or mlp descriptor", who);
    const hjbx_net net = make_net(mlp);
    if (const int rc = check_value_hessian(who, sys, net, x, H, dy_dx, B)) return rc == kEmptyCall ? HJBX_OK : rc;
#define HJBX_HESS_ENTRY(v) hjbx_value_hessian_act##v,
    static value_hessian_fn* const variants[] = {HJBX_HESS_VARIANTS(HJBX_HESS_ENTRY)};
#undef HJBX_HESS_ENTRY
    return variants[net.activation](sys, net, x, H, dy_dx, B, stream, who);
}
#endif
