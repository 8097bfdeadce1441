// hjbx_mlp_kernels.hpp -- the two persistent matrix-core kernels of the value network (design: top of hjbx_mlp.hip), templated on the
// network's head so that hjbx_mlp.hip (PD network, controller/vhjb.py) and hjbx_softpd.hip (soft-PD network of the notebooks) instantiate
// the same work distribution, LDS staging and per-step code.  Each translation unit instantiates only its own head.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstddef>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"
#include "hjbx_mlp_core.hpp"
#include "hjbx_mlp_x3.hpp"
#include "hjbx_mlp_h2.hpp"

using namespace hjbx;

// The head of the network (mlp_value_grad's SOFT) and what it adds to the kernels' arguments and LDS image.
struct MlpHeadPd {   // V = |y|^2 + eps_s |e|^2 (controller/vhjb.py:17-60): nothing beyond the three weight matrices
    static constexpr bool kSoft = false;
    template <int N, int AR> using Lds = typename MlpArith<AR>::template Lds<N>;
};
struct MlpHeadSoft {  // V = act(a3) . w4 + b4 with biases on every layer (SoftPDValueApproximator of the notebooks); f32 MFMA only
    static constexpr bool kSoft = true;
    template <int N, int AR> using Lds = MlpLdsSoft<N>;
    const float *b1, *b2, *b3, *w4, *b4;   // device pointers: (h1), (h2), (h3), (h3), (1)
};

// ---- kernel 1: V and dV/dx for a batch of states (hjbx_value_grad_f32) ---------------------------------------
template <typename S, int TL, int WAVES, int ACT, int AR, typename HEAD = MlpHeadPd>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void k_value_grad_mfma(S sys, MlpP<S::N> p, const float* __restrict__ W1g,
                                                                         const float* __restrict__ W2g, const float* __restrict__ W3g,
                                                                         const float* __restrict__ x, float* __restrict__ Vout,
                                                                         float* __restrict__ gout, int64_t B, int64_t ngroups, HEAD head) {
    constexpr int N = S::N;
    static_assert(N % 2 == 0, "state dimension must be even (k-steps of 2)");
    static_assert(AR == 0 || TL == 1, "the split-operand chains hold one tile per wave");
    __shared__ __attribute__((aligned(256))) typename HEAD::template Lds<N, AR> L;
    const int tid = threadIdx.x;
    if (tid == 0) L.next = WAVES;  // groups 0..WAVES-1 of the range are taken statically
#ifdef HJBX_DIAG_CLOCK
    const unsigned long long tentry = __builtin_amdgcn_s_memrealtime();
#endif
    MlpArith<AR>::template fill<N, WAVES * 64>(L, W1g, W2g, W3g, tid);
    if constexpr (HEAD::kSoft) mlp_fill_bias<WAVES * 64>(L.bias, head.b1, head.b2, head.b3, head.w4, head.b4, tid);
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    // (the context is made inside a lambda, here and in the other kernels: called directly, hipcc forms the lane bases of the swizzled images
    //  with other instructions than it has so far)
    const auto c = [&] { return MlpArith<AR>::template ctx<N>(L, lane); }();
    const int i = c.i, h = c.h;

    // Work distribution: the workgroup owns a contiguous range of tile groups and its waves pull the next one
    // from an LDS counter.  (With a static stride the older wave of each SIMD pair wins the matrix-pipe
    // arbitration, finishes its share ~25 % early and leaves its partner running alone.)
    const int64_t groups_per_wg = (ngroups + gridDim.x - 1) / gridDim.x;
    const int64_t g_begin = (int64_t)blockIdx.x * groups_per_wg;
    const int64_t g_end = (g_begin + groups_per_wg < ngroups) ? g_begin + groups_per_wg : ngroups;

    // one row of x per lane and tile; both lane halves read the same row (the second read hits the same lines)
    auto load_rows = [&](int64_t grp, float (&dst)[TL][N]) {
#pragma unroll
        for (int t = 0; t < TL; ++t) {
            const int64_t en = (grp * TL + t) * 32 + i;
            load_sample<N>(x, p, en, grp < g_end && en < B, dst[t]);
        }
    };

    int64_t grp = g_begin + wave;
#ifdef HJBX_DIAG_CLOCK
    // DIAGNOSTIC BUILD ONLY (tools/diag_clock.py): shader-clock and 100 MHz wall stamps around the tile loop
    const unsigned long long t0c = __builtin_amdgcn_s_memtime(), t0r = __builtin_amdgcn_s_memrealtime();
#endif
    float xs[TL][N], xn[TL][N];
    load_rows(grp, xs);
    for (; grp < g_end;) {
        // the weights are loop invariant: without this barrier LICM hoists LDS reads out of the tile loop
        asm volatile("" ::: "memory");
        // claim the next group now and fetch its rows: the HBM latency hides behind this group's MFMAs
        int nxt = 0;
        if (lane == 0) nxt = atomicAdd(&L.next, 1);
        const int64_t grp_next = g_begin + __builtin_amdgcn_readfirstlane(nxt);
        load_rows(grp_next, xn);

        float V[TL], g[TL][N];
        if constexpr (HEAD::kSoft) mlp_value_grad<S, TL, ACT, true>(sys, p, c, xs, gout != nullptr, V, g, &L.bias);
        else MlpArith<AR>::template value_grad<S, TL, ACT>(sys, p, c, xs, gout != nullptr, V, g);
#pragma unroll
        for (int t = 0; t < TL; ++t) {
            const int64_t env = (grp * TL + t) * 32 + i;
            if (env < B && h == 0) {
#ifndef HJBX_DIAG_CLOCK
                if (Vout) Vout[env] = V[t];
#endif
                if (gout) store_row<N>(gout, env, g[t]);
            }
#pragma unroll
            for (int k = 0; k < N; ++k) xs[t][k] = xn[t][k];
        }
        grp = grp_next;
    }
#ifdef HJBX_DIAG_CLOCK
    {
        const unsigned long long t1c = __builtin_amdgcn_s_memtime(), t1r = __builtin_amdgcn_s_memrealtime();
        // the caller of the diagnostic build passes a scratch "V" buffer of >= 4*gridDim.x*WAVES floats and gradV != NULL
        if (Vout && gout && lane == 0) {
            float* d = Vout + 4 * ((int64_t)blockIdx.x * WAVES + wave);
            d[0] = (float)(t1c - t0c); d[1] = (float)(t1r - t0r);
            d[2] = (float)(t0r - tentry); d[3] = (float)(tentry & 0xFFFFFFull);
        }
    }
#endif
}

// ---- kernel 2: the whole VHJB closed loop for n_steps steps in one launch (hjbx_vhjb_rollout_f32) ----------------
// Per environment tile: state in registers; per step: value gradient on the matrix cores (above), then exactly the
// per-environment code of hjbx_vhjb_step (vhjb_step_env: bounds / termination, control from gradV, cost, HJB
// residual, Euler or RK4 step), then the time-major log slabs.  Tiles are independent, so a wave runs all steps of
// one tile group before pulling the next; the weights are staged into LDS once per launch instead of once per step.
template <int N, int M> struct RolloutOut {
    float* traj;   // (n_steps+1, B, N) or NULL: slab k = state at step t_first + k
    float* u_log;  // (n_steps, B, M) or NULL
    float* cost;   // (n_steps, B)
    float* done;   // (n_steps, B)
    float* resid;  // (n_steps, B) or NULL
    int32_t* done_step;  // (B) in/out
    float* x_out;  // (B, N) or NULL
};

// Work distribution of the persistent rollout kernel.  The caller's workspace (hjbx_rollout_workspace_bytes(), zero-filled once,
// left zeroed by every launch) holds, as 32-bit words:
static constexpr int kWsQueue = 0;                      // schedule 1: head of the device-wide tile queue
static constexpr int kWsStarted = 32;                   // workgroups that have started
static constexpr int kWsExited = 64;                    // workgroups whose waves have all finished (the last one zeroes the workspace)
static constexpr int kWsFlags = 96;                     // [kMaxGrid] 0 = not started, 1 = running its own range, 2 = range open to every wave
static constexpr int kMaxGrid = 1024;
static constexpr int kWsOpen = kWsFlags + kMaxGrid;     // [kMaxGrid] next unclaimed pick of an open range
static constexpr int kWsWords = kWsOpen + kMaxGrid;
#define HJBX_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

template <int INTEG, typename S, int WAVES, int ACT, int AR, typename HEAD = MlpHeadPd>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void k_vhjb_rollout_mfma(S sys_k, MlpP<S::N> p_k, TaskP<float, S::N, S::M> tk_k,
                                                                           Limits<float, S::M> lim_k, const float* __restrict__ W1g,
                                                                           const float* __restrict__ W2g, const float* __restrict__ W3g,
                                                                           int t_first, int n_steps, int T_max, const float* x /* may alias traj slab 0 */,
                                                                           const int32_t* __restrict__ order, RolloutOut<S::N, S::M> o, int64_t B,
                                                                           int64_t ngroups, unsigned* ws, int sched, HEAD head) {
    constexpr int N = S::N, M = S::M;
    static_assert(N % 2 == 0, "state dimension must be even (k-steps of 2)");
    __shared__ __attribute__((aligned(256))) typename HEAD::template Lds<N, AR> L;
    // System, task, limits and normalisation constants are staged in LDS: as kernel arguments they are ~100-250 wave-uniform
    // scalars that do not fit the SGPR file next to the address arithmetic, and hipcc spilled them to VGPR lanes
    // (hundreds of v_readlane / v_writelane per step, some inside the MFMA chains).  LDS broadcast reads cost no SGPRs.
    __shared__ __attribute__((aligned(16))) unsigned char sys_raw[sizeof(S)];  // S has default member initialisers: no __shared__ S
    S& sys_s = *reinterpret_cast<S*>(sys_raw);
    __shared__ MlpP<N> p_s;
    __shared__ TaskP<float, N, M> tk_s;
    __shared__ Limits<float, M> lim_s;
    const int tid = threadIdx.x;
    // One queue per SIMD (the waves w and w + 4 of a workgroup share SIMD w & 3): SIMD q works through the picks q, q + 4, q + 8, ...
    // of this workgroup.  A tile here is a whole n_steps-step rollout, so with a single queue per workgroup the four SIMDs of a
    // CU could end up with 9 / 7 tiles instead of 8 / 8 at B = 2^18 and the CU waited for the unlucky one (+-12 % from build to build).
    __shared__ int q_next[4];
    __shared__ int waves_done;
    __shared__ unsigned my_flag;
    if (tid < 4) q_next[tid] = WAVES / 4;
    if (tid == 0) {
        waves_done = 0;
        // announce this workgroup: 0 -> 1; a 2 coming back means the others have already opened (and taken) its range
        unsigned seen = 0u;
        __hip_atomic_compare_exchange_strong(ws + kWsFlags + blockIdx.x, &seen, 1u, __ATOMIC_RELAXED, HJBX_RLX_AGENT);
        my_flag = seen;
        __hip_atomic_fetch_add(ws + kWsStarted, 1u, HJBX_RLX_AGENT);
        sys_s = sys_k; p_s = p_k; tk_s = tk_k; lim_s = lim_k;
    }
    MlpArith<AR>::template fill<N, WAVES * 64>(L, W1g, W2g, W3g, tid);
    if constexpr (HEAD::kSoft) mlp_fill_bias<WAVES * 64>(L.bias, head.b1, head.b2, head.b3, head.w4, head.b4, tid);
    __syncthreads();
    const S& sys = sys_s;
    const MlpP<N>& p = p_s;
    const TaskP<float, N, M>& tk = tk_s;
    const Limits<float, M>& lim = lim_s;
    // wave index and this workgroup's flag are wave uniform IN FACT; through readfirstlane they are uniform TO THE COMPILER too, so the
    // tile group a wave works on (`grp`) lives in SGPRs and `if (grp < 0) grp = next_group()` is a scalar branch.  With `grp` in VGPRs
    // that branch was an EXEC-predicated region, and a register-allocator spill store placed inside it ran with EXEC = 0 for waves
    // that already had a group: the reload after the join returned garbage (round 2: n = 10 / m = 2 kernels with 14 spilled VGPRs
    // produced wrong trajectories).  A CPU test also keeps every instantiation at zero scratch.
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned my_flag_u = (unsigned)__builtin_amdgcn_readfirstlane((int)my_flag);
    const auto c = [&] { return MlpArith<AR>::template ctx<N>(L, lane); }();
    const int i = c.i, h = c.h;
    const int simd = wave & 3;
    const int G = (int)gridDim.x;
    // schedule 0 (default): every workgroup owns an equal range of tile groups -- contiguous in natural order (measured 12 % faster
    // at B = 2^18 than dealing single groups round-robin); with `order` the live environments come first, so the groups are dealt
    // round-robin (group = workgroup + pick * gridDim) to spread the live tiles over all CUs -- and its SIMDs work through it via the
    // LDS queues above.  A workgroup that finds no free CU when the launch starts (one workgroup fills a CU) would only run after
    // another one has finished, doubling the launch: so a wave that has finished its own share looks for workgroups that have NOT
    // STARTED, opens their ranges (flag 0 -> 2) and every finishing wave takes tiles from the open ranges, one returning atomic per
    // tile; the late workgroup then finds its range taken and only helps.  With every workgroup resident this costs one atomic load.
    // schedule 1: a device-wide queue, one returning atomic per tile (the first tile of every wave is static).
    const int64_t picks_per_wg = (ngroups + G - 1) / G;
    auto group_of = [&](int w, int64_t pick) -> int64_t {
        if (pick >= picks_per_wg) return -1;
        const int64_t g = order ? (int64_t)w + pick * G : (int64_t)w * picks_per_wg + pick;
        return g < ngroups ? g : -1;
    };
    int victim = -1;                                    // schedule 0: < 0 = own range, else the workgroup whose open range is being drained
    auto next_group = [&]() -> int64_t {
        if (sched == 1) {
            unsigned t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ws + kWsQueue, 1u, HJBX_RLX_AGENT);
            const int64_t g = (int64_t)G * WAVES + (unsigned)__builtin_amdgcn_readfirstlane((int)t);
            return g < ngroups ? g : -1;
        }
        if (victim < 0) {
            int nxt = 0;
            if (lane == 0) nxt = atomicAdd(&q_next[simd], 1);
            const int64_t g = my_flag_u == 0u ? group_of(blockIdx.x, simd + 4 * (int64_t)__builtin_amdgcn_readfirstlane(nxt)) : -1;
            if (g >= 0) return g;
            victim = 0;
            unsigned started = 0;
            if (lane == 0) started = __hip_atomic_load(ws + kWsStarted, HJBX_RLX_AGENT);
            if (__builtin_amdgcn_readfirstlane((int)started) >= G) victim = G;     // every workgroup is resident: nothing to take over
        }
        while (victim < G) {
            // flags of workgroups victim .. victim + 63; an unstarted one is opened here and now
            const int w = victim + lane;
            unsigned f = 1u;
            if (w < G) {
                f = __hip_atomic_load(ws + kWsFlags + w, HJBX_RLX_AGENT);
                if (f == 0u && __hip_atomic_compare_exchange_strong(ws + kWsFlags + w, &f, 2u, __ATOMIC_RELAXED, HJBX_RLX_AGENT)) f = 2u;
            }
            unsigned long long open = __builtin_amdgcn_ballot_w64(f == 2u);
            while (open) {
                const int b = __builtin_ctzll(open);
                unsigned t = 0;
                if (lane == 0) t = __hip_atomic_fetch_add(ws + kWsOpen + victim + b, 1u, HJBX_RLX_AGENT);
                const int64_t g = group_of(victim + b, (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)t));
                if (g >= 0) { victim += b; return g; }      // (the scan resumes at this workgroup next time)
                open &= open - 1;
            }
            victim = (victim + 64 < G) ? victim + 64 : G;
        }
        return -1;
    };
    int64_t grp;
    if (sched == 1) grp = (int64_t)blockIdx.x * WAVES + wave < ngroups ? (int64_t)blockIdx.x * WAVES + wave : -1;
    else grp = my_flag_u == 0u ? group_of(blockIdx.x, wave) : -1;   // wave = simd + 4 * (wave >> 2): the first WAVES / 4 picks of each SIMD are static
    if (grp < 0) grp = next_group();
    while (grp >= 0) {
        const int64_t slot = grp * 32 + i;
        const bool valid = slot < B;
        int64_t env = valid ? (order ? (int64_t)order[slot] : slot) : 0;
        env = env < 0 ? 0 : (env >= B ? B - 1 : env);  // a corrupt `order` entry must not become an out-of-bounds access
        const bool writer = valid && h == 0;  // both lane halves carry the same environment; half 0 stores
        float xs[1][N];
        int32_t ds = 0;                        // padding lanes are "done": they hold xf and emit nothing
        if (valid) {
            load_row<N>(x, env, xs[0]);
            ds = o.done_step[env];
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) xs[0][k] = p.xf[k];
        }
        if (o.traj && writer) store_row<N>(o.traj, env, xs[0]);
        for (int k = 0; k < n_steps; ++k) {
            asm volatile("" ::: "memory");
            float xo[N], u[M], cst, dn, res;
            if (__builtin_amdgcn_ballot_w64(ds < 0) == 0) {
                // every environment of this tile has finished: vhjb_step_env would emit zeros and hold the state whatever the
                // value gradient is, so the network is skipped (a finished tile costs its log writes only).  Kept as a separate
                // arm: sharing vhjb_step_env behind a conditional network call made hipcc spill the prefetched weights.
#pragma unroll
                for (int q = 0; q < N; ++q) xo[q] = xs[0][q];
#pragma unroll
                for (int j = 0; j < M; ++j) u[j] = 0.0f;
                cst = dn = res = 0.0f;
            } else {
                float V[1], g[1][N];
                if constexpr (HEAD::kSoft) mlp_value_grad<S, 1, ACT, true>(sys, p, c, xs, true, V, g, &L.bias);
                else MlpArith<AR>::template value_grad<S, 1, ACT>(sys, p, c, xs, true, V, g);
                vhjb_step_env<INTEG>(sys, tk, lim, t_first + k, T_max, o.resid != nullptr, xs[0], g[0], ds, xo, u, cst, dn, res);
            }
            if (writer) {
                const int64_t row = (int64_t)k * B + env;
                o.cost[row] = cst;
                o.done[row] = dn;
                if (o.resid) o.resid[row] = res;
                if (o.u_log) store_row<M>(o.u_log + (int64_t)k * B * M, env, u);
                if (o.traj) store_row<N>(o.traj + (int64_t)(k + 1) * B * N, env, xo);
            }
#pragma unroll
            for (int q = 0; q < N; ++q) xs[0][q] = xo[q];
        }
        if (writer) {
            o.done_step[env] = ds;
            if (o.x_out) store_row<N>(o.x_out, env, xs[0]);
        }
        grp = next_group();
    }
    // the last wave of the last workgroup leaves the workspace zeroed for the next launch
    int lastw = 0;
    if (lane == 0 && atomicAdd(&waves_done, 1) == WAVES - 1) lastw = __hip_atomic_fetch_add(ws + kWsExited, 1u, HJBX_RLX_AGENT) == (unsigned)(G - 1);
    if (__builtin_amdgcn_readfirstlane(lastw)) {
        for (int w = lane; w < kWsWords; w += 64)
            if (w < kWsFlags || (w - kWsFlags) % kMaxGrid < G) __hip_atomic_store(ws + w, 0u, HJBX_RLX_AGENT);
    }
}
