// hjbx_train_coop.hip -- the parameter gradient of the value-learning step (reference controller/vhjb.py:227-253, 282-284) in ONE kernel with
// NO scratch in HBM (round 3; hjbx_train.hip holds the round-2 pair of kernels, which moved 10 KB per sample through HBM and walked a tile's
// 1,552 MFMAs on one wave).  ReLU (controller/vhjb.py), tanh (examples/cartpole_balancing.ipynb cell 6) and sin
// (examples/double_integrator_optimal_time.ipynb cell 5) networks, float32 MFMA.
//
// Math per sample (s = act'(a); ReLU: act'' = 0, tanh: act'' = -2 h s, sin: act'' = -h), q = d loss_hjb / d gradV, r = d loss_term / d V:
//   forward            h1 = act(W1'z)   h2 = act(W2'h1)   y = W3'h2   V = |y|^2 + eps_s |e|^2
//   input gradient     dy = 2y   d2 = (W3 dy).s2   d1 = (W2 d2).s1   g = (W1 d1)/std + 2 eps_s e
//   reverse sweep (q)  gzb = q/std   t1 = W1'gzb   dh1b = t1.s1   t2 = W2'dh1b   dh2b = t2.s2   yb = 2 W3'dh2b
//                      a2b = (W3 yb).s2 - 2 h2.d2.t2 [tanh] - h2.(W3 dy).t2 [sin]      a1b = (W2 a2b).s1 - 2 h1.d1.t1 [tanh] - h1.(W2 d2).t1 [sin]
//   hjb gradient       dW1 = gzb (x) d1 + z (x) a1b      dW2 = dh1b (x) d2 + h1 (x) a2b      dW3 = dh2b (x) dy + h2 (x) yb
//   termination grad.  dW1 = z (x) (r d1)                dW2 = h1 (x) (r d2)                 dW3 = h2 (x) (r dy)
// (the second-order terms of tanh: the adjoint of s = 1 - h^2 is (adjoint of d).(W d_next) and d s / d a = -2 h s, so a_bar gains
//  -2 h . d . t with t the pre-mask value of the reverse sweep.)
//
// Design.  A workgroup = 4 waves = one wave per SIMD with 512 registers; it works on ONE 32-sample tile at a time, COOPERATIVELY:
//  * every 128-wide array (h1, h2, d2, d1, ...) is split by 32-feature block over the four waves, so a product W'X is 64 k-steps of ONE
//    MFMA per wave instead of 256 MFMAs on one wave (latency of a tile / 4: what the reference's minibatch of 256 = 8 tiles needs), and
//    each wave keeps its blocks of h1, h2, dy, d1 (and the tanh corrections) in registers across the whole tile;
//  * a product needs all 128 input features as B operands, so each result block goes through a [feature][sample] image in LDS (stride 33:
//    conflict-free for the column-wise write, the chain's B read and the outer products' A / B reads alike).  Those images ARE the
//    transposition the outer products need (their contraction index is the sample): no scratch, no second kernel.  Three 16.5-KiB
//    images suffice; h1, h2, dy are written again from registers when their partner of an outer product arrives;
//  * the 48 32x32 output blocks of dW2 / dW3 (hjb + termination sets) are MFMA accumulators for the whole launch, 12 per wave (row block
//    w of dW2 and of dW3: their A operands are shared); dW1 (n x 128: 3 % of the flops) is accumulated on the VALU, one feature per thread;
//  * y = W3'h2 has only two 32-row blocks: its contraction is split in halves over wave pairs and summed through LDS, so all four matrix
//    pipes work in every phase.  g = W1 d1 is a 16-k-step MFMA per wave over its own block (B operands straight from the accumulators) +
//    an LDS sum; every wave then evaluates the two residuals for its sample redundantly (same bits) instead of waiting for one.
// LDS: weights 102-104 KB (f32, odd strides, one copy for W and W') + 3 x 16.5 KB images + 5 KB small = 157 KB (n = 10).
// Per tile and wave: 394 chain MFMAs + 336 outer-product MFMAs; HBM traffic = the inputs (4(n+2) B per sample) + the partial sums.
// The device side (CoopLds, the chains, the outer products, k_train_coop) is in hjbx_train_coop_kernels.hpp, which hiprtc compiles as well: a
// user-defined system gets the same kernel for its own struct at run time (hjbx_user_train_kernels.hpp, launch_coop_user below).
#include <hip/hip_runtime.h>
#include <type_traits>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"
#include "hjbx_host.hpp"
#include "hjbx_mlp_core.hpp"
#include "hjbx_adam.hpp"
#include "hjbx_train_coop_kernels.hpp"
#include "hjbx_mlp_host.hpp"

using namespace hjbx;

// Sum of `count` records base[g stride] in a FIXED order: eight interleaved running sums (eight loads in flight: these reductions are latency
// bound at the reference's minibatch), then ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).  Two of them at once for the fused epilogue.
__device__ __forceinline__ float coop_sum8(const float* __restrict__ base, int64_t stride, int count) {
    float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int gI = 0;
    for (; gI + 8 <= count; gI += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s8[k] += base[(int64_t)(gI + k) * stride];
    }
    for (int k = 0; gI < count; ++gI, ++k) s8[k] += base[(int64_t)gI * stride];
    return ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
}
__device__ __forceinline__ void coop_sum8x2(const float* __restrict__ a, const float* __restrict__ b, int64_t stride, int count, float& sa, float& sb) {
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int gI = 0;
    for (; gI + 8 <= count; gI += 8) {
        float va[8], vb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { va[k] = a[(int64_t)(gI + k) * stride]; vb[k] = b[(int64_t)(gI + k) * stride]; }   // sixteen loads in flight
#pragma unroll
        for (int k = 0; k < 8; ++k) { p[k] += va[k]; q[k] += vb[k]; }
    }
    for (int k = 0; gI < count; ++gI, ++k) { p[k] += a[(int64_t)gI * stride]; q[k] += b[(int64_t)gI * stride]; }
    sa = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    sb = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
}

// dW1: two records (sample halves) per owning workgroup.  psplit = 1: the 2 nparts records in order (one sequence); psplit = 4: the owners are the
// workgroups 0, 4, 8, ..., i.e. the records 8 ts + half -- the two halves as two sequences, added at the end
template <int N> __device__ __forceinline__ float coop_sum_w1(const float* __restrict__ base /* partial_w1 + (set, k, f) */, int nparts, int psplit) {
    if (psplit != 4) return coop_sum8(base, 2 * N * 128, 2 * nparts);
    float s0, s1;
    coop_sum8x2(base, base + 2 * N * 128, (int64_t)8 * (2 * N * 128), nparts / 4, s0, s1);
    return s0 + s1;
}

// Which workgroups hold a block of the partial sums.  psplit = 1: every workgroup, all of it.  psplit = 4 (k_train_coop<.., PS = 4, ..>: four
// workgroups per tile): output block b of dW2 / dW3 lives only in the workgroups whose part is b's column block, dW1 and the loss sums only in
// part 0 -- a quarter of the records to add at the reference's minibatch.  -> first workgroup, step between workgroups, number of them
struct CoopOwners { int first, step, count; };
__device__ __forceinline__ CoopOwners coop_owners(int b /* block within its set, or -1: dW1 / loss sums */, int nparts, int psplit) {
    if (psplit != 4) return CoopOwners{0, 1, nparts};
    const int jb = b < 0 ? 0 : (b < 16 ? (b & 3) : ((b - 16) & 1));
    return CoopOwners{jb, 4, nparts / 4};
}

// ---- partial sums -> flat gradient buffer, in workgroup order ---------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_train_coop_reduce(const float* __restrict__ partial, const float* __restrict__ partial_w1, int nparts, int psplit,
                                                          const double* __restrict__ sums_rec, float* __restrict__ flat) {
    constexpr int P = N * kH1 + kH1 * kH2 + kH2 * kH3;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < kCoopBlocks * 1024) {
        const CoopOwners ow = coop_owners((t >> 10) % kCoopSet, nparts, psplit);
        const float s = coop_sum8(partial + (int64_t)ow.first * kCoopBlocks * 1024 + t, (int64_t)ow.step * kCoopBlocks * 1024, ow.count);
        const int blk = t >> 10, reg = (t >> 6) & 15, lane = t & 63;
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col = lane & 31;
        const int set = blk / kCoopSet, b = blk % kCoopSet;
        float* o = flat + set * P;
        if (b < 16) o[N * kH1 + (32 * (b >> 2) + row) * kH2 + 32 * (b & 3) + col] = s;
        else o[N * kH1 + kH1 * kH2 + (32 * ((b - 16) >> 1) + row) * kH3 + 32 * ((b - 16) & 1) + col] = s;
    } else if (t < kCoopBlocks * 1024 + 2 * N * 128) {
        const int u = t - kCoopBlocks * 1024;          // (set, k, f)
        const int set = u / (N * 128), kf = u % (N * 128);
        flat[set * P + kf] = coop_sum_w1<N>(partial_w1 + u, nparts, psplit);
    } else if (t < kCoopBlocks * 1024 + 2 * N * 128 + 4) {
        const int k = t - (kCoopBlocks * 1024 + 2 * N * 128);
        const CoopOwners ow = coop_owners(-1, nparts, psplit);
        double s = 0;
        for (int g = 0; g < ow.count; ++g) s += sums_rec[4 * (ow.first + g * ow.step) + k];
        flat[2 * P + k] = (float)s;
    }
}

// ---- partial sums -> mixed gradient -> Adam, in workgroup order, one launch (hjbx_value_loss_adam_f32) ------------------------------------
// The same sums in the same order as k_train_coop_reduce, but each thread takes ONE parameter of BOTH sets (hjb, termination), divides by the
// counts, mixes (vhjb.py:241, 253, 284) and applies optax.adam's update (hjbx_adam.hpp) to it: the flat buffer is never written.  At the
// reference's minibatch this removes one launch-bound kernel from the update (gather -> gradient -> this).
template <int N>
__global__ __launch_bounds__(256) void k_train_coop_update(const float* __restrict__ partial, const float* __restrict__ partial_w1, int nparts, int psplit,
                                                          const double* __restrict__ sums_rec, AdamArgs a, MixArgs mx, GatherArgs next) {
    __shared__ float sc[2];
    __shared__ double tot[4];
    __shared__ double rec[4 * kCoopMaxGrid];          // the loss-sum records of the workgroups (at most one workgroup per CU)
    // Order of work: everything that needs no other thread first -- thread 0's bias corrections (double pow), the records into LDS, and each
    // thread's own long sums over the workgroups -- then ONE barrier, the four scalar totals, a second barrier, mix + Adam.  (Written in
    // program order -- coefficients, totals, sums -- every thread waited through two serial latencies before it started its loads: 54 us per
    // 256-sample update instead of 47.)
    const float tstep = adam_coef_begin(a, sc);
    for (int idx = threadIdx.x; idx < 4 * nparts; idx += 256) rec[idx] = sums_rec[idx];
    const int t = blockIdx.x * 256 + threadIdx.x;
    float sh = 0.f, st = 0.f;
    int which = -1;
    int64_t j = 0;
    if (t < kCoopSet * 1024) {
        const int b = t >> 10, reg16 = (t >> 6) & 15, lane = t & 63;
        const CoopOwners ow = coop_owners(b, nparts, psplit);
        const float* src = partial + (int64_t)ow.first * kCoopBlocks * 1024 + t;
        coop_sum8x2(src, src + kCoopSet * 1024, (int64_t)ow.step * kCoopBlocks * 1024, ow.count, sh, st);
        const int row = (reg16 & 3) + 8 * (reg16 >> 2) + 4 * (lane >> 5), col = lane & 31;
        if (b < 16) { which = 1; j = (int64_t)(32 * (b >> 2) + row) * kH2 + 32 * (b & 3) + col; }
        else { which = 2; j = (int64_t)(32 * ((b - 16) >> 1) + row) * kH3 + 32 * ((b - 16) & 1) + col; }
    } else if (t < kCoopSet * 1024 + N * 128) {
        const int kf = t - kCoopSet * 1024;            // (k, f) of W1
        sh = coop_sum_w1<N>(partial_w1 + kf, nparts, psplit);
        st = coop_sum_w1<N>(partial_w1 + N * 128 + kf, nparts, psplit);
        which = 0; j = kf;
    }
    __syncthreads();
    if (threadIdx.x < 4) {   // loss sums and counts: the records in workgroup order, like k_train_coop_reduce (every workgroup computes them)
        const CoopOwners ow = coop_owners(-1, nparts, psplit);
        double s = 0;
        for (int g = 0; g < ow.count; ++g) s += rec[4 * (ow.first + g * ow.step) + threadIdx.x];
        tot[threadIdx.x] = (double)(float)s;          // (the flat buffer holds them as float32)
    }
    __syncthreads();
    const AdamCoef c = adam_coef_end(a, tstep, sc);
    const float reg = mx.reg_dev ? mx.reg_dev[0] : mx.reg_host;
    const float ih = 1.0f / ((float)tot[2] + mx.eps), it = 1.0f / ((float)tot[3] + mx.eps);
    const float wt = reg * it;
    if (which >= 0) adam_element(a, c, which, j, sh * ih + st * wt);
    // the NEXT update's minibatch (index = this update's + 1; every workgroup reads the counter before the last one increments it below): its
    // rows by all threads, its regularisation weight by the last workgroup -- the buffer may be the one this launch read `reg` from
    const int64_t k_next = next.enabled && mx.step_counter ? (int64_t)mx.step_counter[0] + 1 : 0;
    if (next.enabled) gather_elements(next, k_next, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
    if (adam_finish(a, c, mx, (float)tot[0] * ih, (float)tot[1] * it, reg) && next.enabled) gather_reg(next, k_next);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
struct CoopWs { size_t partial, partial_w1, sums, total; int grid, psplit; };
static CoopWs coop_ws(int64_t B, int n) {
    CoopWs w{};
    int n_cu = hjbx_device_cus();
    if (n_cu <= 0) n_cu = 256;
    const int64_t ntiles = (B + 31) / 32;
    w.psplit = 4 * ntiles <= n_cu ? 4 : 1;                             // workgroups per tile (small batches: see k_train_coop)
    w.grid = (int)(ntiles * w.psplit < n_cu ? ntiles * w.psplit : n_cu);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    w.partial = up((size_t)w.grid * kCoopBlocks * 1024 * sizeof(float));
    w.partial_w1 = up((size_t)w.grid * 2 * 2 * n * 128 * sizeof(float));
    w.sums = up((size_t)w.grid * 4 * sizeof(double));
    w.total = w.partial + w.partial_w1 + w.sums;
    return w;
}

size_t hjbx_train_coop_workspace_bytes(int64_t B, int n) { return B > 0 ? coop_ws(B, n).total : 0; }

// Everything of a launch but k_train_coop itself: the checks of the fused epilogue's arguments (BEFORE the first launch: an HJBX_EINVAL leaves
// no gradient kernel behind), the by-value argument structs for (N, M), the workspace split, then `main` -- which enqueues k_train_coop for
// its system: the library's own instantiation (launch_coop) or a user system's run-time compiled one (launch_coop_user) -- and the
// library's reduce / update epilogue, which depends on N only.
struct CoopCall {
    const float *W1, *W2, *W3, *x, *cost, *done;
    float eps_term;
    float *partial, *partial_w1;
    double* sums;
    int64_t B, ntiles;
    int grid, psplit;
};
template <int N, int M, typename Main>
static int launch_coop_nm(const hjbx_system* sysh, const hjbx_task* task, const hjbx_mlp* mlp, const float* x, const float* cost, const float* done,
                          float* flat, void* workspace, int64_t B, void* st, const FuseArgs* fuse, Main&& main) {
    static_assert(N % 2 == 0 && N <= HJBX_MAX_N, "state dimension");
    if (hjbx_device_cus() <= 0) return hjbx_set_error(HJBX_ENODEVICE, "hjbx_value_loss_grad_f32: no HIP device");
    const CoopWs w = coop_ws(B, N);
    if (fuse) {
        if (fuse->a.end0 != N * kH1 || fuse->a.end1 - fuse->a.end0 != kH1 * kH2 || fuse->a.P - fuse->a.end1 != kH2 * kH3)
            return hjbx_set_error(HJBX_EINVAL, "hjbx_value_loss_adam_f32: the Adam state's tensors must be W1 (%d x 128), W2 (128 x 128), W3 (128 x 64)", N);
        if (w.grid > kCoopMaxGrid) return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_value_loss_adam_f32: %d workgroups (more than %d CUs?)", w.grid, kCoopMaxGrid);
    }
    const MlpP<N> p = make_mlp_params<N>(make_net(mlp));
    const auto tk = make_task<float, N, M>(task);
    const auto lim = make_limits<float, M>(sysh);
    CoopCall c{(const float*)mlp->W1, (const float*)mlp->W2, (const float*)mlp->W3, x, cost, done, (float)task->eps, (float*)workspace,
               (float*)((char*)workspace + w.partial), (double*)((char*)workspace + w.partial + w.partial_w1), B, (B + 31) / 32, w.grid, w.psplit};
    hipStream_t s = (hipStream_t)st;
    if (int rc = main(c, p, tk, lim, s)) return rc;
    if (fuse) {
        const int nthreads = kCoopSet * 1024 + N * 128;
        hipLaunchKernelGGL((k_train_coop_update<N>), dim3((nthreads + 255) / 256), dim3(256), 0, s, c.partial, c.partial_w1, w.grid, w.psplit, c.sums, fuse->a, fuse->mx, fuse->next);
    } else {
        const int nthreads = kCoopBlocks * 1024 + 2 * N * 128 + 4;
        hipLaunchKernelGGL((k_train_coop_reduce<N>), dim3((nthreads + 255) / 256), dim3(256), 0, s, c.partial, c.partial_w1, w.grid, w.psplit, c.sums, flat);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "hjbx_value_loss_grad_f32: %s", hipGetErrorString(e));
    return HJBX_OK;
}

template <typename S>
static int launch_coop(const hjbx_system* sysh, S sys, const hjbx_task* task, const hjbx_mlp* mlp, int mode, const float* x, const float* cost,
                       const float* done, float* flat, void* workspace, int64_t B, void* st, const FuseArgs* fuse) {
    constexpr int N = S::N, M = S::M;
    if constexpr (N % 2 != 0 || N > HJBX_MAX_N) {
        return HJBX_EUNSUPPORTED;
    } else {
        return launch_coop_nm<N, M>(sysh, task, mlp, x, cost, done, flat, workspace, B, st, fuse,
                                    [&](const CoopCall& c, const MlpP<N>& p, const TaskP<float, N, M>& tk, const Limits<float, M>& lim, hipStream_t s) -> int {
            auto go = [&](auto mode_c, auto act_c) {
                if (c.psplit == 4)
                    hipLaunchKernelGGL((k_train_coop<decltype(mode_c)::value, decltype(act_c)::value, 4, S>), dim3(c.grid), dim3(256), 0, s, sys, p, tk, lim, c.W1, c.W2,
                                       c.W3, c.x, c.cost, c.done, c.eps_term, c.partial, c.partial_w1, c.sums, c.B, c.ntiles);
                else
                    hipLaunchKernelGGL((k_train_coop<decltype(mode_c)::value, decltype(act_c)::value, 1, S>), dim3(c.grid), dim3(256), 0, s, sys, p, tk, lim, c.W1, c.W2,
                                       c.W3, c.x, c.cost, c.done, c.eps_term, c.partial, c.partial_w1, c.sums, c.B, c.ntiles);
            };
            auto with_act = [&](auto mode_c) {
                if (mlp->activation == HJBX_ACT_TANH) go(mode_c, std::integral_constant<int, HJBX_ACT_TANH>{});
                else if (mlp->activation == HJBX_ACT_SIN) {
                    // sin keeps act' = cos(a) beside the activations (32 registers) and its second-order factors from steps 4 / 5 on: with the
                    // state-sized registers of a 6-D or 10-D residual that is 9-12 registers over the 512 of a wave -- n <= 4 only (the network
                    // belongs to the 2-D double integrator of the time-optimal notebook); larger systems keep the autograd path
                    if constexpr (N <= 4) go(mode_c, std::integral_constant<int, HJBX_ACT_SIN>{});
                }
                else go(mode_c, std::integral_constant<int, HJBX_ACT_RELU>{});
            };
            if (mode == HJBX_RESIDUAL_NORMALISED) with_act(std::integral_constant<int, 0>{});
            else with_act(std::integral_constant<int, 1>{});
            return HJBX_OK;
        });
    }
}

// A user-defined system (HJBX_SYS_USER with the matrix-core kernels enabled): the same call with k_train_coop<.., UserSystem<float>> taken from
// the handle's run-time compiled train unit (hjbx_user_train_kernels.hpp; compiled at the first call for this activation, refused as a whole
// when one of its four kernels needs scratch) and launched through the module API -- 256 threads, the kernel's static LDS.  The by-value
// structs are built here from the same headers the unit was compiled from.
static int launch_coop_user(const hjbx_system* sysh, const hjbx_task* task, const hjbx_mlp* mlp, int mode, const float* x, const float* cost,
                            const float* done, float* flat, void* workspace, int64_t B, void* st, const FuseArgs* fuse, const char* who) {
    if (int rc = hjbx_user_train_unit(sysh, mlp->activation, who)) return rc;     // (before any launch; remembered when refused)
    return with_mc_dims(sysh, who, "fused parameter gradient", [&](auto Nc, auto Mc) -> int {
        constexpr int N = decltype(Nc)::value, M = decltype(Mc)::value;
        return launch_coop_nm<N, M>(sysh, task, mlp, x, cost, done, flat, workspace, B, st, fuse,
                                    [&](const CoopCall& c, const MlpP<N>& p, const TaskP<float, N, M>& tk, const Limits<float, M>& lim, hipStream_t s) -> int {
            auto blob = user_blob<float>(sysh);     // the kernel's arguments in order
            void* a[] = {&blob, (void*)&p, (void*)&tk, (void*)&lim, (void*)&c.W1, (void*)&c.W2, (void*)&c.W3, (void*)&c.x, (void*)&c.cost, (void*)&c.done,
                         (void*)&c.eps_term, (void*)&c.partial, (void*)&c.partial_w1, (void*)&c.sums, (void*)&c.B, (void*)&c.ntiles};
            return hjbx_user_train_launch(sysh, mlp->activation, mode == HJBX_RESIDUAL_NORMALISED ? 0 : 1, c.psplit, (unsigned)c.grid, a, s, who);
        });
    });
}

// called by hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 (hjbx_train.hip) after they have validated their arguments
int hjbx_train_coop(const hjbx_system* sys, const hjbx_task* task, const hjbx_mlp* mlp, int mode, const float* x, const float* cost, const float* done,
                    float* flat, void* workspace, int64_t B, void* stream, const FuseArgs* fuse) {
    const char* who = fuse ? "hjbx_value_loss_adam_f32" : "hjbx_value_loss_grad_f32";
    if (mlp->activation == HJBX_ACT_SIN && sys->n > 4)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: the sin network's fused parameter gradient exists for n <= 4 (n = %d)", who, sys->n);
    if (sys->kind == HJBX_SYS_USER) return launch_coop_user(sys, task, mlp, mode, x, cost, done, flat, workspace, B, stream, fuse, who);
    int rc = HJBX_EUNSUPPORTED;
    const bool ok = with_system<float>(sys, [&](auto S) {
#ifdef HJBX_TRAIN_DEV   // development builds: cartpole and the 10-D quadcopter only
        if constexpr (std::is_same<decltype(S), Cartpole<float>>::value || std::is_same<decltype(S), NearHover<float>>::value)
#endif
            rc = launch_coop<decltype(S)>(sys, S, task, mlp, mode, x, cost, done, flat, workspace, B, stream, fuse);
    });
    if (!ok || rc == HJBX_EUNSUPPORTED)
        return hjbx_set_error(HJBX_EUNSUPPORTED, "hjbx_value_loss_grad_f32: no kernel for system kind %d with n=%d m=%d", sys->kind, sys->n, sys->m);
    return rc;
}
