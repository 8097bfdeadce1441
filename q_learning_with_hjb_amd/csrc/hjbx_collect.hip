// The statistics train() reports about a batch of rollouts, taken from the time-major cost log where it lies: the cost of every trajectory
// and, over the batch, their sum, their squared deviations from the mean and the number of tuples.
//
// reference: controller/vhjb.py:302-307 (the trajectories of an epoch), :326-329 (np.mean / np.var(...)**0.5 of their costs, mean length).
//
// One lane per environment: lane b walks cost[0..done_step[b], b] in time order, a sequential float64 chain, so traj_cost[b] is THE
// left-to-right sum (bit-equal to np.cumsum of the float64-cast column).  At a fixed t the lanes of a wave read adjacent b: every load is
// one coalesced segment, and nothing beyond done_step[b] is read (a NaN there stays unseen).  Work and traffic follow the valid tuples.
//
// Two launches on one stream, no host synchronisation between them, both with the same grid and the same environment-to-thread map:
//   k_cost_sums  : the chains -> traj_cost (if asked for); {sum c, 0, sum (done_step + 1)} through block_sum3 -> stats[0..2]; stats[3] = B
//   k_cost_spread: d = c_b - stats[0] / B (c_b read back from traj_cost, or walked again when there is none) and
//                  {sum c, sum d^2, sum (done_step + 1)} through block_sum3 -> stats[0..2]
// block_sum3 (hjbx_stream_kernels.hpp) is the library's deterministic reduction: fixed shuffle trees, per-workgroup records in the caller's
// reduce workspace, the last workgroup to arrive adds them in index order; no float atomics, the tickets left at zero.  The second launch
// forms stats[0] and stats[2] again from the same numbers in the same order, so it rewrites them with the bits they already hold -- and its
// only writer is the workgroup that arrives last, after every workgroup has read the mean.
#include <hip/hip_runtime.h>

#include "hjbx_internal.hpp"
#include "hjbx_stream_kernels.hpp"

using namespace hjbx;

namespace {

constexpr int kAhead = 4;      // loads of one chain issued before their adds

// tuples of environment b that count: done_step[b] + 1, held to [0, S] so that no content of done_step leads outside the log
__device__ inline int64_t tuples_of(const int32_t* __restrict__ done_step, int64_t b, int64_t S) {
    const int64_t L = (int64_t)done_step[b] + 1;
    return L < 0 ? 0 : (L > S ? S : L);
}

// float64 sum of cost[0..L-1, b], left to right
template <typename T> __device__ inline double chain_sum(const T* __restrict__ cost, int64_t b, int64_t B, int64_t L) {
    double c = 0.0;
    const T* p = cost + b;
    int64_t t = 0;
    for (; t + kAhead <= L; t += kAhead) {
        T v[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) v[k] = p[(t + k) * B];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) c += (double)v[k];
    }
    for (; t < L; ++t) c += (double)p[t * B];
    return c;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_cost_sums(const T* __restrict__ cost, const int32_t* __restrict__ done_step, int64_t S, int64_t B,
                                                      double* __restrict__ traj_cost, double* __restrict__ stats, unsigned char* ws) {
    double acc_c = 0.0, acc_l = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kBlock) {
        const int64_t L = tuples_of(done_step, b, S);
        const double c = chain_sum<T>(cost, b, B, L);
        if (traj_cost) traj_cost[b] = c;
        acc_c += c;
        acc_l += (double)L;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[3] = (double)B;
    block_sum3<double>(acc_c, 0.0, acc_l, ws, stats);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_cost_spread(const T* __restrict__ cost, const int32_t* __restrict__ done_step, int64_t S, int64_t B,
                                                        const double* __restrict__ traj_cost, double* stats, unsigned char* ws) {
    const double mean = __hip_atomic_load(stats, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / (double)B;
    double acc_c = 0.0, acc_d = 0.0, acc_l = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kBlock) {
        const int64_t L = tuples_of(done_step, b, S);
        const double c = traj_cost ? traj_cost[b] : chain_sum<T>(cost, b, B, L);
        const double d = c - mean;
        acc_c += c;
        acc_d += d * d;
        acc_l += (double)L;
    }
    block_sum3<double>(acc_c, acc_d, acc_l, ws, stats);
}

template <typename T>
int cost_stats(const char* who, const T* cost, const int32_t* done_step, int64_t S, int64_t B, double* traj_cost, double* stats, void* workspace,
               void* stream_) {
    if (!cost || !done_step || !stats || !workspace) return hjbx_set_error(HJBX_EINVAL, "%s: NULL buffer", who);
    if (B < 0 || S < 1) return hjbx_set_error(HJBX_EINVAL, "%s: B = %lld, S = %lld", who, (long long)B, (long long)S);
    if ((uintptr_t)cost % sizeof(T) || (uintptr_t)done_step % 4 || (uintptr_t)traj_cost % 8 || (uintptr_t)stats % 8 || (uintptr_t)workspace % 16)
        return hjbx_set_error(HJBX_EINVAL, "%s: misaligned buffer", who);
    if (B == 0) return HJBX_OK;
    hipStream_t stream = (hipStream_t)stream_;
    int64_t g = (B + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(g < kReduceBlocks ? g : kReduceBlocks));
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL((k_cost_sums<T>), grid, dim3(kBlock), 0, stream, cost, done_step, S, B, traj_cost, stats, ws);
    hipLaunchKernelGGL((k_cost_spread<T>), grid, dim3(kBlock), 0, stream, cost, done_step, S, B, (const double*)traj_cost, stats, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

}  // namespace

extern "C" int hjbx_rollout_cost_stats_f32(const float* cost, const int32_t* done_step, int64_t S, int64_t B, double* traj_cost, double* stats,
                                           void* workspace, void* stream) {
    return cost_stats<float>("hjbx_rollout_cost_stats_f32", cost, done_step, S, B, traj_cost, stats, workspace, stream);
}

extern "C" int hjbx_rollout_cost_stats_f64(const double* cost, const int32_t* done_step, int64_t S, int64_t B, double* traj_cost, double* stats,
                                           void* workspace, void* stream) {
    return cost_stats<double>("hjbx_rollout_cost_stats_f64", cost, done_step, S, B, traj_cost, stats, workspace, stream);
}
