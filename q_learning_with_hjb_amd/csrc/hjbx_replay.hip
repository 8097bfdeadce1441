// The seam between the rollout and the fit phase: the (x, cost, done) tuples of a time-major rollout log appended to the device-resident replay
// ring, trajectory by trajectory, without a transposed copy of the log and with work proportional to what lands in the ring.
//
// reference: controller/vhjb.py:304-308 (trajectory = rollout_trajectory(); replay_buffer.xs.extend(trajectory)) on the deque(maxlen) of :62-73.
//
// Index arithmetic (include/hjbx.h): environment b emits L_b = done_step[b] + 1 records; off_b = exclusive prefix sum of L, K = sum L,
// drop = max(0, K - capacity); record (b, t) has running index j = off_b + t and lands, iff j >= drop, in slot (head + j - drop) mod capacity.
//
// Three launches on one stream, no persistent state (the workspace needs no initialisation):
//   k_append_slice_sums : sum of L and count of out-of-range done_step entries per SLICE of 64 consecutive environments (one wavefront each)
//   k_append_scan       : one workgroup turns the slice sums into exclusive slice offsets (+ the total) and writes the header
//   k_append_copy       : workgroup (slice, chunk of time tiles) redoes the scan inside its slice and moves tiles of 64 environments x TT steps
//                         through LDS: global loads run along b (contiguous in the log for a fixed t), global stores along t (contiguous in the
//                         ring for a fixed b).  Workgroups whose slice lies entirely below `drop` leave after reading two offsets.
// Records are moved as raw words of the widest size that divides the record and that the pointers are aligned to: 16 bytes (n = 4, 8 in
// float32, even n in float64: one dwordx4 per cartpole record), else 8 bytes (the other even n in float32 -- a ring row of n = 6 or 10 floats
// starts on an 8-byte boundary only -- and odd n in float64), else 4 bytes.
#include <hip/hip_runtime.h>

#include "hjbx_internal.hpp"

namespace {

constexpr int kSlice = 64;            // environments per slice: one wavefront scans it
constexpr int kCopyThreads = 256;
constexpr int kScanThreads = 1024;

// time steps per tile: 64 x TT records of at most 40 bytes (41.5 KiB with the padding), 8 steps for the longer records of float64,
// plus the cost tile: at most 47 KiB of LDS per workgroup, three workgroups per CU
__host__ __device__ constexpr int tile_steps(int record_bytes) { return record_bytes > 40 ? 8 : 16; }

struct alignas(16) Word16 { uint64_t lo, hi; };

struct AppendArgs {
    const void* traj; const void* cost; const int32_t* done_step;
    int64_t T, B;
    void* buf_x; void* buf_cost; void* buf_done;
    int64_t capacity, head;
    const int64_t* off;        // (nslice + 1): exclusive slice offsets, off[nslice] = K
    const int64_t* header;
    int64_t nslice;
};

__device__ inline long long wave_inclusive_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// records of environment e (0 when it lies past B or its done_step is outside [0, T])
__device__ inline long long records_of(const int32_t* __restrict__ done_step, int64_t e, int64_t B, int64_t T, int* bad) {
    if (e >= B) return 0;
    const int64_t d = done_step[e];
    if (d < 0 || d > T) { *bad = 1; return 0; }
    return d + 1;
}

__global__ __launch_bounds__(256) void k_append_slice_sums(const int32_t* __restrict__ done_step, int64_t B, int64_t T, int64_t nslice,
                                                          int64_t* __restrict__ sums, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= nslice) return;      // (wave uniform)
    int b = 0;
    long long L = records_of(done_step, s * kSlice + lane, B, T, &b);
#pragma unroll
    for (int o = 32; o; o >>= 1) { L += __shfl_xor(L, o, 64); b += __shfl_xor(b, o, 64); }
    if (lane == 0) { sums[s] = L; bad[s] = b; }
}

// in place: off[i] = sum of the slice sums before i, off[nslice] = K; header = {K, drop, #bad, 0}
__global__ __launch_bounds__(kScanThreads) void k_append_scan(int64_t* __restrict__ off, const int32_t* __restrict__ bad, int64_t nslice, int64_t capacity,
                                                             int64_t* __restrict__ header) {
    __shared__ long long wsum[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long long carry = 0, nbad = 0;
    for (int64_t base = 0; base < nslice; base += kScanThreads) {
        const int64_t i = base + tid;
        const long long v = i < nslice ? off[i] : 0;
        if (i < nslice) nbad += bad[i];
        const long long inc = wave_inclusive_scan(v, lane);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kScanThreads / 64; ++k) { const long long x = wsum[k]; before += k < w ? x : 0; total += x; }
        if (i < nslice) off[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
    if (lane == 0) wsum[w] = nbad;
    __syncthreads();
    if (tid == 0) {
        long long nb = 0;
        for (int k = 0; k < kScanThreads / 64; ++k) nb += wsum[k];
        off[nslice] = carry;
        header[0] = carry;
        header[1] = carry > capacity ? carry - capacity : 0;
        header[2] = nb;
        header[3] = 0;
    }
}

// W: the word a record is moved in (NW words per record); CW: the word of a cost / done entry
template <typename W, int NW, typename CW>
__global__ __launch_bounds__(kCopyThreads) void k_append_copy(AppendArgs a) {
    constexpr int TT = tile_steps(NW * (int)sizeof(W));
    constexpr int XS = TT * NW + 1;     // words per environment in the tile, odd: the strided side (the LDS stores of the load phase) spreads over the banks
    constexpr int CS = TT + 1;
    constexpr CW kOne = sizeof(CW) == 4 ? (CW)0x3f800000u : (CW)0x3ff0000000000000ull;       // 1.0f / 1.0
    __shared__ W sx[kSlice * XS];
    __shared__ CW sc[kSlice * CS];
    __shared__ long long soff[kSlice], sL[kSlice];
    __shared__ long long smax;

    if (a.header[2] != 0) return;                                   // an out-of-range done_step: the call appends nothing
    const int64_t K = a.off[a.nslice], cap = a.capacity;
    const int64_t drop = K > cap ? K - cap : 0;
    const int64_t s = blockIdx.x;
    if (a.off[s + 1] <= drop) return;                               // every record of this slice falls off the ring again
    const int tid = threadIdx.x;
    const int64_t e0 = s * kSlice, B = a.B;
    if (tid < kSlice) {
        int bad = 0;
        const long long L = records_of(a.done_step, e0 + tid, B, a.T, &bad);
        soff[tid] = a.off[s] + wave_inclusive_scan(L, tid) - L;
        sL[tid] = L;
        long long m = L;
#pragma unroll
        for (int o = 32; o; o >>= 1) { const long long u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
        if (tid == 0) smax = m;
    }
    __syncthreads();
    const int64_t maxL = smax;
    const W* __restrict__ traj = (const W*)a.traj;
    const CW* __restrict__ cost = (const CW*)a.cost;
    W* __restrict__ bx = (W*)a.buf_x;
    CW* __restrict__ bc = (CW*)a.buf_cost;
    CW* __restrict__ bd = (CW*)a.buf_done;

    for (int64_t t0 = (int64_t)blockIdx.y * TT; t0 < maxL; t0 += (int64_t)gridDim.y * TT) {
        // log -> LDS: consecutive lanes walk the words of consecutive environments at one time step
        for (int idx = tid; idx < TT * kSlice * NW; idx += kCopyThreads) {
            const int tl = idx / (kSlice * NW), r = idx % (kSlice * NW), e = r / NW, c = r % NW;
            const int64_t t = t0 + tl;
            if (t < sL[e] && soff[e] + t >= drop) sx[e * XS + tl * NW + c] = traj[((t * B + e0 + e) * NW) + c];
        }
        for (int idx = tid; idx < TT * kSlice; idx += kCopyThreads) {
            const int tl = idx / kSlice, e = idx % kSlice;
            const int64_t t = t0 + tl;
            if (t < sL[e] && soff[e] + t >= drop) sc[e * CS + tl] = cost[t * B + e0 + e];
        }
        __syncthreads();
        // LDS -> ring: consecutive lanes walk the words of consecutive time steps of one environment
        for (int idx = tid; idx < kSlice * TT * NW; idx += kCopyThreads) {
            const int e = idx / (TT * NW), k = idx % (TT * NW), tl = k / NW, c = k % NW;
            const int64_t t = t0 + tl, j = soff[e] + t;
            if (t < sL[e] && j >= drop) {
                int64_t slot = a.head + (j - drop);
                if (slot >= cap) slot -= cap;
                if (slot >= 0 && slot < cap) bx[slot * NW + c] = sx[e * XS + k];
            }
        }
        for (int idx = tid; idx < kSlice * TT; idx += kCopyThreads) {
            const int e = idx / TT, tl = idx % TT;
            const int64_t t = t0 + tl, j = soff[e] + t;
            if (t < sL[e] && j >= drop) {
                int64_t slot = a.head + (j - drop);
                if (slot >= cap) slot -= cap;
                if (slot >= 0 && slot < cap) { bc[slot] = sc[e * CS + tl]; bd[slot] = t == sL[e] - 1 ? kOne : (CW)0; }
            }
        }
        __syncthreads();
    }
}

template <typename W, int NW, typename CW> void launch_copy(const AppendArgs& a, hipStream_t stream) {
    constexpr int TT = tile_steps(NW * (int)sizeof(W));
    const int64_t ntile = a.T / TT + 1;                              // ceil((T + 1) / TT)
    // a workgroup per (slice, tile) while that stays a small grid; big batches give each workgroup a stride of tiles instead, since most
    // of their slices leave at once and an empty workgroup still costs its dispatch
    int64_t gy = 65536 / a.nslice;
    gy = gy < 4 ? 4 : gy;
    gy = gy > ntile ? ntile : gy;
    hipLaunchKernelGGL((k_append_copy<W, NW, CW>), dim3((unsigned)a.nslice, (unsigned)gy), dim3(kCopyThreads), 0, stream, a);
}

// MAXNW: the longest record this word pair is used for (instantiates no kernel beyond it)
template <typename W, typename CW, int MAXNW> bool dispatch_copy(int nw, const AppendArgs& a, hipStream_t stream) {
    switch (nw) {
#define HJBX_APPEND_CASE(NW) case NW: if constexpr (NW <= MAXNW) { launch_copy<W, NW, CW>(a, stream); return true; } break;
    HJBX_APPEND_CASE(1) HJBX_APPEND_CASE(2) HJBX_APPEND_CASE(3) HJBX_APPEND_CASE(4) HJBX_APPEND_CASE(5)
    HJBX_APPEND_CASE(6) HJBX_APPEND_CASE(7) HJBX_APPEND_CASE(8) HJBX_APPEND_CASE(9) HJBX_APPEND_CASE(10)
#undef HJBX_APPEND_CASE
    }
    return false;
}

inline int64_t slices_of(int64_t B) { return (B + kSlice - 1) / kSlice; }

template <typename T>
int replay_append(const char* who, const T* traj, const T* cost, const int32_t* done_step, int64_t T_steps, int64_t B, int n, T* buf_x, T* buf_cost,
                  T* buf_done, int64_t capacity, int64_t head, int64_t* header, void* workspace, void* stream_) {
    if (!traj || !cost || !done_step || !buf_x || !buf_cost || !buf_done || !header || !workspace) return hjbx_set_error(HJBX_EINVAL, "%s: NULL buffer", who);
    if (n < 1 || n > HJBX_MAX_N || B < 0 || T_steps < 0 || capacity < 1) return hjbx_set_error(HJBX_EINVAL, "%s: bad n, B, T or capacity", who);
    if (head < 0 || head >= capacity) return hjbx_set_error(HJBX_EINVAL, "%s: head %lld outside a ring of %lld slots", who, (long long)head, (long long)capacity);
    const int64_t nslice = slices_of(B);
    if (nslice > 0x7fffffff || T_steps > 0x7fffffff) return hjbx_set_error(HJBX_EINVAL, "%s: B or T too large", who);
    const uintptr_t align = (uintptr_t)traj | (uintptr_t)cost | (uintptr_t)buf_x | (uintptr_t)buf_cost | (uintptr_t)buf_done;
    if (align % sizeof(T) || (uintptr_t)header % 8 || (uintptr_t)workspace % 8 || (uintptr_t)done_step % 4)
        return hjbx_set_error(HJBX_EINVAL, "%s: misaligned buffer", who);
    hipStream_t stream = (hipStream_t)stream_;
    if (B == 0) {
        // no records: the header is all there is to write, and it is written only where the runtime knows `header` as memory of its own
        // (nothing is launched on, and nothing is written through, a pointer it does not know)
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, header) == hipSuccess &&
            (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeHost)) {
            if (hipMemsetAsync(header, 0, 4 * sizeof(int64_t), stream) != hipSuccess)
                return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(hipGetLastError()));
        }
        (void)hipGetLastError();
        return HJBX_OK;
    }
    int64_t* off = (int64_t*)workspace;
    int32_t* bad = (int32_t*)(off + nslice + 1);
    hipLaunchKernelGGL(k_append_slice_sums, dim3((unsigned)((nslice + 3) / 4)), dim3(256), 0, stream, done_step, B, T_steps, nslice, off, bad);
    hipLaunchKernelGGL(k_append_scan, dim3(1), dim3(kScanThreads), 0, stream, off, bad, nslice, capacity, header);
    const AppendArgs a{traj, cost, done_step, T_steps, B, buf_x, buf_cost, buf_done, capacity, head, off, header, nslice};
    const size_t rec = (size_t)n * sizeof(T);
    const uintptr_t xalign = (uintptr_t)traj | (uintptr_t)buf_x;
    const bool by16 = rec % 16 == 0 && xalign % 16 == 0;
    bool ok;
    if constexpr (sizeof(T) == 8) {
        ok = by16 ? dispatch_copy<Word16, uint64_t, HJBX_MAX_N / 2>(n / 2, a, stream) : dispatch_copy<uint64_t, uint64_t, HJBX_MAX_N>(n, a, stream);
    } else {
        if (by16) ok = dispatch_copy<Word16, uint32_t, HJBX_MAX_N / 4>(n / 4, a, stream);
        else if (rec % 8 == 0 && xalign % 8 == 0) ok = dispatch_copy<uint64_t, uint32_t, HJBX_MAX_N / 2>(n / 2, a, stream);
        else ok = dispatch_copy<uint32_t, uint32_t, HJBX_MAX_N>(n, a, stream);
    }
    if (!ok) return hjbx_set_error(HJBX_EUNSUPPORTED, "%s: no copy kernel for n = %d", who, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}

}  // namespace

extern "C" size_t hjbx_replay_append_workspace_bytes(int64_t B) {
    const int64_t nslice = slices_of(B < 0 ? 0 : B);
    return (size_t)(((nslice + 1) * 8 + nslice * 4 + 15) / 16 * 16);
}

extern "C" int hjbx_replay_append_f32(const float* traj, const float* cost, const int32_t* done_step, int64_t T, int64_t B, int n, float* buf_x,
                                      float* buf_cost, float* buf_done, int64_t capacity, int64_t head, int64_t* header, void* workspace, void* stream) {
    return replay_append<float>("hjbx_replay_append_f32", traj, cost, done_step, T, B, n, buf_x, buf_cost, buf_done, capacity, head, header, workspace, stream);
}

extern "C" int hjbx_replay_append_f64(const double* traj, const double* cost, const int32_t* done_step, int64_t T, int64_t B, int n, double* buf_x,
                                      double* buf_cost, double* buf_done, int64_t capacity, int64_t head, int64_t* header, void* workspace, void* stream) {
    return replay_append<double>("hjbx_replay_append_f64", traj, cost, done_step, T, B, n, buf_x, buf_cost, buf_done, capacity, head, header, workspace, stream);
}
