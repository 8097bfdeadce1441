// hjbx_probe.hip -- TEST INFRASTRUCTURE: the element-wise activation functions of the matrix-core kernels, evaluated on a plain array.
//
// act1 / dact1 / sincos1 of hjbx_mlp_core.hpp are inlined into every MFMA kernel with a smooth activation, where their results can only be
// seen through three layers of products.  This entry point runs the SAME device functions (nothing is restated here) over an array of
// arguments, so that a test can sweep every binade of the float32 range against a float64 reference in one launch:
//   h[i] = act1<ACT>(a[i])
//   s[i] = the derivative factor as the kernels form it: dact1<ACT>(h[i], 1) for relu (= [h > 0]) and tanh (= 1 - h^2), which take it
//          from the activation; the cosine of sincos1(a[i]) for sin, which keeps it next to the sine.
// A grid-stride loop, one element per lane and trip: no MFMA, no LDS.
#include <hip/hip_runtime.h>

#include "hjbx_internal.hpp"
#include "hjbx_mlp_core.hpp"

using namespace hjbx;

namespace {

constexpr int kBlock = 256, kMaxBlocks = 4096;

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_activation_probe(const float* __restrict__ a, float* __restrict__ h, float* __restrict__ s, int64_t N) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) {
        const float v = a[i];
        float hv, sv;
        if constexpr (ACT == HJBX_ACT_SIN) {
            sincos1(v, hv, sv);
        } else {
            hv = act1<ACT>(v);
            sv = dact1<ACT>(hv, 1.0f);
        }
        if (h) h[i] = hv;
        if (s) s[i] = sv;
    }
}

}  // namespace

extern "C" int hjbx_activation_probe_f32(int activation, const float* a, float* h, float* s, int64_t N, void* stream_) {
    const char* who = "hjbx_activation_probe_f32";
    if (activation != HJBX_ACT_RELU && activation != HJBX_ACT_TANH && activation != HJBX_ACT_SIN)
        return hjbx_set_error(HJBX_EINVAL, "%s: unknown activation %d", who, activation);
    if (N < 0) return hjbx_set_error(HJBX_EINVAL, "%s: N = %lld", who, (long long)N);
    if (N == 0 || (!h && !s)) return HJBX_OK;
    if (!a) return hjbx_set_error(HJBX_EINVAL, "%s: NULL a", who);
    if ((uintptr_t)a % 4 || (uintptr_t)h % 4 || (uintptr_t)s % 4) return hjbx_set_error(HJBX_EINVAL, "%s: misaligned buffer", who);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t g = (N + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(g < kMaxBlocks ? g : kMaxBlocks));
    if (activation == HJBX_ACT_TANH) hipLaunchKernelGGL((k_activation_probe<HJBX_ACT_TANH>), grid, dim3(kBlock), 0, stream, a, h, s, N);
    else if (activation == HJBX_ACT_SIN) hipLaunchKernelGGL((k_activation_probe<HJBX_ACT_SIN>), grid, dim3(kBlock), 0, stream, a, h, s, N);
    else hipLaunchKernelGGL((k_activation_probe<HJBX_ACT_RELU>), grid, dim3(kBlock), 0, stream, a, h, s, N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hjbx_set_error(HJBX_EHIP, "%s: %s", who, hipGetErrorString(e));
    return HJBX_OK;
}
