// hjbx_mlp_core.hpp -- device code shared by the MFMA kernels (hjbx_mlp.hip: inference; hjbx_train.hip: value-loss gradient):
// the software-pipelined f32 MFMA chain, the LDS image of the value network's weights and the fused forward + input-gradient
// of one 32-environment tile.  See the top of hjbx_mlp.hip for the design.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"

using namespace hjbx;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

static constexpr int kH1 = 128, kH2 = 128, kH3 = 64;
static constexpr int kLD1 = 129, kLD2 = 129, kLD3 = 65;  // odd LDS row strides (floats)

// istd = 1 / normalization_std, rounded once on the host: the kernels multiply (an IEEE division is ~10 VALU instructions, 2N of
// them per tile and step otherwise)
template <int N> struct MlpP { float mean[N], istd[N], xf[N], eps_s; };

// accumulator register s of lane-half h holds row perm(s) + 4h of its 32-row block
__device__ __forceinline__ constexpr int perm(int s) { return (s & 3) + 8 * (s >> 2); }

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// relu as ONE instruction: fmaxf / fmed3f compile to a canonicalising v_max plus the v_max.  max on the raw
// bits as a signed integer is the same function (negative floats and -0.0 have the sign bit set -> 0; positive
// floats and +NaN pass through) and stays visible to the compiler's MFMA hazard padding, which an inline-asm
// v_max_f32 would not.
__device__ __forceinline__ float relu1(float v) {
    const int b = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, b > 0 ? b : 0);
}

// tanh for the notebooks' networks (hjbx_mlp.activation = HJBX_ACT_TANH), accurate in RELATIVE terms down to the smallest normal: a PD network
// has no biases, so every pre-activation goes to zero with the error state, and V = |y|^2 and its gradient are only as good as tanh is
// relative to its own size.  Two formulas, both always evaluated, chosen per element by a mask made with integer arithmetic:
//   |x| >= 0.625: 1 - 2 / (exp(2|x|) + 1) on the hardware exp2 / rcp units (each good to 1 ulp).  Here tanh >= 0.55 and the subtraction
//       from 1 amplifies the errors of the quotient by (1 - t) / t <= 0.81: relative error <= 6 x 2^-24 at the threshold, falling to the
//       final rounding as |x| grows (exp2 overflow -> exactly 1);
//   |x| <  0.625: the Cephes single-precision odd polynomial x + x z P(z), z = x^2 (approximation error 0.15 x 2^-24; the correction term
//       is at most 0.13 |x|, so its roundings hardly count): relative error <= 2 x 2^-24, and subnormal inputs come back unchanged.
// 1 - 2 / (exp(2x) + 1) alone, the earlier form, rounds exp(2x) + 1 at ulp(2): 6e-8 of ABSOLUTE error whatever x is, and exactly 0 below 3e-8.
// The exp2 formula runs on |x| and the sign of x is copied onto the result, so tanh1(-x) == -tanh1(x) bit for bit.  NaN gives NaN.
// The choice is written as a mask, the sign of an integer difference of the bit patterns (|x| < 0.625 <=> bits(|x|) < 0x3f200000; NaN and inf
// take the exp2 side); hipcc makes one integer v_cmp + v_cndmask of it, consumed at once -- unlike the three compares per element that sincos1
// avoids, it left no lane mask alive in any instantiation (zero scratch, no spilled register: the audits of tests/).  15 VALU ops, two of them
// quarter rate, three registers live at most; the one kernel that has not got them (the parameter gradient of a user system with n > 4, at
// 498 of 512 VGPRs) fences its evaluations one by one (hjbx_train_coop_kernels.hpp).  The derivative comes from the value: 1 - tanh^2.
__device__ __forceinline__ float tanh1(float v) {
    const float z = v * v;
    float p = fmaf(-5.70498872745e-3f, z, 2.06390887954e-2f);
    p = fmaf(p, z, -5.37397155531e-2f);
    p = fmaf(p, z, 1.33314422036e-1f);
    p = fmaf(p, z, -3.33332819422e-1f);
    const float small = fmaf(p * z, v, v);
    const uint32_t uv = __builtin_bit_cast(uint32_t, v), ua = uv & 0x7fffffffu;
    const float ex = __builtin_amdgcn_exp2f(__builtin_bit_cast(float, ua) * 2.8853900817779268f);  // exp(2|x|) = 2^(2|x| log2 e)
    const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(ex + 1.0f);
    const uint32_t m = (uint32_t)((int32_t)(ua - 0x3f200000u) >> 31);  // all ones below the threshold
    const uint32_t r = (__builtin_bit_cast(uint32_t, small) & m) | (__builtin_bit_cast(uint32_t, big) & ~m);
    return __builtin_bit_cast(float, (r & 0x7fffffffu) | (uv & 0x80000000u));
}
// sin / cos for the time-optimal notebook's network (hjbx_mlp.activation = HJBX_ACT_SIN), branch-free and without the stack frame of the
// library's large-argument path (the matrix-core kernels must stay free of scratch): k = rint(x 2/pi), r = x - k pi/2 by a two-constant
// Cody-Waite reduction under fma (exact for |k| < 2^12 or so: pre-activations are O(1) to O(100)), the Cephes single-precision minimax
// polynomials on [-pi/4, pi/4] (about 1 ulp), quadrant by bit operations.  Absolute error <= 1e-7 for |x| <= 1e3, sin relatively accurate
// as x -> 0.  Beyond 1e3 the two constants no longer reduce exactly: the error grows with |x| (1e-7 still at 1e5, nothing left of the
// phase from ~1e6), and once k is no integer-accurate float (|x| > ~5e7) r is not reduced at all -- so r is held to +-0.8125 (one v_med3;
// inside the domain |r| <= pi/4 + 1e-4 and nothing changes, bit for bit), which bounds both polynomials by 1: EVERY finite x gives
// |sin|, |cos| <= 1, where the bare polynomials returned 85 at 1e8 and inf from 1e13.  v_med3 drops a NaN (it answers with the minimum of
// the other two), so the NaN of a non-finite x (r = inf - inf) is put back into r^2 through r * 0: NaN and +-inf give NaN.
__device__ __forceinline__ void sincos1(float x, float& sn, float& cs) {
    const float k = rintf(x * 0.63661977236758134f);
    float r = fmaf(k, -1.5707963705062866f, x);
    r = fmaf(k, 4.371139000186243e-08f, r);
    const float rc = __builtin_amdgcn_fmed3f(r, -0.8125f, 0.8125f);
    const float r2 = fmaf(rc, rc, r * 0.0f);
    const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f) * r2, rc, rc);
    const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f), r2 * r2, fmaf(-0.5f, r2, 1.0f));
    // quadrant without compares (a compare per element becomes an SGPR lane mask; 64 elements x 3 of them spill): odd k swaps the two
    // polynomials through a bit-field insert under an all-ones / all-zeros mask, bits 1 of k and k + 1 go straight into the sign bits
    const uint32_t q = (uint32_t)(int)k;
    const uint32_t m = 0u - (q & 1u);
    const uint32_t us = __builtin_bit_cast(uint32_t, ps), uc = __builtin_bit_cast(uint32_t, pc);
    const uint32_t a = (uc & m) | (us & ~m), b = (us & m) | (uc & ~m);
    sn = __builtin_bit_cast(float, a ^ ((q & 2u) << 30));
    cs = __builtin_bit_cast(float, b ^ (((q + 1u) & 2u) << 30));
}
__device__ __forceinline__ float sin1(float x) { float s, c; sincos1(x, s, c); return s; }
__device__ __forceinline__ float cos1(float x) { float s, c; sincos1(x, s, c); return c; }

// ACT = hjbx_activation: the activation applied in place to a pre-activation, and the back-propagation factor d * act'(z)
// written in terms of the ACTIVATION h = act(z) (relu: [h > 0]; tanh: 1 - h^2), so no pre-activation has to be kept.
// sin (examples/double_integrator_optimal_time.ipynb cell 5): act' = cos(z) cannot be had from sin(z) (the sign is lost), so the kernels
// keep cos(z) where relu / tanh keep the activation: `h` of dact1 is then that cosine (sincos1 above).
template <int ACT> __device__ __forceinline__ float act1(float v) {
    if constexpr (ACT == HJBX_ACT_TANH) return tanh1(v);
    else if constexpr (ACT == HJBX_ACT_SIN) return sin1(v);
    else return relu1(v);
}
template <int ACT> __device__ __forceinline__ float dact1(float h, float d) {
    if constexpr (ACT == HJBX_ACT_TANH) return d - d * h * h;
    else if constexpr (ACT == HJBX_ACT_SIN) return d * h;          // h = cos(z)
    // relu: d * [h > 0] as two multiplies, the first with the clamp output modifier (v_mul_f32 ... clamp gives exactly 1 for
    // every normal h > 0, and 0 for h <= 0 or NaN).  Same op count as v_cmp + v_cndmask, but no VCC in between: that pair
    // costs an s_nop per element (VALU write of VCC -> VALU read), 192 of them per tile and step.
    else return d * fminf(fmaxf(h * 3.0e38f, 0.f), 1.f);
}

// ---- software-pipelined MFMA chain ------------------------------------------------------------------------
// One GEMM of the chain: acc[t][o] += A_o(step) x b_t(step), step = 0..NSTEPS-1, o = 0..NOUT-1 output blocks,
// t = 0..TL-1 environment tiles; every A operand is one LDS dword per lane.  hipcc sinks compiler-visible
// ds_reads down to their MFMAs and re-uses two operand registers (read -> lgkmcnt(0) -> 2 MFMAs), whatever the
// source order or sched_barrier placement.  So the reads are issued from inline asm DEPTH steps ahead and
// retired with counted s_waitcnt lgkmcnt(N) statements fenced by sched_barrier (guide 5.7, form iii; the ISA is
// audited by tools/audit_asm_loads.py): LDS returns in order, so "at most N newer operations outstanding" means this step's operands have
// landed.  Any LDS / SMEM operation the compiler adds in between only makes the count conservative.
// A chain waits for its first DEPTH steps' operands before its first MFMA (seven prologues per tile and step in mlp_value_grad).  Issuing
// those reads in front of the VALU pass that precedes the chain, and running backward 2 and the layer-1 recomputation through one operand
// pipeline, were both built and measured (cartpole, B = 2^20): no difference beyond run-to-run spread, alone or together, so the chain
// keeps its prologue (profiles/rollout_boundaries.json).
template <int BYTE_OFF> __device__ __forceinline__ float lds_read_b32(uint32_t addr) {
    static_assert(BYTE_OFF >= 0 && BYTE_OFF < 65536, "ds_read_b32 offset field is 16 bits");
    float v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(BYTE_OFF));
    return v;
}
// Counted wait + scheduling fence (guide 5.7, form iii).  The wait is the compiler-visible builtin rather than an asm
// statement: hipcc pads an s_nop between ANY inline-asm statement and a following MFMA (it must assume the statement
// wrote the MFMA's operands with a VALU op), which would cost one more issue slot per MFMA group.
// s_waitcnt simm16 on gfx9: vmcnt = bits 3:0 + 15:14, expcnt = 6:4, lgkmcnt = 11:8 -> 0xC07F leaves vmcnt/expcnt unwaited.
template <int CNT> __device__ __forceinline__ void lds_wait() {
    static_assert(CNT >= 0 && CNT <= 15, "");
    __builtin_amdgcn_s_waitcnt(0xC07F | (CNT << 8));
    __builtin_amdgcn_sched_barrier(0);
}

template <typename Off, int ST, int NOUT, int O = 0> __device__ __forceinline__ void chain_issue(float (&slot)[NOUT], uint32_t base) {
    if constexpr (O < NOUT) {
        slot[O] = lds_read_b32<Off::at(ST, O)>(base);
        chain_issue<Off, ST, NOUT, O + 1>(slot, base);
    }
}

template <typename Off, int NSTEPS, int NOUT, int DEPTH, int TL, int ST, typename GetB>
__device__ __forceinline__ void mfma_chain_step(f32x16 (&acc)[TL][NOUT], float (&ring)[DEPTH + 1][NOUT], float (&b)[2][TL], uint32_t base,
                                                GetB getB) {
    if constexpr (ST < NSTEPS) {
        // order inside a step: asm reads for step ST+DEPTH | B operands of step ST+1 (VALU) | counted wait | MFMAs of
        // step ST.  Two compiler-visible instructions sit between the last asm statement and the first MFMA, and the
        // MFMAs' B operands were written a whole step earlier, so hipcc needs no s_nop pad in front of the group.
        if constexpr (ST + DEPTH < NSTEPS) chain_issue<Off, ST + DEPTH, NOUT>(ring[(ST + DEPTH) % (DEPTH + 1)], base);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ST + 1 < NSTEPS) {
#pragma unroll
            for (int t = 0; t < TL; ++t) b[(ST + 1) & 1][t] = getB(ST + 1, t);
        }
        constexpr int ahead = (NSTEPS - 1 - ST < DEPTH ? NSTEPS - 1 - ST : DEPTH) * NOUT;  // reads issued after this step's
        float(&cur)[NOUT] = ring[ST % (DEPTH + 1)];
        lds_wait<ahead>();
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int t = 0; t < TL; ++t) acc[t][o] = MFMA(cur[o], b[ST & 1][t], acc[t][o]);
        __builtin_amdgcn_sched_barrier(0);  // keep this step's MFMAs in front of the next step's reads and wait
        mfma_chain_step<Off, NSTEPS, NOUT, DEPTH, TL, ST + 1>(acc, ring, b, base, getB);
    }
}

template <typename Off, int NSTEPS, int NOUT, int DEPTH, int TL, typename GetB>
__device__ __forceinline__ void mfma_chain(f32x16 (&acc)[TL][NOUT], float (&ring)[DEPTH + 1][NOUT], uint32_t base, GetB getB) {
    static_assert(NOUT == 1 || NOUT == 2 || NOUT == 4, "");
    static_assert(NOUT * DEPTH <= 15, "lgkmcnt is a 4-bit field");
    static_assert(DEPTH <= 3 && NSTEPS >= 1, "");
    // prologue: the first DEPTH steps' operands and the first step's B operands
    if constexpr (0 < DEPTH && 0 < NSTEPS) chain_issue<Off, 0, NOUT>(ring[0], base);
    if constexpr (1 < DEPTH && 1 < NSTEPS) chain_issue<Off, 1, NOUT>(ring[1], base);
    if constexpr (2 < DEPTH && 2 < NSTEPS) chain_issue<Off, 2, NOUT>(ring[2], base);
    float b[2][TL];
#pragma unroll
    for (int t = 0; t < TL; ++t) b[0][t] = getB(0, t);
    mfma_chain_step<Off, NSTEPS, NOUT, DEPTH, TL, 0>(acc, ring, b, base, getB);
}

// hipcc's hazard recogniser does not look inside inline asm: an asm VALU statement (relu_mask, mask_apply, v_fma_mix) that READS an
// accumulator while the MFMA that writes it is still in flight gets no wait states and sees stale registers -- and such statements are
// pure, so the scheduler may place them directly behind the last MFMA of a chain (seen on one instantiation only, the
// planar quadrotor's f16x2 kernel: its last 32 layer-1 units were masked with half-written values).  Every chain whose results are
// consumed by asm statements is therefore followed by this barrier: enough idle issue
// slots for the last MFMA to retire (8-pass MFMA: 11 wait states, 16-pass: 19), fenced so that nothing moves across it.
template <int PASSES> __device__ __forceinline__ void mfma_results_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PASSES > 8) asm volatile("s_nop 15\n\ts_nop 7");
    else asm volatile("s_nop 15");
    __builtin_amdgcn_sched_barrier(0);
}

// byte offsets (from the lane-dependent base) of the A operand of (step, output block) for each product
struct OffW1F { static constexpr int at(int st, int fb) { return (2 * st * kLD1 + 32 * fb) * 4; } };
struct OffW2F { static constexpr int at(int st, int fb) { return ((32 * (st >> 4) + perm(st & 15)) * kLD2 + 32 * fb) * 4; } };
struct OffW3F { static constexpr int at(int st, int ob) { return ((32 * (st >> 4) + perm(st & 15)) * kLD3 + 32 * ob) * 4; } };
struct OffW3B { static constexpr int at(int st, int fb) { return (32 * fb * kLD3 + 32 * (st >> 4) + perm(st & 15)) * 4; } };
struct OffW2B { static constexpr int at(int st, int fb) { return (32 * fb * kLD2 + 32 * (st >> 4) + perm(st & 15)) * 4; } };

template <int N> struct MlpLds {
    static constexpr int NP = (N + 3) & ~3;  // W1' rows padded to whole float4s
    float W1T[kH1 * NP];                     // W1 transposed [feature][k] (16-byte aligned: first member)
    float W1[N * kLD1];
    float W2[kH1 * kLD2];
    float W3[kH2 * kLD3];
    int next;                                // next unclaimed tile group of this workgroup's range
};

// Soft-PD head (examples/cartpole_balancing.ipynb cell 6, SoftPDValueApproximator): the biases of the three hidden layers and the
// scalar output layer, staged in LDS next to the weights (385 floats).  Hidden feature f of a lane half h sits at accumulator register
// s with f = 32 o + perm(s) + 4h: registers 4q .. 4q + 3 of block o are the four consecutive features 32 o + 8q + 4h + 0..3, one float4.
struct MlpBias {
    float b1[kH1], b2[kH2], b3[kH3], w4[kH3];
    float b4;
};
template <int N> struct MlpLdsSoft : MlpLds<N> {
    alignas(16) MlpBias bias;
};

template <int TL, int NOUT> __device__ __forceinline__ void zero_acc(f32x16 (&a)[TL][NOUT]) {
#pragma unroll
    for (int t = 0; t < TL; ++t)
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int r = 0; r < 16; ++r) a[t][o][r] = 0.f;
}

// accumulators initialised with a bias vector instead of zeros (soft-PD head): the chain then adds the products to it
template <int TL, int NOUT> __device__ __forceinline__ void bias_acc(f32x16 (&a)[TL][NOUT], const float* b, int h) {
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(b + 32 * o + 8 * q + 4 * h);
#pragma unroll
            for (int t = 0; t < TL; ++t) {
                a[t][o][4 * q] = v.x; a[t][o][4 * q + 1] = v.y; a[t][o][4 * q + 2] = v.z; a[t][o][4 * q + 3] = v.w;
            }
        }
}

// lane-dependent LDS operand bases of one wave; everything else is a compile-time offset
struct MlpCtx {
    uint32_t w1f, w2f, w3f, w3b, w2b;
    const float4* w1t;
    int i, h;  // i = lane & 31: A-operand row / environment column; h = lane >> 5: k parity / accumulator row-half
};

template <int N, int THREADS>
__device__ __forceinline__ void mlp_fill_lds(MlpLds<N>& L, const float* __restrict__ W1g, const float* __restrict__ W2g,
                                             const float* __restrict__ W3g, int tid) {
    constexpr int NP = MlpLds<N>::NP;
    for (int idx = tid; idx < N * kH1; idx += THREADS) L.W1[(idx / kH1) * kLD1 + (idx % kH1)] = W1g[idx];
    for (int idx = tid; idx < kH1 * NP; idx += THREADS) {
        const int f = idx / NP, k = idx % NP;
        L.W1T[idx] = k < N ? W1g[k * kH1 + f] : 0.f;
    }
    for (int idx = tid; idx < kH1 * kH2; idx += THREADS) L.W2[(idx / kH2) * kLD2 + (idx % kH2)] = W2g[idx];
    for (int idx = tid; idx < kH2 * kH3; idx += THREADS) L.W3[(idx / kH3) * kLD3 + (idx % kH3)] = W3g[idx];
}

template <int THREADS>
__device__ __forceinline__ void mlp_fill_bias(MlpBias& L, const float* __restrict__ b1g, const float* __restrict__ b2g, const float* __restrict__ b3g,
                                              const float* __restrict__ w4g, const float* __restrict__ b4g, int tid) {
    for (int idx = tid; idx < kH1; idx += THREADS) L.b1[idx] = b1g[idx];
    for (int idx = tid; idx < kH2; idx += THREADS) L.b2[idx] = b2g[idx];
    for (int idx = tid; idx < kH3; idx += THREADS) { L.b3[idx] = b3g[idx]; L.w4[idx] = w4g[idx]; }
    if (tid == 0) L.b4 = b4g[0];
}

template <int N> __device__ __forceinline__ MlpCtx mlp_ctx(MlpLds<N>& L, int lane) {
    constexpr int NP = MlpLds<N>::NP;
    MlpCtx c;
    c.i = lane & 31;
    c.h = lane >> 5;
    // (the low 32 bits of a flat pointer into the LDS aperture are the LDS byte address)
    const uint32_t lds0 = (uint32_t)(uintptr_t)&L;
    c.w1f = lds0 + (uint32_t)offsetof(MlpLds<N>, W1) + 4u * (c.h * kLD1 + c.i);      // forward:  W1[2s + h][32 fb + i]
    c.w2f = lds0 + (uint32_t)offsetof(MlpLds<N>, W2) + 4u * (4 * c.h * kLD2 + c.i);  //           W2[32 kb + perm(s) + 4h][32 fb + i]
    c.w3f = lds0 + (uint32_t)offsetof(MlpLds<N>, W3) + 4u * (4 * c.h * kLD3 + c.i);  //           W3[32 kb + perm(s) + 4h][32 ob + i]
    c.w3b = lds0 + (uint32_t)offsetof(MlpLds<N>, W3) + 4u * (c.i * kLD3 + 4 * c.h);  // backward: W3[32 fb + i][32 kb + perm(s) + 4h]
    c.w2b = lds0 + (uint32_t)offsetof(MlpLds<N>, W2) + 4u * (c.i * kLD2 + 4 * c.h);  //           W2[32 fb + i][32 kb + perm(s) + 4h]
    c.w1t = reinterpret_cast<const float4*>(L.W1T + 4 * c.h * NP);                   // W1'[32 kb + perm(s) + 4h][0..NP)
    return c;
}

// ---- shared by the two split-operand arithmetics (hjbx_mlp_x3.hpp: bf16x3, hjbx_mlp_h2.hpp: f16x2) -------------------------------------
// Their swizzled 16-bit weight images (layout: top of hjbx_mlp_x3.hpp), the two kinds of LDS read on them, and the ReLU masks.
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

static constexpr int kImgRow = 256;               // bytes per image row: 128 input features x 2 B
static constexpr int kImgPiece = 64 * kImgRow;    // one piece of 64 rows
__host__ __device__ constexpr int img_sw(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

template <int BYTE_OFF> __device__ __forceinline__ u32x2 lds_read_b64(uint32_t addr) {
    static_assert(BYTE_OFF >= 0 && BYTE_OFF < 65536 && BYTE_OFF % 8 == 0, "");
    u32x2 v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(BYTE_OFF));
    return v;
}
// EXEC must be all ones (the gather crosses lanes): the chains run with every lane active, padding lanes included
template <int BYTE_OFF> __device__ __forceinline__ u32x2 lds_read_tr16_b64(uint32_t addr) {
    static_assert(BYTE_OFF >= 0 && BYTE_OFF < 65536 && BYTE_OFF % 8 == 0, "");
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(BYTE_OFF));
    return v;
}

// ReLU derivatives as bit masks (128 bits per lane and layer: bit 16 (fb & 1) + r of m[fb >> 1] belongs to register r of block fb)
// v = relu(v) and bit BIT of m = [v > 0]
template <int BIT> __device__ __forceinline__ void relu_mask(float& v, uint32_t& m) {
    v = relu1(v);
    uint32_t t;
    asm("v_min_u32_e32 %0, 1, %2\n\tv_lshl_or_b32 %1, %0, %3, %1" : "=&v"(t), "+v"(m) : "v"(v), "n"(BIT));
}
// x * [bit BIT of m]
template <int BIT> __device__ __forceinline__ float mask_apply(float x, uint32_t m) {
    float y;
    asm("v_bfe_i32 %0, %1, %2, 1\n\tv_and_b32_e32 %0, %0, %3" : "=&v"(y) : "v"(m), "n"(BIT), "v"(x));
    return y;
}

// What happens to the chain's input registers on their way into the B fragments (PRE): the element-wise work between two products runs
// inside the consuming chain, two elements per unit next to their split, instead of in a VALU-only pass in front of it (where this
// wave issues no MFMA for ~500 instructions and relies on its SIMD partner being inside a chain at that moment).
enum { kPreNone = 0, kPreReluMask = 1, kPreMaskApply = 2 };  // relu + record [v > 0] in the mask | multiply by the recorded mask bit

template <int FB, int R> __device__ __forceinline__ void mask_apply_block(f32x16 (&a)[4], const uint32_t (&m)[2]) {
    if constexpr (FB < 4) {
        const float v = a[FB][R];
        a[FB][R] = mask_apply<16 * (FB & 1) + R>(v, m[FB >> 1]);
        if constexpr (R + 1 < 16) mask_apply_block<FB, R + 1>(a, m);
        else mask_apply_block<FB + 1, 0>(a, m);
    }
}

// ---- backward 1 (the VALU product at the end of mlp_value_grad) in groups of features ------------------------------------------------------
// Left to hipcc, every W1' row is read -> s_waitcnt lgkmcnt(0 / 1) -> used by its two v_pk_fma_f32: one LDS latency per feature pair in the open,
// 32 per tile and step, with nothing of this wave's to put under it.  Here the rows of a whole group of G features are fetched by asm
// ds_read_b128 (one per float4 of a row) while the previous group's FMAs run, and retired by one counted wait per group (lds_wait, as in the
// chains; audited by tools/audit_asm_loads.py like them).  Two buffers of G rows: 16 registers each for n <= 8, 24 for n = 10 -- the cartpole
// rollout kernel stays at its 242 VGPRs, and nothing spills anywhere (tests/test_rollout_boundaries_host.py).  Feature f is register f & 15 of
// accumulator block f >> 4 and the groups walk f = 0..63 as the plain loop did: every sum is the same fmaf chain, bit for bit.
// Cartpole B = 2^20: 0.7387 -> 0.7327 ms per step; groups of 8 (255 VGPRs) or 2 measure the same (profiles/rollout_boundaries.json).
// The units compiled at run time for user-defined systems (hjbx_user_mlp_kernels.hpp) keep the plain loop: the run-time compiler's
// build of the same templates put 0.9 KB per lane into scratch with the groups (n = 4; hipcc -S of the same unit: none), and a kernel with
// scratch is refused there.
#ifdef HJBX_USER_MATRIX_CORE_UNIT
static constexpr bool kW1tGroups = false;
#else
static constexpr bool kW1tGroups = true;
#endif
using f32x4 = __attribute__((ext_vector_type(4))) float;
template <int BYTE_OFF> __device__ __forceinline__ f32x4 lds_read_b128(uint32_t addr) {
    static_assert(BYTE_OFF >= 0 && BYTE_OFF < 65536 && BYTE_OFF % 16 == 0, "");
    f32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(BYTE_OFF));
    return v;
}
template <int NP> struct W1tGroup {
    static constexpr int Q = NP / 4;             // float4s per row of W1'
    static constexpr int G = NP <= 4 ? 4 : 2;    // features per group
    static constexpr int READS = G * Q;          // ds_read_b128 per group = entries of the counted wait
    static_assert(64 % G == 0 && READS <= 15, "lgkmcnt is a 4-bit field");
};
// rows of the features F0 .. F0 + G - 1 into buf; base = LDS byte address of W1'[4h][0] (MlpCtx::w1t)
template <int NP, int F0, int J = 0> __device__ __forceinline__ void w1t_issue(f32x4 (&buf)[W1tGroup<NP>::READS], uint32_t base) {
    constexpr int Q = W1tGroup<NP>::Q;
    if constexpr (J < W1tGroup<NP>::READS) {
        constexpr int f = F0 + J / Q, q = J % Q;
        buf[J] = lds_read_b128<((32 * (f >> 4) + perm(f & 15)) * Q + q) * 16>(base);
        w1t_issue<NP, F0, J + 1>(buf, base);
    }
}
template <int NP, int J = 0> __device__ __forceinline__ void w1t_landed(const f32x4 (&buf)[W1tGroup<NP>::READS]) {
    if constexpr (J < W1tGroup<NP>::READS) {
        asm volatile("" : : "v"(buf[J]));
        w1t_landed<NP, J + 1>(buf);
    }
}
// group GI and the ones behind it: part[k] += W1'[f][2k, 2k + 1] . d1[f] act'(a1[f]).  Order inside a group: asm reads of group GI + 1 |
// this group's back-propagation factors (they need no weights and run under the reads) | counted wait | this group's FMAs.
template <int ACT, int NP, int GI = 0>
__device__ __forceinline__ void w1t_backward(const f32x16 (&a1)[4], const f32x16 (&d1)[4], f32x2 (&part)[NP / 2], f32x4 (&wbuf)[2][W1tGroup<NP>::READS],
                                             uint32_t base) {
    constexpr int G = W1tGroup<NP>::G, Q = W1tGroup<NP>::Q, NG = 64 / G;
    if constexpr (GI < NG) {
        if constexpr (GI + 1 < NG) w1t_issue<NP, (GI + 1) * G>(wbuf[(GI + 1) & 1], base);
        __builtin_amdgcn_sched_barrier(0);
        float dv[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int kb = (GI * G + j) >> 4, s = (GI * G + j) & 15;
            dv[j] = dact1<ACT>(ACT == HJBX_ACT_RELU ? a1[kb][s] : ACT == HJBX_ACT_SIN ? cos1(a1[kb][s]) : act1<ACT>(a1[kb][s]), d1[kb][s]);
            if constexpr (ACT == HJBX_ACT_SIN) {   // (fenced one by one: see layer 2 of mlp_value_grad)
                asm volatile("" : "+v"(dv[j]));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        lds_wait<(GI + 1 < NG) ? W1tGroup<NP>::READS : 0>();
        // A row is padded to whole float4s (n = 2, 6, 10: two columns of the last one feed nothing).  The compiler tracks liveness per
        // register, so it handed the unused half of such a destination to other values while the read, which writes all four, was in
        // flight.  One use of the WHOLE vector behind the wait keeps all of it allocated until it has landed (no instruction).
        w1t_landed<NP>(wbuf[GI & 1]);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const f32x2 dv2{dv[j], dv[j]};
#pragma unroll
            for (int q = 0; q < Q; ++q) {   // packed pairs: one v_pk_fma_f32 per two rows of W1
                const f32x4 w = wbuf[GI & 1][j * Q + q];
                part[2 * q + 0] = __builtin_elementwise_fma(f32x2{w[0], w[1]}, dv2, part[2 * q + 0]);
                part[2 * q + 1] = __builtin_elementwise_fma(f32x2{w[2], w[3]}, dv2, part[2 * q + 1]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        w1t_backward<ACT, NP, GI + 1>(a1, d1, part, wbuf, base);
    }
}

// V and dV/dx of the TL tiles whose state rows are in xs (one environment per lane, identical in both lane
// halves).  On return every lane holds its environment's V and (if want_grad) gradient.
// SOFT selects the head: false (PD, controller/vhjb.py) V = |y|^2 + eps_s |e|^2, dV/dy = 2y;  true (soft-PD, `bias` = the LDS copy of
// MlpBias) every layer adds its bias, layer 3 is activated too and V = h3 . w4 + b4, so backward 3 starts from w4 . act'(a3) and there is
// no eps_s term.  The chains are the same in both.
template <typename S, int TL, int ACT = HJBX_ACT_RELU, bool SOFT = false>
__device__ __forceinline__ void mlp_value_grad(const S& sys, const MlpP<S::N>& p, const MlpCtx& c, const float (&xs)[TL][S::N],
                                               bool want_grad, float (&V)[TL], float (&g)[TL][S::N], const MlpBias* bias = nullptr) {
    constexpr int N = S::N;
    constexpr int NP = MlpLds<N>::NP;
    const int h = c.h;
    float e[TL][N], z[TL][N], ee[TL];
#pragma unroll
    for (int t = 0; t < TL; ++t) {
        ee[t] = 0.f;
#pragma unroll
        for (int k = 0; k < N; ++k) e[t][k] = xs[t][k] - p.xf[k];
        sys.wrap(e[t]);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            ee[t] += e[t][k] * e[t][k];
            z[t][k] = (e[t][k] - p.mean[k]) * p.istd[k];
        }
    }
    float ring4[3][4], ring2[3][2];  // operand rings of the chains (DEPTH = 2)

    // ---- layer 1: H1' (128 x 32) = W1' (128 x N) . Z' (N x 32) --------------------------------------
    f32x16 a1[TL][4];
    if constexpr (SOFT) bias_acc(a1, bias->b1, h);
    else zero_acc(a1);
    mfma_chain<OffW1F, N / 2, 4, 2, TL>(a1, ring4, c.w1f, [&](int st, int t) { return h ? z[t][2 * st + 1] : z[t][2 * st]; });

    // Element-wise work between the products (ReLU, mask, 2y, |y|^2) is done in place on the accumulators in short
    // VALU-only passes BEFORE each chain: those overlap the SIMD partner's MFMAs, whereas every instruction issued
    // inside a chain delays this wave's next MFMA (~4 cycles each, tools/ubench/mfma_mix.hip).  Inside a chain a step
    // is then 4 ds_read_b32 + 1 counted wait + 4 MFMAs.

    // ---- layer 2: H2' (128 x 32) = W2' . relu(H1') ---------------------------------------------------
#pragma unroll
    for (int t = 0; t < TL; ++t)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                a1[t][fb][r] = act1<ACT>(a1[t][fb][r]);
                // sin: 64 independent polynomial evaluations -- left alone the scheduler interleaves them all and their temporaries spill
                if constexpr (ACT == HJBX_ACT_SIN) {
                    asm volatile("" : "+v"(a1[t][fb][r]));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
    f32x16 a2[TL][4];
    if constexpr (SOFT) bias_acc(a2, bias->b2, h);
    else zero_acc(a2);
    mfma_chain<OffW2F, 64, 4, 2, TL>(a2, ring4, c.w2f, [&](int st, int t) { return a1[t][st >> 4][st & 15]; });

    // ---- layer 3: Y' (64 x 32) = W3' . relu(H2') ------------------------------------------------------
    f32x16 c2[ACT == HJBX_ACT_SIN ? TL : 1][ACT == HJBX_ACT_SIN ? 4 : 1];   // sin only: cos of layer 2's pre-activations
#pragma unroll
    for (int t = 0; t < TL; ++t)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (ACT == HJBX_ACT_SIN) {   // sin for layer 3; cos kept for backward 2 (a1 is dead here: layer 1 is recomputed for backward 1)
                    float sn, cs;
                    sincos1(a2[t][fb][r], sn, cs);
                    asm volatile("" : "+v"(sn), "+v"(cs));   // evaluated HERE: pure code is otherwise sunk to its uses (chain 3, backward 2) with the pre-activations kept alive
                    a2[t][fb][r] = sn;
                    c2[t][fb][r] = cs;
                    __builtin_amdgcn_sched_barrier(0);   // (see layer 2)
                } else {
                    a2[t][fb][r] = act1<ACT>(a2[t][fb][r]);  // the activation also carries act' for backward 2 (dact1)
                }
            }
    f32x16 y[TL][2];
    if constexpr (SOFT) bias_acc(y, bias->b3, h);
    else zero_acc(y);
    mfma_chain<OffW3F, 64, 2, 2, TL>(y, ring2, c.w3f, [&](int st, int t) { return a2[t][st >> 4][st & 15]; });

    float vpart[TL];
    if constexpr (SOFT) {
        // h3 = act(a3); V = h3 . w4 + b4; the accumulators become dV/da3 = w4 . act'(a3), the start of backward 3
#pragma unroll
        for (int t = 0; t < TL; ++t) {
            f32x2 acc2{0.f, 0.f};
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 w = *reinterpret_cast<const float4*>(bias->w4 + 32 * ob + 8 * q + 4 * h);
                    const float wv[4] = {w.x, w.y, w.z, w.w};
                    float hv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float a = y[t][ob][4 * q + j];
                        if constexpr (ACT == HJBX_ACT_SIN) {   // act' = cos(a3) cannot be had from sin(a3): both now (see layer 3)
                            float sn, cs;
                            sincos1(a, sn, cs);
                            asm volatile("" : "+v"(sn), "+v"(cs));
                            hv[j] = sn;
                            y[t][ob][4 * q + j] = cs * wv[j];
                            __builtin_amdgcn_sched_barrier(0);
                        } else {
                            hv[j] = act1<ACT>(a);
                            y[t][ob][4 * q + j] = dact1<ACT>(hv[j], wv[j]);
                        }
                    }
                    acc2 = __builtin_elementwise_fma(f32x2{hv[0], hv[1]}, f32x2{wv[0], wv[1]}, acc2);
                    acc2 = __builtin_elementwise_fma(f32x2{hv[2], hv[3]}, f32x2{wv[2], wv[3]}, acc2);
                }
            vpart[t] = acc2[0] + acc2[1];
            V[t] = vpart[t] + __shfl_xor(vpart[t], 32, 64) + bias->b4;
        }
    } else {
#pragma unroll
    for (int t = 0; t < TL; ++t) {
        f32x2 acc2{0.f, 0.f};  // packed: one v_pk_fma_f32 and one v_pk_add_f32 per two outputs
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 yy{y[t][ob][r], y[t][ob][r + 1]};
                acc2 = __builtin_elementwise_fma(yy, yy, acc2);
                const f32x2 y2 = yy + yy;  // dV/dy
                y[t][ob][r] = y2[0];
                y[t][ob][r + 1] = y2[1];
            }
        vpart[t] = acc2[0] + acc2[1];
        V[t] = vpart[t] + __shfl_xor(vpart[t], 32, 64) + p.eps_s * ee[t];
    }
    }
    if (!want_grad) return;

    // ---- backward 3: dH2' (128 x 32) = W3 (128 x 64) . (2 Y') -------------------------------------------
    f32x16 d2[TL][4];
    zero_acc(d2);
    mfma_chain<OffW3B, 32, 4, 2, TL>(d2, ring4, c.w3b, [&](int st, int t) { return y[t][st >> 4][st & 15]; });

    // ---- backward 2: dH1' (128 x 32) = W2 . (dH2' . [h2 > 0]) -------------------------------------------
#pragma unroll
    for (int t = 0; t < TL; ++t)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) d2[t][fb][r] = dact1<ACT>(ACT == HJBX_ACT_SIN ? c2[ACT == HJBX_ACT_SIN ? t : 0][ACT == HJBX_ACT_SIN ? fb : 0][r] : a2[t][fb][r], d2[t][fb][r]);
    f32x16 d1[TL][4];
    zero_acc(d1);
    mfma_chain<OffW2B, 64, 4, 2, TL>(d1, ring4, c.w2b, [&](int st, int t) { return d2[t][st >> 4][st & 15]; });

    // ---- backward 1: dZ' (N x 32) = W1 (N x 128) . (dH1' . [h1 > 0]) on the VALU ---------------------------
    // Only N of an MFMA tile's 32 rows would be useful here (7.6 % of all MFMA time for n = 4); instead each
    // lane dots its 64 resident features with W1' rows (wave-uniform float4 LDS broadcasts) and the two lane
    // halves are added with one cross-half shuffle per row.  [h1 > 0] is re-derived by recomputing layer 1
    // (N/2 x 4 MFMAs, 1 % of the tile): cheaper in issue slots than carrying 128 mask bits per lane.
    // The W1' rows come in groups through w1t_backward; the first group's reads go out in front of the recomputation chain (older than the
    // chain's own reads, so its counted waits retire them first) and land under its MFMAs.
    if constexpr (SOFT) bias_acc(a1, bias->b1, h);
    else zero_acc(a1);
    const uint32_t w1t = (uint32_t)(uintptr_t)c.w1t;   // (LDS byte address, as in mlp_ctx)
    f32x4 wbuf[2][W1tGroup<NP>::READS];
    if constexpr (kW1tGroups) w1t_issue<NP, 0>(wbuf[0], w1t);
    mfma_chain<OffW1F, N / 2, 4, 2, TL>(a1, ring4, c.w1f, [&](int st, int t) { return h ? z[t][2 * st + 1] : z[t][2 * st]; });
#pragma unroll
    for (int t = 0; t < TL; ++t) {
        f32x2 part[NP / 2];
#pragma unroll
        for (int k = 0; k < NP / 2; ++k) part[k] = f32x2{0.f, 0.f};
        if constexpr (kW1tGroups) {
            if (t > 0) w1t_issue<NP, 0>(wbuf[0], w1t);
            w1t_backward<ACT, NP>(a1[t], d1[t], part, wbuf, w1t);
        } else {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    float dv = dact1<ACT>(ACT == HJBX_ACT_RELU ? a1[t][kb][s] : ACT == HJBX_ACT_SIN ? cos1(a1[t][kb][s]) : act1<ACT>(a1[t][kb][s]), d1[t][kb][s]);
                    if constexpr (ACT == HJBX_ACT_SIN) {
                        asm volatile("" : "+v"(dv));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const f32x2 dv2{dv, dv};
#pragma unroll
                    for (int q = 0; q < NP / 4; ++q) {
                        const float4 w = c.w1t[(32 * kb + perm(s)) * (NP / 4) + q];
                        part[2 * q + 0] = __builtin_elementwise_fma(f32x2{w.x, w.y}, dv2, part[2 * q + 0]);
                        part[2 * q + 1] = __builtin_elementwise_fma(f32x2{w.z, w.w}, dv2, part[2 * q + 1]);
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float pk = part[k >> 1][k & 1];
            const float v = pk + __shfl_xor(pk, 32, 64);
            if constexpr (SOFT) g[t][k] = v * p.istd[k];
            else g[t][k] = v * p.istd[k] + 2.f * p.eps_s * e[t][k];
        }
    }
}

template <int N> __device__ __forceinline__ void load_row(const float* __restrict__ x, int64_t env, float (&dst)[N]) {
    if constexpr ((N * 4) % 16 == 0) {
        const float4* rp = reinterpret_cast<const float4*>(x + env * N);
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const float4 v = rp[q];
            dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
        }
    } else {
        const float2* rp2 = reinterpret_cast<const float2*>(x + env * N);
#pragma unroll
        for (int q = 0; q < N / 2; ++q) {
            const float2 v = rp2[q];
            dst[2 * q] = v.x; dst[2 * q + 1] = v.y;
        }
    }
}

template <int N> __device__ __forceinline__ void store_row(float* __restrict__ out, int64_t env, const float (&src)[N]) {
    if constexpr ((N * 4) % 16 == 0) {
        float4* op = reinterpret_cast<float4*>(out + env * N);
#pragma unroll
        for (int q = 0; q < N / 4; ++q) op[q] = make_float4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
    } else if constexpr ((N * 4) % 8 == 0) {
        float2* op = reinterpret_cast<float2*>(out + env * N);
#pragma unroll
        for (int q = 0; q < N / 2; ++q) op[q] = make_float2(src[2 * q], src[2 * q + 1]);
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q) out[env * N + q] = src[q];
    }
}

// One sample of a tile for its lane: the state row, or the target state xf for a padding lane (`ok` false: a tile group beyond the range or an
// environment beyond B; such a lane computes like any other and emits nothing) ...
template <int N> __device__ __forceinline__ void load_sample(const float* x, const MlpP<N>& p, int64_t env, bool ok, float (&xv)[N]) {
    if (ok) load_row<N>(x, env, xv);
    else {
#pragma unroll
        for (int k = 0; k < N; ++k) xv[k] = p.xf[k];
    }
}
// ... and, for the parameter-gradient kernels, its done flag (padding: 0) and cost (padding: 1)
template <int N>
__device__ __forceinline__ void load_sample(const float* x, const float* cost, const float* done, const MlpP<N>& p, int64_t env, bool ok, float (&xv)[N],
                                            float& dn, float& cst) {
    load_sample<N>(x, p, env, ok, xv);
    dn = ok ? done[env] : 0.f;
    cst = ok ? cost[env] : 1.f;
}

// ---- partial sums of 32x32 MFMA accumulator blocks (the parameter-gradient kernels and their epilogues) ----------------------------------
// A workgroup's record is the raw accumulator layout [block][register][lane]; the epilogue kernels take one thread per element and invert it
// (row = perm(register) + 4 (lane >> 5), column = lane & 31 of the block).
__device__ __forceinline__ void put_acc_block(float* out, int blk, int lane, const f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[blk * 1024 + r * 64 + lane] = a[r];
}

// ---- the arithmetic of the 128 / 64-wide products (HJBX_OPT_MLP_ARITHMETIC) as the kernels see it ----------------------------------------
// MlpArith<AR>: the LDS image of the weights, its fill (every thread of the workgroup calls it; a __syncthreads() follows), the lane context
// made from it and the value gradient of one tile group.  AR = 0: f32 MFMA (here), 1: bf16x3 (hjbx_mlp_x3.hpp), 2: f16x2 (hjbx_mlp_h2.hpp);
// the split-operand arithmetics hold one tile per wave and exist for the ReLU network.  The soft-PD head (f32 MFMA only) stays with the
// kernels' HEAD parameter.
template <int AR> struct MlpArith;
template <> struct MlpArith<0> {
    template <int N> using Lds = MlpLds<N>;
    template <int N, int THREADS>
    static __device__ __forceinline__ void fill(Lds<N>& L, const float* __restrict__ W1g, const float* __restrict__ W2g, const float* __restrict__ W3g, int tid) {
        mlp_fill_lds<N, THREADS>(L, W1g, W2g, W3g, tid);
    }
    template <int N> static __device__ __forceinline__ MlpCtx ctx(Lds<N>& L, int lane) { return mlp_ctx<N>(L, lane); }
    template <typename S, int TL, int ACT>
    static __device__ __forceinline__ void value_grad(const S& sys, const MlpP<S::N>& p, const MlpCtx& c, const float (&xs)[TL][S::N], bool want_grad,
                                                      float (&V)[TL], float (&g)[TL][S::N]) {
        mlp_value_grad<S, TL, ACT>(sys, p, c, xs, want_grad, V, g);
    }
};
