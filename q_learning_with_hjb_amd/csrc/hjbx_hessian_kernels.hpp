// hjbx_hessian_kernels.hpp -- the device code of the two Hessian units (hjbx_hessian.hip: PD value network; hjbx_softpd_hessian.hip: soft-PD
// network of the notebooks): mlp_value_hessian, one column of a tile, i.e. its sample's forward and reverse sweep and the tangent sweep along
// its direction on the five chains of the value gradient, and k_value_hessian, the persistent kernel around it, templated on the network's
// head like the kernels of hjbx_mlp_kernels.hpp.  Design and register budget: top of hjbx_hessian.hip; launcher, dispatcher and checks:
// hjbx_mlp_host.hpp.  Each unit instantiates only its own head.
#pragma once
#include <hip/hip_runtime.h>

#include "hjbx_internal.hpp"
#include "hjbx_systems.hpp"
#include "hjbx_mlp_core.hpp"
#include "hjbx_mlp_kernels.hpp"   // the heads: MlpHeadPd, MlpHeadSoft

using namespace hjbx;

// One column of a tile: the state row of its sample in xs (every column computes; `j` is its direction, 0 for an idle column), `sj` = 1 / std_j.
// dyp: this lane's part of row j of dy_dx (its 8 float4s at 32 ob + 8 q, already offset by 4 h floats), or NULL.  On return, if want_h,
// Hcol[k] = H_x[k][j] in both lane halves.
// SOFT selects the head: false (PD) V = |y|^2 + eps_s |e|^2, the reverse sweeps start from 2y and 2y.;  true (soft-PD, `bias` = the LDS copy
// of MlpBias, smooth activations only) every layer adds its bias (the accumulators of a1, a2 and a3 start from it; a tangent has no bias),
// layer 3 is activated and V = act(a3) . w4 + b4, so the sweeps start from d3 = w4 . act'(a3) and d3. = w4 . act''(a3) . a3.; there is no
// eps_s term and no dy_dx output (dyp and want_h are not looked at: H is all there is).  The chains are the same in both.
template <typename S, int ACT, bool SOFT = false>
__device__ __forceinline__ void mlp_value_hessian(const S& sys, const MlpP<S::N>& p, const MlpCtx& c, const float (&xs)[S::N], int j, float sj,
                                                  bool want_h, float* __restrict__ dyp, float (&Hcol)[S::N], const MlpBias* bias = nullptr) {
    constexpr int N = S::N;
    constexpr int NP = MlpLds<N>::NP;
    constexpr bool kSmooth = ACT != HJBX_ACT_RELU;   // act'' != 0: the sample's reverse sweep (r2, r1) enters the Hessian
    constexpr bool kSin = ACT == HJBX_ACT_SIN;
    static_assert(!SOFT || kSmooth, "the soft-PD Hessian of a ReLU network is identically zero: no kernel");
    const int h = c.h;
    float e[N], z[N];
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = xs[k] - p.xf[k];
    sys.wrap(e);
#pragma unroll
    for (int k = 0; k < N; ++k) z[k] = (e[k] - p.mean[k]) * p.istd[k];
    float ring4[3][4], ring2[3][2];  // operand rings of the chains (DEPTH = 2)
    // One element-wise evaluation at a time for the smooth activations: left alone the scheduler interleaves the 64 independent polynomial
    // evaluations of a pass and their temporaries spill (see mlp_value_grad).
    auto fence = [&](float& v) {
        if constexpr (kSmooth) {
            asm volatile("" : "+v"(v));
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto getz = [&](int st, int) { return h ? z[2 * st + 1] : z[2 * st]; };
    auto getej = [&](int st, int) { return (2 * st + h) == j ? 1.0f : 0.0f; };   // the unit vector e_j: the chain then returns W1[j,:] exactly

    // ---- layer 1 and its tangent: h1 = act(a1), a2 = h1 W2;  a1. = W1[j,:], h1. = act'(a1) . a1. ------------------------------------------
    f32x16 a1[1][4];
    if constexpr (SOFT) bias_acc(a1, bias->b1, h);
    else zero_acc(a1);
    mfma_chain<OffW1F, N / 2, 4, 2, 1>(a1, ring4, c.w1f, getz);
    f32x16 c1[1][kSin ? 4 : 1];   // sin only: cos(a1), until h1. is formed
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (kSin) {
                float sn, cs;
                sincos1(a1[0][fb][r], sn, cs);
                asm volatile("" : "+v"(sn), "+v"(cs));
                a1[0][fb][r] = sn;
                c1[0][kSin ? fb : 0][r] = cs;
                __builtin_amdgcn_sched_barrier(0);
            } else {
                float v = act1<ACT>(a1[0][fb][r]);
                fence(v);
                a1[0][fb][r] = v;
            }
        }
    f32x16 a2[1][4];   // after its pass below: h2 = act(a2) (sin: sin(a2), with cos(a2) in c2)
    if constexpr (SOFT) bias_acc(a2, bias->b2, h);
    else zero_acc(a2);
    mfma_chain<OffW2F, 64, 4, 2, 1>(a2, ring4, c.w2f, [&](int st, int) { return a1[0][st >> 4][st & 15]; });
    f32x16 t1[1][4];
    zero_acc(t1);
    mfma_chain<OffW1F, N / 2, 4, 2, 1>(t1, ring4, c.w1f, getej);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int r = 0; r < 16; ++r) t1[0][fb][r] = dact1<ACT>(kSin ? c1[0][kSin ? fb : 0][r] : a1[0][fb][r], t1[0][fb][r]);

    // ---- layer 2 and its tangent: h2 = act(a2);  a2. = h1. W2, h2. = act'(a2) . a2., y. = h2. W3 ---------------------------------------------
    f32x16 c2[1][kSin ? 4 : 1];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (kSin) {
                float sn, cs;
                sincos1(a2[0][fb][r], sn, cs);
                asm volatile("" : "+v"(sn), "+v"(cs));
                a2[0][fb][r] = sn;
                c2[0][kSin ? fb : 0][r] = cs;
                __builtin_amdgcn_sched_barrier(0);
            } else {
                float v = act1<ACT>(a2[0][fb][r]);
                fence(v);
                a2[0][fb][r] = v;
            }
        }
    // act'(a2) . d in terms of what is kept of layer 2
    auto dact2 = [&](int fb, int r, float d) { return dact1<ACT>(kSin ? c2[0][kSin ? fb : 0][r] : a2[0][fb][r], d); };
    // The element-wise passes between the chains touch at most three 64-register quantities each and are fenced from one another: what a
    // pass works on has to sit in the architectural half of the register file, the rest waits in the accumulation half.
    f32x16 t2[1][4];   // a2.; later act''(a2) . a2., then q2 = r2 . act''(a2) . a2.
    zero_acc(t2);
    mfma_chain<OffW2F, 64, 4, 2, 1>(t2, ring4, c.w2f, [&](int st, int) { return t1[0][st >> 4][st & 15]; });
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int r = 0; r < 16; ++r) t1[0][fb][r] = dact2(fb, r, t2[0][fb][r]);   // h2. (h1. is dead)
    f32x16 yd[1][2];   // y. (soft-PD: a3.); then the start of the tangent's reverse sweep, 2 y. (soft-PD: d3.)
    zero_acc(yd);
    mfma_chain<OffW3F, 64, 2, 2, 1>(yd, ring2, c.w3f, [&](int st, int) { return t1[0][st >> 4][st & 15]; });
    if constexpr (!SOFT) {
        // registers 4q .. 4q + 3 of block ob are the outputs 32 ob + 8 q + 4 h + 0..3: one float4
        if (dyp) {
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(dyp + 32 * ob + 8 * q) =
                        make_float4(yd[0][ob][4 * q] * sj, yd[0][ob][4 * q + 1] * sj, yd[0][ob][4 * q + 2] * sj, yd[0][ob][4 * q + 3] * sj);
        }
        if (!want_h) return;
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int r = 0; r < 16; ++r) yd[0][ob][r] = yd[0][ob][r] + yd[0][ob][r];
    }

    // ---- the sample's reverse sweep (smooth activations): r2 = 2y W3', q2 = r2 . act''(a2) . a2., r1 = (r2 . act'(a2)) W2' ----------------
    f32x16 r1[1][4];   // r1, then m1 = r1 . a1.
    zero_acc(r1);
    if constexpr (kSmooth) {
        // act''(a2) . a2.: sin -sin(a2) a2.;  tanh -2 h (1 - h^2) a2.
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (kSin) t2[0][fb][r] = -a2[0][fb][r] * t2[0][fb][r];
                else t2[0][fb][r] = -2.0f * a2[0][fb][r] * dact2(fb, r, t2[0][fb][r]);
            }
        f32x16 y[1][2];   // y, then the start of the sample's reverse sweep: 2y (soft-PD: a3, then d3)
        if constexpr (SOFT) bias_acc(y, bias->b3, h);
        else zero_acc(y);
        mfma_chain<OffW3F, 64, 2, 2, 1>(y, ring2, c.w3f, [&](int st, int) { return a2[0][st >> 4][st & 15]; });
        if constexpr (SOFT) {
            // d3 = w4 . act'(a3) in place of a3, d3. = w4 . act''(a3) . a3. in place of a3. (w4 from the LDS bias block, as in mlp_value_grad)
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 w = *reinterpret_cast<const float4*>(bias->w4 + 32 * ob + 8 * q + 4 * h);
                    const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const float a = y[0][ob][4 * q + jj];
                        float d3, d3t;
                        if constexpr (kSin) {
                            float sn, cs;
                            sincos1(a, sn, cs);
                            d3 = cs * wv[jj];
                            d3t = -(sn * wv[jj]) * yd[0][ob][4 * q + jj];                 // act'' = -sin
                        } else {
                            const float hh = tanh1(a);
                            d3 = dact1<ACT>(hh, wv[jj]);
                            d3t = -2.0f * hh * d3 * yd[0][ob][4 * q + jj];                // act'' = -2 h act'
                        }
                        asm volatile("" : "+v"(d3), "+v"(d3t));
                        y[0][ob][4 * q + jj] = d3;
                        yd[0][ob][4 * q + jj] = d3t;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
        } else {
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) y[0][ob][r] = y[0][ob][r] + y[0][ob][r];
        }
        f32x16 r2[1][4];
        zero_acc(r2);
        mfma_chain<OffW3B, 32, 4, 2, 1>(r2, ring4, c.w3b, [&](int st, int) { return y[0][st >> 4][st & 15]; });
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) t2[0][fb][r] = t2[0][fb][r] * r2[0][fb][r];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) r2[0][fb][r] = dact2(fb, r, r2[0][fb][r]);
        mfma_chain<OffW2B, 64, 4, 2, 1>(r1, ring4, c.w2b, [&](int st, int) { return r2[0][st >> 4][st & 15]; });
        // m1 = r1 . a1. (a1. = W1[j,:] once more; h2. in t1 is dead)
        zero_acc(t1);
        mfma_chain<OffW1F, N / 2, 4, 2, 1>(t1, ring4, c.w1f, getej);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 16; ++r) r1[0][fb][r] = r1[0][fb][r] * t1[0][fb][r];
    }

    // ---- tangent, reverse: r2. = 2 y. W3', d2. = r2. . act'(a2) + q2, r1. = d2. W2' ---------------------------------------------------------
    f32x16 u2[1][4];
    zero_acc(u2);
    mfma_chain<OffW3B, 32, 4, 2, 1>(u2, ring4, c.w3b, [&](int st, int) { return yd[0][st >> 4][st & 15]; });
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (kSmooth) u2[0][fb][r] = dact2(fb, r, u2[0][fb][r]) + t2[0][fb][r];
            else u2[0][fb][r] = dact2(fb, r, u2[0][fb][r]);
        }
    f32x16 u1[1][4];
    zero_acc(u1);
    mfma_chain<OffW2B, 64, 4, 2, 1>(u1, ring4, c.w2b, [&](int st, int) { return u2[0][st >> 4][st & 15]; });

    // ---- d1. = r1. . act'(a1) + act''(a1) . m1 and the last product H_z[:,j] = d1. W1' on the VALU, as backward 1 of mlp_value_grad ---------
    // layer 1 once more for act'(a1), act''(a1) (n / 2 x 4 MFMAs)
    if constexpr (SOFT) bias_acc(a1, bias->b1, h);
    else zero_acc(a1);
    mfma_chain<OffW1F, N / 2, 4, 2, 1>(a1, ring4, c.w1f, getz);
    if constexpr (kSmooth) {   // d1. in place of r1., in a pass of its own (three quantities; the products below then read one)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                float dv;
                if constexpr (kSin) {
                    float sn, cs;
                    sincos1(a1[0][kb][s], sn, cs);
                    dv = cs * u1[0][kb][s] - sn * r1[0][kb][s];                       // act'' = -sin
                } else {
                    const float hh = tanh1(a1[0][kb][s]);
                    dv = dact1<ACT>(hh, u1[0][kb][s] - 2.0f * hh * r1[0][kb][s]);      // act'' = -2 h act'
                }
                fence(dv);
                u1[0][kb][s] = dv;
            }
    }
    f32x2 part[NP / 2];
#pragma unroll
    for (int k = 0; k < NP / 2; ++k) part[k] = f32x2{0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            float dv;
            if constexpr (kSmooth) dv = u1[0][kb][s];
            else dv = dact1<ACT>(a1[0][kb][s], u1[0][kb][s]);
            const f32x2 dv2{dv, dv};
#pragma unroll
            for (int q = 0; q < NP / 4; ++q) {
                const float4 w = c.w1t[(32 * kb + perm(s)) * (NP / 4) + q];
                part[2 * q + 0] = __builtin_elementwise_fma(f32x2{w.x, w.y}, dv2, part[2 * q + 0]);
                part[2 * q + 1] = __builtin_elementwise_fma(f32x2{w.z, w.w}, dv2, part[2 * q + 1]);
            }
        }
    if constexpr (SOFT) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float pk = part[k >> 1][k & 1];
            const float v = pk + __shfl_xor(pk, 32, 64);
            Hcol[k] = v * p.istd[k] * sj;
        }
    } else {
        // (j as the tile loop's code sees it here and now: the n diagonal terms [k == j] 2 eps_s are per-lane loop invariants otherwise, hoisted
        //  out of the tile loop and kept in registers through every chain)
        int jd = j;
        asm volatile("" : "+v"(jd));
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float pk = part[k >> 1][k & 1];
            const float v = pk + __shfl_xor(pk, 32, 64);
            Hcol[k] = v * p.istd[k] * sj + (k == jd ? 2.f * p.eps_s : 0.f);
        }
    }
}

// ---- the kernel: H (B,n,n) and, PD head only, dy_dx (B,n,64) for a batch of states (hjbx_value_hessian_f32, hjbx_softpd_value_hessian_f32) ----
// Tile group g = the samples g C .. g C + C - 1; work distribution and LDS staging as in k_value_grad_mfma (a contiguous range of groups per
// workgroup, pulled by its waves from an LDS counter).  The soft-PD head has H as its one output: it takes Hout as given and ignores dyout.
static constexpr int kHessWaves = 4;   // one wave per SIMD: up to 512 registers each

template <typename S, int WAVES, int ACT, typename HEAD>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void k_value_hessian(S sys, MlpP<S::N> p, const float* __restrict__ W1g,
                                                                       const float* __restrict__ W2g, const float* __restrict__ W3g,
                                                                       const float* __restrict__ x, float* __restrict__ Hout,
                                                                       float* __restrict__ dyout, int64_t B, int64_t ngroups, HEAD head) {
    constexpr int N = S::N;
    constexpr int C = 32 / N;   // samples per tile
    static_assert(N % 2 == 0 && C >= 1, "state dimension must be even (k-steps of 2) and at most 32");
    __shared__ __attribute__((aligned(256))) typename HEAD::template Lds<N, 0> L;
    const int tid = threadIdx.x;
    if (tid == 0) L.next = WAVES;  // groups 0..WAVES-1 of the range are taken statically
    mlp_fill_lds<N, WAVES * 64>(L, W1g, W2g, W3g, tid);
    if constexpr (HEAD::kSoft) mlp_fill_bias<WAVES * 64>(L.bias, head.b1, head.b2, head.b3, head.w4, head.b4, tid);
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
        bool want_h = true;   // soft-PD: no run-time test of either output pointer
        if constexpr (HEAD::kSoft) {
            mlp_value_hessian<S, ACT, true>(sys, p, c, xs, j, sj, true, nullptr, Hcol, &L.bias);
        } else {
            want_h = Hout != nullptr;
            float* dyp = (dyout && live) ? dyout + (env * N + j) * kH3 + 4 * h : nullptr;
            mlp_value_hessian<S, ACT>(sys, p, c, xs, j, sj, want_h, dyp, Hcol);
        }
        if (want_h && live && h == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k) Hout[(env * N + k) * N + j] = Hcol[k];
        }
        int nxt = 0;
        if (lane == 0) nxt = atomicAdd(&L.next, 1);
        grp = g_begin + __builtin_amdgcn_readfirstlane(nxt);
    }
}
