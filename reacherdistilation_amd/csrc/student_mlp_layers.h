// student_mlp.hip's layers on a row block in LDS: the f32 forward, data-gradient, weight-gradient
// and bias-gradient templates (v_mfma_f32_16x16x4_f32), their bf16 siblings (student_mlp_bf16.h,
// included below, after the templates it builds on) and the selectors fwd / dgrad / wgrad, which
// take layer L to the arithmetic of a kernel instance.  Included inside student_mlp.hip's anonymous
// namespace after student_mlp_layout.h; expects rd_device.h (f32x4, mfma, ld4, tanh_fast, the SrcC
// fence).
#pragma once

// Forward of layer L: Y[row][pk(c)] = act(b[c] + sum_k X[row][k] W[k][c]), c = 16 cb + i.
// FENCE: every k-group's MFMAs are SrcC-fenced (rd_device.h), for a kernel in which hipcc would
// otherwise load the next operands into a register an in-flight MFMA still reads as SrcC (the bias
// quad shared by a wave's row blocks: student_mlp_envs_kernel<64, true>); the same values.
template <int RB, int L, int SI, int SO, bool FENCE = false>
__device__ __forceinline__ void fwd_layer(const float* X, float* Y, const float* img, int wave, int i, int g) {
    constexpr int NCB = MP[L] / 16, KG = (IN[L] + 15) / 16;
    using PT = Part<NCB, RB>;
    if (!PT::active(wave)) return;
    const float* W = img + FW[L];
    const float* bias = img + BB[L];
    f32x4 acc[PT::CPW][PT::RPW];
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c) {
        const float b = bias[16 * PT::cb(wave, c) + i];
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) acc[c][r] = f32x4{b, b, b, b};
    }
#pragma unroll 2
    for (int S = 0; S < KG; ++S) {   // 4 k-steps per iteration: k = 16 S + 4 sub + g
        f32x4 a[PT::RPW];
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) a[r] = ld4(X + (16 * PT::rb(wave, r) + i) * SI + 16 * S + 4 * g);
#pragma unroll
        for (int c = 0; c < PT::CPW; ++c) {
            const f32x4 w = ld4(W + ((S * MP[L] + 16 * PT::cb(wave, c) + i) << 4) + 4 * g);
            if constexpr (FENCE) fence_begin(acc[c]);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int r = 0; r < PT::RPW; ++r) acc[c][r] = mfma(a[r][sub], w[sub], acc[c][r]);
            if constexpr (FENCE) fence_end(acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c)
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = acc[c][r][q];
                Y[(16 * PT::rb(wave, r) + 4 * g + q) * SO + pk(16 * PT::cb(wave, c) + i)] = TANH[L] ? tanh_fast(v) : v;
            }
}

// Backward data of layer L: out[row][pk(c)] = (sum_m D[row][m] W[c][m]) * act'(H[row][c]),
// c = 16 cb + i an input feature of layer L; act' = 1 - H^2 when layer L-1 ends in tanh
// (H = X_L, the layer's input).
template <int RB, int L, int SD, int SH, int SO>
__device__ __forceinline__ void dgrad_layer(const float* D, const float* H, float* out, const float* img, int wave,
                                            int i, int g) {
    constexpr int NCB = KP[L] / 16, MG = (OUT[L] + 15) / 16;
    using PT = Part<NCB, RB>;
    if (!PT::active(wave)) return;
    const float* W = img + BW[L];
    f32x4 acc[PT::CPW][PT::RPW];
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c)
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) acc[c][r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int S = 0; S < MG; ++S) {
        f32x4 a[PT::RPW];
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) a[r] = ld4(D + (16 * PT::rb(wave, r) + i) * SD + 16 * S + 4 * g);
#pragma unroll
        for (int c = 0; c < PT::CPW; ++c) {
            const f32x4 w = ld4(W + ((S * KP[L] + 16 * PT::cb(wave, c) + i) << 4) + 4 * g);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int r = 0; r < PT::RPW; ++r) acc[c][r] = mfma(a[r][sub], w[sub], acc[c][r]);
        }
    }
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c)
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * PT::rb(wave, r) + 4 * g + q, pos = pk(16 * PT::cb(wave, c) + i);
                float v = acc[c][r][q];
                if (TANH[L - 1]) {
                    const float h = H[row * SH + pos];
                    v *= fmaf(-h, h, 1.0f);
                }
                out[row * SO + pos] = v;
            }
}

// Weight gradient of layer L over the block: G[16kb + 4g + q][16cb + i] += sum_row
// H[row][16kb + 4g + q] D[row][16cb + i].  A wave owns one column block cb = wave % NCB
// (its B operand is loaded once per k-step) and the row blocks kb = wave / NCB + (8/NCB) t.
template <int L>
struct WG {
    static constexpr int NCB = MP[L] / 16, KBN = KP[L] / 16, STEP = WAVES / NCB;
    static constexpr int Q = (KBN + STEP - 1) / STEP;
    static_assert(WAVES % NCB == 0, "wgrad partition");
    __device__ static int kb(int wave, int t) { return wave / NCB + STEP * t; }
    __device__ static bool ok(int wave, int t) { return KBN % STEP == 0 || kb(wave, t) < KBN; }
};

// Each k-step's MFMAs are SrcC-fenced (rd_device.h): unfenced, hipcc issues the next k-step's
// operand loads into registers an in-flight MFMA still reads as SrcC.
template <int ROWS, int L, int SH, int SD>
__device__ __forceinline__ void wgrad_layer(const float* H, const float* D, f32x4 (&G)[WG<L>::Q], int wave, int i,
                                            int g) {
    using W = WG<L>;
    const int cb = wave % W::NCB;
#pragma unroll 4
    for (int s = 0; s < ROWS / 4; ++s) {
        const int row = 4 * s + g;
        const float b = D[row * SD + pk(16 * cb + i)];
        float h[W::Q];
#pragma unroll
        for (int t = 0; t < W::Q; ++t) h[t] = W::ok(wave, t) ? H[row * SH + pk(16 * W::kb(wave, t) + i)] : 0.0f;
        fence_begin(G);
#pragma unroll
        for (int t = 0; t < W::Q; ++t)
            if (W::ok(wave, t)) G[t] = mfma(h[t], b, G[t]);
        fence_end(G);
    }
}

// partial-row stores (non-temporal measured no gain: profiles/r05_removed_diagnostic_variants.diff)
__device__ __forceinline__ void wst(float* p, float v) { *p = v; }

template <int L>
__device__ __forceinline__ void store_wgrad(float* ws, const f32x4 (&G)[WG<L>::Q], int wave, int i, int g) {
    using W = WG<L>;
    const int cb = wave % W::NCB;
#pragma unroll
    for (int t = 0; t < W::Q; ++t)
        if (W::ok(wave, t))
#pragma unroll
            for (int q = 0; q < 4; ++q)
                wst(ws + GW[L] + (16 * W::kb(wave, t) + 4 * g + q) * MP[L] + 16 * cb + i, G[t][q]);
}

// bias gradient: thread t < OUT[L] sums column t of dZ_L over the block's rows
template <int ROWS, int L, int SD>
__device__ __forceinline__ void bgrad_layer(const float* D, float& gb, int tid) {
    if (tid < OUT[L]) {
        const int col = pk(tid);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int r = 0; r < ROWS; r += 4) {
            s0 += D[(r + 0) * SD + col];
            s1 += D[(r + 1) * SD + col];
            s2 += D[(r + 2) * SD + col];
            s3 += D[(r + 3) * SD + col];
        }
        gb += (s0 + s1) + (s2 + s3);
    }
}

// the bf16 siblings of the three layer templates above, and the bf16 weight image
#include "student_mlp_bf16.h"

// Layer L in the arithmetic of the instance: BF takes layers 1..3 to their bf16 siblings.
template <bool BF, int RB, int L, int SI, int SO, bool FENCE = false>
__device__ __forceinline__ void fwd(const float* X, float* Y, const float* img, int wave, int i, int g) {
    if constexpr (BF && is_bf_layer(L)) fwd_layer_bf<RB, L, SI, SO>(X, Y, img, wave, i, g);
    else fwd_layer<RB, L, SI, SO, FENCE>(X, Y, img, wave, i, g);
}
template <bool BF, int RB, int L, int SD, int SH, int SO>
__device__ __forceinline__ void dgrad(const float* D, const float* H, float* out, const float* img, int wave, int i,
                                      int g) {
    if constexpr (BF && is_bf_layer(L)) dgrad_layer_bf<RB, L, SD, SH, SO>(D, H, out, img, wave, i, g);
    else dgrad_layer<RB, L, SD, SH, SO>(D, H, out, img, wave, i, g);
}
template <bool BF, int ROWS, int L, int SH, int SD>
__device__ __forceinline__ void wgrad(const float* H, const float* D, f32x4 (&G)[WG<L>::Q], int wave, int i, int g) {
    if constexpr (BF && is_bf_layer(L)) wgrad_layer_bf<ROWS, L, SH, SD>(H, D, G, wave, i, g);
    else wgrad_layer<ROWS, L, SH, SD>(H, D, G, wave, i, g);
}
