// student_lstm.hip's fused head (at most HF_MAX_ROWS rows): head_layer and head_stage, the packed
// weight image and pack_heads_kernel, HeadLoss / row_loss, head_fwd_kernel, the data- and
// weight-gradient pieces, head_bwd_kernel, and the launches that finish the gradient after BPTT
// (head_part_sum, dense32_dot, grad_finish_kernel, head_wgrad_reduce_kernel, dense32_grad_kernel).
// Included inside student_lstm.hip's anonymous namespace after student_lstm_layout.h (the
// persistent header stands between, to keep the kernels' order in the object); expects rd_gemm.h.
#pragma once

// The head 200-64-128-64-32-4 (student_nn.py:42-46) over a few hundred rows is five launches of
// ~10 us each, none of them busy.  head_fwd_kernel runs all five layers for 16 rows per
// workgroup: activations stay in LDS between layers, weights stream from L2 as the B
// operands, and every layer's output is also stored (A1..A4 for the backward, Y).  Same MFMA
// k order and epilogue (acc + b, tanhf) as the unsplit rd_gemm launches it replaces.
// FENCE: the chain of a column block in groups of HF_FG k steps whose operands are in registers before
// the group starts, each group between fence_begin / fence_end (rd_device.h); same MFMAs in the same
// order.  For a kernel that runs out of registers around the head: the register allocator there renames
// the chain's accumulator and lets an operand's LDS read or a spilled value's reload land in the SrcC
// registers it freed while the 8-pass MFMA still reads them (scripts/isa/hazards.py class LDSRC).
constexpr int HF_FG = 16;
constexpr int HF_ROWS = 16, HF_MAX_ROWS = 1 << 18;
constexpr int64_t HPART_MAX_FLOATS = (int64_t)128 << 20;   // the fused head's partial rows: at most 512 MB (reacher_student_lstm.h)
template <int K, int N, bool TANH, int NW = 4, bool FENCE = false, int LI, int LO>
__device__ __forceinline__ void head_layer(const float (*in)[LI], float (*out)[LO], const float* __restrict__ W,
                                           const float* __restrict__ b, float* __restrict__ gout, int ldg,
                                           int64_t row0, int64_t R) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, gq = lane >> 4;
    constexpr int NB = (N + 15) / 16;
#pragma unroll
    for (int it = 0; it < (NB + NW - 1) / NW; ++it) {   // unrolled: every weight load of the layer in flight at once
        const int cb = wave + NW * it;   // NW waves share the layer's column blocks
        if (cb >= NB) break;
        const int col = 16 * cb + i;
        const bool cv = col < N;
        rdg::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (FENCE) {
            rdg::f32x4 fa[1] = {acc};
#pragma unroll
            for (int k0 = 0; k0 < K / 4; k0 += HF_FG) {
                float av[HF_FG], wv[HF_FG];
#pragma unroll
                for (int e = 0; e < HF_FG; ++e) {
                    const int k = 4 * (k0 + e) + gq;
                    av[e] = k0 + e < K / 4 ? in[i][k] : 0.0f;
                    wv[e] = k0 + e < K / 4 && cv ? W[k * N + col] : 0.0f;
                }
                fence_begin(fa);
#pragma unroll
                for (int e = 0; e < HF_FG; ++e)
                    if (k0 + e < K / 4) fa[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wv[e], fa[0], 0, 0, 0);
                fence_end(fa);
            }
            acc = fa[0];
        } else {
#pragma unroll
            for (int kq = 0; kq < K / 4; ++kq) {
                const int k = 4 * kq + gq;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(in[i][k], cv ? W[k * N + col] : 0.0f, acc, 0, 0, 0);
            }
        }
        const float bv = cv ? b[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * gq + r;
            float v = acc[r] + bv;
            if (TANH) v = tanhf(v);
            if (cv) {
                out[row][col] = v;
                if (row0 + row < R) gout[(row0 + row) * ldg + col] = v;
            }
        }
    }
    __syncthreads();
}

// rows row0.. of a [R][ld] matrix, columns 0..COLS-1 -> dst[16][LDD] (zero past R): every
// load of the thread issued before its first LDS store (one round trip, not one per element)
template <int COLS, int LDD, int NT = 256>
__device__ __forceinline__ void head_stage(const float* __restrict__ src, int ld, int64_t row0, int64_t R,
                                           float (*dst)[LDD], int tid) {
    constexpr int PER = (HF_ROWS * COLS + NT - 1) / NT;
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int x = tid + NT * j, row = x / COLS, c = x - row * COLS;
        v[j] = (x < HF_ROWS * COLS && row0 + row < R) ? src[(row0 + row) * ld + c] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int x = tid + NT * j, row = x / COLS, c = x - row * COLS;
        if (x < HF_ROWS * COLS) dst[row][c] = v[j];
    }
}

// workgroup (t, rb) of the grid T x nb: rows t B + 16 rb .. of step t, with step t's head.
// WL (grids of at most HB_WIDE_GRID workgroups, e.g. the reference's 20 windows): the head's
// 31,652 parameters are copied into LDS first (LDS-DMA, one issue burst beside the row
// staging), so the five layers read their B operands from LDS instead of paying an L2/HBM
// round trip each (round 5); same values, same MFMA order.  Larger grids stream them from L2
// (124 KB of LDS would leave one workgroup per CU).
constexpr int HB_WIDE_GRID = 256;   // at most this many one-tile workgroups: the latency-bound forms
static_assert(HSZ % 4 == 0 && (OFF_H % 4) == 0, "16-B pieces of a head's parameters");
// A head's weights in the head backward's MFMA operand order ("packed"), kept beside the
// parameters (t->wpack, [T][HWP]): written by the Adam kernel with every update and by
// pack_heads_kernel when the parameters are set.  Per layer (W5, W4, W3, W2, W1 of [NI][KO]),
// per column block cb < ceil(NI / 16) and k step kq < KO / 4, 64 floats, lane (i, gq) ->
// W[16 cb + i][4 kq + gq] (zero past NI).  A wave of head_bwd_kernel<false, 16> loads each of its
// B operands with one coalesced 256-B access instead of sixteen 16-B pieces of sixteen lines
// (the [NI][KO] layout read per lane cost the backward 15 us of a 24 us launch at 20 windows,
// profiles/r05p_*).
__host__ __device__ constexpr int hw_size(int KO, int NI) { return ((NI + 15) / 16) * 16 * KO; }
constexpr int HWP_5 = 0, HWP_4 = HWP_5 + hw_size(4, H4), HWP_3 = HWP_4 + hw_size(H4, H3),
              HWP_2 = HWP_3 + hw_size(H3, H2), HWP_1 = HWP_2 + hw_size(H2, H1), HWP = HWP_1 + hw_size(H1, U);
// packed index of head offset o (within one head's HSZ), or -1 for the biases (KO is a power of
// two in every layer: shifts and masks, no divisions)
template <int KO>
__device__ __forceinline__ int hw_at(int base, int rel) {
    const int col = rel / KO, k = rel & (KO - 1);
    return base + (((col >> 4) * (KO / 4) + (k >> 2)) << 6) + ((k & 3) << 4) + (col & 15);
}
__device__ __forceinline__ int hw_index(int o) {
    static_assert((H1 & (H1 - 1)) == 0 && (H2 & (H2 - 1)) == 0 && (H3 & (H3 - 1)) == 0 && (H4 & (H4 - 1)) == 0,
                  "power-of-two layer widths");
    if (o < OFF_B1) return hw_at<H1>(HWP_1, o - OFF_W1);
    if (o >= OFF_W2 && o < OFF_B2) return hw_at<H2>(HWP_2, o - OFF_W2);
    if (o >= OFF_W3 && o < OFF_B3) return hw_at<H3>(HWP_3, o - OFF_W3);
    if (o >= OFF_W4 && o < OFF_B4) return hw_at<H4>(HWP_4, o - OFF_W4);
    if (o >= OFF_W5 && o < OFF_B5) return hw_at<4>(HWP_5, o - OFF_W5);
    return -1;
}
__global__ __launch_bounds__(256) void pack_heads_kernel(const float* __restrict__ P, float* __restrict__ wpack, int T) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)T * HSZ) return;
    const int ts = (int)(q / HSZ), o = (int)(q - (int64_t)ts * HSZ);
    const int w = hw_index(o);
    if (w >= 0) wpack[(int64_t)ts * HWP + w] = P[OFF_H + q];
}
// step t's head -> W (16-B LDS-DMA pieces, lane l of a wave's burst to base + 16 l); the caller
// waits (vmcnt) before its barrier
__device__ __forceinline__ void head_params_to_lds(const float* __restrict__ P, float* W) {
    constexpr int V4 = HSZ / 4, PER = (V4 + 255) / 256;
    const int wbase = threadIdx.x & ~63;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int x = threadIdx.x + 256 * u;
        if (x < V4) __builtin_amdgcn_global_load_lds(P + 4 * x, W + 4 * (wbase + 256 * u), 16, 0, 0);
    }
}
// The loss of a training forward (small batches; loss_kernel's per-row arithmetic) at the end
// of head_fwd_kernel: dY of the workgroup's rows and its loss / squared-error sums; the metrics
// (their sum in workgroup order) are formed by grad_finish_kernel after BPTT.
struct HeadLoss {
    const float* tgt;   // null: no loss (inference forward)
    float* dY;
    float* part;        // [grid][2] partial sums
    float inv_n;
    int loss;
};
__device__ __forceinline__ float2 row_loss(const float* o, const float* t, int loss, float inv_n, float* d) {
    const float e0 = o[0] - t[0], e1 = o[1] - t[1];
    const float sq = fmaf(e0, e0, e1 * e1);
    float lv, d0, d1, d2 = 0.f, d3 = 0.f;
    if (loss == RDL_LOSS_MSE) {
        d0 = e0 * inv_n;
        d1 = e1 * inv_n;
        lv = 0.5f * inv_n * sq;
    } else {
        const float ivt0 = expf(-2.0f * t[2]), ivt1 = expf(-2.0f * t[3]);
        const float vs0 = expf(2.0f * o[2]), vs1 = expf(2.0f * o[3]);
        lv = ((t[2] - o[2]) + 0.5f * (vs0 + e0 * e0) * ivt0 - 0.5f) +
             ((t[3] - o[3]) + 0.5f * (vs1 + e1 * e1) * ivt1 - 0.5f);
        d0 = e0 * ivt0;
        d1 = e1 * ivt1;
        d2 = fmaf(vs0, ivt0, -1.0f);
        d3 = fmaf(vs1, ivt1, -1.0f);
    }
    d[0] = d0; d[1] = d1; d[2] = d2; d[3] = d3;
    return make_float2(lv, sq);
}
template <bool WL>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ Hc, const float* __restrict__ P0,
                                                       float* A1, float* A2, float* A3, float* A4, float* Y, int64_t B,
                                                       int nb, HeadLoss hl) {
    __shared__ __attribute__((aligned(16))) float Wl[WL ? HSZ : 4];
    __shared__ __attribute__((aligned(16))) float X0[HF_ROWS][U + 4];
    __shared__ __attribute__((aligned(16))) float X1[HF_ROWS][L1];
    __shared__ __attribute__((aligned(16))) float X2[HF_ROWS][L2];
    __shared__ __attribute__((aligned(16))) float X3[HF_ROWS][L3];
    __shared__ __attribute__((aligned(16))) float X4[HF_ROWS][L4];
    __shared__ __attribute__((aligned(16))) float X5[HF_ROWS][8];
    const int ts = blockIdx.x / nb, rb = blockIdx.x - ts * nb;
    const int64_t row0 = (int64_t)ts * B + (int64_t)rb * HF_ROWS, R = (int64_t)(ts + 1) * B;
    const float* P = P0 + OFF_H + (int64_t)ts * HSZ;
    if constexpr (WL) head_params_to_lds(P, Wl);
    head_stage<U, U + 4>(Hc, U, row0, R, X0, threadIdx.x);
    if constexpr (WL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of Wl have landed
    __syncthreads();
    const float* W = WL ? (const float*)Wl : P;
    head_layer<U, H1, true>(X0, X1, W + OFF_W1, W + OFF_B1, A1, L1, row0, R);
    head_layer<H1, H2, true>(X1, X2, W + OFF_W2, W + OFF_B2, A2, L2, row0, R);
    head_layer<H2, H3, true>(X2, X3, W + OFF_W3, W + OFF_B3, A3, L3, row0, R);
    head_layer<H3, H4, true>(X3, X4, W + OFF_W4, W + OFF_B4, A4, L4, row0, R);
    head_layer<H4, 4, false>(X4, X5, W + OFF_W5, W + OFF_B5, Y, 4, row0, R);
    if (!hl.tgt) return;   // (uniform) inference forward
    __shared__ float ls[HF_ROWS][2];
    const int tid = threadIdx.x;
    if (tid < HF_ROWS) {   // X5 holds the layer's output rows (head_layer ends with a barrier)
        float2 v = make_float2(0.f, 0.f);
        if (row0 + tid < R) {
            float o[4] = {X5[tid][0], X5[tid][1], X5[tid][2], X5[tid][3]};
            float d[4];
            v = row_loss(o, hl.tgt + (row0 + tid) * 4, hl.loss, hl.inv_n, d);
            *reinterpret_cast<rdg::f32x4*>(hl.dY + (row0 + tid) * 4) = rdg::f32x4{d[0], d[1], d[2], d[3]};
        }
        ls[tid][0] = v.x;
        ls[tid][1] = v.y;
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, b = 0.f;
        for (int r = 0; r < HF_ROWS; ++r) { a += ls[r][0]; b += ls[r][1]; }
        hl.part[2 * blockIdx.x] = a;
        hl.part[2 * blockIdx.x + 1] = b;
    }
}

// Head backward for the same small batches: per 16-row workgroup the data gradients down the
// head (tanh' of the stored activations fused, as the EPI_DTANH GEMMs), dh_head for BPTT,
// and the five [dW; db] weight-gradient partials over its rows (the stored activations carry
// the ones column; Hc gets one in LDS) as one partial row of the flat [W1 b1 ... W5 b5] range;
// head_wgrad_reduce_kernel sums the rows in a fixed order.  Two launches instead of six.
constexpr int HB_PART = HSZ;   // 31,652 floats: [W1;b1][W2;b2][W3;b3][W4;b4][W5;b5] of one head
// dIn[16][NI] = (dOut[16][KO] . W^T) (* (1 - act^2) when DT); W is [NI][KO] (layer input x output)
// wf(it, kq, cv, col, k): the weight W[col][k] of this lane's column block it, k step kq (zero
// past NI): streamed from L2 (head_dgrad) or held in registers (head_bwd_kernel<true>)
template <int KO, int NI, bool DT, int NW, int LD, int LI, int LA, class WF>
__device__ __forceinline__ void head_dgrad_f(const float (*dout)[LD], float (*din)[LI], const float (*act)[LA], WF wf,
                                             float* gout, int ldg, int64_t row0, int64_t R, int tid) {
    const int wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    constexpr int NB = (NI + 15) / 16, IT = (NB + NW - 1) / NW;
    if constexpr (NW != 16) {   // four waves (mid-size batches: weights streamed per MFMA, 56 VGPRs;
                                // the fenced form below held 167 and ran slower) and MT (weights in
                                // registers already): the round-4 chains, clean in the hazard scan
#pragma unroll
        for (int it = 0; it < IT; ++it) {   // unrolled: every weight load of the layer in flight at once
            const int cb = wave + NW * it;
            if (cb >= NB) break;
            const int col = 16 * cb + i;
            const bool cv = col < NI;
            rdg::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kq = 0; kq < KO / 4; ++kq) {
                const int k = 4 * kq + gq;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dout[i][k], wf(it, kq, cv, col, k), acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * gq + r;
                float v = acc[r];
                if (DT) {
                    const float a = act[row][col < NI ? col : 0];
                    v *= fmaf(-a, a, 1.0f);
                }
                if (cv) {
                    if (din) din[row][col] = v;
                    if (gout && row0 + row < R) gout[(row0 + row) * ldg + col] = v;
                }
            }
        }
        return;
    }
    // the chains' operands: dout's (shared by every column block) and this lane's weights, all
    // loads issued before the first MFMA; the chains interleave (one accumulator per block)
    float av[KO / 4], bv[IT][KO / 4];
#pragma unroll
    for (int kq = 0; kq < KO / 4; ++kq) av[kq] = dout[i][4 * kq + gq];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int col = 16 * (wave + NW * it) + i;
        const bool cv = wave + NW * it < NB && col < NI;
#pragma unroll
        for (int kq = 0; kq < KO / 4; ++kq) bv[it][kq] = wf(it, kq, cv, col, 4 * kq + gq);
    }
    rdg::f32x4 acc[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) acc[it] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
    fence_begin(acc);
#pragma unroll
    for (int kq = 0; kq < KO / 4; ++kq) {
#pragma unroll
        for (int it = 0; it < IT; ++it)
            if (wave + NW * it < NB) acc[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kq], bv[it][kq], acc[it], 0, 0, 0);
    }
    fence_end(acc);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int cb = wave + NW * it;
        if (cb >= NB) break;
        const int col = 16 * cb + i;
        const bool cv = col < NI;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * gq + r;
            float v = acc[it][r];
            if (DT) {
                const float a = act[row][col < NI ? col : 0];
                v *= fmaf(-a, a, 1.0f);
            }
            if (cv) {
                if (din) din[row][col] = v;
                if (gout && row0 + row < R) gout[(row0 + row) * ldg + col] = v;
            }
        }
    }
}
template <int KO, int NI, bool DT, int NW = 4, int LD, int LI, int LA>
__device__ __forceinline__ void head_dgrad(const float (*dout)[LD], float (*din)[LI], const float (*act)[LA],
                                           const float* __restrict__ W, float* gout, int ldg, int64_t row0, int64_t R,
                                           int tid) {
    head_dgrad_f<KO, NI, DT, NW>(dout, din, act,
                                 [W](int, int, bool cv, int col, int k) { return cv ? W[col * KO + k] : 0.0f; }, gout,
                                 ldg, row0, R, tid);
}
// this lane's weights of head_dgrad_f's column blocks (it) and k steps (kq), loaded once
template <int KO, int NI, int NW>
struct HeadW {
    static constexpr int NB = (NI + 15) / 16, IT = (NB + NW - 1) / NW;
    float w[IT][KO / 4];
    __device__ __forceinline__ void load(const float* __restrict__ W, int tid) {
        const int wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int cb = wave + NW * it, col = 16 * cb + i;
            const bool cv = cb < NB && col < NI;
#pragma unroll
            for (int kq = 0; kq < KO / 4; ++kq) w[it][kq] = cv ? W[col * KO + 4 * kq + gq] : 0.0f;
        }
    }
    // from the packed layout (pack_layer): one coalesced load per operand
    __device__ __forceinline__ void load_packed(const float* __restrict__ Wp, int tid) {
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int cb = wave + NW * it;
#pragma unroll
            for (int kq = 0; kq < KO / 4; ++kq) w[it][kq] = cb < NB ? Wp[(cb * (KO / 4) + kq) * 64 + lane] : 0.0f;
        }
    }
    __device__ __forceinline__ float operator()(int it, int kq, bool, int, int) const { return w[it][kq]; }
};
// part[m][n] = sum over the 16 rows of act[row][m] d[row][n], m < M (the last input row is the
// ones column: the bias gradient), n < N (one tile of rows: head_bwd_kernel<false>)
template <int M, int N, int NW, int LA, int LD>
__device__ __forceinline__ void head_wgrad(const float (*act)[LA], const float (*d)[LD], float* __restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, gq = lane >> 4;
    constexpr int MB = (M + 15) / 16, NB = (N + 15) / 16;
    for (int t = wave; t < MB * NB; t += NW) {
        const int m0 = 16 * (t / NB), n0 = 16 * (t % NB);
        const int mc = m0 + i < M ? m0 + i : M - 1, nc = n0 + i < N ? n0 + i : N - 1;
        rdg::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 4 * s + gq;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(act[k][mc], d[k][nc], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * gq + r, n = n0 + i;
            if (m < M && n < N) part[m * N + n] = acc[r];
        }
    }
}
// acc += sum over the 16 rows of act[row][m] d[row][n], m < M (the last input row is the ones
// column: the bias gradient), n < N: 16x16 output tiles t = wave, wave + 4, ...; the
// accumulators stay in registers over a workgroup's tiles of rows (head_bwd_kernel)
template <int M, int N, int NW = 4>
constexpr int wq() { return (((M + 15) / 16) * ((N + 15) / 16) + NW - 1) / NW; }
template <int M, int N, int NW = 4, int LA, int LD>
__device__ __forceinline__ void head_wgrad_acc(const float (*act)[LA], const float (*d)[LD],
                                               rdg::f32x4 (&acc)[wq<M, N, NW>()], int tid) {
    const int wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    constexpr int MB = (M + 15) / 16, NB = (N + 15) / 16;
#pragma unroll
    for (int q = 0; q < wq<M, N, NW>(); ++q) {
        const int t = wave + NW * q;
        if (t >= MB * NB) break;
        const int m0 = 16 * (t / NB), n0 = 16 * (t % NB);
        const int mc = m0 + i < M ? m0 + i : M - 1, nc = n0 + i < N ? n0 + i : N - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 4 * s + gq;
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(act[k][mc], d[k][nc], acc[q], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);   // one tile's LDS operands live at a time
    }
}
// part[m][n] = the accumulated tiles
template <int M, int N, int NW = 4>
__device__ __forceinline__ void head_wgrad_store(const rdg::f32x4 (&acc)[wq<M, N, NW>()], float* __restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, gq = lane >> 4;
    constexpr int MB = (M + 15) / 16, NB = (N + 15) / 16;
#pragma unroll
    for (int q = 0; q < wq<M, N, NW>(); ++q) {
        const int t = wave + NW * q;
        if (t >= MB * NB) break;
        const int m0 = 16 * (t / NB), n0 = 16 * (t % NB);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * gq + r, n = n0 + i;
            if (m < M && n < N) part[m * N + n] = acc[q][r];
        }
    }
}

// MT: tpb tiles per workgroup with the weight-gradient accumulators in registers over all of them
// (eight waves share them), for large batches; else one tile per workgroup, NWV waves: sixteen
// when the whole grid is one wave of workgroups (e.g. the reference's 20 windows: 20
// workgroups on 256 CUs, latency bound -- round 5), else four
template <bool MT, int NWV>
__global__ __launch_bounds__(64 * NWV) void head_bwd_kernel(const float* __restrict__ Hc, const float* __restrict__ P0,
                                                       const float* __restrict__ A1, const float* __restrict__ A2,
                                                       const float* __restrict__ A3, const float* __restrict__ A4,
                                                       const float* __restrict__ dY, float* __restrict__ dHh,
                                                       float* __restrict__ part, int64_t B, int nb, int tpb,
                                                       const float* __restrict__ wpack) {
    __shared__ __attribute__((aligned(16))) float X0[HF_ROWS][U + 4];   // Hc, ones column U
    __shared__ __attribute__((aligned(16))) float X1[HF_ROWS][L1];
    __shared__ __attribute__((aligned(16))) float X2[HF_ROWS][L2];
    __shared__ __attribute__((aligned(16))) float X3[HF_ROWS][L3];
    __shared__ __attribute__((aligned(16))) float X4[HF_ROWS][L4];
    __shared__ __attribute__((aligned(16))) float D5[HF_ROWS][8];
    __shared__ __attribute__((aligned(16))) float D4[HF_ROWS][L4];
    __shared__ __attribute__((aligned(16))) float D3[HF_ROWS][L3];
    __shared__ __attribute__((aligned(16))) float D2[HF_ROWS][L2];
    __shared__ __attribute__((aligned(16))) float D1[HF_ROWS][L1];
    // workgroup (t, rb): rows t B + 16 tpb rb .. of step t, tpb tiles of 16 rows in turn; the
    // weight-gradient accumulators run over all of them and leave one partial row
    const int ts = blockIdx.x / nb, rb = blockIdx.x - ts * nb;
    const int64_t R = (int64_t)(ts + 1) * B;
    const float* P = P0 + OFF_H + (int64_t)ts * HSZ;
    float* pw = part + (int64_t)blockIdx.x * HB_PART;
    constexpr int NW = NWV, NT = 64 * NW;   // MT: eight waves share the accumulators
    static_assert(!MT || NW == 8, "the MT form runs eight waves");
    rdg::f32x4 a1[wq<U + 1, H1, NW>()], a2[wq<H1 + 1, H2, NW>()], a3[wq<H2 + 1, H3, NW>()],
        a4[wq<H3 + 1, H4, NW>()], a5[wq<H4 + 1, 4, NW>()];
#define RDL_ZERO(a) _Pragma("unroll") for (auto& x : a) x = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
    RDL_ZERO(a1) RDL_ZERO(a2) RDL_ZERO(a3) RDL_ZERO(a4) RDL_ZERO(a5)
#undef RDL_ZERO
    // MT: this lane's share of step ts's head weights held in registers over all the tiles
    HeadW<4, H4, NW> w5;
    HeadW<H4, H3, NW> w4;
    HeadW<H3, H2, NW> w3;
    HeadW<H2, H1, NW> w2;
    HeadW<H1, U, NW> w1;
    // RW: the weights held in registers -- MT (read once per workgroup over its tiles) and the
    // sixteen-wave form (one column block per wave: every layer's weights in one round trip at
    // entry, beside the row staging, instead of one round trip per layer)
    constexpr bool RW = MT || NW == 16;
    if (RW && wpack) {   // (uniform) the packed copy of this step's head weights
        const float* d = wpack + (int64_t)ts * HWP;
        w5.load_packed(d + HWP_5, threadIdx.x);
        w4.load_packed(d + HWP_4, threadIdx.x);
        w3.load_packed(d + HWP_3, threadIdx.x);
        w2.load_packed(d + HWP_2, threadIdx.x);
        w1.load_packed(d + HWP_1, threadIdx.x);
    } else if constexpr (RW) {
        w5.load(P + OFF_W5, threadIdx.x);
        w4.load(P + OFF_W4, threadIdx.x);
        w3.load(P + OFF_W3, threadIdx.x);
        w2.load(P + OFF_W2, threadIdx.x);
        w1.load(P + OFF_W1, threadIdx.x);
    }
    for (int k = 0; k < (MT ? tpb : 1); ++k) {
        const int64_t row0 = (int64_t)ts * B + ((int64_t)rb * tpb + k) * HF_ROWS;
        if (row0 >= R) break;   // workgroup-uniform
        // loop-invariant weights and lane indices: opaque copies keep their loads and address
        // arithmetic inside the loop (hoisted, every layer's operands and addresses would be live
        // at once and spill)
        const float* Pk = P;
        int tid = threadIdx.x;
        if constexpr (MT) asm volatile("" : "+s"(Pk), "+v"(tid));
        // rows past R (the step's last row) are zero (activations and gradients): they add nothing
        head_stage<U, U + 4, NT>(Hc, U, row0, R, X0, tid);
        head_stage<H1 + 1, L1, NT>(A1, L1, row0, R, X1, tid);   // with the ones column
        head_stage<H2 + 1, L2, NT>(A2, L2, row0, R, X2, tid);
        head_stage<H3 + 1, L3, NT>(A3, L3, row0, R, X3, tid);
        head_stage<H4 + 1, L4, NT>(A4, L4, row0, R, X4, tid);
        head_stage<4, 8, NT>(dY, 4, row0, R, D5, tid);
        if (tid < HF_ROWS) X0[tid][U] = row0 + tid < R ? 1.0f : 0.0f;
        __syncthreads();
        if constexpr (RW) {
            head_dgrad_f<4, H4, true, NW>(D5, D4, X4, w5, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad_f<H4, H3, true, NW>(D4, D3, X3, w4, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad_f<H3, H2, true, NW>(D3, D2, X2, w3, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad_f<H2, H1, true, NW>(D2, D1, X1, w2, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad_f<H1, U, false, NW>(D1, (float(*)[U + 4]) nullptr, X0, w1, dHh, U, row0, R, tid);   // dh_head
        } else {
            head_dgrad<4, H4, true, NW>(D5, D4, X4, Pk + OFF_W5, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad<H4, H3, true, NW>(D4, D3, X3, Pk + OFF_W4, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad<H3, H2, true, NW>(D3, D2, X2, Pk + OFF_W3, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad<H2, H1, true, NW>(D2, D1, X1, Pk + OFF_W2, nullptr, 0, row0, R, tid);
            __syncthreads();
            head_dgrad<H1, U, false, NW>(D1, (float(*)[U + 4]) nullptr, X0, Pk + OFF_W1, dHh, U, row0, R, tid);
        }
        if constexpr (MT) {   // [dW1; db1] .. [dW5; db5] accumulated over the tiles
            head_wgrad_acc<U + 1, H1, NW>(X0, D1, a1, tid);
            head_wgrad_acc<H1 + 1, H2, NW>(X1, D2, a2, tid);
            head_wgrad_acc<H2 + 1, H3, NW>(X2, D3, a3, tid);
            head_wgrad_acc<H3 + 1, H4, NW>(X3, D4, a4, tid);
            head_wgrad_acc<H4 + 1, 4, NW>(X4, D5, a5, tid);
            __syncthreads();   // the next tile restages the LDS rows
        } else {              // one tile: each layer's partial stored at once
            head_wgrad<U + 1, H1, NW>(X0, D1, pw);
            head_wgrad<H1 + 1, H2, NW>(X1, D2, pw + (OFF_W2 - OFF_W1));
            head_wgrad<H2 + 1, H3, NW>(X2, D3, pw + (OFF_W3 - OFF_W1));
            head_wgrad<H3 + 1, H4, NW>(X3, D4, pw + (OFF_W4 - OFF_W1));
            head_wgrad<H4 + 1, 4, NW>(X4, D5, pw + (OFF_W5 - OFF_W1));
        }
    }
    if constexpr (MT) {
        head_wgrad_store<U + 1, H1, NW>(a1, pw);
        head_wgrad_store<H1 + 1, H2, NW>(a2, pw + (OFF_W2 - OFF_W1));
        head_wgrad_store<H2 + 1, H3, NW>(a3, pw + (OFF_W3 - OFF_W1));
        head_wgrad_store<H3 + 1, H4, NW>(a4, pw + (OFF_W4 - OFF_W1));
        head_wgrad_store<H4 + 1, 4, NW>(a5, pw + (OFF_W5 - OFF_W1));
    }
}

// One launch for the gradient's last pieces (small batches, after BPTT): blocks < T HB_BLK run
// head_wgrad_reduce_kernel's sums, the next 160 (dense) dense32_grad_kernel's dot products.
constexpr int HB_BLK = (HB_PART + 255) / 256;
__device__ __forceinline__ void head_part_sum(const float* __restrict__ part, int nb, float* __restrict__ g, int t, int p) {
    if (p >= HB_PART) return;
    const float* q = part + (int64_t)t * nb * HB_PART + p;
    float a = 0.f, b = 0.f;
    int w = 0;
    for (; w + 1 < nb; w += 2) {
        a += q[(int64_t)w * HB_PART];
        b += q[(int64_t)(w + 1) * HB_PART];
    }
    if (w < nb) a += q[(int64_t)w * HB_PART];
    g[OFF_H + (int64_t)t * HSZ + p] = a + b;
}
// dWp = Q . Wl[11:43]^T and dbp = Wl[11:43] . dbl: the input-side dense32 layer's gradients
// (student_nn.py:26) from the BPTT kernel's gate sums, without materialising dP = dZ . Wl^T
// (the same sums in another order: sum over the rows first, then over the 800 gate columns)
__device__ __forceinline__ void dense32_dot(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ g,
                                            int o) {
    // o: 0..127 dWp[a][c] (a = o / 32), 128..159 dbp[c]; a fixed-order tree over 256 threads
    __shared__ float red[256];
    const int c = o & 31;
    const float* w = P + OFF_WL + (int64_t)(11 + c) * G4;
    const float* q = o < 128 ? Q + (o >> 5) * G4 : g + OFF_BL;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < (G4 + 255) / 256; ++j) {
        const int k = threadIdx.x + 256 * j;
        if (k < G4) v = fmaf(w[k], q[k], v);
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) g[(o < 128 ? OFF_WP : OFF_BP - 128) + o] = red[0];
}
// The last block: the metrics of the step from head_fwd_kernel's loss partials (lpart, nl
// workgroups, summed in workgroup order) into the ring slot, and the step words' snapshot for
// the Adam kernel (loss_kernel's job on the other paths).
__global__ __launch_bounds__(256) void grad_finish_kernel(const float* __restrict__ part, int nb, int T,
                                                          const float* __restrict__ P, const float* __restrict__ Q,
                                                          float* __restrict__ g, const float* __restrict__ lpart, int nl,
                                                          float rows, uint32_t* ctl, float* hist, int hist_len) {
    const int b = blockIdx.x;
    if (b < T * HB_BLK) {
        head_part_sum(part, nb, g, b / HB_BLK, (b % HB_BLK) * 256 + threadIdx.x);
    } else if (b < T * HB_BLK + 160) {
        dense32_dot(P, Q, g, b - T * HB_BLK);   // (uniform per block)
    } else if (threadIdx.x == 0) {
        float a = 0.f, c = 0.f;
        for (int w = 0; w < nl; ++w) {
            a += lpart[2 * w];
            c += lpart[2 * w + 1];
        }
        float* h = hist + (int64_t)(ctl[0] % (uint32_t)hist_len) * N_MET;
        h[0] = a;
        h[1] = c;
        h[2] = rows;
        h[3] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) ctl[4 + k] = ctl[k];
    }
}

// head t's gradient (blockIdx.y = t): grad[OFF_H + t HSZ + p] = sum over step t's nb
// workgroups' partial rows, in row order
__global__ __launch_bounds__(256) void head_wgrad_reduce_kernel(const float* __restrict__ part, int nb,
                                                                float* __restrict__ g) {
    head_part_sum(part, nb, g, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void dense32_grad_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                           float* __restrict__ g) {
    dense32_dot(P, Q, g, blockIdx.x);
}
