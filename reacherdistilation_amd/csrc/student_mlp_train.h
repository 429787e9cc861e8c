// student_mlp.hip's forward and training kernel: SmArgs and student_mlp_kernel<TRAIN, ROWS, BF>,
// the five layers of a row block and, when training, the loss, the backward and the workgroup's
// partial gradient row.  Included inside student_mlp.hip's anonymous namespace after
// student_mlp_layers.h; expects rd_device.h (philox, u01, wave_sum).
#pragma once

struct SmArgs {
    const float* x;        // [n][16]
    const float* tgt;      // [n][4] teacher pdflat (training)
    float* out;            // [n][4] pdflat (forward)
    int64_t n;
    const float* img;      // weight image [IMG_ALL]: f32, then the bf16 images
    float* ws;             // [gridDim.x][WS_ROW] partials (training)
    uint32_t* ctl;
    int loss;
    float inv_n_global;
    float keep_prob;       // < 1: dropout on inputs 0..10 (training only)
    uint64_t seed;
    int64_t row_base;
};

template <bool TRAIN, int ROWS, bool BF>
__global__ __launch_bounds__(BLOCK) void student_mlp_kernel(SmArgs a) {
    using LY = Lay<ROWS>;
    constexpr int RB = LY::RB;
    __shared__ __attribute__((aligned(16))) float lds[LY::LDS_FLOATS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    if (TRAIN && blockIdx.x == 0 && tid < 4) a.ctl[4 + tid] = a.ctl[tid];   // snapshot for the Adam kernel
    const uint32_t step = TRAIN ? a.ctl[0] : 0u;   // optimiser step (dropout counter); only Adam writes it
    f32x4 G0[WG<0>::Q], G1[WG<1>::Q], G2[WG<2>::Q], G3[WG<3>::Q], G4[WG<4>::Q];
    auto zero = [](auto& G) {
#pragma unroll
        for (auto& v : G) v = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    zero(G0); zero(G1); zero(G2); zero(G3); zero(G4);
    float gb0 = 0.f, gb1 = 0.f, gb2 = 0.f, gb3 = 0.f, gb4 = 0.f;
    float lsum = 0.f, ssum = 0.f, nrows = 0.f;
    float* X0 = lds + LY::O_X0;
    float* X1 = lds + LY::O_X1;
    float* X2 = lds + LY::O_X2;
    float* X3 = lds + LY::O_X3;
    float* X4 = lds + LY::O_X4;
    float* D5 = lds + LY::O_D5;
    float* D4 = lds + LY::O_D4;
    float* DA = lds + LY::O_DA;
    const int64_t nblk = (a.n + ROWS - 1) / ROWS;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * ROWS;
        if (tid < ROWS * 4) {   // ROWS rows x 16 inputs as 16-B vectors
            const int r = tid >> 2, c = tid & 3;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row0 + r < a.n) v = *reinterpret_cast<const f32x4*>(a.x + (row0 + r) * RDM_IN + 4 * c);
            if (TRAIN && a.keep_prob < 1.0f && c < 3) {   // tf.nn.dropout on the observation
                const uint64_t grow = (uint64_t)(a.row_base + row0 + r);
                uint32_t w[4];
                rd::philox((uint32_t)grow, (uint32_t)(grow >> 32), step, (uint32_t)c, (uint32_t)a.seed,
                           (uint32_t)(a.seed >> 32), w);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * c + k < 11) v[k] = rd::u01(w[k]) < a.keep_prob ? v[k] / a.keep_prob : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) X0[r * S_X0 + pk(4 * c + k)] = v[k];
        }
        __syncthreads();
        fwd<BF, RB, 0, S_X0, S_X1>(X0, X1, a.img, wave, i, g);
        __syncthreads();
        fwd<BF, RB, 1, S_X1, S_X2>(X1, X2, a.img, wave, i, g);
        __syncthreads();
        fwd<BF, RB, 2, S_X2, S_X3>(X2, X3, a.img, wave, i, g);
        __syncthreads();
        fwd<BF, RB, 3, S_X3, S_X4>(X3, X4, a.img, wave, i, g);
        __syncthreads();
        fwd<BF, RB, 4, S_X4, S_D5>(X4, D5, a.img, wave, i, g);
        __syncthreads();
        if constexpr (!TRAIN) {
            // the next block's first write (X0) is ordered after this block's F0 by the barriers above
            if (tid < ROWS * RDM_OUT) {
                const int r = tid >> 2, c = tid & 3;
                if (row0 + r < a.n) a.out[(row0 + r) * RDM_OUT + c] = D5[r * S_D5 + pk(c)];
            }
            continue;
        } else {
            // loss (reference loss.py:3-13 / action-MSE) and dZ5 = dL/dpdflat, one row per thread
            if (tid < ROWS) {
                const int64_t row = row0 + tid;
                float* o = D5 + tid * S_D5;
                float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
                if (row < a.n) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(a.tgt + row * RDM_OUT);
                    const float e0 = o[pk(0)] - t[0], e1 = o[pk(1)] - t[1];
                    ssum = fmaf(e0, e0, fmaf(e1, e1, ssum));
                    nrows += 1.0f;
                    if (a.loss == RDM_LOSS_MSE) {
                        d0 = e0 * a.inv_n_global;
                        d1 = e1 * a.inv_n_global;
                        lsum = fmaf(0.5f * a.inv_n_global, fmaf(e0, e0, e1 * e1), lsum);
                    } else {
                        const float ivt0 = expf(-2.0f * t[2]), ivt1 = expf(-2.0f * t[3]);
                        const float vs0 = expf(2.0f * o[pk(2)]), vs1 = expf(2.0f * o[pk(3)]);
                        lsum += (t[2] - o[pk(2)]) + 0.5f * (vs0 + e0 * e0) * ivt0 - 0.5f;
                        lsum += (t[3] - o[pk(3)]) + 0.5f * (vs1 + e1 * e1) * ivt1 - 0.5f;
                        d0 = e0 * ivt0;
                        d1 = e1 * ivt1;
                        d2 = fmaf(vs0, ivt0, -1.0f);
                        d3 = fmaf(vs1, ivt1, -1.0f);
                    }
                }
                o[pk(0)] = d0; o[pk(1)] = d1; o[pk(2)] = d2; o[pk(3)] = d3;   // columns 4..15 are exactly 0
            }
            __syncthreads();
            // layer 4 (32 -> 4): dW4, db4, dZ4 = (dZ5 W4^T) * (1 - H4^2)
            wgrad<BF, ROWS, 4, S_X4, S_D5>(X4, D5, G4, wave, i, g);
            bgrad_layer<ROWS, 4, S_D5>(D5, gb4, tid);
            dgrad<BF, RB, 4, S_D5, S_X4, S_D4>(D5, X4, D4, a.img, wave, i, g);
            __syncthreads();
            // layer 3 (128 -> 32): dZ3 = dZ4 W3^T (H3 is linear)
            wgrad<BF, ROWS, 3, S_X3, S_D4>(X3, D4, G3, wave, i, g);
            bgrad_layer<ROWS, 3, S_D4>(D4, gb3, tid);
            dgrad<BF, RB, 3, S_D4, S_X3, S_DA>(D4, X3, DA, a.img, wave, i, g);
            __syncthreads();
            // layer 2 (128 -> 128): dZ2 = (dZ3 W2^T) * (1 - H2^2) into X3's buffer (H3 is dead)
            wgrad<BF, ROWS, 2, S_X2, S_DA>(X2, DA, G2, wave, i, g);
            bgrad_layer<ROWS, 2, S_DA>(DA, gb2, tid);
            dgrad<BF, RB, 2, S_DA, S_X2, S_X3>(DA, X2, X3, a.img, wave, i, g);
            __syncthreads();
            // layer 1 (24 -> 128): dZ1 = (dZ2 W1^T) * (1 - H1^2) into DA
            wgrad<BF, ROWS, 1, S_X1, S_X3>(X1, X3, G1, wave, i, g);
            bgrad_layer<ROWS, 1, S_X3>(X3, gb1, tid);
            dgrad<BF, RB, 1, S_X3, S_X1, S_DA>(X3, X1, DA, a.img, wave, i, g);
            __syncthreads();
            // layer 0 (16 -> 24)
            wgrad<BF, ROWS, 0, S_X0, S_DA>(X0, DA, G0, wave, i, g);
            bgrad_layer<ROWS, 0, S_DA>(DA, gb0, tid);
            __syncthreads();
        }
    }
    if constexpr (TRAIN) {
        float* ws = a.ws + (int64_t)blockIdx.x * WS_ROW;
        store_wgrad<0>(ws, G0, wave, i, g);
        store_wgrad<1>(ws, G1, wave, i, g);
        store_wgrad<2>(ws, G2, wave, i, g);
        store_wgrad<3>(ws, G3, wave, i, g);
        store_wgrad<4>(ws, G4, wave, i, g);
        if (tid < OUT[0]) wst(ws + GB[0] + tid, gb0);
        if (tid < OUT[1]) wst(ws + GB[1] + tid, gb1);
        if (tid < OUT[2]) wst(ws + GB[2] + tid, gb2);
        if (tid < OUT[3]) wst(ws + GB[3] + tid, gb3);
        if (tid < OUT[4]) wst(ws + GB[4] + tid, gb4);
        if (wave == 0) {
            lsum = wave_sum(lsum);
            ssum = wave_sum(ssum);
            nrows = wave_sum(nrows);
            if (lane == 0) {
                ws[GIMG + 0] = lsum;
                ws[GIMG + 1] = ssum;
                ws[GIMG + 2] = nrows;
                ws[GIMG + 3] = 0.f;
            }
        }
    }
}
