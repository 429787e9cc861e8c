// student_lstm.hip's point-wise and reduction kernels around the GEMM paths: cell_bwd_kernel (the
// per-step BPTT's last cell; it stands here, not beside student_lstm_step.h's forward, so that the
// kernels keep their order in the object and with it their label numbers), loss_kernel,
// metrics_kernel, ones_column_kernel, colsum_kernel, the Adam update (AdamArgs, adam_param,
// adam_kernel) and init_ctl_kernel.  Included inside student_lstm.hip's anonymous namespace after
// student_lstm_head.h, whose packed image (hw_index, HWP) the Adam update writes; expects
// student_lstm_layout.h and rd_device.h.
#pragma once

// BPTT through one cell (dh = dh_head + dh_next; dc carried in place).  The fused backward
// runs this only for the last step; the others ride in the dh GEMM's epilogue
// (rdg::EPI_LSTM_BWD, the same arithmetic)
__global__ __launch_bounds__(256) void cell_bwd_kernel(const float* dh_head, const float* dh_next, int add_next,
                                                       const float* G, const float* c_t, const float* c_prev,
                                                       float* dc, float* dZ, int64_t B) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * U) return;
    const int64_t b = idx / U;
    const int u = (int)(idx % U);
    const float* g = G + b * G4;
    const float gi = g[u], gj = g[U + u], gf = g[2 * U + u], go = g[3 * U + u];
    const float dh = add_next ? dh_head[idx] + dh_next[idx] : dh_head[idx];
    const float tc = tanhf(c_t[idx]);
    const float dcv = fmaf(dh * go, fmaf(-tc, tc, 1.0f), dc[idx]);
    float* dz = dZ + b * G4;
    dz[u] = dcv * gj * gi * (1.0f - gi);
    dz[U + u] = dcv * gi * fmaf(-gj, gj, 1.0f);
    dz[2 * U + u] = dcv * c_prev[idx] * gf * (1.0f - gf);
    dz[3 * U + u] = dh * tc * go * (1.0f - go);
    dc[idx] = dcv * gf;
}

// loss (reference loss.py:3-13 / action-MSE) and dY; per-block partials (fixed-order tree)
__global__ __launch_bounds__(LOSS_BLOCK) void loss_kernel(const float* Y, const float* tgt, float* dY, int64_t R,
                                                          int loss, float inv_n, float* part, uint32_t* ctl, float* hist,
                                                          int hist_len) {
    __shared__ float sl[LOSS_BLOCK], ss[LOSS_BLOCK];
    const int64_t r = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    float lv = 0.f, sq = 0.f;
    if (r < R) {
        const float* o = Y + r * 4;
        const float* t = tgt + r * 4;
        const float e0 = o[0] - t[0], e1 = o[1] - t[1];
        sq = fmaf(e0, e0, e1 * e1);
        float d0, d1, d2 = 0.f, d3 = 0.f;
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
        float* d = dY + r * 4;
        d[0] = d0; d[1] = d1; d[2] = d2; d[3] = d3;
    }
    sl[threadIdx.x] = lv;
    ss[threadIdx.x] = sq;
    __syncthreads();
    for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sl[threadIdx.x] += sl[threadIdx.x + s];
            ss[threadIdx.x] += ss[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sl[0];
        part[2 * blockIdx.x + 1] = ss[0];
    }
    if (gridDim.x == 1 && hist) {   // one block: metrics_kernel's work here (one launch fewer)
        if (threadIdx.x == 0) {
            float* h = hist + (int64_t)(ctl[0] % (uint32_t)hist_len) * N_MET;
            h[0] = sl[0];
            h[1] = ss[0];
            h[2] = (float)R;
            h[3] = 0.f;
        }
        __syncthreads();   // ctl[0] is read before the snapshot below rewrites nothing it needs
        if (threadIdx.x < 4) ctl[4 + threadIdx.x] = ctl[threadIdx.x];
    }
}

// metrics of this rollout into the ring slot of the current optimiser step; snapshot of the
// step words for the Adam kernel (whose block 0 rewrites them)
__global__ void metrics_kernel(const float* part, int nblk, float rows, uint32_t* ctl, float* hist, int hist_len) {
    __shared__ float sl[256], ss[256];
    float a = 0.f, b = 0.f;
    for (int k = threadIdx.x; k < nblk; k += 256) {
        a += part[2 * k];
        b += part[2 * k + 1];
    }
    sl[threadIdx.x] = a;
    ss[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sl[threadIdx.x] += sl[threadIdx.x + s];
            ss[threadIdx.x] += ss[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* h = hist + (int64_t)(ctl[0] % (uint32_t)hist_len) * N_MET;
        h[0] = sl[0];
        h[1] = ss[0];
        h[2] = rows;
        h[3] = 0.f;
    }
    if (threadIdx.x < 4) ctl[4 + threadIdx.x] = ctl[threadIdx.x];
}

// deterministic column sums: out[c] (+ blockIdx.y * ld_out) = sum over rows [y*chunk, ...)
// column `col` of a [rows][ld] buffer = 1
__global__ __launch_bounds__(256) void ones_column_kernel(float* A, int64_t rows, int ld, int col) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < rows) A[r * ld + col] = 1.0f;
}

__global__ __launch_bounds__(256) void colsum_kernel(const float* src, int64_t M, int N, int64_t ld, int64_t chunk,
                                                     float* out, int64_t ld_out) {
    __shared__ float s[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(M, r0 + chunk);
    float a = 0.f, b = 0.f;
    if (c < N) {
        int64_t r = r0 + ph;
        for (; r + 4 < r1; r += 8) {   // two chains: loads of 2 rows in flight per step
            a += src[r * ld + c];
            b += src[(r + 4) * ld + c];
        }
        if (r < r1) a += src[r * ld + c];
    }
    s[ph][threadIdx.x & 63] = a + b;
    __syncthreads();
    if (ph == 0 && c < N) out[(int64_t)blockIdx.y * ld_out + c] = (s[0][threadIdx.x] + s[1][threadIdx.x]) +
                                                                 (s[2][threadIdx.x] + s[3][threadIdx.x]);
}

struct AdamArgs {
    const float* grad;
    float* params;
    float* wpack;   // the heads' weights in the head backward's operand order (hw_index)
    float* m;
    float* v;
    uint32_t* ctl;
    float lr, b1, b2, eps;
    int64_t n;   // parameters (params_of(T))
};

// TF1 ApplyAdam (lstm_train.py:73-79) of parameter p with gradient g; the heads' weights also
// into their packed copy
__device__ __forceinline__ void adam_param(const AdamArgs& a, int p, float g, float b1p, float b2p) {
    {
        const float alpha = rd::adam_alpha(a.lr, b1p, b2p);
        float m = a.m[p], v = a.v[p];
        m = rd::adam_m(g, m, a.b1);
        v = rd::adam_v(g, v, a.b2);
        a.m[p] = m;
        a.v[p] = v;
        const float w = a.params[p] - rd::adam_delta(m, v, alpha, a.eps);
        a.params[p] = w;
        if (p >= OFF_H) {
            const int q = p - OFF_H, ts = q / HSZ, x = hw_index(q - ts * HSZ);
            if (x >= 0) a.wpack[(int64_t)ts * HWP + x] = w;
        }
    }
}
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const uint32_t S = a.ctl[4];
    const float b1p = __uint_as_float(a.ctl[5]), b2p = __uint_as_float(a.ctl[6]);
    if (p < a.n) adam_param(a, p, a.grad[p], b1p, b2p);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctl[0] = S + 1u;
        a.ctl[1] = __float_as_uint(b1p * a.b1);
        a.ctl[2] = __float_as_uint(b2p * a.b2);
    }
}

__global__ void init_ctl_kernel(uint32_t* ctl, float b1, float b2) {
    if (threadIdx.x < 2) {
        const int o = 4 * threadIdx.x;
        ctl[o] = 0u; ctl[o + 1] = __float_as_uint(b1); ctl[o + 2] = __float_as_uint(b2); ctl[o + 3] = 0u;
    }
}
