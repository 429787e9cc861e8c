// distill.hip, part 3 of 5: the partials workspace (RED_*, ws_index: the rollout writes it) and
// its reduction with TF1 Adam -- ReduceArgs (with the ctl words), col_rows, col_finish, bump_ctl,
// reduce_adam_kernel.  Expects distill_layout.h, distill_forward.h (put, pack_param) and
// rd_device.h (the Adam update).
#pragma once

// ctl words: [0] env steps C (the episode clocks), [1] optimiser steps S (metrics ring),
// [2] beta1^S, [3] beta2^S (f32 bits); [4..7] the rollout's snapshot of [0..3], which this
// kernel reads so that block 0 may rewrite [0..3] without racing the other blocks (no
// atomics, no fences: stream order suffices); [8] hand-off timeout; [12] 1 if the last
// rollout stepped the envs.
struct ReduceArgs {
    const float* ws;
    int nblk;
    float* grad;       // [P]
    float* params;     // student params [P] (in the student net buffer)
    float* m;
    float* v;
    uint32_t* ctl;
    float* hist;       // [hist_len][4]
    int hist_len;
    int reduce, adam, accum;   // accum: grad (and the metrics slot) += this rollout's sums
    int bump_env, bump_opt;    // advance the env clock (after a reduce) / the optimiser step
    float lr, b1, b2, eps;
    float* simg;       // student LDS image, refreshed with every updated parameter
    int img_kind;      // IMG_F32 / IMG_SPLIT / IMG_BF16
    const uint32_t* xerr;   // bound exchange's failure word (xGMI) or null: nonzero = skip Adam
};

// The partials workspace is column-chunked: chunk c (params 32c .. 32c+31) holds the rows of
// every workgroup of the launch contiguously, [chunk][row][RED_COLS], one 128-B line per row,
// so one reduce block per chunk reads one contiguous run and the reduce spreads over 159
// blocks (with [row][P_PAD] rows a block needed 64 columns for 256-B segments: 80 blocks
// pulled c4's 5.2 MB of partials).  Bitwise the same sums (the row order per column depends
// on RED_ROWS only).  16-column chunks (317 blocks) make the rollout's stores half lines and
// cost it 5 us at c4 (profiles/r02_ws_chunked.txt).
constexpr int RED_COLS = 32;                        // params per reduce block = chunk width
constexpr int RED_ROWS = 16;                        // partial rows summed in parallel
constexpr int RED_BLOCK = RED_COLS * RED_ROWS;
constexpr int RED_GRID = (P_PAD + RED_COLS - 1) / RED_COLS;
constexpr int P_WS = RED_GRID * RED_COLS;           // workspace floats per partial row
__device__ __forceinline__ int64_t ws_index(int p, int row, int rows) {
    return ((int64_t)(p / RED_COLS) * rows + row) * RED_COLS + (p % RED_COLS);
}

// The per-column arithmetic of the reduction: RED_ROWS row-threads per parameter, each
// summing rows row, row + RED_ROWS, ... in four interleaved partial sums; the row-threads'
// sums are then added in a fixed order (deterministic).
__device__ __forceinline__ float col_rows(const float* ws, int nblk, int p, int row) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const float* w = ws + ws_index(p, 0, nblk);   // row b of column p at w[b * RED_COLS]
    int b = row;
#pragma unroll 4
    for (; b + 3 * RED_ROWS < nblk; b += 4 * RED_ROWS) {
        s0 += w[b * RED_COLS];
        s1 += w[(b + RED_ROWS) * RED_COLS];
        s2 += w[(b + 2 * RED_ROWS) * RED_COLS];
        s3 += w[(b + 3 * RED_ROWS) * RED_COLS];
    }
    for (; b < nblk; b += RED_ROWS) s0 += w[b * RED_COLS];
    return (s0 + s1) + (s2 + s3);
}

// parameter p: total of its row-threads' sums (part[r * stride], r < RED_ROWS), the gradient /
// metrics slot, then the TF1 ApplyAdam functor (training_ops.cc) and the image refresh
__device__ __forceinline__ void col_finish(const ReduceArgs& a, int p, const float* part, int stride, float m_p,
                                           float v_p, float w_p, uint32_t S, float b1p, float b2p) {
    float g;
    if (a.reduce) {
        float q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RED_ROWS; ++r) q[r & 3] += part[r * stride];
        g = (q[0] + q[1]) + (q[2] + q[3]);
        if (p < P_TOT) {
            if (a.accum) g += a.grad[p];
            put(a.grad + p, g);
        } else {
            float* h = a.hist + (int64_t)(S % (uint32_t)a.hist_len) * N_MET + (p - P_TOT);
            put(h, a.accum ? *h + g : g);
        }
    } else {
        g = p < P_TOT ? a.grad[p] : 0.f;
    }
    if (a.adam && p < P_TOT) {
        const float alpha = rd::adam_alpha(a.lr, b1p, b2p);
        float m = m_p, v = v_p;
        m = rd::adam_m(g, m, a.b1);
        v = rd::adam_v(g, v, a.b2);
        put(a.m + p, m);
        put(a.v + p, v);
        const float w = w_p - rd::adam_delta(m, v, alpha, a.eps);
        put(a.params + p, w);
        pack_param(a.simg, p, w, true, a.img_kind);
    }
}

__device__ __forceinline__ void bump_ctl(const ReduceArgs& a, uint32_t C, uint32_t S, float b1p, float b2p,
                                         uint32_t stepped) {
    if (a.bump_env) a.ctl[0] = C + stepped;   // env steps: only after a launch that stepped the envs
    if (a.bump_opt) {
        a.ctl[1] = S + 1u;                     // optimiser steps
        a.ctl[2] = __float_as_uint(b1p * a.b1);
        a.ctl[3] = __float_as_uint(b2p * a.b2);
    }
}

// Sum the rollout's per-workgroup partials (fixed order: deterministic), then TF1 Adam.
__global__ __launch_bounds__(RED_BLOCK) void reduce_adam_kernel(ReduceArgs a) {
    __shared__ float part[RED_ROWS][RED_COLS];
    if (a.adam && a.xerr && __hip_atomic_load(a.xerr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        // the gradient exchange before this update failed (reacher_comm.h): no replica applies
        // a partial sum; the step is reported by the host readers (ctl[13]) and rdd_step
        a.adam = 0;
        a.bump_opt = 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[13] = 1u;
    }
    const uint32_t C = a.ctl[4], S = a.ctl[5];
    const float b1p = __uint_as_float(a.ctl[6]), b2p = __uint_as_float(a.ctl[7]);
    const int col = threadIdx.x & (RED_COLS - 1), row = threadIdx.x / RED_COLS;
    const int p = blockIdx.x * RED_COLS + col;
    // the Adam operands are loaded first, so their round trip overlaps the partial sums
    float m_p = 0.f, v_p = 0.f, w_p = 0.f;
    if (a.adam && row == 0 && p < P_TOT) {
        m_p = a.m[p];
        v_p = a.v[p];
        w_p = a.params[p];
    }
    if (a.reduce) part[row][col] = p < P_PAD ? col_rows(a.ws, a.nblk, p, row) : 0.f;
    __syncthreads();
    if (row == 0 && p < P_PAD) col_finish(a, p, &part[0][col], RED_COLS, m_p, v_p, w_p, S, b1p, b2p);
    if (blockIdx.x == 0 && threadIdx.x == 0) bump_ctl(a, C, S, b1p, b2p, a.ctl[12]);
}
