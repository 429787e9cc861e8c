// student_lstm.hip's per-step forward (batches above PR_ROWS windows, RDL_KERNELS_STEP_RECURRENCE):
// inputs_kernel forms the x rows of all steps, cell_fwd_kernel states the TF1 cell, and
// lstm_rec_fwd_kernel (the RF_* tiling, the K split LSTM_KH) is one step's recurrent product with
// that cell in its epilogue.  The persistent forward (student_lstm_persist.h), the closed-loop step
// (student_lstm_query.h) and the bf16 step (student_lstm_bf16.h) restate this arithmetic and name
// these kernels.  The path's backward is rd_gemm.h's EPI_LSTM_BWD launches after cell_bwd_kernel,
// which stands in student_lstm_optim.h.  Included inside student_lstm.hip's anonymous namespace
// after student_lstm_layout.h; expects rd_gemm.h and rd_physics.h.
#pragma once

// X[r] =[dropout(ob[r]) (11) | prev[r] . Wp + bp (32) | 0]; r = t B + b (the persistent forward
// forms its steps' rows itself with the same arithmetic)
__global__ __launch_bounds__(256) void inputs_kernel(const float* ob, const float* prev, const float* params,
                                                     float* X, int64_t R, int64_t B, float keep_prob, uint64_t seed,
                                                     int64_t row_base, const uint32_t* ctl) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= R * XLD) return;
    const int64_t r = idx / XLD;
    const int col = (int)(idx % XLD);
    float v = 0.0f;
    if (col < 11) {
        v = ob[r * 11 + col];
        if (keep_prob < 1.0f) {   // tf.nn.dropout (student_nn.py:24)
            const int64_t t = r / B, b = r % B;
            const uint64_t w = (uint64_t)(row_base + b);
            uint32_t o[4];
            rd::philox((uint32_t)w, (uint32_t)(w >> 32), ctl[0], (uint32_t)(4 * t + col / 4), (uint32_t)seed,
                       (uint32_t)(seed >> 32), o);
            v = rd::u01(o[col & 3]) < keep_prob ? v / keep_prob : 0.0f;
        }
    } else if (col < XI) {        // hid_prev_pdflat = dense(prev_pdflat, 32) (student_nn.py:26)
        const int c = col - 11;
        const float* p = prev + r * 4;
        v = params[OFF_BP + c];
#pragma unroll
        for (int a = 0; a < 4; ++a) v = fmaf(p[a], params[OFF_WP + a * 32 + c], v);
    }
    X[idx] = v;
}

// TF1 LSTMCell: z = [i | j | f | o]; c = sig(f + 1) c_prev + sig(i) tanh(j); h = sig(o) tanh(c)
__global__ __launch_bounds__(256) void cell_fwd_kernel(const float* Z, const float* c_prev, float* G, float* c_out,
                                                       float* h_out, int64_t B) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * U) return;
    const int64_t b = idx / U;
    const int u = (int)(idx % U);
    const float* z = Z + b * G4;
    const float gi = sigm(z[u]), gj = tanhf(z[U + u]), gf = sigm(z[2 * U + u] + 1.0f), go = sigm(z[3 * U + u]);
    const float c = fmaf(gf, c_prev[idx], gi * gj);
    float* g = G + b * G4;
    g[u] = gi; g[U + u] = gj; g[2 * U + u] = gf; g[3 * U + u] = go;
    c_out[idx] = c;
    h_out[idx] = go * tanhf(c);
}

// One step of the forward recurrence with the cell in the epilogue (replaces the recurrent
// GEMM accumulating into Z + cell_fwd_kernel): a workgroup owns 64 rows x 16 units, i.e. the
// 64 gate columns {i, j, f, o} x those units of Wr, so at the end of the K loop every lane
// holds all four gate pre-activations of its (row, unit) outputs.  4 waves, wave w = rows
// 16w..16w+15 x the 4 gate blocks (one A and four B operands per k-step, 4 MFMAs).  The K sum
// runs as two chains, k < 112 and k >= 112, and the epilogue's z = ((lo + hi) + 0) + Zx: the
// persistent kernel's order (its waves split K there), so both give bitwise the same G, c and
// h.  Z_s keeps the input half (the backward reuses Z).
constexpr int RF_ROWS = 64, RF_UNITS = 16, RF_TK = 16, RF_LS = 64 + 16;
constexpr int LSTM_KH = 112;   // the recurrent K sum as two chains, k < 112 and k >= 112, added (lo + hi)
__global__ __launch_bounds__(256) void lstm_rec_fwd_kernel(const float* __restrict__ Hp, const float* __restrict__ Wr,
                                                           const float* __restrict__ Zx,
                                                           const float* __restrict__ cprev, float* __restrict__ Gs,
                                                           float* __restrict__ cs, float* __restrict__ hs,
                                                           int64_t B) {
    __shared__ __attribute__((aligned(16))) float As[2][RF_TK][RF_LS];   // [k][row]
    __shared__ __attribute__((aligned(16))) float Bs[2][RF_TK][RF_LS];   // [k][16 gate + unit]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * RF_ROWS;
    const int u0 = blockIdx.x * RF_UNITS;
    // staging: thread t loads 4 consecutive k of row m0 + t/4 (A) and 4 consecutive units of
    // gate (t%16)/4 at k row t/16 (B, one 16-B load from Wr's row)
    const int64_t am = m0 + (tid >> 2);
    const int ak = 4 * (tid & 3);
    const int bk = tid >> 4, bq = tid & 15, by = bq >> 2, bu = u0 + 4 * (bq & 3);
    auto load_a = [&](int k0) { return rdg::load4<true>(Hp + am * U + k0 + ak, am < B ? min(4, U - (k0 + ak)) : 0); };
    auto load_b = [&](int k0) {
        const int k = k0 + bk;
        return rdg::load4<true>(Wr + (int64_t)k * G4 + by * U + bu, k < U ? min(4, U - bu) : 0);
    };
    auto stage = [&](int buf, rdg::f32x4 a, rdg::f32x4 b) {
#pragma unroll
        for (int e = 0; e < 4; ++e) As[buf][ak + e][tid >> 2] = a[e];
        *reinterpret_cast<rdg::f32x4*>(&Bs[buf][bk][16 * by + 4 * (bq & 3)]) = b;
    };
    rdg::f32x4 lo[4], hi[4];   // the two K chains (the persistent kernel's waves kh = 0, 1)
#pragma unroll
    for (int y = 0; y < 4; ++y) lo[y] = hi[y] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
    auto tile = [&](int buf, rdg::f32x4 (&acc)[4]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kk = 4 * s + gq;
            const float a = As[buf][kk][16 * wave + i];
#pragma unroll
            for (int y = 0; y < 4; ++y)
                acc[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[buf][kk][16 * y + i], acc[y], 0, 0, 0);
        }
    };
    // load pipeline of rd_gemm.h: tile t+2's loads issue right after tile t+1 is staged, so
    // they stay in flight across the barrier and the next MFMA phase
    constexpr int NT = (U + RF_TK - 1) / RF_TK;
    static_assert(LSTM_KH % RF_TK == 0, "the K split falls on a tile boundary");
    stage(0, load_a(0), load_b(0));
    rdg::f32x4 na = load_a(RF_TK), nb = load_b(RF_TK);
    __syncthreads();
    for (int kt = 0; kt < NT; ++kt) {
        const int buf = kt & 1;
        if (kt < LSTM_KH / RF_TK) tile(buf, lo);
        else tile(buf, hi);
        if (kt + 1 < NT) {
            stage(buf ^ 1, na, nb);
            if (kt + 2 < NT) {
                na = load_a((kt + 2) * RF_TK);
                nb = load_b((kt + 2) * RF_TK);
            }
        }
        __syncthreads();
    }
    // epilogue: operands first, then TF1 LSTMCell (cell_fwd_kernel's arithmetic)
    const int u = u0 + i;
    float zx[4][4], cpv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + 16 * wave + 4 * gq + r;
        const bool ok = row < B && u < U;
#pragma unroll
        for (int y = 0; y < 4; ++y) zx[y][r] = ok ? Zx[row * G4 + y * U + u] : 0.0f;
        cpv[r] = ok ? cprev[row * U + u] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + 16 * wave + 4 * gq + r;
        if (row >= B || u >= U) continue;
        const float gi = sigm(((lo[0][r] + hi[0][r]) + 0.0f) + zx[0][r]), gj = tanhf(((lo[1][r] + hi[1][r]) + 0.0f) + zx[1][r]);
        const float gf = sigm(((lo[2][r] + hi[2][r]) + 0.0f) + zx[2][r] + 1.0f), go = sigm(((lo[3][r] + hi[3][r]) + 0.0f) + zx[3][r]);
        const float c = fmaf(gf, cpv[r], gi * gj);
        float* g = Gs + row * G4;
        g[u] = gi; g[U + u] = gj; g[2 * U + u] = gf; g[3 * U + u] = go;
        cs[row * U + u] = c;
        hs[row * U + u] = go * tanhf(c);
    }
}
