// student_lstm.hip's persistent recurrence: the PR_* / PB_* tiling, the sc1 buffer accesses and the
// data-tagged granules of the hand-off between workgroups, lstm_fwd_persist_kernel and
// lstm_bptt_persist_kernel.  Included inside student_lstm.hip's anonymous namespace after
// student_lstm_step.h, whose K split (LSTM_KH, RF_TK) and arithmetic it keeps; expects
// student_lstm_layout.h, rd_gemm.h and rd_physics.h.
#pragma once

// Small batches (B <= PR_ROWS windows, e.g. the reference's 20) are latency bound: ~10 us per
// recurrent step as separate launches whatever the work.  lstm_fwd_persist_kernel runs ALL T
// steps of the forward recurrence in one launch and lstm_bptt_persist_kernel all T steps of BPTT.
// Workgroup w owns units 4w..4w+3 (50 workgroups, round 5; 13 of 16 units before): its 16 gate
// columns c = 4 y + j (gate y, unit j), its slice of Wr held in REGISTERS as the MFMA B operands
// for the whole launch, its cell points (row, unit) one per thread.  Per step the critical path
// is the h hand-off, one short MFMA chain per wave and one cell evaluation per thread: at 13
// workgroups each SIMD issued 104 f32 MFMAs per step with LDS-fed operands (2.9 us) and a thread
// ran two cells (2.2 us), stamped in profiles/r05l_lstm_stamps.jsonl.  The forward's h travels
// as data-tagged granules, no grid barrier; BPTT keeps the write-through payload + agent-scope
// arrival counter form (its granule form measured slower at 13 workgroups, profiles/r05i_*).
// The forward's K sum is two chains, k < PR_KH and k >= PR_KH, added (lo + hi) -- the per-step
// kernel's order -- so G, c and h are bitwise those of the per-step launches.
constexpr int PR_ROWS = 32, PR_UNITS = 4, PR_GRID = U / PR_UNITS;   // 50 workgroups
constexpr int PR_COLS = 4 * PR_UNITS;   // 16 gate columns per workgroup: c = 4 y + j
constexpr int PR_KH = LSTM_KH;          // K split of the forward's gate sums (lstm_rec_fwd_kernel's)
constexpr int PR_KQ = PR_KH / 4, PR_KQ1 = (U - PR_KH) / 4;   // k steps of the two halves (28, 22: pad k >= U skipped)
constexpr uint32_t PR_SPIN_LIMIT = 1u << 22;
static_assert(U % PR_UNITS == 0 && PR_KH % RF_TK == 0 && PR_KQ1 <= PR_KQ, "persistent LSTM tiling");

// BPTT's hand-off between the workgroups of a persistent launch (cdna_hip_programming.md §6
// Guideline 16, the write-through form): the exchanged payload (partial dh) is stored with sc1
// buffer stores and drained (s_waitcnt vmcnt(0)) before the workgroup's arrival on an agent-scope
// counter, and EVERY load of it is an sc1 buffer load -- no L2 writeback or L1 invalidate fences
// (a release/acquire pair per step measured ~3.5 us).  All other data these kernels read was
// written before the launch.
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pr_rsrc(const float* base, int64_t floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)(floats * 4), 0x00020000);
}
__device__ __forceinline__ rdg::f32x4 pr_load4(__amdgpu_buffer_rsrc_t r, int64_t idx) {   // sc1
    return __builtin_bit_cast(rdg::f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(idx * 4), 0, 16));
}

// Data-tagged granules (cdna_hip_programming.md §6 Guideline 16, R2 / MI355X_MICROARCH.md
// "allgather"): each exchanged f32 travels as ONE naturally aligned 8-byte word {tag, value},
// written by one agent-scope (sc1) store and read by agent-scope loads; a consumer re-reads
// its granules until every tag is the one it waits for.  No payload drain, no arrival counter,
// no barrier poll per step: the data is the flag.  Tags = (generation << 12) | phase, the
// generation advanced on the device once per forward call (the forward's last workgroup, bar[3];
// a replayed graph advances it too), so a granule left by an earlier call never matches.  Two buffers by
// step parity: a workgroup overwrites parity p only after it read every other workgroup's
// granules of the step between, which those wrote only after reading parity p themselves.
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
__device__ __forceinline__ void gr_store(unsigned long long* p, uint32_t tag, float v) {
    __hip_atomic_store((gu64_t*)(p), ((unsigned long long)tag << 32) | __float_as_uint(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long gr_load(const unsigned long long* p) {
    return __hip_atomic_load((const gu64_t*)(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// phase = the unrolled step s + 1 <= T - 1 in its own 12 bits (persistent() admits T < PR_MAX_T),
// the generation in the 20 above: with an 8-bit phase, T >= 258 let step 257 of call g - 1 carry
// step 1's tag of call g
constexpr int PR_PHASE_BITS = 12;
constexpr int PR_MAX_T = 1 << PR_PHASE_BITS;
__device__ __forceinline__ uint32_t gr_tag(uint32_t gen, uint32_t phase) { return (gen << PR_PHASE_BITS) | phase; }

// bar: [0] the forward's finished-workgroup count, [1] the BPTT's barrier counter, [2] timeout
// flag, [3] granule generation.  The last forward workgroup to finish (every one has read the
// generation by then) resets [0] and [1] and advances [3], so the next call's tags are new.
// hx: h granules [2][PR_ROWS][U] (step parity).  state0: null (zero state) or [c | h] of
// [B][U] each; Cs/H rows of step 0 are written from it for the backward.  Wave (rb, kh): rows
// 16 rb.. x the 16 local columns over K half kh; thread t < 4 B: the cell point (row t / 4,
// unit u0 + t % 4).  The launch also forms the inputs (round 5: no inputs_kernel, no Zx GEMM
// launch): per step s the rows X_s = [dropout(ob) | prev . Wp + bp] (x_value: inputs_kernel's
// arithmetic; workgroup 0 stores them for the weight gradient) and the input half of the gates
// Zx_s = X_s Wl[0:43] + bl of the local columns (the Zx GEMM's MFMA k order and epilogue), so
// G, c and h stay bitwise those of the per-step path.  Zx of step s+1 is formed right after step
// s publishes h, while the granules travel.
constexpr int PR_XQ = (XI + 3) / 4;                    // Zx k steps (11; k = 43 is the zero column)
// FU: units per forward workgroup (FNCB column blocks of 16 gate columns each; grid U / FU).
// Measured at 20 windows (round 5): FU 2 / 4 / 8 (100 / 50 / 25 workgroups) forward 43.7 / 43.0 /
// 51.7 us -- fewer readers of the h granules do not pay for the longer MFMA chains
constexpr int FU = 4, FNCB = (FU + 3) / 4, PR_GRID_F = U / FU;
static_assert(U % FU == 0 && (FU % 4 == 0 || FU < 4) && FU * PR_ROWS <= 256, "forward tiling: a cell point per thread");
__global__ __launch_bounds__(256) void lstm_fwd_persist_kernel(const float* __restrict__ P, const float* __restrict__ ob,
                                                               const float* __restrict__ prev, float* __restrict__ X,
                                                               const float* __restrict__ state0, float* __restrict__ G,
                                                               float* __restrict__ Cs, float* __restrict__ H, int B,
                                                               int T, float keep_prob, uint64_t seed, int64_t row_base,
                                                               const uint32_t* __restrict__ ctl, uint32_t* bar,
                                                               unsigned long long* hx) {
    __shared__ __attribute__((aligned(16))) float Zp[2][PR_ROWS][16 * FNCB + 1];   // the K halves' sums [row][c]
    __shared__ __attribute__((aligned(16))) float Xs[PR_ROWS][XLD];               // X_s rows; zero past B
    __shared__ __attribute__((aligned(16))) float Zx[PR_ROWS][16 * FNCB + 1];     // Zx_s of the local columns
    __shared__ int fail_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    const int u0 = blockIdx.x * FU;
    const int rb = wave & 1, kh = wave >> 1;
    const int kq0 = kh ? PR_KQ : 0;
    const uint32_t gen = bar[3], step = ctl[0];
    const float* Wr = P + OFF_WL + XI * G4;
    if (tid == 0) fail_s = 0;
    // this lane's B operands over the launch: Wr[k][y U + u0 + 4 cb + j] of column i = 4 y + j of
    // block cb, and (block zcb = wave / 2 of the Zx product) Wl[k][..], k < 43, with its bias
    float bw[FNCB][PR_KQ], bx[PR_XQ];
#pragma unroll
    for (int cb = 0; cb < FNCB; ++cb) {
        const int64_t col = (int64_t)(i >> 2) * U + u0 + 4 * cb + (i & 3);
#pragma unroll
        for (int q = 0; q < PR_KQ; ++q) {
            const int k = 4 * (kq0 + q) + gq;
            bw[cb][q] = (q < PR_KQ1 || kh == 0) ? Wr[(int64_t)k * G4 + col] : 0.0f;
        }
    }
    const int zcb = wave >> 1;   // Zx: waves (rb, zcb) for zcb < FNCB
    const int64_t zcol = (int64_t)(i >> 2) * U + u0 + 4 * (zcb < FNCB ? zcb : 0) + (i & 3);
#pragma unroll
    for (int q = 0; q < PR_XQ; ++q) {
        const int k = 4 * q + gq;
        bx[q] = (zcb < FNCB && k < XI) ? P[OFF_WL + (int64_t)k * G4 + zcol] : 0.0f;
    }
    const float bias = P[OFF_BL + zcol];
    // this thread's column of the dense32 part of X (c = 11 + tid % 32 for every row it forms)
    const int dc = tid & 31;
    float wp[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) wp[a] = P[OFF_WP + a * 32 + dc];
    const float bpc = P[OFF_BP + dc];
    for (int x = tid; x < PR_ROWS * XLD; x += 256) (&Xs[0][0])[x] = 0.0f;
    const bool pt = tid < FU * B;
    const int pr = tid / FU, pj = tid % FU, pu = u0 + pj;
    const int pc = 16 * (pj >> 2) + (pj & 3);   // the point's local column of gate 0 (+ 4 y)
    float cst = 0.0f;
    if (pt) {
        const int64_t idx = (int64_t)pr * U + pu;
        const float c0 = state0 ? state0[idx] : 0.0f, h0 = state0 ? state0[(int64_t)B * U + idx] : 0.0f;
        cst = c0;
        Cs[idx] = c0;   // rows of step 0, read by the backward
        H[idx] = h0;
    }
    // X_s -> Xs (and X, workgroup 0): x_value's arithmetic with one Philox draw per (row, 4
    // columns) of the dropout part and the dense32 part's weights held in registers; then
    // Zx_s = Xs Wl[0:43] + bl on waves 0, 1 -> Zx
    auto inputs = [&](int s) {
        for (int x = tid; x < 3 * B; x += 256) {   // dropout(ob) (student_nn.py:24): columns 4 q .. 4 q + 3 < 11
            const int r = x / 3, q = x - 3 * r;
            const int64_t rg = (int64_t)s * B + r;
            uint32_t o[4] = {0u, 0u, 0u, 0u};
            if (keep_prob < 1.0f) {
                const uint64_t w = (uint64_t)(row_base + r);
                rd::philox((uint32_t)w, (uint32_t)(w >> 32), step, (uint32_t)(4 * s + q), (uint32_t)seed,
                           (uint32_t)(seed >> 32), o);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * q + e;
                if (c < 11) {
                    float v = ob[rg * 11 + c];
                    if (keep_prob < 1.0f) v = rd::u01(o[e]) < keep_prob ? v / keep_prob : 0.0f;
                    Xs[r][c] = v;
                    if (blockIdx.x == 0) X[rg * XLD + c] = v;
                }
            }
        }
        for (int x = tid; x < 32 * B; x += 256) {   // prev . Wp + bp (student_nn.py:26)
            const int r = x >> 5;
            const int64_t rg = (int64_t)s * B + r;
            const float* pv = prev + rg * 4;
            float v = bpc;
#pragma unroll
            for (int a = 0; a < 4; ++a) v = fmaf(pv[a], wp[a], v);
            Xs[r][11 + dc] = v;
            if (blockIdx.x == 0) X[rg * XLD + 11 + dc] = v;
        }
        if (blockIdx.x == 0)
            for (int r = tid; r < B; r += 256) X[((int64_t)s * B + r) * XLD + XI] = 0.0f;
        __syncthreads();   // Xs complete; the previous step's cell has read Zx
        if (zcb < FNCB) {
            float av[PR_XQ];
#pragma unroll
            for (int q = 0; q < PR_XQ; ++q) av[q] = Xs[16 * rb + i][4 * q + gq];
            rdg::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
            fence_begin(acc);
#pragma unroll
            for (int q = 0; q < PR_XQ; ++q) acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bx[q], acc[0], 0, 0, 0);
            fence_end(acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) Zx[16 * rb + 4 * gq + r][16 * zcb + i] = acc[0][r] + bias;
        }
    };
    __syncthreads();   // Xs zeroed before the staging writes
    inputs(0);
    const int arow = 16 * rb + i;   // this lane's A-operand row (h_s row), k = 4 (kq0 + q) + gq
    const bool av_ok = arow < B;
    for (int s = 0; s < T; ++s) {
        // this wave's A operands: h_s[arow][k] over its K half, straight into registers -- each
        // wave gathers its own quadrant of the other workgroups' granules (re-read until every
        // tag matches) and starts its chain when they are in, no staging, no workgroup barrier
        float av[PR_KQ];
        if (s > 0) {
            const unsigned long long* src = hx + (int64_t)(s & 1) * PR_ROWS * U + (int64_t)(av_ok ? arow : 0) * U + 4 * kq0 + gq;
            const uint32_t want = gr_tag(gen, (uint32_t)s);
            for (uint32_t spins = 0;;) {
                unsigned long long v[PR_KQ];
#pragma unroll
                for (int q = 0; q < PR_KQ1; ++q) v[q] = av_ok ? gr_load(src + 4 * q) : (unsigned long long)want << 32;
                if (kh == 0) {
#pragma unroll
                    for (int q = PR_KQ1; q < PR_KQ; ++q) v[q] = av_ok ? gr_load(src + 4 * q) : (unsigned long long)want << 32;
                }
                bool ok = true;
#pragma unroll
                for (int q = 0; q < PR_KQ; ++q) ok &= (q < PR_KQ1 || kh == 0) ? (uint32_t)(v[q] >> 32) == want : true;
#pragma unroll
                for (int q = 0; q < PR_KQ; ++q) av[q] = (q < PR_KQ1 || kh == 0) ? __uint_as_float((uint32_t)v[q]) : 0.0f;
                if (__all(ok)) break;
                if (++spins > PR_SPIN_LIMIT) {
                    __hip_atomic_store(bar + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    fail_s = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        } else {
            const float* hs = state0 && av_ok ? state0 + (int64_t)B * U + (int64_t)arow * U + 4 * kq0 + gq : nullptr;
#pragma unroll
            for (int q = 0; q < PR_KQ; ++q) av[q] = hs && (q < PR_KQ1 || kh == 0) ? hs[4 * q] : 0.0f;
        }
        // this wave's K half: one accumulation chain per column block in k order (the per-step
        // kernel's lo / hi), the blocks' chains interleaved
        rdg::f32x4 acc[FNCB];
#pragma unroll
        for (int cb = 0; cb < FNCB; ++cb) acc[cb] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
        fence_begin(acc);
#pragma unroll
        for (int q = 0; q < PR_KQ1; ++q) {
#pragma unroll
            for (int cb = 0; cb < FNCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bw[cb][q], acc[cb], 0, 0, 0);
        }
        if (kh == 0) {
#pragma unroll
            for (int q = PR_KQ1; q < PR_KQ; ++q) {
#pragma unroll
                for (int cb = 0; cb < FNCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bw[cb][q], acc[cb], 0, 0, 0);
            }
        }
        fence_end(acc);
#pragma unroll
        for (int cb = 0; cb < FNCB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) Zp[kh][16 * rb + 4 * gq + r][16 * cb + i] = acc[cb][r];   // C: rows 4 gq + r, column i
        __syncthreads();
        if (fail_s) break;   // (uniform) a peer's granules never arrived: the timeout flag is raised
        // TF1 LSTMCell (lstm_rec_fwd_kernel's arithmetic) at this thread's point
        if (pt) {
            float z[4];
#pragma unroll
            for (int y = 0; y < 4; ++y) z[y] = ((Zp[0][pr][pc + 4 * y] + Zp[1][pr][pc + 4 * y]) + 0.0f) + Zx[pr][pc + 4 * y];
            const float gi = sigm(z[0]), gj = tanhf(z[1]), gf = sigm(z[2] + 1.0f), go = sigm(z[3]);
            const float c = fmaf(gf, cst, gi * gj);
            cst = c;
            const float h = go * tanhf(c);
            if (s + 1 < T) gr_store(hx + (int64_t)((s + 1) & 1) * PR_ROWS * U + (int64_t)pr * U + pu, gr_tag(gen, (uint32_t)(s + 1)), h);
            const int64_t row_g = (int64_t)s * B + pr;
            float* g = G + row_g * G4 + pu;
            g[0] = gi; g[U] = gj; g[2 * U] = gf; g[3 * U] = go;
            Cs[(row_g + B) * U + pu] = c;
            H[(row_g + B) * U + pu] = h;   // for the backward (a later launch)
        }
        if (s + 1 < T) inputs(s + 1);
    }
    // the last workgroup to finish advances the generation (every workgroup read it at entry)
    __syncthreads();
    if (tid == 0) {
        const uint32_t done = __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done + 1 == gridDim.x) {
            __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(bar + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(bar + 3, gen + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// BPTT of all T steps, split-K over the workgroups: per step s (T-1 .. 0) workgroup w
//  (1) sums dh_next at its points from the 50 partials of step s+1 (fixed order, sc1 loads),
//  (2) runs the cell backward at its points -> dz_s of its 16 gate columns (to LDS),
//  (3) multiplies those 16 columns by its 16 rows of Wr^T: a partial dh_{s-1} for ALL units,
//      stored sc1 to its slot of a per-step-parity partial buffer, arrives at the grid barrier,
//  (4) while the other workgroups arrive: its 16 columns of dWl += [x_s | h_{s-1}]^T dz_s (the
//      LSTM kernel's weight gradient, 243 x 16 per workgroup, accumulated in registers over the
//      steps: no dz round trip through HBM and no weight-gradient launch, round 5).
constexpr int PB_N = 208;    // units, padded: 13 column blocks of 16
constexpr int PB_PART = PB_N * PR_ROWS;   // floats of one workgroup's partial [unit][row]
constexpr int PB_RED = 4 + 16;            // per point: the dbl sums (4 gates) and Q = prev^T dz (4 x 4)
__global__ __launch_bounds__(256) void lstm_bptt_persist_kernel(const float* __restrict__ Wr, const float* __restrict__ dHh,
                                                                const float* __restrict__ G, const float* __restrict__ Cs,
                                                                const float* __restrict__ X, const float* __restrict__ Hp,
                                                                float* __restrict__ dWl, float* __restrict__ part,
                                                                float* __restrict__ dbl, const float* __restrict__ prev,
                                                                float* __restrict__ Q, int B, int T, uint32_t* bar) {
    __shared__ __attribute__((aligned(16))) float Dz[PR_ROWS][PR_COLS + 1];          // dz_s [row][c]; zero past B
    __shared__ float red[PR_ROWS][PR_UNITS][PB_RED];
    __shared__ int ok_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    const int u0 = blockIdx.x * PR_UNITS;
    // (4)'s operands and sums: wave w owns dWl rows 16 (w + 4 q) .. +15 (q < 4) x the 16 local
    // columns; xa[q][rq] = A^T[k = 16 (w + 4 q) + i][r = 4 rq + gq], A = [x_s | h_{s-1}] rows of step s
    rdg::f32x4 accw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) accw[q] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
    float xa[4][PR_ROWS / 4];
    auto load_a = [&](int s) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 16 * (wave + 4 * q) + i;
#pragma unroll
            for (int rq = 0; rq < PR_ROWS / 4; ++rq) {
                const int r = 4 * rq + gq;
                const int64_t row = (int64_t)s * B + r;
                // branch-free: every lane loads (a lane without an entry from X[0]) and selects, so
                // the 32 loads stay in flight together (as branches, the no-SLP build waited
                // vmcnt(0) between them: BPTT 45 -> 56 us at 20 windows, profiles/r06e_*)
                const bool in = r < B && k < XI + U;
                const float* src = !in ? X : k < XI ? X + row * XLD + k : Hp + row * U + (k - XI);
                const float v = *src;
                xa[q][rq] = in ? v : 0.0f;
            }
        }
    };
    auto dwl_step = [&]() {   // dz_s is in Dz (rows >= B zero)
        float dv[PR_ROWS / 4];
#pragma unroll
        for (int rq = 0; rq < PR_ROWS / 4; ++rq) dv[rq] = Dz[4 * rq + gq][i];
        const int nrq = (B + 3) >> 2;
        fence_begin(accw);
#pragma unroll
        for (int rq = 0; rq < PR_ROWS / 4; ++rq) {
            if (rq < nrq) {
#pragma unroll
                for (int q = 0; q < 4; ++q) accw[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[q][rq], dv[rq], accw[q], 0, 0, 0);
            }
        }
        fence_end(accw);
    };
    const int rb = wave & 1, cbo = wave >> 1;   // rows 16 rb.., unit blocks cbo, cbo + 2, .. (7 or 6 of 13)
    const __amdgpu_buffer_rsrc_t rP = pr_rsrc(part, (int64_t)2 * PR_GRID * PB_PART);
    // this lane's B operands over the launch: B[k][n] = Wr[n][y U + u0 + j] at k = 4 y + j = 4 q4 + gq
    float bw[7][4];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int n = 16 * (cbo + 2 * q) + i;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) bw[q][q4] = n < U ? Wr[(int64_t)n * G4 + q4 * U + u0 + gq] : 0.0f;
    }
    for (int x = tid; x < PR_ROWS * (PR_COLS + 1); x += 256) (&Dz[0][0])[x] = 0.0f;
    const bool pt = tid < 4 * B;
    const int pr = tid >> 2, pj = tid & 3, pu = u0 + pj;
    float dcs = 0.f;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};   // dbl: this point's row, all steps, per gate
    float qsum[4][4] = {};                    // Q = prev^T dz: [prev component][gate]
    float cg[4], cct, ccp, cdh, cpv[4];
    auto load_cell = [&](int s) {   // gates, c_t, c_{t-1}, dh from the head: written before the launch
        // branch-free as load_a: a lane without a point loads row (s, 0) of its unit (valid) and
        // its values are never used (every use is under pt)
        const int64_t rs = (int64_t)s * B + (pt ? pr : 0);
        const float* g = G + rs * G4 + pu;
#pragma unroll
        for (int y = 0; y < 4; ++y) cg[y] = g[y * U];
        cct = Cs[(rs + B) * U + pu];
        ccp = Cs[rs * U + pu];
        cdh = dHh[rs * U + pu];
#pragma unroll
        for (int a = 0; a < 4; ++a) cpv[a] = prev[rs * 4 + a];
    };
    load_cell(T - 1);
    load_a(T - 1);
    __syncthreads();   // Dz zeroed
    uint32_t nsync = 0;
    for (int s = T - 1; s >= 0; --s) {
        float dhn = 0.f;
        if (s < T - 1 && pt) {   // (1) dh_next at the point: the 50 partials of step s+1, summed in workgroup order
            const int64_t pb = (int64_t)((s + 1) & 1) * PR_GRID * PB_PART + (int64_t)pu * PR_ROWS + pr;
            float v[PR_GRID];
#pragma unroll
            for (int w = 0; w < PR_GRID; ++w)
                v[w] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rP, (int)((pb + (int64_t)w * PB_PART) * 4), 0, 16));
            float acc = v[0];
#pragma unroll
            for (int w = 1; w < PR_GRID; ++w) acc += v[w];
            dhn = acc;
        }
        // (2) TF1 LSTMCell backward (cell_bwd_kernel's arithmetic)
        if (pt) {
            const float gi = cg[0], gj = cg[1], gf = cg[2], go = cg[3];
            const float dh = s < T - 1 ? cdh + dhn : cdh;
            const float tc = tanhf(cct);
            const float dcv = fmaf(dh * go, fmaf(-tc, tc, 1.0f), dcs);
            const float z0 = dcv * gj * gi * (1.0f - gi), z1 = dcv * gi * fmaf(-gj, gj, 1.0f);
            const float z2 = dcv * ccp * gf * (1.0f - gf), z3 = dh * tc * go * (1.0f - go);
            Dz[pr][pj] = z0; Dz[pr][4 + pj] = z1; Dz[pr][8 + pj] = z2; Dz[pr][12 + pj] = z3;
            bsum[0] += z0; bsum[1] += z1; bsum[2] += z2; bsum[3] += z3;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                qsum[a][0] = fmaf(cpv[a], z0, qsum[a][0]);
                qsum[a][1] = fmaf(cpv[a], z1, qsum[a][1]);
                qsum[a][2] = fmaf(cpv[a], z2, qsum[a][2]);
                qsum[a][3] = fmaf(cpv[a], z3, qsum[a][3]);
            }
            dcs = dcv * gf;
        }
        if (s == 0) break;
        load_cell(s - 1);
        __syncthreads();
        // (3) partial dh_{s-1}[row][n] over the 16 local columns, for every unit n
        rdg::f32x4 acc[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) acc[q] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
        {
            float av[4];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) av[q4] = Dz[16 * rb + i][4 * q4 + gq];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
                for (int q = 0; q < 6; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q4], bw[q][q4], acc[q], 0, 0, 0);
                if (cbo == 0) acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q4], bw[6][q4], acc[6], 0, 0, 0);
            }
        }
        const int64_t po = (int64_t)(s & 1) * PR_GRID * PB_PART + (int64_t)blockIdx.x * PB_PART;
#pragma unroll
        for (int q = 0; q < 7; ++q) {   // lane (i, gq): rows 16 rb + 4 gq .. +3 of unit 16 (cbo + 2 q) + i
            if (q < 6 || cbo == 0)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[q]), rP,
                                                       (int)((po + (int64_t)(16 * (cbo + 2 * q) + i) * PR_ROWS + 16 * rb + 4 * gq) * 4),
                                                       0, 16);
        }
        // (4) while the sc1 partial stores drain, then arrive (every wave's stores landed first)
        dwl_step();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        load_a(s - 1);
        if (tid == 0) {
            const uint32_t target = ++nsync * gridDim.x;
            int ok = 1;
            for (uint32_t spins = 0; __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target;) {
                if (++spins > PR_SPIN_LIMIT) {
                    __hip_atomic_store(bar + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            ok_s = ok;
        }
        __syncthreads();   // Dz is rewritten by the next step
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // keeps the payload loads below the poll
        if (!ok_s) return;
    }
    __syncthreads();   // dz_0 in Dz
    dwl_step();
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // C: rows k = 16 (w + 4 q) + 4 gq + r, local column i
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * (wave + 4 * q) + 4 * gq + r;
            if (k < XI + U) dWl[(int64_t)k * G4 + (i >> 2) * U + u0 + (i & 3)] = accw[q][r];
        }
    }
    // dbl (the gate bias gradient) and Q = prev^T dz of the local columns: the points' sums, in row order
    __syncthreads();
    if (pt) {
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            red[pr][pj][y] = bsum[y];
#pragma unroll
            for (int a = 0; a < 4; ++a) red[pr][pj][4 + 4 * a + y] = qsum[a][y];
        }
    }
    __syncthreads();
    for (int o = tid; o < PR_UNITS * PB_RED; o += 256) {
        const int jj = o / PB_RED, e = o - jj * PB_RED, uu = u0 + jj;
        float v = 0.f;
        for (int r = 0; r < B; ++r) v += red[r][jj][e];
        if (e < 4) dbl[e * U + uu] = v;
        else Q[((e - 4) >> 2) * G4 + ((e - 4) & 3) * U + uu] = v;
    }
}
