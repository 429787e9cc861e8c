// student_lstm.hip's persistent envs (rdl_envs_*, rdl_rollout_envs, rdl_step_envs,
// include/reacher_student_lstm.h): one launch takes the handle's n lockstep envs through K env steps
// under the teacher's or the LSTM student's mean action, writes the K n records and the training
// windows that lie wholly inside an episode, which the training path (rdl_rollout's launches) then
// reads as any caller's windows (DESIGN.md §3 "On-policy distillation of the LSTM student").
// Included inside student_lstm.hip's anonymous namespace after student_lstm_eval.h: tch::, the EV_*
// tiling, lstm_eval_pack_kernel's image and head_layer are its.
//
// It is student_lstm_evaluate_kernel with the envs kept between launches.  A workgroup (8 waves) owns
// a block of 16 envs for the launch; at entry it loads from the handle's device arrays, and at exit
// writes back,
//  * the physics state, the reward the last step returned, the clock (step 0..49, episode) and the
//    teacher's last pdflat (lanes 0..15 of wave 0: registers between),
//  * the query state (c, h) (LDS between),
//  * the RAW fields of the ring's T records, ob[11] | prev[4]: they live in the x rows' LDS ring
//    itself, ob in columns 0..10 (the x row's own) and prev in the spare columns 48..51 (the A
//    operands read columns 0..47 only).
// The x rows' dense part (prev . Wp + bp, columns 11..42) is NOT carried: the parameters change
// between calls (an optimiser step, rdl_set_params), so every call re-forms it from the raw prev with
// the Wp, bp it reads, as the stepwise loop forms every window's X at every query (inputs_kernel's
// arithmetic: bias first, then four fmaf).
// STUDENT_ACTS = false (the driver's warm-up: the teacher steps the envs): no cell, no head, (c, h)
// neither read nor written, s_pdflat and stepped_with written as 0; the ring's raw fields are kept
// all the same, for the windows and for a later student call.
// After an env's step 49 it resets from Philox(seed, env_base + i, episode + 1), inside the step as
// rd_step does; the carried reward and (c, h) survive the reset.  The clock is the device's: no
// host-side count enters the arguments, and a captured launch replays the next steps.
// Windows: at an episode step s >= T-1 the query's window is the records s-T+1 .. s of one episode;
// the workgroup writes its 16 windows from the ring (ob, prev, and the records' own t_pdflat: prev of
// the next record, the teacher's output for the last) in the trainer's [T][B][.] layout, window
// index = (qualifying steps of the call so far) n + env, B = LsEnvsArgs::windows.
// Every env's chain depends on no other env and every operation is the stepwise forward's in its
// order, so the outputs are bitwise those of K x { rdd_forward (teacher), the window, rdl_forward,
// rd_step }, whatever the grid and the split of the steps over launches.
#pragma once

constexpr int EH_REC = 16;                    // a ring record in the handle's history: ob[11] | prev[4] | 0
constexpr int EH_PREV = 48;                   // the raw prev's columns of an LDS x row
constexpr int ENV_AUX = 1 + 4;                // per env, SoA rows: carried reward | the teacher's last pdflat[4]
static_assert(EH_PREV >= 4 * 4 * EV_GX && EH_PREV + 4 <= EV_XS && rd::kObsDim + 4 <= EH_REC, "ring layout");

struct LsEnvsArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;       // teacher net: params | ob mean | ob std
    const float* P;          // the student's flat parameters
    const float* img;        // lstm_eval_pack_kernel's image of Wl [EV_IMG]
    float* state;            // [8][n] SoA (rd_get_state's layout)
    float* aux;              // [ENV_AUX][n]
    int32_t* clock;          // [2][n]: step of the episode, episode
    float* q;                // [2][n][U] = (c, h)
    float* hist;             // [n][T][EH_REC], slot j % T = record j of the open episode
    float* records;          // [K][n][EV_REC]
    float* reward;           // [K][n] or null
    float* ob_w;             // [T][windows][11] or null (no windows written)
    float* prev_w;           // [T][windows][4]
    float* t_w;              // [T][windows][4]
    int64_t windows;         // B: the window buffers' stride and capacity
    int steps, T;            // K
};

// tch::load_net without its transposed half, restated for this kernel alone: that function is a plain
// __device__ one with a single caller in this translation unit, and further callers change how hipcc
// inlines it into student_lstm_evaluate_kernel, whose instruction text stays what it was.  Same
// stores in the same order: the image is load_net's.
__device__ __forceinline__ void envs_load_net(float* L, const float* g) {
    using namespace tch;
    constexpr int nthreads = EV_THREADS;
    const float* mu = g + P_TOT;
    const float* sd = g + P_TOT + OBD;
    for (int i = threadIdx.x; i < 12 * HID; i += nthreads) {
        const int k = i >> 6, f = i & 63;
        L[N_W1 + k * HID + (f & 15) * 4 + (f >> 4)] = kTanhScale * (k < OBD ? g[P_W1 + i] : g[P_B1 + f]);
    }
    for (int i = threadIdx.x; i < HID * HID; i += nthreads) {
        const int k = i >> 6, f = i & 63;
        L[N_W2 + k * HID + (f & 15) * 4 + (f >> 4)] = kTanhScale * g[P_W2 + i];
    }
    for (int i = threadIdx.x; i < HID; i += nthreads) L[N_B2 + i] = kTanhScale * g[P_B2 + i];
    for (int i = threadIdx.x; i < HID * ACD; i += nthreads) L[N_W3 + i] = g[P_W3 + i];
    if (threadIdx.x < ACD) {
        L[N_B3 + threadIdx.x] = g[P_B3 + threadIdx.x];
        L[N_LS + threadIdx.x] = g[P_LS + threadIdx.x];
    }
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;
        L[N_MU + k] = k < OBD ? mu[k] : 0.0f;
        L[N_RS + k] = k < OBD ? 1.0f / sd[k] : 1.0f;
    }
}

// episode 0 of every env; clock and aux to 0 (rd_reset's arithmetic); q and hist are memset by the host
__global__ __launch_bounds__(256) void student_lstm_envs_reset_kernel(LsEnvsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    float d[6];
    rd::philox_draw(a.seed, (uint64_t)(a.env_base + i), 0u, d);
    rd::State st;
    rd::env_reset(st, d);
    rd::store_state(a.state, a.n, i, st);
#pragma unroll
    for (int k = 0; k < ENV_AUX; ++k) a.aux[k * a.n + i] = 0.0f;
    a.clock[i] = 0;
    a.clock[a.n + i] = 0;
}

template <bool STUDENT_ACTS>
__global__ __launch_bounds__(EV_THREADS) void student_lstm_envs_kernel(LsEnvsArgs a) {
    __shared__ __attribute__((aligned(16))) float LT[tch::NET];                  // the teacher (load_net)
    __shared__ __attribute__((aligned(16))) float SO[EV_ROWS * tch::SOS];        // raw obs rows (component 11 = 1)
    __shared__ __attribute__((aligned(16))) float TO[2][EV_ROWS][4];             // the teacher's pdflat, by step parity
    __shared__ __attribute__((aligned(16))) float Xr[EV_MAX_T][EV_ROWS][EV_XS];  // x rows of records j, slot j % T; raw prev at EH_PREV
    __shared__ __attribute__((aligned(16))) float Xz[EV_XS];                     // the zero record's x row [0 | bp | 0]
    __shared__ __attribute__((aligned(16))) float Hb[2][EV_ROWS][EV_HS];         // h, read / written by position parity
    __shared__ __attribute__((aligned(16))) float Cst[EV_ROWS][EV_HS];           // c
    __shared__ __attribute__((aligned(16))) float X1[HF_ROWS][L1];
    __shared__ __attribute__((aligned(16))) float X2[HF_ROWS][L2];
    __shared__ __attribute__((aligned(16))) float X3[HF_ROWS][L3];
    __shared__ __attribute__((aligned(16))) float X4[HF_ROWS][L4];
    __shared__ __attribute__((aligned(16))) float X5[HF_ROWS][8];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // in an SGPR: the weight addresses are scalar + lane
    const int T = a.T;
    const float* P = a.P;
    const float* Ph0 = P + OFF_H + (int64_t)(T - 1) * HSZ;   // head T-1: the only one a query evaluates
    const rdg::f32x4* img4 = reinterpret_cast<const rdg::f32x4*>(a.img);
    envs_load_net(LT, a.tnet);   // published by the first block's barriers
    // this thread's point of the dense32 part of x: row tid / 32, column 11 + tid % 32
    const int dr = tid >> 5, dc = tid & 31;
    float wp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wp[q] = STUDENT_ACTS ? P[OFF_WP + q * 32 + dc] : 0.0f;
    const float bpc = STUDENT_ACTS ? P[OFF_BP + dc] : 0.0f;
    for (int x = tid; x < EV_MAX_T * EV_ROWS * EV_XS; x += EV_THREADS) (&Xr[0][0][0])[x] = 0.0f;
    if (tid < EV_XS) Xz[tid] = 0.0f;
    __syncthreads();
    if (STUDENT_ACTS && tid < 32) {   // inputs_kernel's arithmetic on a zero prev: bias first, then four fmaf
        float v = bpc;
#pragma unroll
        for (int q = 0; q < 4; ++q) v = fmaf(0.0f, wp[q], v);
        Xz[11 + tid] = v;
    }
    const bool phys = wave == 0 && lane < EV_ROWS;   // the env of this lane
    const bool win = a.ob_w != nullptr;
    const int64_t n = a.n, nblk = (n + EV_ROWS - 1) / EV_ROWS;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * EV_ROWS;
        const bool valid = phys && row0 + lane < n;
        const int64_t env = row0 + (valid ? lane : 0);   // a ragged block's spare lanes repeat its env 0
        __syncthreads();   // the previous block's last reads and its write-back
        int s = a.clock[row0];   // lockstep: one clock for the block
        if (STUDENT_ACTS) {
            for (int x = tid; x < EV_ROWS * U; x += EV_THREADS) {   // the carried query state
                const int r = x / U, u = x - r * U;
                const int64_t er = row0 + r < n ? row0 + r : row0;
                Cst[r][u] = a.q[er * U + u];
                Hb[0][r][u] = a.q[(n + er) * U + u];
            }
        }
        for (int x = tid; x < EV_ROWS * T * EH_REC; x += EV_THREADS) {   // the ring's raw fields
            const int r = x / (T * EH_REC), y = x - r * (T * EH_REC), slot = y / EH_REC, c = y - slot * EH_REC;
            const int64_t er = row0 + r < n ? row0 + r : row0;
            const float v = a.hist[(er * T + slot) * EH_REC + c];
            if (c < rd::kObsDim) Xr[slot][r][c] = v;
            else if (c < rd::kObsDim + 4) Xr[slot][r][EH_PREV + c - rd::kObsDim] = v;
        }
        int hp = 0;   // Hb[hp] holds the current h
        rd::State st;
        float carry = 0.0f;   // the reward this env's previous step returned
        float tp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int32_t episode = 0;
        if (phys) {
            rd::load_state(a.state, n, env, st);
            carry = a.aux[env];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                tp[c] = a.aux[(1 + c) * n + env];
                TO[(s + 1) & 1][lane][c] = tp[c];   // T_{s-1}: the next record's prev
            }
            episode = a.clock[n + env];
        }
        __syncthreads();
        if (STUDENT_ACTS) {   // the carried records' x rows, from their raw prev and THIS call's Wp, bp
            for (int slot = 0; slot < T; ++slot) {
                float v = bpc;
#pragma unroll
                for (int q = 0; q < 4; ++q) v = fmaf(Xr[slot][dr][EH_PREV + q], wp[q], v);
                Xr[slot][dr][11 + dc] = v;
            }
            __syncthreads();
        }
        int64_t wrow = row0;   // this block's first window of the current qualifying step
        for (int k = 0; k < a.steps; ++k) {
            const int slot = s % T;
            float* rec = valid ? a.records + ((int64_t)k * n + env) * EV_REC : nullptr;
            if (phys) {   // record s: ob_s | the carried reward; its raw fields into the ring
                float ob[rd::kObsDim];
                rd::observe<true>(st, ob);
#pragma unroll
                for (int c = 0; c < rd::kObsDim; ++c) {
                    SO[lane * tch::SOS + c] = ob[c];
                    Xr[slot][lane][c] = ob[c];
                }
                SO[lane * tch::SOS + tch::OBD] = 1.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) Xr[slot][lane][EH_PREV + c] = s ? TO[(s - 1) & 1][lane][c] : 0.0f;
                if (rec) {
#pragma unroll
                    for (int c = 0; c < rd::kObsDim; ++c) rec[c] = ob[c];
                    rec[rd::kObsDim] = carry;
                    rec[EV_REC - 1] = STUDENT_ACTS ? 1.0f : 0.0f;
                }
            }
            if (STUDENT_ACTS) {   // prev . Wp + bp of record s: prev = T_{s-1}, zero at s = 0
                float v = bpc;
#pragma unroll
                for (int q = 0; q < 4; ++q) v = fmaf(s ? TO[(s - 1) & 1][dr][q] : 0.0f, wp[q], v);
                Xr[slot][dr][11 + dc] = v;
            }
            __syncthreads();
            if (wave == EV_WAVES - 1) {   // T_s
                rd::f32x4 A1[4], A2[4];
                float m0, m1;
                tch::mlp_forward<true>(LT, SO, i, gq, A1, A2, m0, m1);
                if (gq == 0) {
                    float* o = TO[s & 1][i];
                    o[0] = m0; o[1] = m1; o[2] = LT[tch::N_LS]; o[3] = LT[tch::N_LS + 1];
                }
            }
            if constexpr (STUDENT_ACTS) {
                // the query: positions p = 0 .. T-1 hold records s - (T-1) + p, from the carried (c, h)
                // (student_lstm_evaluate_kernel's loop, kept instruction for instruction)
                for (int p = 0; p < T; ++p) {
                    const int j = s - (T - 1) + p;
                    const float* xrow = j < 0 ? Xz : &Xr[j % T][i][0];
                    const float* hrow = &Hb[hp][i][0];
                    for (int it = 0; it < (EV_UB + EV_WAVES - 1) / EV_WAVES; ++it) {
                        const int ub = wave + EV_WAVES * it;
                        if (ub >= EV_UB) break;   // (wave-uniform)
                        const int u = 16 * ub + i;
                        const bool uv = u < U;
                        uint32_t here = 0;   // (opaque: the image's 64 load addresses are formed where they are used)
                        asm volatile("" : "+s"(here));
                        const rdg::f32x4* wb = img4 + (int64_t)ub * (EV_G * 4 * 64) + here;
                        const uint32_t ln = (uint32_t)lane;
                        rdg::f32x4 b[EV_PF][4];
                        float av[EV_PF][4];
                        auto fetch = [&](int g) {
#pragma unroll
                            for (int y = 0; y < 4; ++y) b[g % EV_PF][y] = wb[(g * 4 + y) * 64 + ln];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int q = 4 * (g < EV_GX ? g : g - EV_GX) + e;
                                av[g % EV_PF][e] = g < EV_GX ? xrow[4 * q + gq] : 4 * q < U ? hrow[4 * q + gq] : 0.0f;
                            }
                        };
#pragma unroll
                        for (int g = 0; g < EV_PF; ++g) fetch(g);
                        float bias[4];
#pragma unroll
                        for (int y = 0; y < 4; ++y) bias[y] = uv ? P[OFF_BL + y * U + u] : 0.0f;
                        rdg::f32x4 zx[4], lo[4], hi[4];
#pragma unroll
                        for (int y = 0; y < 4; ++y) zx[y] = lo[y] = hi[y] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
                        // a group: four k steps of the four gates' chains, the loads of group g + EV_PF
                        // issued before its MFMAs start (SrcC fence)
                        auto group = [&](int g, rdg::f32x4 (&acc)[4]) {
                            rdg::f32x4 cur[4];
                            float ca[4];
#pragma unroll
                            for (int y = 0; y < 4; ++y) {
                                cur[y] = b[g % EV_PF][y];
                                ca[y] = av[g % EV_PF][y];
                            }
                            if (g + EV_PF < EV_G) fetch(g + EV_PF);
                            fence_begin(acc);
#pragma unroll
                            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                                for (int y = 0; y < 4; ++y)
                                    acc[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[kk], cur[y][kk], acc[y], 0, 0, 0);
                            fence_end(acc);
                        };
#pragma unroll
                        for (int g = 0; g < EV_G; ++g) {
                            if (g < EV_GX) group(g, zx);
                            else if (g < EV_GX + EV_GLO) group(g, lo);
                            else group(g, hi);
                        }
                        // TF1 LSTMCell at rows 4 gq + r of unit u (lstm_rec_fwd_kernel's epilogue)
                        if (uv) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 4 * gq + r;
                                float z[4];
#pragma unroll
                                for (int y = 0; y < 4; ++y) {
                                    const float zxv = zx[y][r] + bias[y];
                                    z[y] = ((lo[y][r] + hi[y][r]) + 0.0f) + zxv;
                                }
                                const float gi = sigm(z[0]), gj = tanhf(z[1]), gf = sigm(z[2] + 1.0f), go = sigm(z[3]);
                                const float c = fmaf(gf, Cst[row][u], gi * gj);
                                Cst[row][u] = c;
                                Hb[hp ^ 1][row][u] = go * tanhf(c);
                            }
                        }
                    }
                    hp ^= 1;
                    __syncthreads();
                }
            } else {
                __syncthreads();   // T_s
            }
            // the window of this query, if it lies inside the episode: records s-T+1 .. s from the ring
            // (T_s was published by the barriers above; the ring's next write follows the barriers below)
            if (win && s >= T - 1) {
                for (int x = tid; x < T * EV_ROWS * rd::kObsDim; x += EV_THREADS) {
                    const int p = x / (EV_ROWS * rd::kObsDim), y = x - p * (EV_ROWS * rd::kObsDim);
                    const int r = y / rd::kObsDim, c = y - r * rd::kObsDim;
                    const int64_t w = wrow + r;
                    if (row0 + r < n && w < a.windows)
                        a.ob_w[((int64_t)p * a.windows + w) * rd::kObsDim + c] = Xr[(s - (T - 1) + p) % T][r][c];
                }
                for (int x = tid; x < T * EV_ROWS * 4; x += EV_THREADS) {
                    const int p = x / (EV_ROWS * 4), r = (x >> 2) & (EV_ROWS - 1), c = x & 3;
                    const int j = s - (T - 1) + p;
                    const int64_t w = wrow + r;
                    if (row0 + r < n && w < a.windows) {
                        const int64_t o = ((int64_t)p * a.windows + w) * 4 + c;
                        a.prev_w[o] = Xr[j % T][r][EH_PREV + c];
                        a.t_w[o] = p < T - 1 ? Xr[(j + 1) % T][r][EH_PREV + c] : TO[s & 1][r][c];
                    }
                }
                wrow += n;
            }
            if constexpr (STUDENT_ACTS) {
                // head T-1 on the final h (head_fwd_kernel's layers; nothing stored to global: R = 0)
                const float (*X0)[EV_HS] = Hb[hp];
                uint32_t hoff = 0;   // (opaque, as the image's base: the layers' addresses are formed here)
                asm volatile("" : "+s"(hoff));
                const float* Ph = Ph0 + hoff;
                head_layer<U, H1, true, EV_WAVES>(X0, X1, Ph + OFF_W1, Ph + OFF_B1, nullptr, 0, 0, 0);
                head_layer<H1, H2, true, EV_WAVES>(X1, X2, Ph + OFF_W2, Ph + OFF_B2, nullptr, 0, 0, 0);
                head_layer<H2, H3, true, EV_WAVES>(X2, X3, Ph + OFF_W3, Ph + OFF_B3, nullptr, 0, 0, 0);
                head_layer<H3, H4, true, EV_WAVES>(X3, X4, Ph + OFF_W4, Ph + OFF_B4, nullptr, 0, 0, 0);
                head_layer<H4, 4, false, EV_WAVES>(X4, X5, Ph + OFF_W5, Ph + OFF_B5, nullptr, 0, 0, 0);
            }
            if (phys) {
                float sp[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sp[c] = STUDENT_ACTS ? X5[lane][c] : 0.0f;
                    tp[c] = TO[s & 1][lane][c];
                }
                if (rec) {
                    float* r = rec + rd::kObsDim + 1;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        r[c] = tp[c];
                        r[4 + c] = sp[c];
                    }
                }
                carry = STUDENT_ACTS ? rd::env_step<true>(st, sp[0], sp[1]) : rd::env_step<true>(st, tp[0], tp[1]);
                if (valid && a.reward) a.reward[(int64_t)k * n + env] = carry;
            }
            if (++s == rd::kEpisodeSteps) {   // TimeLimit: the env resets inside its last step
                s = 0;
                if (phys) {
                    float d[6];
                    ++episode;
                    rd::philox_draw(a.seed, (uint64_t)(a.env_base + env), (uint32_t)episode, d);
                    rd::env_reset(st, d);
                }
            }
            // the next step's first writes (SO, the ring's slot, TO's other parity) follow every read of
            // them: the head's barriers, or this one
            if constexpr (!STUDENT_ACTS) __syncthreads();
        }
        // write back: (c, h) after the call's last query, the ring's raw fields, the envs
        if (STUDENT_ACTS) {
            for (int x = tid; x < EV_ROWS * U; x += EV_THREADS) {
                const int r = x / U, u = x - r * U;
                if (row0 + r < n) {
                    a.q[(row0 + r) * U + u] = Cst[r][u];
                    a.q[(n + row0 + r) * U + u] = Hb[hp][r][u];
                }
            }
        }
        for (int x = tid; x < EV_ROWS * T * EH_REC; x += EV_THREADS) {
            const int r = x / (T * EH_REC), y = x - r * (T * EH_REC), slot = y / EH_REC, c = y - slot * EH_REC;
            if (row0 + r < n)
                a.hist[((row0 + r) * T + slot) * EH_REC + c] =
                    c < rd::kObsDim ? Xr[slot][r][c] : c < rd::kObsDim + 4 ? Xr[slot][r][EH_PREV + c - rd::kObsDim] : 0.0f;
        }
        if (valid) {
            rd::store_state(a.state, n, env, st);
            a.aux[env] = carry;
#pragma unroll
            for (int c = 0; c < 4; ++c) a.aux[(1 + c) * n + env] = tp[c];
            a.clock[env] = s;
            a.clock[n + env] = episode;
        }
    }
}
