// One closed-loop step of the LSTM student on a block of 16 envs: what student_lstm_evaluate_kernel
// (student_lstm_eval.h) and student_lstm_envs_kernel (student_lstm_envs.h) both run, once.  Included
// inside student_lstm.hip's anonymous namespace after student_lstm_head.h (head_layer); expects
// rd_device.h, rd_gemm.h, rd_physics.h and student_lstm_layout.h's constants.
//
// A workgroup (8 waves, two per SIMD) owns a block of 16 envs -- one MFMA row tile:
//  * lanes 0..15 of wave 0 keep the envs (rd::observe<true>, rd::env_step<true>: rd_step's functions);
//  * wave 7 (one unit block of its own, below) runs the teacher, tch::mlp_forward<true> on the
//    load_net image (forward_kernel's, kept in LDS for the launch);
//  * the x rows of an episode's last T records (inputs_kernel's arithmetic) stay in an LDS ring, c
//    and h in LDS; a record before the episode's first is the zero row's x = [0 | bp];
//  * per window position the eight waves share the 13 blocks of 16 units (a SIMD's second wave
//    issues MFMAs while the first evaluates its cells: a block's 20 exp / tanh per lane cost about
//    as much issue time as its 256 MFMAs).  A wave forms the four gates of its block -- Zx (k < 43,
//    one chain, the Zx GEMM's order and epilogue) and the recurrent half as the two chains k < 112 /
//    k >= 112 of lstm_rec_fwd_kernel -- with the weights streamed from L2 out of an image packed once
//    per call (lstm_eval_pack_kernel: every B operand of a lane for four k steps is one 16-byte
//    load, a wave's load one contiguous KB), then the cell at its points (lstm_rec_fwd_kernel's
//    epilogue);
//  * head T-1 runs as head_fwd_kernel's five head_layer calls on the final h, over eight waves.
// The two kernels call these pieces in one order, with the barriers where the pieces say; their
// bitwise equality with the stepwise path, and with each other, rests on that.  ls_positions is the
// f32 query's; student_lstm_query_bf16.h holds its sibling on the bf16 cell (rdl_set_query_dtype),
// which a kernel instance selects by a template argument and which changes nothing else in a step.
#pragma once

#include "teacher_f32.h"   // namespace tch: the teacher's layouts, load_net and mlp_forward

constexpr int EV_ROWS = 16;                          // envs per workgroup: one MFMA row tile
constexpr int EV_MAX_T = RDL_EVAL_MAX_STEPS;         // the history ring's rows per env
constexpr int EV_REC = rd::kObsDim + 1 + 4 + 4 + 1;  // dataset.py's record: ob | reward | t_pdflat | s_pdflat | stepped_with
constexpr int EV_UB = (U + 15) / 16;                 // 13 blocks of 16 units (the last holds 8)
// k steps of a (unit block, gate) in groups of four: 3 of Zx (k < 43; the rest zero), 7 of the
// recurrent chain k < 112, 6 of the chain k >= 112 (k >= 200 zero)
constexpr int EV_GX = 3, EV_GLO = LSTM_KH / 16, EV_GHI = (U - LSTM_KH + 15) / 16, EV_G = EV_GX + EV_GLO + EV_GHI;
constexpr int EV_IMG = EV_UB * EV_G * 4 * 64 * 4;    // the packed image: [ub][group][gate][lane][4 k steps], 212,992 floats
constexpr int EV_WAVES = 8, EV_THREADS = 64 * EV_WAVES;
constexpr int EV_PF = 3;                             // groups of B operands in flight ahead of the MFMAs
constexpr int EV_XS = 52, EV_HS = U + 4;             // LDS row strides of x and h / c (64 distinct banks per A-operand read)
// An x row's columns: ob 0..10, prev . Wp + bp 11..42, zeros to 47 (the A operands read 0..47);
// 48..51 hold the record's RAW prev where a kernel carries the ring between launches (the envs')
constexpr int EH_PREV = 48;
static_assert(EV_MAX_T >= 16 && XI + 1 <= 4 * 4 * EV_GX && LSTM_KH % 16 == 0 && EV_G == 16 && tch::OBD == rd::kObsDim &&
              EH_PREV >= 4 * 4 * EV_GX && EH_PREV + 4 <= EV_XS && EV_ROWS == HF_ROWS && EV_THREADS == EV_ROWS * 32,
              "evaluation tiling");

// image[ub][g][y][lane = (gq, i)][e] = the weight of gate y, unit 16 ub + i at k = 4 (4 g' + e) + gq of
// its chain: Wl[k] (g < 3, k < 43), Wr[k] (k < 112), Wr[112 + k] (k < 88); zero past the matrix
__global__ __launch_bounds__(256) void lstm_eval_pack_kernel(const float* __restrict__ P, float* __restrict__ img) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= EV_IMG) return;
    const int e = x & 3, lane = (x >> 2) & 63, y = (x >> 8) & 3, g = (x >> 10) & 15, ub = x >> 14;
    const int i = lane & 15, gq = lane >> 4, u = 16 * ub + i;
    int row;   // of Wl [243][800], -1: zero
    if (g < EV_GX) {
        const int k = 4 * (4 * g + e) + gq;
        row = k < XI ? k : -1;
    } else if (g < EV_GX + EV_GLO) {
        row = XI + 4 * (4 * (g - EV_GX) + e) + gq;
    } else {
        const int k = LSTM_KH + 4 * (4 * (g - EV_GX - EV_GLO) + e) + gq;
        row = k < U ? XI + k : -1;
    }
    img[x] = row >= 0 && u < U ? P[OFF_WL + (int64_t)row * G4 + y * U + u] : 0.0f;
}

// The block's LDS, 131 KiB together: the two kernels' one set of arrays (a kernel instance is
// charged what it uses: the teacher-stepped envs none of the second group).  Separate arrays, not
// members of one object: the compiler then knows that a store to c does not touch h, and the cell's
// LDS traffic is scheduled as before.
namespace lds {
// what every step uses, whoever acts
__shared__ __attribute__((aligned(16))) float LT[tch::NET];                  // the teacher (load_net)
__shared__ __attribute__((aligned(16))) float SO[EV_ROWS * tch::SOS];        // raw obs rows (component 11 = 1)
__shared__ __attribute__((aligned(16))) float TO[2][EV_ROWS][4];             // the teacher's pdflat, by step parity
__shared__ __attribute__((aligned(16))) float Xr[EV_MAX_T][EV_ROWS][EV_XS];  // x rows of records j, slot j % T
__shared__ __attribute__((aligned(16))) float Xz[EV_XS];                     // the zero record's x row [0 | bp | 0]
// what only the student's query uses
__shared__ __attribute__((aligned(16))) float Hb[2][EV_ROWS][EV_HS];         // h, read / written by position parity
__shared__ __attribute__((aligned(16))) float Cst[EV_ROWS][EV_HS];           // c
__shared__ __attribute__((aligned(16))) float X1[HF_ROWS][L1];               // head T-1's layers
__shared__ __attribute__((aligned(16))) float X2[HF_ROWS][L2];
__shared__ __attribute__((aligned(16))) float X3[HF_ROWS][L3];
__shared__ __attribute__((aligned(16))) float X4[HF_ROWS][L4];
__shared__ __attribute__((aligned(16))) float X5[HF_ROWS][8];
}  // namespace lds

struct LsThread {   // a thread's constants of the launch
    int tid, lane, i, gq;
    int wave;                  // in an SGPR: the weight addresses are scalar + lane
    int dr, dc;                // its point of the dense32 part of x: row tid / 32, column 11 + tid % 32
    int T;
    const float* P;            // the student's flat parameters
    const float* Ph0;          // head T-1: the only one a query evaluates
    const rdg::f32x4* img4;    // lstm_eval_pack_kernel's image
    float wp[4], bpc;          // Wp's column dc and bp[dc] (zeros where no student runs)
};

// inputs_kernel's arithmetic at this thread's column of the dense32 part: bias first, then four fmaf
// over prev (has = false: the zero prev, the products still taken)
__device__ __forceinline__ float ls_dense(const LsThread& q, bool has, const float* prev) {
    float v = q.bpc;
#pragma unroll
    for (int k = 0; k < 4; ++k) v = fmaf(has ? prev[k] : 0.0f, q.wp[k], v);
    return v;
}

// The launch's prologue: the teacher image (published by the first step's barriers), this thread's
// Wp / bp, the ring zeroed, the zero record's x row.  Ends behind one barrier.
template <bool STUDENT = true>
__device__ __forceinline__ LsThread ls_prologue(const float* tnet, const float* P, const float* img, int T) {
    LsThread q;
    q.tid = threadIdx.x, q.lane = q.tid & 63, q.i = q.lane & 15, q.gq = q.lane >> 4;
    q.wave = __builtin_amdgcn_readfirstlane(q.tid >> 6);
    q.dr = q.tid >> 5, q.dc = q.tid & 31;
    q.T = T;
    q.P = P;
    q.Ph0 = P + OFF_H + (int64_t)(T - 1) * HSZ;
    q.img4 = reinterpret_cast<const rdg::f32x4*>(img);
    tch::load_net(lds::LT, tnet, false, EV_THREADS);
#pragma unroll
    for (int k = 0; k < 4; ++k) q.wp[k] = STUDENT ? P[OFF_WP + k * 32 + q.dc] : 0.0f;
    q.bpc = STUDENT ? P[OFF_BP + q.dc] : 0.0f;
    for (int x = q.tid; x < EV_MAX_T * EV_ROWS * EV_XS; x += EV_THREADS) (&lds::Xr[0][0][0])[x] = 0.0f;
    if (q.tid < EV_XS) lds::Xz[q.tid] = 0.0f;
    __syncthreads();
    if (STUDENT && q.tid < 32) lds::Xz[11 + q.tid] = ls_dense(q, false, nullptr);
    return q;
}

// The block's (c, h) from src = [2][n][U] (null: zeros) into Cst and Hb[0]; a ragged block's spare
// rows repeat its row 0
__device__ __forceinline__ void ls_state_load(int tid, const float* src, int64_t n, int64_t row0) {
    for (int x = tid; x < EV_ROWS * U; x += EV_THREADS) {
        const int r = x / U, u = x - r * U;
        const int64_t er = row0 + r < n ? row0 + r : row0;
        lds::Cst[r][u] = src ? src[er * U + u] : 0.0f;
        lds::Hb[0][r][u] = src ? src[(n + er) * U + u] : 0.0f;
    }
}
// and back, after a query (whose last position ends with a barrier): Cst and Hb[hp] to dst = [2][n][U]
__device__ __forceinline__ void ls_state_store(int tid, float* dst, int64_t n, int64_t row0, int hp) {
    for (int x = tid; x < EV_ROWS * U; x += EV_THREADS) {
        const int r = x / U, u = x - r * U;
        if (row0 + r < n) {
            dst[(row0 + r) * U + u] = lds::Cst[r][u];
            dst[(n + row0 + r) * U + u] = lds::Hb[hp][r][u];
        }
    }
}

// Record s of this lane's env: ob_s into the teacher's rows and the ring's slot; ob | the carried
// reward | stepped_with into the record (null: not kept)
__device__ __forceinline__ void ls_record_head(int lane, int slot, const rd::State& st, float* rec,
                                               float carry, float stepped_with) {
    float ob[rd::kObsDim];
    rd::observe<true>(st, ob);
#pragma unroll
    for (int k = 0; k < rd::kObsDim; ++k) {
        lds::SO[lane * tch::SOS + k] = ob[k];
        lds::Xr[slot][lane][k] = ob[k];
    }
    lds::SO[lane * tch::SOS + tch::OBD] = 1.0f;
    if (rec) {
#pragma unroll
        for (int k = 0; k < rd::kObsDim; ++k) rec[k] = ob[k];
        rec[rd::kObsDim] = carry;
        rec[EV_REC - 1] = stepped_with;
    }
}

// T_s: the teacher's wave on the block's raw obs rows, its pdflat into TO[s & 1]
__device__ __forceinline__ void ls_teacher(const LsThread& q, int s) {
    if (q.wave == EV_WAVES - 1) {
        rd::f32x4 A1[4], A2[4];
        float m0, m1;
        tch::mlp_forward<true>(lds::LT, lds::SO, q.i, q.gq, A1, A2, m0, m1);
        if (q.gq == 0) {
            float* o = lds::TO[s & 1][q.i];
            o[0] = m0; o[1] = m1; o[2] = lds::LT[tch::N_LS]; o[3] = lds::LT[tch::N_LS + 1];
        }
    }
}

// The query of episode step s: positions p = 0 .. T-1 hold records s - (T-1) + p, from the carried
// (c, h) in Cst, Hb[hp].  Every position ends with a barrier; returns the parity of the final h.
__device__ __forceinline__ int ls_positions(const LsThread& q, int s, int hp) {
    const int T = q.T, i = q.i, gq = q.gq;
    for (int p = 0; p < T; ++p) {
        const int j = s - (T - 1) + p;
        const float* xrow = j < 0 ? lds::Xz : &lds::Xr[j % T][i][0];
        const float* hrow = &lds::Hb[hp][i][0];
        for (int it = 0; it < (EV_UB + EV_WAVES - 1) / EV_WAVES; ++it) {
            const int ub = q.wave + EV_WAVES * it;
            if (ub >= EV_UB) break;   // (wave-uniform)
            const int u = 16 * ub + i;
            const bool uv = u < U;
            // the block's image: a scalar base (opaque here, so that its 64 load addresses are
            // formed where they are used, not once per launch and kept in registers) + the lane
            uint32_t here = 0;
            asm volatile("" : "+s"(here));
            const rdg::f32x4* wb = q.img4 + (int64_t)ub * (EV_G * 4 * 64) + here;
            const uint32_t ln = (uint32_t)q.lane;
            // group g's operands: the four gates' B (one 16-byte load each) and this lane's
            // A values x[i][k] / h[i][k], k = 4 (4 g' + e) + gq (zero past U: the B rows are zero
            // there, the LDS pad is not)
            rdg::f32x4 b[EV_PF][4];
            float av[EV_PF][4];
            auto fetch = [&](int g) {
#pragma unroll
                for (int y = 0; y < 4; ++y) b[g % EV_PF][y] = wb[(g * 4 + y) * 64 + ln];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k4 = 4 * (g < EV_GX ? g : g - EV_GX) + e;
                    av[g % EV_PF][e] = g < EV_GX ? xrow[4 * k4 + gq] : 4 * k4 < U ? hrow[4 * k4 + gq] : 0.0f;
                }
            };
#pragma unroll
            for (int g = 0; g < EV_PF; ++g) fetch(g);
            float bias[4];
#pragma unroll
            for (int y = 0; y < 4; ++y) bias[y] = uv ? q.P[OFF_BL + y * U + u] : 0.0f;
            rdg::f32x4 zx[4], lo[4], hi[4];
#pragma unroll
            for (int y = 0; y < 4; ++y) zx[y] = lo[y] = hi[y] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
            // a group: four k steps of the four gates' chains, its operands in registers
            // and the loads of group g + EV_PF issued before its MFMAs start (SrcC fence)
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
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int y = 0; y < 4; ++y)
                        acc[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[k], cur[y][k], acc[y], 0, 0, 0);
                fence_end(acc);
            };
#pragma unroll
            for (int g = 0; g < EV_G; ++g) {
                if (g < EV_GX) group(g, zx);
                else if (g < EV_GX + EV_GLO) group(g, lo);
                else group(g, hi);
            }
            // TF1 LSTMCell at rows 4 gq + r of unit u (lstm_rec_fwd_kernel's epilogue; Zx = acc + bias
            // is the Zx GEMM's)
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
                    const float c = fmaf(gf, lds::Cst[row][u], gi * gj);
                    lds::Cst[row][u] = c;
                    lds::Hb[hp ^ 1][row][u] = go * tanhf(c);
                }
            }
        }
        hp ^= 1;
        __syncthreads();
    }
    return hp;
}

// Head T-1 on the final h = Hb[hp] into X5 (head_fwd_kernel's layers, a barrier behind each; nothing
// stored to global: R = 0).  FENCE: head_layer's (the bf16 instances, which spill around the head).
template <bool FENCE = false>
__device__ __forceinline__ void ls_head(const LsThread& q, int hp) {
    const float (*X0)[EV_HS] = lds::Hb[hp];
    uint32_t hoff = 0;   // (opaque, as the image's base: the layers' addresses are formed here)
    asm volatile("" : "+s"(hoff));
    const float* Ph = q.Ph0 + hoff;
    head_layer<U, H1, true, EV_WAVES, FENCE>(X0, lds::X1, Ph + OFF_W1, Ph + OFF_B1, nullptr, 0, 0, 0);
    head_layer<H1, H2, true, EV_WAVES, FENCE>(lds::X1, lds::X2, Ph + OFF_W2, Ph + OFF_B2, nullptr, 0, 0, 0);
    head_layer<H2, H3, true, EV_WAVES, FENCE>(lds::X2, lds::X3, Ph + OFF_W3, Ph + OFF_B3, nullptr, 0, 0, 0);
    head_layer<H3, H4, true, EV_WAVES, FENCE>(lds::X3, lds::X4, Ph + OFF_W4, Ph + OFF_B4, nullptr, 0, 0, 0);
    head_layer<H4, 4, false, EV_WAVES, FENCE>(lds::X4, lds::X5, Ph + OFF_W5, Ph + OFF_B5, nullptr, 0, 0, 0);
}

// Step s's two pdflats at this lane's env: tp = T_s, sp = the head's row of X5 (no STUDENT: zeros,
// the teacher steps); the record's tail t_pdflat | s_pdflat (rec null: not kept)
template <bool STUDENT = true>
__device__ __forceinline__ void ls_record_tail(int lane, int s, float* rec, float (&tp)[4], float (&sp)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        sp[c] = STUDENT ? lds::X5[lane][c] : 0.0f;
        tp[c] = lds::TO[s & 1][lane][c];
    }
    if (rec) {
        float* r = rec + rd::kObsDim + 1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            r[c] = tp[c];
            r[4 + c] = sp[c];
        }
    }
}

// The noisy instances' draws (action noise, include/reacher_action_noise.h; student_lstm_noise.hip):
// taken in the env's lane before the step's first barrier, so that Philox and Box-Muller run beside
// the positions, and parked in LDS until ls_record_tail's side of the step -- the kernels run at the
// register limit, and two more values live across the step moved a spill's reload into an f32 MFMA's
// SrcC window (scripts/isa/hazards.py LDSRC).  The lane reads back what it wrote: no barrier.  Only
// the instances that call these carry the 128 bytes.
__device__ __forceinline__ float* ls_noise_park() {
    __shared__ float xi[EV_ROWS * 2];
    return xi;
}
__device__ __forceinline__ void ls_noise_draw(int lane, uint64_t seed, uint64_t env_id, int32_t episode, int32_t step) {
    float xi0, xi1;
    rd::action_noise_draw(seed, env_id, episode, step, xi0, xi1);
    ls_noise_park()[2 * lane] = xi0;
    ls_noise_park()[2 * lane + 1] = xi1;
}

// The faulty instances' pieces (sensor faults on the student's observation,
// include/reacher_obs_faults.h; student_lstm_faults.hip).  The positions read a record's observation
// from columns 0..10 of its x row in the ring, so that is where the mask goes: ls_fault_mask replaces
// row `row` of slot `slot`, record (episode, step) of env `env_id`, by what the student reads of it
// (rd::obs_fault_keep, rd::obs_fault_see) and, with `clean`, copies the clean readings there first.
// The record keeps that mask in every later query that still holds it; the zero record's row (Xz) is
// never touched.  The teacher's SO row and the record written to global memory keep the clean values.
// ls_fault_clean: the envs kernel's clean copy of the ring's observations, which its windows and the
// handle's history are written from; only the instances that call it carry the 11 KiB.
__device__ __forceinline__ float (*ls_fault_clean())[EV_ROWS][rd::kObsDim] {
    __shared__ float ob[EV_MAX_T][EV_ROWS][rd::kObsDim];
    return ob;
}
__device__ __forceinline__ void ls_fault_mask(int row, int slot, int32_t mode, float keep_prob, uint64_t seed,
                                              uint64_t env_id, int32_t episode, int32_t step,
                                              float (*clean)[EV_ROWS][rd::kObsDim]) {
    const uint32_t keep = rd::obs_fault_keep(seed, env_id, episode, step, keep_prob);
#pragma unroll
    for (int k = 0; k < rd::kObsDim; ++k) {
        const float v = lds::Xr[slot][row][k];
        if (clean) clean[slot][row][k] = v;
        lds::Xr[slot][row][k] = rd::obs_fault_see(mode, keep_prob, keep, k, v);
    }
}
