// The closed-loop step's window positions on the bf16 cell (rdl_set_query_dtype's RDL_DTYPE_BF16,
// include/reacher_student_lstm.h "Arithmetic"): ls_positions' sibling.  Included inside
// student_lstm.hip's anonymous namespace after student_lstm_query.h (the block's LDS, LsThread, the
// EV_* tiling) and student_lstm_bf16.h (bf16x8, bf_mfma, bf_pack8, the WF image's layout).
//
// One position is one lstm_bf16_fwd_kernel step on the block's 16 envs:
//     z = bl + sum over k' < 256 of bf([x | 0 | h | 0]_k') bf(Wl),
// the accumulators started from the bias, the same eight k-steps of 32 in the same order and the same
// lane-to-k' map (lane (i, g) holds k' = 32 S + 8 g .. + 7 of row i and of column i), then that
// kernel's cell at the lane's four (env, unit) points.  An MFMA row depends on no other row, so
// the 16 envs of a block give the bits the window pass gives their rows, wherever those lie in its
// 32-row tiles.  Everything else in a step -- ls_prologue, ls_record_head, ls_teacher, ls_head,
// ls_record_tail, the barriers -- is the one shared code of student_lstm_query.h, which the two
// kernels run in one order with either positions function: their bitwise equality with the stepwise
// path, and with each other, rests on that.
//
// Operands.  B comes straight from the handle's forward image WF (lstm_bf16_image_kernel, re-formed
// on the stream after every change of the master): no per-call pack launch.  A (unit block, k-step)
// is four 16-byte loads per lane, a wave's load of one gate one contiguous KB, 410 KB per position
// against the f32 image's 852 KB.  A is 8 consecutive floats of the env's x row (columns 0..47: 43..47
// are the ring's zeros, as X's zero column and the layout's pad) or h row in LDS, two ds_read_b128,
// rounded by bf_pack8; k' >= 248 selects zeros (h's LDS pad is not zero).  The f32 path's arrays and
// strides serve as they are: rows of 52 and 204 floats keep every read 16-byte aligned, and put a
// ds_read_b128 lane group's sixteen 16-byte slots two deep on six banks -- 16 such reads per wave
// and position, beside its 32 or 64 MFMAs and as many 16-byte weight loads.
// Tiling.  The 13 unit blocks go over the 8 waves as in ls_positions: wave w owns block w, and
// block w + 8 where there is one; its (block, k-step) pairs form ONE software pipeline, BQ_PF steps
// of weights in flight, which runs on into the next position's first steps (the weights of a wave
// are the same at every position) so that the cell's exp / tanh and the barrier cover their latency.
// The bf16 (XDL) MFMAs' SrcC is interlocked by the hardware (rd_device.h): no fence here.
#pragma once

constexpr int BQ_PF = 4;   // (unit block, k-step) pairs of B operands in flight ahead of the MFMAs
static_assert(BF_FS % BQ_PF == 0, "the pipeline's slots repeat from one position to the next");
static_assert(BF_XK + 8 <= EH_PREV && EV_XS % 4 == 0 && EV_HS % 4 == 0 && BF_HK0 + U + 8 == 32 * BF_FS &&
                  EV_UB <= 2 * EV_WAVES,
              "bf16 query tiling: x's groups end before the raw prev columns; 16-byte aligned rows");

// the weights of pipeline step idx = 8 (block of the wave) + S: the four gates' groups of the lane's
// unit, at a scalar base (the image + the step's and gate's offset) + the lane's 32-bit byte offset vo[.]
__device__ __forceinline__ void bq_load_b(const char* WFb, const uint32_t (&vo)[2], int idx, bf16x8 (&b)[4]) {
    const int S = idx % BF_FS, n = idx / BF_FS;
#pragma unroll
    for (int y = 0; y < 4; ++y)
        b[y] = *reinterpret_cast<const bf16x8*>(WFb + (size_t)((S * G4 + y * U) << 2) * sizeof(bf16x8) + vo[n]);
}
// the image's base, opaque here so that a lane's 32 or 64 load addresses are formed where they are
// used (a scalar base + the lane's offset), not once per launch and kept in registers
__device__ __forceinline__ const char* bq_image(const LsThread& q) {
    uint32_t here = 0;
    asm volatile("" : "+s"(here));
    return reinterpret_cast<const char*>(q.img4) + here;
}
// lane (i, g)'s byte offset into a (k-step, gate) slab of the image: unit uc's group g
__device__ __forceinline__ uint32_t bq_lane_offset(int uc, int g) {
    return (uint32_t)((uc << 2) + g) * (uint32_t)sizeof(bf16x8);
}

// this lane's A operand of k-step S: [x | 0 | h | 0] at k' = 32 S + 8 g .. + 7 of its env's rows
__device__ __forceinline__ bf16x8 bq_load_a(const float* xrow, const float* hrow, int g, int S) {
    const int kk = 32 * S + 8 * g;
    const bool ok = kk < BF_HK0 + U;
    const float* p = kk < BF_HK0 ? xrow + kk : hrow + (ok ? kk - BF_HK0 : 0);
    rdg::f32x4 lo = rd::ld4(p), hi = rd::ld4(p + 4);
    if (!ok) lo = hi = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
    return bf_pack8(lo, hi);
}

// One position for a wave that owns NUB unit blocks (ub0, ub0 + 8).  b holds the weights of the
// pipeline's first BQ_PF steps on entry, and again on return.
template <int NUB>
__device__ __forceinline__ void bq_position(const LsThread& q, const float* xrow, const float* hrow, int hp, int ub0,
                                            bf16x8 (&b)[BQ_PF][4]) {
    constexpr int N = NUB * BF_FS;
    const char* WFb = bq_image(q);
    const int i = q.i, g = q.gq;
    int u[2], uc[2];
    uint32_t vo[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        u[n] = 16 * (ub0 + EV_WAVES * (n < NUB ? n : 0)) + i;
        uc[n] = u[n] < U ? u[n] : U - 1;   // a lane past the last unit computes unit U - 1 again and stores nothing
        vo[n] = bq_lane_offset(uc[n], g);
    }
    rdg::f32x4 acc[NUB][4];
#pragma unroll
    for (int n = 0; n < NUB; ++n)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const float bias = q.P[OFF_BL + y * U + uc[n]];
            acc[n][y] = rdg::f32x4{bias, bias, bias, bias};
        }
    bf16x8 a[BQ_PF];
#pragma unroll
    for (int idx = 0; idx < BQ_PF; ++idx) a[idx] = bq_load_a(xrow, hrow, g, idx % BF_FS);
#pragma unroll
    for (int idx = 0; idx < N; ++idx) {
        const int n = idx / BF_FS;
        bf16x8 cw[4];
#pragma unroll
        for (int y = 0; y < 4; ++y) cw[y] = b[idx % BQ_PF][y];
        const bf16x8 ca = a[idx % BQ_PF];
        // step idx + BQ_PF into the slot just read; past the position's last, the next position's first
        bq_load_b(WFb, vo, (idx + BQ_PF) % N, b[idx % BQ_PF]);
        if (idx + BQ_PF < N) a[idx % BQ_PF] = bq_load_a(xrow, hrow, g, (idx + BQ_PF) % BF_FS);
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[n][y] = bf_mfma(ca, cw[y], acc[n][y]);
    }
    // TF1 LSTMCell at rows 4 g + r of the units (lstm_bf16_fwd_kernel's epilogue)
#pragma unroll
    for (int n = 0; n < NUB; ++n) {
        if (u[n] >= U) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * g + r;
            const float gi = sigm(acc[n][0][r]), gj = tanhf(acc[n][1][r]);
            const float gf = sigm(acc[n][2][r] + 1.0f), go = sigm(acc[n][3][r]);
            const float c = fmaf(gf, lds::Cst[row][u[n]], gi * gj);
            lds::Cst[row][u[n]] = c;
            lds::Hb[hp ^ 1][row][u[n]] = go * tanhf(c);
        }
    }
}

// ls_positions on the bf16 cell: positions p = 0 .. T-1 hold records s - (T-1) + p, from the carried
// (c, h) in Cst, Hb[hp].  Every position ends with a barrier; returns the parity of the final h.
__device__ __forceinline__ int ls_positions_bf16(const LsThread& q, int s, int hp) {
    const int T = q.T, i = q.i;
    const bool two = q.wave + EV_WAVES < EV_UB;   // (wave-uniform: wave is in an SGPR)
    bf16x8 b[BQ_PF][4];
    {
        const char* WFb = bq_image(q);
        const int u0 = 16 * q.wave + i;
        const uint32_t vo[2] = {bq_lane_offset(u0 < U ? u0 : U - 1, q.gq), 0};
#pragma unroll
        for (int idx = 0; idx < BQ_PF; ++idx) bq_load_b(WFb, vo, idx, b[idx]);
    }
    for (int p = 0; p < T; ++p) {
        const int j = s - (T - 1) + p;
        const float* xrow = j < 0 ? lds::Xz : &lds::Xr[j % T][i][0];
        const float* hrow = &lds::Hb[hp][i][0];
        if (two) bq_position<2>(q, xrow, hrow, hp, q.wave, b);
        else bq_position<1>(q, xrow, hrow, hp, q.wave, b);
        hp ^= 1;
        __syncthreads();
    }
    return hp;
}

// the positions of a kernel instance: the f32 master (ls_positions) or the bf16 cell
template <bool BF16Q>
__device__ __forceinline__ int ls_positions_of(const LsThread& q, int s, int hp) {
    if constexpr (BF16Q) return ls_positions_bf16(q, s, hp);
    else return ls_positions(q, s, hp);
}
