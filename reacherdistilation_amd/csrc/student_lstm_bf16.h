// student_lstm.hip's bf16 mixed-precision arithmetic (rdl_create_dtype's RDL_DTYPE_BF16,
// include/reacher_student_lstm.h "Arithmetic"): the three products that hold the cell matrix
// Wl[243][800] -- 86 % of the multiply-adds per row -- on v_mfma_f32_16x16x32_bf16, siblings of
// lstm_rec_fwd_kernel (forward step, TF1 cell in the epilogue), rdg::EPI_LSTM_BWD (data gradient,
// cell backward of the step before in the epilogue) and the dWl GEMMs (weight gradient, split-K).
// Master weights, biases, the prev_pdflat projection, the cell's point-wise arithmetic, the heads,
// the loss, dbl, dWp, dbp and every sum stay f32.  Included inside student_lstm.hip's anonymous
// namespace: U, G4, XI, XLD, OFF_WL and sigm are student_lstm_layout.h's.
//
// Operands.  Activations stay f32 in HBM in the f32 path's buffers and are rounded where they
// are loaded (v_cvt_pk_bf16_f32, round-to-nearest-even); the weights come from two bf16 images of
// the master, re-formed on the stream after every change of it (lstm_bf16_image_kernel).  A sum
// over k does not depend on the order of its exact products, so the k of one MFMA are whatever 32
// the lane layout makes cheap, the same for A and B; lane (i, g) takes 8 consecutive floats of
// its row (two 16-byte loads) and the matching 8 weights of its column as one 16-byte load:
//  * forward, K' = 256 = 8 x 32 over [x_t (44: column 43 is X's zero column) | 0 (4) | h_{t-1}
//    (200) | 0 (8)], so that every 8-float group lies inside one 16-byte aligned row of X or H:
//      WF: bf(Wl[row(k')][c]) at ((k'/32) 800 + c) 32 + k' % 32
//  * data gradient, K = 800 = 25 x 32 gate columns, output columns n = dP (32: Wl rows 11..42) |
//    dh (200: Wl rows 43..242) | 0 (8), so that the dh blocks start at a unit multiple of 16:
//      WB: bf(Wl[row(n)][c]) at ((c/32) 240 + n) 32 + c % 32
//  * weight gradient, K = the T x B rows: element j of lane (i, g) is row 32 s + 8 g + j of
//    column i of its block, for [x | h_prev]^T as for dz (4-byte loads, 64-byte segments).
// No LDS, no barrier, no atomics, no hand-off between workgroups: every output has one owner and
// the split-K partials of the weight gradient are summed in split order by a second launch.
// The bf16 (XDL) MFMAs' SrcC is interlocked by the hardware (rd_device.h), so these kernels carry
// no fence: the loads of the next k-step are in flight under the current one's MFMAs.
#pragma once

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BF_FS = 8;                   // forward k-steps of 32
constexpr int BF_XK = 40;                  // k' of X's last group: columns 40..43, then 4 zeros
constexpr int BF_HK0 = 48;                 // k' of h_{t-1}[0]
constexpr int BF_BS = G4 / 32;             // data gradient k-steps of 32 (25)
constexpr int BF_BN = 32 + 208;            // its output columns: dP | dh | pad
constexpr int BF_NCB = BF_BN / 16;         // 15 column blocks: 0, 1 = dP; 2..14 = units 16 (cb - 2) ..
constexpr int BF_WF_GROUPS = BF_FS * G4 * 4, BF_WB_GROUPS = BF_BS * BF_BN * 4;   // 8-element groups
constexpr int BF_IMG_GROUPS = BF_WF_GROUPS + BF_WB_GROUPS;                       // 49,600 x 16 B
constexpr int BF_RB = 2, BF_ROWS = 16 * BF_RB;   // 16-row blocks per wave; rows per workgroup
constexpr int BF_KWL = XI + U;             // 243 rows of Wl
constexpr int BF_WG_SPLITS = 64;           // weight gradient: at most this many row chunks
constexpr int BF_WG_CHUNK = 64;            // of at least this many rows (a multiple of 32)
static_assert(G4 % 32 == 0 && U % 8 == 0 && XLD % 4 == 0 && BF_XK + 4 == XLD && BF_HK0 + U <= 32 * BF_FS &&
                  BF_HK0 % 8 == 0 && BF_BN % 16 == 0 && BF_BN >= 32 + U && BF_WG_CHUNK % 32 == 0,
              "bf16 tiling: whole 8-float groups, 16-byte aligned");

// the weight gradient's row chunk and split count for R rows (ns <= BF_WG_SPLITS, and
// <= ceil(Rmax / BF_WG_CHUNK) for every R <= Rmax: the workspace is sized from that at create)
__host__ __device__ constexpr int64_t bf_wg_chunk(int64_t R) {
    const int64_t c = ((R + BF_WG_SPLITS - 1) / BF_WG_SPLITS + 31) / 32 * 32;
    return c < BF_WG_CHUNK ? BF_WG_CHUNK : c;
}
__host__ __device__ constexpr int bf_wg_splits(int64_t R) { return (int)((R + bf_wg_chunk(R) - 1) / bf_wg_chunk(R)); }

// lane l: A[row l&15][k 8(l>>4)+j], B[k 8(l>>4)+j][col l&15]; D[row 4(l>>4)+q][col l&15]
__device__ __forceinline__ rdg::f32x4 bf_mfma(bf16x8 a, bf16x8 b, rdg::f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 bf_pack8(rdg::f32x4 lo, rdg::f32x4 hi) {
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3],
                  (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}
// 8 consecutive floats at p (16-byte aligned), rounded; zeros unless ok (p is not read then)
__device__ __forceinline__ bf16x8 bf_ld8(const float* p, bool ok) {
    rdg::f32x4 lo = rdg::f32x4{0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (ok) {
        lo = rd::ld4(p);
        hi = rd::ld4(p + 4);
    }
    return bf_pack8(lo, hi);
}

// Both images from the master: one thread per 8-element group.
__global__ __launch_bounds__(256) void lstm_bf16_image_kernel(const float* __restrict__ P, bf16x8* __restrict__ img) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= BF_IMG_GROUPS) return;
    const float* Wl = P + OFF_WL;
    float v[8];
    if (x < BF_WF_GROUPS) {   // WF[S][c][g]: k' = 32 S + 8 g + j
        const int g = x & 3, c = (x >> 2) % G4, S = (x >> 2) / G4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 32 * S + 8 * g + j;
            const int row = kk < XI ? kk : (kk >= BF_HK0 && kk < BF_HK0 + U) ? XI + kk - BF_HK0 : -1;
            v[j] = row >= 0 ? Wl[(int64_t)row * G4 + c] : 0.0f;
        }
    } else {                  // WB[S][n][g]: c = 32 S + 8 g + j
        const int y = x - BF_WF_GROUPS, g = y & 3, n = (y >> 2) % BF_BN, S = (y >> 2) / BF_BN;
        const int row = n < 32 ? 11 + n : n - 32 < U ? XI + n - 32 : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row >= 0 ? Wl[(int64_t)row * G4 + 32 * S + 8 * g + j] : 0.0f;
    }
    img[x] = bf16x8{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3],
                    (__bf16)v[4], (__bf16)v[5], (__bf16)v[6], (__bf16)v[7]};
}

// the forward's A operand of row `row` at k' = kk (a multiple of 8): [x | 0 | h_prev | 0]
__device__ __forceinline__ bf16x8 bf_fwd_a(const float* X, const float* Hp, int64_t row, bool rok, int kk) {
    rdg::f32x4 lo = rdg::f32x4{0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (rok) {
        if (kk < BF_XK) {
            lo = rd::ld4(X + row * XLD + kk);
            hi = rd::ld4(X + row * XLD + kk + 4);
        } else if (kk == BF_XK) {
            lo = rd::ld4(X + row * XLD + kk);   // columns 40..43, the last X's zero column
        } else if (kk >= BF_HK0 && kk < BF_HK0 + U) {
            lo = rd::ld4(Hp + row * U + (kk - BF_HK0));
            hi = rd::ld4(Hp + row * U + (kk - BF_HK0) + 4);
        }
    }
    return bf_pack8(lo, hi);
}

// One step of the forward recurrence, input half included (no Zx product): z = bl + [x_s | h_{s-1}]
// . Wl on the bf16 MFMAs, then lstm_rec_fwd_kernel's cell.  A workgroup owns BF_ROWS rows x 64
// units; wave w the 16 units of block 4 blockIdx.x + w (13 blocks: the waves past them leave) and
// all four gates of them, so a lane ends with the four pre-activations of its (row, unit) points.
__global__ __launch_bounds__(256) void lstm_bf16_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Hp,
                                                            const float* __restrict__ cprev,
                                                            const bf16x8* __restrict__ WF, const float* __restrict__ bl,
                                                            float* __restrict__ Gs, float* __restrict__ cs,
                                                            float* __restrict__ hs, int64_t B) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int ub = 4 * blockIdx.x + wave;
    if (16 * ub >= U) return;   // (uniform per wave; the kernel has no barrier)
    const int u = 16 * ub + i;
    const bool uok = u < U;
    const int uc = uok ? u : U - 1;   // a lane past the last unit computes unit U - 1 again and stores nothing
    const int64_t m0 = (int64_t)blockIdx.y * BF_ROWS;
    rdg::f32x4 acc[BF_RB][4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        const float b = bl[y * U + uc];
#pragma unroll
        for (int r = 0; r < BF_RB; ++r) acc[r][y] = rdg::f32x4{b, b, b, b};
    }
    bf16x8 a[BF_RB], w[4];
    auto load = [&](int S) {
#pragma unroll
        for (int r = 0; r < BF_RB; ++r) {
            const int64_t row = m0 + 16 * r + i;
            a[r] = bf_fwd_a(X, Hp, row, row < B, 32 * S + 8 * g);
        }
#pragma unroll
        for (int y = 0; y < 4; ++y) w[y] = WF[((S * G4 + y * U + uc) << 2) + g];
    };
    load(0);
#pragma unroll
    for (int S = 0; S < BF_FS; ++S) {
        bf16x8 ca[BF_RB], cw[4];
#pragma unroll
        for (int r = 0; r < BF_RB; ++r) ca[r] = a[r];
#pragma unroll
        for (int y = 0; y < 4; ++y) cw[y] = w[y];
        if (S + 1 < BF_FS) load(S + 1);
#pragma unroll
        for (int r = 0; r < BF_RB; ++r)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[r][y] = bf_mfma(ca[r], cw[y], acc[r][y]);
    }
    // TF1 LSTMCell (cell_fwd_kernel's arithmetic) at this lane's points
#pragma unroll
    for (int r = 0; r < BF_RB; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t row = m0 + 16 * r + 4 * g + q;
            if (row >= B || !uok) continue;
            const float gi = sigm(acc[r][0][q]), gj = tanhf(acc[r][1][q]);
            const float gf = sigm(acc[r][2][q] + 1.0f), go = sigm(acc[r][3][q]);
            const float c = fmaf(gf, cprev[row * U + u], gi * gj);
            float* gp = Gs + row * G4;
            gp[u] = gi; gp[U + u] = gj; gp[2 * U + u] = gf; gp[3 * U + u] = go;
            cs[row * U + u] = c;
            hs[row * U + u] = go * tanhf(c);
        }
    }
}

// Data gradient of step s: [dP_s | dh_{s-1}] = bf(dz_s) . bf(Wl rows 11..242)^T over the column
// blocks cb0 .. cb1 - 1 of the WB image.  Blocks 0, 1 store dP_s [B][32]; blocks 2.. carry the
// cell backward of step s - 1 in their epilogue (cell_bwd_kernel's arithmetic with dh = dh_head +
// this product): dz_{s-1} and dc in place, each (row, unit) by the one lane that owns it.  A
// workgroup owns BF_ROWS rows; wave w the blocks cb0 + 4 w .. + 3.  The launch of the last step's
// dP alone (blocks 0, 1 of dz_0) reads none of the cell pointers.
struct BfDgradArgs {
    const float* dz;        // dz_s [B][800]
    const bf16x8* WB;
    float* dP;              // dP_s [B][32]
    const float* dHh;       // dh of step s - 1 from its head [B][200]
    const float* G;         // gates of step s - 1 [B][800]
    const float* ct;        // c_{s-1} [B][200]
    const float* cp;        // c_{s-2} [B][200]
    float* dc;              // [B][200], in place
    float* dzo;             // dz_{s-1} [B][800]
    int64_t B;
    int cb0, cb1;
};
__global__ __launch_bounds__(256) void lstm_bf16_dgrad_kernel(BfDgradArgs p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int cbw = p.cb0 + 4 * wave;
    const int ncb = min(4, p.cb1 - cbw);
    if (ncb <= 0) return;   // (uniform per wave; no barrier)
    const int64_t m0 = (int64_t)blockIdx.x * BF_ROWS;
    rdg::f32x4 acc[BF_RB][4];
#pragma unroll
    for (int r = 0; r < BF_RB; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a[BF_RB], w[4];
    auto load = [&](int S) {
#pragma unroll
        for (int r = 0; r < BF_RB; ++r) {
            const int64_t row = m0 + 16 * r + i;
            a[r] = bf_ld8(p.dz + row * G4 + 32 * S + 8 * g, row < p.B);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // a block past the wave's last reads its first again, unused
            const int cb = c < ncb ? cbw + c : cbw;
            w[c] = p.WB[((S * BF_BN + 16 * cb + i) << 2) + g];
        }
    };
    load(0);
#pragma unroll 5
    for (int S = 0; S < BF_BS; ++S) {
        bf16x8 ca[BF_RB], cw[4];
#pragma unroll
        for (int r = 0; r < BF_RB; ++r) ca[r] = a[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) cw[c] = w[c];
        if (S + 1 < BF_BS) load(S + 1);
#pragma unroll
        for (int r = 0; r < BF_RB; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = bf_mfma(ca[r], cw[c], acc[r][c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= ncb) break;
        const int cb = cbw + c;
#pragma unroll
        for (int r = 0; r < BF_RB; ++r) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t row = m0 + 16 * r + 4 * g + q;
                if (row >= p.B) continue;
                const float v = acc[r][c][q];
                if (cb < 2) {
                    p.dP[row * 32 + 16 * cb + i] = v;
                    continue;
                }
                const int n = 16 * (cb - 2) + i;
                if (n >= U) continue;
                const int64_t idx = row * U + n;
                const float* gp = p.G + row * G4;
                const float gi = gp[n], gj = gp[U + n], gf = gp[2 * U + n], go = gp[3 * U + n];
                const float dh = p.dHh[idx] + v;
                const float tc = tanhf(p.ct[idx]);
                const float dcv = fmaf(dh * go, fmaf(-tc, tc, 1.0f), p.dc[idx]);
                float* dz = p.dzo + row * G4;
                dz[n] = dcv * gj * gi * (1.0f - gi);
                dz[U + n] = dcv * gi * fmaf(-gj, gj, 1.0f);
                dz[2 * U + n] = dcv * p.cp[idx] * gf * (1.0f - gf);
                dz[3 * U + n] = dh * tc * go * (1.0f - go);
                p.dc[idx] = dcv * gf;
            }
        }
    }
}

// Weight gradient, split-K: part[split][k][c] = sum over the split's rows r of bf([x | h_prev][r][k])
// bf(dz[r][c]), k < 243, c < 800.  Workgroup (bx, split): the 64 columns 64 bx .. and all 16 row
// blocks of the output, wave w the blocks 4 w .. 4 w + 3 (16 accumulators); rows r0 + 32 s + 8 g + j
// of the chunk per MFMA, rows past its end as zeros.  X: [R][XLD], Hp: [R][U] (h_{t-1} of row r),
// dz: [R][800].  lstm_bf16_wgrad_reduce_kernel sums the splits in split order.
__global__ __launch_bounds__(256) void lstm_bf16_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ Hp,
                                                              const float* __restrict__ dz, float* __restrict__ part,
                                                              int64_t R, int64_t chunk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(R, r0 + chunk);
    // this lane's operand columns: a lane without one (k >= 243, c >= 800) reads column 0 and selects 0
    const float* ap[4];
    int64_t as[4];
    bool aok[4], bok[4];
    int bc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = 16 * (4 * wave + q) + i;
        aok[q] = k < BF_KWL;
        ap[q] = !aok[q] ? X : k < XI ? X + k : Hp + (k - XI);
        as[q] = aok[q] && k >= XI ? U : XLD;
        const int c = 16 * (4 * blockIdx.x + q) + i;
        bok[q] = c < G4;
        bc[q] = bok[q] ? c : 0;
    }
    rdg::f32x4 acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[q][c] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int64_t r = r0; r < r1; r += 32) {
        int64_t rr[8];
        bool rok[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t x = r + 8 * g + j;
            rok[j] = x < r1;
            rr[j] = rok[j] ? x : r0;   // a valid row, its value unused
        }
        bf16x8 av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float va[8], vb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                va[j] = ap[q][rr[j] * as[q]];
                vb[j] = dz[rr[j] * G4 + bc[q]];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                va[j] = rok[j] && aok[q] ? va[j] : 0.0f;
                vb[j] = rok[j] && bok[q] ? vb[j] : 0.0f;
            }
            av[q] = bf16x8{(__bf16)va[0], (__bf16)va[1], (__bf16)va[2], (__bf16)va[3],
                           (__bf16)va[4], (__bf16)va[5], (__bf16)va[6], (__bf16)va[7]};
            bv[q] = bf16x8{(__bf16)vb[0], (__bf16)vb[1], (__bf16)vb[2], (__bf16)vb[3],
                           (__bf16)vb[4], (__bf16)vb[5], (__bf16)vb[6], (__bf16)vb[7]};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[q][c] = bf_mfma(av[q], bv[c], acc[q][c]);
    }
    float* out = part + (int64_t)blockIdx.y * BF_KWL * G4;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 16 * (4 * wave + q) + 4 * g + e;
                if (k < BF_KWL && bok[c]) out[(int64_t)k * G4 + bc[c]] = acc[q][c][e];
            }
}

// dWl[e] = part[0][e] + part[1][e] + ... in split order
__global__ __launch_bounds__(256) void lstm_bf16_wgrad_reduce_kernel(const float* __restrict__ part, int ns,
                                                                     float* __restrict__ dWl) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= BF_KWL * G4) return;
    float v = part[e];
    for (int s = 1; s < ns; ++s) v += part[(int64_t)s * BF_KWL * G4 + e];
    dWl[e] = v;
}
