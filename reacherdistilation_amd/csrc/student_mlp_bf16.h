// student_mlp.hip's bf16 mixed-precision arithmetic (rdm_create_dtype's RDM_DTYPE_BF16,
// include/reacher_student_mlp.h): siblings of fwd_layer, dgrad_layer and wgrad_layer for the three
// wide layers 1, 2, 3 (24->128, 128->128, 128->32: 97.9 % of the MACs) on
// v_mfma_f32_16x16x32_bf16.  Layers 0 and 4, the biases, tanh, the loss, db and every sum stay the
// f32 kernel's.  Included inside student_mlp.hip's anonymous namespace after the f32 layer
// templates: Part, WG, pk, the strides and the image offsets are its.
//
// Operands.  The activations stay f32 in LDS, in the f32 kernel's buffers and layout
// ([row][pk(feature)], so the LDS budget is Lay<ROWS>'s); an operand is rounded where it is loaded
// (v_cvt_pk_bf16_f32, round-to-nearest-even).  A sum over k does not depend on the order of its
// exact products' operands, only on which the MFMA adds where, so the k of one MFMA are whatever 32
// the lane layout makes cheap, the same for A and B:
//  * forward / dgrad: lane (i, g) takes the 8 consecutive LDS floats 32 S + 8 g .. + 7 of its row
//    (two ds_read_b128), i.e. features 32 S + pk(8 g + j); the bf16 weight image stores the
//    matching 8 weights of a column as one 16-byte global load:
//      forward  HF[L]: bf(W[k][c]) at ((k/32) MP + c) 32 + pk(k % 32)
//      backward HB[L]: bf(W[k][c]) at ((c/32) KP + k) 32 + pk(c % 32)
//    (bf16 elements after the f32 image; zero padding that stays zero);
//  * wgrad (K = the block's rows): element j of lane (i, g) is row 32 s + 4 g + (j & 3) + 16 (j >> 2):
//    rows 4 apart land 16 banks apart at every stride in use (36, 132), so the 64 lanes of one
//    ds_read_b32 hit 64 banks.  The 16-row instance has no rows 16..31: elements 4..7 are zero.
#pragma once

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// lane l: A[row l&15][k 8(l>>4)+j], B[k 8(l>>4)+j][col l&15]; D[row 4(l>>4)+q][col l&15]
__device__ __forceinline__ f32x4 mfma_bf(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3],
                  (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}

// bf16 weight image, in bf16 elements from the end of the f32 image (layers 1..3 only)
constexpr int hf(int l) { return l <= 1 ? 0 : hf(l - 1) + 2 * KP[l - 1] * MP[l - 1]; }
constexpr int HF[NL] = {0, hf(1), hf(2), hf(3), 0};
constexpr int HB[NL] = {0, hf(1) + KP[1] * MP[1], hf(2) + KP[2] * MP[2], hf(3) + KP[3] * MP[3], 0};
constexpr int HIMG = hf(4);                     // 49,152 bf16 = 96 KiB
constexpr int IMG_ALL = IMG + HIMG / 2;         // floats of the whole allocation
static_assert(KP[1] % 32 == 0 && KP[2] % 32 == 0 && KP[3] % 32 == 0 && MP[1] % 32 == 0 && MP[2] % 32 == 0 &&
                  MP[3] % 32 == 0 && IMG % 4 == 0 && HIMG % 8 == 0,
              "bf16 image: whole 32-k groups, 16-byte aligned");
constexpr bool is_bf_layer(int l) { return l >= 1 && l <= 3; }
// the bf16 instances keep the activations in f32 in the f32 kernel's buffers and add none
static_assert(Lay<64>::LDS_FLOATS * 4 <= 160 * 1024 && Lay<16>::LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");

__device__ __forceinline__ const bf16x8* himg(const float* img, int off) {
    return reinterpret_cast<const bf16x8*>(reinterpret_cast<const unsigned short*>(img + IMG) + off);
}

// Forward of layer L (fwd_layer's contract): Y[row][pk(c)] = act(b[c] + sum_k bf(X[row][k]) bf(W[k][c])).
// Every column block's MFMAs are SrcC-fenced (rd_device.h), as fwd_layer<.., FENCE = true>.
template <int RB, int L, int SI, int SO>
__device__ __forceinline__ void fwd_layer_bf(const float* X, float* Y, const float* img, int wave, int i, int g) {
    static_assert(is_bf_layer(L), "bf16 layers");
    constexpr int NCB = MP[L] / 16, KG = KP[L] / 32;
    using PT = Part<NCB, RB>;
    if (!PT::active(wave)) return;
    const bf16x8* W = himg(img, HF[L]);
    const float* bias = img + BB[L];
    f32x4 acc[PT::CPW][PT::RPW];
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c) {
        const float b = bias[16 * PT::cb(wave, c) + i];
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) acc[c][r] = f32x4{b, b, b, b};
    }
#pragma unroll 2
    for (int S = 0; S < KG; ++S) {   // one K = 32 step per iteration
        bf16x8 a[PT::RPW];
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) {
            const float* p = X + (16 * PT::rb(wave, r) + i) * SI + 32 * S + 8 * g;
            a[r] = pack8(ld4(p), ld4(p + 4));
        }
#pragma unroll
        for (int c = 0; c < PT::CPW; ++c) {
            const bf16x8 w = W[((S * MP[L] + 16 * PT::cb(wave, c) + i) << 2) + g];
            fence_begin(acc[c]);
#pragma unroll
            for (int r = 0; r < PT::RPW; ++r) acc[c][r] = mfma_bf(a[r], w, acc[c][r]);
            fence_end(acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c)
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = acc[c][r][q];
                Y[(16 * PT::rb(wave, r) + 4 * g + q) * SO + pk(16 * PT::cb(wave, c) + i)] = TANH[L] ? tanh_fast(v) : v;
            }
}

// Backward data of layer L (dgrad_layer's contract):
// out[row][pk(c)] = (sum_m bf(D[row][m]) bf(W[c][m])) * act'(H[row][c]), H in f32.
template <int RB, int L, int SD, int SH, int SO>
__device__ __forceinline__ void dgrad_layer_bf(const float* D, const float* H, float* out, const float* img, int wave,
                                               int i, int g) {
    static_assert(is_bf_layer(L), "bf16 layers");
    constexpr int NCB = KP[L] / 16, MG = MP[L] / 32;
    using PT = Part<NCB, RB>;
    if (!PT::active(wave)) return;
    const bf16x8* W = himg(img, HB[L]);
    f32x4 acc[PT::CPW][PT::RPW];
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c)
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) acc[c][r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int S = 0; S < MG; ++S) {
        bf16x8 a[PT::RPW];
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r) {
            const float* p = D + (16 * PT::rb(wave, r) + i) * SD + 32 * S + 8 * g;
            a[r] = pack8(ld4(p), ld4(p + 4));
        }
#pragma unroll
        for (int c = 0; c < PT::CPW; ++c) {
            const bf16x8 w = W[((S * KP[L] + 16 * PT::cb(wave, c) + i) << 2) + g];
            fence_begin(acc[c]);
#pragma unroll
            for (int r = 0; r < PT::RPW; ++r) acc[c][r] = mfma_bf(a[r], w, acc[c][r]);
            fence_end(acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < PT::CPW; ++c)
#pragma unroll
        for (int r = 0; r < PT::RPW; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * PT::rb(wave, r) + 4 * g + q, pos = pk(16 * PT::cb(wave, c) + i);
                float v = acc[c][r][q];
                if (TANH[L - 1]) {
                    const float h = H[row * SH + pos];
                    v *= fmaf(-h, h, 1.0f);
                }
                out[row * SO + pos] = v;
            }
}

// column `pos` of 8 rows of a [row][stride] buffer as one MFMA operand: rows row0 + (j & 3) + 16 (j >> 2)
template <int ROWS, int ST>
__device__ __forceinline__ bf16x8 ld_rows8(const float* B, int row0, int pos) {
    f32x4 lo, hi = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) lo[j] = B[(row0 + j) * ST + pos];
    if constexpr (ROWS >= 32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) hi[j] = B[(row0 + 16 + j) * ST + pos];
    }
    return pack8(lo, hi);
}

// Weight gradient of layer L over the block (wgrad_layer's contract and partition):
// G[16kb + 4g + q][16cb + i] += sum_row bf(H[row][16kb + 4g + q]) bf(D[row][16cb + i]), 32 rows per MFMA.
template <int ROWS, int L, int SH, int SD>
__device__ __forceinline__ void wgrad_layer_bf(const float* H, const float* D, f32x4 (&G)[WG<L>::Q], int wave, int i,
                                               int g) {
    static_assert(is_bf_layer(L) && (ROWS == 16 || ROWS % 32 == 0), "bf16 layers; whole 32-row steps or one padded");
    using W = WG<L>;
    const int cb = wave % W::NCB;
#pragma unroll 1
    for (int s = 0; s < (ROWS + 31) / 32; ++s) {   // not unrolled: 8 operand quads are live per step
        const int row0 = 32 * s + 4 * g;
        const bf16x8 b = ld_rows8<ROWS, SD>(D, row0, pk(16 * cb + i));
        bf16x8 h[W::Q];
#pragma unroll
        for (int t = 0; t < W::Q; ++t)
            h[t] = W::ok(wave, t) ? ld_rows8<ROWS, SH>(H, row0, pk(16 * W::kb(wave, t) + i)) : bf16x8{};
        fence_begin(G);
#pragma unroll
        for (int t = 0; t < W::Q; ++t)
            if (W::ok(wave, t)) G[t] = mfma_bf(h[t], b, G[t]);
        fence_end(G);
    }
}

// the bf16 images of one weight (param_index's k, c of layer L)
__device__ __forceinline__ void store_param_bf(float* img, int L, int k, int c, float w) {
    int kp = 0, mp = 0, hfo = 0, hbo = 0;
#pragma unroll
    for (int l = 1; l <= 3; ++l)
        if (l == L) {
            kp = KP[l]; mp = MP[l]; hfo = HF[l]; hbo = HB[l];
        }
    unsigned short* h = reinterpret_cast<unsigned short*>(img + IMG);
    const unsigned short v = __builtin_bit_cast(unsigned short, (__bf16)w);
    h[hfo + (((k >> 5) * mp + c) << 5) + pk(k & 31)] = v;
    h[hbo + (((c >> 5) * kp + k) << 5) + pk(c & 31)] = v;
}
