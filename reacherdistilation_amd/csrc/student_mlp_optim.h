// student_mlp.hip's parameter kernels: the map from a flat parameter to its places in the gradient
// workspace and the weight images (PIdx, param_index, store_param), pack_kernel (rdm_set_params),
// reduce_adam_kernel (the fixed-order sum of the partial rows, the metrics row and TF1 Adam) and
// init_ctl_kernel (rdm_reset).  Included last inside student_mlp.hip's anonymous namespace, after
// the closed-loop kernels, which is where these kernels stand in the object; expects
// student_mlp_layout.h, student_mlp_bf16.h (store_param_bf) and rd_device.h (the adam_* steps).
#pragma once

// flat parameter index -> (layer, k, c) -> positions in the gradient workspace and images
struct PIdx {
    int g;        // workspace (gradient) index
    int f, b;     // image positions (b < 0 for a bias)
};
__device__ __forceinline__ PIdx param_index(int p) {
    int L = 0;
#pragma unroll
    for (int k = 1; k < NL; ++k) L += p >= PW[k] ? 1 : 0;
    int base = 0, in = 0, out = 0, kp = 0, mp = 0, gwo = 0, gbo = 0, fwo = 0, bwo = 0, bbo = 0;
#pragma unroll
    for (int k = 0; k < NL; ++k)
        if (k == L) {
            base = PW[k]; in = IN[k]; out = OUT[k]; kp = KP[k]; mp = MP[k];
            gwo = GW[k]; gbo = GB[k]; fwo = FW[k]; bwo = BW[k]; bbo = BB[k];
        }
    const int o = p - base;
    PIdx r;
    if (o < in * out) {
        const int k = o / out, c = o % out;
        r.g = gwo + k * mp + c;
        r.f = fwo + ((((k >> 4) * mp + c)) << 4) + ((k & 3) << 2) + ((k >> 2) & 3);
        r.b = bwo + ((((c >> 4) * kp + k)) << 4) + ((c & 3) << 2) + ((c >> 2) & 3);
    } else {
        r.g = gbo + (o - in * out);
        r.f = bbo + (o - in * out);
        r.b = -1;
    }
    return r;
}

__device__ __forceinline__ void store_param(float* img, const PIdx& ix, float w) {
    img[ix.f] = w;
    if (ix.b >= 0) img[ix.b] = w;
}

// BF: the bf16 images of layers 1..3 are re-formed with the f32 image (roundings of the same master)
template <bool BF>
__device__ __forceinline__ void store_param(float* img, int p, const PIdx& ix, float w) {
    store_param(img, ix, w);
    if constexpr (BF) {
        if (ix.b >= 0 && p >= PW[1] && p < PW[4]) {
            const int L = p < PW[2] ? 1 : p < PW[3] ? 2 : 3;
            const int o = p - (L == 1 ? PW[1] : L == 2 ? PW[2] : PW[3]), out = L == 3 ? OUT[3] : OUT[1];
            store_param_bf(img, L, o / out, o % out, w);
        }
    }
}

template <bool BF>
__global__ __launch_bounds__(256) void pack_kernel(const float* params, float* img) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < P_REF) store_param<BF>(img, p, param_index(p), params[p]);
}

// ctl: [0] optimiser steps S, [1] beta1^S, [2] beta2^S (f32 bits); [4..6] the training
// kernel's snapshot of them (block 0 of the Adam kernel rewrites [0..2]).
struct AdamArgs {
    const float* ws;
    int nblk;
    float* grad;
    float* params;
    float* img;
    float* m;
    float* v;
    uint32_t* ctl;
    float* hist;
    int hist_len;
    int reduce, adam;
    float lr, b1, b2, eps;
};

constexpr int ADAM_BLOCK = 256;
constexpr int ADAM_GRID = (P_REF + N_MET + ADAM_BLOCK - 1) / ADAM_BLOCK;

template <bool BF>
__global__ __launch_bounds__(ADAM_BLOCK) void reduce_adam_kernel(AdamArgs a) {
    const int p = blockIdx.x * ADAM_BLOCK + threadIdx.x;
    const uint32_t S = a.ctl[4];
    const float b1p = __uint_as_float(a.ctl[5]), b2p = __uint_as_float(a.ctl[6]);
    if (p < P_REF + N_MET) {
        const PIdx ix = p < P_REF ? param_index(p) : PIdx{GIMG + (p - P_REF), 0, -1};
        const int ip = ix.g;
        float gsum;
        if (a.reduce) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            const float* w = a.ws + ip;
            int b = 0;
            for (; b + 3 < a.nblk; b += 4) {
                s0 += w[(int64_t)b * WS_ROW];
                s1 += w[(int64_t)(b + 1) * WS_ROW];
                s2 += w[(int64_t)(b + 2) * WS_ROW];
                s3 += w[(int64_t)(b + 3) * WS_ROW];
            }
            for (; b < a.nblk; ++b) s0 += w[(int64_t)b * WS_ROW];
            gsum = (s0 + s1) + (s2 + s3);
            if (p < P_REF) a.grad[p] = gsum;
            else a.hist[(int64_t)(S % (uint32_t)a.hist_len) * N_MET + (p - P_REF)] = gsum;
        } else {
            gsum = p < P_REF ? a.grad[p] : 0.f;
        }
        if (a.adam && p < P_REF) {   // TF1 ApplyAdam (mlp_train.py:75-80)
            const float alpha = rd::adam_alpha(a.lr, b1p, b2p);
            float m = a.m[p], v = a.v[p];
            m = rd::adam_m(gsum, m, a.b1);
            v = rd::adam_v(gsum, v, a.b2);
            a.m[p] = m;
            a.v[p] = v;
            const float w = a.params[p] - rd::adam_delta(m, v, alpha, a.eps);
            a.params[p] = w;
            store_param<BF>(a.img, p, ix, w);
        }
    }
    if (a.adam && blockIdx.x == 0 && threadIdx.x == 0) {
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
