// The reference's LSTM student (include/reacher_student_lstm.h): forward over T unrolled
// steps of B windows and one truncated-BPTT distillation step, for gfx950.
//
// Graph (reference student_nn.py:21-49): x_t = [dropout(ob_t), dense32(prev_pdflat_t)];
// TF1 LSTMCell(200) (gates i, j, f, o; forget_bias 1); head 200-64-128-64-32-4 (tanh) -- one
// head PER UNROLLED STEP: the reference builds it with tf.layers.dense inside its Python loop
// over the T steps without reuse, so step t has its own five layers (dense_{5t+1..5t+5}),
// while the LSTMCell object (and the prev-pdflat dense) are shared.
//
// MI355X mapping.  Rows = (t, window) pairs, t-major, so every per-step slice is contiguous.
// All GEMM-shaped work runs on one MFMA GEMM (csrc/rd_gemm.h) with fused epilogues:
//  * the input half of the gate GEMM, [x_t] . Wl[0:43], is ONE GEMM over all T x B rows
//    (bias fused); only the recurrent half h_{t-1} . Wl[43:243] is per step, with the cell
//    fused into its epilogue (lstm_rec_fwd_kernel);
//  * the heads run once over all T x B rows after the recurrence (bias + tanh fused), step t's
//    rows with step t's weights;
//  * backward: each head layer's weight gradient and data gradient (tanh' of the stored
//    activation fused) run as one grouped launch (rdg::gemm2); BPTT is one launch per step,
//    dh_{t-1} = dz_t Wr^T with the cell backward of step t-1 in its epilogue; the LSTM weight
//    gradients ([x | h_prev]^T dz over all T x B rows) are one grouped launch at the end,
//    split-K with a fixed-order reduction when the output tile grid is small;
//  * bias gradients are deterministic two-level column sums; no atomics anywhere.
// Activations of all steps stay resident in HBM (sized at create for max_windows).
// rdl_create_dtype's RDL_DTYPE_BF16 sends the three products of the cell matrix Wl (the gate product of
// each step, input half included; dh / dP; dWl) to the bf16 MFMA kernels of student_lstm_bf16.h, always
// on this per-step path; everything else, and an f32 handle, runs what is described above.
// rdl_set_query_dtype's RDL_DTYPE_BF16 also sends the gate product of the closed-loop query (rdl_evaluate,
// the envs calls) to those MFMAs (student_lstm_query_bf16.h); by default it stays f32 on the master.
//
// One translation unit: the device code is the eight student_lstm_*.h that student_lstm_device.h
// includes and the two included below, in the order the kernels stand in the object.  This file keeps
// rdl_trainer, the choice of launches for a batch (Path), one function per cell path and head path, and
// the C ABI.  (The closed
// loop's noisy and faulty instances -- action noise, sensor faults on the student's observation -- are
// compiled in student_lstm_noise.hip and student_lstm_faults.hip: student_lstm_acting.h.)
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "student_lstm_device.h"
// after the ABI header, whose codes it returns
#include "rd_host.h"

namespace {

// the persistent recurrence (at most PR_ROWS windows): lstm_fwd_persist_kernel, lstm_bptt_persist_kernel
#include "student_lstm_persist.h"
// cell_bwd_kernel, loss_kernel, metrics_kernel, the column sums, adam_kernel, init_ctl_kernel
#include "student_lstm_optim.h"

}  // namespace

struct rdl_trainer {
    rdl_config cfg{};
    int device = 0, cus = 256;
    hipStream_t stream = nullptr;
    int T = 0;
    int64_t np = 0;   // flat parameters: the shared cell part + T heads (params_of(T))
    int64_t Bmax = 0;
    float *params = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *own_grad = nullptr;
    float *X = nullptr, *H = nullptr, *Cs = nullptr, *Z = nullptr, *G = nullptr;
    float *A1 = nullptr, *A2 = nullptr, *A3 = nullptr, *A4 = nullptr, *Y = nullptr, *dY = nullptr;
    float *D32 = nullptr, *D64a = nullptr, *D128 = nullptr, *D64b = nullptr, *dHh = nullptr, *dP = nullptr;
    float *dhn = nullptr, *dc = nullptr;
    float *split = nullptr, *colws = nullptr, *lpart = nullptr, *hist = nullptr;
    float* hpart = nullptr;    // fused head backward: one partial row of HB_PART per workgroup (head_nb)
    float* wpack = nullptr;    // [T][HWP]: the heads' weights packed by the training forward (small batches)
    int64_t colws_floats = 0;
    uint32_t* ctl = nullptr;
    uint32_t* bar = nullptr;   // persistent kernels: [0] forward / [1] BPTT barrier arrivals, [2] timeout flag,
                               // [3] granule generation
    float* bpart = nullptr;                // persistent BPTT: per-step-parity partial dh of every workgroup
    unsigned long long* hx = nullptr;      // persistent forward: per-step-parity h granules
    float* qbuf = nullptr;     // persistent BPTT: Q = prev^T dz [4][800]
    int64_t last_B = 0;   // windows of the last forward pass (rdl_final_state)
    float* tnet = nullptr;     // rdl_evaluate's teacher: params [tch::P_TOT] | ob mean [11] | ob std [11]
    float* eimg = nullptr;     // rdl_evaluate's packed image of Wl [EV_IMG], rebuilt by every call
    rd::DeviceAllocs mem;      // every device buffer of the handle but the envs'
    bool has_teacher = false;
    // the persistent envs (rdl_envs_attach)
    rd::EnvBufs envs;                                 // state [8][n] SoA, aux [ENV_AUX][n], clock [2][n]
    float* env_q = nullptr;                           // [2][n][U] = (c, h) of the envs' last query
    float* env_hist = nullptr;                        // [n][T][EH_REC]: the raw fields of the ring's records
    // RDL_DTYPE_BF16 (student_lstm_bf16.h): the bf16 images of Wl (forward, then transposed) and the
    // weight gradient's split-K partials [wsplits][243][800]; both null on an f32 handle
    int dtype = RDL_DTYPE_F32;
    bf16x8* wimg = nullptr;
    float* wpart = nullptr;
    // the closed-loop query's arithmetic (rdl_set_query_dtype): RDL_DTYPE_BF16 reads wimg's forward image
    int qdtype = RDL_DTYPE_F32;
    rd::Acting act;   // how the envs calls act (rdl_envs_set_*, rdl_envs_bind_actions); no stepped_with is ever bound
};

namespace {

constexpr int64_t SPLIT_FLOATS = 16 << 20;  // split-K partials (64 MB)

rdg::GemmArgs ga(int M, int N, int K, const float* A, int64_t lda, int ta, const float* B, int64_t ldb, int tb,
                 float* C, int64_t ldc, int epi = rdg::EPI_NONE, const float* aux = nullptr, int64_t ldaux = 0) {
    rdg::GemmArgs g{};
    g.M = M; g.N = N; g.K = K;
    g.A = A; g.lda = lda; g.ta = ta;
    g.B = B; g.ldb = ldb; g.tb = tb;
    g.C = C; g.ldc = ldc;
    g.epi = epi; g.aux = aux; g.ldaux = ldaux;
    return g;
}

hipError_t mm(rdl_trainer* t, int M, int N, int K, const float* A, int64_t lda, int ta, const float* B, int64_t ldb,
              int tb, float* C, int64_t ldc, const float* bias = nullptr, int epi = rdg::EPI_NONE) {
    rdg::GemmArgs g = ga(M, N, K, A, lda, ta, B, ldb, tb, C, ldc, epi);
    g.bias = bias;
    return rdg::gemm(t->stream, g, t->split, SPLIT_FLOATS, t->cus);
}

// two independent GEMMs as one grouped launch (rdg::gemm2): a head layer's weight gradient
// beside its data gradient, the two halves of the LSTM weight gradient
hipError_t mm2(rdl_trainer* t, const rdg::GemmArgs& g0, const rdg::GemmArgs& g1) {
    return rdg::gemm2(t->stream, g0, g1, t->split, SPLIT_FLOATS, t->cus);
}

hipError_t colsum(rdl_trainer* t, const float* src, int64_t M, int N, int64_t ld, float* out) {
    const unsigned gx = (unsigned)((N + 63) / 64);
    if (M <= COLSUM_CHUNK) {
        hipLaunchKernelGGL(colsum_kernel, dim3(gx, 1), dim3(256), 0, t->stream, src, M, N, ld, (int64_t)COLSUM_CHUNK,
                           out, (int64_t)0);
        return hipGetLastError();
    }
    const int64_t nch = (M + COLSUM_CHUNK - 1) / COLSUM_CHUNK;
    hipLaunchKernelGGL(colsum_kernel, dim3(gx, (unsigned)nch), dim3(256), 0, t->stream, src, M, N, ld,
                       (int64_t)COLSUM_CHUNK, t->colws, (int64_t)N);
    hipLaunchKernelGGL(colsum_kernel, dim3(gx, 1), dim3(256), 0, t->stream, (const float*)t->colws, nch, N,
                       (int64_t)N, nch, out, (int64_t)0);
    return hipGetLastError();
}

// head_bwd_kernel's 16-row tiles per workgroup: one while the T x ceil(B / 16) tiles fill at
// most ~4 workgroups per CU, then up to 8, so the partial rows (HB_PART floats each) and their
// reduce shrink with the batch
int head_tpb(int T, int64_t B) {
    const int64_t tiles = (B + HF_ROWS - 1) / HF_ROWS;
    return (int)std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)T * tiles / 1024));
}
int head_nb(int T, int64_t B) {
    const int64_t tiles = (B + HF_ROWS - 1) / HF_ROWS, tpb = head_tpb(T, B);
    return (int)((tiles + tpb - 1) / tpb);
}

// the fused head's one-tile workgroups are few enough for its latency-bound forms (head_fwd_kernel<true>)
bool head_wide(int T, int64_t B) { return (int64_t)T * ((B + HF_ROWS - 1) / HF_ROWS) <= HB_WIDE_GRID; }

bool bf16_cell(const rdl_trainer* t) { return t->dtype == RDL_DTYPE_BF16; }
bool bf16_query(const rdl_trainer* t) { return t->qdtype == RDL_DTYPE_BF16; }

// The launches that a pass over B windows issues, decided once per call (path_of) and handed to
// run_forward and run_backward: the persistent recurrence kernels for batches of at most PR_ROWS
// windows, and the one-launch head for at most HF_MAX_ROWS rows; rdl_config.kernels can select the
// per-step / per-layer launches instead (RDL_KERNELS_*: tests compare the two paths).
enum class Cell { Persistent, StepF32, StepBf16 };
struct Path {
    Cell cell;
    bool fused_head;     // head_fwd_kernel / head_bwd_kernel; else rd_gemm launches per step and layer
    bool loss_in_head;   // the head forward forms dY and the loss sums, grad_finish_kernel the metrics
};

Path path_of(const rdl_trainer* t, int64_t B, bool train) {
    Path p{};
    // a bf16 handle always takes the per-step path: the persistent kernels are f32 only
    // (T < PR_MAX_T: every phase fits its tag field)
    p.cell = bf16_cell(t) ? Cell::StepBf16
             : !(t->cfg.kernels & RDL_KERNELS_STEP_RECURRENCE) && B <= PR_ROWS && t->T < PR_MAX_T ? Cell::Persistent
                                                                                                   : Cell::StepF32;
    // the partial rows of the fused head's T x head_nb workgroups live in hpart (sized at create for
    // max_windows when that fits HPART_MAX_FLOATS); with one head per step, the per-layer path
    // is T x 11 launches, so the fused head now covers up to 16,384 rows
    p.fused_head = !(t->cfg.kernels & RDL_KERNELS_LAYER_HEAD) && t->hpart && (int64_t)t->T * B <= HF_MAX_ROWS;
    // training: the loss rides in the head forward where that runs as one wide-grid launch
    p.loss_in_head = train && p.fused_head && p.cell == Cell::Persistent && head_wide(t->T, B);
    return p;
}

// the bf16 images of Wl from the master weights, on the stream (after every change of the master)
int bf16_images(rdl_trainer* t) {
    hipLaunchKernelGGL(lstm_bf16_image_kernel, dim3((BF_IMG_GROUPS + 255) / 256), dim3(256), 0, t->stream,
                       (const float*)t->params, t->wimg);
    RD_HIP(hipGetLastError(), "rdl lstm_bf16_image_kernel");
    return RD_OK;
}

// ---------------------------------------------------------------- forward: one function per path
// X, Zx and all T recurrent steps in one launch (it writes the step-0 state rows)
int cell_forward_persistent(rdl_trainer* t, const float* ob, const float* prev, const float* state0, int64_t B,
                            float kp) {
    hipLaunchKernelGGL(lstm_fwd_persist_kernel, dim3(PR_GRID_F), dim3(256), 0, t->stream, (const float*)t->params, ob,
                       prev, t->X, state0, t->G, t->Cs, t->H, (int)B, t->T, kp, t->cfg.seed, t->cfg.row_base,
                       (const uint32_t*)t->ctl, t->bar, t->hx);
    RD_HIP(hipGetLastError(), "rdl lstm_fwd_persist_kernel");
    return RD_OK;
}

// the per-step paths' X rows of all steps and the step-0 state rows
int step_inputs(rdl_trainer* t, const float* ob, const float* prev, const float* state0, int64_t B, float kp) {
    const int64_t R = (int64_t)t->T * B;
    hipLaunchKernelGGL(inputs_kernel, dim3((unsigned)((R * XLD + 255) / 256)), dim3(256), 0, t->stream, ob, prev,
                       (const float*)t->params, t->X, R, B, kp, t->cfg.seed, t->cfg.row_base, (const uint32_t*)t->ctl);
    RD_HIP(hipGetLastError(), "rdl inputs_kernel");
    if (state0) {
        RD_HIP(hipMemcpyAsync(t->Cs, state0, sizeof(float) * B * U, hipMemcpyDeviceToDevice, t->stream), "rdl state");
        RD_HIP(hipMemcpyAsync(t->H, state0 + B * U, sizeof(float) * B * U, hipMemcpyDeviceToDevice, t->stream),
               "rdl state");
    } else {
        RD_HIP(hipMemsetAsync(t->Cs, 0, sizeof(float) * B * U, t->stream), "rdl state");
        RD_HIP(hipMemsetAsync(t->H, 0, sizeof(float) * B * U, t->stream), "rdl state");
    }
    return RD_OK;
}

int cell_forward_step_f32(rdl_trainer* t, const float* ob, const float* prev, const float* state0, int64_t B,
                          float kp) {
    if (int rc = step_inputs(t, ob, prev, state0, B, kp)) return rc;
    const int T = t->T;
    const float* P = t->params;
    // input half of the gate pre-activations for all steps: Z = X[:, :43] Wl[0:43] + bl
    RD_HIP(mm(t, (int)(T * B), G4, XI, t->X, XLD, 0, P + OFF_WL, G4, 0, t->Z, G4, P + OFF_BL), "rdl gemm Zx");
    const dim3 grid((U + RF_UNITS - 1) / RF_UNITS, (unsigned)((B + RF_ROWS - 1) / RF_ROWS));
    for (int s = 0; s < T; ++s) {
        hipLaunchKernelGGL(lstm_rec_fwd_kernel, grid, dim3(256), 0, t->stream,
                           (const float*)(t->H + (int64_t)s * B * U), P + OFF_WL + XI * G4,
                           (const float*)(t->Z + (int64_t)s * B * G4), (const float*)(t->Cs + (int64_t)s * B * U),
                           t->G + (int64_t)s * B * G4, t->Cs + (int64_t)(s + 1) * B * U,
                           t->H + (int64_t)(s + 1) * B * U, B);
        RD_HIP(hipGetLastError(), "rdl lstm_rec_fwd_kernel");
    }
    return RD_OK;
}

// both halves of the gate product in the step's launch, from the bf16 image
int cell_forward_step_bf16(rdl_trainer* t, const float* ob, const float* prev, const float* state0, int64_t B,
                           float kp) {
    if (int rc = step_inputs(t, ob, prev, state0, B, kp)) return rc;
    const dim3 grid((U / 16 + 4) / 4, (unsigned)((B + BF_ROWS - 1) / BF_ROWS));
    for (int s = 0; s < t->T; ++s) {
        hipLaunchKernelGGL(lstm_bf16_fwd_kernel, grid, dim3(256), 0, t->stream,
                           (const float*)(t->X + (int64_t)s * B * XLD), (const float*)(t->H + (int64_t)s * B * U),
                           (const float*)(t->Cs + (int64_t)s * B * U), (const bf16x8*)t->wimg,
                           (const float*)t->params + OFF_BL, t->G + (int64_t)s * B * G4,
                           t->Cs + (int64_t)(s + 1) * B * U, t->H + (int64_t)(s + 1) * B * U, B);
        RD_HIP(hipGetLastError(), "rdl lstm_bf16_fwd_kernel");
    }
    return RD_OK;
}

// step t's head over its B rows (student_nn.py:42-46, one head per unrolled step), as one launch
int head_forward_fused(rdl_trainer* t, const Path& p, int64_t B, float* out_pdflat, const float* tgt,
                       int64_t B_global) {
    const int T = t->T, nb = (int)((B + HF_ROWS - 1) / HF_ROWS);
    HeadLoss hl{};
    if (p.loss_in_head) hl = HeadLoss{tgt, t->dY, t->lpart, 1.0f / ((float)T * (float)B_global), t->cfg.loss};
    auto* kern = head_wide(T, B) ? head_fwd_kernel<true> : head_fwd_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(T * nb)), dim3(256), 0, t->stream, (const float*)(t->H + B * U),
                       (const float*)t->params, t->A1, t->A2, t->A3, t->A4, out_pdflat, B, nb, hl);
    RD_HIP(hipGetLastError(), "rdl head_fwd_kernel");
    return RD_OK;
}

// the same heads as five GEMMs per step (bias + tanh fused)
int head_forward_layers(rdl_trainer* t, int64_t B, float* out_pdflat) {
    const float* Hc = t->H + B * U;
    const int Bi = (int)B;
    for (int s = 0; s < t->T; ++s) {
        const float* Ph = t->params + OFF_H + (int64_t)s * HSZ;
        const int64_t r0 = (int64_t)s * B;
        RD_HIP(mm(t, Bi, H1, U, Hc + r0 * U, U, 0, Ph + OFF_W1, H1, 0, t->A1 + r0 * L1, L1, Ph + OFF_B1, rdg::EPI_TANH),
               "rdl head1");
        RD_HIP(mm(t, Bi, H2, H1, t->A1 + r0 * L1, L1, 0, Ph + OFF_W2, H2, 0, t->A2 + r0 * L2, L2, Ph + OFF_B2,
                  rdg::EPI_TANH), "rdl head2");
        RD_HIP(mm(t, Bi, H3, H2, t->A2 + r0 * L2, L2, 0, Ph + OFF_W3, H3, 0, t->A3 + r0 * L3, L3, Ph + OFF_B3,
                  rdg::EPI_TANH), "rdl head3");
        RD_HIP(mm(t, Bi, H4, H3, t->A3 + r0 * L3, L3, 0, Ph + OFF_W4, H4, 0, t->A4 + r0 * L4, L4, Ph + OFF_B4,
                  rdg::EPI_TANH), "rdl head4");
        RD_HIP(mm(t, Bi, 4, H4, t->A4 + r0 * L4, L4, 0, Ph + OFF_W5, 4, 0, out_pdflat + r0 * 4, 4, Ph + OFF_B5),
               "rdl head5");
    }
    return RD_OK;
}

// forward over all T steps of B windows.  out_pdflat: where the head's output goes (the
// internal Y when training).  tgt: the targets of a training pass (dropout on; where
// p.loss_in_head, the head forward forms the loss from them), null for inference.
int run_forward(rdl_trainer* t, const Path& p, const float* ob, const float* prev, const float* state0, int64_t B,
                float* out_pdflat, const float* tgt = nullptr, int64_t B_global = 0) {
    t->last_B = B;
    const float kp = tgt ? t->cfg.keep_prob : 1.0f;
    int rc = RD_OK;
    switch (p.cell) {
        case Cell::Persistent: rc = cell_forward_persistent(t, ob, prev, state0, B, kp); break;
        case Cell::StepF32: rc = cell_forward_step_f32(t, ob, prev, state0, B, kp); break;
        case Cell::StepBf16: rc = cell_forward_step_bf16(t, ob, prev, state0, B, kp); break;
    }
    if (rc) return rc;
    return p.fused_head ? head_forward_fused(t, p, B, out_pdflat, tgt, B_global)
                        : head_forward_layers(t, B, out_pdflat);
}

// ---------------------------------------------------------------- backward: one function per path
// the heads' backward as two launches (head_bwd_kernel + fixed-order reduce; where p.loss_in_head,
// grad_finish_kernel sums the partial rows after BPTT instead)
int head_backward_fused(rdl_trainer* t, const Path& p, int64_t B) {
    const int T = t->T, nb = head_nb(T, B), tpb = head_tpb(T, B);
    const bool wide = tpb == 1 && (int64_t)T * nb <= HB_WIDE_GRID;
    auto* kern = tpb > 1 ? head_bwd_kernel<true, 8> : wide ? head_bwd_kernel<false, 16> : head_bwd_kernel<false, 4>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(T * nb)), dim3(tpb > 1 ? 512 : wide ? 1024 : 256), 0, t->stream,
                       (const float*)(t->H + B * U), (const float*)t->params, (const float*)t->A1, (const float*)t->A2,
                       (const float*)t->A3, (const float*)t->A4, (const float*)t->dY, t->dHh, t->hpart, B, nb, tpb,
                       wide ? (const float*)t->wpack : nullptr);
    RD_HIP(hipGetLastError(), "rdl head_bwd_kernel");
    if (!p.loss_in_head) {
        hipLaunchKernelGGL(head_wgrad_reduce_kernel, dim3((HB_PART + 255) / 256, (unsigned)T), dim3(256), 0, t->stream,
                           (const float*)t->hpart, nb, t->grad);
        RD_HIP(hipGetLastError(), "rdl head_wgrad_reduce_kernel");
    }
    return RD_OK;
}

// step s's head backward over its B rows: per layer, [dW; db] (weight gradient, ones column)
// beside the data gradient with tanh' fused
int head_backward_layers(rdl_trainer* t, int64_t B) {
    const float* Hc = t->H + B * U;
    const int Bi = (int)B;
    for (int s = 0; s < t->T; ++s) {
        const float* Ph = t->params + OFF_H + (int64_t)s * HSZ;
        float* gh = t->grad + OFF_H + (int64_t)s * HSZ;
        const int64_t r0 = (int64_t)s * B;
        const float *a1 = t->A1 + r0 * L1, *a2 = t->A2 + r0 * L2, *a3 = t->A3 + r0 * L3, *a4 = t->A4 + r0 * L4;
        const float* dy = t->dY + r0 * 4;
        float *d32 = t->D32 + r0 * H4, *d64a = t->D64a + r0 * H3, *d128 = t->D128 + r0 * H2, *d64b = t->D64b + r0 * H1;
        RD_HIP(mm2(t, ga(H4 + 1, 4, Bi, a4, L4, 1, dy, 4, 0, gh + OFF_W5, 4),
                   ga(Bi, H4, 4, dy, 4, 0, Ph + OFF_W5, 4, 1, d32, H4, rdg::EPI_DTANH, a4, L4)),
               "rdl dW5 db5 | dZ4");
        RD_HIP(mm2(t, ga(H3 + 1, H4, Bi, a3, L3, 1, d32, H4, 0, gh + OFF_W4, H4),
                   ga(Bi, H3, H4, d32, H4, 0, Ph + OFF_W4, H4, 1, d64a, H3, rdg::EPI_DTANH, a3, L3)),
               "rdl dW4 db4 | dZ3");
        RD_HIP(mm2(t, ga(H2 + 1, H3, Bi, a2, L2, 1, d64a, H3, 0, gh + OFF_W3, H3),
                   ga(Bi, H2, H3, d64a, H3, 0, Ph + OFF_W3, H3, 1, d128, H2, rdg::EPI_DTANH, a2, L2)),
               "rdl dW3 db3 | dZ2");
        RD_HIP(mm2(t, ga(H1 + 1, H2, Bi, a1, L1, 1, d128, H2, 0, gh + OFF_W2, H2),
                   ga(Bi, H1, H2, d128, H2, 0, Ph + OFF_W2, H2, 1, d64b, H1, rdg::EPI_DTANH, a1, L1)),
               "rdl dW2 db2 | dZ1");
        RD_HIP(mm2(t, ga(U, H1, Bi, Hc + r0 * U, U, 1, d64b, H1, 0, gh + OFF_W1, H1),
                   ga(Bi, U, H1, d64b, H1, 0, Ph + OFF_W1, H1, 1, t->dHh + r0 * U, U)),
               "rdl dW1 | dHhead");
        RD_HIP(colsum(t, d64b, B, H1, H1, gh + OFF_B1), "rdl db1");
    }
    return RD_OK;
}

// Each cell backward runs BPTT from dHh and leaves dWl and dbl in the gradient, and for the dense32
// tail either Q = prev^T dz in qbuf (persistent) or dP (per step).  The per-step paths reuse the
// gate buffer Z for dz: the forward keeps the activations in G.

// all T steps of BPTT, dWl, dbl and Q in one launch
int cell_backward_persistent(rdl_trainer* t, const float* prev, int64_t B) {
    hipLaunchKernelGGL(lstm_bptt_persist_kernel, dim3(PR_GRID), dim3(256), 0, t->stream,
                       (const float*)t->params + OFF_WL + XI * G4, (const float*)t->dHh, (const float*)t->G,
                       (const float*)t->Cs, (const float*)t->X, (const float*)t->H, t->grad + OFF_WL, t->bpart,
                       t->grad + OFF_BL, prev, t->qbuf, (int)B, t->T, t->bar);
    RD_HIP(hipGetLastError(), "rdl lstm_bptt_persist_kernel");
    return RD_OK;
}

// the per-step paths' first launches: dc = 0 and the last step's cell alone -> dz_{T-1}
int bptt_last_cell(rdl_trainer* t, int64_t B) {
    const int T = t->T;
    RD_HIP(hipMemsetAsync(t->dc, 0, sizeof(float) * B * U, t->stream), "rdl bptt");
    hipLaunchKernelGGL(cell_bwd_kernel, dim3((unsigned)((B * U + 255) / 256)), dim3(256), 0, t->stream,
                       (const float*)(t->dHh + (int64_t)(T - 1) * B * U), (const float*)t->dhn, 0,
                       (const float*)(t->G + (int64_t)(T - 1) * B * G4), (const float*)(t->Cs + (int64_t)T * B * U),
                       (const float*)(t->Cs + (int64_t)(T - 1) * B * U), t->dc, t->Z + (int64_t)(T - 1) * B * G4, B);
    RD_HIP(hipGetLastError(), "rdl cell_bwd_kernel");
    return RD_OK;
}

// per step s the GEMM dh_{s-1} = dz_s . Wr^T whose epilogue (or split-K reduce) runs the cell
// backward of step s-1 -> dz_{s-1}, dc; then dWl = [x | h_prev]^T dz over all rows, dbl, dP
int cell_backward_step_f32(rdl_trainer* t, int64_t B) {
    if (int rc = bptt_last_cell(t, B)) return rc;
    const int T = t->T, Ri = (int)(T * B);
    const float* P = t->params;
    float *dZl = t->Z, *g = t->grad;
    for (int s = T - 1; s > 0; --s) {
        rdg::GemmArgs a = ga((int)B, U, G4, dZl + (int64_t)s * B * G4, G4, 0, P + OFF_WL + XI * G4, G4, 1, t->dhn, U,
                             rdg::EPI_LSTM_BWD, t->dHh + (int64_t)(s - 1) * B * U, U);
        a.lg = t->G + (int64_t)(s - 1) * B * G4;
        a.lct = t->Cs + (int64_t)s * B * U;
        a.lcp = t->Cs + (int64_t)(s - 1) * B * U;
        a.lcc = t->dc;
        a.lz = dZl + (int64_t)(s - 1) * B * G4;
        RD_HIP(rdg::gemm(t->stream, a, t->split, SPLIT_FLOATS, t->cus), "rdl gemm dh + cell");
    }
    RD_HIP(mm2(t, ga(XI, G4, Ri, t->X, XLD, 1, dZl, G4, 0, g + OFF_WL, G4),
               ga(U, G4, Ri, t->H, U, 1, dZl, G4, 0, g + OFF_WL + XI * G4, G4)),
           "rdl dWl x | h");
    RD_HIP(colsum(t, dZl, Ri, G4, G4, g + OFF_BL), "rdl dbl");
    RD_HIP(mm(t, Ri, 32, G4, dZl, G4, 0, P + OFF_WL + 11 * G4, G4, 1, t->dP, 32), "rdl dP");
    return RD_OK;
}

// per step s [dP_s | dh_{s-1}] from the transposed bf16 image, the cell backward of step s - 1 fused;
// then dWl split-K over the rows, the partials summed in split order, and dbl
int cell_backward_step_bf16(rdl_trainer* t, int64_t B) {
    if (int rc = bptt_last_cell(t, B)) return rc;
    const int T = t->T;
    const int64_t R = (int64_t)T * B;
    float *dZl = t->Z, *g = t->grad;
    const unsigned gx = (unsigned)((B + BF_ROWS - 1) / BF_ROWS);
    for (int s = T - 1; s >= 0; --s) {
        BfDgradArgs a{};
        a.dz = dZl + (int64_t)s * B * G4;
        a.WB = t->wimg + BF_WF_GROUPS;
        a.dP = t->dP + (int64_t)s * B * 32;
        a.B = B;
        a.cb0 = 0;
        a.cb1 = 2;   // step 0: its dP alone
        if (s > 0) {
            a.cb1 = BF_NCB;
            a.dHh = t->dHh + (int64_t)(s - 1) * B * U;
            a.G = t->G + (int64_t)(s - 1) * B * G4;
            a.ct = t->Cs + (int64_t)s * B * U;
            a.cp = t->Cs + (int64_t)(s - 1) * B * U;
            a.dc = t->dc;
            a.dzo = dZl + (int64_t)(s - 1) * B * G4;
        }
        hipLaunchKernelGGL(lstm_bf16_dgrad_kernel, dim3(gx), dim3(256), 0, t->stream, a);
        RD_HIP(hipGetLastError(), "rdl lstm_bf16_dgrad_kernel");
    }
    const int ns = bf_wg_splits(R);
    hipLaunchKernelGGL(lstm_bf16_wgrad_kernel, dim3((G4 + 63) / 64, (unsigned)ns), dim3(256), 0, t->stream,
                       (const float*)t->X, (const float*)t->H, (const float*)dZl, t->wpart, R, bf_wg_chunk(R));
    RD_HIP(hipGetLastError(), "rdl lstm_bf16_wgrad_kernel");
    hipLaunchKernelGGL(lstm_bf16_wgrad_reduce_kernel, dim3((BF_KWL * G4 + 255) / 256), dim3(256), 0, t->stream,
                       (const float*)t->wpart, ns, g + OFF_WL);
    RD_HIP(hipGetLastError(), "rdl lstm_bf16_wgrad_reduce_kernel");
    RD_HIP(colsum(t, dZl, R, G4, G4, g + OFF_BL), "rdl dbl");
    return RD_OK;
}

// dWp, dbp of the input-side dense32 layer, last in the gradient
int dense32_backward(rdl_trainer* t, const Path& p, const float* prev, int64_t B) {
    const int T = t->T;
    const int64_t R = (int64_t)T * B;
    float* g = t->grad;
    if (p.loss_in_head) {   // with the heads' row sums and the metrics, from the BPTT kernel's dbl and Q: one launch
        hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)(T * HB_BLK + 161)), dim3(256), 0, t->stream,
                           (const float*)t->hpart, head_nb(T, B), T, (const float*)t->params, (const float*)t->qbuf, g,
                           (const float*)t->lpart, (int)(T * ((B + HF_ROWS - 1) / HF_ROWS)), (float)R, t->ctl, t->hist,
                           t->cfg.metrics_len);
        RD_HIP(hipGetLastError(), "rdl grad_finish_kernel");
    } else if (p.cell == Cell::Persistent) {   // from the BPTT kernel's dbl and Q = prev^T dz: one launch
        hipLaunchKernelGGL(dense32_grad_kernel, dim3(160), dim3(256), 0, t->stream, (const float*)t->params,
                           (const float*)t->qbuf, g);
        RD_HIP(hipGetLastError(), "rdl dense32_grad_kernel");
    } else {   // from the per-step paths' dP
        RD_HIP(mm(t, 4, 32, (int)R, prev, 4, 1, t->dP, 32, 0, g + OFF_WP, 32), "rdl dWp");
        RD_HIP(colsum(t, t->dP, R, 32, 32, g + OFF_BP), "rdl dbp");
    }
    return RD_OK;
}

int run_backward(rdl_trainer* t, const Path& p, const float* prev, const float* tgt, int64_t B, int64_t B_global) {
    const int64_t R = (int64_t)t->T * B;
    if (!p.loss_in_head) {   // else the head forward formed dY and the loss sums
        const int lblk = (int)((R + LOSS_BLOCK - 1) / LOSS_BLOCK);
        const bool fold = lblk == 1;   // a single loss block writes the metrics itself
        hipLaunchKernelGGL(loss_kernel, dim3(lblk), dim3(LOSS_BLOCK), 0, t->stream, (const float*)t->Y, tgt, t->dY, R,
                           t->cfg.loss, 1.0f / ((float)t->T * (float)B_global), t->lpart, t->ctl,
                           fold ? t->hist : nullptr, t->cfg.metrics_len);
        RD_HIP(hipGetLastError(), "rdl loss_kernel");
        if (!fold) {
            hipLaunchKernelGGL(metrics_kernel, dim3(1), dim3(256), 0, t->stream, (const float*)t->lpart, lblk, (float)R,
                               t->ctl, t->hist, t->cfg.metrics_len);
            RD_HIP(hipGetLastError(), "rdl metrics_kernel");
        }
    }
    if (int rc = p.fused_head ? head_backward_fused(t, p, B) : head_backward_layers(t, B)) return rc;
    int rc = RD_OK;
    switch (p.cell) {
        case Cell::Persistent: rc = cell_backward_persistent(t, prev, B); break;
        case Cell::StepF32: rc = cell_backward_step_f32(t, B); break;
        case Cell::StepBf16: rc = cell_backward_step_bf16(t, B); break;
    }
    if (rc) return rc;
    return dense32_backward(t, p, prev, B);
}

// one training pass over B windows: the path is decided here, once, for the forward and the backward
int run_train(rdl_trainer* t, const float* ob, const float* prev, const float* tgt, const float* state0, int64_t B,
              int64_t B_global) {
    const Path p = path_of(t, B, true);
    if (int rc = run_forward(t, p, ob, prev, state0, B, t->Y, tgt, B_global)) return rc;
    return run_backward(t, p, prev, tgt, B, B_global);
}

int launch_adam(rdl_trainer* t) {
    AdamArgs a{t->grad, t->params, t->wpack, t->m, t->v, t->ctl, t->cfg.lr, t->cfg.beta1, t->cfg.beta2, t->cfg.eps, t->np};
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((t->np + 255) / 256)), dim3(256), 0, t->stream, a);
    RD_HIP(hipGetLastError(), "rdl adam_kernel");
    return bf16_cell(t) ? bf16_images(t) : RD_OK;
}

bool bad_windows(const rdl_trainer* t, int64_t B) { return B <= 0 || B > t->Bmax; }

// (c, h) after the last step of the last forward over B windows: the rows of step T
int copy_final_state(rdl_trainer* t, int64_t B, float* state_out, const char* what) {
    const int64_t last = (int64_t)t->T * B * U;
    RD_HIP(hipMemcpyAsync(state_out, t->Cs + last, sizeof(float) * B * U, hipMemcpyDeviceToDevice, t->stream), what);
    RD_HIP(hipMemcpyAsync(state_out + B * U, t->H + last, sizeof(float) * B * U, hipMemcpyDeviceToDevice, t->stream),
           what);
    return RD_OK;
}

// the closed-loop kernels' packed image of Wl from the current parameters (student_lstm_query.h);
// the bf16 query reads the handle's forward image, which is current on the stream: no launch
int launch_eval_pack(rdl_trainer* t) {
    if (bf16_query(t)) return RD_OK;
    hipLaunchKernelGGL(lstm_eval_pack_kernel, dim3((EV_IMG + 255) / 256), dim3(256), 0, t->stream,
                       (const float*)t->params, t->eimg);
    RD_HIP(hipGetLastError(), "lstm_eval_pack_kernel launch");
    return RD_OK;
}

// ---------------------------------------------------------------- persistent envs
void free_envs(rdl_trainer* t) {
    t->envs.release();
    for (float* p : {t->env_q, t->env_hist})
        if (p) (void)hipFree(p);
    t->env_q = t->env_hist = nullptr;
}

LsEnvsArgs envs_args(const rdl_trainer* t) {
    LsEnvsArgs a{};
    a.n = t->envs.n;
    a.env_base = t->envs.base;
    a.seed = t->envs.seed;
    a.tnet = t->tnet;
    a.P = t->params;
    a.img = bf16_query(t) ? (const float*)t->wimg : t->eimg;
    a.state = t->envs.state;
    a.aux = t->envs.aux;
    a.clock = t->envs.clock;
    a.q = t->env_q;
    a.hist = t->env_hist;
    a.T = t->T;
    return a;
}

// The argument checks of rdl_envs_act / rdl_rollout_envs / rdl_step_envs, `fn` naming the caller:
// everything that needs no handle first, then what the handle says.  train: the two training calls
// (window buffers required, steps a multiple of the episode); *B: the windows the call writes.
int envs_check(const char* fn, const rdl_trainer* t, int act_with, int steps, const float* records, const float* ob_w,
               const float* prev_w, const float* t_w, bool train, int64_t* B) {
    if (!t) return rd::set_error(RD_EINVAL, "%s: null trainer", fn);
    if (!records) return rd::set_error(RD_EINVAL, "%s: null records", fn);
    if (steps < 1) return rd::set_error(RD_EINVAL, "%s: steps %d < 1", fn, steps);
    if (act_with != RDL_ACT_TEACHER && act_with != RDL_ACT_STUDENT)
        return rd::set_error(RD_EINVAL, "%s: unknown act_with %d", fn, act_with);
    if (train ? !ob_w || !prev_w || !t_w : (ob_w || prev_w || t_w) && (!ob_w || !prev_w || !t_w))
        return rd::set_error(RD_EINVAL, "%s: null ob_w, prev_w or t_w (the window buffers go together)", fn);
    if (!train && ob_w && *B < 1) return rd::set_error(RD_EINVAL, "%s: windows %lld < 1", fn, (long long)*B);
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "%s: no envs attached (rdl_envs_attach)", fn);
    if (!t->has_teacher) return rd::set_error(RD_EINVAL, "%s: no teacher set (rdl_set_teacher)", fn);
    if (t->T > EV_MAX_T)
        return rd::set_error(RD_EINVAL, "%s: rdl_config.steps = %d unrolled steps, the kernel keeps at most %d records "
                                        "of history", fn, t->T, EV_MAX_T);
    if (t->envs.n > ((int64_t)1 << 31) / steps)
        return rd::set_error(RD_EINVAL, "%s: steps x n_envs = %d x %lld rows > 2^31", fn, steps, (long long)t->envs.n);
    if (int rc = rd::check_bound_rows(fn, t->act, steps, t->envs.n)) return rc;
    if (train) {
        if (steps % rd::kEpisodeSteps)
            return rd::set_error(RD_EINVAL, "%s: steps %d is not a multiple of the episode's %d", fn, steps,
                                 rd::kEpisodeSteps);
        if (t->T > rd::kEpisodeSteps)
            return rd::set_error(RD_EINVAL, "%s: rdl_config.steps = %d exceeds the episode's %d steps", fn, t->T,
                                 rd::kEpisodeSteps);
        *B = t->envs.n * (steps / rd::kEpisodeSteps) * (rd::kEpisodeSteps + 1 - t->T);
        if (*B > t->Bmax)
            return rd::set_error(RD_EINVAL, "%s: %lld windows > rdl_config.max_windows = %lld", fn, (long long)*B,
                                 (long long)t->Bmax);
    }
    return RD_OK;
}

// K env steps of every env: a block of 16 envs per workgroup for the whole launch, one workgroup
// per CU (its LDS), as rdl_evaluate
int launch_envs(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w, float* prev_w,
                float* t_w, int64_t B) {
    const bool stu = act_with == RDL_ACT_STUDENT;
    if (stu)
        if (int rc = launch_eval_pack(t)) return rc;
    LsEnvsArgs a = envs_args(t);
    a.records = records;
    a.reward = reward;
    a.ob_w = ob_w;
    a.prev_w = prev_w;
    a.t_w = t_w;
    a.windows = ob_w ? B : 0;
    a.steps = steps;
    const int64_t nblk = (a.n + EV_ROWS - 1) / EV_ROWS, cap = t->envs.grid > 0 ? t->envs.grid : t->cus;
    const dim3 grid((unsigned)(nblk < cap ? nblk : cap)), block(EV_THREADS);
    auto* kern = !stu ? student_lstm_envs_kernel<false, false>
                 : bf16_query(t) ? student_lstm_envs_kernel<true, true> : student_lstm_envs_kernel<true, false>;
    const rd::LstmEnvsLaunch l{&a, &t->act, stu, bf16_query(t), grid.x, block.x, t->stream};
    switch (rd::tier_of(t->act, stu)) {
        case rd::Tier::Faulty: RD_HIP(rd::launch_lstm_envs_faulty(l), "student_lstm_envs_kernel (faulty) launch"); break;
        case rd::Tier::Noisy: RD_HIP(rd::launch_lstm_envs_noisy(l), "student_lstm_envs_kernel (noisy) launch"); break;
        case rd::Tier::Mixed: {   // these instances alone live in this unit
            auto* mixed = bf16_query(t) ? student_lstm_envs_kernel<true, true, LsEnvsMixArgs>
                                        : student_lstm_envs_kernel<true, false, LsEnvsMixArgs>;
            hipLaunchKernelGGL(mixed, grid, block, 0, t->stream, acting_args<LsEnvsMixArgs>(a, t->act));
            RD_HIP(hipGetLastError(), "student_lstm_envs_kernel (mixed) launch");
            break;
        }
        case rd::Tier::Plain:
            hipLaunchKernelGGL(kern, grid, block, 0, t->stream, a);
            RD_HIP(hipGetLastError(), "student_lstm_envs_kernel launch");
    }
    return RD_OK;
}

// act, then the training path on the B windows just written, as rdl_rollout / rdl_step run it
int envs_train(const char* fn, rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w,
               float* prev_w, float* t_w, int adam) {
    int64_t B = 0;
    if (int rc = envs_check(fn, t, act_with, steps, records, ob_w, prev_w, t_w, true, &B)) return rc;
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, fn);
    if (int rc = launch_envs(t, act_with, steps, records, reward, ob_w, prev_w, t_w, B)) return rc;
    if (int rc = run_train(t, ob_w, prev_w, t_w, nullptr, B, B)) return rc;
    return adam ? launch_adam(t) : RD_OK;
}

}  // namespace

extern "C" {

int64_t rdl_param_count(int32_t steps) { return steps > 0 ? params_of(steps) : -1; }

int rdl_create(rdl_trainer** out, const rdl_config* cfg, int device, void* hip_stream) {
    return rdl_create_dtype(out, cfg, RDL_DTYPE_F32, device, hip_stream);
}

int rdl_create_dtype(rdl_trainer** out, const rdl_config* cfg, int32_t dtype, int device, void* hip_stream) {
    if (!out || !cfg) return rd::set_error(RD_EINVAL, "rdl_create: null argument");
    if (dtype != RDL_DTYPE_F32 && dtype != RDL_DTYPE_BF16)
        return rd::set_error(RD_EINVAL, "rdl_create_dtype: unknown dtype %d", (int)dtype);
    if ((cfg->loss != RDL_LOSS_MSE && cfg->loss != RDL_LOSS_KL) || !(cfg->lr > 0) || cfg->steps <= 0 ||
        cfg->max_windows <= 0 || (int64_t)cfg->steps * cfg->max_windows > ((int64_t)1 << 22) || cfg->metrics_len < 0 ||
        !(cfg->keep_prob > 0.0f && cfg->keep_prob <= 1.0f) || cfg->row_base < 0 ||
        (cfg->kernels & ~(RDL_KERNELS_STEP_RECURRENCE | RDL_KERNELS_LAYER_HEAD)))
        return rd::set_error(RD_EINVAL, "rdl_create: bad config");
    rd::DeviceGuard dg(device);
    RD_HIP(dg.err, "rdl_create: hipSetDevice");
    rdl_trainer* t = new (std::nothrow) rdl_trainer();
    if (!t) return rd::set_error(RD_EINVAL, "rdl_create: out of host memory");
    t->cfg = *cfg;
    if (t->cfg.metrics_len == 0) t->cfg.metrics_len = 4096;
    t->device = device;
    t->cus = rd::cu_count(device);
    t->stream = (hipStream_t)hip_stream;
    t->T = cfg->steps;
    t->dtype = dtype;
    t->np = params_of(t->T);
    t->Bmax = cfg->max_windows;
    const int64_t R = (int64_t)t->T * t->Bmax, B = t->Bmax;
    const int64_t nch = (R + COLSUM_CHUNK - 1) / COLSUM_CHUNK;
    t->colws_floats = nch * G4;
    rd::DeviceAllocs& mem = t->mem;
    mem.stream = t->stream;
    mem.zeroed(&t->params, t->np);
    mem.zeroed(&t->m, t->np);
    mem.zeroed(&t->v, t->np);
    mem.zeroed(&t->own_grad, t->np);
    mem.zeroed(&t->X, R * XLD);
    mem.zeroed(&t->H, (R + B) * U);
    mem.zeroed(&t->Cs, (R + B) * U);
    mem.zeroed(&t->Z, R * G4);
    mem.zeroed(&t->G, R * G4);
    mem.zeroed(&t->A1, R * L1);
    mem.zeroed(&t->A2, R * L2);
    mem.zeroed(&t->A3, R * L3);
    mem.zeroed(&t->A4, R * L4);
    mem.zeroed(&t->Y, R * 4);
    mem.zeroed(&t->dY, R * 4);
    mem.zeroed(&t->D32, R * H4);
    mem.zeroed(&t->D64a, R * H3);
    mem.zeroed(&t->D128, R * H2);
    mem.zeroed(&t->D64b, R * H1);
    mem.zeroed(&t->dHh, R * U);
    mem.zeroed(&t->dP, R * 32);
    mem.zeroed(&t->dhn, B * U);
    mem.zeroed(&t->dc, B * U);
    mem.zeroed(&t->split, SPLIT_FLOATS);
    int64_t nbmax = 0;   // the most workgroups of any batch up to Bmax (head_nb is not monotone)
    for (int64_t b = HF_ROWS; b < t->Bmax + HF_ROWS; b += HF_ROWS) nbmax = std::max<int64_t>(nbmax, head_nb(t->T, b));
    const int64_t hp = (int64_t)t->T * nbmax * HB_PART;
    if (hp <= HPART_MAX_FLOATS) mem.zeroed(&t->hpart, hp);
    mem.zeroed(&t->wpack, (int64_t)t->T * HWP);
    mem.zeroed(&t->colws, t->colws_floats);
    mem.zeroed(&t->lpart, std::max<int64_t>(2 * ((R + LOSS_BLOCK - 1) / LOSS_BLOCK), 2 * HB_WIDE_GRID));
    mem.zeroed(&t->hist, (int64_t)t->cfg.metrics_len * N_MET);
    mem.raw(&t->ctl, 8);
    mem.raw(&t->bar, 4);
    mem.zeroed(&t->bpart, (int64_t)2 * PR_GRID * PB_PART);
    mem.zeroed(&t->hx, (size_t)2 * PR_ROWS * U);
    mem.zeroed(&t->qbuf, 4 * G4);
    mem.zeroed(&t->tnet, tch::P_TOT + 2 * tch::OBD);
    mem.zeroed(&t->eimg, EV_IMG);
    if (bf16_cell(t)) {
        mem.raw(&t->wimg, BF_IMG_GROUPS);
        mem.zeroed(&t->wpart, std::min<int64_t>(BF_WG_SPLITS, (R + BF_WG_CHUNK - 1) / BF_WG_CHUNK) * BF_KWL * G4);
    }
    hipError_t e = mem.err;
    if (e == hipSuccess) e = hipMemsetAsync(t->bar, 0, sizeof(uint32_t) * 4, t->stream);
    t->grad = t->own_grad;
    if (e != hipSuccess) {
        rdl_destroy(t);
        return rd::hip_fail(e, "rdl_create: allocation");
    }
    {   // the ones columns of the head activations (the head GEMMs write columns 0..H_l-1)
        const unsigned gr = (unsigned)((R + 255) / 256);
        hipLaunchKernelGGL(ones_column_kernel, dim3(gr), dim3(256), 0, t->stream, t->A1, R, L1, H1);
        hipLaunchKernelGGL(ones_column_kernel, dim3(gr), dim3(256), 0, t->stream, t->A2, R, L2, H2);
        hipLaunchKernelGGL(ones_column_kernel, dim3(gr), dim3(256), 0, t->stream, t->A3, R, L3, H3);
        hipLaunchKernelGGL(ones_column_kernel, dim3(gr), dim3(256), 0, t->stream, t->A4, R, L4, H4);
        if ((e = hipGetLastError()) != hipSuccess) {
            rdl_destroy(t);
            return rd::hip_fail(e, "rdl_create: ones columns");
        }
    }
    if (int rc = rdl_reset(t)) {
        rdl_destroy(t);
        return rc;
    }
    if (bf16_cell(t))   // the images of the zero master
        if (int rc = bf16_images(t)) {
            rdl_destroy(t);
            return rc;
        }
    *out = t;
    return RD_OK;
}

int rdl_set_query_dtype(rdl_trainer* t, int32_t dtype) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_set_query_dtype: null trainer");
    if (dtype != RDL_DTYPE_F32 && dtype != RDL_DTYPE_BF16)
        return rd::set_error(RD_EINVAL, "rdl_set_query_dtype: unknown dtype %d", (int)dtype);
    if (dtype == RDL_DTYPE_BF16 && !bf16_cell(t))
        return rd::set_error(RD_EINVAL, "rdl_set_query_dtype: dtype RDL_DTYPE_BF16 needs a handle created with "
                                        "RDL_DTYPE_BF16 (rdl_create_dtype): an f32 handle keeps no bf16 image of Wl");
    t->qdtype = dtype;
    return RD_OK;
}

int rdl_query_dtype(const rdl_trainer* t) { return t ? t->qdtype : -1; }

int rdl_destroy(rdl_trainer* t) {
    if (!t) return RD_OK;
    rd::DeviceGuard dg(t->device);
    t->mem.free_all();
    free_envs(t);
    delete t;
    return RD_OK;
}

int rdl_set_stream(rdl_trainer* t, void* hip_stream) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_set_stream: null handle");
    t->stream = (hipStream_t)hip_stream;
    return RD_OK;
}

int rdl_set_params(rdl_trainer* t, const float* params) {
    if (!t || !params) return rd::set_error(RD_EINVAL, "rdl_set_params: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_set_params");
    RD_HIP(hipMemcpyAsync(t->params, params, sizeof(float) * t->np, hipMemcpyDeviceToDevice, t->stream),
           "rdl_set_params");
    const int64_t n = (int64_t)t->T * HSZ;
    hipLaunchKernelGGL(pack_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream,
                       (const float*)t->params, t->wpack, t->T);
    RD_HIP(hipGetLastError(), "rdl_set_params: pack_heads_kernel");
    return bf16_cell(t) ? bf16_images(t) : RD_OK;
}

int rdl_get_params(rdl_trainer* t, float* params) {
    if (!t || !params) return rd::set_error(RD_EINVAL, "rdl_get_params: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_get_params");
    RD_HIP(hipMemcpyAsync(params, t->params, sizeof(float) * t->np, hipMemcpyDeviceToDevice, t->stream),
           "rdl_get_params");
    return RD_OK;
}

int rdl_get_slots(rdl_trainer* t, float* m, float* v) {
    if (!t || !m || !v) return rd::set_error(RD_EINVAL, "rdl_get_slots: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_get_slots");
    RD_HIP(hipMemcpyAsync(m, t->m, sizeof(float) * t->np, hipMemcpyDeviceToDevice, t->stream), "rdl_get_slots");
    RD_HIP(hipMemcpyAsync(v, t->v, sizeof(float) * t->np, hipMemcpyDeviceToDevice, t->stream), "rdl_get_slots");
    return RD_OK;
}

int rdl_set_slots(rdl_trainer* t, const float* m, const float* v) {
    if (!t || !m || !v) return rd::set_error(RD_EINVAL, "rdl_set_slots: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_set_slots");
    RD_HIP(hipMemcpyAsync(t->m, m, sizeof(float) * t->np, hipMemcpyDeviceToDevice, t->stream), "rdl_set_slots");
    RD_HIP(hipMemcpyAsync(t->v, v, sizeof(float) * t->np, hipMemcpyDeviceToDevice, t->stream), "rdl_set_slots");
    return RD_OK;
}

int rdl_reset(rdl_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_reset: null handle");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_reset");
    RD_HIP(hipMemsetAsync(t->m, 0, sizeof(float) * t->np, t->stream), "rdl_reset");
    RD_HIP(hipMemsetAsync(t->v, 0, sizeof(float) * t->np, t->stream), "rdl_reset");
    hipLaunchKernelGGL(init_ctl_kernel, dim3(1), dim3(64), 0, t->stream, t->ctl, t->cfg.beta1, t->cfg.beta2);
    RD_HIP(hipGetLastError(), "rdl_reset");
    return RD_OK;
}

int rdl_forward(rdl_trainer* t, const float* ob, const float* prev_pdflat, const float* state0, int64_t windows,
                float* pdflat, float* state_out) {
    if (!t || !ob || !prev_pdflat || !pdflat || bad_windows(t, windows))
        return rd::set_error(RD_EINVAL, "rdl_forward: bad argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_forward");
    if (int rc = run_forward(t, path_of(t, windows, false), ob, prev_pdflat, state0, windows, pdflat)) return rc;
    return state_out ? copy_final_state(t, windows, state_out, "rdl_forward: state") : RD_OK;
}

int rdl_final_state(rdl_trainer* t, int64_t windows, float* state_out) {
    if (!t || !state_out || windows <= 0 || windows != t->last_B)
        return rd::set_error(RD_EINVAL, "rdl_final_state: no forward pass of %lld windows to read",
                             (long long)windows);
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_final_state");
    return copy_final_state(t, windows, state_out, "rdl_final_state");
}

int rdl_rollout(rdl_trainer* t, const float* ob, const float* prev_pdflat, const float* t_pdflat,
                const float* state0, int64_t windows, int64_t windows_global) {
    if (!t || !ob || !prev_pdflat || !t_pdflat || bad_windows(t, windows) || windows_global < windows)
        return rd::set_error(RD_EINVAL, "rdl_rollout: bad argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_rollout");
    return run_train(t, ob, prev_pdflat, t_pdflat, state0, windows, windows_global);
}

int rdl_apply(rdl_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_apply: null handle");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_apply");
    return launch_adam(t);
}

int rdl_step(rdl_trainer* t, const float* ob, const float* prev_pdflat, const float* t_pdflat, const float* state0,
             int64_t windows) {
    if (int rc = rdl_rollout(t, ob, prev_pdflat, t_pdflat, state0, windows, windows)) return rc;
    return launch_adam(t);
}

float* rdl_grad_buffer(rdl_trainer* t) { return t ? t->grad : nullptr; }

int rdl_bind_grad_buffer(rdl_trainer* t, float* grad) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_bind_grad_buffer: null handle");
    t->grad = grad ? grad : t->own_grad;
    return RD_OK;
}

int rdl_head_path(const rdl_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_head_path: null handle");
    return (t->cfg.kernels & RDL_KERNELS_LAYER_HEAD) || !t->hpart ? 0 : 1;
}

int rdl_get_counter(rdl_trainer* t, int64_t* opt_steps) {
    if (!t || !opt_steps) return rd::set_error(RD_EINVAL, "rdl_get_counter: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_get_counter");
    uint32_t c[8], b[4];
    RD_HIP(hipMemcpyAsync(c, t->ctl, sizeof(c), hipMemcpyDeviceToHost, t->stream), "rdl_get_counter");
    RD_HIP(hipMemcpyAsync(b, t->bar, sizeof(b), hipMemcpyDeviceToHost, t->stream), "rdl_get_counter");
    RD_HIP(hipStreamSynchronize(t->stream), "rdl_get_counter");
    if (b[2])   // a persistent launch gave up at a grid barrier (workgroups not co-resident)
        return rd::set_error(RD_EINVAL, "rdl: a persistent recurrence launch timed out at its grid barrier; "
                                        "the steps since are invalid (rdl_config.kernels = RDL_KERNELS_STEP_RECURRENCE avoids the persistent kernels)");
    *opt_steps = c[0];
    return RD_OK;
}

int rdl_read_metrics(rdl_trainer* t, int64_t count, double* out) {
    if (!t || !out || count < 0) return rd::set_error(RD_EINVAL, "rdl_read_metrics: bad argument");
    int64_t steps = 0;
    if (int rc = rdl_get_counter(t, &steps)) return rc;
    return rd::read_ring("rdl_read_metrics", "steps", t->hist, t->cfg.metrics_len, N_MET, steps, count, out);
}

int rdl_set_teacher(rdl_trainer* t, const float* params, const float* ob_mean, const float* ob_std) {
    if (!t || !params || !ob_mean || !ob_std) return rd::set_error(RD_EINVAL, "rdl_set_teacher: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_set_teacher");
    if (int rc = rd::upload_net("rdl_set_teacher", t->tnet, params, tch::P_TOT, ob_mean, ob_std, tch::OBD, t->stream))
        return rc;
    t->has_teacher = true;
    return RD_OK;
}

}  // extern "C"

namespace {

// rdl_evaluate (nz = of = null), rdl_evaluate_noisy (of = null) and rdl_evaluate_faulty (nz = null: the
// mean acts), `fn` naming the caller; the tier follows from the settings given (rd::tier_of)
int evaluate(const char* fn, rdl_trainer* t, const rdl_eval_config* cfg, const rd_action_noise* nz,
             const rd_obs_faults* of, const float* state0,
             float* returns, float* final_dist, float* records, float* state_out) {
    if (!t || !cfg || !returns) return rd::set_error(RD_EINVAL, "%s: null trainer, config or returns", fn);
    if (cfg->n_envs < 1 || cfg->n_envs > ((int64_t)1 << 31))
        return rd::set_error(RD_EINVAL, "%s: n_envs %lld outside 1 .. 2^31", fn, (long long)cfg->n_envs);
    if (cfg->episodes < 1) return rd::set_error(RD_EINVAL, "%s: episodes %d < 1", fn, cfg->episodes);
    if (cfg->env_base < 0 || cfg->first_episode < 0 || cfg->grid < 0)
        return rd::set_error(RD_EINVAL, "%s: negative env_base, first_episode or grid", fn);
    if (!t->has_teacher) return rd::set_error(RD_EINVAL, "%s: no teacher set (rdl_set_teacher)", fn);
    if (t->T > EV_MAX_T)
        return rd::set_error(RD_EINVAL, "%s: %d unrolled steps, the kernel keeps at most %d records of history", fn,
                             t->T, EV_MAX_T);
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, fn);
    if (int rc = launch_eval_pack(t)) return rc;
    LsEvalArgs a;
    a.n = cfg->n_envs;
    a.env_base = cfg->env_base;
    a.seed = cfg->seed;
    a.tnet = t->tnet;
    a.P = t->params;
    a.img = bf16_query(t) ? (const float*)t->wimg : t->eimg;
    a.draws = cfg->draws;
    a.state0 = state0;
    a.returns = returns;
    a.final_dist = final_dist;
    a.records = records;
    a.state_out = state_out;
    a.episodes = cfg->episodes;
    a.first_episode = cfg->first_episode;
    a.T = t->T;
    // a block of 16 envs per workgroup for the whole launch, one workgroup per CU (its LDS)
    const int64_t nblk = (a.n + EV_ROWS - 1) / EV_ROWS, cap = cfg->grid > 0 ? cfg->grid : t->cus;
    auto* kern = bf16_query(t) ? student_lstm_evaluate_kernel<true> : student_lstm_evaluate_kernel<false>;
    rd::Acting act;
    if (nz) act.noise = *nz;
    if (of) act.faults = *of;
    const rd::LstmEvalLaunch l{&a, &act, bf16_query(t), (unsigned)(nblk < cap ? nblk : cap), EV_THREADS, t->stream};
    switch (rd::tier_of(act, true)) {
        case rd::Tier::Faulty: RD_HIP(rd::launch_lstm_eval_faulty(l), "student_lstm_evaluate_kernel (faulty) launch"); break;
        case rd::Tier::Noisy: RD_HIP(rd::launch_lstm_eval_noisy(l), "student_lstm_evaluate_kernel (noisy) launch"); break;
        default:
            hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, t->stream, a);
            RD_HIP(hipGetLastError(), "student_lstm_evaluate_kernel launch");
    }
    return RD_OK;
}

}  // namespace

extern "C" {

int rdl_evaluate(rdl_trainer* t, const rdl_eval_config* cfg, const float* state0, float* returns, float* final_dist,
                 float* records, float* state_out) {
    return evaluate("rdl_evaluate", t, cfg, nullptr, nullptr, state0, returns, final_dist, records, state_out);
}

int rdl_evaluate_noisy(rdl_trainer* t, const rdl_eval_config* cfg, const rd_action_noise* nz, const float* state0,
                       float* returns, float* final_dist, float* records, float* state_out) {
    if (int rc = rd::check_action_noise("rdl_evaluate_noisy", nz, false)) return rc;
    return evaluate("rdl_evaluate_noisy", t, cfg, nz, nullptr, state0, returns, final_dist, records, state_out);
}

int rdl_evaluate_faulty(rdl_trainer* t, const rdl_eval_config* cfg, const rd_obs_faults* of, const rd_action_noise* nz,
                        const float* state0, float* returns, float* final_dist, float* records, float* state_out) {
    if (int rc = rd::check_obs_faults("rdl_evaluate_faulty", of, false)) return rc;
    if (nz) {
        if (int rc = rd::check_action_noise("rdl_evaluate_faulty", nz, true)) return rc;
    }
    return evaluate("rdl_evaluate_faulty", t, cfg, nz, of, state0, returns, final_dist, records, state_out);
}

int rdl_envs_reset(rdl_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdl_envs_reset: null trainer");
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "rdl_envs_reset: no envs attached (rdl_envs_attach)");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_envs_reset");
    const size_t n = (size_t)t->envs.n;
    RD_HIP(hipMemsetAsync(t->env_q, 0, sizeof(float) * 2 * n * U, t->stream), "rdl_envs_reset: query state");
    RD_HIP(hipMemsetAsync(t->env_hist, 0, sizeof(float) * n * t->T * EH_REC, t->stream), "rdl_envs_reset: history");
    hipLaunchKernelGGL(student_lstm_envs_reset_kernel, dim3((unsigned)((t->envs.n + 255) / 256)), dim3(256), 0, t->stream,
                       envs_args(t));
    RD_HIP(hipGetLastError(), "student_lstm_envs_reset_kernel launch");
    return RD_OK;
}

int rdl_envs_attach(rdl_trainer* t, const rdl_envs_config* cfg) {
    if (int rc = rd::envs_attach_check("rdl_envs_attach", t, cfg)) return rc;
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_envs_attach");
    if (t->envs.state) {   // replace: launches that still read the old envs finish first
        RD_HIP(hipStreamSynchronize(t->stream), "rdl_envs_attach");
        free_envs(t);
    }
    const size_t n = (size_t)cfg->n_envs;
    hipError_t e = rd::envs_alloc(t->envs, *cfg, rd::kStateDim, ENV_AUX);
    if (e == hipSuccess) e = hipMalloc((void**)&t->env_q, sizeof(float) * 2 * n * U);
    if (e == hipSuccess) e = hipMalloc((void**)&t->env_hist, sizeof(float) * n * t->T * EH_REC);
    if (e != hipSuccess) {
        free_envs(t);
        return rd::hip_fail(e, "rdl_envs_attach: allocation");
    }
    return rdl_envs_reset(t);
}

int rdl_envs_act(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w, float* prev_w,
                 float* t_w, int64_t windows) {
    int64_t B = windows;
    if (int rc = envs_check("rdl_envs_act", t, act_with, steps, records, ob_w, prev_w, t_w, false, &B)) return rc;
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_envs_act");
    return launch_envs(t, act_with, steps, records, reward, ob_w, prev_w, t_w, B);
}

int rdl_rollout_envs(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w, float* prev_w,
                     float* t_w) {
    return envs_train("rdl_rollout_envs", t, act_with, steps, records, reward, ob_w, prev_w, t_w, 0);
}

int rdl_step_envs(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w, float* prev_w,
                  float* t_w) {
    return envs_train("rdl_step_envs", t, act_with, steps, records, reward, ob_w, prev_w, t_w, 1);
}

// how the envs calls act: the checks and the settings are rd_acting.h's
int rdl_envs_set_teacher_share(rdl_trainer* t, float beta, uint64_t coin_seed) {
    return rd::set_teacher_share("rdl_envs_set_teacher_share", rd::acting_of(t), beta, coin_seed);
}

float rdl_envs_teacher_share(const rdl_trainer* t) { return rd::teacher_share(rd::acting_of(t)); }

int rdl_envs_set_action_noise(rdl_trainer* t, const rd_action_noise* nz) {
    return rd::set_action_noise("rdl_envs_set_action_noise", rd::acting_of(t), nz);
}

int rdl_envs_action_noise(const rdl_trainer* t, rd_action_noise* out) {
    return rd::get_action_noise("rdl_envs_action_noise", rd::acting_of(t), out);
}

int rdl_envs_bind_actions(rdl_trainer* t, float* buf, int64_t rows) {
    return rd::bind_actions("rdl_envs_bind_actions", rd::acting_of(t), buf, rows);
}

int rdl_envs_set_obs_faults(rdl_trainer* t, const rd_obs_faults* of) {
    return rd::set_obs_faults("rdl_envs_set_obs_faults", rd::acting_of(t), of);
}

int rdl_envs_obs_faults(const rdl_trainer* t, rd_obs_faults* out) {
    return rd::get_obs_faults("rdl_envs_obs_faults", rd::acting_of(t), out);
}

int rdl_envs_get_state(rdl_trainer* t, float* state, int32_t* step, int32_t* episode) {
    if (!t || !state) return rd::set_error(RD_EINVAL, "rdl_envs_get_state: null trainer or state");
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "rdl_envs_get_state: no envs attached (rdl_envs_attach)");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_envs_get_state");
    return rd::envs_get_state("rdl_envs_get_state", t->envs, rd::kStateDim, t->stream, state, step, episode);
}

int rdl_envs_get_query_state(rdl_trainer* t, float* state_out) {
    if (!t || !state_out) return rd::set_error(RD_EINVAL, "rdl_envs_get_query_state: null trainer or state_out");
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "rdl_envs_get_query_state: no envs attached (rdl_envs_attach)");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdl_envs_get_query_state");
    RD_HIP(hipMemcpyAsync(state_out, t->env_q, sizeof(float) * 2 * t->envs.n * U, hipMemcpyDeviceToDevice, t->stream),
           "rdl_envs_get_query_state: copy");
    return RD_OK;
}

}  // extern "C"
