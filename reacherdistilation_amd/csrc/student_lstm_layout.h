// student_lstm.hip's layout: the network's dimensions, the row strides of its activation buffers, the
// flat parameter offsets (params_of, with their static_asserts), the metrics row, the block sizes
// that the host sizes buffers by, sigm, and the SrcC fence's names.  Every other student_lstm_*.h
// reads these.  Included first inside student_lstm.hip's anonymous namespace; expects
// include/reacher_student_lstm.h (RDL_*) and rd_device.h.
#pragma once

constexpr int U = RDL_UNITS;            // 200
constexpr int G4 = 4 * U;                // 800 gates
constexpr int XI = 11 + 32;              // 43 cell inputs
constexpr int XLD = 44;                  // X row stride (16-B rows)
constexpr int H1 = 64, H2 = 128, H3 = 64, H4 = 32;
// head activations A_l are stored [row][H_l + 4] with column H_l = 1, so the next layer's
// weight-gradient GEMM over H_l + 1 rows of A^T yields [dW; db] in the flat [W | b] layout
// (tf.layers.dense order) in one launch, no column-sum pass
constexpr int L1 = H1 + 4, L2 = H2 + 4, L3 = H3 + 4, L4 = H4 + 4;

// flat parameter offsets (variable-creation order): the shared part, then the T heads; OFF_W1 ..
// OFF_B5 are offsets inside a head (head t at OFF_H + t HSZ)
constexpr int OFF_WP = 0;
constexpr int OFF_BP = OFF_WP + 4 * 32;
constexpr int OFF_WL = OFF_BP + 32;
constexpr int OFF_BL = OFF_WL + (XI + U) * G4;
constexpr int OFF_H = OFF_BL + G4;
constexpr int OFF_W1 = 0;
constexpr int OFF_B1 = OFF_W1 + U * H1;
constexpr int OFF_W2 = OFF_B1 + H1;
constexpr int OFF_B2 = OFF_W2 + H1 * H2;
constexpr int OFF_W3 = OFF_B2 + H2;
constexpr int OFF_B3 = OFF_W3 + H2 * H3;
constexpr int OFF_W4 = OFF_B3 + H3;
constexpr int OFF_B4 = OFF_W4 + H3 * H4;
constexpr int OFF_W5 = OFF_B4 + H4;
constexpr int OFF_B5 = OFF_W5 + H4 * 4;
constexpr int HSZ = OFF_B5 + 4;                 // 31,652 floats per head
static_assert(OFF_H == RDL_CELL_PARAMS && HSZ == RDL_HEAD_PARAMS && RDL_PARAMS == OFF_H + 10 * HSZ, "flat layout");
static_assert(OFF_WL % 4 == 0 && OFF_H % 4 == 0 && HSZ % 4 == 0 && OFF_W2 % 4 == 0 && OFF_W3 % 4 == 0 &&
                  OFF_W4 % 4 == 0 && OFF_W5 % 4 == 0 && (OFF_WL + XI * G4) % 4 == 0,
              "16-B aligned weight matrices");
__host__ __device__ constexpr int64_t params_of(int T) { return OFF_H + (int64_t)T * HSZ; }

constexpr int N_MET = 4;
constexpr int LOSS_BLOCK = 256;
constexpr int COLSUM_CHUNK = 512;         // rows per first-level column-sum block

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// SrcC fence around MFMA chains (rd_device.h), every operand in registers before they start: the
// head's data gradients (sixteen-wave head backward, round 5), the persistent BPTT's weight gradients
using rd::fence_begin, rd::fence_end;
