// student_mlp.hip's layout: the network's dimensions, the flat parameter vector (pw), the gradient
// workspace (gw, gb) and the padded weight image (fw; PW .. BB), the metrics row, the column
// permutation pk, the LDS row strides and buffers of a row block (Lay<ROWS>) and the split of a
// layer's output blocks over the eight waves (Part).  Every other student_mlp_*.h reads these.
// Included first inside student_mlp.hip's anonymous namespace; expects
// include/reacher_student_mlp.h (RDM_*).
#pragma once

namespace sm {

constexpr int NL = 5;
constexpr int IN[NL] = {16, 24, 128, 128, 32};
constexpr int OUT[NL] = {24, 128, 128, 32, 4};
constexpr int KP[NL] = {16, 32, 128, 128, 32};   // padded fan-in  (multiple of 16)
constexpr int MP[NL] = {32, 128, 128, 32, 16};   // padded fan-out (multiple of 16)
constexpr bool TANH[NL] = {true, true, false, true, false};

// flat parameter vector: per layer W[in][out] then b[out] (tf.layers.dense order)
constexpr int pw(int l) { return l == 0 ? 0 : pw(l - 1) + IN[l - 1] * OUT[l - 1] + OUT[l - 1]; }
constexpr int P_REF = pw(NL);
static_assert(P_REF == RDM_PARAMS, "flat layout");
// gradient workspace: per layer dW[KP][MP] (row-major) then db[MP]
constexpr int gw(int l) { return l == 0 ? 0 : gw(l - 1) + KP[l - 1] * MP[l - 1] + MP[l - 1]; }
constexpr int gb(int l) { return gw(l) + KP[l] * MP[l]; }
constexpr int GIMG = gw(NL);                    // 25,936
// weight image (zero padding that stays zero): per layer
//   forward  FW[L]: W[k][c] at ((k/16) MP + c) 16 + 4 (k%4) + (k/4)%4
//   backward BW[L]: W[k][c] at ((c/16) KP + k) 16 + 4 (c%4) + (c/4)%4
//   bias     BB[L]: b[c] at c
// so the B operand of 4 consecutive k-steps (k = 16 S + 4 sub + g, sub = 0..3) is one 16-B
// load per lane, in both the forward (K = fan-in) and the backward (K = fan-out) GEMMs.
constexpr int fw(int l) { return l == 0 ? 0 : fw(l - 1) + 2 * KP[l - 1] * MP[l - 1] + MP[l - 1]; }
constexpr int IMG = fw(NL);                     // 51,808
constexpr int PW[NL + 1] = {pw(0), pw(1), pw(2), pw(3), pw(4), pw(5)};
constexpr int GW[NL] = {gw(0), gw(1), gw(2), gw(3), gw(4)};
constexpr int GB[NL] = {gb(0), gb(1), gb(2), gb(3), gb(4)};
constexpr int FW[NL] = {fw(0), fw(1), fw(2), fw(3), fw(4)};
constexpr int BW[NL] = {fw(0) + KP[0] * MP[0], fw(1) + KP[1] * MP[1], fw(2) + KP[2] * MP[2], fw(3) + KP[3] * MP[3],
                        fw(4) + KP[4] * MP[4]};
constexpr int BB[NL] = {BW[0] + KP[0] * MP[0], BW[1] + KP[1] * MP[1], BW[2] + KP[2] * MP[2], BW[3] + KP[3] * MP[3],
                        BW[4] + KP[4] * MP[4]};
constexpr int N_MET = 4;                        // loss, sq err, rows, 0
constexpr int WS_ROW = GIMG + N_MET;

// Activations are stored with the columns of every 16-group permuted, k -> pk(k), so that
// the A operand of 4 consecutive k-steps (k = 16 S + 4 sub + g) is one ds_read_b128.
__host__ __device__ constexpr int pk(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }

constexpr int WAVES = 8, BLOCK = 64 * WAVES;

// LDS buffers [row][pk(feature)], stride = width + 4
constexpr int S_X0 = 20, S_X1 = 36, S_X2 = 132, S_X3 = 132, S_X4 = 36, S_D5 = 20, S_D4 = 36, S_DA = 132;
// Row block of ROWS rows per workgroup pass: 64 (the throughput kernel) or 16 (small
// batches, e.g. the reference's 200-row step: 13 workgroups in parallel instead of 4).
template <int ROWS>
struct Lay {
    static constexpr int RB = ROWS / 16;                   // 16-row MFMA blocks of a row block
    static constexpr int O_X0 = 0;
    static constexpr int O_X1 = O_X0 + ROWS * S_X0;
    static constexpr int O_X2 = O_X1 + ROWS * S_X1;
    static constexpr int O_X3 = O_X2 + ROWS * S_X2;
    static constexpr int O_X4 = O_X3 + ROWS * S_X3;
    static constexpr int O_D5 = O_X4 + ROWS * S_X4;        // layer-5 outputs, then dZ5
    static constexpr int O_D4 = O_D5 + ROWS * S_D5;        // dZ4
    static constexpr int O_DA = O_D4 + ROWS * S_D4;        // dZ3, later dZ1
    static constexpr int LDS_FLOATS = O_DA + ROWS * S_DA;  // 34,816 floats = 136 KiB at 64 rows
    static_assert(ROWS % 16 == 0 && ROWS * 4 <= BLOCK && LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
};
static_assert(S_X0 == KP[0] + 4 && S_X1 == KP[1] + 4 && S_X2 == KP[2] + 4 && S_X3 == KP[3] + 4 &&
                  S_X4 == KP[4] + 4 && S_D5 == MP[4] + 4 && S_D4 == MP[3] + 4 && S_DA == MP[2] + 4,
              "buffer strides");

}  // namespace sm

using namespace sm;

// Output blocks of a [ROWS x 16*NCB] result (RB = ROWS / 16), split over the 8 waves: for
// NCB >= 8 a wave owns NCB/8 column blocks x all RB row blocks (the B operand is shared by
// its row blocks); for NCB < 8 a wave owns at most one block.
template <int NCB, int RB>
struct Part {
    static constexpr int CPW = NCB >= WAVES ? NCB / WAVES : 1;
    static constexpr int RPW = NCB >= WAVES ? RB : 1;
    static_assert(NCB < WAVES || NCB % WAVES == 0, "partition");
    __device__ static bool active(int wave) { return NCB >= WAVES || wave < RB * NCB; }
    __device__ static int rb(int wave, int r) { return NCB >= WAVES ? r : wave % RB; }
    __device__ static int cb(int wave, int c) { return NCB >= WAVES ? wave * CPW + c : wave / RB; }
};
