// distill.hip, part 1 of 5: the layouts.  Flat parameter vector (P_*), the LDS images of a net in
// the exact-f32 (N_*), bf16 (NB_*) and split (NX_*) modes with Off<> and img_t / img_s, the
// rollout's per-pair scratch (P_S*) and its final-reduction rows (RROW / ridx).  Constants only;
// needs <stdint.h>, and is included inside distill.hip's anonymous namespace like the other parts.
#pragma once

// flat parameters of one MlpPolicy: W1 | b1 | W2 | b2 | W3 | b3 | logstd
constexpr int OBD = 11, HID = 64, ACD = 2;
constexpr int P_W1 = 0;
constexpr int P_B1 = P_W1 + OBD * HID;   // 704
constexpr int P_W2 = P_B1 + HID;         // 768
constexpr int P_B2 = P_W2 + HID * HID;   // 4864
constexpr int P_W3 = P_B2 + HID;         // 4928
constexpr int P_B3 = P_W3 + HID * ACD;   // 5056
constexpr int P_LS = P_B3 + ACD;         // 5058
constexpr int P_TOT = P_LS + ACD;        // 5060
constexpr int P_PAD = P_TOT + 4;         // + metrics: reward, loss, sq err, envs
constexpr int N_MET = 4;

constexpr int WAVES = 8, BLOCK = 64 * WAVES;   // rollout: 2 waves per SIMD
constexpr int FWAVES = 4, FBLOCK = 64 * FWAVES; // forward_kernel
constexpr int GROUP = 64;                      // envs per wave pass (one per lane)
constexpr int TILE = 16;                       // envs per MFMA tile

// ---------------------------------------------------------------- LDS image of a net
// Weight images are [k][j][fb] = W[k][16 fb + j]: the four A operands a lane needs for one
// k-step (output blocks fb = 0..3, row j) are one 16-B ds_read_b128, and a 16-lane group
// reads one contiguous 256-B row: conflict-free, no padding.
constexpr int N_W1 = 0;                  // [12][16][4]: rows 0..10 = W1, row 11 = b1
constexpr int N_W2 = N_W1 + 12 * HID;    // [64][16][4]
constexpr int N_B2 = N_W2 + HID * HID;   // [64]
constexpr int N_W3 = N_B2 + HID;         // [64][2]
constexpr int N_B3 = N_W3 + HID * ACD;   // [2]
constexpr int N_LS = N_B3 + ACD;         // [2]
constexpr int N_MU = N_LS + ACD;         // [12] filter mean (0 for the bias input 11)
constexpr int N_RS = N_MU + 12;          // [12] 1/std     (1 for the bias input 11)
constexpr int NET = (N_RS + 12 + 3) & ~3;
constexpr int N_W2T = NET;               // student only: [j][i&15][i>>4] = W2[i][j]
constexpr int NET_S = NET + HID * HID;
static_assert(N_B2 % 4 == 0 && N_W3 % 4 == 0 && NET % 4 == 0, "16-B aligned LDS vectors");

// ---------------------------------------------------------------- per-pair scratch
// Waves w and w + 4 of a workgroup share a SIMD.  They form a PAIR with fixed roles:
// the producer (w < 4) computes observations, teacher and student forwards, the loss and
// dZ2; the consumer (w + 4) computes the weight gradients and dH1/dZ1 and steps the envs.
// They hand over one 16-env tile at a time through an LDS slot guarded by two counters.
constexpr int PAIRS = WAVES / 2;
constexpr int SOS = 12;                         // raw obs rows (11 + the bias input = 1)
constexpr int SAS = 68;                         // transposed activation rows [env][64 + pad]
constexpr int P_SO = 0;                         // [64][12] raw obs of the producer's group (its own)
constexpr int P_ACT = P_SO + GROUP * SOS;       // [64][2] actions (the producer's env step)
constexpr int P_H1T = P_ACT + GROUP * 2;        // slot: H1^T [16][SAS]
constexpr int P_DZT = P_H1T + TILE * SAS;       // slot: dZ2^T [16][SAS]
constexpr int P_SA = P_DZT + TILE * SAS;        // consumer-private: dZ1^T [16][SAS]
constexpr int P_SOB = P_SA + TILE * SAS;        // slot: the tile's raw obs rows [16][12] (the consumer's dW1 inputs)
constexpr int P_SACT = P_SOB + TILE * SOS;      // slot: the tile's actions [16][2] (CP: for the consumer's env step)
constexpr int P_FLAGS = P_SACT + TILE * 2;      // u32 [0] tiles published [1] tiles consumed
constexpr int PSCR = P_FLAGS + 4;
constexpr int LDS_FLOATS = NET + NET_S + PAIRS * PSCR;
static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
static_assert(PSCR % 4 == 0 && P_H1T % 4 == 0 && P_DZT % 4 == 0 && P_SA % 4 == 0 && P_SOB % 4 == 0,
              "16-B aligned scratch");
// Final per-workgroup reduction: pair p fills LDS region p.  The 76 rows of 64 that hold
// W1 (with b1 as row 11) and W2 are stored with a row stride of 68 floats, so that the
// consumer's register-layout writes (lane (g, j) -> row 4g + r, column j) hit 64 distinct
// banks; everything after W2 follows at +304 (region of RPAD floats).
constexpr int RROW = 68;
constexpr int RSHIFT = (P_B2 / HID) * (RROW - HID);   // 304
constexpr int RPAD = P_PAD + RSHIFT;
static_assert(P_B1 == P_W1 + OBD * HID && P_W2 == P_B1 + HID && P_B2 % HID == 0, "W1|b1|W2 rows");
static_assert(PAIRS * RPAD <= LDS_FLOATS && RPAD % 4 == 0 && P_PAD % 4 == 0, "final reduction must fit in the LDS");
__device__ __forceinline__ int ridx(int p) { return p < P_B2 ? (p >> 6) * RROW + (p & 63) : p + RSHIFT; }
[[maybe_unused]] constexpr int NSTAMP = 24;                      // RD_STAMPS debug slots per wave (scripts/stamps.py)
constexpr uint32_t SPIN_LIMIT = 1u << 22;       // ~0.1 s of s_sleep: a broken hand-off ends the launch

// Student image in the bf16 mode (offsets in floats; bf16 arrays hold 2 per float):
//   W1 A operands [g 4][fb 4][i 16][jj 8] = W1[8g+jj][16fb+i] (0 beyond input 10)
//   W2 forward    [s 2][g 4][fb 4][i 16][jj 8] = W2[kp(s,g,jj)][16fb+i]
//   W2 for dH1    [s 2][g 4][mb 4][i 16][jj 8] = W2[16mb+i][kp(s,g,jj)]
//   kp(s,g,jj) = 32s + 4g + (jj&3) + 16(jj>>2): the k order in which a layer's accumulator
//   (lane g holds features 16fb+4g+r) feeds the next 16x16x32 step with no lane movement.
//   f32: b1, b2, W3 (bf16-rounded values), b3, logstd, filter mean, 1/std.
constexpr int NB_W1 = 0;
constexpr int NB_W2F = NB_W1 + 4 * 4 * 16 * 8 / 2;
constexpr int NB_W2B = NB_W2F + 2 * 4 * 4 * 16 * 8 / 2;
constexpr int NB_B1 = NB_W2B + 2 * 4 * 4 * 16 * 8 / 2;
constexpr int NB_B2 = NB_B1 + HID;
constexpr int NB_W3 = NB_B2 + HID;
constexpr int NB_B3 = NB_W3 + HID * ACD;
constexpr int NB_LS = NB_B3 + ACD;
constexpr int NB_MU = NB_LS + ACD;
constexpr int NB_RS = NB_MU + 12;
constexpr int NETB_S = (NB_RS + 12 + 3) & ~3;   // bf16 student image (floats)
static_assert(NETB_S <= NET_S && NB_B1 % 4 == 0 && NB_W3 % 4 == 0, "bf16 student image");

// Split-mode image of a net (offsets in floats): the small vectors first, then the three
// pieces of the scaled W2 in the bf16 student's permuted forward order
// [q][s 2][g 4][fb 4][i 16][jj 8] = piece q of kTanhScale W2[kperm(s,g,jj)][16fb+i], then layer 1:
// the A operands of layer1_split's two piece pairings [v 2][g 4][fb 4][i 16][jj 8]: slot
// jj = 2s + c (s < 3) holds piece (v ? (0,1) : (0,2))[c] of kTanhScale W1[4s + g][16fb + i]
// (row 11 = b1), slots 6, 7 zero.  The student adds the pieces of the unscaled W2 for dH1 in
// the NB_W2B order.
constexpr int SP_PIECE = 2 * 4 * 4 * 16 * 8;      // bf16 elements per piece
constexpr int NX_B2 = 0;
constexpr int NX_W3 = NX_B2 + HID;                // 64
constexpr int NX_B3 = NX_W3 + HID * ACD;          // 192
constexpr int NX_LS = NX_B3 + ACD;
constexpr int NX_MU = NX_LS + ACD;
constexpr int NX_RS = NX_MU + 12;
constexpr int NX_W2F = NX_RS + 12;                // 220
constexpr int NX_W1S = NX_W2F + 3 * SP_PIECE / 2; // 6364
constexpr int NETX = NX_W1S + 2 * 4 * 4 * 16 * 8 / 2;   // 8412
constexpr int NX_W2B = NETX;                      // student only
constexpr int NETX_S = NX_W2B + 3 * SP_PIECE / 2; // 14556
static_assert(NX_W3 % 4 == 0 && NX_B2 % 4 == 0 && NX_W2F % 4 == 0 && NX_W1S % 4 == 0 && NETX % 4 == 0 &&
              NETX_S % 4 == 0, "16-B aligned split images");

// the student image's W3 / filter offsets by kind: exact f32 (N_*), split (NX_*), bf16 (NB_*)
template <int K> struct Off;
template <> struct Off<0> { static constexpr int W3 = N_W3, MU = N_MU, RS = N_RS; };
template <> struct Off<1> { static constexpr int W3 = NX_W3, MU = NX_MU, RS = NX_RS; };
template <> struct Off<2> { static constexpr int W3 = NB_W3, MU = NB_MU, RS = NB_RS; };

// LDS floats of the teacher / student images of a rollout instance
constexpr int img_t(bool SPL) { return SPL ? NETX : NET; }
constexpr int img_s(bool BS, bool SPL) { return BS ? NETB_S : (SPL ? NETX_S : NET_S); }
static_assert((NETX + NETX_S + PAIRS * PSCR) * 4 <= 160 * 1024 && (NETX + NETB_S + PAIRS * PSCR) * 4 <= 160 * 1024,
              "LDS budget (split images)");
