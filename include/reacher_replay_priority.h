/* reacher_replay_priority.h -- C ABI of prioritised draws from the device-resident episode replay ring
 * (reacher_replay.h; libreacher.so): a priority table beside the ring, a weighted draw in place of the
 * uniform one, and the calls that fill and refresh the table.
 *
 * Once the student tracks the teacher on most states, almost every uniformly drawn record carries a
 * near-zero gradient.  Here a record is drawn in proportion to a priority, by default the student's
 * disagreement with the teacher on it (loss-proportional, or prioritised, replay).  The contract is
 * the ring's: no host RNG, no index upload, no sync, capturable.  A ring that never enables priorities
 * launches exactly what it launched before.
 *
 * Table
 *   q[capacity][50] uint32, one entry per record, slot-major like the ring.
 *   table NULL: the library allocates (and frees) it; else a caller-owned device buffer that outlives
 *   the handle, as rd_replay_create's `ring` is.
 *   rd_replay_prio_enable allocates the scratch of the draw (below), sets every entry to q_init, and
 *   may be called once per handle.  RD_EINVAL, naming the field: a capacity above
 *   RD_REPLAY_PRIO_MAX_CAPACITY, a second call, a bad config field.  It is the only call here that
 *   allocates; every other one is asynchronous on the handle's stream, does not sync, and is capturable.
 *   The table belongs to the caller: any stream-ordered kernel or torch op may write it, so an
 *   exponent alpha other than 1 (RD_PRIO_SQERR read as a squared error) or 1/2 (RD_PRIO_ERR) is a
 *   one-line torch op and needs no further API.  Every READ of an entry clamps it to
 *   1 .. RD_REPLAY_PRIO_MAX: whatever the caller writes, a total is never zero and never overflows.
 *   rd_replay_reset leaves the table alone, as it leaves the floats.
 *
 * Score of a record.  The student's output is S = mean[2] | logstd[2]; the record's own teacher output
 * is t = t_pdflat in the ring.
 *   e_i = __fsub_rn(S[i], t[i]), i = 0, 1
 *   d   = __fadd_rn(__fmul_rn(e0, e0), __fmul_rn(e1, e1))            RD_PRIO_SQERR: score = d
 *   RD_PRIO_ERR: score = __fsqrt_rn(d)
 * Every operation is a single IEEE round-to-nearest one and nothing is fused into a multiply-add, so a
 * NumPy float32 model is bitwise.  (A KL-based measure is out of scope: expf has no bitwise model.)
 *
 * Quantisation
 *   v = __fmul_rn(score, 2^shift)
 *   q = RD_REPLAY_PRIO_MAX if !(v < 16777216.0f) (which covers NaN and inf), else (uint32_t)v, truncated
 *   q = max(q, q_min)
 *
 * Pushes.  While priorities are enabled, each of the four pushes (rd_replay_push_steps, _episodes,
 * _rows, _rows_flags) adds ONE launch between its copy and the counter bump, which writes the 50
 * entries of each pushed episode's slot: q_init under RD_PRIO_INIT_CONST; under RD_PRIO_INIT_RECORD the
 * quantised score of the record's own s_pdflat against its t_pdflat -- the student as it was when it
 * acted, with no extra forward.  The launch reads `pushed` from the device header, so a captured push
 * replays the NEXT slots.  While priorities are not enabled, every call of reacher_replay.h issues
 * exactly the launches it issued before.  rd_replay_prio_configure is host-only: the new config
 * enters the launches issued after it (a captured launch keeps the config it was captured with).
 *
 * Updates.  idx [B][2] is what a sample wrote, (slot, step) or (slot, start); s_pdflat is [B][4] for
 * rows (rdm_forward on the sampled x) and [T][B][4] position-major for windows (rdl_forward on the
 * sampled windows).  Each named record gets the quantised score of the given output against the
 * ring's t_pdflat of that record.  A record named more than once ends with the MAXIMUM over its
 * writers: two launches, in the first every writer stores 0, in the second every writer does an
 * atomicMax on the uint32 entry (a vector atomic, order-independent), so the table is a bitwise
 * function of the inputs.  An entry with slot outside 0 .. capacity - 1, a negative step / start, or
 * step + T > 50 is skipped on the device: nothing is ever written outside the table.  If a push has
 * overwritten the slot since the sample, the score is taken against the NEW record's t_pdflat and lands
 * on the new record: harmless (it is a valid disagreement of some student output with some teacher
 * output, and the next update of that record replaces it), and cheaper than a generation check.
 *
 * Draw.  With d = the low 32 bits of `draws` and w = window_base + b; count and the eligible episodes
 * exactly as in the uniform draw (`recent` included); ranks j = 0 .. count - 1 from the oldest
 * eligible episode, slot_j = (pushed - count + j) % capacity:
 *   W(slot, s) = sum over p < T of clamp(q[slot][s + p]),  s = 0 .. 50 - T
 *   E_j        = sum over s of W(slot_j, s);  X_j = the exclusive prefix of E;  total = X_count
 *   (r0, r1, ., .) = Philox4x32-10(ctr = {w lo, w hi, d, 2}, key = {seed lo, seed hi})
 *   (counter word 3 = 2 keeps the stream disjoint from the uniform draw, word 3 = 0, and from the
 *   common start, word 3 = 1)
 *   target = ((r0 2^32 + r1) total) >> 64                                  (__umul64hi)
 *   rank   = the j with X_j <= target < X_{j+1}
 *   start  = the s at which the running sum of W(slot_rank, .) first exceeds target - X_rank
 * One 64-bit word therefore draws a window with probability W / total, to within total / 2^64.  All
 * sums are uint64 (E <= 650 x 2^24, total < 2^56): exact and order-independent, so the draw is a
 * bitwise function of the table, the counters and the sample struct.
 *   prob[b] = (float)((double)W / (double)total); prob may be NULL.
 * Rows are the case T = 1 (start = step).  RD_REPLAY_START_COMMON returns RD_EINVAL here.  draws += 1,
 * the same counter as the uniform samples.
 *
 * Launches of a sample, ordered by the stream alone:
 *   1. episode weights: E_j into scratch, one thread per episode, and each workgroup's sum of its
 *      RD_REPLAY_PRIO_SCAN_TILE episodes into the partials;
 *   2. ONE workgroup scans the partials (exclusive) and leaves the total;
 *   3. the add: each workgroup scans its tile and adds its partial's prefix, E -> X in place
 *      (two levels at any capacity this header admits);
 *   4. the draw: a binary search over X, then at most 50 steps inside the episode;
 *   5. the EXISTING gather kernels of reacher_replay.h, launched on the same scratch idx;
 *   6. the bump.
 * There is no wait of one workgroup on another, no cooperative launch, no grid barrier and no spin of
 * any kind (the ring's convention: "no atomics, no grid-wide sync"; the only atomic is the update's
 * atomicMax).
 *
 * Conventions as in reacher_replay.h.  All checks that need no handle come before the handle is
 * read, and all checks come before any device call; rd_last_error() names the function and the field.
 * RD_EINVAL: priorities not enabled; a NULL required pointer; a misaligned x; steps outside 1 .. 50;
 * windows / rows < 1 or > max_batch; a negative window_base or recent; RD_REPLAY_START_COMMON; a ring
 * never pushed to; shift outside 0 .. 24; q_min or q_init (or rd_replay_prio_fill's q) outside
 * 1 .. 2^24; an unknown measure or init_mode; reserved != 0.
 */
#ifndef REACHER_REPLAY_PRIORITY_H
#define REACHER_REPLAY_PRIORITY_H
#include <stdint.h>

#include "reacher_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RD_REPLAY_PRIO_MAX 16777216            /* 2^24: the largest priority a read returns         */
#define RD_REPLAY_PRIO_MAX_CAPACITY 4194304    /* 2^22: the largest ring that can enable priorities */
#define RD_REPLAY_PRIO_SCAN_TILE 256           /* episodes one workgroup of the scan covers per pass */
#define RD_PRIO_SQERR 0
#define RD_PRIO_ERR 1
#define RD_PRIO_INIT_CONST 0
#define RD_PRIO_INIT_RECORD 1

typedef struct {
    int32_t  measure;    /* RD_PRIO_SQERR | RD_PRIO_ERR                              */
    int32_t  shift;      /* 0..24: fixed-point scale 2^shift of the score            */
    uint32_t q_min;      /* 1..RD_REPLAY_PRIO_MAX: floor of every quantised priority */
    uint32_t q_init;     /* 1..RD_REPLAY_PRIO_MAX: the INIT_CONST value              */
    int32_t  init_mode;  /* RD_PRIO_INIT_*: what a push writes for its episodes      */
    int32_t  reserved;   /* 0                                                        */
} rd_replay_prio_config;   /* 24 bytes */

/* table NULL: library-owned; else a device buffer [capacity][50] uint32.  Once per handle. */
int rd_replay_prio_enable(rd_replay* h, const rd_replay_prio_config* cfg, uint32_t* table);
/* host-only: replaces the config for the launches issued from now on */
int rd_replay_prio_configure(rd_replay* h, const rd_replay_prio_config* cfg);
/* 1 / 0; -1 for a NULL handle */
int rd_replay_prio_enabled(const rd_replay* h);
/* the table's device pointer; NULL while priorities are off (and for a NULL handle) */
uint32_t* rd_replay_prio_table(rd_replay* h);
/* every entry of the table = q (1 .. RD_REPLAY_PRIO_MAX) */
int rd_replay_prio_fill(rd_replay* h, uint32_t q);
/* idx [rows][2] int32 (slot, step), s_pdflat [rows][4]; rows 1 .. max_batch */
int rd_replay_prio_update_rows(rd_replay* h, const int32_t* idx, const float* s_pdflat, int64_t rows);
/* idx [windows][2] int32 (slot, start), s_pdflat [steps][windows][4]; steps 1 .. 50, windows 1 .. max_batch */
int rd_replay_prio_update_windows(rd_replay* h, const int32_t* idx, const float* s_pdflat, int32_t steps,
                                  int64_t windows);
/* rd_replay_sample_rows / rd_replay_sample_windows with the weighted draw; the outputs as there, and
 * prob [B] f32 (may be NULL, as idx may) */
int rd_replay_prio_sample_rows(rd_replay* h, const rd_replay_sample* s, float* x, float* t_pdflat, int32_t* idx,
                               float* prob);
int rd_replay_prio_sample_windows(rd_replay* h, const rd_replay_sample* s, float* ob_w, float* prev_w, float* t_w,
                                  float* prew_w, int32_t* idx, float* prob);

#ifdef __cplusplus
}
#endif
#endif
