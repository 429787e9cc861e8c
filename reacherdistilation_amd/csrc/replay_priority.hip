// Prioritised draws from the replay ring (include/reacher_replay_priority.h): a uint32 priority per
// record beside the ring, filled by the pushes and refreshed from the student's outputs, and a draw
// in proportion to it.
//
// Everything is integer but the score, and the score is four float32 operations with no fused
// multiply-add, so tests/replay_prio_model.py reproduces every kernel bitwise.
//
// A sample is six launches on the handle's stream: episode weights + tile sums, the scan of the tile
// sums by ONE workgroup, the add (E -> X in place), the draw, then replay.hip's gather and bump.  The
// stream orders them: no workgroup waits on another, nothing spins, nothing is launched cooperatively.
// The counters are read from the device header by every kernel, as in replay.hip, so a captured call
// replays the next push or draw; a grid is sized by the host-known bound (capacity, `recent`) and the
// workgroups past the device's count return at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rd_common.h"
#include "rd_physics.h"
#include "replay_internal.h"

namespace {

using Header = rd::ReplayHeader;

constexpr int kSteps = RD_REPLAY_EPISODE_STEPS;
constexpr int kRec = RD_REPLAY_RECORD;
constexpr int F_T = 12, F_S = 16;
constexpr int kBlock = 256;
constexpr int kTile = RD_REPLAY_PRIO_SCAN_TILE;   // one episode per thread of a scan workgroup
constexpr int64_t kMaxGrid = 8192;
constexpr uint32_t kQMax = RD_REPLAY_PRIO_MAX;
static_assert(kTile == kBlock, "the scan kernels hold one episode per thread");

// how a score becomes an entry: the measure, 2^shift as a float, the floor
struct Quant {
    int32_t measure;
    float scale;
    uint32_t q_min;
};

__device__ __forceinline__ uint32_t clamp_q(uint32_t q) { return q < 1u ? 1u : (q > kQMax ? kQMax : q); }

// the quantised score of the output S (mean 0..1 read) against the teacher's t: one rounding per
// operation, written as separate statements under contract(off) so that none fuses (the header's
// __fsub_rn / __fmul_rn / __fadd_rn / __fsqrt_rn; sqrtf is the correctly rounded one of this build)
__device__ __forceinline__ uint32_t quantise(const float* __restrict__ S, const float* __restrict__ t, Quant z) {
#pragma clang fp contract(off)
    const float e0 = S[0] - t[0];
    const float e1 = S[1] - t[1];
    const float a = e0 * e0;
    const float b = e1 * e1;
    float score = a + b;
    if (z.measure == RD_PRIO_ERR) score = sqrtf(score);
    const float v = score * z.scale;
    uint32_t q = kQMax;
    if (v < 16777216.0f) q = (uint32_t)v;   // false for NaN and inf too
    return q < z.q_min ? z.q_min : q;
}

__device__ __forceinline__ int64_t eligible(const Header* hdr, int64_t capacity, int64_t recent, int64_t* pushed) {
    *pushed = hdr->pushed;
    int64_t count = *pushed < capacity ? *pushed : capacity;
    if (recent > 0 && recent < count) count = recent;
    return count;
}

// exclusive prefix of v over the workgroup's kBlock threads and their sum (Hillis-Steele in LDS)
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* lds, uint64_t* sum) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const uint64_t a = tid >= off ? lds[tid - off] : 0;
        __syncthreads();
        lds[tid] += a;
        __syncthreads();
    }
    const uint64_t incl = lds[tid];
    *sum = lds[kBlock - 1];
    __syncthreads();   // lds is reused by the caller's next pass
    return incl - v;
}

__global__ __launch_bounds__(kBlock) void prio_fill_kernel(uint32_t* __restrict__ table, int64_t entries, uint32_t q) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < entries; e += (int64_t)gridDim.x * kBlock)
        table[e] = q;
}

// the entries of the slots a push has just written (it runs before the push's bump)
__global__ __launch_bounds__(kBlock) void prio_push_kernel(uint32_t* __restrict__ table, const float* __restrict__ ring,
                                                          const Header* hdr, int64_t episodes, int64_t capacity,
                                                          int record, uint32_t q_init, Quant z) {
    const int64_t pushed = hdr->pushed;
    const int64_t total = episodes * kSteps;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t q = e / kSteps;
        const int s = (int)(e - q * kSteps);
        const int64_t at = ((pushed + q) % capacity) * kSteps + s;
        uint32_t v = q_init;
        if (record) {
            const float* rec = ring + at * kRec;
            v = quantise(rec + F_S, rec + F_T, z);
        }
        table[at] = v;
    }
}

// writer e = (p, b) of [T][B]: record start_b + p of slot_b.  phase 0 stores 0, phase 1 takes the
// maximum, so a record named more than once ends with the maximum over its writers in any order.
__global__ __launch_bounds__(kBlock) void prio_update_kernel(uint32_t* __restrict__ table, const float* __restrict__ ring,
                                                            const int32_t* __restrict__ idx,
                                                            const float* __restrict__ s_pdflat, int64_t B, int T,
                                                            int64_t capacity, int phase, Quant z) {
    const int64_t total = B * T;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t p = e / B, b = e - p * B;
        const int64_t slot = idx[2 * b], start = idx[2 * b + 1];
        if (slot < 0 || slot >= capacity || start < 0 || start + T > kSteps) continue;
        const int64_t at = slot * kSteps + start + p;
        if (phase == 0) table[at] = 0u;
        else atomicMax(table + at, quantise(s_pdflat + e * 4, ring + at * kRec + F_T, z));
    }
}

// E_j of rank j = the sum over the episode's 51 - T windows of their T clamped entries: entry i lies
// in min(i, 50 - T) - max(0, i - T + 1) + 1 of them.  Also the tile's sum into partials[tile].
__global__ __launch_bounds__(kBlock) void prio_weights_kernel(const Header* hdr, const uint32_t* __restrict__ table,
                                                             uint64_t* __restrict__ weights,
                                                             uint64_t* __restrict__ partials, int64_t recent,
                                                             int64_t capacity, int T) {
    __shared__ uint64_t lds[kBlock];
    int64_t pushed;
    const int64_t count = eligible(hdr, capacity, recent, &pushed);
    if ((int64_t)blockIdx.x * kTile >= count) return;   // the whole workgroup
    const int64_t j = (int64_t)blockIdx.x * kTile + threadIdx.x;
    uint64_t E = 0;
    if (j < count) {
        const uint32_t* row = table + ((pushed - count + j) % capacity) * kSteps;
        for (int i = 0; i < kSteps; ++i) {
            const int lo = i - T + 1 > 0 ? i - T + 1 : 0, hi = i < kSteps - T ? i : kSteps - T;
            E += (uint64_t)clamp_q(row[i]) * (uint32_t)(hi - lo + 1);
        }
        weights[j] = E;
    }
    uint64_t sum;
    (void)block_scan(E, lds, &sum);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// ONE workgroup: partials[0 .. tiles) -> their exclusive prefix, in passes of kBlock with a carry;
// the total into *total
__global__ __launch_bounds__(kBlock) void prio_scan_partials_kernel(const Header* hdr, uint64_t* __restrict__ partials,
                                                                   uint64_t* __restrict__ total, int64_t recent,
                                                                   int64_t capacity) {
    __shared__ uint64_t lds[kBlock];
    int64_t pushed;
    const int64_t count = eligible(hdr, capacity, recent, &pushed);
    const int64_t tiles = (count + kTile - 1) / kTile;
    uint64_t carry = 0;
    for (int64_t base = 0; base < tiles; base += kBlock) {
        const int64_t g = base + threadIdx.x;
        const uint64_t v = g < tiles ? partials[g] : 0;
        uint64_t sum;
        const uint64_t ex = block_scan(v, lds, &sum);
        if (g < tiles) partials[g] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

// E_j -> X_j in place: the tile's own exclusive scan plus the prefix of the tiles before it
__global__ __launch_bounds__(kBlock) void prio_scan_add_kernel(const Header* hdr, uint64_t* __restrict__ weights,
                                                              const uint64_t* __restrict__ partials, int64_t recent,
                                                              int64_t capacity) {
    __shared__ uint64_t lds[kBlock];
    int64_t pushed;
    const int64_t count = eligible(hdr, capacity, recent, &pushed);
    if ((int64_t)blockIdx.x * kTile >= count) return;
    const int64_t j = (int64_t)blockIdx.x * kTile + threadIdx.x;
    const uint64_t v = j < count ? weights[j] : 0;
    uint64_t sum;
    const uint64_t ex = block_scan(v, lds, &sum);
    if (j < count) weights[j] = partials[blockIdx.x] + ex;
}

// idx[b] = (slot, start) of window b, drawn with probability W / total
__global__ __launch_bounds__(kBlock) void prio_draw_kernel(const Header* hdr, const uint32_t* __restrict__ table,
                                                          const uint64_t* __restrict__ X,
                                                          const uint64_t* __restrict__ total_p, int2* __restrict__ scratch,
                                                          int32_t* __restrict__ idx_out, float* __restrict__ prob,
                                                          int64_t windows, int64_t window_base, int64_t recent,
                                                          uint64_t seed, int64_t capacity, int T) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= windows) return;
    int64_t pushed;
    const int64_t count = eligible(hdr, capacity, recent, &pushed);
    int2 v = make_int2(0, 0);
    float pr = 0.0f;
    if (count > 0) {   // (0 only for a captured sample replayed after a reset: slot 0, as the uniform draw)
        const uint32_t d = (uint32_t)hdr->draws;
        const uint64_t total = *total_p;
        const uint64_t w = (uint64_t)(window_base + b);
        uint32_t o[4];
        rd::philox((uint32_t)w, (uint32_t)(w >> 32), d, 2u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        const uint64_t target = __umul64hi(((uint64_t)o[0] << 32) | o[1], total);   // < total
        int64_t lo = 0, hi = count;   // X[lo] <= target < X[hi] (X[count] = total)
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (X[mid] <= target) lo = mid;
            else hi = mid;
        }
        const uint64_t rem = target - X[lo];
        const int64_t slot = (pushed - count + lo) % capacity;
        const uint32_t* row = table + slot * kSteps;
        uint64_t W = 0;
        for (int p = 0; p < T; ++p) W += clamp_q(row[p]);
        uint64_t run = 0;
        int start = 0;
        for (;;) {
            run += W;
            if (run > rem || start == kSteps - T) break;   // rem < E_rank: the sum reaches it by the last start
            W += clamp_q(row[start + T]);
            W -= clamp_q(row[start]);
            ++start;
        }
        v = make_int2((int)slot, start);
        pr = (float)((double)W / (double)total);
    }
    scratch[b] = v;
    if (idx_out) {
        idx_out[2 * b] = v.x;
        idx_out[2 * b + 1] = v.y;
    }
    if (prob) prob[b] = pr;
}

int grid_for(int64_t elements) {
    const int64_t g = (elements + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

int64_t tiles_of(int64_t episodes) { return (episodes + kTile - 1) / kTile; }

Quant quant_of(const rd_replay_prio_config& c) { return Quant{c.measure, (float)(1u << c.shift), c.q_min}; }

int check_q(const char* fn, const char* field, uint32_t q) {
    if (q < 1u || q > kQMax) return rd::set_error(RD_EINVAL, "%s: %s %u outside 1 .. 2^24", fn, field, q);
    return RD_OK;
}

int check_config(const char* fn, const rd_replay_prio_config* c) {
    if (c->measure != RD_PRIO_SQERR && c->measure != RD_PRIO_ERR)
        return rd::set_error(RD_EINVAL, "%s: unknown measure %d", fn, c->measure);
    if (c->shift < 0 || c->shift > 24) return rd::set_error(RD_EINVAL, "%s: shift %d outside 0 .. 24", fn, c->shift);
    if (int rc = check_q(fn, "q_min", c->q_min)) return rc;
    if (int rc = check_q(fn, "q_init", c->q_init)) return rc;
    if (c->init_mode != RD_PRIO_INIT_CONST && c->init_mode != RD_PRIO_INIT_RECORD)
        return rd::set_error(RD_EINVAL, "%s: unknown init_mode %d", fn, c->init_mode);
    if (c->reserved != 0) return rd::set_error(RD_EINVAL, "%s: reserved %d != 0", fn, c->reserved);
    return RD_OK;
}

int check_enabled(const char* fn, const rd_replay* h) {
    if (!h->prio.enabled) return rd::set_error(RD_EINVAL, "%s: priorities are not enabled", fn);
    return RD_OK;
}

// the checks both samples share: first those that need no handle, then those that read it
int check_sample(const char* fn, const rd_replay* h, const rd_replay_sample* s) {
    if (s->windows < 1) return rd::set_error(RD_EINVAL, "%s: windows %lld < 1", fn, (long long)s->windows);
    if (s->window_base < 0) return rd::set_error(RD_EINVAL, "%s: negative window_base", fn);
    if (s->recent < 0) return rd::set_error(RD_EINVAL, "%s: negative recent", fn);
    if (int rc = check_enabled(fn, h)) return rc;
    if (s->windows > h->max_batch)
        return rd::set_error(RD_EINVAL, "%s: windows %lld exceed max_batch %lld", fn, (long long)s->windows,
                             (long long)h->max_batch);
    if (h->host_pushed < 1) return rd::set_error(RD_EINVAL, "%s: the ring has never been pushed to", fn);
    return RD_OK;
}

// launches 1 to 4 of a sample: weights, the two-level scan, the draw into h->scratch (and idx, prob)
int draw(const char* fn, rd_replay* h, const rd_replay_sample* s, int T, int32_t* idx, float* prob) {
    rd::ReplayPrio& pr = h->prio;
    const int64_t bound = s->recent > 0 && s->recent < h->capacity ? s->recent : h->capacity;
    const unsigned tiles = (unsigned)tiles_of(bound);
    uint64_t* total = pr.partials + tiles_of(h->capacity);
    hipLaunchKernelGGL(prio_weights_kernel, dim3(tiles), dim3(kBlock), 0, h->stream, h->hdr, pr.table, pr.weights,
                       pr.partials, s->recent, h->capacity, T);
    RD_HIP(hipGetLastError(), fn);
    hipLaunchKernelGGL(prio_scan_partials_kernel, dim3(1), dim3(kBlock), 0, h->stream, h->hdr, pr.partials, total,
                       s->recent, h->capacity);
    RD_HIP(hipGetLastError(), fn);
    hipLaunchKernelGGL(prio_scan_add_kernel, dim3(tiles), dim3(kBlock), 0, h->stream, h->hdr, pr.weights, pr.partials,
                       s->recent, h->capacity);
    RD_HIP(hipGetLastError(), fn);
    hipLaunchKernelGGL(prio_draw_kernel, dim3((unsigned)((s->windows + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream,
                       h->hdr, pr.table, pr.weights, total, h->scratch, idx, prob, s->windows, s->window_base, s->recent,
                       s->seed, h->capacity, T);
    RD_HIP(hipGetLastError(), fn);
    return RD_OK;
}

int update(const char* fn, rd_replay* h, const int32_t* idx, const float* s_pdflat, int T, int64_t B) {
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, fn);
    for (int phase = 0; phase < 2; ++phase) {
        hipLaunchKernelGGL(prio_update_kernel, dim3(grid_for(B * T)), dim3(kBlock), 0, h->stream, h->prio.table, h->ring,
                           idx, s_pdflat, B, T, h->capacity, phase, quant_of(h->prio.cfg));
        RD_HIP(hipGetLastError(), fn);
    }
    return RD_OK;
}

}  // namespace

namespace rd {

int replay_prio_push_init(const char* what, rd_replay* h, int64_t episodes) {
    const rd_replay_prio_config& c = h->prio.cfg;
    hipLaunchKernelGGL(prio_push_kernel, dim3(grid_for(episodes * kSteps)), dim3(kBlock), 0, h->stream, h->prio.table,
                       h->ring, h->hdr, episodes, h->capacity, c.init_mode == RD_PRIO_INIT_RECORD ? 1 : 0, c.q_init,
                       quant_of(c));
    RD_HIP(hipGetLastError(), what);
    return RD_OK;
}

void replay_prio_destroy(rd_replay* h) {
    if (h->prio.weights) (void)hipFree(h->prio.weights);
    if (h->prio.partials) (void)hipFree(h->prio.partials);
    if (h->prio.owns_table && h->prio.table) (void)hipFree(h->prio.table);
    h->prio = ReplayPrio();
}

}  // namespace rd

extern "C" {

int rd_replay_prio_enable(rd_replay* h, const rd_replay_prio_config* cfg, uint32_t* table) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_prio_enable: null handle");
    if (!cfg) return rd::set_error(RD_EINVAL, "rd_replay_prio_enable: null config");
    if (int rc = check_config("rd_replay_prio_enable", cfg)) return rc;
    if (h->capacity > RD_REPLAY_PRIO_MAX_CAPACITY)
        return rd::set_error(RD_EINVAL, "rd_replay_prio_enable: capacity %lld above %d", (long long)h->capacity,
                             RD_REPLAY_PRIO_MAX_CAPACITY);
    if (h->prio.enabled) return rd::set_error(RD_EINVAL, "rd_replay_prio_enable: priorities are already enabled");
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_prio_enable: hipSetDevice");
    rd::ReplayPrio& pr = h->prio;
    const int64_t entries = h->capacity * kSteps;
    hipError_t err = hipMalloc(&pr.weights, sizeof(uint64_t) * (size_t)h->capacity);
    if (err == hipSuccess) err = hipMalloc(&pr.partials, sizeof(uint64_t) * (size_t)(tiles_of(h->capacity) + 1));
    pr.table = table;
    if (err == hipSuccess && !table) {
        err = hipMalloc(&pr.table, sizeof(uint32_t) * (size_t)entries);
        pr.owns_table = err == hipSuccess;
    }
    if (err == hipSuccess) {
        hipLaunchKernelGGL(prio_fill_kernel, dim3(grid_for(entries)), dim3(kBlock), 0, h->stream, pr.table, entries,
                           cfg->q_init);
        err = hipGetLastError();
    }
    if (err != hipSuccess) {
        rd::replay_prio_destroy(h);
        return rd::hip_fail(err, "rd_replay_prio_enable: allocation");
    }
    pr.cfg = *cfg;
    pr.enabled = true;
    return RD_OK;
}

int rd_replay_prio_configure(rd_replay* h, const rd_replay_prio_config* cfg) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_prio_configure: null handle");
    if (!cfg) return rd::set_error(RD_EINVAL, "rd_replay_prio_configure: null config");
    if (int rc = check_config("rd_replay_prio_configure", cfg)) return rc;
    if (int rc = check_enabled("rd_replay_prio_configure", h)) return rc;
    h->prio.cfg = *cfg;
    return RD_OK;
}

int rd_replay_prio_enabled(const rd_replay* h) { return h ? (h->prio.enabled ? 1 : 0) : -1; }

uint32_t* rd_replay_prio_table(rd_replay* h) { return h && h->prio.enabled ? h->prio.table : nullptr; }

int rd_replay_prio_fill(rd_replay* h, uint32_t q) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_prio_fill: null handle");
    if (int rc = check_q("rd_replay_prio_fill", "q", q)) return rc;
    if (int rc = check_enabled("rd_replay_prio_fill", h)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_prio_fill: hipSetDevice");
    const int64_t entries = h->capacity * kSteps;
    hipLaunchKernelGGL(prio_fill_kernel, dim3(grid_for(entries)), dim3(kBlock), 0, h->stream, h->prio.table, entries, q);
    RD_HIP(hipGetLastError(), "rd_replay_prio_fill: launch");
    return RD_OK;
}

int rd_replay_prio_update_rows(rd_replay* h, const int32_t* idx, const float* s_pdflat, int64_t rows) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_rows: null handle");
    if (!idx) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_rows: null idx");
    if (!s_pdflat) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_rows: null s_pdflat");
    if (rows < 1) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_rows: rows %lld < 1", (long long)rows);
    if (int rc = check_enabled("rd_replay_prio_update_rows", h)) return rc;
    if (rows > h->max_batch)
        return rd::set_error(RD_EINVAL, "rd_replay_prio_update_rows: rows %lld exceed max_batch %lld", (long long)rows,
                             (long long)h->max_batch);
    return update("rd_replay_prio_update_rows: launch", h, idx, s_pdflat, 1, rows);
}

int rd_replay_prio_update_windows(rd_replay* h, const int32_t* idx, const float* s_pdflat, int32_t steps,
                                  int64_t windows) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_windows: null handle");
    if (!idx) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_windows: null idx");
    if (!s_pdflat) return rd::set_error(RD_EINVAL, "rd_replay_prio_update_windows: null s_pdflat");
    if (steps < 1 || steps > kSteps)
        return rd::set_error(RD_EINVAL, "rd_replay_prio_update_windows: steps %d outside 1 .. 50", steps);
    if (windows < 1)
        return rd::set_error(RD_EINVAL, "rd_replay_prio_update_windows: windows %lld < 1", (long long)windows);
    if (int rc = check_enabled("rd_replay_prio_update_windows", h)) return rc;
    if (windows > h->max_batch)
        return rd::set_error(RD_EINVAL, "rd_replay_prio_update_windows: windows %lld exceed max_batch %lld",
                             (long long)windows, (long long)h->max_batch);
    return update("rd_replay_prio_update_windows: launch", h, idx, s_pdflat, steps, windows);
}

int rd_replay_prio_sample_rows(rd_replay* h, const rd_replay_sample* s, float* x, float* t_pdflat, int32_t* idx,
                               float* prob) {
    const char* fn = "rd_replay_prio_sample_rows";
    if (!h) return rd::set_error(RD_EINVAL, "%s: null handle", fn);
    if (!s) return rd::set_error(RD_EINVAL, "%s: null sample", fn);
    if (!x) return rd::set_error(RD_EINVAL, "%s: null x", fn);
    if (!t_pdflat) return rd::set_error(RD_EINVAL, "%s: null t_pdflat", fn);
    if ((uintptr_t)x & 15) return rd::set_error(RD_EINVAL, "%s: x is not 16-byte aligned", fn);
    if (int rc = check_sample(fn, h, s)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_prio_sample_rows: hipSetDevice");
    if (int rc = draw("rd_replay_prio_sample_rows: draw launches", h, s, 1, idx, prob)) return rc;
    if (int rc = rd::replay_gather_rows("rd_replay_prio_sample_rows: gather launch", h, x, t_pdflat, s->windows)) return rc;
    return rd::replay_bump("rd_replay_prio_sample_rows: bump launch", h, 0, 1);
}

int rd_replay_prio_sample_windows(rd_replay* h, const rd_replay_sample* s, float* ob_w, float* prev_w, float* t_w,
                                  float* prew_w, int32_t* idx, float* prob) {
    const char* fn = "rd_replay_prio_sample_windows";
    if (!h) return rd::set_error(RD_EINVAL, "%s: null handle", fn);
    if (!s) return rd::set_error(RD_EINVAL, "%s: null sample", fn);
    if (!ob_w) return rd::set_error(RD_EINVAL, "%s: null ob_w", fn);
    if (!prev_w) return rd::set_error(RD_EINVAL, "%s: null prev_w", fn);
    if (!t_w) return rd::set_error(RD_EINVAL, "%s: null t_w", fn);
    if (s->steps < 1 || s->steps > kSteps) return rd::set_error(RD_EINVAL, "%s: steps %d outside 1 .. 50", fn, s->steps);
    if (s->start_mode != RD_REPLAY_START_PER_WINDOW)
        return rd::set_error(RD_EINVAL, "%s: start_mode %d: a prioritised draw has a start per window only", fn,
                             s->start_mode);
    if (int rc = check_sample(fn, h, s)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_prio_sample_windows: hipSetDevice");
    if (int rc = draw("rd_replay_prio_sample_windows: draw launches", h, s, s->steps, idx, prob)) return rc;
    if (int rc = rd::replay_gather_windows("rd_replay_prio_sample_windows: gather launch", h, ob_w, prev_w, t_w, prew_w,
                                           s->steps, s->windows))
        return rc;
    return rd::replay_bump("rd_replay_prio_sample_windows: bump launch", h, 0, 1);
}

}  // extern "C"
