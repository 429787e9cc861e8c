// Device-resident episode replay ring (include/reacher_replay.h): pushes are pure copies into
// rec[capacity][50][21], draws are Philox4x32-10 words mapped by multiply-high, gathers copy floats.
//
// Counters: a two-word header on the device (pushed, draws).  Every kernel reads it when it RUNS and
// a 1-thread launch behind each push / sample adds to it, so the stream orders everything and a
// captured call replays the next push or draw.  No atomics, no grid-wide sync.
//
// Kernel shape.  All launches are grid-stride loops over flat OUTPUT elements, so a wave's 64 lanes
// store 64 consecutive floats (256 B): the ring side of a push, and per output tensor of a sample the
// position-major stream [p][b][f], in which the rows of consecutive windows b of one position are
// contiguous.  The scattered side is the read of the 84-byte records (and the step-major source rows
// of a push), which runs of 4 to 21 lanes share.  A sample is three launches on the handle's stream:
// draw (idx[B] into the handle's scratch, and the caller's idx), gather (blockIdx.y picks the output
// tensor, so each has its own compile-time row width), bump.  The priority table and the weighted draw
// are replay_priority.hip's; it launches this file's gathers and bump through replay_internal.h, and a
// push ends with its launch only while priorities are enabled (push_done).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "rd_common.h"
#include "rd_physics.h"
#include "replay_internal.h"

namespace {

constexpr int kSteps = RD_REPLAY_EPISODE_STEPS;   // 50 records per episode
constexpr int kRec = RD_REPLAY_RECORD;            // 21 floats per record
constexpr int kOb = 11, kPd = 4;
constexpr int F_REW = 11, F_T = 12, F_S = 16, F_WITH = 20;
constexpr int kBlock = 256;
constexpr int64_t kMaxGrid = 8192;

using Header = rd::ReplayHeader;

__global__ void replay_bump_kernel(Header* hdr, int64_t pushed, int64_t draws) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr->pushed += pushed;
        hdr->draws += draws;
    }
}

// element e of the E pushed episodes [E][50][21] -> (episode q, step s, field f) and its ring address
__device__ __forceinline__ int64_t ring_index(int64_t pushed, int64_t capacity, int64_t q, int rem) {
    return ((pushed + q) % capacity) * (kSteps * kRec) + rem;
}

// records [K][n][21] step-major; episode q = (k / 50) n + i
__global__ __launch_bounds__(kBlock) void replay_push_steps_kernel(float* __restrict__ ring, const Header* hdr,
                                                                  const float* __restrict__ records, int64_t episodes,
                                                                  int64_t n, int64_t capacity) {
    const int64_t pushed = hdr->pushed;
    const int64_t total = episodes * (kSteps * kRec);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t q = e / (kSteps * kRec);
        const int rem = (int)(e - q * (kSteps * kRec));
        const int s = rem / kRec, f = rem - s * kRec;
        const int64_t blk = q / n, i = q - blk * n;
        ring[ring_index(pushed, capacity, q, rem)] = records[((blk * kSteps + s) * n + i) * kRec + f];
    }
}

// records [E][50][21] episode-major
__global__ __launch_bounds__(kBlock) void replay_push_episodes_kernel(float* __restrict__ ring, const Header* hdr,
                                                                     const float* __restrict__ records,
                                                                     int64_t episodes, int64_t capacity) {
    const int64_t pushed = hdr->pushed;
    const int64_t total = episodes * (kSteps * kRec);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t q = e / (kSteps * kRec);
        const int rem = (int)(e - q * (kSteps * kRec));
        ring[ring_index(pushed, capacity, q, rem)] = records[e];
    }
}

// rdm_envs_act's outputs, step-major; the record's fields are assembled per element
// (with_rows: the per-row stepped_with [K][n] of rd_replay_push_rows_flags, else the scalar)
__global__ __launch_bounds__(kBlock) void replay_push_rows_kernel(float* __restrict__ ring, const Header* hdr,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ t_pdflat,
                                                                 const float* __restrict__ s_pdflat,
                                                                 const float* __restrict__ reward,
                                                                 const float* __restrict__ carry, int64_t episodes,
                                                                 int64_t n, int64_t capacity, float stepped_with,
                                                                 const float* __restrict__ with_rows) {
    const int64_t pushed = hdr->pushed;
    const int64_t total = episodes * (kSteps * kRec);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t q = e / (kSteps * kRec);
        const int rem = (int)(e - q * (kSteps * kRec));
        const int s = rem / kRec, f = rem - s * kRec;
        const int64_t blk = q / n, i = q - blk * n;
        const int64_t k = blk * kSteps + s, row = k * n + i;
        float v;
        if (f < kOb) v = x[row * 16 + f];
        else if (f == F_REW) v = k > 0 ? reward[row - n] : (carry ? carry[i] : 0.0f);
        else if (f < F_S) v = t_pdflat[row * kPd + (f - F_T)];
        else if (f < F_WITH) v = s_pdflat ? s_pdflat[row * kPd + (f - F_S)] : 0.0f;
        else v = with_rows ? with_rows[row] : stepped_with;
        ring[ring_index(pushed, capacity, q, rem)] = v;
    }
}

__device__ __forceinline__ uint32_t mulhi_map(uint32_t word, uint32_t m) { return __umulhi(word, m); }

// idx[b] = (slot, start) of window b.  span = 51 - T (windows) or 50 (rows); common: one start per batch
__global__ __launch_bounds__(kBlock) void replay_draw_kernel(const Header* hdr, int2* __restrict__ scratch,
                                                            int32_t* __restrict__ idx_out, int64_t windows,
                                                            int64_t window_base, int64_t recent, uint64_t seed,
                                                            int64_t capacity, uint32_t span, int common) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= windows) return;
    const int64_t pushed = hdr->pushed;
    const uint32_t d = (uint32_t)hdr->draws;
    int64_t count = pushed < capacity ? pushed : capacity;
    if (recent > 0 && recent < count) count = recent;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint64_t w = (uint64_t)(window_base + b);
    uint32_t o[4];
    rd::philox((uint32_t)w, (uint32_t)(w >> 32), d, 0u, k0, k1, o);
    const int64_t rank = (int64_t)mulhi_map(o[0], (uint32_t)count);   // count < 2^31
    uint32_t sw = o[1];
    if (common) {
        uint32_t c[4];
        rd::philox(0xFFFFFFFFu, 0xFFFFFFFFu, d, 1u, k0, k1, c);
        sw = c[0];
    }
    const int2 v = make_int2((int)((pushed - count + rank) % capacity), (int)mulhi_map(sw, span));
    scratch[b] = v;
    if (idx_out) {
        idx_out[2 * b] = v.x;
        idx_out[2 * b + 1] = v.y;
    }
}

// one output tensor [T][B][W] of a window batch: element (p, b, f) <- field FIELD + f of record
// start + p - PREV of the window's episode (zero when PREV reaches before record 0)
template <int W, int FIELD, int PREV>
__device__ __forceinline__ void gather_windows(const float* __restrict__ ring, const int2* __restrict__ scratch,
                                               float* __restrict__ out, uint32_t T, uint32_t B) {
    const uint32_t total = T * B * W;   // < 2^32: B <= 2^22, T <= 50, W <= 11
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
        const uint32_t row = e / W, f = e - row * W;
        const uint32_t p = row / B, b = row - p * B;
        const int2 v = scratch[b];
        const int j = v.y + (int)p - PREV;
        out[e] = j >= 0 ? ring[((int64_t)v.x * kSteps + j) * kRec + FIELD + f] : 0.0f;
        if (e + stride < e) break;   // the 32-bit index would wrap
    }
}

__global__ __launch_bounds__(kBlock) void replay_gather_windows_kernel(const float* __restrict__ ring,
                                                                      const int2* __restrict__ scratch,
                                                                      float* __restrict__ ob_w,
                                                                      float* __restrict__ prev_w,
                                                                      float* __restrict__ t_w,
                                                                      float* __restrict__ prew_w, uint32_t T,
                                                                      uint32_t B) {
    switch (blockIdx.y) {
    case 0: gather_windows<kOb, 0, 0>(ring, scratch, ob_w, T, B); break;
    case 1: gather_windows<kPd, F_T, 1>(ring, scratch, prev_w, T, B); break;
    case 2: gather_windows<kPd, F_T, 0>(ring, scratch, t_w, T, B); break;
    default: gather_windows<1, F_REW, 1>(ring, scratch, prew_w, T, B); break;
    }
}

// rows: x [B][16] as float4 quads (ob 0..10 | prev t 11..14 | prev rew 15), t_pdflat [B][4]
__global__ __launch_bounds__(kBlock) void replay_gather_rows_kernel(const float* __restrict__ ring,
                                                                   const int2* __restrict__ scratch,
                                                                   float* __restrict__ x, float* __restrict__ t_pdflat,
                                                                   uint32_t B) {
    const uint32_t total = B * 4;
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
        const uint32_t b = e >> 2, q = e & 3;
        const int2 v = scratch[b];
        const float* rec = ring + ((int64_t)v.x * kSteps + v.y) * kRec;
        if (blockIdx.y == 1) {
            t_pdflat[e] = rec[F_T + q];
            continue;
        }
        float r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int f = (int)q * 4 + c;   // field of the row
            if (f < kOb) r[c] = rec[f];
            else if (v.y == 0) r[c] = 0.0f;
            else r[c] = f < kOb + kPd ? rec[-kRec + F_T + (f - kOb)] : rec[-kRec + F_REW];
        }
        reinterpret_cast<float4*>(x)[e] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

int grid_for(int64_t elements) {
    const int64_t g = (elements + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

}  // namespace

// struct rd_replay: replay_internal.h (shared with replay_priority.hip)

extern "C" {

int rd_replay_create(rd_replay** out, const rd_replay_config* cfg, float* ring, int device, void* hip_stream) {
    if (!out) return rd::set_error(RD_EINVAL, "rd_replay_create: null out");
    if (!cfg) return rd::set_error(RD_EINVAL, "rd_replay_create: null config");
    if (cfg->capacity < 1 || cfg->capacity > 0x7FFFFFFF)
        return rd::set_error(RD_EINVAL, "rd_replay_create: capacity %lld outside 1 .. 2^31 - 1", (long long)cfg->capacity);
    if (cfg->max_batch < 1 || cfg->max_batch > RD_REPLAY_MAX_BATCH)
        return rd::set_error(RD_EINVAL, "rd_replay_create: max_batch %lld outside 1 .. %d", (long long)cfg->max_batch,
                             RD_REPLAY_MAX_BATCH);
    rd::DeviceGuard g(device);
    RD_HIP(g.err, "rd_replay_create: hipSetDevice");
    rd_replay* h = new (std::nothrow) rd_replay();
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_create: out of host memory");
    h->capacity = cfg->capacity;
    h->max_batch = cfg->max_batch;
    h->device = device;
    h->stream = (hipStream_t)hip_stream;
    h->ring = ring;
    const size_t ring_bytes = sizeof(float) * kSteps * kRec * (size_t)cfg->capacity;
    hipError_t err = hipMalloc(&h->hdr, sizeof(Header));
    if (err == hipSuccess) err = hipMalloc(&h->scratch, sizeof(int2) * (size_t)cfg->max_batch);
    if (err == hipSuccess && !ring) {
        err = hipMalloc(&h->ring, ring_bytes);
        h->owns_ring = err == hipSuccess;
        if (err == hipSuccess) err = hipMemsetAsync(h->ring, 0, ring_bytes, h->stream);
    }
    if (err == hipSuccess) err = hipMemsetAsync(h->hdr, 0, sizeof(Header), h->stream);
    if (err == hipSuccess) err = hipMemsetAsync(h->scratch, 0, sizeof(int2) * (size_t)cfg->max_batch, h->stream);
    if (err != hipSuccess) {
        rd_replay_destroy(h);
        return rd::hip_fail(err, "rd_replay_create: allocation");
    }
    *out = h;
    return RD_OK;
}

int rd_replay_destroy(rd_replay* h) {
    if (!h) return RD_OK;
    rd::DeviceGuard g(h->device);
    if (h->hdr) (void)hipFree(h->hdr);
    if (h->scratch) (void)hipFree(h->scratch);
    if (h->owns_ring && h->ring) (void)hipFree(h->ring);
    rd::replay_prio_destroy(h);
    delete h;
    return RD_OK;
}

int rd_replay_set_stream(rd_replay* h, void* hip_stream) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_set_stream: null handle");
    h->stream = (hipStream_t)hip_stream;
    return RD_OK;
}

int rd_replay_reset(rd_replay* h) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_reset: null handle");
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_reset: hipSetDevice");
    RD_HIP(hipMemsetAsync(h->hdr, 0, sizeof(Header), h->stream), "rd_replay_reset: hipMemsetAsync");
    h->host_pushed = 0;
    return RD_OK;
}

float* rd_replay_ring(rd_replay* h) { return h ? h->ring : nullptr; }

int rd_replay_counters(rd_replay* h, int64_t* pushed, int64_t* draws) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_counters: null handle");
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_counters: hipSetDevice");
    Header host;
    RD_HIP(hipMemcpyAsync(&host, h->hdr, sizeof(Header), hipMemcpyDeviceToHost, h->stream),
           "rd_replay_counters: hipMemcpyAsync");
    RD_HIP(hipStreamSynchronize(h->stream), "rd_replay_counters: hipStreamSynchronize");
    if (pushed) *pushed = host.pushed;
    if (draws) *draws = host.draws;
    return RD_OK;
}

// the K / n_envs / capacity rules the step-major pushes share; episodes = (K / 50) n_envs
static int check_steps(const char* fn, const rd_replay* h, int64_t steps, int64_t n_envs, int64_t* episodes) {
    if (steps < 1 || steps % kSteps)
        return rd::set_error(RD_EINVAL, "%s: steps %lld is not a positive multiple of 50", fn, (long long)steps);
    if (n_envs < 1 || n_envs > 0x7FFFFFFF)
        return rd::set_error(RD_EINVAL, "%s: n_envs %lld outside 1 .. 2^31 - 1", fn, (long long)n_envs);
    if (steps / kSteps > 0x7FFFFFFF / n_envs || (steps / kSteps) * n_envs > h->capacity)
        return rd::set_error(RD_EINVAL, "%s: (steps / 50) n_envs = %lld x %lld episodes exceed the capacity %lld", fn,
                             (long long)(steps / kSteps), (long long)n_envs, (long long)h->capacity);
    *episodes = (steps / kSteps) * n_envs;
    return RD_OK;
}

static int bump(const char* what, rd_replay* h, int64_t pushed, int64_t draws) {
    hipLaunchKernelGGL(replay_bump_kernel, dim3(1), dim3(64), 0, h->stream, h->hdr, pushed, draws);
    RD_HIP(hipGetLastError(), what);
    h->host_pushed += pushed;
    return RD_OK;
}

// the end of every push: with priorities enabled the launch that writes the pushed slots' entries
// (reacher_replay_priority.h), then the bump
static int push_done(const char* what, rd_replay* h, int64_t episodes) {
    if (h->prio.enabled)
        if (int rc = rd::replay_prio_push_init(what, h, episodes)) return rc;
    return bump(what, h, episodes, 0);
}

int rd_replay_push_steps(rd_replay* h, const float* records, int64_t steps, int64_t n_envs) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_push_steps: null handle");
    if (!records) return rd::set_error(RD_EINVAL, "rd_replay_push_steps: null records");
    int64_t E = 0;
    if (int rc = check_steps("rd_replay_push_steps", h, steps, n_envs, &E)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_push_steps: hipSetDevice");
    hipLaunchKernelGGL(replay_push_steps_kernel, dim3(grid_for(E * kSteps * kRec)), dim3(kBlock), 0, h->stream, h->ring,
                       h->hdr, records, E, n_envs, h->capacity);
    RD_HIP(hipGetLastError(), "rd_replay_push_steps: launch");
    return push_done("rd_replay_push_steps: bump launch", h, E);
}

int rd_replay_push_episodes(rd_replay* h, const float* records, int64_t episodes) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_push_episodes: null handle");
    if (!records) return rd::set_error(RD_EINVAL, "rd_replay_push_episodes: null records");
    if (episodes < 1) return rd::set_error(RD_EINVAL, "rd_replay_push_episodes: episodes %lld < 1", (long long)episodes);
    if (episodes > h->capacity)
        return rd::set_error(RD_EINVAL, "rd_replay_push_episodes: episodes %lld exceed the capacity %lld",
                             (long long)episodes, (long long)h->capacity);
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_push_episodes: hipSetDevice");
    hipLaunchKernelGGL(replay_push_episodes_kernel, dim3(grid_for(episodes * kSteps * kRec)), dim3(kBlock), 0, h->stream,
                       h->ring, h->hdr, records, episodes, h->capacity);
    RD_HIP(hipGetLastError(), "rd_replay_push_episodes: launch");
    return push_done("rd_replay_push_episodes: bump launch", h, episodes);
}

// rd_replay_push_rows and rd_replay_push_rows_flags, `fn` naming the caller; flags: the latter's
// per-row stepped_with (required there)
static int push_rows(const char* fn, rd_replay* h, const float* x, const float* t_pdflat, const float* s_pdflat,
                     const float* reward, const float* carry, int64_t steps, int64_t n_envs, float stepped_with,
                     const float* with_rows, bool flags) {
    if (!h) return rd::set_error(RD_EINVAL, "%s: null handle", fn);
    if (!x) return rd::set_error(RD_EINVAL, "%s: null x", fn);
    if (!t_pdflat) return rd::set_error(RD_EINVAL, "%s: null t_pdflat", fn);
    if (!reward) return rd::set_error(RD_EINVAL, "%s: null reward", fn);
    if (flags && !with_rows) return rd::set_error(RD_EINVAL, "%s: null stepped_with_rows", fn);
    int64_t E = 0;
    if (int rc = check_steps(fn, h, steps, n_envs, &E)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, fn);
    hipLaunchKernelGGL(replay_push_rows_kernel, dim3(grid_for(E * kSteps * kRec)), dim3(kBlock), 0, h->stream, h->ring,
                       h->hdr, x, t_pdflat, s_pdflat, reward, carry, E, n_envs, h->capacity, stepped_with, with_rows);
    RD_HIP(hipGetLastError(), fn);
    return push_done(fn, h, E);
}

int rd_replay_push_rows(rd_replay* h, const float* x, const float* t_pdflat, const float* s_pdflat, const float* reward,
                        const float* carry, int64_t steps, int64_t n_envs, float stepped_with) {
    return push_rows("rd_replay_push_rows", h, x, t_pdflat, s_pdflat, reward, carry, steps, n_envs, stepped_with, nullptr,
                     false);
}

int rd_replay_push_rows_flags(rd_replay* h, const float* x, const float* t_pdflat, const float* s_pdflat,
                              const float* reward, const float* carry, int64_t steps, int64_t n_envs,
                              const float* stepped_with_rows) {
    return push_rows("rd_replay_push_rows_flags", h, x, t_pdflat, s_pdflat, reward, carry, steps, n_envs, 0.0f,
                     stepped_with_rows, true);
}

// the checks both samples share; those that need no handle come first
static int check_sample(const char* fn, const rd_replay* h, const rd_replay_sample* s) {
    if (s->windows < 1) return rd::set_error(RD_EINVAL, "%s: windows %lld < 1", fn, (long long)s->windows);
    if (s->window_base < 0) return rd::set_error(RD_EINVAL, "%s: negative window_base", fn);
    if (s->recent < 0) return rd::set_error(RD_EINVAL, "%s: negative recent", fn);
    if (s->windows > h->max_batch)
        return rd::set_error(RD_EINVAL, "%s: windows %lld exceed max_batch %lld", fn, (long long)s->windows,
                             (long long)h->max_batch);
    if (h->host_pushed < 1) return rd::set_error(RD_EINVAL, "%s: the ring has never been pushed to", fn);
    return RD_OK;
}

static int draw(const char* what, rd_replay* h, const rd_replay_sample* s, int32_t* idx, uint32_t span, int common) {
    hipLaunchKernelGGL(replay_draw_kernel, dim3((unsigned)((s->windows + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       h->stream, h->hdr, h->scratch, idx, s->windows, s->window_base, s->recent, s->seed, h->capacity,
                       span, common);
    RD_HIP(hipGetLastError(), what);
    return RD_OK;
}

int rd_replay_sample_windows(rd_replay* h, const rd_replay_sample* s, float* ob_w, float* prev_w, float* t_w,
                             float* prew_w, int32_t* idx) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: null handle");
    if (!s) return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: null sample");
    if (!ob_w) return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: null ob_w");
    if (!prev_w) return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: null prev_w");
    if (!t_w) return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: null t_w");
    if (s->steps < 1 || s->steps > kSteps)
        return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: steps %d outside 1 .. 50", s->steps);
    if (s->start_mode != RD_REPLAY_START_PER_WINDOW && s->start_mode != RD_REPLAY_START_COMMON)
        return rd::set_error(RD_EINVAL, "rd_replay_sample_windows: unknown start_mode %d", s->start_mode);
    if (int rc = check_sample("rd_replay_sample_windows", h, s)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_sample_windows: hipSetDevice");
    if (int rc = draw("rd_replay_sample_windows: draw launch", h, s, idx, (uint32_t)(kSteps + 1 - s->steps),
                      s->start_mode == RD_REPLAY_START_COMMON))
        return rc;
    if (int rc = rd::replay_gather_windows("rd_replay_sample_windows: gather launch", h, ob_w, prev_w, t_w, prew_w,
                                           s->steps, s->windows))
        return rc;
    return bump("rd_replay_sample_windows: bump launch", h, 0, 1);
}

int rd_replay_sample_rows(rd_replay* h, const rd_replay_sample* s, float* x, float* t_pdflat, int32_t* idx) {
    if (!h) return rd::set_error(RD_EINVAL, "rd_replay_sample_rows: null handle");
    if (!s) return rd::set_error(RD_EINVAL, "rd_replay_sample_rows: null sample");
    if (!x) return rd::set_error(RD_EINVAL, "rd_replay_sample_rows: null x");
    if (!t_pdflat) return rd::set_error(RD_EINVAL, "rd_replay_sample_rows: null t_pdflat");
    if ((uintptr_t)x & 15) return rd::set_error(RD_EINVAL, "rd_replay_sample_rows: x is not 16-byte aligned");
    if (int rc = check_sample("rd_replay_sample_rows", h, s)) return rc;
    rd::DeviceGuard g(h->device);
    RD_HIP(g.err, "rd_replay_sample_rows: hipSetDevice");
    if (int rc = draw("rd_replay_sample_rows: draw launch", h, s, idx, (uint32_t)kSteps, 0)) return rc;
    if (int rc = rd::replay_gather_rows("rd_replay_sample_rows: gather launch", h, x, t_pdflat, s->windows)) return rc;
    return bump("rd_replay_sample_rows: bump launch", h, 0, 1);
}

}  // extern "C"

// what replay_priority.hip launches of this file's kernels (replay_internal.h)
namespace rd {

int replay_gather_rows(const char* what, rd_replay* h, float* x, float* t_pdflat, int64_t rows) {
    hipLaunchKernelGGL(replay_gather_rows_kernel, dim3(grid_for(rows * 4), 2), dim3(kBlock), 0, h->stream, h->ring,
                       h->scratch, x, t_pdflat, (uint32_t)rows);
    RD_HIP(hipGetLastError(), what);
    return RD_OK;
}

int replay_gather_windows(const char* what, rd_replay* h, float* ob_w, float* prev_w, float* t_w, float* prew_w,
                          int32_t steps, int64_t windows) {
    const int64_t ob_elems = (int64_t)steps * windows * kOb;
    hipLaunchKernelGGL(replay_gather_windows_kernel, dim3(grid_for(ob_elems), prew_w ? 4 : 3), dim3(kBlock), 0, h->stream,
                       h->ring, h->scratch, ob_w, prev_w, t_w, prew_w, (uint32_t)steps, (uint32_t)windows);
    RD_HIP(hipGetLastError(), what);
    return RD_OK;
}

int replay_bump(const char* what, rd_replay* h, int64_t pushed, int64_t draws) { return bump(what, h, pushed, draws); }

}  // namespace rd
