// The replay ring's handle and the few host entry points its two translation units share:
// replay.hip (the ring: pushes, uniform draws, gathers) and replay_priority.hip (the priority table
// and the weighted draw, include/reacher_replay_priority.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_replay_priority.h"

namespace rd {

struct ReplayHeader {
    int64_t pushed;
    int64_t draws;
};

// the priority side of a handle; all zero while priorities are off
struct ReplayPrio {
    bool enabled = false;
    bool owns_table = false;
    rd_replay_prio_config cfg = {};
    uint32_t* table = nullptr;     // q [capacity][50]
    uint64_t* weights = nullptr;   // E_j, then X_j in place [capacity]
    uint64_t* partials = nullptr;  // per scan tile [ceil(capacity / tile)], then the total
};

// replay.hip: the gathers on h->scratch and the counter bump, as the uniform samples launch them
int replay_gather_rows(const char* what, rd_replay* h, float* x, float* t_pdflat, int64_t rows);
int replay_gather_windows(const char* what, rd_replay* h, float* ob_w, float* prev_w, float* t_w, float* prew_w,
                          int32_t steps, int64_t windows);
int replay_bump(const char* what, rd_replay* h, int64_t pushed, int64_t draws);
// replay_priority.hip: the launch a push adds while priorities are enabled (before its bump)
int replay_prio_push_init(const char* what, rd_replay* h, int64_t episodes);
void replay_prio_destroy(rd_replay* h);

}  // namespace rd

struct rd_replay {
    int64_t capacity = 0, max_batch = 0;
    int64_t host_pushed = 0;   // pushes ISSUED; only to refuse a sample from a ring never pushed to
    float* ring = nullptr;
    bool owns_ring = false;
    rd::ReplayHeader* hdr = nullptr;
    int2* scratch = nullptr;   // idx [max_batch]
    int device = 0;
    hipStream_t stream = nullptr;
    rd::ReplayPrio prio;
};
