// Host plumbing that the trainers' C ABI has in common (distill.hip, ppo.hip, student_mlp.hip,
// student_lstm.hip): the list of a handle's device allocations, the read-back of a metrics ring,
// the upload of a teacher net, and the buffers of a student's persistent envs.  Host only: nothing
// here is device code, and nothing knows a trainer's type.  Error strings carry the ABI function's
// name, which every helper takes as `fn`.
#pragma once
#include <stdint.h>

#include <new>
#include <vector>

#include "rd_common.h"

namespace rd {

inline int hip_fail(hipError_t e, const char* fn, const char* stage) {
    return set_error(-(int)e, "%s: %s: %s", fn, stage, hipGetErrorString(e));
}

// The device buffers a handle owns for its whole life.  *_create allocates through it, in order;
// after the first failure every later call does nothing and `err` keeps that failure.  *_destroy
// calls free_all.  Buffers with a shorter life (the envs', freed on re-attach) are not kept here.
struct DeviceAllocs {
    hipStream_t stream = nullptr;   // zeroed() clears on it
    hipError_t err = hipSuccess;
    std::vector<void*> ptrs;

    template <class T>
    void raw(T** p, size_t count) {
        if (err == hipSuccess) err = hipMalloc((void**)p, sizeof(T) * count);
        if (err == hipSuccess) ptrs.push_back(*p);
    }
    template <class T>
    void zeroed(T** p, size_t count) {
        raw(p, count);
        if (err == hipSuccess) err = hipMemsetAsync(*p, 0, sizeof(T) * count, stream);
    }
    void free_all() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// The newest `count` rows of a device ring of `len` rows x n_met floats into out, oldest first;
// `steps` rows have been written so far (row s at s % len).  `noun`: what a row is, for the error.
inline int read_ring(const char* fn, const char* noun, const float* ring, int64_t len, int n_met, int64_t steps,
                     int64_t count, double* out) {
    if (count > steps || count > len)
        return set_error(RD_EINVAL, "%s: only %lld %s kept", fn, (long long)(steps < len ? steps : len), noun);
    float* host = new (std::nothrow) float[(size_t)len * n_met];
    if (!host) return set_error(RD_EINVAL, "%s: out of host memory", fn);
    const hipError_t e = hipMemcpy(host, ring, sizeof(float) * len * n_met, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (int64_t k = 0; k < count; ++k) {
            const int64_t s = (steps - count + k) % len;
            for (int j = 0; j < n_met; ++j) out[k * n_met + j] = host[s * n_met + j];
        }
    delete[] host;
    return e == hipSuccess ? RD_OK : hip_fail(e, fn);
}

// A teacher (or student) net into its device buffer: params [n_params] | ob mean [obd] | ob std [obd]
inline int upload_net(const char* fn, float* dst, const float* params, int n_params, const float* ob_mean,
                      const float* ob_std, int obd, hipStream_t stream) {
    RD_HIP(hipMemcpyAsync(dst, params, sizeof(float) * n_params, hipMemcpyDeviceToDevice, stream), fn);
    RD_HIP(hipMemcpyAsync(dst + n_params, ob_mean, sizeof(float) * obd, hipMemcpyDeviceToDevice, stream), fn);
    RD_HIP(hipMemcpyAsync(dst + n_params + obd, ob_std, sizeof(float) * obd, hipMemcpyDeviceToDevice, stream), fn);
    return RD_OK;
}

// A student's persistent envs (rd?_envs_attach): what both students keep per env
struct EnvBufs {
    int64_t n = 0, base = 0;
    uint64_t seed = 0;
    int grid = 0;               // 0 = the handle's
    float* state = nullptr;     // [state_dim][n] SoA (rd_get_state's layout)
    float* aux = nullptr;       // [aux_rows][n]
    int32_t* clock = nullptr;   // [2][n]: step of the episode, episode

    void release() {
        for (void* p : {(void*)state, (void*)aux, (void*)clock})
            if (p) (void)hipFree(p);
        state = aux = nullptr;
        clock = nullptr;
    }
};

// rd?_envs_attach's argument checks; Cfg = rd?_envs_config
template <class Cfg>
int envs_attach_check(const char* fn, const void* trainer, const Cfg* cfg) {
    if (!trainer) return set_error(RD_EINVAL, "%s: null trainer", fn);
    if (!cfg) return set_error(RD_EINVAL, "%s: null config", fn);
    if (cfg->n_envs < 1 || cfg->n_envs > ((int64_t)1 << 31))
        return set_error(RD_EINVAL, "%s: n_envs %lld outside 1 .. 2^31", fn, (long long)cfg->n_envs);
    if (cfg->env_base < 0) return set_error(RD_EINVAL, "%s: negative env_base", fn);
    if (cfg->grid < 0) return set_error(RD_EINVAL, "%s: negative grid", fn);
    return RD_OK;
}

// cfg's envs into released buffers (not cleared: the caller's reset launch writes every entry)
template <class Cfg>
hipError_t envs_alloc(EnvBufs& e, const Cfg& cfg, int state_dim, int aux_rows) {
    const size_t n = (size_t)cfg.n_envs;
    hipError_t err = hipMalloc((void**)&e.state, sizeof(float) * state_dim * n);
    if (err == hipSuccess) err = hipMalloc((void**)&e.aux, sizeof(float) * aux_rows * n);
    if (err == hipSuccess) err = hipMalloc((void**)&e.clock, sizeof(int32_t) * 2 * n);
    e.n = cfg.n_envs;
    e.base = cfg.env_base;
    e.seed = cfg.seed;
    e.grid = cfg.grid;
    return err;
}

// rd?_envs_get_state: the states to a device buffer, env 0's clock to the host (the envs run in
// lockstep); synchronises the stream
inline int envs_get_state(const char* fn, const EnvBufs& e, int state_dim, hipStream_t stream, float* state,
                          int32_t* step, int32_t* episode) {
    int32_t c[2] = {0, 0};
    hipError_t err = hipMemcpyAsync(state, e.state, sizeof(float) * state_dim * e.n, hipMemcpyDeviceToDevice, stream);
    if (err != hipSuccess) return hip_fail(err, fn, "copy");
    err = hipMemcpyAsync(&c[0], e.clock, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (err == hipSuccess) err = hipMemcpyAsync(&c[1], e.clock + e.n, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (err != hipSuccess) return hip_fail(err, fn, "clock");
    RD_HIP(hipStreamSynchronize(stream), fn);
    if (step) *step = c[0];
    if (episode) *episode = c[1];
    return RD_OK;
}

}  // namespace rd
