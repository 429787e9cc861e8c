// rd_mask_obs (include/reacher_obs_faults.h): the sensor faults of the students' closed loop as a
// stepwise primitive -- one small kernel over n envs that calls the device functions the fused kernels
// inline (rd::obs_fault_keep, rd::obs_fault_see in rd_physics.h), so a stepwise loop
// { teacher forward, rd_mask_obs, student forward on the masked row, rd_step } steps its envs with the
// fused calls' bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_obs_faults.h"
#include "rd_common.h"
#include "rd_obs_faults.h"
#include "rd_physics.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void mask_obs_kernel(rd_obs_faults of, int64_t env_base, int64_t n, int32_t episode,
                                                          int32_t step, const float* __restrict__ ob,
                                                          float* __restrict__ seen, uint8_t* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = rd::obs_fault_keep(of.seed, (uint64_t)(env_base + i), episode, step, of.keep_prob);
#pragma unroll
    for (int k = 0; k < rd::kObsDim; ++k) {
        seen[i * rd::kObsDim + k] = rd::obs_fault_see(of.mode, of.keep_prob, bits, k, ob[i * rd::kObsDim + k]);
        if (kept) kept[i * rd::kObsDim + k] = (uint8_t)((bits >> k) & 1u);
    }
}

}  // namespace

extern "C" int rd_mask_obs(const rd_obs_faults* of, int64_t env_base, int64_t n, int32_t episode, int32_t step,
                           const float* ob, float* seen, uint8_t* kept, int device, void* hip_stream) {
    const char* fn = "rd_mask_obs";
    if (int rc = rd::check_obs_faults(fn, of, true)) return rc;
    if (!ob) return rd::set_error(RD_EINVAL, "%s: null ob", fn);
    if (!seen) return rd::set_error(RD_EINVAL, "%s: null seen", fn);
    if (n < 1 || n > ((int64_t)1 << 31)) return rd::set_error(RD_EINVAL, "%s: n %lld outside 1 .. 2^31", fn, (long long)n);
    if (env_base < 0) return rd::set_error(RD_EINVAL, "%s: negative env_base", fn);
    if (episode < 0) return rd::set_error(RD_EINVAL, "%s: negative episode", fn);
    if (step < 0 || step >= rd::kEpisodeSteps)
        return rd::set_error(RD_EINVAL, "%s: step %d outside 0 .. %d", fn, (int)step, rd::kEpisodeSteps - 1);
    rd::DeviceGuard g(device);
    RD_HIP(g.err, "rd_mask_obs: hipSetDevice");
    hipLaunchKernelGGL(mask_obs_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, *of, env_base, n, episode, step, ob, seen, kept);
    RD_HIP(hipGetLastError(), "rd_mask_obs: launch");
    return RD_OK;
}
