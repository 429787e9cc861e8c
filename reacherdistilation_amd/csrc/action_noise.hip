// rd_perturb_actions (include/reacher_action_noise.h): the action noise of the students' closed loop
// as a stepwise primitive -- one small kernel over n envs that calls the device functions the fused
// kernels inline (rd::action_noise_draw, rd::action_noise_apply in rd_physics.h), so a stepwise loop
// { forward, rd_perturb_actions, rd_step } steps its envs with the fused calls' bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_action_noise.h"
#include "rd_action_noise.h"
#include "rd_common.h"
#include "rd_physics.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void perturb_actions_kernel(rd_action_noise nz, int64_t env_base, int64_t n,
                                                                 int32_t episode, int32_t step,
                                                                 const float* __restrict__ pdflat,
                                                                 float* __restrict__ actions, float* __restrict__ xi) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float xi0, xi1, a0, a1;
    rd::action_noise_draw(nz.seed, (uint64_t)(env_base + i), episode, step, xi0, xi1);
    const float* p = pdflat + i * 4;
    rd::action_noise_apply(nz.mode, nz.scale, xi0, xi1, p[0], p[1], p[2], p[3], a0, a1);
    actions[2 * i] = a0;
    actions[2 * i + 1] = a1;
    if (xi) {
        xi[2 * i] = xi0;
        xi[2 * i + 1] = xi1;
    }
}

}  // namespace

extern "C" int rd_perturb_actions(const rd_action_noise* nz, int64_t env_base, int64_t n, int32_t episode, int32_t step,
                                  const float* pdflat, float* actions, float* xi, int device, void* hip_stream) {
    const char* fn = "rd_perturb_actions";
    if (int rc = rd::check_action_noise(fn, nz, true)) return rc;
    if (!pdflat) return rd::set_error(RD_EINVAL, "%s: null pdflat", fn);
    if (!actions) return rd::set_error(RD_EINVAL, "%s: null actions", fn);
    if (n < 1 || n > ((int64_t)1 << 31)) return rd::set_error(RD_EINVAL, "%s: n %lld outside 1 .. 2^31", fn, (long long)n);
    if (env_base < 0) return rd::set_error(RD_EINVAL, "%s: negative env_base", fn);
    if (episode < 0) return rd::set_error(RD_EINVAL, "%s: negative episode", fn);
    if (step < 0 || step >= rd::kEpisodeSteps)
        return rd::set_error(RD_EINVAL, "%s: step %d outside 0 .. %d", fn, (int)step, rd::kEpisodeSteps - 1);
    rd::DeviceGuard g(device);
    RD_HIP(g.err, "rd_perturb_actions: hipSetDevice");
    hipLaunchKernelGGL(perturb_actions_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, *nz, env_base, n, episode, step, pdflat, actions, xi);
    RD_HIP(hipGetLastError(), "rd_perturb_actions: launch");
    return RD_OK;
}
