// The launch of student_mlp_envs_kernel's mixed instances (DAgger's beta-mixture,
// rdm_envs_set_teacher_share), which live in a translation unit of their own, student_mlp_mix.hip:
// instantiated inside student_mlp.hip, each of them makes hipcc lay out anew the student instance it is
// the twin of, even with the mixture's statements compiled out of it
// (profiles/envs_teacher_share_isa.txt), and those six instances' instruction text is kept as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rd {

struct MlpEnvsMixLaunch {
    const void* args;        // the call's SmEnvsArgs (student_mlp_envs.h), filled as for the student instance
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
    float* stepped_with;     // [K][n] or null
    bool bf, small;          // the bf16 layers; 16-env blocks
    unsigned grid, threads;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_mlp_envs_mixed(const MlpEnvsMixLaunch& l);

}  // namespace rd
