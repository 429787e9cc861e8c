// The launches of the reference MLP student's noisy closed-loop instances (action noise,
// include/reacher_action_noise.h): student_mlp_envs_kernel's for rdm_envs_set_action_noise /
// rdm_envs_bind_actions and student_mlp_evaluate_kernel's for rdm_evaluate_noisy.  They live in a
// translation unit of their own, student_mlp_noise.hip, for student_mlp_mix.h's reason: instantiated
// inside student_mlp.hip they make hipcc lay out anew the instances they are the twins of, and those
// instances' instruction text is kept as it was (profiles/envs_action_noise_isa.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_action_noise.h"

namespace rd {

struct MlpEnvsNoiseLaunch {
    const void* args;        // the call's SmEnvsArgs (student_mlp_envs.h), filled as for the plain instance
    bool student;            // RDM_ACT_STUDENT: the instance carries the coin (beta = 0 never fires)
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
    float* stepped_with;     // [K][n] or null (student calls; a teacher call's is cleared by the host)
    rd_action_noise noise;
    float* actions;          // [K][n][2] or null
    bool bf, small;          // the bf16 layers; 16-env blocks
    unsigned grid, threads;
    hipStream_t stream;
};

struct MlpEvalNoiseLaunch {
    const void* args;        // the call's SmEvalArgs (student_mlp_eval.h)
    rd_action_noise noise;
    bool bf, small;
    unsigned grid, threads;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_mlp_envs_noisy(const MlpEnvsNoiseLaunch& l);
hipError_t launch_mlp_eval_noisy(const MlpEvalNoiseLaunch& l);

}  // namespace rd
