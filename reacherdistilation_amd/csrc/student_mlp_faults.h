// The launches of the reference MLP student's faulty closed-loop instances (sensor faults on the
// student's observation, include/reacher_obs_faults.h): student_mlp_envs_kernel's for
// rdm_envs_set_obs_faults and student_mlp_evaluate_kernel's for rdm_evaluate_faulty.  They live in a
// translation unit of their own, student_mlp_faults.hip, for student_mlp_noise.h's reason: the
// instances they are the twins of keep their instruction text (profiles/envs_obs_faults_isa.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_action_noise.h"
#include "../../include/reacher_obs_faults.h"

namespace rd {

// a student call's (RDM_ACT_STUDENT): the instance carries the coin and the noise too, either of
// which may be off (beta = 0 never fires; RD_NOISE_NONE steps with the mean)
struct MlpEnvsFaultLaunch {
    const void* args;        // the call's SmEnvsArgs (student_mlp_envs.h), filled as for the plain instance
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
    float* stepped_with;     // [K][n] or null
    rd_action_noise noise;
    float* actions;          // [K][n][2] or null
    rd_obs_faults faults;    // RD_OBS_DROPOUT or RD_OBS_MISSING
    bool bf, small;          // the bf16 layers; 16-env blocks
    unsigned grid, threads;
    hipStream_t stream;
};

struct MlpEvalFaultLaunch {
    const void* args;        // the call's SmEvalArgs (student_mlp_eval.h)
    rd_action_noise noise;   // RD_NOISE_NONE: the mean acts
    rd_obs_faults faults;
    bool bf, small;
    unsigned grid, threads;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_mlp_envs_faulty(const MlpEnvsFaultLaunch& l);
hipError_t launch_mlp_eval_faulty(const MlpEvalFaultLaunch& l);

}  // namespace rd
