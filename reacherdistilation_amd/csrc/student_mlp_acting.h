// The launches of the reference MLP student's closed-loop instances beyond the plain ones, one function
// per tier (rd::Tier, rd_acting.h) and kernel family: student_mlp_envs_kernel's mixed, noisy and faulty
// instances and student_mlp_evaluate_kernel's noisy and faulty ones.  Each tier lives in a translation
// unit of its own -- student_mlp_mix.hip, student_mlp_noise.hip, student_mlp_faults.hip -- because
// hipcc's layout of an instance depends on which twins share its unit: instantiated inside
// student_mlp.hip, a tier's instances make hipcc lay out anew the instances they are the twins of, even
// with the tier's statements compiled out of those, and merged into one unit the three tiers move the
// mixed instances (profiles/envs_teacher_share_isa.txt, envs_action_noise_isa.txt, envs_obs_faults_isa.txt,
// acting_refactor_isa.txt).  Every instance's instruction text is kept as it was.
#pragma once
#include <hip/hip_runtime.h>

#include "rd_acting.h"

namespace rd {

struct MlpEnvsLaunch {
    const void* args;        // the call's SmEnvsArgs (student_mlp_envs.h), filled as for the plain instance
    const Acting* act;       // the handle's settings: what the tier's argument struct adds
    bool student;            // RDM_ACT_STUDENT (the noisy tier alone has teacher instances)
    bool bf, small;          // the bf16 layers; 16-env blocks
    unsigned grid, threads;
    hipStream_t stream;
};

struct MlpEvalLaunch {
    const void* args;        // the call's SmEvalArgs (student_mlp_eval.h)
    const Acting* act;       // the call's noise (RD_NOISE_NONE: the mean acts) and faults
    bool bf, small;
    unsigned grid, threads;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_mlp_envs_mixed(const MlpEnvsLaunch& l);
hipError_t launch_mlp_envs_noisy(const MlpEnvsLaunch& l);
hipError_t launch_mlp_envs_faulty(const MlpEnvsLaunch& l);
hipError_t launch_mlp_eval_noisy(const MlpEvalLaunch& l);
hipError_t launch_mlp_eval_faulty(const MlpEvalLaunch& l);

}  // namespace rd
