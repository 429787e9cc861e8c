// The teacher inside another translation unit's kernels: the 2x64 MlpPolicy's layouts and exact-f32
// forward, the definitions distill.hip compiles, in a namespace of their own (their WAVES, BLOCK,
// N_MET ... are not the including file's).  Included inside the anonymous namespace of
// student_mlp.hip (by student_mlp_eval.h) and of student_lstm.hip (by student_lstm_query.h); expects
// rd_device.h.
#pragma once

namespace tch {
using rd::f32x4, rd::mfma, rd::ld4, rd::kTanhScale, rd::tanh_pre;
constexpr bool kFenceAll = false;   // the all-fenced diagnostic build is distill.hip's; mlp_forward<true> is fenced
#include "distill_layout.h"
#include "distill_forward_f32.h"
}  // namespace tch
