// How a student's closed loop acts (student_mlp.hip, student_lstm.hip): the handle's acting settings --
// DAgger's beta-mixture, the action noise, the sensor faults and the buffers bound for what they record
// -- the validated setters and getters behind rd?_envs_set_* / rd?_envs_bind_*, and the one rule that
// picks the tier of kernel instances a call launches.  Host only, and like rd_host.h it knows no
// trainer's type: a trainer holds one rd::Acting and its ABI functions forward here with their name as
// `fn` and the handle's settings as `a` (null for a null handle).
#pragma once
#include <stdint.h>

#include "rd_action_noise.h"
#include "rd_common.h"
#include "rd_obs_faults.h"

namespace rd {

// Host-side settings of the handle, not of its envs: attach and reset leave them
struct Acting {
    float beta = 0.0f;               // the teacher's share of a student call's env steps
    uint64_t coin_seed = 0;          // the coins' Philox key
    float* stepped_with = nullptr;   // the caller's buffer [stepped_rows] or null (the MLP student's alone)
    int64_t stepped_rows = 0;
    rd_action_noise noise{RD_NOISE_NONE, 1.0f, 0};
    float* actions = nullptr;        // the caller's buffer [action_rows][2] of the actions that stepped, or null
    int64_t action_rows = 0;
    rd_obs_faults faults{RD_OBS_CLEAN, 1.0f, 0};   // on what the student reads in a student call
};

// The kernel instances of a call, each tier carrying the ones before it as run-time arguments that may
// be off (beta = 0 never fires; RD_NOISE_NONE steps with the mean):
//  Faulty  a student call with a fault mode set.  A teacher call evaluates no student: it ignores the
//          faults and the mixture and launches what it launched without them;
//  Noisy   either actor, once a noise is set or an actions buffer wants the actions;
//  Mixed   a student call once a coin can fall (beta > 0) or a stepped_with buffer wants its flags;
//  Plain   otherwise: the launch that was there before any of them, with the arguments it always had.
// The evaluations build an Acting from the rd_action_noise / rd_obs_faults they are given (student = true).
enum class Tier { Plain, Mixed, Noisy, Faulty };

inline Tier tier_of(const Acting& a, bool student_acts) {
    if (student_acts && a.faults.mode != RD_OBS_CLEAN) return Tier::Faulty;
    if (a.noise.mode != RD_NOISE_NONE || a.actions) return Tier::Noisy;
    if (student_acts && (a.beta > 0.0f || a.stepped_with)) return Tier::Mixed;
    return Tier::Plain;
}

// a handle's settings, null for a null handle
template <class Trainer>
auto acting_of(Trainer* t) -> decltype(&t->act) {
    return t ? &t->act : nullptr;
}

inline int set_teacher_share(const char* fn, Acting* a, float beta, uint64_t coin_seed) {
    if (!a) return set_error(RD_EINVAL, "%s: null trainer", fn);
    if (!(beta >= 0.0f && beta <= 1.0f))   // NaN too
        return set_error(RD_EINVAL, "%s: beta %g outside 0 .. 1", fn, (double)beta);
    a->beta = beta;
    a->coin_seed = coin_seed;
    return RD_OK;
}

inline float teacher_share(const Acting* a) { return a ? a->beta : -1.0f; }

inline int set_action_noise(const char* fn, Acting* a, const rd_action_noise* nz) {
    if (!a) return set_error(RD_EINVAL, "%s: null trainer", fn);
    if (int rc = check_action_noise(fn, nz, true)) return rc;
    a->noise = *nz;
    return RD_OK;
}

inline int get_action_noise(const char* fn, const Acting* a, rd_action_noise* out) {
    if (!a || !out) return set_error(RD_EINVAL, "%s: null trainer or out", fn);
    *out = a->noise;
    return RD_OK;
}

// the setting before the handle
inline int set_obs_faults(const char* fn, Acting* a, const rd_obs_faults* of) {
    if (int rc = check_obs_faults(fn, of, true)) return rc;
    if (!a) return set_error(RD_EINVAL, "%s: null trainer", fn);
    a->faults = *of;
    return RD_OK;
}

inline int get_obs_faults(const char* fn, const Acting* a, rd_obs_faults* out) {
    if (!a || !out) return set_error(RD_EINVAL, "%s: null trainer or out", fn);
    *out = a->faults;
    return RD_OK;
}

// a caller's buffer of `rows` rows into one of the Acting's (buffer, rows) pairs; a null buf unbinds
inline int bind_rows(const char* fn, Acting* a, float* Acting::*buf_of, int64_t Acting::*rows_of, float* buf,
                     int64_t rows) {
    if (!a) return set_error(RD_EINVAL, "%s: null trainer", fn);
    if (buf && rows < 1) return set_error(RD_EINVAL, "%s: rows %lld < 1", fn, (long long)rows);
    a->*buf_of = buf;
    a->*rows_of = buf ? rows : 0;
    return RD_OK;
}

inline int bind_actions(const char* fn, Acting* a, float* buf, int64_t rows) {
    return bind_rows(fn, a, &Acting::actions, &Acting::action_rows, buf, rows);
}

inline int bind_stepped_with(const char* fn, Acting* a, float* buf, int64_t rows) {
    return bind_rows(fn, a, &Acting::stepped_with, &Acting::stepped_rows, buf, rows);
}

// envs_check's part: a call of `steps` steps of n envs fits the bound buffers.  The binding function it
// names carries the ABI prefix, fn's first three characters
inline int check_bound_rows(const char* fn, const Acting& a, int steps, int64_t n) {
    if (a.stepped_with && (int64_t)steps * n > a.stepped_rows)
        return set_error(RD_EINVAL, "%s: steps x n_envs = %d x %lld > rows = %lld of the stepped_with buffer "
                                    "(%.3s_envs_bind_stepped_with)", fn, steps, (long long)n, (long long)a.stepped_rows, fn);
    if (a.actions && (int64_t)steps * n > a.action_rows)
        return set_error(RD_EINVAL, "%s: steps x n_envs = %d x %lld > rows = %lld of the actions buffer "
                                    "(%.3s_envs_bind_actions)", fn, steps, (long long)n, (long long)a.action_rows, fn);
    return RD_OK;
}

}  // namespace rd
