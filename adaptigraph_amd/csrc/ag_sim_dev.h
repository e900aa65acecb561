// ag_sim_dev.h — what the four simulator sources (ag_sim.hip, ag_sim_pile.hip, ag_sim_cloth.hip, ag_sim_box.hip) share: the schedule of a push
// (its frames), the schedule checks of their C entries, and the device code that is the same sequence of operations in every kernel.  A model's
// arithmetic, its bounds and its null-pointer checks stay in its own source.
#pragma once
#include "ag_host.h"

namespace {

// the frame written after the settle: behind those of steps 0, record_every, 2 record_every ... < n_push
__host__ __device__ __forceinline__ int sim_final_frame(int n_push, int record_every) { return (n_push - 1) / record_every + 1; }
// frames a push of n_push steps writes
inline int sim_frames(int n_push, int record_every) { return sim_final_frame(n_push, record_every) + 1; }

// The checks every entry makes of E, n_max, the schedule, F_max and h.  `n_name` names the macro that is n_hi; n_push_lo is the fewest steps the
// longest push may have (the cloth's two segments: 2); `has_iters`: iters is an argument of the entry; `noun` is what F_max's message calls a push.
inline int sim_check_schedule(const char *entry, int E, int n_max, int n_lo, int n_hi, const char *n_name, int F_max, int n_push_max, int n_push_lo,
                              int substeps, bool has_iters, int iters, int record_every, int settle, float h, const char *noun)
{
    if (E < 1) return ag_fail(AG_ERR_ARG, "%s: E = %d episodes", entry, E);
    if (n_max < n_lo || n_max > n_hi) return ag_fail(AG_ERR_ARG, "%s: n_max = %d outside %d .. %d (%s)", entry, n_max, n_lo, n_hi, n_name);
    if (n_push_max < n_push_lo || substeps < 1 || (has_iters && iters < 1) || record_every < 1 || settle < 0 ||
        n_push_max > INT32_MAX / substeps - settle - 1) {
        if (has_iters)
            return ag_fail(AG_ERR_ARG, "%s: n_push_max = %d substeps = %d iters = %d record_every = %d settle = %d", entry, n_push_max, substeps,
                           iters, record_every, settle);
        return ag_fail(AG_ERR_ARG, "%s: n_push_max = %d substeps = %d record_every = %d settle = %d", entry, n_push_max, substeps, record_every,
                       settle);
    }
    if (F_max < sim_frames(n_push_max, record_every))
        return ag_fail(AG_ERR_ARG, "%s: F_max = %d frames, a %s of %d steps recorded every %d writes %d", entry, F_max, noun, n_push_max,
                       record_every, sim_frames(n_push_max, record_every));
    if (!(h > 0.f)) return ag_fail(AG_ERR_ARG, "%s: substep h = %g", entry, (double)h);
    return AG_OK;
}

// (uniform over the workgroup) an episode outside its bounds, which the host's checks could not see: no frame, nothing else touched
__device__ __forceinline__ void sim_no_frame(int32_t *n_frames, int e, int t)
{
    if (t == 0) n_frames[e] = 0;
}

// substep s of step st, S substeps a step: t = float(k) inv, k 1-based over the substeps of the push; the tool's centre c = s + (e - s) t
__device__ __forceinline__ float sim_substep_t(int st, int S, int s, float inv) { return (float)(st * S + s + 1) * inv; }
__device__ __forceinline__ void sim_tool_centre(float &cx, float &cz, float sx, float sz, float ex, float ez, float t)
{
    cx = sx + (ex - sx) * t; cz = sz + (ez - sz) * t;
}

// Coulomb friction on the table over one substep: the factor of (vx, vz), mgh = (mu g) h
__device__ __forceinline__ float sim_coulomb(float vx, float vz, float mgh)
{
    const float sp = sqrtf(vx * vx + vz * vz);
    return sp > mgh ? 1.f - mgh / sp : 0.f;
}

// the frame a step st with st % record_every == 0 records into (< F_max: checked on the host against n_push_max)
__device__ __forceinline__ int sim_recorded_frame(int st, int record_every) { return st / record_every; }

__device__ __forceinline__ void sim_store3(float *o, float x, float y, float z) { o[0] = x; o[1] = y; o[2] = z; }

}  // namespace
