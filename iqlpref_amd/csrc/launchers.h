// The few host functions that one .hip file defines and another calls, outside the two training steps (those are
// in iql_step.h and iql_deep.h).  Included by the file that defines each and by the files that call it, so a
// definition is checked against the one declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/iqlhip.h"

namespace iqlhip {

// mlp_f32.hip.  Callers: iqlhip_explore_action (api.hip: the actor on its fp32 masters), k_bb_episodes' weight
// images (bb_sim.hip).  d has passed the checks of iqlhip_mlp_forward.
hipError_t launch_mlp_f32(const iqlhip_mlp_desc &d, const float *x, int64_t n, int x_stride, float *out,
                          int out_stride, hipStream_t st);
size_t mlp_image_offset(const iqlhip_mlp_desc &d, int l);
hipError_t launch_mlp_repack(const iqlhip_mlp_desc &d, float *wf, hipStream_t st);

// online.hip.  Callers: iqlhip_explore_action, iqlhip_explore_action_group (api.hip, which builds the actors'
// descriptors from the trainers' arenas).
hipError_t launch_explore_epilogue(float *act, int64_t rows, int A, const float *log_std, const float *eps,
                                   float expl_noise, float noise_clip, float max_action, uint64_t seed, uint32_t call,
                                   hipStream_t st);
hipError_t launch_explore_group(const iqlhip_mlp_desc *actors, const float *const *log_std, int K, const float *s,
                                int s_stride, const float *eps, float expl_noise, float noise_clip, float max_action,
                                float *out, hipStream_t st);

}  // namespace iqlhip
