// The evaluation simulator of algorithms/custom_offline/iql_bb.py:675-867 ("bref"), one step per launch:
// what iqlpref_amd/custom_offline_bb.py:bb_run_eval_IQL does between two actor.act calls, on the state of
// ONE episode that lives on the device.  The actor's forward (iqlhip_mlp_forward on the row k_bb_step
// leaves behind) and k_bb_step alternate on one stream; the host waits for nothing in between.
//   k_bb_step(reset = 1)  observation row 0 from the uploaded set-up, counter and done flag to 0;
//   k_bb_step(reset = 0)  clamp the actor's output, move the agent and the obstacles, test the goal,
//                         write observation row t + 1 and the next actor input.
// One work-group: an episode has 50 / 100 / 150 obstacles and a few hundred operations per step.
//
// Arithmetic.  The simulator is numpy, and every operation here is the one numpy performs, in its type:
//   * obstacles, goal test, distances, observation, normalisation: float64;
//   * the agent's move: FLOAT32.  actor.act returns a float32 array, and under numpy's scalar promotion
//     (NEP 50, numpy >= 2) `deg * (pi / 180)`, np.cos / np.sin, the product with the speed and the sum
//     `px + ...` with the Python float px all stay float32; `float(...)` then widens the rounded sum.  So
//     the agent's coordinates are float32 values from step 1 on, and the cosine is numpy's float32
//     cosine -- np_trig_f32 below restates that routine (numpy/_core/src/umath/loops_trigonometric:
//     Cody-Waite reduction by pi/2 in three fmas, two short polynomials, max 1.49 ulp) operation for
//     operation, because a correctly rounded cosine differs from it in 17 % of the arguments;
//   * no contraction of a * b + c into an fma anywhere numpy has none (the pragma below).
#include "../../include/iqlhip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace iqlhip {

constexpr int BB_THREADS = 256;
constexpr int BB_MAX_OBS = 1024;
constexpr int BB_MAX_NEAR = 16;

// numpy's float32 sin / cos for |x| <= 71476 (cos) / 117435 (sin), bit for bit; beyond that numpy calls the
// C library, and so does this (the simulator's angles are degrees in [-360, 360] times pi / 180).
__device__ __forceinline__ float np_trig_f32(float x, bool want_cos) {
  if (!(fabsf(x) <= 71476.0625f)) return want_cos ? cosf(x) : sinf(x);
  float q = x * 0x1.45f306p-1f;  // x * 2 / pi, rounded to the nearest integer by the magic constant
  q = q + 0x1.8p+23f;
  q = q - 0x1.8p+23f;
  float r = fmaf(q, -0x1.921fb0p+00f, x);
  r = fmaf(q, -0x1.5110b4p-22f, r);
  r = fmaf(q, -0x1.846988p-48f, r);
  const float r2 = r * r;
  float c = fmaf(0x1.98e616p-16f, r2, -0x1.6c06dcp-10f);
  c = fmaf(c, r2, 0x1.55553cp-05f);
  c = fmaf(c, r2, -0x1.000000p-01f);
  c = fmaf(c, r2, 1.0f);
  float s = fmaf(0x1.7d3bbcp-19f, r2, -0x1.a06bbap-13f);
  s = fmaf(s, r2, 0x1.11119ap-07f);
  s = fmaf(s, r2, -0x1.555556p-03f);
  s = fmaf(s, r2, 0.0f);
  s = fmaf(s, r, r);
  int iq = (int)q;
  if (want_cos) iq += 1;
  float v = (iq & 1) == 0 ? s : c;
  if ((iq & 2) == 2) v = 0.0f - v;
  return v;
}

// np.isclose(a, b) for a Python-scalar b: |a - b| <= atol + rtol |b| with the right side formed in double
// (and, for a float32 a, rounded to float32 for the comparison, as numpy's weak-scalar rule does).
__device__ __forceinline__ bool isclose_f64(double a, double b) { return fabs(a - b) <= 1e-8 + 1e-5 * fabs(b); }
__device__ __forceinline__ bool isclose_f32(float a, double b) {
  return fabsf(a - (float)b) <= (float)(1e-8 + 1e-5 * fabs(b));
}

constexpr double BB_RAD = 3.141592653589793 / 180.0;

// _cos_deg / _sin_deg of custom_offline_bb.py on a float64 array element ...
__device__ __forceinline__ double cos_deg_f64(double deg) {
  double c = cos(deg * BB_RAD);
  if (isclose_f64(deg, 90.0)) c = 0.0;
  if (isclose_f64(deg, 270.0)) c = 0.0;
  return c;
}
__device__ __forceinline__ double sin_deg_f64(double deg) {
  double s = sin(deg * BB_RAD);
  if (isclose_f64(deg, 360.0)) s = 0.0;
  if (isclose_f64(deg, 180.0)) s = 0.0;
  return s;
}
// ... and on a float32 scalar (the action's heading)
__device__ __forceinline__ float cos_deg_f32(float deg) {
  float c = np_trig_f32(deg * (float)BB_RAD, true);
  if (isclose_f32(deg, 90.0)) c = 0.f;
  if (isclose_f32(deg, 270.0)) c = 0.f;
  return c;
}
__device__ __forceinline__ float sin_deg_f32(float deg) {
  float s = np_trig_f32(deg * (float)BB_RAD, false);
  if (isclose_f32(deg, 360.0)) s = 0.f;
  if (isclose_f32(deg, 180.0)) s = 0.f;
  return s;
}

// torch.clamp(x, lo, hi) = min(max(x, lo), hi); a NaN stays a NaN
__device__ __forceinline__ float clamp_torch(float x, float lo, float hi) {
  if (x != x) return x;
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

// state: [0] agent x, [1] agent y, [2] goal x, [3] goal y, [4..8) level, ai, attempt, day,
//        [8 ..) ox[n_obs], oy[n_obs], oang[n_obs]
__global__ __launch_bounds__(BB_THREADS) void k_bb_step(const iqlhip_bb_sim P, int reset) {
  __shared__ double s_dist[BB_MAX_OBS];
  __shared__ int s_sel[BB_MAX_NEAR];
  __shared__ double s_pos[2];
  __shared__ int s_reached;
  const int tid = threadIdx.x, n_obs = P.n_obs, n_near = P.n_near, S = P.state_dim, A = P.action_dim;
  const int t = reset ? -1 : ldg(P.ctl);
  if (!reset && (ldg(P.ctl + 1) != 0 || t < 0 || t >= P.max_horizon)) return;  // (uniform: nothing is written)
  double *ox = P.state + 8, *oy = ox + n_obs, *oang = oy + n_obs;
  if (tid < BB_MAX_NEAR) s_sel[tid] = 0;
  if (tid == 0) {
    const double qx = ldg(P.state), qy = ldg(P.state + 1);
    double px = qx, py = qy;
    int reached = 0;
    if (!reset) {
      const float *raw = P.actor_out + (size_t)t * P.actor_out_stride;
      const float a0 = clamp_torch(ldg(raw), ldg(P.min_actions), ldg(P.max_actions));
      const float a1 = clamp_torch(ldg(raw + 1), ldg(P.min_actions + 1), ldg(P.max_actions + 1));
      stg(P.act_hist + (size_t)t * A, a0);
      stg(P.act_hist + (size_t)t * A + 1, a1);
      // float(px + action[0] * _cos_deg(action[1])): float32 throughout, px rounded to float32 first
      px = (double)((float)qx + a0 * cos_deg_f32(a1));
      py = (double)((float)qy + a0 * sin_deg_f32(a1));
      // _segment_hits_goal: the point of the segment q -> p closest to the goal
      const double gx = ldg(P.state + 2), gy = ldg(P.state + 3);
      const double vx = gx - qx, vy = gy - qy, dx = px - qx, dy = py - qy;
      double u = (vx * dx + vy * dy) / ((dx * dx) + (dy * dy));
      if (u != u) u = 0.0;
      if (u < 0) u = 0.0;
      if (u > 1) u = 1.0;
      const double cx = qx + dx * u, cy = qy + dy * u;
      const double d2 = ((cx - gx) * (cx - gx)) + ((cy - gy) * (cy - gy));
      const double reach = 0.3 + 1.0, lim = reach * reach;  // (AGENT_RADIUS + GOAL_RADIUS) ** 2
      reached = (d2 < lim) || isclose_f64(d2, lim);
    }
    s_pos[0] = px, s_pos[1] = py;
    s_reached = reached;
  }
  if (!reset) {  // the obstacles drift along their headings; one that leaves re-enters at its mirrored OLD place
    const double *drift = P.drift + (size_t)t * n_obs;
    for (int i = tid; i < n_obs; i += BB_THREADS) {
      const double x = ldg(ox + i), y = ldg(oy + i), ang = ldg(oang + i), d = ldg(drift + i);
      const double nx = x + (d * cos_deg_f64(ang)), ny = y + (d * sin_deg_f64(ang));
      const bool out = sqrt((nx * nx) + (ny * ny)) > 50.0;
      stg(ox + i, out ? -x : nx);
      stg(oy + i, out ? -y : ny);
    }
  }
  __syncthreads();
  const double px = s_pos[0], py = s_pos[1];
  for (int i = tid; i < n_obs; i += BB_THREADS) {  // (every thread reads back the entries it wrote itself)
    const double ex = ldg(ox + i) - px, ey = ldg(oy + i) - py;
    s_dist[i] = sqrt((ex * ex) + (ey * ey));
  }
  __syncthreads();
  // the n_near nearest in ascending distance: the rank of an entry is the number of entries before it in
  // the order (distance, index); ranks are distinct, so every slot below n_near has exactly one writer
  for (int i = tid; i < n_obs; i += BB_THREADS) {
    const double di = s_dist[i];
    int rank = 0;
    for (int j = 0; j < n_obs; ++j) {
      const double dj = s_dist[j];
      rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
    }
    if (rank < n_near && di == di) s_sel[rank] = i;
  }
  __syncthreads();
  if (tid < S) {
    double v;
    const int c = tid, k = (c - 2) / 3, j = (c - 2) - 3 * k;
    if (c < 2)
      v = c == 0 ? px : py;
    else if (c < 2 + 3 * n_near)
      v = ldg((j == 0 ? ox : j == 1 ? oy : oang) + s_sel[k]);
    else
      v = ldg(P.state + 2 + (c - 2 - 3 * n_near));  // goal x, y, level, ai, attempt, day
    const size_t row = (size_t)(t + 1) * S + c;
    stg(P.record + row, v);
    stg(P.obs_hist + row, (float)v);
    stg(P.actor_in + c, (float)((v - ldg(P.state_mean + c)) / ldg(P.state_std + c)));
  }
  if (tid == 0) {
    stg(P.state, px);
    stg(P.state + 1, py);
    stg(P.ctl, t + 1);  // the episode's length once done is set
    stg(P.ctl + 1, s_reached);
  }
}

hipError_t launch_bb_step(const iqlhip_bb_sim &sim, int reset, hipStream_t st) {
  hipLaunchKernelGGL(k_bb_step, dim3(1), dim3(BB_THREADS), 0, st, sim, reset);
  return hipGetLastError();
}

}  // namespace iqlhip
