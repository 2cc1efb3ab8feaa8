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
#include "errors.h"
#include "launchers.h"

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

// The LDS of one simulated step
struct BbShared {
  double dist[BB_MAX_OBS];
  int sel[BB_MAX_NEAR];
  double pos[2];
  int reached;
};

// One simulator step of a 256-thread work-group, shared by k_bb_step (one step per launch) and k_bb_episodes (a
// whole episode per work-group): reset != 0 writes observation row 0 (t = -1), otherwise step t.  raw(i) is
// component i of the actor's unclamped output (read by thread 0 only); lds_in, when not null, receives the
// next actor input as well.  sh.reached holds the goal test once the caller has passed a barrier.
// state: [0] agent x, [1] agent y, [2] goal x, [3] goal y, [4..8) level, ai, attempt, day,
//        [8 ..) ox[n_obs], oy[n_obs], oang[n_obs]
template <class Raw>
__device__ __forceinline__ void bb_step_body(const iqlhip_bb_sim &P, int reset, int t, Raw raw, BbShared &sh,
                                             float *lds_in) {
  double *s_dist = sh.dist;
  int *s_sel = sh.sel;
  const int tid = threadIdx.x, n_obs = P.n_obs, n_near = P.n_near, S = P.state_dim, A = P.action_dim;
  double *ox = P.state + 8, *oy = ox + n_obs, *oang = oy + n_obs;
  if (tid < BB_MAX_NEAR) s_sel[tid] = 0;
  if (tid == 0) {
    const double qx = ldg(P.state), qy = ldg(P.state + 1);
    double px = qx, py = qy;
    int reached = 0;
    if (!reset) {
      const float a0 = clamp_torch(raw(0), ldg(P.min_actions), ldg(P.max_actions));
      const float a1 = clamp_torch(raw(1), ldg(P.min_actions + 1), ldg(P.max_actions + 1));
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
    sh.pos[0] = px, sh.pos[1] = py;
    sh.reached = reached;
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
  const double px = sh.pos[0], py = sh.pos[1];
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
    const float in = (float)((v - ldg(P.state_mean + c)) / ldg(P.state_std + c));
    stg(P.actor_in + c, in);
    if (lds_in) lds_in[c] = in;
  }
  if (tid == 0) {
    stg(P.state, px);
    stg(P.state + 1, py);
    stg(P.ctl, t + 1);  // the episode's length once done is set
    stg(P.ctl + 1, sh.reached);
  }
}

__global__ __launch_bounds__(BB_THREADS) void k_bb_step(const iqlhip_bb_sim P, int reset) {
  __shared__ BbShared sh;
  const int t = reset ? -1 : ldg(P.ctl);
  if (!reset && (ldg(P.ctl + 1) != 0 || t < 0 || t >= P.max_horizon)) return;  // (uniform: nothing is written)
  const float *table = P.actor_out + (size_t)(reset ? 0 : t) * P.actor_out_stride;
  bb_step_body(P, reset, t, [table](int i) { return ldg(table + i); }, sh, nullptr);
}

static hipError_t launch_bb_step(const iqlhip_bb_sim &sim, int reset, hipStream_t st) {
  hipLaunchKernelGGL(k_bb_step, dim3(1), dim3(BB_THREADS), 0, st, sim, reset);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// A whole episode per work-group: k_bb_step(reset = 1), then up to max_horizon times { the actor's forward on
// the one-row input; the body of k_bb_step(reset = 0) }, without a launch in between.  n episodes (of n actors:
// the members of a seed group) are n work-groups of one launch; they share nothing and wait for nothing.
//
// The forward restates k_mlp_f32 (mlp_f32.hip) for one row, so that equal input rows give equal action bits on
// both paths.  What fixes the bits of an output element is the order of the operations on ITS accumulator:
//   hidden layer   acc = 0; for ks = 0 .. nk-1, c = 0 .. 3: one mfma_f32_16x16x4f32 over the k-group
//                  {16 ks + 4 q + c}; then + bias, then the activation;
//   last layer     (2 outputs: fewer than 4 n-tiles, the k-split path of k_mlp_f32) four partial accumulators
//                  over ks = w, w + 4, ... for w = 0 .. 3, summed as ((p0 + p1) + p2) + p3 -- exact zeros
//                  included when nk < 4 --, then + bias, then the output activation.
// Rows of an MFMA tile do not mix, so the one live row of a 16-row tile (the others stay zero) gets what row i
// of a 64-row work-group of k_mlp_f32 gets; n-tiles do not mix either, so wave w taking tiles w, w + 4, ... is
// a choice of speed only.  Zero K padding and zeroed padded output columns as there.  The B fragments come from
// the fragment-major image k_mlp_repack wrote once, ahead of the launch.
//
// LDS: BbShared (8.3 KB) + the activation image [16][260] fp32 (16.6 KB) + 72 floats.  The obstacles stay in
// global memory, advanced in place as k_bb_step does, so that both kernels run ONE step body.
constexpr int BB_LDA = 260;  // >= round_up(256, 16) + 4, the row stride k_mlp_f32 uses at width 256

struct BbEpisodeArgs {
  iqlhip_bb_sim sim;
  int32_t n_layers;  // 0: every step reads its row of the injected table, no forward
  int32_t dims[IQLHIP_MLP_MAX_LAYERS + 1];
  int32_t hidden_act, out_act;  // 0 relu / none, 1 tanh
  const float *Wf[IQLHIP_MLP_MAX_LAYERS];  // fragment-major images
  const float *b[IQLHIP_MLP_MAX_LAYERS];
};

__global__ __launch_bounds__(BB_THREADS) void k_bb_episodes(const BbEpisodeArgs *__restrict__ args) {
  using PF = Prec<false>;
  __shared__ BbShared sh;
  __shared__ __attribute__((aligned(16))) float s_act[16 * BB_LDA];
  __shared__ float s_red[4][16];
  __shared__ float s_out[2];
  const BbEpisodeArgs *E = args + blockIdx.x;
  const iqlhip_bb_sim P = E->sim;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int n_layers = E->n_layers, hidden_act = E->hidden_act, out_act = E->out_act;
  const int S = P.state_dim, K0p = round_up(S, 16);
  const float *so = s_out;
  auto raw = [so](int i) { return so[i]; };

  for (int e = tid; e < 16 * BB_LDA; e += BB_THREADS) s_act[e] = 0.f;  // rows 1 .. 15 stay zero for good
  if (tid < 2) s_out[tid] = 0.f;
  __syncthreads();
  bb_step_body(P, 1, -1, raw, sh, s_act);
  __syncthreads();

  for (int t = 0; t < P.max_horizon; ++t) {
    if (n_layers == 0) {
      if (tid < 2) s_out[tid] = ldg(P.actor_out + (size_t)t * P.actor_out_stride + tid);
      __syncthreads();
    }
    for (int l = 0; l < n_layers; ++l) {
      const int K = E->dims[l], N = E->dims[l + 1];
      const int nk = round_up(K, 16) / 16, ntile = round_up(N, 16) / 16;
      const float *Wf = E->Wf[l], *bias = E->b[l];
      if (l == n_layers - 1) {  // N = 2: the k-split output layer
        f32x4 pacc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = wave; ks < nk; ks += 4) {
          const uint4 a = *reinterpret_cast<const uint4 *>(s_act + r * BB_LDA + 16 * ks + 4 * q);
          const uint4 b = ldg16(Wf + frag_off<PF>(0, ks, nk, lane));
          PF::mma(a, b, pacc);
        }
        if (q == 0) s_red[wave][r] = pacc[0];  // row 0 of the tile
        __syncthreads();
        if (tid < N) {
          float sum = s_red[0][tid];
#pragma unroll
          for (int w = 1; w < 4; ++w) sum += s_red[w][tid];
          const float v = sum + ldg(bias + tid);
          const float o = out_act == 1 ? tanhf(v) : v;
          s_out[tid] = o;
          stg(P.actor_out + tid, o);  // (what the launch pair leaves there)
        }
        __syncthreads();
        continue;
      }
      int tile[4];
      bool live[4];
      f32x4 acc[4];
      float bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        live[j] = wave + 4 * j < ntile;
        tile[j] = live[j] ? wave + 4 * j : 0;
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        bv[j] = ldg(bias + (16 * tile[j] + r < N ? 16 * tile[j] + r : N - 1));
      }
      if (live[0]) {  // (wave-uniform)
        uint4 bq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[j] = ldg16(Wf + frag_off<PF>(tile[j], 0, nk, lane));
        for (int ks = 0; ks < nk; ++ks) {
          uint4 bn[4];  // the next k-step's fragments, in flight during this step's MFMAs
          const int kn = ks + 1 < nk ? ks + 1 : ks;
#pragma unroll
          for (int j = 0; j < 4; ++j) bn[j] = ldg16(Wf + frag_off<PF>(tile[j], kn, nk, lane));
          const f32x4 af =
              __builtin_bit_cast(f32x4, *reinterpret_cast<const uint4 *>(s_act + r * BB_LDA + 16 * ks + 4 * q));
          f32x4 bf[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) bf[j] = __builtin_bit_cast(f32x4, bq[j]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (live[j]) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[c], bf[j][c], acc[j], 0, 0, 0);
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) bq[j] = bn[j];
        }
      }
      __syncthreads();  // every wave has read its last A fragment: row 0 may be overwritten
      if (q == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!live[j]) continue;
          const int ncol = 16 * tile[j] + r;
          const float v = acc[j][0] + bv[j];
          s_act[ncol] = ncol < N ? (hidden_act == 0 ? fmaxf(v, 0.f) : tanhf(v)) : 0.f;  // zero K padding
        }
      }
      __syncthreads();
    }
    bb_step_body(P, 0, t, raw, sh, s_act);
    if (tid >= S && tid < K0p) s_act[tid] = 0.f;  // the input's K padding, overwritten by the hidden layers
    __syncthreads();
    if (sh.reached) break;  // (uniform; the next write of it lies behind a barrier of the next step)
  }
}

static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// scratch: the n argument blocks, then one weight image per actor that is not NULL, each on a 256-byte boundary
static size_t bb_episodes_scratch_bytes(const iqlhip_mlp_desc *const *actors, int n) {
  size_t total = up256((size_t)n * sizeof(BbEpisodeArgs));
  for (int k = 0; k < n; ++k)
    if (actors[k]) total += up256(mlp_image_offset(*actors[k], actors[k]->n_layers) * sizeof(float));
  return total;
}

static hipError_t launch_bb_episodes(const iqlhip_bb_sim *sims, const iqlhip_mlp_desc *const *actors, int n, void *scratch,
                                     hipStream_t st) {
  BbEpisodeArgs host[IQLHIP_MAX_GROUP];
  char *base = static_cast<char *>(scratch);
  size_t off = up256((size_t)n * sizeof(BbEpisodeArgs));
  for (int k = 0; k < n; ++k) {
    BbEpisodeArgs &a = host[k];
    a = BbEpisodeArgs{};
    a.sim = sims[k];
    const iqlhip_mlp_desc *d = actors[k];
    if (!d) continue;
    float *wf = reinterpret_cast<float *>(base + off);
    off += up256(mlp_image_offset(*d, d->n_layers) * sizeof(float));
    if (sims[k].actor_out_stride != 0) continue;  // the injected table stands in for this actor
    if (hipError_t e = launch_mlp_repack(*d, wf, st); e != hipSuccess) return e;
    a.n_layers = d->n_layers, a.hidden_act = d->hidden_act, a.out_act = d->out_act;
    for (int i = 0; i <= d->n_layers; ++i) a.dims[i] = d->dims[i];
    for (int i = 0; i < d->n_layers; ++i) a.Wf[i] = wf + mlp_image_offset(*d, i), a.b[i] = d->biases[i];
  }
  // (a pageable source: the copy has left `host` when the call returns)
  hipError_t e = hipMemcpyAsync(scratch, host, (size_t)n * sizeof(BbEpisodeArgs), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bb_episodes, dim3(n), dim3(BB_THREADS), 0, st, static_cast<const BbEpisodeArgs *>(scratch));
  return hipGetLastError();
}

}  // namespace iqlhip

using namespace iqlhip;

// ------------------------------------------------------------ entry points --
static int bb_sim_check(const iqlhip_bb_sim *s) {
  if (!s) return fail(IQLHIP_ERR_INVALID, "null simulator");
  if (!s->state || !s->drift || !s->ctl || !s->obs_hist || !s->act_hist || !s->record || !s->actor_in ||
      !s->actor_out || !s->state_mean || !s->state_std || !s->min_actions || !s->max_actions)
    return fail(IQLHIP_ERR_INVALID, "null pointer in the simulator");
  if (s->n_obs < 1 || s->n_obs > 1024) return fail(IQLHIP_ERR_UNSUPPORTED, "n_obs = %d outside 1..1024", s->n_obs);
  const int near_max = s->n_obs < 16 ? s->n_obs : 16;
  if (s->n_near < 1 || s->n_near > near_max)
    return fail(IQLHIP_ERR_UNSUPPORTED, "n_near = %d outside 1..%d", s->n_near, near_max);
  if (s->action_dim != 2)
    return fail(IQLHIP_ERR_UNSUPPORTED, "action_dim = %d: the simulator's action is (speed, heading)", s->action_dim);
  if (s->state_dim != 2 + 3 * s->n_near + 6)
    return fail(IQLHIP_ERR_INVALID, "state_dim = %d, an observation of %d obstacles has %d columns", s->state_dim,
                s->n_near, 2 + 3 * s->n_near + 6);
  if (s->max_horizon < 1) return fail(IQLHIP_ERR_INVALID, "max_horizon = %d must be >= 1", s->max_horizon);
  if (s->actor_out_stride != 0 && s->actor_out_stride < s->action_dim)
    return fail(IQLHIP_ERR_INVALID, "actor_out_stride = %d must be 0 or >= 2", s->actor_out_stride);
  return 0;
}

extern "C" int iqlhip_bb_sim_reset(const iqlhip_bb_sim *sim, void *stream) {
  if (int rc = bb_sim_check(sim)) return rc;
  HIP_TRY(launch_bb_step(*sim, 1, (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_bb_sim_step(const iqlhip_bb_sim *sim, void *stream) {
  if (int rc = bb_sim_check(sim)) return rc;
  HIP_TRY(launch_bb_step(*sim, 0, (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_bb_sim_rollout(const iqlhip_bb_sim *sim, const iqlhip_mlp_desc *actor, int32_t n_steps,
                                     void *stream) {
  if (int rc = bb_sim_check(sim)) return rc;
  if (!actor) return fail(IQLHIP_ERR_INVALID, "null actor");
  if (n_steps < 1) return fail(IQLHIP_ERR_INVALID, "n_steps = %d must be >= 1", n_steps);
  if (sim->actor_out_stride != 0)
    return fail(IQLHIP_ERR_INVALID, "a rollout reads the forward's live output row: actor_out_stride must be 0");
  if (actor->n_layers < 1 || actor->n_layers > IQLHIP_MLP_MAX_LAYERS)
    return fail(IQLHIP_ERR_INVALID, "n_layers must be in [1, %d]", IQLHIP_MLP_MAX_LAYERS);
  if (actor->dims[0] != sim->state_dim || actor->dims[actor->n_layers] != sim->action_dim)
    return fail(IQLHIP_ERR_INVALID, "the actor maps %d -> %d, the simulator needs %d -> %d", actor->dims[0],
                actor->dims[actor->n_layers], sim->state_dim, sim->action_dim);
  for (int i = 0; i < n_steps; ++i) {
    if (int rc = iqlhip_mlp_forward(actor, sim->actor_in, 1, sim->state_dim, sim->actor_out, sim->action_dim, stream))
      return rc;
    HIP_TRY(launch_bb_step(*sim, 0, (hipStream_t)stream));
  }
  return 0;
}

// The envelope of k_bb_episodes' fused forward: that of k_mlp_f32 (widths <= 256, relu / tanh hidden layers,
// no / tanh output, no dropout), two outputs
static int bb_actor_check(const iqlhip_mlp_desc *a, int k) {
  if (a->n_layers < 1 || a->n_layers > IQLHIP_MLP_MAX_LAYERS)
    return fail(IQLHIP_ERR_INVALID, "actor %d: n_layers must be in [1, %d]", k, IQLHIP_MLP_MAX_LAYERS);
  for (int i = 0; i <= a->n_layers; ++i) {
    if (a->dims[i] < 1) return fail(IQLHIP_ERR_INVALID, "actor %d: layer width %d", k, a->dims[i]);
    if (a->dims[i] > 256)
      return fail(IQLHIP_ERR_UNSUPPORTED, "actor %d: layer width %d > 256, the fused forward's limit (the launch "
                                          "pair of iqlhip_bb_sim_rollout takes wider actors)", k, a->dims[i]);
  }
  for (int i = 0; i < a->n_layers; ++i)
    if (!a->weights[i] || !a->biases[i]) return fail(IQLHIP_ERR_INVALID, "actor %d: null weight pointer", k);
  if (a->hidden_act < 0 || a->hidden_act > 1 || a->out_act < 0 || a->out_act > 1)
    return fail(IQLHIP_ERR_UNSUPPORTED, "actor %d: activations %d / %d, the fused forward has relu or tanh hidden "
                                        "layers and no or a tanh output", k, a->hidden_act, a->out_act);
  if (a->dropout_p > 0.f)
    return fail(IQLHIP_ERR_UNSUPPORTED, "actor %d: dropout_p > 0, the fused forward is an eval-mode forward", k);
  return 0;
}

extern "C" int iqlhip_bb_sim_episodes_scratch_bytes(const iqlhip_mlp_desc *const *actors, int32_t n, size_t *bytes) {
  if (!actors || !bytes) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n < 1 || n > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "n = %d: 1..%d episodes", n, IQLHIP_MAX_GROUP);
  for (int k = 0; k < n; ++k)
    if (actors[k])
      if (int rc = bb_actor_check(actors[k], k)) return rc;
  *bytes = bb_episodes_scratch_bytes(actors, n);
  return 0;
}

extern "C" int iqlhip_bb_sim_episodes(const iqlhip_bb_sim *sims, const iqlhip_mlp_desc *const *actors, int32_t n,
                                      void *scratch, size_t scratch_bytes, void *stream) {
  if (!sims) return fail(IQLHIP_ERR_INVALID, "null simulators");
  if (!actors) return fail(IQLHIP_ERR_INVALID, "null actors");
  if (!scratch) return fail(IQLHIP_ERR_INVALID, "null scratch");
  if (n < 1 || n > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "n = %d: 1..%d episodes", n, IQLHIP_MAX_GROUP);
  if ((uintptr_t)scratch & 15) return fail(IQLHIP_ERR_INVALID, "scratch must start on a 16-byte boundary");
  for (int k = 0; k < n; ++k) {
    if (int rc = bb_sim_check(sims + k)) return rc;
    const iqlhip_mlp_desc *a = actors[k];
    if (!a) {
      if (sims[k].actor_out_stride == 0)
        return fail(IQLHIP_ERR_INVALID, "episode %d: null actor and no injected table", k);
      continue;
    }
    if (int rc = bb_actor_check(a, k)) return rc;
    if (a->dims[0] != sims[k].state_dim || a->dims[a->n_layers] != sims[k].action_dim)
      return fail(IQLHIP_ERR_INVALID, "actor %d maps %d -> %d, the simulator needs %d -> %d", k, a->dims[0],
                  a->dims[a->n_layers], sims[k].state_dim, sims[k].action_dim);
  }
  const size_t need = bb_episodes_scratch_bytes(actors, n);
  if (scratch_bytes < need)
    return fail(IQLHIP_ERR_INVALID, "scratch of %zu bytes, %d episodes need %zu (iqlhip_bb_sim_episodes_scratch_bytes)",
                scratch_bytes, n, need);
  HIP_TRY(launch_bb_episodes(sims, actors, n, scratch, (hipStream_t)stream));
  return 0;
}
