// Offline TD3+BC (algorithms/offline/td3_bc.py, "tdbc"): an actor Linear(S,H) ReLU Linear(H,H) ReLU Linear(H,A) Tanh
// times max_action, two critics Linear(S+A,H) ReLU Linear(H,H) ReLU Linear(H,1) and a Polyak target of each of the
// three (tdbc:244-282), fp32 throughout (the reference has no autocast): exact fp32 MFMA.  The third family on the
// slab-step core (slab_step.h) after BC and AWAC, with AWAC's policies: FourChains, SumDouble, adam_apply_v64 (on the
// double beta2 and 1 - beta2: step_math.h has why).
// One TD3_BC.train (tdbc:324-380) is two launches, or five when the actor steps (total_it % policy_freq == 0):
//
//   k_td3_critic_fwd_bwd  one work-group of sixteen waves per 16-row slab and member: gathers the slab's rows, draws
//                         (or reads) eps: a' = clamp(actor_target(s') + clamp(eps policy_noise, +-noise_clip),
//                         +-max_action); both target critics at (s', a'): y = r + ((1 - d) discount) min; both
//                         critics at (s, a) with the activations in LDS, the two MSE heads (a sum, tdbc:352) and the
//                         backward down to dz1.  Leaves x, h1, h2, dz1..dz3 feature-major and the slab's two sums of
//                         squared errors.
//   k_td3_critic_update   one wave per 16x16 weight tile or 16 bias entries of both critics: Adam, the forward and
//                         transposed copies; on an actor step also the critics' targets (tdbc:376-377: nothing reads
//                         them before the next step, and the actor loss reads critic 1 itself); the logged critic loss.
//   k_td3_actor_fwd       per slab: the actor at s with h1, h2 kept as planes, pi = max_action tanh; the NEW critic 1
//                         at (s, pi) and its row-local backward down to dq/dpi; the slab's sums of q and |q| in double.
//   k_td3_actor_bwd       lmbda = alpha / mean|q| from the slab partials, summed in slab order by every work-group
//                         alike; the head (-(lmbda / B) dq/dpi + (2 / (B A)) (pi - a)) max_action (1 - tanh^2) and the
//                         actor's backward; the slab's sum of (pi - a)^2.
//   k_td3_actor_update    Adam on the actor's tiles, its copies, the actor's target (tdbc:378), the logged actor loss.
//
// The kernel boundaries are the two whole-batch dependencies: Adam needs the batch's gradient, lmbda the batch's
// mean|q| before the actor's backward can start.
//
// A batch of any size is padded to whole 16-row slabs: padding rows gather nothing, their head gradients are zero
// and the sums count the B real rows.  The members of a group are the y coordinate of every launch; EVERY
// hyperparameter is the member's own (TdMember), and whether a step is an actor step is decided per member on its own
// count: the three actor launches are issued when any member needs them, and a member that does not returns at its
// first instruction.  On such a step its actor, the actor's moments and all three targets keep their bits.
//
// eps: [n_steps][B][A] as given, or (null) standard normals by slab_normal on Philox stream STREAM_TD3 of the
// trainer's key at the zero-based total_it.  Either way the eps of the last step stay in the workspace.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"
#include "host_plan.h"
#include "slab_step.h"
#include "step_math.h"

namespace iqlhip {

constexpr uint32_t STREAM_TD3 = 7;  // (0-3 common.h, 4 online.hip, 5-6 awac_step.hip, 8.. drop_stream)
constexpr int TD_MAX_H = 256, TD_MAX_S = 128, TD_MAX_A = 32;
constexpr int TD_LS = TD_MAX_H + 4;             // floats; rows stay 16-byte aligned, 4 r mod 32 banks apart
constexpr int TD_XS = TD_MAX_S + TD_MAX_A + 4;  // of a [s | a] row
constexpr int TD_DS = TD_MAX_A + 4;             // of a head row
constexpr int TD_WAVES = 16, TD_THREADS = TD_WAVES * WAVE;
constexpr int TD_ACTOR = 0, TD_C1 = 1, TD_C2 = 2, TD_TA = 3, TD_T1 = 4, TD_T2 = 5, TD_NETS = 6;
constexpr int TD_COPIES = 6;  // per net: forward copies of the three layers, transposed copies of the three

// One network: Linear l has OUT_l x IN_l real entries, its forward copy is [OP_l][KP_l] and (trained nets: l >= 1;
// critic 1: l = 0 too, for dq/dpi) its transposed copy [KP_l][OP_l].  Element offsets: o_* in the parameter arena
// (targets: the same offsets of the target arena), everything else in the member's workspace.
struct TdNet {
  int o_w[3], o_b[3];
  int c_w[3], t_w[3];
  int pl_h[2], pl_dz[3];  // planes [H][BP] x 2; [H][BP] x 2 and [OP][BP]
  int K1, K1P, OUT, OP;
};

struct TdShape {
  int S, A, B, H;
  int SP, AP, BP, XP;  // padded to 16; XP: S + A
  int row_stride, next_off;
  int pl_x;                    // [XP][BP] (s | a), feature-major
  int o_eps;                   // [B][A]
  int o_pi, o_th, o_dq;        // [BP][AP] each: pi, tanh, dq/dpi of the actor step
  int o_cpart, o_qpart, o_apart;  // doubles [BP/16][2] (squared errors), [BP/16][2] (q, |q|), [BP/16] ((pi - a)^2)
  float two_over_B, fB, two_over_BA;
  TdNet net[TD_NETS];
};

__host__ __device__ inline bool td_has_tr(int n, int l) { return n <= TD_C2 && (l > 0 || n == TD_C1); }

struct TdMember {
  float *P, *M, *V, *G, *T;  // arenas (G may be null); T: the target arena, laid out as P
  float *ws;
  const float *rows;    // replay rows of this call
  const int64_t *idx;   // [n_steps][B] of this call
  const float *eps;     // [n_steps][B][A] of this call, or null
  float *loss;          // [n_steps][2] of this call, or null
  int64_t n_rows;
  uint64_t seed;
  int64_t step0;        // total_it of the call's first step (the noise stream)
  AdamCoef coef;        // of the step being launched: neg_step = critic 1, critic 2, actor; bc2_sqrt: the critics'
  float actor_bc2_sqrt; // the actor's, on its own step count
  double b2, one_m_b2;  // beta2 and 1 - beta2 as the optimisers hold them (adam_apply_v64)
  float discount, tau, one_m_tau, policy_noise, noise_clip, max_action, alpha;
  int actor_step;       // this step updates the actor and the targets
};

struct TdArgs {
  TdShape s;
  int64_t step;  // of this call
  TdMember m[IQLHIP_MAX_GROUP];
};
static_assert(sizeof(TdArgs) <= 4096, "the argument block travels by value");

// ---------------------------------------------------------------------------------------------------
// pieces of a slab's walk
// ---------------------------------------------------------------------------------------------------
// tdbc:259: max_action * tanh(z); the tanh correctly rounded
__device__ __forceinline__ float td_tanh(float z) { return (float)tanh((double)z); }

// tdbc:333-339: clamp(pi_target + clamp(eps * policy_noise, +-noise_clip), +-max_action), every step rounded
__device__ __forceinline__ float td_next_action(const TdMember &m, float pi_t, float eps) {
#pragma clang fp contract(off)
  const float noise = fminf(fmaxf(eps * m.policy_noise, -m.noise_clip), m.noise_clip);
  return fminf(fmaxf(pi_t + noise, -m.max_action), m.max_action);
}

// The head of the actor loss through max_action * tanh (tdbc:366-368): d pi = (-lmbda / B) dq/dpi + (2 / (B A))
// (pi - a); the scale's backward, then tanh's grad * (1 - t * t).  Not autograd's roundings throughout: autograd
// carries -lmbda / B as the upstream gradient through critic 1's backward, the kernel runs that backward from 1 and
// scales dq/dpi here -- the same number up to a rounding or two per entry, inside the envelope test's bound.
__device__ __forceinline__ float td_actor_head(float neg_lmbda_over_B, float two_over_BA, float max_action, float dq, float pi,
                                               float a, float th) {
#pragma clang fp contract(off)
  const float dpi = neg_lmbda_over_B * dq + two_over_BA * (pi - a);
  return (dpi * max_action) * (1.f - th * th);
}

// The walk's pieces are slab_step.h's at this family's sizes: two hidden layers, LDS rows of TD_LS / TD_XS / TD_DS.
// td_hidden: in [16][K1P] -> H0 -> H1, biases from `arena`; r0 >= 0: the activations are also kept as planes.
__device__ __forceinline__ void td_hidden(const TdShape &s, const TdMember &m, int n, const float *arena, const float *in,
                                          float *H0, float *H1, int r0, int wave, int lane) {
  const TdNet &N = s.net[n];
  float *const bufs[2] = {H0, H1};
  slab_hidden<2, TD_LS, TD_WAVES, FourChains>(in, TD_XS, m.ws, N.c_w, N.K1P, s.H, arena, N.o_b, bufs, r0 >= 0 ? m.ws : nullptr,
                                             N.pl_h, s.BP, r0, wave, lane);
}
__device__ __forceinline__ void td_q(const TdShape &s, const TdMember &m, int n, const float *arena, const float *h2, float *q,
                                     int wave, int lane) {
  slab_q<TD_LS, TD_WAVES, FourChains>(h2, m.ws + s.net[n].c_w[2], s.H, arena + s.net[n].o_b[2], q, wave, lane);
}
// the backward of trained network n from DZ3; dz1 replaces h1 in H0 when `keep1`; r0 >= 0: both go to their planes
__device__ __forceinline__ void td_backward(const TdShape &s, const TdMember &m, int n, const float *DZ3, float *H0, float *H1,
                                            bool keep1, int r0, int wave, int lane) {
  const TdNet &N = s.net[n];
  float *const bufs[2] = {H0, H1};
  slab_backward<2, TD_LS, TD_DS, TD_WAVES, FourChains>(DZ3, N.OP, m.ws, N.t_w + 1, s.H, bufs, keep1, r0 >= 0 ? m.ws : nullptr,
                                                      N.pl_dz, s.BP, r0, wave, lane);
}
__device__ __forceinline__ void td_gather(const TdShape &s, const TdMember &m, int64_t step, int r0, bool next, float *X,
                                          float *X2, float *rd, int64_t *ridx, int tid) {
  slab_gather<TD_XS, TD_THREADS>(s, m.idx, m.rows, m.n_rows, step, r0, next, X, X2, rd, ridx, tid);
}

// The last layer of an actor (n: TD_ACTOR from P, TD_TA from T) over the slab: t = tanh(h2 W3^T + b3), pi =
// max_action t.  ep(row, column, pi, t) for the A real columns.  Ends behind a barrier.
template <class Ep>
__device__ __forceinline__ void td_actor_head_fwd(const TdShape &s, const TdMember &m, int n, const float *arena, const float *h2,
                                                  int wave, int lane, Ep &&ep) {
  const TdNet &N = s.net[n];
  slab_layer<FourChains, TD_WAVES>(h2, TD_LS, m.ws + N.c_w[2], s.H, s.AP / 16, wave, lane, [&](int j, int row, f32x4 z) {
    if (j >= s.A) return;
    const float b = ldg(arena + N.o_b[2] + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float th = td_tanh(z[e] + b);
      ep(row + e, j, m.max_action * th, th);
    }
  });
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------
// launch 1: the critics' forward, heads and backward
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TD_THREADS) void k_td3_critic_fwd_bwd(const TdArgs args) {
  const TdShape &s = args.s;
  const TdMember &m = args.m[blockIdx.y];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * 16;
  __shared__ __attribute__((aligned(16))) float Xs[16 * TD_XS], Xn[16 * TD_XS];
  __shared__ __attribute__((aligned(16))) float H0[16 * TD_LS], H1[16 * TD_LS];
  __shared__ __attribute__((aligned(16))) float DZ3[16 * TD_DS], EPS[16 * TD_DS];
  __shared__ int64_t ridx[16];
  __shared__ float rd[32], qt[2][16];
  __shared__ double sq[16];

  td_gather(s, m, args.step, r0, true, Xs, Xn, rd, ridx, tid);
  for (int i = tid; i < 16 * s.XP; i += TD_THREADS) {  // x = (s | a), feature-major, for dW1 of all three nets
    const int c = i >> 4, r = i & 15;
    stg(m.ws + s.pl_x + (size_t)c * s.BP + r0 + r, Xs[r * TD_XS + c]);
  }
  for (int i = tid; i < 16 * TD_DS; i += TD_THREADS) DZ3[i] = 0.f;  // (a critic's head writes column 0 only)
  slab_noise<TD_DS, TD_THREADS>(m.eps ? m.eps + (size_t)args.step * s.B * s.A : nullptr, m.ws + s.o_eps, m.seed,
                                m.step0 + args.step, STREAM_TD3, s.B, s.A, EPS, r0, tid);

  // ---- a' from the actor's target at s' (tdbc:333-339) ----
  td_hidden(s, m, TD_TA, m.T, Xn, H0, H1, -1, wave, lane);
  td_actor_head_fwd(s, m, TD_TA, m.T, H1, wave, lane, [&](int r, int j, float pi, float) {
    if (r0 + r < s.B) Xn[r * TD_XS + s.S + j] = td_next_action(m, pi, EPS[r * TD_DS + j]);
  });

  // ---- min of both target critics at (s', a') (tdbc:342-344) ----
  for (int t = 0; t < 2; ++t) {
    td_hidden(s, m, TD_T1 + t, m.T, Xn, H0, H1, -1, wave, lane);
    td_q(s, m, TD_T1 + t, m.T, H1, qt[t], wave, lane);
  }

  // ---- both critics at (s, a), the MSE heads (tdbc:348-352), the backward ----
  for (int c = 0; c < 2; ++c) {
    const int n = TD_C1 + c;
    const TdNet &N = s.net[n];
    td_hidden(s, m, n, m.P, Xs, H0, H1, r0, wave, lane);
    slab_layer<FourChains, TD_WAVES>(H1, TD_LS, m.ws + N.c_w[2], s.H, 1, wave, lane, [&](int f, int row, f32x4 z) {
      const float b = f == 0 ? ldg(m.P + N.o_b[2]) : 0.f;
      f32x4 dz = {};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = row + e;
        if (f == 0 && r0 + r < s.B) {
          const float qn = fminf(qt[0][r], qt[1][r]);
          const float diff = (z[e] + b) - slab_td_target(rd[r], rd[16 + r], m.discount, qn);
          dz[e] = s.two_over_B * diff;  // mse_loss backward: (2 / B) (q - y)
          // (the logged loss from the same fp32 values without the roundings of q + b, y and q - y)
          const double dd = ((double)z[e] + (double)b) -
                            ((double)rd[r] + ((double)m.discount * (1.0 - (double)rd[16 + r])) * (double)qn);
          sq[r] = dd * dd;
        } else if (f == 0) {
          sq[r] = 0.0;
        }
        if (f == 0) DZ3[r * TD_DS] = dz[e];
      }
      slab_plane4(m.ws + N.pl_dz[2], s.BP, f, r0 + row, dz);
    });
    __syncthreads();
    if (tid == 0) {  // in double and in one fixed order: the logged loss is the correctly rounded mean
      double t = 0.0;
      for (int i = 0; i < 16; ++i) t += sq[i];
      stg(reinterpret_cast<double *>(m.ws + s.o_cpart) + 2 * blockIdx.x + c, t);
    }
    td_backward(s, m, n, DZ3, H0, H1, false, r0, wave, lane);
  }
}

// ---------------------------------------------------------------------------------------------------
// launch 3: the actor's forward, q = Q1(s, pi) at the new critic 1 and dq/dpi
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TD_THREADS) void k_td3_actor_fwd(const TdArgs args) {
  const TdMember &m = args.m[blockIdx.y];
  if (!m.actor_step) return;
  const TdShape &s = args.s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * 16;
  __shared__ __attribute__((aligned(16))) float Xp[16 * TD_XS];
  __shared__ __attribute__((aligned(16))) float H0[16 * TD_LS], H1[16 * TD_LS];
  __shared__ __attribute__((aligned(16))) float DZ3[16 * TD_DS];
  __shared__ int64_t ridx[16];
  __shared__ float q[16];

  td_gather(s, m, args.step, r0, false, nullptr, Xp, nullptr, ridx, tid);  // (s | 0): pi goes behind the state columns
  for (int i = tid; i < 16 * TD_DS; i += TD_THREADS) DZ3[i] = (i % TD_DS) == 0 ? 1.f : 0.f;  // dq/dq of every row

  // ---- pi = actor(s), h1 and h2 kept as planes (tdbc:364) ----
  td_hidden(s, m, TD_ACTOR, m.P, Xp, H0, H1, r0, wave, lane);
  td_actor_head_fwd(s, m, TD_ACTOR, m.P, H1, wave, lane, [&](int r, int j, float pi, float th) {
    const size_t o = (size_t)(r0 + r) * s.AP + j;
    stg(m.ws + s.o_pi + o, pi), stg(m.ws + s.o_th + o, th);
    if (r0 + r < s.B) Xp[r * TD_XS + s.S + j] = pi;
  });

  // ---- q = Q1(s, pi) at the critic 1 just updated (tdbc:365); the slab's sums of q and |q| ----
  td_hidden(s, m, TD_C1, m.P, Xp, H0, H1, -1, wave, lane);
  td_q(s, m, TD_C1, m.P, H1, q, wave, lane);
  if (tid == 0) {
    double sum = 0.0, sabs = 0.0;
    for (int r = 0; r < 16 && r0 + r < s.B; ++r) sum += (double)q[r], sabs += fabs((double)q[r]);
    double *part = reinterpret_cast<double *>(m.ws + s.o_qpart) + 2 * blockIdx.x;
    stg(part, sum), stg(part + 1, sabs);
  }

  // ---- dq/dpi: the row-local backward of critic 1 down to its input's action columns ----
  td_backward(s, m, TD_C1, DZ3, H0, H1, true, -1, wave, lane);
  const TdNet &N = s.net[TD_C1];
  const int t0 = s.S / 16, t1 = (s.S + s.A - 1) / 16;  // the 16-column tiles of x that hold action columns
  slab_layer<FourChains, TD_WAVES>(H0, TD_LS, m.ws + N.t_w[0] + (size_t)t0 * 16 * s.H, s.H, t1 - t0 + 1, wave, lane,
                                   [&](int f, int row, f32x4 g) {
                                     const int j = f + 16 * t0 - s.S;
                                     if (j < 0 || j >= s.A) return;
#pragma unroll
                                     for (int e = 0; e < 4; ++e) stg(m.ws + s.o_dq + (size_t)(r0 + row + e) * s.AP + j, g[e]);
                                   });
}

// ---------------------------------------------------------------------------------------------------
// launch 4: lmbda, the actor's head and backward
// ---------------------------------------------------------------------------------------------------
// lmbda = alpha / mean|q| (tdbc:366) and mean q from the slab partials, in slab order.
__device__ __forceinline__ void td_lmbda(const TdShape &s, const TdMember &m, float &lmbda, double &qmean) {
  const double *part = reinterpret_cast<const double *>(m.ws + s.o_qpart);
  double sum = 0.0, sabs = 0.0;
  for (int i = 0; i < s.BP / 16; ++i) sum += ldg(part + 2 * i), sabs += ldg(part + 2 * i + 1);
  lmbda = m.alpha / (float)(sabs / (double)s.B);
  qmean = sum / (double)s.B;
}

__global__ __launch_bounds__(TD_THREADS) void k_td3_actor_bwd(const TdArgs args) {
  const TdMember &m = args.m[blockIdx.y];
  if (!m.actor_step) return;
  const TdShape &s = args.s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * 16;
  __shared__ __attribute__((aligned(16))) float H0[16 * TD_LS], H1[16 * TD_LS];
  __shared__ __attribute__((aligned(16))) float DZ3[16 * TD_DS];
  __shared__ int64_t ridx[16];
  __shared__ float lm;
  __shared__ double bc[16 * TD_DS];
  const TdNet &N = s.net[TD_ACTOR];

  slab_row_indices(m.idx, args.step, s.B, r0, m.n_rows, ridx, tid);
  if (tid == TD_THREADS - 1) {
    double qmean;
    float lmbda;
    td_lmbda(s, m, lmbda, qmean);
    lm = lmbda;
  }
  for (int i = tid; i < 16 * s.H; i += TD_THREADS) {  // h1, h2 of the slab back from their planes
    const int f = i >> 4, r = i & 15;
    H0[r * TD_LS + f] = ldg(m.ws + N.pl_h[0] + (size_t)f * s.BP + r0 + r);
    H1[r * TD_LS + f] = ldg(m.ws + N.pl_h[1] + (size_t)f * s.BP + r0 + r);
  }
  for (int i = tid; i < 16 * TD_DS; i += TD_THREADS) DZ3[i] = 0.f;
  __syncthreads();

  for (int i = tid; i < 16 * s.AP; i += TD_THREADS) {  // one thread per (row, column) of the head
    const int j = i >> 4, r = i & 15;
    const int64_t row = ridx[r];
    float dz = 0.f;
    double d2 = 0.0;
    if (row >= 0 && j < s.A) {
      const size_t o = (size_t)(r0 + r) * s.AP + j;
      const float pi = ldg(m.ws + s.o_pi + o), a = ldg(m.rows + row * s.row_stride + s.S + j);
      dz = td_actor_head(-lm / s.fB, s.two_over_BA, m.max_action, ldg(m.ws + s.o_dq + o), pi, a, ldg(m.ws + s.o_th + o));
      const double d = (double)pi - (double)a;
      d2 = d * d;
    }
    DZ3[r * TD_DS + j] = dz, bc[r * TD_DS + j] = d2;
    stg(m.ws + N.pl_dz[2] + (size_t)j * s.BP + r0 + r, dz);
  }
  __syncthreads();
  if (tid == 0) {  // in double and in one fixed order
    double t = 0.0;
    for (int r = 0; r < 16; ++r)
      for (int j = 0; j < s.A; ++j) t += bc[r * TD_DS + j];
    stg(reinterpret_cast<double *>(m.ws + s.o_apart) + blockIdx.x, t);
  }
  td_backward(s, m, TD_ACTOR, DZ3, H0, H1, false, r0, wave, lane);
}

// ---------------------------------------------------------------------------------------------------
// launches 2 and 5: dW per tile, Adam, the refreshed copies, the targets, the logged losses
// ---------------------------------------------------------------------------------------------------
// Wave w of trained net n's update (w < slab_net_waves<3>): a weight tile or 16 bias entries of Linear l, and the same
// entries of its target: on an actor step (1 - tau) t + tau p into the target arena, else the target as it stands;
// either way into the target's forward copy.
__device__ __forceinline__ void td_update_wave(const TdShape &s, const TdMember &m, int n, int w, const AdamCoef &coef,
                                               float neg_step, int lane) {
  const TdNet &N = s.net[n], &TN = s.net[n + (TD_TA - TD_ACTOR)];
  const auto adam = [&](float &p, float &mm, float &vv, float g) { adam_apply_v64(p, mm, vv, g, coef, neg_step, m.b2, m.one_m_b2); };
  const auto tile = [&](int l, bool bias) {
    return SlabTile{m.P, m.M, m.V, m.G, (size_t)(bias ? N.o_b[l] : N.o_w[l]), slab_out<3>(s, n, l), slab_in(s, n, l),
                    slab_op<3>(s, n, l), slab_kp(s, n, l), s.BP, m.ws + N.pl_dz[l], m.ws + (l == 0 ? s.pl_x : N.pl_h[l - 1]),
                    m.ws + N.c_w[l], td_has_tr(n, l) ? m.ws + N.t_w[l] : nullptr, m.ws + TN.c_w[l]};
  };
  const auto target = [&](int l, bool bias) {  // of that tensor of the target arena (laid out as P)
    const int off = bias ? N.o_b[l] : N.o_w[l];
    return [&m, off](size_t rel, float p) {
      const float t = ldg(m.T + off + rel);
      if (!m.actor_step) return t;
      const float tv = slab_polyak(m.one_m_tau, m.tau, t, p);
      stg(m.T + off + rel, tv);
      return tv;
    };
  };
  slab_update_wave<3, FourChains, SumDouble>(s, n, w, lane, tile, adam, target);
}

__global__ __launch_bounds__(256) void k_td3_critic_update(const TdArgs args) {
  const TdShape &s = args.s;
  const TdMember &m = args.m[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int per = slab_net_waves<3>(s, TD_C1);
  if (w > 2 * per) return;
  if (w < 2 * per) {
    const int c = w >= per ? 1 : 0;
    return td_update_wave(s, m, TD_C1 + c, w - c * per, m.coef, m.coef.neg_step[c], lane);
  }
  if (lane == 0 && m.loss) {  // tdbc:352: mse + mse; the actor's column is 0 unless k_td3_actor_update writes it
    const double *cp = reinterpret_cast<const double *>(m.ws + s.o_cpart);
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < s.BP / 16; ++i) s1 += ldg(cp + 2 * i), s2 += ldg(cp + 2 * i + 1);
    stg(m.loss + 2 * args.step, (float)(s1 / (double)s.B) + (float)(s2 / (double)s.B));
    stg(m.loss + 2 * args.step + 1, 0.f);
  }
}

__global__ __launch_bounds__(256) void k_td3_actor_update(const TdArgs args) {
  const TdMember &m = args.m[blockIdx.y];
  if (!m.actor_step) return;
  const TdShape &s = args.s;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int per = slab_net_waves<3>(s, TD_ACTOR);
  if (w > per) return;
  if (w < per) {
    AdamCoef coef = m.coef;
    coef.bc2_sqrt = m.actor_bc2_sqrt;
    return td_update_wave(s, m, TD_ACTOR, w, coef, m.coef.neg_step[2], lane);
  }
  if (lane == 0 && m.loss) {  // tdbc:368: -lmbda * mean(q) + mse(pi, a), its own arithmetic in double
    const double *ap = reinterpret_cast<const double *>(m.ws + s.o_apart);
    float lmbda;
    double qmean, sa = 0.0;
    td_lmbda(s, m, lmbda, qmean);
    for (int i = 0; i < s.BP / 16; ++i) sa += ldg(ap + i);
    stg(m.loss + 2 * args.step + 1, (float)(-(double)lmbda * qmean + sa / ((double)s.B * (double)s.A)));
  }
}

// The copies from the fp32 masters (creation, load_state_dict): blockIdx.y = net * 6 + copy, one thread per
// element of the padded copy.
__global__ void k_td3_sync(const TdShape s, const float *P, const float *T, float *ws) {
  const int n = blockIdx.y / TD_COPIES, kind = blockIdx.y % TD_COPIES;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const TdNet &N = s.net[n];
  const float *src = n >= TD_TA ? T : P;
  const bool tr = kind >= 3;
  const int l = tr ? kind - 3 : kind;
  if (tr && !td_has_tr(n, l)) return;
  const int OUT = slab_out<3>(s, n, l), IN = slab_in(s, n, l), OP = slab_op<3>(s, n, l), KP = slab_kp(s, n, l);
  if (i >= OP * KP) return;
  slab_padded_copy(ws + (tr ? N.t_w[l] : N.c_w[l]), src + N.o_w[l], OUT, IN, OP, KP, tr, i);
}

}  // namespace iqlhip

using namespace iqlhip;

// ---------------------------------------------------------------------------------------------------
// entry points (include/iqlhip.h)
// ---------------------------------------------------------------------------------------------------
struct iqlhip_td3bc : SlabTrainer {
  static constexpr int QUEUE_STEPS = 512;  // at most ~2 x 512 steps are ever queued ahead of the device
  TdShape s{};
  float *T = nullptr;        // the target arena
  double lr[3] = {0, 0, 0};  // critic 1, critic 2, actor
  uint64_t seed = 0;
  int64_t actor_it = 0;      // the actor optimiser's own step count
  int64_t policy_freq = 2;
  float discount = 0, tau = 0, one_m_tau = 0, policy_noise = 0, noise_clip = 0, max_action = 0, alpha = 0;
  iqlhip_td3bc() : SlabTrainer(QUEUE_STEPS) {}
  float *ws() const { return static_cast<float *>(mem); }
};

struct iqlhip_td3bc_group : SlabGroup<iqlhip_td3bc> {};

// The envelope, checked before any HIP call.
static int td3bc_check(const iqlhip_trainer_config *c) {
  if (!c) return fail(IQLHIP_ERR_INVALID, "null config");
  if (c->precision != IQLHIP_PREC_FP32)
    return fail(IQLHIP_ERR_UNSUPPORTED, "TD3+BC runs at precision fp32 only (the reference has no autocast)");
  if (c->n_hidden != 2) return fail(IQLHIP_ERR_UNSUPPORTED, "TD3+BC trains networks of two hidden layers (n_hidden %d)", c->n_hidden);
  if (c->hidden_dim < 16 || c->hidden_dim > TD_MAX_H || c->hidden_dim % 16)
    return fail(IQLHIP_ERR_UNSUPPORTED, "hidden_dim %d is not a multiple of 16 in 16..%d", c->hidden_dim, TD_MAX_H);
  if (c->state_dim < 1 || c->action_dim < 1 || c->batch_size < 1)
    return fail(IQLHIP_ERR_INVALID, "state_dim, action_dim and batch_size must be positive");
  if (c->state_dim > TD_MAX_S || c->action_dim > TD_MAX_A)
    return fail(IQLHIP_ERR_UNSUPPORTED, "state_dim %d > %d or action_dim %d > %d", c->state_dim, TD_MAX_S, c->action_dim,
                TD_MAX_A);
  // (the workspace is addressed with 32-bit element offsets: ~15 planes of hidden_dim x batch_size floats)
  if ((int64_t)c->batch_size > (1 << 16)) return fail(IQLHIP_ERR_UNSUPPORTED, "batch_size %d > 2^16", c->batch_size);
  if (c->dropout_p > 0.f) return fail(IQLHIP_ERR_UNSUPPORTED, "the TD3+BC networks have no dropout");
  return 0;
}

// Arena offsets: every tensor starts on a 128-byte line.  The target arena has the parameter arena's layout.
static TdShape td3bc_arena_shape(const iqlhip_trainer_config *c, int64_t *n_params) {
  TdShape s{};
  s.S = c->state_dim, s.A = c->action_dim, s.B = c->batch_size, s.H = c->hidden_dim;
  s.SP = round_up(s.S, 16), s.AP = round_up(s.A, 16), s.BP = round_up(s.B, 16), s.XP = round_up(s.S + s.A, 16);
  s.row_stride = iqlhip_replay_row_stride(s.S, s.A), s.next_off = iqlhip_replay_next_offset(s.S, s.A);
  for (int n = 0; n < TD_NETS; ++n) {
    TdNet &N = s.net[n];
    const bool actor = n % 3 == TD_ACTOR;
    N.K1 = actor ? s.S : s.S + s.A, N.K1P = actor ? s.SP : s.XP, N.OUT = actor ? s.A : 1, N.OP = actor ? s.AP : 16;
  }
  int64_t off = 0;
  const auto take = [&](int64_t n) {
    const int64_t o = off;
    off += (n + 31) / 32 * 32;
    return (int)o;
  };
  for (int n = TD_ACTOR; n <= TD_C2; ++n)
    for (int l = 0; l < 3; ++l) {
      s.net[n].o_w[l] = s.net[n + 3].o_w[l] = take((int64_t)slab_out<3>(s, n, l) * slab_in(s, n, l));
      s.net[n].o_b[l] = s.net[n + 3].o_b[l] = take(slab_out<3>(s, n, l));
    }
  if (n_params) *n_params = off;
  return s;
}

// The workspace of one trainer (element offsets, floats).  Everything is zero at creation; padding is only
// ever rewritten with zeros.
static size_t td3bc_plan(TdShape &s) {
  size_t off = 0;
  const auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 63) / 64 * 64;  // 256-byte blocks
    return (int)o;
  };
  for (int n = 0; n < TD_NETS; ++n) {
    TdNet &N = s.net[n];
    for (int l = 0; l < 3; ++l) N.c_w[l] = take((size_t)slab_op<3>(s, n, l) * slab_kp(s, n, l));
    if (n >= TD_TA) continue;
    for (int l = 0; l < 3; ++l)
      if (td_has_tr(n, l)) N.t_w[l] = take((size_t)slab_kp(s, n, l) * slab_op<3>(s, n, l));
    for (int l = 0; l < 2; ++l) N.pl_h[l] = take((size_t)s.H * s.BP);
    for (int l = 0; l < 3; ++l) N.pl_dz[l] = take((size_t)slab_op<3>(s, n, l) * s.BP);
  }
  s.pl_x = take((size_t)s.XP * s.BP);
  s.o_eps = take((size_t)s.B * s.A);
  s.o_pi = take((size_t)s.BP * s.AP), s.o_th = take((size_t)s.BP * s.AP), s.o_dq = take((size_t)s.BP * s.AP);
  s.o_cpart = take((size_t)4 * (s.BP / 16));  // doubles [BP / 16][2]
  s.o_qpart = take((size_t)4 * (s.BP / 16));  // doubles [BP / 16][2]
  s.o_apart = take((size_t)2 * (s.BP / 16));  // doubles [BP / 16]
  return off * sizeof(float);
}

extern "C" int iqlhip_td3bc_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[18], int64_t *n_params) {
  if (!offsets || !n_params) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = td3bc_check(cfg)) return rc;
  const TdShape s = td3bc_arena_shape(cfg, n_params);
  int i = 0;
  for (int n = TD_ACTOR; n <= TD_C2; ++n)
    for (int l = 0; l < 3; ++l) offsets[i++] = s.net[n].o_w[l], offsets[i++] = s.net[n].o_b[l];
  return 0;
}

static int td3bc_sync(iqlhip_td3bc *t, hipStream_t st) {
  const int n = TD_MAX_H * (t->s.XP > t->s.H ? t->s.XP : t->s.H);
  hipLaunchKernelGGL(k_td3_sync, dim3((n + 255) / 256, TD_NETS * TD_COPIES), dim3(256), 0, st, t->s, (const float *)t->P,
                     (const float *)t->T, t->ws());
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_td3bc_destroy(iqlhip_td3bc *t) { return slab_destroy(t); }

extern "C" int iqlhip_td3bc_create(iqlhip_td3bc **out, const iqlhip_trainer_config *cfg, double tau, float policy_noise,
                                   float noise_clip, float max_action, float alpha, int64_t policy_freq,
                                   const iqlhip_arenas *arenas) {
  if (!out || !arenas) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = td3bc_check(cfg)) return rc;
  if (!arenas->params || !arenas->exp_avg || !arenas->exp_avg_sq || !arenas->target) return fail(IQLHIP_ERR_INVALID, "null arena");
  if (!(max_action > 0.f) || !(policy_noise >= 0.f) || !(noise_clip >= 0.f))
    return fail(IQLHIP_ERR_INVALID, "max_action must be positive, policy_noise and noise_clip not negative");
  if (policy_freq < 1) return fail(IQLHIP_ERR_UNSUPPORTED, "policy_freq %lld < 1", (long long)policy_freq);
  if (!(tau >= 0.0 && tau <= 1.0)) return fail(IQLHIP_ERR_INVALID, "tau must lie in [0, 1]");
  iqlhip_td3bc *t = new (std::nothrow) iqlhip_td3bc;
  if (!t) return fail(IQLHIP_ERR_NOMEM, "out of host memory");
  t->s = td3bc_arena_shape(cfg, nullptr);
  TdShape &s = t->s;
  s.two_over_B = (float)(2.0 / (double)s.B), s.fB = (float)s.B, s.two_over_BA = (float)(2.0 / ((double)s.B * (double)s.A));
  // tdbc:79: the Python doubles tau and 1 - tau, each rounded to fp32 once (cfg->tau is already fp32: 1 - it is another number)
  t->discount = cfg->discount, t->tau = (float)tau, t->one_m_tau = (float)(1.0 - tau);
  t->policy_noise = policy_noise, t->noise_clip = noise_clip, t->max_action = max_action, t->alpha = alpha;
  t->policy_freq = policy_freq;
  t->P = arenas->params, t->M = arenas->exp_avg, t->V = arenas->exp_avg_sq, t->G = arenas->grads, t->T = arenas->target;
  t->lr[0] = cfg->lr_q, t->lr[1] = cfg->lr_v, t->lr[2] = cfg->lr_actor;
  t->beta1 = cfg->adam_beta1, t->beta2 = cfg->adam_beta2, t->eps = cfg->adam_eps, t->seed = cfg->seed;
  t->bytes = td3bc_plan(s);
  return slab_finish_create(out, t, [](iqlhip_td3bc *t) { return td3bc_sync(t, nullptr); });
}

extern "C" int iqlhip_td3bc_sync_weights(iqlhip_td3bc *t, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  return td3bc_sync(t, (hipStream_t)stream);
}

extern "C" int iqlhip_td3bc_set_step(iqlhip_td3bc *t, int64_t total_it, int64_t actor_it) {
  if (actor_it < 0) return fail(IQLHIP_ERR_INVALID, "negative actor step");
  if (int rc = slab_set_step(t, total_it)) return rc;
  t->actor_it = actor_it;
  return 0;
}

extern "C" int iqlhip_td3bc_set_lr(iqlhip_td3bc *t, double lr_actor, double lr_critic_1, double lr_critic_2) {
  if (!t || !(lr_actor >= 0) || !(lr_critic_1 >= 0) || !(lr_critic_2 >= 0))
    return fail(IQLHIP_ERR_INVALID, "null trainer or negative lr");
  t->lr[0] = lr_critic_1, t->lr[1] = lr_critic_2, t->lr[2] = lr_actor;
  return 0;
}

extern "C" int iqlhip_td3bc_copy_out(iqlhip_td3bc *t, int32_t which, float *dst, void *stream) {
  if (!t || !dst) return fail(IQLHIP_ERR_INVALID, "null argument");
  const TdShape &s = t->s;
  const float *src = nullptr;
  size_t n = 0;
  if (which == 0) {
    src = t->ws() + s.o_eps, n = (size_t)s.B * s.A;
  } else if (which >= 1 && which <= TD_NETS * TD_COPIES) {
    const int net = (which - 1) / TD_COPIES, kind = (which - 1) % TD_COPIES, l = kind % 3;
    if (kind >= 3 && !td_has_tr(net, l)) return fail(IQLHIP_ERR_INVALID, "net %d has no transposed copy of Linear %d", net, l + 1);
    src = t->ws() + (kind >= 3 ? s.net[net].t_w[l] : s.net[net].c_w[l]);
    n = (size_t)slab_op<3>(s, net, l) * slab_kp(s, net, l);
  } else {
    return fail(IQLHIP_ERR_INVALID, "which must be in 0..%d", TD_NETS * TD_COPIES);
  }
  HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// n_steps steps of the members m[0..n): two launches per step for all of them, five when any member's actor steps.
static int td3bc_run(iqlhip_td3bc *const *mem, int n, SlabQueueBound &bound, const iqlhip_replay_view *views, int64_t n_steps,
                     const int64_t *const *idx, const float *const *eps, float *const *losses, hipStream_t st) {
  if (int rc = slab_check_call(mem, n, views, idx, n_steps, "TD3+BC")) return rc;
  TdArgs a{};
  a.s = mem[0]->s;
  int64_t actor_it[IQLHIP_MAX_GROUP];
  for (int k = 0; k < n; ++k) {
    const iqlhip_td3bc *t = mem[k];
    TdMember &m = a.m[k];
    m.P = t->P, m.M = t->M, m.V = t->V, m.G = t->G, m.T = t->T, m.ws = t->ws();
    m.rows = views[k].rows, m.n_rows = views[k].n_rows, m.idx = idx[k], m.eps = eps ? eps[k] : nullptr;
    m.loss = losses ? losses[k] : nullptr, m.seed = t->seed, m.step0 = t->total_it;
    m.discount = t->discount, m.tau = t->tau, m.one_m_tau = t->one_m_tau, m.policy_noise = t->policy_noise;
    m.noise_clip = t->noise_clip, m.max_action = t->max_action, m.alpha = t->alpha;
    m.b2 = t->beta2, m.one_m_b2 = 1.0 - t->beta2;
    actor_it[k] = t->actor_it;
  }
  const int slabs = a.s.BP / 16;
  const dim3 g1(slabs, n), g2((2 * slab_net_waves<3>(a.s, TD_C1) + 1 + 3) / 4, n), g5((slab_net_waves<3>(a.s, TD_ACTOR) + 1 + 3) / 4, n);
  const int rc = slab_run(mem, n, bound, n_steps, st, [&](int64_t i) {
    bool any = false;
    for (int k = 0; k < n; ++k) {
      const iqlhip_td3bc *t = mem[k];
      TdMember &m = a.m[k];
      const int64_t it = t->total_it + i + 1;  // tdbc:326: one-based
      m.coef = make_adam_coef(t->beta1, t->beta2, t->eps, t->lr[0], t->lr[1], 0.0, 1, it);
      m.actor_step = it % t->policy_freq == 0;
      if (m.actor_step) {
        const AdamCoef ca = make_adam_coef(t->beta1, t->beta2, t->eps, t->lr[2], 0.0, 0.0, 1, ++actor_it[k]);
        m.coef.neg_step[2] = ca.neg_step[0], m.actor_bc2_sqrt = ca.bc2_sqrt;
        any = true;
      }
    }
    a.step = i;
    hipLaunchKernelGGL(k_td3_critic_fwd_bwd, g1, dim3(TD_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_td3_critic_update, g2, dim3(256), 0, st, a);
    if (!any) return;
    hipLaunchKernelGGL(k_td3_actor_fwd, g1, dim3(TD_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_td3_actor_bwd, g1, dim3(TD_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_td3_actor_update, g5, dim3(256), 0, st, a);
  });
  if (rc) return rc;
  for (int k = 0; k < n; ++k) mem[k]->actor_it = actor_it[k];
  return 0;
}

extern "C" int iqlhip_td3bc_group_create(iqlhip_td3bc_group **out, iqlhip_td3bc *const *members, int32_t n) {
  return slab_group_create(
      out, members, n, [](const TdShape &a, const TdShape &b) { return a.S == b.S && a.A == b.A && a.B == b.B && a.H == b.H; },
      "dims, width and batch size");
}

extern "C" int iqlhip_td3bc_group_destroy(iqlhip_td3bc_group *g) { return slab_group_destroy(g); }

extern "C" int iqlhip_td3bc_group_train_steps(iqlhip_td3bc_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                              const int64_t *const *idx, const float *const *eps, float *const *losses_out,
                                              void *stream) {
  if (!g) return fail(IQLHIP_ERR_INVALID, "null group");
  return td3bc_run(g->member, g->n, g->bound, views, n_steps, idx, eps, losses_out, (hipStream_t)stream);
}

extern "C" int iqlhip_td3bc_train_steps(iqlhip_td3bc *t, const iqlhip_replay_view *view, int64_t n_steps, const int64_t *idx,
                                        const float *eps, float *losses_out, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  return td3bc_run(&t, 1, t->bound, view, n_steps, &idx, eps ? &eps : nullptr, losses_out ? &losses_out : nullptr,
                   (hipStream_t)stream);
}
