// Offline AWAC (algorithms/offline/awac.py, "awac"): the training step of an actor and two critics with two
// Polyak targets, every network Linear(in, H) ReLU Linear(H, H) ReLU Linear(H, H) ReLU Linear(H, out)
// (awac:134-210), fp32 throughout (the reference has no autocast): exact fp32 MFMA (v_mfma_f32_16x16x4_f32).
// One update (awac:301-310) is four launches -- an Adam step needs the whole batch's gradient, and the actor
// loss reads the critics that the step has just updated:
//
//   k_awac_critic_fwd_bwd  one work-group of sixteen waves per 16-row slab and member: gathers the slab's rows,
//                          runs the actor at s' and draws (or reads) eps_1: a' = clamp(mu + sigma eps_1, -1, 1);
//                          both target critics at (s', a'): y = r + gamma (1 - d) min; both critics at (s, a)
//                          with the activations held in LDS, the two MSE heads (awac:280-282: a sum, not a
//                          half-sum) and the backward down to dz1.  Leaves x, h1..h3, dz1..dz4 feature-major
//                          ([feature][batch row]) and the slab's two sums of squared errors.
//   k_awac_critic_update   one wave per 16x16 tile of a weight matrix (dW = dz^T x activation, the batch as the
//                          K dimension) or per 16 bias entries of both critics: Adam on the fp32 masters, the
//                          padded forward copy and the transposed copy, and the target update (awac:213-215:
//                          two rounded products and a sum) with the targets' forward copy.  Nothing reads the
//                          targets before the next step and the critics do not change again within the step.
//   k_awac_actor_fwd_bwd   per slab and member: the actor at s with the activations kept, eps_2:
//                          pi = clamp(mu + sigma eps_2, -1, 1); the new critics at (s, pi) and (s, a):
//                          w = min(exp((q - v) / lambda), exp_adv_max); the head of
//                          mean(-w sum_A log N(a; mu, sigma)) (d mu, per-slab d sigma sums) and the backward.
//   k_awac_actor_update    Adam on the actor's tiles and on _log_std (exp and clamp backward: the clamp passes
//                          the gradient inside [-20, 2] only), and both logged losses, summed in slab order.
//
// A batch of any size is padded to whole 16-row slabs: padding rows gather nothing, their head gradients are
// zero and so is everything behind them; the means divide by the B real rows.  The members of a group are the
// y coordinate of every launch; a member's arguments are its own entry of the by-value argument block and its
// arithmetic does not depend on who else is launched with it.
//
// eps: [n_steps][2][B][A] as given, or (null) standard normals from the trainer's Philox key by Box-Muller as
// online.hip draws them: block (row * 8 + column / 4, step lo, step hi, STREAM_AWAC_NEXT | STREAM_AWAC_PI), words
// (x, y) and (z, w) each one pair, evaluated in double.  Either way the eps of the last step stay in the
// workspace (iqlhip_awac_copy_out).
//
// The slab walk, the tile updates and the host side are slab_step.h's, with this family's policies: four MFMA
// chains per tile added pairwise (FourChains), the bias gradient summed in double (SumDouble), step_math.h's adam_apply_v64.
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

constexpr uint32_t STREAM_AWAC_NEXT = 5, STREAM_AWAC_PI = 6;  // (0-3 common.h, 4 online.hip, 8.. drop_stream)
constexpr int AW_MAX_H = 256, AW_MAX_S = 128, AW_MAX_A = 32;
constexpr int AW_LS = AW_MAX_H + 4;             // floats; rows stay 16-byte aligned, 4 r mod 32 banks apart
constexpr int AW_XS = AW_MAX_S + AW_MAX_A + 4;  // of a [s | a] row
constexpr int AW_DS = AW_MAX_A + 4;             // of a head-gradient row
constexpr int AW_WAVES = 16, AW_THREADS = AW_WAVES * WAVE;
constexpr int AW_ACTOR = 0, AW_C1 = 1, AW_C2 = 2, AW_T1 = 3, AW_T2 = 4, AW_NETS = 5;
constexpr int AW_COPIES = 7;  // per net: forward copies of the four layers, transposed copies of layers 2..4

// One network: Linear l has OUT_l x IN_l real entries, its forward copy is [OP_l][KP_l] and (trained nets,
// l >= 1) its transposed copy [KP_l][OP_l]; OP_l = KP_(l+1).  Element offsets: o_* in the parameter arena
// (targets: the target arena), everything else in the member's workspace.
struct AwNet {
  int o_w[4], o_b[4];
  int c_w[4], t_w[3];
  int pl_h[3], pl_dz[4];  // planes [H][BP] x 3; [H][BP] x 3 and [OP][BP]
  int K1, K1P, OUT, OP;
};

struct AwShape {
  int S, A, B, H;
  int SP, AP, BP, XP;  // padded to 16; XP: S + A
  int row_stride, next_off;
  int o_log_std;
  int pl_x;                      // [XP][BP] (s | a), feature-major
  int o_eps;                     // [2][B][A]
  int o_qpart, o_apart, o_lsp;   // doubles [BP/16][2], [BP/16]; floats [BP/16][AP]
  float gamma, tau, one_m_tau, lambda, exp_adv_max, two_over_B, fB;
  AwNet net[AW_NETS];
};

struct AwMember {
  float *P, *M, *V, *G, *T;  // arenas (G may be null)
  float *ws;
  const float *rows;    // replay rows of this call
  const int64_t *idx;   // [n_steps][B] of this call
  const float *eps;     // [n_steps][2][B][A] of this call, or null
  float *loss;          // [n_steps][2] of this call, or null
  int64_t n_rows;
  uint64_t seed;
  int64_t step0;        // total_it of the call's first step (the noise streams)
  AdamCoef coef;        // of the step being launched: neg_step = critic 1, critic 2, actor
};

struct AwArgs {
  AwShape s;
  int64_t step;  // of this call
  AwMember m[IQLHIP_MAX_GROUP];
};
static_assert(sizeof(AwArgs) <= 4096, "the argument block travels by value");

// ---------------------------------------------------------------------------------------------------
// pieces of a slab's walk
// ---------------------------------------------------------------------------------------------------
// A Linear layer of the slab is slab_layer<FourChains, AW_WAVES>: its n_tiles tiles of 16 features go round the
// sixteen waves (hidden layers: H / 16 of them; a critic's head: one; the actor's head: AP / 16).

// exp(clamp(_log_std, -20, 2)) (awac:163-164), correctly rounded
__device__ __forceinline__ float aw_std(float ls) { return (float)exp((double)fminf(fmaxf(ls, -20.f), 2.f)); }

// awac:174-175: rsample = mean + eps * std (a product and a sum, each rounded), clamped to [-1, 1]
__device__ __forceinline__ float aw_sample(float mean, float sd, float eps) {
#pragma clang fp contract(off)
  return fminf(fmaxf(mean + eps * sd, -1.f), 1.f);
}

// The walk's pieces are slab_step.h's at this family's sizes: three hidden layers, LDS rows of AW_LS / AW_XS / AW_DS.
// aw_hidden: a network without kept activations, in -> Ha -> Hb -> Ha.
__device__ __forceinline__ void aw_hidden(const AwShape &s, const AwMember &m, int n, const float *arena, const float *in,
                                          float *Ha, float *Hb, int wave, int lane) {
  const AwNet &N = s.net[n];
  float *const bufs[3] = {Ha, Hb, Ha};
  slab_hidden<3, AW_LS, AW_WAVES, FourChains>(in, AW_XS, m.ws, N.c_w, N.K1P, s.H, arena, N.o_b, bufs, nullptr, N.pl_h, s.BP, 0,
                                             wave, lane);
}
__device__ __forceinline__ void aw_q(const AwShape &s, const AwMember &m, int n, const float *arena, const float *h3,
                                     float *q, int wave, int lane) {
  slab_q<AW_LS, AW_WAVES, FourChains>(h3, m.ws + s.net[n].c_w[3], s.H, arena + s.net[n].o_b[3], q, wave, lane);
}
// a trained network with the activations kept in H0, H1, H2 and as planes; the caller runs the last layer
__device__ __forceinline__ void aw_hidden_kept(const AwShape &s, const AwMember &m, int n, const float *in, int in_stride,
                                               float *H0, float *H1, float *H2, int r0, int wave, int lane) {
  const AwNet &N = s.net[n];
  float *const bufs[3] = {H0, H1, H2};
  slab_hidden<3, AW_LS, AW_WAVES, FourChains>(in, in_stride, m.ws, N.c_w, N.K1P, s.H, m.P, N.o_b, bufs, m.ws, N.pl_h, s.BP, r0,
                                             wave, lane);
}
// its backward from the head gradient DZ4 (its plane already written): dz1 goes to its plane only
__device__ __forceinline__ void aw_backward(const AwShape &s, const AwMember &m, int n, const float *DZ4, float *H0,
                                            float *H1, float *H2, int r0, int wave, int lane) {
  const AwNet &N = s.net[n];
  float *const bufs[3] = {H0, H1, H2};
  slab_backward<3, AW_LS, AW_DS, AW_WAVES, FourChains>(DZ4, N.OP, m.ws, N.t_w, s.H, bufs, false, m.ws, N.pl_dz, s.BP, r0, wave,
                                                      lane);
}
__device__ __forceinline__ void aw_gather(const AwShape &s, const AwMember &m, int64_t step, int r0, bool next, float *X,
                                          float *X2, float *rd, int64_t *ridx, int tid) {
  slab_gather<AW_XS, AW_THREADS>(s, m.idx, m.rows, m.n_rows, step, r0, next, X, X2, rd, ridx, tid);
}
// draw `which` (0: a', 1: pi) of the step
__device__ __forceinline__ void aw_noise(const AwShape &s, const AwMember &m, int64_t step, int which, float *EPS, int r0,
                                         int tid) {
  const size_t draw = (size_t)s.B * s.A;
  slab_noise<AW_DS, AW_THREADS>(m.eps ? m.eps + (size_t)(step * 2 + which) * draw : nullptr, m.ws + s.o_eps + which * draw,
                                m.seed, m.step0 + step, which ? STREAM_AWAC_PI : STREAM_AWAC_NEXT, s.B, s.A, EPS, r0, tid);
}

// The last layer of the actor over the slab: mu = H2 W4^T + b4 (kept in MU, or not: null) and the clamped sample
// written behind the state columns of X2 (the critics' input).  MUD: mu without the rounding of the bias add, for
// the logged loss.  Ends behind a barrier.
__device__ __forceinline__ void aw_actor_sample(const AwShape &s, const AwMember &m, const float *H2, float *X2, float *MU,
                                                double *MUD, const float *EPS, int r0, int wave, int lane) {
  const AwNet &N = s.net[AW_ACTOR];
  slab_layer<FourChains, AW_WAVES>(H2, AW_LS, m.ws + N.c_w[3], s.H, s.AP / 16, wave, lane, [&](int j, int row, f32x4 z) {
    if (j >= s.A) return;
    const float b = ldg(m.P + N.o_b[3] + j);
    const float sd = aw_std(ldg(m.P + s.o_log_std + j));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mu = z[e] + b;
      if (MU) MU[(row + e) * AW_DS + j] = mu, MUD[(row + e) * AW_DS + j] = (double)z[e] + (double)b;
      if (r0 + row + e < s.B) X2[(row + e) * AW_XS + s.S + j] = aw_sample(mu, sd, EPS[(row + e) * AW_DS + j]);
    }
  });
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------
// launch 1: the critics' forward, heads and backward
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AW_THREADS) void k_awac_critic_fwd_bwd(const AwArgs args) {
  const AwShape &s = args.s;
  const AwMember &m = args.m[blockIdx.y];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * 16;
  __shared__ __attribute__((aligned(16))) float Xs[16 * AW_XS], Xn[16 * AW_XS];
  __shared__ __attribute__((aligned(16))) float H0[16 * AW_LS], H1[16 * AW_LS], H2[16 * AW_LS];
  __shared__ __attribute__((aligned(16))) float DZ4[16 * AW_DS], EPS[16 * AW_DS];
  __shared__ int64_t ridx[16];
  __shared__ float rd[32], qt[2][16];
  __shared__ double sq[16];

  aw_gather(s, m, args.step, r0, true, Xs, Xn, rd, ridx, tid);
  for (int i = tid; i < 16 * s.XP; i += AW_THREADS) {  // x = (s | a), feature-major, for dW1 of all three nets
    const int c = i >> 4, r = i & 15;
    stg(m.ws + s.pl_x + (size_t)c * s.BP + r0 + r, Xs[r * AW_XS + c]);
  }
  for (int i = tid; i < 16 * AW_DS; i += AW_THREADS) DZ4[i] = 0.f;  // (a critic's head writes column 0 only)

  // ---- a' = clamp(mu(s') + sigma eps_1, -1, 1) from the actor as it stands (awac:268-269) ----
  aw_noise(s, m, args.step, 0, EPS, r0, tid);
  aw_hidden(s, m, AW_ACTOR, m.P, Xn, H0, H1, wave, lane);
  aw_actor_sample(s, m, H0, Xn, nullptr, nullptr, EPS, r0, wave, lane);

  // ---- q_next = min of both targets at (s', a') (awac:271-274) ----
  for (int t = 0; t < 2; ++t) {
    aw_hidden(s, m, AW_T1 + t, m.T, Xn, H0, H1, wave, lane);
    aw_q(s, m, AW_T1 + t, m.T, H0, qt[t], wave, lane);
  }

  // ---- both critics at (s, a), the MSE heads (awac:277-282), the backward ----
  for (int c = 0; c < 2; ++c) {
    const int n = AW_C1 + c;
    const AwNet &N = s.net[n];
    aw_hidden_kept(s, m, n, Xs, AW_XS, H0, H1, H2, r0, wave, lane);
    slab_layer<FourChains, AW_WAVES>(H2, AW_LS, m.ws + N.c_w[3], s.H, 1, wave, lane, [&](int f, int row, f32x4 z) {
      const float b = f == 0 ? ldg(m.P + N.o_b[3]) : 0.f;
      f32x4 dz = {};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = row + e;
        if (f == 0 && r0 + r < s.B) {
          const float qn = fminf(qt[0][r], qt[1][r]);
          const float diff = (z[e] + b) - slab_td_target(rd[r], rd[16 + r], s.gamma, qn);
          dz[e] = s.two_over_B * diff;  // mse_loss backward: (2 / B) (q - y)
          // (the logged loss from the same fp32 values without the roundings of q + b, y and q - y)
          const double dd = ((double)z[e] + (double)b) -
                            ((double)rd[r] + ((double)s.gamma * (1.0 - (double)rd[16 + r])) * (double)qn);
          sq[r] = dd * dd;
        } else if (f == 0) {
          sq[r] = 0.0;
        }
        if (f == 0) DZ4[r * AW_DS] = dz[e];
      }
      slab_plane4(m.ws + N.pl_dz[3], s.BP, f, r0 + row, dz);
    });
    __syncthreads();
    if (tid == 0) {  // in double and in one fixed order: the logged loss is the correctly rounded mean
      double t = 0.0;
      for (int i = 0; i < 16; ++i) t += sq[i];
      stg(reinterpret_cast<double *>(m.ws + s.o_qpart) + 2 * blockIdx.x + c, t);
    }
    aw_backward(s, m, n, DZ4, H0, H1, H2, r0, wave, lane);
  }
}

// ---------------------------------------------------------------------------------------------------
// launch 3: the actor's forward, head and backward
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AW_THREADS) void k_awac_actor_fwd_bwd(const AwArgs args) {
  const AwShape &s = args.s;
  const AwMember &m = args.m[blockIdx.y];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * 16;
  __shared__ __attribute__((aligned(16))) float Xs[16 * AW_XS], Xp[16 * AW_XS];
  __shared__ __attribute__((aligned(16))) float H0[16 * AW_LS], H1[16 * AW_LS], H2[16 * AW_LS];
  __shared__ __attribute__((aligned(16))) float E0[16 * AW_LS], E1[16 * AW_LS];
  __shared__ __attribute__((aligned(16))) float DZ4[16 * AW_DS], MU[16 * AW_DS], GS[16 * AW_DS], EPS[16 * AW_DS];
  __shared__ int64_t ridx[16];
  __shared__ float qv[4][16], SD[AW_MAX_A];
  __shared__ double LSD[AW_MAX_A], SDD[AW_MAX_A], MUD[16 * AW_DS];
  __shared__ double nll[16];
  const AwNet &N = s.net[AW_ACTOR];

  aw_gather(s, m, args.step, r0, false, Xs, Xp, nullptr, ridx, tid);
  for (int i = tid; i < 16 * AW_DS; i += AW_THREADS) DZ4[i] = 0.f, MU[i] = 0.f;
  if (tid < s.A) {  // sigma_j and log sigma_j, once per slab (Normal.log_prob takes the log of the scale)
    SD[tid] = aw_std(ldg(m.P + s.o_log_std + tid));
    LSD[tid] = (double)fminf(fmaxf(ldg(m.P + s.o_log_std + tid), -20.f), 2.f);
    SDD[tid] = exp(LSD[tid]);
  }

  // ---- the actor at s, activations kept; pi = clamp(mu + sigma eps_2, -1, 1) (awac:250) ----
  aw_noise(s, m, args.step, 1, EPS, r0, tid);
  aw_hidden_kept(s, m, AW_ACTOR, Xp, AW_XS, H0, H1, H2, r0, wave, lane);
  aw_actor_sample(s, m, H2, Xp, MU, MUD, EPS, r0, wave, lane);

  // ---- v = min Q_i(s, pi), q = min Q_i(s, a) at the critics just updated (awac:251-257) ----
  for (int c = 0; c < 4; ++c) {
    aw_hidden(s, m, AW_C1 + (c & 1), m.P, c < 2 ? Xp : Xs, E0, E1, wave, lane);
    aw_q(s, m, AW_C1 + (c & 1), m.P, E0, qv[c], wave, lane);
  }

  // ---- w = min(exp((q - v) / lambda), exp_adv_max) (awac:258-261); the head of mean(-w log_prob) ----
  if (tid < 16) {
    const int r = tid;
    const bool real = r0 + r < s.B;
    const float qmin = fminf(qv[2][r], qv[3][r]), vmin = fminf(qv[0][r], qv[1][r]);
    const float w = real ? fminf((float)exp((double)((qmin - vmin) / s.lambda)), s.exp_adv_max) : 0.f;
    const float gbc = w / s.fB;
    // (the logged loss from the same fp32 values, its own arithmetic in double: log sigma is the clamped _log_std)
    const double wd = fmin(exp(((double)qmin - (double)vmin) / (double)s.lambda), (double)s.exp_adv_max);
    double lp = 0.0;  // -log_prob of the row: Normal.log_prob term by term, summed over the actions
    for (int j = 0; j < s.A; ++j) {
      const float sd = SD[j], var = sd * sd;
      const float zg = Xs[r * AW_XS + s.S + j] - MU[r * AW_DS + j];
      const double zd = (double)Xs[r * AW_XS + s.S + j] - MUD[r * AW_DS + j], sdd = SDD[j];
      lp += (zd * zd) / (2.0 * sdd * sdd) + LSD[j] + 0.91893853320467274178;
      const float dmu = real ? -gbc * (zg / var) : 0.f;
      DZ4[r * AW_DS + j] = dmu;
      GS[r * AW_DS + j] = real ? gbc * (-(zg * zg) / (var * sd) + 1.f / sd) : 0.f;
      stg(m.ws + N.pl_dz[3] + (size_t)j * s.BP + r0 + r, dmu);
    }
    for (int j = s.A; j < s.AP; ++j) stg(m.ws + N.pl_dz[3] + (size_t)j * s.BP + r0 + r, 0.f);
    nll[r] = real ? wd * lp : 0.0;
  }
  __syncthreads();
  if (tid < s.AP) {  // the slab's d loss / d sigma_j, rows in order
    float g = 0.f;
    if (tid < s.A)
      for (int r = 0; r < 16; ++r) g += GS[r * AW_DS + tid];
    stg(m.ws + s.o_lsp + (size_t)blockIdx.x * s.AP + tid, g);
  }
  if (tid == 64) {
    double t = 0.0;
    for (int i = 0; i < 16; ++i) t += nll[i];
    stg(reinterpret_cast<double *>(m.ws + s.o_apart) + blockIdx.x, t);
  }
  aw_backward(s, m, AW_ACTOR, DZ4, H0, H1, H2, r0, wave, lane);
}

// ---------------------------------------------------------------------------------------------------
// launches 2 and 4: dW per tile, Adam, the refreshed copies, the targets, the logged losses
// ---------------------------------------------------------------------------------------------------
// Wave w of net n's update (w < slab_net_waves<4>): a weight tile or 16 bias entries of Linear l.  TARGET: the target
// net of critic n follows it -- (1 - tau) t + tau p into the target arena and into the target's forward copy.
template <bool TARGET>
__device__ __forceinline__ void aw_update_wave(const AwShape &s, const AwMember &m, int n, int w, float neg_step, int lane) {
  const AwNet &N = s.net[n], &TN = s.net[TARGET ? n + (AW_T1 - AW_C1) : n];
  const auto adam = [&](float &p, float &mm, float &vv, float g) { adam_apply_v64(p, mm, vv, g, m.coef, neg_step); };
  const auto tile = [&](int l, bool bias) {
    return SlabTile{m.P, m.M, m.V, m.G, (size_t)(bias ? N.o_b[l] : N.o_w[l]), slab_out<4>(s, n, l), slab_in(s, n, l),
                    slab_op<4>(s, n, l), slab_kp(s, n, l), s.BP, m.ws + N.pl_dz[l], m.ws + (l == 0 ? s.pl_x : N.pl_h[l - 1]),
                    m.ws + N.c_w[l], l > 0 ? m.ws + N.t_w[l - 1] : nullptr, TARGET ? m.ws + TN.c_w[l] : nullptr};
  };
  const auto target = [&](int l, bool bias) {  // of that tensor of the target arena
    if constexpr (TARGET) {
      const int off = bias ? TN.o_b[l] : TN.o_w[l];
      return [&m, &s, off](size_t rel, float p) {
        const float tv = slab_polyak(s.one_m_tau, s.tau, ldg(m.T + off + rel), p);
        stg(m.T + off + rel, tv);
        return tv;
      };
    } else {
      return SlabNoTarget{};
    }
  };
  slab_update_wave<4, FourChains, SumDouble>(s, n, w, lane, tile, adam, target);
}

__global__ __launch_bounds__(256) void k_awac_critic_update(const AwArgs args) {
  const AwShape &s = args.s;
  const AwMember &m = args.m[blockIdx.y];
  const int lane = threadIdx.x & 63;
  int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int per = slab_net_waves<4>(s, AW_C1);
  if (w >= 2 * per) return;
  const int c = w >= per ? 1 : 0;
  aw_update_wave<true>(s, m, AW_C1 + c, w - c * per, m.coef.neg_step[c], lane);
}

__global__ __launch_bounds__(256) void k_awac_actor_update(const AwArgs args) {
  const AwShape &s = args.s;
  const AwMember &m = args.m[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int per = slab_net_waves<4>(s, AW_ACTOR);
  if (w > per) return;
  if (w < per) return aw_update_wave<false>(s, m, AW_ACTOR, w, m.coef.neg_step[2], lane);
  const int ns = s.BP / 16;
  if (lane < s.A) {  // _log_std: sigma = exp(clamp(ls, -20, 2)); the slab sums in slab order
    double gs = 0.0;
    for (int i = 0; i < ns; ++i) gs += (double)ldg(m.ws + s.o_lsp + (size_t)i * s.AP + lane);
    const size_t o = (size_t)s.o_log_std + lane;
    float p = ldg(m.P + o), mm = ldg(m.M + o), vv = ldg(m.V + o);
    const float g = (p >= -20.f && p <= 2.f) ? (float)gs * aw_std(p) : 0.f;
    adam_apply_v64(p, mm, vv, g, m.coef, m.coef.neg_step[2]);
    stg(m.P + o, p), stg(m.M + o, mm), stg(m.V + o, vv);
    if (m.G) stg(m.G + o, g);
  }
  if (lane == 63 && m.loss) {  // awac:282, 264: mse + mse; the mean of -w log_prob
    const double *qp = reinterpret_cast<const double *>(m.ws + s.o_qpart);
    const double *apart = reinterpret_cast<const double *>(m.ws + s.o_apart);
    double s1 = 0.0, s2 = 0.0, sa = 0.0;
    for (int i = 0; i < ns; ++i) s1 += ldg(qp + 2 * i), s2 += ldg(qp + 2 * i + 1), sa += ldg(apart + i);
    stg(m.loss + 2 * args.step, (float)(s1 / (double)s.B) + (float)(s2 / (double)s.B));
    stg(m.loss + 2 * args.step + 1, (float)(sa / (double)s.B));
  }
}

// The copies from the fp32 masters (creation, load_state_dict): blockIdx.y = net * 7 + copy, one thread per
// element of the padded copy.
__global__ void k_awac_sync(const AwShape s, const float *P, const float *T, float *ws) {
  const int n = blockIdx.y / AW_COPIES, kind = blockIdx.y % AW_COPIES;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const AwNet &N = s.net[n];
  const float *src = n >= AW_T1 ? T : P;
  const bool tr = kind >= 4;
  if (tr && n >= AW_T1) return;
  const int l = tr ? kind - 3 : kind;
  const int OUT = slab_out<4>(s, n, l), IN = slab_in(s, n, l), OP = slab_op<4>(s, n, l), KP = slab_kp(s, n, l);
  if (i >= OP * KP) return;
  slab_padded_copy(ws + (tr ? N.t_w[l - 1] : N.c_w[l]), src + N.o_w[l], OUT, IN, OP, KP, tr, i);
}

}  // namespace iqlhip

using namespace iqlhip;

// ---------------------------------------------------------------------------------------------------
// entry points (include/iqlhip.h)
// ---------------------------------------------------------------------------------------------------
struct iqlhip_awac : SlabTrainer {
  static constexpr int QUEUE_STEPS = 512;  // at most ~2 x 512 steps are ever queued ahead of the device
  AwShape s{};
  float *T = nullptr;        // the target arena
  double lr[3] = {0, 0, 0};  // critic 1, critic 2, actor
  uint64_t seed = 0;
  iqlhip_awac() : SlabTrainer(QUEUE_STEPS) {}
  float *ws() const { return static_cast<float *>(mem); }
};

struct iqlhip_awac_group : SlabGroup<iqlhip_awac> {};

// The envelope, checked before any HIP call.
static int awac_check(const iqlhip_trainer_config *c) {
  if (!c) return fail(IQLHIP_ERR_INVALID, "null config");
  if (c->precision != IQLHIP_PREC_FP32)
    return fail(IQLHIP_ERR_UNSUPPORTED, "AWAC runs at precision fp32 only (the reference has no autocast)");
  if (c->n_hidden != 3) return fail(IQLHIP_ERR_UNSUPPORTED, "AWAC trains networks of three hidden layers (n_hidden %d)", c->n_hidden);
  if (c->hidden_dim < 16 || c->hidden_dim > AW_MAX_H || c->hidden_dim % 16)
    return fail(IQLHIP_ERR_UNSUPPORTED, "hidden_dim %d is not a multiple of 16 in 16..%d", c->hidden_dim, AW_MAX_H);
  if (c->state_dim < 1 || c->action_dim < 1 || c->batch_size < 1)
    return fail(IQLHIP_ERR_INVALID, "state_dim, action_dim and batch_size must be positive");
  if (c->state_dim > AW_MAX_S || c->action_dim > AW_MAX_A)
    return fail(IQLHIP_ERR_UNSUPPORTED, "state_dim %d > %d or action_dim %d > %d", c->state_dim, AW_MAX_S, c->action_dim,
                AW_MAX_A);
  // (the workspace is addressed with 32-bit element offsets: ~20 planes of hidden_dim x batch_size floats)
  if ((int64_t)c->batch_size > (1 << 16)) return fail(IQLHIP_ERR_UNSUPPORTED, "batch_size %d > 2^16", c->batch_size);
  if (c->dropout_p > 0.f) return fail(IQLHIP_ERR_UNSUPPORTED, "the AWAC networks have no dropout");
  return 0;
}

// Arena offsets: every tensor starts on a 128-byte line.
static AwShape awac_arena_shape(const iqlhip_trainer_config *c, int64_t *n_params, int64_t *n_target) {
  AwShape s{};
  s.S = c->state_dim, s.A = c->action_dim, s.B = c->batch_size, s.H = c->hidden_dim;
  s.SP = round_up(s.S, 16), s.AP = round_up(s.A, 16), s.BP = round_up(s.B, 16), s.XP = round_up(s.S + s.A, 16);
  s.row_stride = iqlhip_replay_row_stride(s.S, s.A), s.next_off = iqlhip_replay_next_offset(s.S, s.A);
  for (int n = 0; n < AW_NETS; ++n) {
    AwNet &N = s.net[n];
    const bool actor = n == AW_ACTOR;
    N.K1 = actor ? s.S : s.S + s.A, N.K1P = actor ? s.SP : s.XP, N.OUT = actor ? s.A : 1, N.OP = actor ? s.AP : 16;
  }
  int64_t off = 0;
  const auto take = [&](int64_t n) {
    const int64_t o = off;
    off += (n + 31) / 32 * 32;
    return (int)o;
  };
  const auto lay = [&](int n) {
    for (int l = 0; l < 4; ++l) {
      s.net[n].o_w[l] = take((int64_t)slab_out<4>(s, n, l) * slab_in(s, n, l));
      s.net[n].o_b[l] = take(slab_out<4>(s, n, l));
    }
  };
  lay(AW_ACTOR);
  s.o_log_std = take(s.A);
  const int64_t critics = off;
  lay(AW_C1), lay(AW_C2);
  if (n_params) *n_params = off;
  if (n_target) *n_target = off - critics;
  for (int t = 0; t < 2; ++t)
    for (int l = 0; l < 4; ++l) {
      s.net[AW_T1 + t].o_w[l] = s.net[AW_C1 + t].o_w[l] - (int)critics;
      s.net[AW_T1 + t].o_b[l] = s.net[AW_C1 + t].o_b[l] - (int)critics;
    }
  return s;
}

// The workspace of one trainer (element offsets, floats).  Everything is zero at creation; padding is only
// ever rewritten with zeros.  (Offsets into one allocation, not pointers as bc_step.hip's BcWorkspace holds: the
// members' arguments travel by value, and 16 members' pointers to some sixty pieces would not fit the 4 KB block.)
static size_t awac_plan(AwShape &s) {
  size_t off = 0;
  const auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 63) / 64 * 64;  // 256-byte blocks
    return (int)o;
  };
  for (int n = 0; n < AW_NETS; ++n) {
    AwNet &N = s.net[n];
    for (int l = 0; l < 4; ++l) N.c_w[l] = take((size_t)slab_op<4>(s, n, l) * slab_kp(s, n, l));
    if (n >= AW_T1) continue;
    for (int l = 1; l < 4; ++l) N.t_w[l - 1] = take((size_t)slab_kp(s, n, l) * slab_op<4>(s, n, l));
    for (int l = 0; l < 3; ++l) N.pl_h[l] = take((size_t)s.H * s.BP);
    for (int l = 0; l < 4; ++l) N.pl_dz[l] = take((size_t)slab_op<4>(s, n, l) * s.BP);
  }
  s.pl_x = take((size_t)s.XP * s.BP);
  s.o_eps = take((size_t)2 * s.B * s.A);
  s.o_qpart = take((size_t)4 * (s.BP / 16));  // doubles [BP / 16][2]
  s.o_apart = take((size_t)2 * (s.BP / 16));  // doubles [BP / 16]
  s.o_lsp = take((size_t)(s.BP / 16) * s.AP);
  return off * sizeof(float);
}

extern "C" int iqlhip_awac_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[25], int64_t *n_params,
                                        int64_t *n_target) {
  if (!offsets || !n_params || !n_target) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = awac_check(cfg)) return rc;
  const AwShape s = awac_arena_shape(cfg, n_params, n_target);
  int i = 0;
  for (int n = AW_ACTOR; n <= AW_C2; ++n) {
    for (int l = 0; l < 4; ++l) offsets[i++] = s.net[n].o_w[l], offsets[i++] = s.net[n].o_b[l];
    if (n == AW_ACTOR) offsets[i++] = s.o_log_std;
  }
  return 0;
}

static int awac_sync(iqlhip_awac *t, hipStream_t st) {
  const int n = AW_MAX_H * (t->s.XP > t->s.H ? t->s.XP : t->s.H);
  hipLaunchKernelGGL(k_awac_sync, dim3((n + 255) / 256, AW_NETS * AW_COPIES), dim3(256), 0, st, t->s, (const float *)t->P,
                     (const float *)t->T, t->ws());
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_awac_destroy(iqlhip_awac *t) { return slab_destroy(t); }

extern "C" int iqlhip_awac_create(iqlhip_awac **out, const iqlhip_trainer_config *cfg, double tau, float exp_adv_max,
                                  const iqlhip_arenas *arenas) {
  if (!out || !arenas) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = awac_check(cfg)) return rc;
  if (!arenas->params || !arenas->exp_avg || !arenas->exp_avg_sq || !arenas->target) return fail(IQLHIP_ERR_INVALID, "null arena");
  if (!(cfg->beta > 0.f) || !(exp_adv_max > 0.f)) return fail(IQLHIP_ERR_INVALID, "awac_lambda and exp_adv_max must be positive");
  if (!(tau >= 0.0 && tau <= 1.0)) return fail(IQLHIP_ERR_INVALID, "tau must lie in [0, 1]");
  iqlhip_awac *t = new (std::nothrow) iqlhip_awac;
  if (!t) return fail(IQLHIP_ERR_NOMEM, "out of host memory");
  t->s = awac_arena_shape(cfg, nullptr, nullptr);
  AwShape &s = t->s;
  // awac:215: the Python doubles tau and 1 - tau, each rounded to fp32 once (cfg->tau is already fp32: 1 - it is another number)
  s.gamma = cfg->discount, s.tau = (float)tau, s.one_m_tau = (float)(1.0 - tau);
  s.lambda = cfg->beta, s.exp_adv_max = exp_adv_max;
  s.two_over_B = (float)(2.0 / (double)s.B), s.fB = (float)s.B;
  t->P = arenas->params, t->M = arenas->exp_avg, t->V = arenas->exp_avg_sq, t->G = arenas->grads, t->T = arenas->target;
  t->lr[0] = cfg->lr_q, t->lr[1] = cfg->lr_v, t->lr[2] = cfg->lr_actor;
  t->beta1 = cfg->adam_beta1, t->beta2 = cfg->adam_beta2, t->eps = cfg->adam_eps, t->seed = cfg->seed;
  t->bytes = awac_plan(s);
  return slab_finish_create(out, t, [](iqlhip_awac *t) { return awac_sync(t, nullptr); });
}

extern "C" int iqlhip_awac_sync_weights(iqlhip_awac *t, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  return awac_sync(t, (hipStream_t)stream);
}

extern "C" int iqlhip_awac_set_step(iqlhip_awac *t, int64_t total_it) { return slab_set_step(t, total_it); }

extern "C" int iqlhip_awac_set_lr(iqlhip_awac *t, double lr_actor, double lr_critic_1, double lr_critic_2) {
  if (!t || !(lr_actor >= 0) || !(lr_critic_1 >= 0) || !(lr_critic_2 >= 0))
    return fail(IQLHIP_ERR_INVALID, "null trainer or negative lr");
  t->lr[0] = lr_critic_1, t->lr[1] = lr_critic_2, t->lr[2] = lr_actor;
  return 0;
}

extern "C" int iqlhip_awac_copy_out(iqlhip_awac *t, int32_t which, float *dst, void *stream) {
  if (!t || !dst) return fail(IQLHIP_ERR_INVALID, "null argument");
  const AwShape &s = t->s;
  const float *src = nullptr;
  size_t n = 0;
  if (which == 0) {
    src = t->ws() + s.o_eps, n = (size_t)2 * s.B * s.A;
  } else if (which >= 1 && which <= AW_NETS * AW_COPIES) {
    const int net = (which - 1) / AW_COPIES, kind = (which - 1) % AW_COPIES, l = kind >= 4 ? kind - 3 : kind;
    if (kind >= 4 && net >= AW_T1) return fail(IQLHIP_ERR_INVALID, "the targets have no transposed copies");
    src = t->ws() + (kind >= 4 ? s.net[net].t_w[l - 1] : s.net[net].c_w[l]);
    n = (size_t)slab_op<4>(s, net, l) * slab_kp(s, net, l);
  } else {
    return fail(IQLHIP_ERR_INVALID, "which must be in 0..%d", AW_NETS * AW_COPIES);
  }
  HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// n_steps steps of the members m[0..n): four launches per step for all of them.
static int awac_run(iqlhip_awac *const *mem, int n, SlabQueueBound &bound, const iqlhip_replay_view *views, int64_t n_steps,
                    const int64_t *const *idx, const float *const *eps, float *const *losses, hipStream_t st) {
  if (int rc = slab_check_call(mem, n, views, idx, n_steps, "AWAC")) return rc;
  AwArgs a{};
  a.s = mem[0]->s;
  for (int k = 0; k < n; ++k) {
    const iqlhip_awac *t = mem[k];
    AwMember &m = a.m[k];
    m.P = t->P, m.M = t->M, m.V = t->V, m.G = t->G, m.T = t->T, m.ws = t->ws();
    m.rows = views[k].rows, m.n_rows = views[k].n_rows, m.idx = idx[k], m.eps = eps ? eps[k] : nullptr;
    m.loss = losses ? losses[k] : nullptr, m.seed = t->seed, m.step0 = t->total_it;
  }
  const int slabs = a.s.BP / 16;
  const dim3 g1(slabs, n), g2((2 * slab_net_waves<4>(a.s, AW_C1) + 3) / 4, n), g4((slab_net_waves<4>(a.s, AW_ACTOR) + 1 + 3) / 4, n);
  return slab_run(mem, n, bound, n_steps, st, [&](int64_t i) {
    a.step = i;
    for (int k = 0; k < n; ++k) {
      const iqlhip_awac *t = mem[k];
      a.m[k].coef = make_adam_coef(t->beta1, t->beta2, t->eps, t->lr[0], t->lr[1], 0.0, 1, t->total_it + i + 1);
      a.m[k].coef.neg_step[2] =
          make_adam_coef(t->beta1, t->beta2, t->eps, t->lr[2], 0.0, 0.0, 1, t->total_it + i + 1).neg_step[0];
    }
    hipLaunchKernelGGL(k_awac_critic_fwd_bwd, g1, dim3(AW_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_awac_critic_update, g2, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_awac_actor_fwd_bwd, g1, dim3(AW_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_awac_actor_update, g4, dim3(256), 0, st, a);
  });
}

extern "C" int iqlhip_awac_group_create(iqlhip_awac_group **out, iqlhip_awac *const *members, int32_t n) {
  return slab_group_create(
      out, members, n,
      [](const AwShape &a, const AwShape &b) {
        return a.S == b.S && a.A == b.A && a.B == b.B && a.H == b.H && a.gamma == b.gamma && a.tau == b.tau &&
               a.lambda == b.lambda && a.exp_adv_max == b.exp_adv_max;
      },
      "dims, width, batch size, gamma, tau, awac_lambda and exp_adv_max");
}

extern "C" int iqlhip_awac_group_destroy(iqlhip_awac_group *g) { return slab_group_destroy(g); }

extern "C" int iqlhip_awac_group_train_steps(iqlhip_awac_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                             const int64_t *const *idx, const float *const *eps, float *const *losses_out,
                                             void *stream) {
  if (!g) return fail(IQLHIP_ERR_INVALID, "null group");
  return awac_run(g->member, g->n, g->bound, views, n_steps, idx, eps, losses_out, (hipStream_t)stream);
}

extern "C" int iqlhip_awac_train_steps(iqlhip_awac *t, const iqlhip_replay_view *view, int64_t n_steps, const int64_t *idx,
                                       const float *eps, float *losses_out, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  return awac_run(&t, 1, t->bound, view, n_steps, &idx, eps ? &eps : nullptr, losses_out ? &losses_out : nullptr,
                  (hipStream_t)stream);
}
