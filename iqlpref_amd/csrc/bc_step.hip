// Any-percent behaviour cloning (algorithms/minari/any_percent_bc.py, "bcref"): the training step of ONE
// network -- Actor [S, 256] ReLU [256, 256] ReLU [256, A] Tanh, times max_action (bcref:195-209);
// F.mse_loss(pi, action) (bcref:235-236); plain Adam (bcref:330) -- in two launches, exact fp32 MFMA
// (v_mfma_f32_16x16x4_f32) throughout.  No critics, no advantage weight, no schedule, no log_std, no dropout:
// nothing of the IQL step is launched or switched off here.
//
//   k_bc_fwd_bwd   one work-group of sixteen waves per 16-row slab and member: gathers the slab's rows by the step's indices,
//                  runs the three Linear layers forward with the activations held in LDS, forms the loss head
//                  and runs the backward down to dz1.  It leaves what the update needs feature-major
//                  ([feature][batch row]: the C layout of an MFMA tile is 4 consecutive rows of one feature per
//                  lane, one 16-byte store): x, h1, h2, dz1, dz2, dz3, and the slab's sum of squared errors.
//   k_bc_update    one wave per 16x16 tile of a weight matrix (dW = dz^T x activation, the batch as the K
//                  dimension) or per 16 bias entries; applies Adam (step_math.h: torch's _single_tensor_adam)
//                  to the fp32 masters and refreshes the padded copy the forward reads (W[out][in padded to 16])
//                  and the transposed copy the backward reads (W^T[in][out padded to 16]); one more wave adds
//                  the slab sums in slab order into the step's logged loss.
//
// A batch of any size is padded to whole 16-row slabs: padding rows gather nothing (their input is zero),
// their dz3 is zero and so is everything behind it, and the mean divides by the B x A real elements.
// The members of a group are the y coordinate of both launches; each member's arguments are its own entry
// of the by-value argument block, its arithmetic does not depend on who else is launched with it.
//
// The slab walk, the tile updates and the host side are slab_step.h's, with this family's policies: one MFMA
// chain per tile (OneChain), the bias gradient summed in float (SumFloat), step_math.h's adam_apply<false>.
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

constexpr int BC_H = 256;         // bcref:199-203: the fixed hidden width
constexpr int BC_MAX_S = 128, BC_MAX_A = 32;
constexpr int BC_LDS_STRIDE = BC_H + 4;  // floats; rows stay 16-byte aligned, 4 r mod 32 banks apart
constexpr int BC_WAVES = 16;             // of k_bc_fwd_bwd: one 16-feature tile of a 256-wide layer each
constexpr int BC_THREADS = BC_WAVES * WAVE;

struct BcShape {
  int S, A, B;
  int SP, AP, BP;  // padded to 16
  int row_stride;  // floats of a replay row
  float max_action, two_over_n;  // n = B x A (F.mse_loss: mean over all elements)
  // element offsets in the parameter arena (iqlhip_bc_arena_layout)
  int o_w1, o_b1, o_w2, o_b2, o_w3, o_b3;
};

// The workspace of one trainer (floats).  Everything is zero at creation; padding is only ever rewritten
// with zeros.
struct BcWorkspace {
  float *w1c, *w2c, *w3c;  // forward copies  [256][SP] [256][256] [AP][256]
  float *w2t, *w3t;        // transposed      [256][256] [256][AP]
  float *xT, *h1T, *h2T, *dz1T, *dz2T, *dz3T;  // feature-major planes [..][BP]
  double *partial;         // [BP / 16] sums of squared errors
};

static size_t bc_plan(WorkspacePlan &p, const BcShape &s, BcWorkspace &w) {
  w.w1c = p.take<float>((size_t)BC_H * s.SP);
  w.w2c = p.take<float>((size_t)BC_H * BC_H);
  w.w3c = p.take<float>((size_t)s.AP * BC_H);
  w.w2t = p.take<float>((size_t)BC_H * BC_H);
  w.w3t = p.take<float>((size_t)BC_H * s.AP);
  w.xT = p.take<float>((size_t)s.SP * s.BP);
  w.h1T = p.take<float>((size_t)BC_H * s.BP);
  w.h2T = p.take<float>((size_t)BC_H * s.BP);
  w.dz1T = p.take<float>((size_t)BC_H * s.BP);
  w.dz2T = p.take<float>((size_t)BC_H * s.BP);
  w.dz3T = p.take<float>((size_t)s.AP * s.BP);
  w.partial = p.take<double>((size_t)s.BP / 16);
  return p.end();
}

struct BcMember {
  float *P, *M, *V, *G;  // arenas (G may be null)
  BcWorkspace ws;
  const float *rows;     // replay rows of this call
  const int64_t *idx;    // [n_steps][B] of this call
  float *loss;           // [n_steps] of this call, or null
  int64_t n_rows;
  AdamCoef coef;         // of the step being launched (neg_step[0])
};

struct BcArgs {
  BcShape s;
  int64_t step;  // of this call
  BcMember m[IQLHIP_MAX_GROUP];
};

// ---------------------------------------------------------------------------------------------------
// forward / loss head / backward of one 16-row slab
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BC_THREADS) void k_bc_fwd_bwd(const BcArgs args) {
  const BcShape &s = args.s;
  const BcMember &m = args.m[blockIdx.y];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * 16;
  constexpr int LS = BC_LDS_STRIDE;
  __shared__ __attribute__((aligned(16))) float Xs[16 * (BC_MAX_S + 4)];
  __shared__ __attribute__((aligned(16))) float As[16 * (BC_MAX_A + 4)];
  __shared__ __attribute__((aligned(16))) float H1s[16 * LS], H2s[16 * LS], DZ2s[16 * LS];
  __shared__ __attribute__((aligned(16))) float DZ3s[16 * (BC_MAX_A + 4)];
  __shared__ int64_t ridx[16];
  __shared__ double sqs[2 * 64];  // the loss head's per-lane sums of squared errors
  const int XS = s.SP + 4, AS = s.AP + 4;

  // ---- gather (bcref:180-187): padding rows have no index and read nothing ----
  slab_row_indices(m.idx, args.step, s.B, r0, m.n_rows, ridx, tid);
  __syncthreads();
  for (int i = tid; i < 16 * s.SP; i += BC_THREADS) {
    const int r = i / s.SP, c = i - r * s.SP;
    const int64_t row = ridx[r];
    Xs[r * XS + c] = (row >= 0 && c < s.S) ? ldg(m.rows + row * s.row_stride + c) : 0.f;
  }
  for (int i = tid; i < 16 * s.AP; i += BC_THREADS) {
    const int r = i / s.AP, c = i - r * s.AP;
    const int64_t row = ridx[r];
    As[r * AS + c] = (row >= 0 && c < s.A) ? ldg(m.rows + row * s.row_stride + s.S + c) : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < 16 * s.SP; i += BC_THREADS) {  // x, feature-major, for dW1
    const int c = i >> 4, r = i & 15;
    stg(m.ws.xT + (size_t)c * s.BP + r0 + r, Xs[r * XS + c]);
  }

  const auto plane4 = [&](float *plane, int f, int row, const f32x4 &v) { slab_plane4(plane, s.BP, f, r0 + row, v); };
  // One 256-wide Linear layer of the slab, forward or backward: one 16-feature tile per wave, so slab_layer's tile
  // loop is one pass.  (Four waves with four tiles each measured 22.6k steps/s at the pen shape: a slab is a chain
  // of 256 dependent MFMAs per wave and wide layer; sixteen waves cut the chain to 64.)
  const auto wide_layer = [&](const float *act, int act_stride, const float *Wm, int K, auto &&ep) {
    slab_layer<OneChain, BC_WAVES>(act, act_stride, Wm, K, BC_WAVES, wave, lane, ep);
  };
  // ---- layer 1, layer 2: h = relu(x W^T + b) ----
  wide_layer(Xs, XS, m.ws.w1c, s.SP, [&](int f, int row, f32x4 z) {
    const float b = ldg(m.P + s.o_b1 + f);
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = fmaxf(z[e] + b, 0.f), H1s[(row + e) * LS + f] = z[e];
    plane4(m.ws.h1T, f, row, z);
  });
  __syncthreads();
  wide_layer(H1s, LS, m.ws.w2c, BC_H, [&](int f, int row, f32x4 z) {
    const float b = ldg(m.P + s.o_b2 + f);
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = fmaxf(z[e] + b, 0.f), H2s[(row + e) * LS + f] = z[e];
    plane4(m.ws.h2T, f, row, z);
  });
  __syncthreads();

  // ---- layer 3 and the loss head: pi = max_action tanh(z3), loss = mean (pi - a)^2 ----
  // (one 16-feature tile per wave, AP / 16 <= 2 of them; the other waves wait at the barrier)
  static_assert(BC_WAVES * 16 == BC_H, "one tile of a hidden layer per wave");
  // (its own k-loop: through slab_layer's unrolled walk the kernel takes 96 VGPRs instead of 54)
  if (wave < s.AP / 16) {
    using P = Prec<false>;
    const int r = lane & 15, q = lane >> 4, j = 16 * wave + r;
    f32x4 acc = {};
    for (int ks = 0; ks < BC_H / 16; ++ks) {
      const uint4 a = *reinterpret_cast<const uint4 *>(H2s + r * LS + ks * 16 + 4 * q);
      const uint4 b = ldg16(m.ws.w3c + (size_t)j * BC_H + ks * 16 + 4 * q);
      P::mma(a, b, acc);
    }
    const float b3 = j < s.A ? ldg(m.P + s.o_b3 + j) : 0.f;
    f32x4 dz;
    double sq = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = 4 * q + e;
      const bool real = j < s.A && r0 + row < s.B;
      // (tanh through double: correctly rounded, where tanhf is a few ulp off and pi - a cancels)
      const float t = (float)tanh((double)(acc[e] + b3));
      const float diff = s.max_action * t - As[row * AS + j];
      sq += real ? (double)(diff * diff) : 0.0;
      // mse_loss backward (2 / n) (pi - a), times max_action, through tanh
      dz[e] = real ? ((s.two_over_n * diff) * s.max_action) * (1.f - t * t) : 0.f;
      DZ3s[row * AS + j] = dz[e];
    }
    plane4(m.ws.dz3T, j, 4 * q, dz);
    sqs[64 * wave + lane] = sq;
  }
  __syncthreads();
  if (tid == 0) {  // in double and in one fixed order: the logged loss is the correctly rounded mean
    double t = 0.0;
    for (int i = 0; i < 64 * (s.AP / 16); ++i) t += sqs[i];
    stg(m.ws.partial + blockIdx.x, t);
  }

  // ---- backward: dz2 = (dz3 W3) [h2 > 0], dz1 = (dz2 W2) [h1 > 0] (the transposed copies) ----
  wide_layer(DZ3s, AS, m.ws.w3t, s.AP, [&](int f, int row, f32x4 g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = H2s[(row + e) * LS + f] > 0.f ? g[e] : 0.f, DZ2s[(row + e) * LS + f] = g[e];
    plane4(m.ws.dz2T, f, row, g);
  });
  __syncthreads();
  wide_layer(DZ2s, LS, m.ws.w2t, BC_H, [&](int f, int row, f32x4 g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = H1s[(row + e) * LS + f] > 0.f ? g[e] : 0.f;
    plane4(m.ws.dz1T, f, row, g);
  });
}

// ---------------------------------------------------------------------------------------------------
// dW per tile, Adam, the refreshed copies, the logged loss
// ---------------------------------------------------------------------------------------------------
// The waves of one member, in order: the 16x16 tiles of W2, W1, W3, then 16 bias entries each of b1, b2,
// b3, then the loss.
struct BcTiles {
  int w2, w1, w3, b1, b2, b3;
  __host__ __device__ int total() const { return w2 + w1 + w3 + b1 + b2 + b3 + 1; }
};
__host__ __device__ inline BcTiles bc_tiles(const BcShape &s) {
  return {16 * 16, 16 * (s.SP / 16), (s.AP / 16) * 16, 16, 16, s.AP / 16};
}

__global__ __launch_bounds__(256) void k_bc_update(const BcArgs args) {
  const BcShape &s = args.s;
  const BcMember &m = args.m[blockIdx.y];
  const int lane = threadIdx.x & 63;
  int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const BcTiles t = bc_tiles(s);
  if (w >= t.total()) return;
  const BcWorkspace &ws = m.ws;
  const auto adam = [&](float &p, float &mm, float &vv, float g) { adam_apply<false>(p, mm, vv, g, m.coef, m.coef.neg_step[0]); };
  // Linear W[OUT][IN] (or its bias) at `off`: dz and act the planes, fwd [..][KP] and tr [..][OP] the copies
  const auto tile = [&](int off, int OUT, int IN, const float *dz, const float *act, float *fwd, int KP, float *tr, int OP) {
    return SlabTile{m.P, m.M, m.V, m.G, (size_t)off, OUT, IN, OP, KP, s.BP, dz, act, fwd, tr, nullptr};
  };
  const auto weight = [&](const SlabTile &tl, int jt, int kt) { slab_weight_tile<OneChain>(tl, jt, kt, lane, adam, SlabNoTarget{}); };
  const auto bias = [&](int off, int OUT, const float *dz, int bt) {
    slab_bias_tile<SumFloat>(tile(off, OUT, 0, dz, nullptr, nullptr, 0, nullptr, 0), bt, lane, adam, SlabNoTarget{});
  };
  if (w < t.w2) return weight(tile(s.o_w2, BC_H, BC_H, ws.dz2T, ws.h1T, ws.w2c, BC_H, ws.w2t, BC_H), w >> 4, w & 15);
  w -= t.w2;
  if (w < t.w1) {
    const int nk = s.SP / 16;
    return weight(tile(s.o_w1, BC_H, s.S, ws.dz1T, ws.xT, ws.w1c, s.SP, nullptr, 0), w / nk, w % nk);
  }
  w -= t.w1;
  if (w < t.w3) return weight(tile(s.o_w3, s.A, BC_H, ws.dz3T, ws.h2T, ws.w3c, BC_H, ws.w3t, s.AP), w >> 4, w & 15);
  w -= t.w3;
  if (w < t.b1) return bias(s.o_b1, BC_H, ws.dz1T, w);
  w -= t.b1;
  if (w < t.b2) return bias(s.o_b2, BC_H, ws.dz2T, w);
  w -= t.b2;
  if (w < t.b3) return bias(s.o_b3, s.A, ws.dz3T, w);
  if (lane == 0 && m.loss) {  // actor_loss (bcref:236-237): the slab sums in slab order, over n
    double sum = 0.0;
    for (int i = 0; i < s.BP / 16; ++i) sum += ldg(ws.partial + i);
    stg(m.loss + args.step, (float)(sum / ((double)s.B * s.A)));
  }
}

// The copies from the fp32 masters (creation, load_state_dict): one thread per element of a padded copy.
__global__ void k_bc_sync(const BcShape s, const float *P, const BcWorkspace ws) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < BC_H * s.SP) slab_padded_copy(ws.w1c, P + s.o_w1, BC_H, s.S, BC_H, s.SP, false, i);
  if (i < BC_H * BC_H) {
    slab_padded_copy(ws.w2c, P + s.o_w2, BC_H, BC_H, BC_H, BC_H, false, i);
    slab_padded_copy(ws.w2t, P + s.o_w2, BC_H, BC_H, BC_H, BC_H, true, i);
  }
  if (i < s.AP * BC_H) {
    slab_padded_copy(ws.w3c, P + s.o_w3, s.A, BC_H, s.AP, BC_H, false, i);
    slab_padded_copy(ws.w3t, P + s.o_w3, s.A, BC_H, s.AP, BC_H, true, i);
  }
}

}  // namespace iqlhip

using namespace iqlhip;

// ---------------------------------------------------------------------------------------------------
// entry points (include/iqlhip.h)
// ---------------------------------------------------------------------------------------------------
struct iqlhip_bc : SlabTrainer {
  static constexpr int QUEUE_STEPS = 1024;  // at most ~2 x 1024 steps are ever queued ahead of the device
  BcShape s{};
  BcWorkspace ws{};
  double lr = 0;
  iqlhip_bc() : SlabTrainer(QUEUE_STEPS) {}
};

struct iqlhip_bc_group : SlabGroup<iqlhip_bc> {};

// The envelope, checked before any HIP call.
static int bc_check(const iqlhip_trainer_config *c) {
  if (!c) return fail(IQLHIP_ERR_INVALID, "null config");
  if (c->precision != IQLHIP_PREC_FP32)
    return fail(IQLHIP_ERR_UNSUPPORTED, "behaviour cloning runs at precision fp32 only (the reference has no autocast)");
  if (c->hidden_dim != BC_H || (c->n_hidden != 0 && c->n_hidden != 2))
    return fail(IQLHIP_ERR_UNSUPPORTED, "behaviour cloning trains the reference's 256-256 actor (hidden_dim %d, n_hidden %d)",
                c->hidden_dim, c->n_hidden);
  if (c->state_dim < 1 || c->action_dim < 1 || c->batch_size < 1)
    return fail(IQLHIP_ERR_INVALID, "state_dim, action_dim and batch_size must be positive");
  if (c->state_dim > BC_MAX_S || c->action_dim > BC_MAX_A)
    return fail(IQLHIP_ERR_UNSUPPORTED, "state_dim %d > %d or action_dim %d > %d", c->state_dim, BC_MAX_S, c->action_dim,
                BC_MAX_A);
  if ((int64_t)c->batch_size > (1 << 20)) return fail(IQLHIP_ERR_UNSUPPORTED, "batch_size %d > 2^20", c->batch_size);
  if (c->dropout_p > 0.f) return fail(IQLHIP_ERR_UNSUPPORTED, "the behaviour-cloning actor has no dropout");
  return 0;
}

static BcShape bc_shape(const iqlhip_trainer_config *c, float max_action) {
  BcShape s{};
  s.S = c->state_dim, s.A = c->action_dim, s.B = c->batch_size;
  s.SP = round_up(s.S, 16), s.AP = round_up(s.A, 16), s.BP = round_up(s.B, 16);
  s.row_stride = iqlhip_replay_row_stride(s.S, s.A);
  const double n = (double)s.B * s.A;
  s.max_action = max_action, s.two_over_n = (float)(2.0 / n);
  s.o_w1 = 0, s.o_b1 = s.o_w1 + BC_H * s.S, s.o_w2 = s.o_b1 + BC_H, s.o_b2 = s.o_w2 + BC_H * BC_H;
  s.o_w3 = s.o_b2 + BC_H, s.o_b3 = s.o_w3 + s.A * BC_H;
  return s;
}

extern "C" int iqlhip_bc_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[6], int64_t *n_params) {
  if (!offsets || !n_params) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = bc_check(cfg)) return rc;
  const BcShape s = bc_shape(cfg, 1.f);
  const int o[6] = {s.o_w1, s.o_b1, s.o_w2, s.o_b2, s.o_w3, s.o_b3};
  for (int i = 0; i < 6; ++i) offsets[i] = o[i];
  *n_params = s.o_b3 + s.A;
  return 0;
}

static int bc_sync(iqlhip_bc *t, hipStream_t st) {
  const int n = BC_H * (t->s.SP > BC_H ? t->s.SP : BC_H);
  hipLaunchKernelGGL(k_bc_sync, dim3((n + 255) / 256), dim3(256), 0, st, t->s, (const float *)t->P, t->ws);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_bc_destroy(iqlhip_bc *t) { return slab_destroy(t); }

extern "C" int iqlhip_bc_create(iqlhip_bc **out, const iqlhip_trainer_config *cfg, float max_action,
                                const iqlhip_arenas *arenas) {
  if (!out || !arenas) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = bc_check(cfg)) return rc;
  if (!arenas->params || !arenas->exp_avg || !arenas->exp_avg_sq) return fail(IQLHIP_ERR_INVALID, "null arena");
  if (!(max_action > 0.f)) return fail(IQLHIP_ERR_INVALID, "max_action must be positive");
  iqlhip_bc *t = new (std::nothrow) iqlhip_bc;
  if (!t) return fail(IQLHIP_ERR_NOMEM, "out of host memory");
  t->s = bc_shape(cfg, max_action);
  t->P = arenas->params, t->M = arenas->exp_avg, t->V = arenas->exp_avg_sq, t->G = arenas->grads;
  t->lr = cfg->lr_actor, t->beta1 = cfg->adam_beta1, t->beta2 = cfg->adam_beta2, t->eps = cfg->adam_eps;
  WorkspacePlan measure;
  BcWorkspace none;
  t->bytes = bc_plan(measure, t->s, none);
  return slab_finish_create(out, t, [](iqlhip_bc *t) {
    WorkspacePlan place(t->mem);
    bc_plan(place, t->s, t->ws);
    return bc_sync(t, nullptr);
  });
}

extern "C" int iqlhip_bc_sync_weights(iqlhip_bc *t, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  return bc_sync(t, (hipStream_t)stream);
}

extern "C" int iqlhip_bc_set_step(iqlhip_bc *t, int64_t total_it) { return slab_set_step(t, total_it); }

extern "C" int iqlhip_bc_set_lr(iqlhip_bc *t, double lr) {
  if (!t || !(lr >= 0)) return fail(IQLHIP_ERR_INVALID, "null trainer or negative lr");
  t->lr = lr;
  return 0;
}

extern "C" int iqlhip_bc_copy_out(iqlhip_bc *t, int32_t which, float *dst, void *stream) {
  if (!t || !dst) return fail(IQLHIP_ERR_INVALID, "null argument");
  const BcShape &s = t->s;
  const float *src[5] = {t->ws.w1c, t->ws.w2c, t->ws.w3c, t->ws.w2t, t->ws.w3t};
  const size_t n[5] = {(size_t)BC_H * s.SP, (size_t)BC_H * BC_H, (size_t)s.AP * BC_H, (size_t)BC_H * BC_H,
                       (size_t)BC_H * s.AP};
  if (which < 0 || which > 4) return fail(IQLHIP_ERR_INVALID, "which must be in 0..4");
  HIP_TRY(hipMemcpyAsync(dst, src[which], n[which] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// n_steps steps of the members m[0..n): two launches per step for all of them.
static int bc_run(iqlhip_bc *const *mem, int n, SlabQueueBound &bound, const iqlhip_replay_view *views, int64_t n_steps,
                  const int64_t *const *idx, float *const *losses, hipStream_t st) {
  if (int rc = slab_check_call(mem, n, views, idx, n_steps, "behaviour cloning")) return rc;
  BcArgs a{};
  a.s = mem[0]->s;
  for (int k = 0; k < n; ++k) {
    const iqlhip_bc *t = mem[k];
    BcMember &m = a.m[k];
    m.P = t->P, m.M = t->M, m.V = t->V, m.G = t->G, m.ws = t->ws;
    m.rows = views[k].rows, m.n_rows = views[k].n_rows, m.idx = idx[k], m.loss = losses ? losses[k] : nullptr;
  }
  const BcTiles tiles = bc_tiles(a.s);
  const dim3 g1(a.s.BP / 16, n), g2((tiles.total() + 3) / 4, n);
  return slab_run(mem, n, bound, n_steps, st, [&](int64_t i) {
    a.step = i;
    for (int k = 0; k < n; ++k)
      a.m[k].coef = make_adam_coef(mem[k]->beta1, mem[k]->beta2, mem[k]->eps, mem[k]->lr, mem[k]->lr, mem[k]->lr, 1,
                                   mem[k]->total_it + i + 1);
    hipLaunchKernelGGL(k_bc_fwd_bwd, g1, dim3(BC_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_bc_update, g2, dim3(256), 0, st, a);
  });
}

extern "C" int iqlhip_bc_group_create(iqlhip_bc_group **out, iqlhip_bc *const *members, int32_t n) {
  return slab_group_create(
      out, members, n,
      [](const BcShape &a, const BcShape &b) { return a.S == b.S && a.A == b.A && a.B == b.B && a.max_action == b.max_action; },
      "dims, batch size and max_action");
}

extern "C" int iqlhip_bc_group_destroy(iqlhip_bc_group *g) { return slab_group_destroy(g); }

extern "C" int iqlhip_bc_group_train_steps(iqlhip_bc_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                           const int64_t *const *idx, float *const *losses_out, void *stream) {
  if (!g) return fail(IQLHIP_ERR_INVALID, "null group");
  return bc_run(g->member, g->n, g->bound, views, n_steps, idx, losses_out, (hipStream_t)stream);
}

extern "C" int iqlhip_bc_train_steps(iqlhip_bc *t, const iqlhip_replay_view *view, int64_t n_steps, const int64_t *idx,
                                     float *losses_out, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  return bc_run(&t, 1, t->bound, view, n_steps, &idx, losses_out ? &losses_out : nullptr, (hipStream_t)stream);
}
