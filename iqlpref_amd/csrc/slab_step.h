// The slab-step core: what the behaviour-cloning step (bc_step.hip), the AWAC step (awac_step.hip) and the TD3+BC
// step (td3_bc_step.hip) are made of.  A training step of this kind is
//
//   a slab launch    one work-group of WAVES waves walks a 16-row slab of the batch through its layers with the
//                    activations in LDS (slab_layer), and leaves x, h and dz feature-major ([feature][batch row],
//                    slab_plane4) for
//   an update launch one wave per 16x16 tile of a weight matrix (slab_weight_tile: dW = dz^T x activation, the
//                    batch as the K dimension) or per 16 bias entries (slab_bias_tile): Adam on the fp32 masters,
//                    the padded forward copy and the transposed copy refreshed (slab_padded_copy builds them from
//                    the masters at creation), an optional Polyak-averaged twin.
//
// Group members are gridDim.y of a by-value argument block; the host side is one trainer core (SlabTrainer), one
// group (SlabGroup), one bound on queued work (SlabQueueBound) and one step loop (slab_run).
//
// The families differ on purpose in three pieces of arithmetic; each is a compile-time policy here, never a merged
// formula ("The slab-step core"):
//                            BC                  | AWAC                          | TD3+BC
//   MFMA accumulation        OneChain            | FourChains (added pairwise)   | FourChains
//   bias-gradient batch sum  SumFloat            | SumDouble                     | SumDouble
//   Adam (the `adam` call)   adam_apply<false>   | adam_apply_v64 on the fp32    | adam_apply_v64 on the doubles beta2
//                                                | b2, 1 - b2 of AdamCoef        | and 1 - beta2: a third policy
// The actor-critic families (AWAC, TD3+BC) also share their walk: the gather, the noise, the hidden layers, a critic's
// head, the backward and the update's wave order, generic over depth and LDS strides (below).
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <type_traits>

#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"

namespace iqlhip {

// ---------------------------------------------------------------------------------------------------
// device: the slab walk
// ---------------------------------------------------------------------------------------------------
// Exact fp32 MFMA (common.h, Prec<false>) on ONE accumulator: the sequential sum over K.
struct OneChain {
  static constexpr bool UNROLL_LAYER = true;  // (slab_layer: the walk keeps the unroll it was tuned with)
  f32x4 acc = {};
  __device__ __forceinline__ void mma(const uint4 &a, const uint4 &b) { Prec<false>::mma(a, b, acc); }
  __device__ __forceinline__ f32x4 sum() const { return acc; }
};

// The same MFMAs on four accumulators, one per component of the 16-byte fragments, added pairwise at the end: four
// independent chains a quarter as long as one -- a quarter of the latency between dependent MFMAs, and the
// rounding error of a four-way pairwise sum instead of a sequential one.
struct FourChains {
  static constexpr bool UNROLL_LAYER = false;
  f32x4 acc[4] = {};
  __device__ __forceinline__ void mma(const uint4 &a, const uint4 &b) {
    const float4 af = __builtin_bit_cast(float4, a), bf = __builtin_bit_cast(float4, b);
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.x, bf.x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.y, bf.y, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.z, bf.z, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.w, bf.w, acc[3], 0, 0, 0);
  }
  __device__ __forceinline__ f32x4 sum() const { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }
};

// The slab's rows: the first sixteen threads write ridx[16], the step's row numbers of rows r0 .. r0 + 15 clamped
// into the buffer, -1 for padding rows (they have no index and read nothing).  No barrier of its own.
__device__ __forceinline__ void slab_row_indices(const int64_t *idx, int64_t step, int B, int r0, int64_t n_rows,
                                                 int64_t *ridx, int tid) {
  if (tid < 16) {
    int64_t i = -1;
    if (r0 + tid < B) {
      i = ldg(idx + step * B + r0 + tid);
      i = i < 0 ? 0 : (i >= n_rows ? n_rows - 1 : i);  // (an index outside the buffer must not leave it)
    }
    ridx[tid] = i;
  }
}

// Four consecutive batch rows (from `row`) of feature f of a feature-major plane [..][BP]: the C layout of an MFMA
// tile is 4 consecutive rows of one feature per lane, one 16-byte store.
__device__ __forceinline__ void slab_plane4(float *plane, int BP, int f, int row, const f32x4 &v) {
  stg16(plane + (size_t)f * BP + row, make_float4(v[0], v[1], v[2], v[3]));
}

// One Linear layer of the slab, forward or backward: tile t (features 16 t .. 16 t + 16) of out[16][16 n_tiles] =
// act[16][K] (LDS, rows act_stride apart) x Wm^T, Wm row-major [16 n_tiles][K] (row = output feature, 16-byte
// pieces along K); the tiles go round the WAVES waves.  ep(feature, first of 4 rows, values).  With n_tiles ==
// WAVES known at compile time the tile loop is one pass.
template <class Acc, int WAVES, class Epilogue>
__device__ __forceinline__ void slab_layer(const float *act, int act_stride, const float *Wm, int K, int n_tiles,
                                           int wave, int lane, Epilogue &&ep) {
  const int r = lane & 15, q = lane >> 4;
  for (int t = wave; t < n_tiles; t += WAVES) {
    const int f = 16 * t + r;
    Acc acc;
    const auto k_step = [&](int ks) {
      const uint4 a = *reinterpret_cast<const uint4 *>(act + r * act_stride + ks * 16 + 4 * q);
      const uint4 b = ldg16(Wm + (size_t)f * K + ks * 16 + 4 * q);
      acc.mma(a, b);
    };
    if constexpr (Acc::UNROLL_LAYER) {
#pragma unroll 4
      for (int ks = 0; ks < K / 16; ++ks) k_step(ks);
    } else {
      for (int ks = 0; ks < K / 16; ++ks) k_step(ks);
    }
    ep(f, 4 * q, acc.sum());
  }
}

// ---------------------------------------------------------------------------------------------------
// device: the walk of the actor-critic families (AWAC: L = 4 Linears per network; TD3+BC: L = 3)
// ---------------------------------------------------------------------------------------------------
// Their shapes (AwShape, TdShape) spell these fields alike: S, A, B, H, XP, BP, row_stride, next_off and per network
// net[n].{K1, K1P, OUT, OP}.  Linear l of network n has OUT x IN real entries, padded to OP x KP.
template <int L, class Shape>
__host__ __device__ inline int slab_out(const Shape &s, int n, int l) { return l < L - 1 ? s.H : s.net[n].OUT; }
template <int L, class Shape>
__host__ __device__ inline int slab_op(const Shape &s, int n, int l) { return l < L - 1 ? s.H : s.net[n].OP; }
template <class Shape>
__host__ __device__ inline int slab_in(const Shape &s, int n, int l) { return l == 0 ? s.net[n].K1 : s.H; }
template <class Shape>
__host__ __device__ inline int slab_kp(const Shape &s, int n, int l) { return l == 0 ? s.net[n].K1P : s.H; }

// The waves of one network's update, in order: the 16x16 tiles of W1..WL, then 16 bias entries each of b1..bL.
template <int L, class Shape>
__host__ __device__ inline int slab_net_waves(const Shape &s, int n) {
  int t = 0;
  for (int l = 0; l < L; ++l) t += (slab_op<L>(s, n, l) / 16) * (slab_kp(s, n, l) / 16) + slab_op<L>(s, n, l) / 16;
  return t;
}

// The slab's rows: padding rows have no index and read nothing.  X[16][XS] = (s | a | 0) (or null), X2 = (s' | 0) or
// (s | 0) (`next`; or null), rd = reward and done (or null).  Ends behind a barrier.
template <int XS, int THREADS, class Shape>
__device__ __forceinline__ void slab_gather(const Shape &s, const int64_t *idx, const float *rows, int64_t n_rows,
                                            int64_t step, int r0, bool next, float *X, float *X2, float *rd, int64_t *ridx,
                                            int tid) {
  slab_row_indices(idx, step, s.B, r0, n_rows, ridx, tid);
  __syncthreads();
  for (int i = tid; i < 16 * s.XP; i += THREADS) {
    const int r = i / s.XP, c = i - r * s.XP;
    const int64_t row = ridx[r];
    const bool real = row >= 0;
    if (X) X[r * XS + c] = (real && c < s.S + s.A) ? ldg(rows + row * s.row_stride + c) : 0.f;
    if (X2) X2[r * XS + c] = (real && c < s.S) ? ldg(rows + row * s.row_stride + (next ? s.next_off : 0) + c) : 0.f;
  }
  if (rd && tid < 32) {
    const int64_t row = ridx[tid & 15];
    rd[tid] = row >= 0 ? ldg(rows + row * s.row_stride + s.S + s.A + (tid >> 4)) : 0.f;
  }
  __syncthreads();
}

// The NH hidden layers (Linear + ReLU) of one network over the slab: in [16][K1P] -> bufs[0] -> .. -> bufs[NH - 1]
// (LDS, [16][LS]; entries may repeat where nothing is kept), weights from the forward copies ws + c_w[l], biases from
// arena + o_b[l].  planes (or null): layer l is also kept feature-major at planes + pl_h[l].  Ends behind a barrier.
template <int NH, int LS, int WAVES, class Acc>
__device__ __forceinline__ void slab_hidden(const float *in, int in_stride, const float *ws, const int *c_w, int K1P, int H,
                                            const float *arena, const int *o_b, float *const (&bufs)[NH], float *planes,
                                            const int *pl_h, int BP, int r0, int wave, int lane) {
#pragma unroll
  for (int l = 0; l < NH; ++l) {
    float *dst = bufs[l];
    slab_layer<Acc, WAVES>(l == 0 ? in : bufs[l - 1], l == 0 ? in_stride : LS, ws + c_w[l], l == 0 ? K1P : H, H / 16, wave, lane,
                           [&](int f, int row, f32x4 z) {
                             const float b = ldg(arena + o_b[l] + f);
#pragma unroll
                             for (int e = 0; e < 4; ++e) z[e] = fmaxf(z[e] + b, 0.f), dst[(row + e) * LS + f] = z[e];
                             if (planes) slab_plane4(planes + pl_h[l], BP, f, r0 + row, z);
                           });
    __syncthreads();
  }
}

// A critic's value of the slab's rows, q[16] = h Wc^T + b: one tile, its column 0.  Ends behind a barrier.
template <int LS, int WAVES, class Acc>
__device__ __forceinline__ void slab_q(const float *h, const float *Wc, int H, const float *bias, float *q, int wave, int lane) {
  slab_layer<Acc, WAVES>(h, LS, Wc, H, 1, wave, lane, [&](int f, int row, f32x4 z) {
    if (f != 0) return;
    const float b = ldg(bias);
#pragma unroll
    for (int e = 0; e < 4; ++e) q[row + e] = z[e] + b;
  });
  __syncthreads();
}

// The backward of a trained network from the head gradient DZ [16][DS] (LDS, OP columns): hidden layer l = NH - 1 .. 0
// takes dz_l = (dz_(l+1) W_(l+1)) [h_l > 0] through the transposed copy ws + t_w[l] of the Linear behind it; it
// replaces h_l in bufs[l] (layer 0 only when `keep_first`) and, with planes, goes to planes + pl_dz[l].  Ends behind
// a barrier.
template <int NH, int LS, int DS, int WAVES, class Acc>
__device__ __forceinline__ void slab_backward(const float *DZ, int OP, const float *ws, const int *t_w, int H,
                                              float *const (&bufs)[NH], bool keep_first, float *planes, const int *pl_dz,
                                              int BP, int r0, int wave, int lane) {
#pragma unroll
  for (int l = NH - 1; l >= 0; --l) {
    float *h = bufs[l];
    const bool keep = l > 0 || keep_first;
    slab_layer<Acc, WAVES>(l == NH - 1 ? DZ : bufs[l + 1], l == NH - 1 ? DS : LS, ws + t_w[l], l == NH - 1 ? OP : H, H / 16, wave,
                           lane, [&](int f, int row, f32x4 g) {
#pragma unroll
                             for (int e = 0; e < 4; ++e) {
                               g[e] = h[(row + e) * LS + f] > 0.f ? g[e] : 0.f;
                               if (keep) h[(row + e) * LS + f] = g[e];
                             }
                             if (planes) slab_plane4(planes + pl_dz[l], BP, f, r0 + row, g);
                           });
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// device: arithmetic the actor-critic families (AWAC, TD3+BC) spell the same way
// ---------------------------------------------------------------------------------------------------
// A standard normal of (row, column) of the step: Box-Muller in double on one Philox block per four columns.
__device__ __forceinline__ float slab_normal(uint64_t seed, int64_t step, int row, int c, uint32_t stream) {
  const Philox4 r = philox4x32_10((uint32_t)row * 8u + (uint32_t)(c >> 2), (uint32_t)step, (uint32_t)((uint64_t)step >> 32),
                                  stream, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t ua = (c & 2) ? r.z : r.x, ub = (c & 2) ? r.w : r.y;
  const double u1 = ((double)ua + 1.0) * (1.0 / 4294967296.0), u2 = (double)ub * (1.0 / 4294967296.0);
  // (sinpi / cospi: the angle 2 pi u2 without the large-argument reduction of sin / cos, which costs registers)
  const double rad = sqrt(-2.0 * log(u1)), turn = 2.0 * u2;
  return (float)(rad * ((c & 1) ? sinpi(turn) : cospi(turn)));
}

// The slab's standard normals of one draw, one thread per (row, column): read from eps ([B][A] of this draw) or
// (null) drawn by slab_normal, kept at `kept` ([B][A], the workspace) and in EPS[16][DS].  Padding rows draw and read
// nothing.  No barrier of its own.
template <int DS, int THREADS>
__device__ __forceinline__ void slab_noise(const float *eps, float *kept, uint64_t seed, int64_t step, uint32_t stream, int B,
                                           int A, float *EPS, int r0, int tid) {
  for (int i = tid; i < 16 * A; i += THREADS) {
    const int r = i / A, j = i - r * A, gr = r0 + r;
    float ep = 0.f;
    if (gr < B) {
      ep = eps ? ldg(eps + (size_t)gr * A + j) : slab_normal(seed, step, gr, j, stream);
      stg(kept + (size_t)gr * A + j, ep);
    }
    EPS[r * DS + j] = ep;
  }
}

// awac:275, tdbc:345: r + gamma * (1 - d) * q_next in the tensor expression's order (the product of the two
// factors first, in either order)
__device__ __forceinline__ float slab_td_target(float r, float d, float gamma, float qn) {
#pragma clang fp contract(off)
  return r + (gamma * (1.f - d)) * qn;
}

// awac:215, tdbc:79: (1 - tau) * t + tau * p, two rounded products and a sum
__device__ __forceinline__ float slab_polyak(float one_m_tau, float tau, float t, float p) {
#pragma clang fp contract(off)
  return (one_m_tau * t) + (tau * p);
}

// ---------------------------------------------------------------------------------------------------
// device: the update
// ---------------------------------------------------------------------------------------------------
// One Linear of one network as the update sees it.  W[OUT][IN] and b[OUT] are real entries of the arenas from
// `off`; dz [OP][BP] and act [KP][BP] are feature-major planes; fwd [OP][KP] is the padded copy the forward reads,
// tr [KP][OP] (or null) the transposed copy the backward reads, tfwd (or null) the forward copy of the target.
struct SlabTile {
  float *P, *M, *V, *G;  // arenas (G may be null)
  size_t off;            // of the tensor in P, M, V, G
  int OUT, IN, OP, KP, BP;
  const float *dz, *act;
  float *fwd, *tr, *tfwd;
};

// `target` of a network without a Polyak-averaged twin.
struct SlabNoTarget {};

// The batch sum of a bias gradient, one wave per 16 features: every lane adds its 4 rows per 16-row slab, the four
// lanes of a feature are then added across the wave.
struct SumFloat {
  float g = 0.f;
  __device__ __forceinline__ void add(const float4 &v) { g += (v.x + v.y) + (v.z + v.w); }
  __device__ __forceinline__ float total() {
    g = xor16_sum(g);
    g = xor32_sum(g);
    return g;
  }
};
// (in double: the rows' terms cancel, and a one-entry bias has no other entries to hide behind)
struct SumDouble {
  double g = 0.0;
  __device__ __forceinline__ void add(const float4 &v) { g += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w); }
  __device__ __forceinline__ float total() {
    g += __shfl_xor(g, 16);
    g += __shfl_xor(g, 32);
    return (float)g;
  }
};

// Adam on entry o of the arenas with gradient g; returns the new parameter.
template <class Adam>
__device__ __forceinline__ float slab_adam_entry(const SlabTile &t, size_t o, float g, Adam &&adam) {
  float p = ldg(t.P + o), mm = ldg(t.M + o), vv = ldg(t.V + o);
  adam(p, mm, vv, g);
  stg(t.P + o, p), stg(t.M + o, mm), stg(t.V + o, vv);
  if (t.G) stg(t.G + o, g);
  return p;
}

// One weight tile: rows jt (output features), columns kt (input features).  adam(p, m, v, g) steps one entry;
// target(entry within the tensor, new parameter) writes the target's master and returns it (or SlabNoTarget).
template <class Acc, class Adam, class Target>
__device__ __forceinline__ void slab_weight_tile(const SlabTile &t, int jt, int kt, int lane, Adam &&adam, Target &&target) {
  constexpr bool has_target = !std::is_same_v<std::decay_t<Target>, SlabNoTarget>;
  const int r = lane & 15, q = lane >> 4;
  Acc accs;
  const float *ap = t.dz + (size_t)(16 * jt + r) * t.BP + 4 * q;
  const float *bp = t.act + (size_t)(16 * kt + r) * t.BP + 4 * q;
  for (int ks = 0; ks < t.BP / 16; ++ks) accs.mma(ldg16(ap + ks * 16), ldg16(bp + ks * 16));
  const f32x4 acc = accs.sum();
  const int k = 16 * kt + r;  // C layout: column = lane & 15, rows 4 q + e
  float pv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 16 * jt + 4 * q + e;
    float tv = 0.f;
    pv[e] = 0.f;
    if (j < t.OUT && k < t.IN) {
      const size_t rel = (size_t)j * t.IN + k;
      pv[e] = slab_adam_entry(t, t.off + rel, acc[e], adam);
      if constexpr (has_target) tv = target(rel, pv[e]);
    }
    stg(t.fwd + (size_t)j * t.KP + k, pv[e]);
    if constexpr (has_target) stg(t.tfwd + (size_t)j * t.KP + k, tv);
  }
  if (t.tr) stg16(t.tr + (size_t)k * t.OP + 16 * jt + 4 * q, make_float4(pv[0], pv[1], pv[2], pv[3]));
}

// 16 bias entries (t.off: the bias): db[f] = sum over the batch rows of dz[f][.]
template <class Sum, class Adam, class Target>
__device__ __forceinline__ void slab_bias_tile(const SlabTile &t, int bt, int lane, Adam &&adam, Target &&target) {
  const int r = lane & 15, q = lane >> 4, f = 16 * bt + r;
  Sum sum;
  for (int ks = 0; ks < t.BP / 16; ++ks)
    sum.add(__builtin_bit_cast(float4, ldg16(t.dz + (size_t)f * t.BP + ks * 16 + 4 * q)));
  const float g = sum.total();
  if (q == 0 && f < t.OUT) {
    const float p = slab_adam_entry(t, t.off + f, g, adam);
    if constexpr (!std::is_same_v<std::decay_t<Target>, SlabNoTarget>) target((size_t)f, p);
  }
}

// Wave w of network n's update (w < slab_net_waves<L>): a weight tile or 16 bias entries of Linear l.  tile(l, bias)
// gives the SlabTile of Linear l (off: its weight, or its bias), target(l, bias) the `target` of that tensor.
template <int L, class Acc, class Sum, class Shape, class Tile, class Adam, class Target>
__device__ __forceinline__ void slab_update_wave(const Shape &s, int n, int w, int lane, Tile &&tile, Adam &&adam,
                                                 Target &&target) {
  for (int l = 0; l < L; ++l) {
    const int nk = slab_kp(s, n, l) / 16, cnt = (slab_op<L>(s, n, l) / 16) * nk;
    if (w < cnt) return slab_weight_tile<Acc>(tile(l, false), w / nk, w % nk, lane, adam, target(l, false));
    w -= cnt;
  }
  for (int l = 0; l < L; ++l) {
    const int cnt = slab_op<L>(s, n, l) / 16;
    if (w < cnt) return slab_bias_tile<Sum>(tile(l, true), w, lane, adam, target(l, true));
    w -= cnt;
  }
}

// Element i of a padded copy of W[OUT][IN] (masters at src): the forward copy [OP][KP], or (`tr`) the transposed
// copy [KP][OP].  Padding is zero.
__device__ __forceinline__ void slab_padded_copy(float *dst, const float *src, int OUT, int IN, int OP, int KP, bool tr,
                                                 int i) {
  const int j = tr ? i % OP : i / KP, k = tr ? i / OP : i % KP;
  stg(dst + i, (j < OUT && k < IN) ? ldg(src + (size_t)j * IN + k) : 0.f);
}

// ---------------------------------------------------------------------------------------------------
// host: the trainer core, the group, the step loop
// ---------------------------------------------------------------------------------------------------
// Bounds what calls leave queued ahead of the device: one event, synchronise-then-record every `every` steps, so
// at most ~2 x every steps are ever queued.  (api.hip's Throttle is another mechanism: dispatch-count windows.)
struct SlabQueueBound {
  const int every;
  hipEvent_t ev = nullptr;
  bool used = false;
  explicit SlabQueueBound(int every_) : every(every_) {}
  bool due(int64_t i) const { return i % every == every - 1; }
  int hold(hipStream_t st) {
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (used) HIP_TRY(hipEventSynchronize(ev));
    HIP_TRY(hipEventRecord(ev, st));
    used = true;
    return 0;
  }
  void release(bool wait) {
    if (!ev) return;
    if (wait) (void)hipEventSynchronize(ev);
    (void)hipEventDestroy(ev);
  }
};

// What a trainer of either family holds: the borrowed arenas, its workspace, Adam's constants, the step count.  A
// family's opaque type derives from it and names the steps of its queue bound (QUEUE_STEPS).
struct SlabTrainer {
  float *P = nullptr, *M = nullptr, *V = nullptr, *G = nullptr;
  void *mem = nullptr;  // the workspace
  size_t bytes = 0;
  double beta1 = 0, beta2 = 0, eps = 0;
  int64_t total_it = 0;
  SlabQueueBound bound;
  explicit SlabTrainer(int queue_steps) : bound(queue_steps) {}
};

template <class T>
int slab_destroy(T *t) {
  if (!t) return 0;
  if (t->mem) {
    (void)hipDeviceSynchronize();
    (void)hipFree(t->mem);
  }
  t->bound.release(false);
  delete t;
  return 0;
}

// The tail of a family's create, t->bytes known: allocates and zeroes the workspace, builds the weight copies
// (sync(t): places what it has to in t->mem and launches the family's sync kernel on the null stream), waits.  On
// any failure everything built is destroyed.
template <class T, class Sync>
int slab_finish_create(T **out, T *t, Sync &&sync) {
  const size_t bytes = t->bytes;
  if (hipMalloc(&t->mem, bytes) != hipSuccess) {
    t->mem = nullptr;
    slab_destroy(t);
    return fail(IQLHIP_ERR_NOMEM, "hipMalloc of %zu workspace bytes failed", bytes);
  }
  int rc = 0;
  if (hipMemset(t->mem, 0, bytes) != hipSuccess) rc = fail(IQLHIP_ERR_HIP, "hipMemset of the workspace failed");
  if (!rc) rc = sync(t);
  if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(IQLHIP_ERR_HIP, "building the weight copies failed");
  if (rc) {
    slab_destroy(t);
    return rc;
  }
  *out = t;
  return 0;
}

inline int slab_set_step(SlabTrainer *t, int64_t total_it) {
  if (!t || total_it < 0) return fail(IQLHIP_ERR_INVALID, "null trainer or negative step");
  t->total_it = total_it;
  return 0;
}

template <class T>
struct SlabGroup {
  int n = 0;
  T *member[IQLHIP_MAX_GROUP] = {};
  SlabQueueBound bound{T::QUEUE_STEPS};
};

// same(a, b): the two members can share a launch; `shared`: what that takes, for the message.
template <class G, class T, class Same>
int slab_group_create(G **out, T *const *members, int32_t n, Same &&same, const char *shared) {
  if (!out || !members) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n < 1 || n > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_UNSUPPORTED, "a group has 1..%d members (got %d)", IQLHIP_MAX_GROUP, n);
  for (int k = 0; k < n; ++k) {
    if (!members[k]) return fail(IQLHIP_ERR_INVALID, "member %d is null", k);
    if (!same(members[0]->s, members[k]->s))
      return fail(IQLHIP_ERR_INVALID, "member %d: the members of a group share %s", k, shared);
    for (int j = 0; j < k; ++j)
      if (members[j] == members[k]) return fail(IQLHIP_ERR_INVALID, "member %d appears twice", k);
  }
  G *g = new (std::nothrow) G;
  if (!g) return fail(IQLHIP_ERR_NOMEM, "out of host memory");
  g->n = n;
  for (int k = 0; k < n; ++k) g->member[k] = members[k];
  *out = g;
  return 0;
}

template <class G>
int slab_group_destroy(G *g) {
  if (!g) return 0;
  g->bound.release(true);
  delete g;
  return 0;
}

// The arguments of a train_steps call, before anything is launched: member k steps on views[k] by idx[k].
template <class T>
int slab_check_call(T *const *mem, int n, const iqlhip_replay_view *views, const int64_t *const *idx, int64_t n_steps,
                    const char *family) {
  if (!views || !idx) return fail(IQLHIP_ERR_INVALID, "null views or indices");
  if (n_steps < 0) return fail(IQLHIP_ERR_INVALID, "n_steps must be >= 0");
  for (int k = 0; k < n; ++k) {
    const auto &s = mem[k]->s;
    const iqlhip_replay_view &v = views[k];
    if (!idx[k]) return fail(IQLHIP_ERR_INVALID, "member %d: %s takes its indices from the caller", k, family);
    if (!v.rows || v.n_rows < 1) return fail(IQLHIP_ERR_INVALID, "member %d: empty replay view", k);
    if (v.state_dim != s.S || v.action_dim != s.A || v.row_stride != s.row_stride)
      return fail(IQLHIP_ERR_INVALID, "member %d: the replay view does not have the trainer's dims", k);
  }
  return 0;
}

// n_steps steps of the members mem[0..n): per_step(i) fills the step's coefficients and issues its launches on st.
template <class T, class PerStep>
int slab_run(T *const *mem, int n, SlabQueueBound &bound, int64_t n_steps, hipStream_t st, PerStep &&per_step) {
  for (int64_t i = 0; i < n_steps; ++i) {
    per_step(i);
    if (bound.due(i)) {
      HIP_TRY(hipGetLastError());
      if (int rc = bound.hold(st)) return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  for (int k = 0; k < n; ++k) mem[k]->total_it += n_steps;
  return 0;
}

}  // namespace iqlhip
