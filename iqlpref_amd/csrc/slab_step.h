// The slab-step core: what the behaviour-cloning step (bc_step.hip) and the AWAC step (awac_step.hip) are both
// made of.  A training step of this kind is
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
// The two families differ on purpose in three pieces of arithmetic; each is a compile-time policy here, never a
// merged formula ("The slab-step core"):
//   MFMA accumulation        OneChain (BC)           | FourChains (AWAC: four chains added pairwise)
//   bias-gradient batch sum  SumFloat (BC)           | SumDouble (AWAC)
//   Adam                     the `adam` callable: adam_apply<false> (BC) | second moment in double (AWAC)
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
