// numpy's legacy MT19937 word stream and its masked-rejection bounded draw, as one work-group of
// NP_THREADS lanes produces it (np_sampler.hip has the derivation).  Shared by k_np_randint (int64
// replay indices) and k_choice_draw (uint16 posterior indices, posterior_choice.hip), which both call
// np_draw_stream, and by k_np_randint_growing (online.hip), whose bound changes inside the stream: it runs the same
// np_twist / np_judge rounds, so the streams cannot drift apart.
#pragma once
#include "common.h"
#include "errors.h"

namespace iqlhip {

constexpr int MT_N = 624, MT_M = 397;
constexpr int MT_SEG = MT_N - MT_M;        // 227: lanes that own a chain
constexpr int MT_TAIL = MT_N - 2 * MT_SEG;  // 170: chains with a third element
constexpr int NP_THREADS = 256;
constexpr int NP_WAVES = NP_THREADS / 64;

// new key[i] from old key[i], key[i + 1] and key[i + 397 mod 624] (old or new, as the twist has it)
__device__ __forceinline__ uint32_t mt_mix(uint32_t ki, uint32_t ki1, uint32_t km) {
  const uint32_t y = (ki & 0x80000000u) | (ki1 & 0x7fffffffu);
  return km ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// The lane's share of one work-group of NP_THREADS lanes: lane t < 227 owns the chain of key elements t, t + 227 and
// (t < 170) t + 454, whose untempered words it keeps in registers.
struct NpLane {
  int wave, lane;
  bool own, own2;
  int e0, e1, e2;
  uint32_t w0, w1, w2;  // key[e0], key[e1], key[e2] (untempered)
  uint64_t below;       // the lanes of this wave before this one
};

// Load the state st = key[624], pos into LDS and registers; returns pos (checked to be <= 624 by the host).
__device__ __forceinline__ int np_lane_load(NpLane &L, const uint32_t *__restrict__ st, uint32_t *key) {
  const int t = threadIdx.x;
  L.wave = t >> 6, L.lane = t & 63;
  L.own = t < MT_SEG, L.own2 = t < MT_TAIL;
  L.e0 = t, L.e1 = t + MT_SEG, L.e2 = t + 2 * MT_SEG;
  L.w0 = L.w1 = L.w2 = 0;
  if (L.own) {
    L.w0 = st[L.e0], L.w1 = st[L.e1];
    key[L.e0] = L.w0, key[L.e1] = L.w1;
    if (L.own2) L.w2 = st[L.e2], key[L.e2] = L.w2;
  }
  L.below = L.lane ? (~0ull >> (64 - L.lane)) : 0ull;
  const int pos = (int)st[MT_N];
  __syncthreads();
  return pos;
}

__device__ __forceinline__ void np_lane_store(const NpLane &L, uint32_t *__restrict__ st) {
  if (L.own) {
    st[L.e0] = L.w0, st[L.e1] = L.w1;
    if (L.own2) st[L.e2] = L.w2;
  }
}

// twist: read the old key, one barrier, store the new one
__device__ __forceinline__ void np_twist(NpLane &L, uint32_t *key) {
  if (L.own) {
    const uint32_t n0 = mt_mix(L.w0, key[L.e0 + 1], key[L.e0 + MT_M]);
    const uint32_t n1 = mt_mix(L.w1, key[L.e1 + 1], n0);  // new key[e1 - 227] = n0
    if (L.own2) {
      const uint32_t nxt = L.e2 + 1 < MT_N ? key[L.e2 + 1] : mt_mix(key[0], key[1], key[MT_M]);  // new key[0]
      L.w2 = mt_mix(L.w2, nxt, n1);  // new key[e2 - 227] = n1
    }
    L.w0 = n0, L.w1 = n1;
  }
  __syncthreads();
  if (L.own) {
    key[L.e0] = L.w0, key[L.e1] = L.w1;
    if (L.own2) key[L.e2] = L.w2;
  }
}

// One judgement of the key's words from `pos` on under (rng, mask): which of the lane's three words are accepted
// (a*), their masked values (v*), the number of accepted words before each in stream order (pre*), and how many
// the whole key gave (got).  cnt: the [3][NP_WAVES] LDS counts of this judgement -- callers alternate between two
// of them, so that the next judgement's writes cannot pass this one's reads; one barrier.
struct NpJudged {
  bool a0, a1, a2;
  uint32_t v0, v1, v2;
  int pre0, pre1, pre2, got;
};

__device__ __forceinline__ NpJudged np_judge(const NpLane &L, int32_t (*cnt)[NP_WAVES], int pos, uint32_t rng,
                                             uint32_t mask) {
  NpJudged J;
  J.v0 = mt_temper(L.w0) & mask, J.v1 = mt_temper(L.w1) & mask, J.v2 = mt_temper(L.w2) & mask;
  J.a0 = L.own && L.e0 >= pos && J.v0 <= rng;
  J.a1 = L.own && L.e1 >= pos && J.v1 <= rng;
  J.a2 = L.own2 && L.e2 >= pos && J.v2 <= rng;
  const uint64_t b0 = __ballot(J.a0), b1 = __ballot(J.a1), b2 = __ballot(J.a2);
  if (L.lane == 0) {
    cnt[0][L.wave] = __popcll(b0);
    cnt[1][L.wave] = __popcll(b1);
    cnt[2][L.wave] = __popcll(b2);
  }
  __syncthreads();
  int seg[3], pre[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    int all = 0, lower = 0;
#pragma unroll
    for (int w = 0; w < NP_WAVES; ++w) {
      const int c = cnt[s][w];
      all += c;
      lower += w < L.wave ? c : 0;
    }
    seg[s] = all, pre[s] = lower;
  }
  J.pre0 = pre[0] + __popcll(b0 & L.below);
  J.pre1 = pre[1] + __popcll(b1 & L.below) + seg[0];
  J.pre2 = pre[2] + __popcll(b2 & L.below) + seg[0] + seg[1];
  J.got = seg[0] + seg[1] + seg[2];
  return J;
}

// `total` (>= 1) values of randint(0, rng + 1) from the state st = key[624], pos into out[0 .. total), in
// stream order, by the NP_THREADS lanes of one work-group; st is advanced in place (pos one past the
// word that gave the last value).  rng >= 1, mask = smallest 2^k - 1 >= rng, pos <= 624.
template <typename OutT>
__device__ __forceinline__ void np_draw_stream(uint32_t *__restrict__ st, OutT *__restrict__ out, uint32_t rng,
                                               uint32_t mask, int64_t total) {
  __shared__ uint32_t key[MT_N];
  __shared__ int32_t cnt[2][3][NP_WAVES];  // accepted words per (round parity, segment, wave)
  NpLane L;
  int pos = np_lane_load(L, st, key);
  int64_t done = 0;
  for (int par = 0;; par ^= 1) {
    if (pos >= MT_N) {
      np_twist(L, key);
      pos = 0;
    }
    const NpJudged J = np_judge(L, cnt[par], pos, rng, mask);
    const int64_t need = total - done;
    if (J.a0 && J.pre0 < need) out[done + J.pre0] = (OutT)J.v0;
    if (J.a1 && J.pre1 < need) out[done + J.pre1] = (OutT)J.v1;
    if (J.a2 && J.pre2 < need) out[done + J.pre2] = (OutT)J.v2;
    if (J.got < need) {  // every word of the key consumed
      done += J.got;
      pos = MT_N;
      continue;
    }
    // the need-th accepted word of this round gave the last value: pos one past it
    if (J.a0 && J.pre0 == need - 1) st[MT_N] = (uint32_t)(L.e0 + 1);
    if (J.a1 && J.pre1 == need - 1) st[MT_N] = (uint32_t)(L.e1 + 1);
    if (J.a2 && J.pre2 == need - 1) st[MT_N] = (uint32_t)(L.e2 + 1);
    break;
  }
  np_lane_store(L, st);
}

// smallest 2^k - 1 >= rng (numpy's mask of a bounded draw)
__host__ __device__ inline uint32_t np_mask_of(uint64_t rng) {
  uint64_t mask = rng;
  mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
  return (uint32_t)mask;
}

// Host, ahead of a draw from K states (iqlhip_np_randint, iqlhip_np_randint_growing): pos of every state in one
// strided copy of the K words, then the stream is synchronised; each must lie in 0..624.
inline int np_check_pos(const uint32_t *state, int K, hipStream_t st) {
  uint32_t pos[IQLHIP_MAX_GROUP];
  HIP_TRY(hipMemcpy2DAsync(pos, sizeof(uint32_t), state + 624, 625 * sizeof(uint32_t), sizeof(uint32_t), K,
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int k = 0; k < K; ++k)
    if (pos[k] > 624) return fail(IQLHIP_ERR_INVALID, "state %d: pos = %u outside 0..624", k, pos[k]);
  return 0;
}

}  // namespace iqlhip
