// numpy's legacy MT19937 word stream and its masked-rejection bounded draw, as one work-group of
// NP_THREADS lanes produces it (np_sampler.hip has the derivation).  Shared by k_np_randint (int64
// replay indices) and k_choice_draw (uint16 posterior indices, posterior_choice.hip): both call
// np_draw_stream, so the two streams cannot drift apart.
#pragma once
#include "common.h"

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

// `total` (>= 1) values of randint(0, rng + 1) from the state st = key[624], pos into out[0 .. total), in
// stream order, by the NP_THREADS lanes of one work-group; st is advanced in place (pos one past the
// word that gave the last value).  rng >= 1, mask = smallest 2^k - 1 >= rng, pos <= 624.
template <typename OutT>
__device__ __forceinline__ void np_draw_stream(uint32_t *__restrict__ st, OutT *__restrict__ out, uint32_t rng,
                                               uint32_t mask, int64_t total) {
  __shared__ uint32_t key[MT_N];
  __shared__ int32_t cnt[2][3][NP_WAVES];  // accepted words per (round parity, segment, wave)
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const bool own = t < MT_SEG, own2 = t < MT_TAIL;
  const int e0 = t, e1 = t + MT_SEG, e2 = t + 2 * MT_SEG;
  uint32_t w0 = 0, w1 = 0, w2 = 0;  // key[e0], key[e1], key[e2] (untempered)
  if (own) {
    w0 = st[e0], w1 = st[e1];
    key[e0] = w0, key[e1] = w1;
    if (own2) w2 = st[e2], key[e2] = w2;
  }
  int pos = (int)st[MT_N];  // (checked to be <= 624 by the host)
  __syncthreads();
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int64_t done = 0;
  for (int par = 0;; par ^= 1) {
    if (pos >= MT_N) {  // twist: read the old key, one barrier, store the new one
      if (own) {
        const uint32_t n0 = mt_mix(w0, key[e0 + 1], key[e0 + MT_M]);
        const uint32_t n1 = mt_mix(w1, key[e1 + 1], n0);  // new key[e1 - 227] = n0
        if (own2) {
          const uint32_t nxt = e2 + 1 < MT_N ? key[e2 + 1] : mt_mix(key[0], key[1], key[MT_M]);  // new key[0]
          w2 = mt_mix(w2, nxt, n1);  // new key[e2 - 227] = n1
        }
        w0 = n0, w1 = n1;
      }
      __syncthreads();
      if (own) {
        key[e0] = w0, key[e1] = w1;
        if (own2) key[e2] = w2;
      }
      pos = 0;
    }
    const uint32_t v0 = mt_temper(w0) & mask, v1 = mt_temper(w1) & mask, v2 = mt_temper(w2) & mask;
    const bool a0 = own && e0 >= pos && v0 <= rng;
    const bool a1 = own && e1 >= pos && v1 <= rng;
    const bool a2 = own2 && e2 >= pos && v2 <= rng;
    const uint64_t b0 = __ballot(a0), b1 = __ballot(a1), b2 = __ballot(a2);
    if (lane == 0) {
      cnt[par][0][wave] = __popcll(b0);
      cnt[par][1][wave] = __popcll(b1);
      cnt[par][2][wave] = __popcll(b2);
    }
    __syncthreads();
    int seg[3], pre[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      int all = 0, lower = 0;
#pragma unroll
      for (int w = 0; w < NP_WAVES; ++w) {
        const int c = cnt[par][s][w];
        all += c;
        lower += w < wave ? c : 0;
      }
      seg[s] = all, pre[s] = lower;
    }
    pre[0] += __popcll(b0 & below);
    pre[1] += __popcll(b1 & below) + seg[0];
    pre[2] += __popcll(b2 & below) + seg[0] + seg[1];
    const int64_t need = total - done, got = seg[0] + seg[1] + seg[2];
    if (a0 && pre[0] < need) out[done + pre[0]] = (OutT)v0;
    if (a1 && pre[1] < need) out[done + pre[1]] = (OutT)v1;
    if (a2 && pre[2] < need) out[done + pre[2]] = (OutT)v2;
    if (got < need) {  // every word of the key consumed
      done += got;
      pos = MT_N;
      continue;
    }
    // the need-th accepted word of this round gave the last value: pos one past it
    if (a0 && pre[0] == need - 1) st[MT_N] = (uint32_t)(e0 + 1);
    if (a1 && pre[1] == need - 1) st[MT_N] = (uint32_t)(e1 + 1);
    if (a2 && pre[2] == need - 1) st[MT_N] = (uint32_t)(e2 + 1);
    break;
  }
  if (own) {
    st[e0] = w0, st[e1] = w1;
    if (own2) st[e2] = w2;
  }
}

// smallest 2^k - 1 >= rng (numpy's mask of a bounded draw)
inline uint32_t np_mask_of(uint64_t rng) {
  uint64_t mask = rng;
  mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
  return (uint32_t)mask;
}

}  // namespace iqlhip
