// numpy's legacy RandomState.randint(0, hi, size) on the device (algorithms/custom_offline/iql.py:277-284
// draws its replay indices with it), bit for bit, for up to IQLHIP_MAX_GROUP independent MT19937 states.
//
// What numpy does (random_bounded_uint64_fill with use_masked, mt19937_gen / mt19937_next32):
//   word():  if pos == 624 { twist the key; pos = 0 }  y = key[pos++], tempered.
//   value:   rng = hi - 1, mask = smallest 2^k - 1 >= rng; repeat v = word() & mask until v <= rng.
//   hi == 1 consumes no word and yields 0.  Consecutive calls are one stream, so n calls of B values
//   equal one call of n B values, and after the last value pos sits one past the word that gave it.
//
// One work-group of 256 lanes per stream, the key in LDS.  The twist of element i reads the NEW
// key[i - 227] for i >= 227 and key[623] reads the new key[0]; lane t < 227 therefore owns the chain
// of elements t, t + 227, t + 454 (t < 170), whose later links read exactly the values the same lane
// produced before -- the dependency never crosses a lane, and the twist costs one barrier (between
// reading the old key and storing the new one).  Element 623 recomputes the new key[0] from old words.
// Every round then tempers and masks the lane's three words, takes the block prefix count of the
// accept flags in index order (one 64-bit ballot + popcount per wave and segment, 3 x 4 counts in
// LDS) and stores the accepted values at their place in the output stream.  The round that reaches
// the last value stores only up to it and sets pos one past the word that produced it.
#include "../../include/iqlhip.h"
#include "common.h"

namespace iqlhip {

constexpr int MT_N = 624, MT_M = 397;
constexpr int MT_SEG = MT_N - MT_M;        // 227: lanes that own a chain
constexpr int MT_TAIL = MT_N - 2 * MT_SEG;  // 170: chains with a third element
constexpr int NP_THREADS = 256;
constexpr int NP_WAVES = NP_THREADS / 64;

struct NpDrawArgs {
  int64_t *out[IQLHIP_MAX_GROUP];
  uint32_t rng[IQLHIP_MAX_GROUP];   // hi - 1
  uint32_t mask[IQLHIP_MAX_GROUP];  // smallest 2^k - 1 >= rng
};

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

__global__ __launch_bounds__(NP_THREADS) void k_np_randint(uint32_t *__restrict__ state, NpDrawArgs a,
                                                            int64_t total) {
  __shared__ uint32_t key[MT_N];
  __shared__ int32_t cnt[2][3][NP_WAVES];  // accepted words per (round parity, segment, wave)
  const int k = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  uint32_t *st = state + (size_t)k * (MT_N + 1);
  int64_t *out = a.out[k];
  const uint32_t rng = a.rng[k], mask = a.mask[k];
  if (rng == 0) {  // hi == 1: zeros, no word consumed
    for (int64_t i = t; i < total; i += NP_THREADS) out[i] = 0;
    return;
  }
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
    if (a0 && pre[0] < need) out[done + pre[0]] = (int64_t)v0;
    if (a1 && pre[1] < need) out[done + pre[1]] = (int64_t)v1;
    if (a2 && pre[2] < need) out[done + pre[2]] = (int64_t)v2;
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

hipError_t launch_np_randint(uint32_t *state, const int64_t *hi, int K, int64_t total, int64_t *const *out,
                             hipStream_t st) {
  NpDrawArgs a = {};
  for (int k = 0; k < K; ++k) {
    const uint64_t rng = (uint64_t)(hi[k] - 1);
    uint64_t mask = rng;
    mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
    a.out[k] = out[k], a.rng[k] = (uint32_t)rng, a.mask[k] = (uint32_t)mask;
  }
  hipLaunchKernelGGL(k_np_randint, dim3(K), dim3(NP_THREADS), 0, st, state, a, total);
  return hipGetLastError();
}

}  // namespace iqlhip
