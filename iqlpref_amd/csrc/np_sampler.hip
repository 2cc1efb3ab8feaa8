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
// The stream itself is np_draw_stream (np_stream.h), shared with the posterior-choice draw.
#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"
#include "np_stream.h"

namespace iqlhip {

struct NpDrawArgs {
  int64_t *out[IQLHIP_MAX_GROUP];
  uint32_t rng[IQLHIP_MAX_GROUP];   // hi - 1
  uint32_t mask[IQLHIP_MAX_GROUP];  // smallest 2^k - 1 >= rng
};

__global__ __launch_bounds__(NP_THREADS) void k_np_randint(uint32_t *__restrict__ state, NpDrawArgs a,
                                                            int64_t total) {
  const int k = blockIdx.x, t = threadIdx.x;
  int64_t *out = a.out[k];
  const uint32_t rng = a.rng[k];
  if (rng == 0) {  // hi == 1: zeros, no word consumed
    for (int64_t i = t; i < total; i += NP_THREADS) out[i] = 0;
    return;
  }
  np_draw_stream<int64_t>(state + (size_t)k * (MT_N + 1), out, rng, a.mask[k], total);
}

// The epoch walk of algorithms/custom_offline/iql_bb.py:208-238 (RandomBatchSampler under a BatchSampler):
// one permutation of the nb = N / B whole blocks, walked again every epoch of ceil(N / B) steps; the
// rows N % B left over are one short batch at the end of each epoch.  One thread per index; the entries
// of a short batch beyond its valid count point at the last row (they are gathered, never counted).
__global__ __launch_bounds__(256) void k_block_epoch(const int64_t *__restrict__ perm, int64_t N, int B, int64_t t0,
                                                      int64_t n_steps, int64_t *__restrict__ idx,
                                                      int32_t *__restrict__ n_valid) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_steps * B) return;
  const int64_t i = e / B, j = e - i * B;
  const int64_t nb = N / B, tail = N - nb * B, slots = nb + (tail ? 1 : 0);
  const int64_t slot = (t0 + i) % slots;
  int64_t row;
  if (slot < nb) {
    const int64_t p = perm[slot];
    row = (p < 0 ? 0 : (p >= nb ? nb - 1 : p)) * B + j;  // (a permutation of 0..nb-1 is the caller's to give)
  } else {
    row = nb * B + j;
    if (row > N - 1) row = N - 1;
  }
  idx[e] = row;
  if (j == 0) n_valid[i] = slot < nb ? B : (int32_t)tail;
}

// The same walk for the K members of a seed group in ONE launch: blockIdx.y = member, its permutation and its
// index array passed by value in the argument block (as NpDrawArgs).  All members walk the same N and B, so the
// valid-row counts are one array, written by member 0.
struct BlockEpochGroupArgs {
  const int64_t *perm[IQLHIP_MAX_GROUP];
  int64_t *idx[IQLHIP_MAX_GROUP];
};

__global__ __launch_bounds__(256) void k_block_epoch_group(BlockEpochGroupArgs a, int64_t N, int B, int64_t t0,
                                                            int64_t n_steps, int32_t *__restrict__ n_valid) {
  const int k = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_steps * B) return;
  const int64_t i = e / B, j = e - i * B;
  const int64_t nb = N / B, tail = N - nb * B, slots = nb + (tail ? 1 : 0);
  const int64_t slot = (t0 + i) % slots;
  int64_t row;
  if (slot < nb) {
    const int64_t p = a.perm[k][slot];
    row = (p < 0 ? 0 : (p >= nb ? nb - 1 : p)) * B + j;
  } else {
    row = nb * B + j;
    if (row > N - 1) row = N - 1;
  }
  a.idx[k][e] = row;
  if (k == 0 && j == 0) n_valid[i] = slot < nb ? B : (int32_t)tail;
}

}  // namespace iqlhip

using namespace iqlhip;

// ------------------------------------------------------- numpy index stream --
extern "C" int iqlhip_np_randint(uint32_t *state, const int64_t *hi, int32_t K, int32_t batch,
                                 int64_t n_batches, int64_t *const *out, void *stream) {
  if (!state || !hi || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (K < 1 || K > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "K = %d: 1..%d streams", K, IQLHIP_MAX_GROUP);
  if (batch < 1) return fail(IQLHIP_ERR_INVALID, "batch = %d must be >= 1", batch);
  if (n_batches < 0) return fail(IQLHIP_ERR_INVALID, "n_batches = %lld must be >= 0", (long long)n_batches);
  for (int k = 0; k < K; ++k) {
    if (hi[k] < 1 || hi[k] > (int64_t(1) << 32))
      return fail(IQLHIP_ERR_INVALID, "hi[%d] = %lld outside 1..2^32", k, (long long)hi[k]);
    if (!out[k]) return fail(IQLHIP_ERR_INVALID, "null out[%d]", k);
  }
  hipStream_t st = (hipStream_t)stream;
  if (int rc = np_check_pos(state, K, st)) return rc;
  if (n_batches == 0) return 0;
  NpDrawArgs a = {};
  for (int k = 0; k < K; ++k) {
    const uint64_t rng = (uint64_t)(hi[k] - 1);
    a.out[k] = out[k], a.rng[k] = (uint32_t)rng, a.mask[k] = np_mask_of(rng);
  }
  hipLaunchKernelGGL(k_np_randint, dim3(K), dim3(NP_THREADS), 0, st, state, a, n_batches * (int64_t)batch);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ------------------------------------------------------- block-shuffled epochs --
// what one walk and the walks of a group check alike
static int block_epoch_check(int32_t batch, int64_t n_rows, int64_t t0, int64_t n_steps) {
  if (batch < 1) return fail(IQLHIP_ERR_INVALID, "batch = %d must be >= 1", batch);
  if (n_rows < 1) return fail(IQLHIP_ERR_INVALID, "n_rows = %lld must be >= 1", (long long)n_rows);
  if (t0 < 0 || n_steps < 0)
    return fail(IQLHIP_ERR_INVALID, "t0 = %lld and n_steps = %lld must be >= 0", (long long)t0, (long long)n_steps);
  return 0;
}

extern "C" int iqlhip_block_epoch_indices(const int64_t *perm, int64_t n_rows, int32_t batch, int64_t t0,
                                          int64_t n_steps, int64_t *idx, int32_t *n_valid, void *stream) {
  if (!idx || !n_valid) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = block_epoch_check(batch, n_rows, t0, n_steps)) return rc;
  if (!perm && n_rows >= batch) return fail(IQLHIP_ERR_INVALID, "null perm with %lld whole blocks", (long long)(n_rows / batch));
  if (n_steps == 0) return 0;
  hipLaunchKernelGGL(k_block_epoch, dim3((unsigned)((n_steps * batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     perm, n_rows, batch, t0, n_steps, idx, n_valid);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_block_epoch_indices_group(const int64_t *const *perm, int64_t n_rows, int32_t batch, int64_t t0,
                                                int64_t n_steps, int64_t *const *idx, int32_t *n_valid, int32_t K,
                                                void *stream) {
  if (!idx || !n_valid) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (K < 1 || K > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "K = %d: 1..%d members", K, IQLHIP_MAX_GROUP);
  if (int rc = block_epoch_check(batch, n_rows, t0, n_steps)) return rc;
  for (int k = 0; k < K; ++k) {
    if (!idx[k]) return fail(IQLHIP_ERR_INVALID, "null idx[%d]", k);
    if ((!perm || !perm[k]) && n_rows >= batch)
      return fail(IQLHIP_ERR_INVALID, "null perm[%d] with %lld whole blocks", k, (long long)(n_rows / batch));
  }
  if (n_steps == 0) return 0;
  BlockEpochGroupArgs a = {};
  for (int k = 0; k < K; ++k) a.perm[k] = perm ? perm[k] : nullptr, a.idx[k] = idx[k];
  hipLaunchKernelGGL(k_block_epoch_group, dim3((unsigned)((n_steps * batch + 255) / 256), K), dim3(256), 0,
                     (hipStream_t)stream, a, n_rows, batch, t0, n_steps, n_valid);
  HIP_TRY(hipGetLastError());
  return 0;
}
