// Device-side dataset preparation: what the reference does in Python loops over
// the N transitions before training starts --
//   keep mask + episode step       ref:701-716 (= ref:1236-1253, 1127-1141, 938-951)
//   per-episode return range       ref:344-360  return_reward_range
//   reward normalisation           ref:363-401  modify_reward
//   state mean / std, z-scoring    ref:132-139, 1438-1448
// -- as HBM-bound integer / float kernels.  Everything here is one pass over N elements
// (N ~ 1e6): the kernels are simple and coalesced, none is worth more than that.
//
// Building block: an exclusive "index of the last flagged element" scan,
//   last[i] = max{ j < i : flag[j] }  (or -1),
// in two launches (per-chunk last index; then look-back over the chunk table + an in-chunk
// scan).  The episode-step counter and the episode segmentation are closed forms of it.
#include <cstring>

#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"

namespace iqlhip {

constexpr int CHUNK = 1024;  // elements per work-group of the scan (256 threads x 4)
constexpr int TRAJ_MAX_LEN = 1 << 20;  // iqlhip_prep_trajectory_returns: the longest trajectory cut (rows of `scale`)

// ---- flags -----------------------------------------------------------------
// Counter reset AFTER transition i (ref:708-716 with a timeouts array):
//   final and not terminate_on_end -> dropped, counter := 0          (kind 1)
//   else terminal or final          -> counter := 0 then += 1 -> 1   (kind 2)
//   else                            -> counter += 1                  (kind 0)
__device__ __forceinline__ int reset_kind(const uint8_t *term, const uint8_t *tmo, int64_t i, int toe) {
  const bool fin = tmo[i] != 0, done = term[i] != 0;
  if (fin && !toe) return 1;
  return (done || fin) ? 2 : 0;
}

template <int MODE>  // 0: reset flags of (terminals, timeouts); 1: terminals alone
__device__ __forceinline__ bool flag_at(const uint8_t *term, const uint8_t *tmo, int64_t i, int toe) {
  if constexpr (MODE == 0)
    return reset_kind(term, tmo, i, toe) != 0;
  else
    return term[i] != 0;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_chunk_last(const uint8_t *__restrict__ term,
                                                    const uint8_t *__restrict__ tmo, int64_t n, int toe,
                                                    int64_t *__restrict__ chunk_last) {
  __shared__ long long red[4];
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 4;
  long long best = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < n && flag_at<MODE>(term, tmo, base + k, toe)) best = base + k;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(best, off);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long b = red[0];
    for (int w = 1; w < 4; ++w) b = red[w] > b ? red[w] : b;
    chunk_last[blockIdx.x] = b;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_last_scan(const uint8_t *__restrict__ term,
                                                   const uint8_t *__restrict__ tmo, int64_t n, int toe,
                                                   const int64_t *__restrict__ chunk_last,
                                                   int64_t *__restrict__ last) {
  __shared__ long long carry_s;
  __shared__ long long wave_last[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {  // look back over the chunk table (resets are at most an episode apart)
    long long c = -1;
    for (int64_t b = (int64_t)blockIdx.x - 1; b >= 0 && c < 0; --b) c = chunk_last[b];
    carry_s = c;
  }
  const int64_t base = (int64_t)blockIdx.x * CHUNK + tid * 4;
  long long own[4], run = -1;  // own[k]: last flagged index among this thread's elements < k
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    own[k] = run;
    if (base + k < n && flag_at<MODE>(term, tmo, base + k, toe)) run = base + k;
  }
  // inclusive max-scan of `run` over the wave, then over the 4 waves
  long long inc = run;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long o = __shfl_up(inc, off);
    if (lane >= off) inc = o > inc ? o : inc;
  }
  if (lane == 63) wave_last[wave] = inc;
  __syncthreads();
  long long before = carry_s;  // everything before this thread: carry, earlier waves, earlier lanes
  for (int w = 0; w < wave; ++w) before = wave_last[w] > before ? wave_last[w] : before;
  const long long prev_lane = __shfl_up(inc, 1);
  if (lane > 0) before = prev_lane > before ? prev_lane : before;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < n) last[base + k] = own[k] > before ? own[k] : before;
}

// ---- keep mask / episode step, timeouts present ---------------------------------
// ep_steps[i] = value of the counter when transition i is visited; `last` = index of the last
// reset before i.  (tests: bit-exact against the reference loop)
__global__ void k_keep_steps(const uint8_t *__restrict__ term, const uint8_t *__restrict__ tmo, int64_t n1,
                             int toe, const int64_t *__restrict__ last, uint8_t *__restrict__ keep,
                             int64_t *__restrict__ ep_steps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  const int64_t l = last[i];
  int64_t ep;
  if (l < 0)
    ep = i;  // never reset: one increment per earlier transition
  else
    ep = (i - 1 - l) + (reset_kind(term, tmo, l, toe) == 2 ? 1 : 0);
  ep_steps[i] = ep;
  keep[i] = (tmo[i] != 0 && !toe) ? 0 : 1;
}

// ---- keep mask / episode step, no timeouts: final = (counter == M - 1) -------------
// The counter feeds back into the reset condition, so the scan above does not apply.  One wave
// walks the array 64 transitions at a time: inside a terminal-free run that starts at index a
// with counter c the value at a + t is a closed form (ramp, then a sawtooth of period M - base);
// terminals (found with a ballot) start a new run.  This path is the fallback for datasets
// without a timeouts array (every D4RL v2 file has one).
__global__ __launch_bounds__(64) void k_keep_steps_counter(const uint8_t *__restrict__ term, int64_t n1,
                                                          int64_t M, int toe, uint8_t *__restrict__ keep,
                                                          int64_t *__restrict__ ep_steps) {
  const int lane = threadIdx.x;
  const int64_t base = toe ? 1 : 0;  // counter after a `final` transition
  int64_t a = 0, c = 0;              // current run: starts at index a with counter c
  auto value = [&](int64_t i) -> int64_t {
    const int64_t t = i - a;
    if (c > M - 1) return c + t;               // already past M - 1: never final again in this run
    const int64_t f0 = M - 1 - c;              // offset of the run's first final transition
    if (t <= f0) return c + t;
    if (base <= M - 1) return (t - f0 - 1) % (M - base) + base;
    return base + (t - f0 - 1);                // M == 1 with terminate_on_end
  };
  for (int64_t p = 0; p < n1; p += 64) {
    const int64_t i = p + lane;
    const bool in = i < n1;
    const bool tm = in && term[i] != 0;
    unsigned long long pending = __ballot(tm);
    int64_t v = in ? value(i) : 0;
    while (pending) {  // terminals of this group, in order: each one ends the current run
      const int L = __ffsll((long long)pending) - 1;
      pending &= pending - 1;
      const int64_t vt = __shfl(v, L);  // counter at the terminal (wave-uniform)
      a = p + L + 1;
      c = (vt == M - 1) ? base : 1;     // final there -> base, else a kept terminal -> 1
      if (lane > L && in) v = value(i);
    }
    if (in) {
      ep_steps[i] = v;
      keep[i] = (v == M - 1 && !toe) ? 0 : 1;
    }
  }
}

// ---- per-episode returns (ref:344-360) ------------------------------------------
// An episode ends at a terminal or after M transitions (counted from the previous episode's
// end).  `last` = index of the last terminal before i, so i starts an episode iff
// (i - last - 1) % M == 0.  The thread of every episode start walks its episode in order and
// adds float(r) in double exactly as the reference loop does -> the sums are bit-identical.
// trj_lens[i] = length of i's episode (the trailing partial episode: its length so far).
__device__ __forceinline__ unsigned long long dbl_key(double x) {  // order-preserving integer image
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__global__ void k_episode_walk(const float *__restrict__ rew, const uint8_t *__restrict__ term, int64_t n,
                               int64_t M, const int64_t *__restrict__ last, double *__restrict__ trj_lens,
                               unsigned long long *__restrict__ minmax_key, int64_t *__restrict__ n_complete) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if ((i - last[i] - 1) % M != 0) return;
  double ret = 0.0;
  int64_t j = i, len = 0;
  bool complete = false;
  while (j < n) {
    ret += (double)rew[j];
    ++len;
    const bool d = term[j] != 0;
    ++j;
    if (d || len == M) {
      complete = true;
      break;
    }
  }
  for (int64_t k = i; k < j; ++k) trj_lens[k] = (double)len;
  if (complete) {
    const unsigned long long key = dbl_key(ret);
    atomicMin(minmax_key, key);  // min / max are order independent: deterministic
    atomicMax(minmax_key + 1, key);
    atomicAdd((unsigned long long *)n_complete, 1ull);
  }
}

// ---- any-percent selection (algorithms/offline/any_percent_bc.py:206-239 keep_best_trajectories) ----
// A trajectory ends at a terminal or at M rows, the rule of k_episode_walk above: with `last` = index of the
// last terminal before i, row i starts one iff (i - last - 1) % M == 0.  Its number in dataset order is the
// count of starts before it (only the trailing run can be incomplete, and nothing follows that one): an
// exclusive sum of the start flags -- per-chunk counts, one block that scans the chunk table, and the in-chunk
// scan fused into the walk.  The walker of a start adds float32(scale[k] * r) in float32 in row order, each
// product and each sum rounded on its own: numpy's `cur_return += reward_scale * reward` on float32 rewards.
// c + fp32(s * r): what __fadd_rn(c, __fmul_rn(s, r)) says.  HIP defines those two as plain `+` and `*`, which
// the compiler's default contraction fuses into one fma across the inlined calls; the pragma keeps the product's
// own rounding (by hand: k_traj_walk's code has v_mul_f32 / v_add_f32 here and no fma).
__device__ __forceinline__ float add_rounded_product(float c, float s, float r) {
#pragma clang fp contract(off)
  const float p = s * r;
  return c + p;
}

__device__ __forceinline__ bool traj_start(const int64_t *last, int64_t i, int64_t M) {
  return (i - last[i] - 1) % M == 0;
}

__global__ __launch_bounds__(256) void k_start_count(const int64_t *__restrict__ last, int64_t n, int64_t M,
                                                     int64_t *__restrict__ chunk_starts) {
  __shared__ int red[4];
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 4;
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < n && traj_start(last, base + k, M)) ++c;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunk_starts[blockIdx.x] = (int64_t)red[0] + red[1] + red[2] + red[3];
}

// one block: chunk_starts[b] := sum of the entries before b
__global__ __launch_bounds__(256) void k_chunk_offsets(int64_t *__restrict__ chunk_starts, int nchunk) {
  __shared__ long long wave_sum[4];
  __shared__ long long carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nchunk; b0 += 256) {
    const int b = b0 + tid;
    const long long v = b < nchunk ? chunk_starts[b] : 0;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long o = __shfl_up(inc, off);
      if (lane >= off) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    long long before = carry_s;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (b < nchunk) chunk_starts[b] = before + inc - v;
    __syncthreads();
    if (tid == 255) carry_s = before + inc;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_traj_walk(const float *__restrict__ rew, const uint8_t *__restrict__ term,
                                                   int64_t n, int64_t M, const float *__restrict__ scale,
                                                   const int64_t *__restrict__ last,
                                                   const int64_t *__restrict__ chunk_off, int64_t *__restrict__ starts,
                                                   int64_t *__restrict__ lengths, float *__restrict__ returns,
                                                   int64_t *__restrict__ n_traj) {
  __shared__ int wave_sum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * CHUNK + tid * 4;
  bool f[4];
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[k] = base + k < n && traj_start(last, base + k, M);
    cnt += f[k] ? 1 : 0;
  }
  int inc = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int64_t rank = chunk_off[blockIdx.x] + (inc - cnt);
  for (int w = 0; w < wave; ++w) rank += wave_sum[w];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!f[k]) continue;
    const int64_t i = base + k;
    float c = 0.f;
    int64_t j = i, len = 0;
    bool complete = false;
    while (j < n) {
      c = add_rounded_product(c, scale[len], rew[j]);
      ++len;
      const bool d = term[j] != 0;
      ++j;
      if (d || len == M) {
        complete = true;
        break;
      }
    }
    if (complete) starts[rank] = i, lengths[rank] = len, returns[rank] = c;
    if (j == n) *n_traj = complete ? rank + 1 : rank;  // the one walker that reaches the end of the data
    ++rank;
  }
}

// dst rows [dst_off[j], dst_off[j] + lengths[c]) := src rows [starts[c], ...), c = chosen[j]: one block column per
// chosen trajectory, gridDim.y blocks share its len * width contiguous floats.  float4 pieces when both ends are
// on 16-byte boundaries, floats otherwise and for the tail.  An entry that does not fit (c outside [0, n_traj), rows
// outside src or dst) is skipped: nothing is read or written for it.
__global__ __launch_bounds__(256) void k_gather_traj(const float *__restrict__ src, int64_t n, int width,
                                                     const int64_t *__restrict__ starts,
                                                     const int64_t *__restrict__ lengths, int64_t n_traj,
                                                     const int64_t *__restrict__ chosen,
                                                     const int64_t *__restrict__ dst_off, int64_t total_rows,
                                                     float *__restrict__ dst) {
  const int64_t c = chosen[blockIdx.x];
  if (c < 0 || c >= n_traj) return;
  const int64_t s = starts[c], len = lengths[c], o = dst_off[blockIdx.x];
  if (s < 0 || len < 1 || len > n - s || o < 0 || len > total_rows - o) return;
  const float *from = src + s * width;
  float *to = dst + o * width;
  const int64_t count = len * width;
  const int64_t t0 = (int64_t)blockIdx.y * 256 + threadIdx.x, stride = (int64_t)gridDim.y * 256;
  if ((((uintptr_t)from | (uintptr_t)to) & 15) == 0) {
    const int64_t n4 = count >> 2;
    for (int64_t q = t0; q < n4; q += stride)
      reinterpret_cast<float4 *>(to)[q] = reinterpret_cast<const float4 *>(from)[q];
    for (int64_t e = (n4 << 2) + t0; e < count; e += stride) to[e] = from[e];
  } else {
    for (int64_t e = t0; e < count; e += stride) to[e] = from[e];
  }
}

// ---- reward normalisation (ref:363-401), numpy's in-place float32 semantics --------
//   rewards op= python scalar  -> the scalar is rounded to float32, the op runs in float32
//   rewards -= float64 array   -> the op runs in float64, the result is rounded to float32
struct RewardOps {
  int32_t sub_first;    // 0 none, 1 `-= min_ret` (float32), 2 `-= min_ret / trj_lens` (float64)
  int32_t scale;        // `/= (max_ret - min_ret)` then `*= max_episode_steps`
  int32_t sub_one;      // `-= 1.0`
  double min_ret, range;
  float steps;
};
__global__ void k_modify_reward(float *__restrict__ rew, int64_t n, const double *__restrict__ trj_lens,
                                RewardOps op) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r = rew[i];
  if (op.sub_first == 1) r = r - (float)op.min_ret;
  if (op.sub_first == 2) r = (float)((double)r - op.min_ret / trj_lens[i]);
  if (op.scale) {
    r = r / (float)op.range;
    r = r * op.steps;
  }
  if (op.sub_one) r = r - 1.0f;
  rew[i] = r;
}

// ---- state statistics (ref:132-135): column mean and std in double, fixed order ------
// pass 1: per-block column sums; pass 2 (host-launched again with the mean): squared deviations.
// Partial sums of a column are added in block order by one thread: run-to-run deterministic.
constexpr int STAT_ROWS = 2048;  // rows per block
__global__ __launch_bounds__(256) void k_col_partial(const float *__restrict__ x, int64_t n, int S,
                                                     const double *__restrict__ mean,  // null: plain sums
                                                     double *__restrict__ partial) {
  // thread t handles column t % S for rows r0 + t / S, stepping by 256 / S rows (S <= 256)
  const int per = 256 / S;
  const int col = threadIdx.x % S, sub = threadIdx.x / S;
  __shared__ double acc[256];
  double s = 0.0;
  if (sub < per) {
    const int64_t r0 = (int64_t)blockIdx.x * STAT_ROWS;
    const int64_t r1 = r0 + STAT_ROWS < n ? r0 + STAT_ROWS : n;
    const double m = mean ? mean[col] : 0.0;
    for (int64_t r = r0 + sub; r < r1; r += per) {
      const double v = (double)x[r * S + col] - m;
      s += mean ? v * v : v;
    }
  }
  acc[threadIdx.x] = s;
  __syncthreads();
  if (sub == 0) {
    double t = 0.0;
    for (int k = 0; k < per; ++k) t += acc[k * S + col];
    partial[(size_t)blockIdx.x * S + col] = t;
  }
}
__global__ void k_col_final(const double *__restrict__ partial, int nblk, int S, int64_t n, int pass,
                            double eps, double *__restrict__ mean, float *__restrict__ mean_f,
                            float *__restrict__ std_f) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= S) return;
  double t = 0.0;
  for (int b = 0; b < nblk; ++b) t += partial[(size_t)b * S + col];
  if (pass == 0) {
    mean[col] = t / (double)n;
    mean_f[col] = (float)(t / (double)n);
  } else {
    std_f[col] = (float)(sqrt(t / (double)n) + eps);  // states.std(0) + eps
  }
}

// ---- pack with fused z-scoring (ref:1438-1456): rows = [ (s-m)/sd | a | r | d | (s'-m)/sd ] ---
__global__ void k_pack_norm(float *__restrict__ rows, int stride, int S, int A, int64_t first, int64_t n,
                            const float *__restrict__ obs, const float *__restrict__ act,
                            const float *__restrict__ rew, const float *__restrict__ nxt,
                            const float *__restrict__ done, const float *__restrict__ mean,
                            const float *__restrict__ sd) {
  const int NO = round_up(S + A + 2, 4), W = NO + S;  // s' starts on a 16-byte boundary
  const int64_t total = n * (int64_t)stride;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e / stride;
    const int c = (int)(e - row * stride);
    float v = 0.f;
    if (c < S)
      v = (obs[row * S + c] - mean[c]) / sd[c];
    else if (c < S + A)
      v = act[row * A + (c - S)];
    else if (c == S + A)
      v = rew[row];
    else if (c == S + A + 1)
      v = done[row];
    else if (c >= NO && c < W)
      v = (nxt[row * S + (c - NO)] - mean[c - NO]) / sd[c - NO];
    rows[(first + row) * stride + c] = v;
  }
}

// ------------------------------------------------------------------ launchers --
template <int MODE>
static hipError_t last_flag_scan(const uint8_t *term, const uint8_t *tmo, int64_t n, int toe, int64_t *last,
                                 hipStream_t st) {
  const int nchunk = (int)((n + CHUNK - 1) / CHUNK);
  int64_t *chunk_last = nullptr;
  hipError_t e = hipMallocAsync((void **)&chunk_last, sizeof(int64_t) * nchunk, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_chunk_last<MODE>, dim3(nchunk), dim3(256), 0, st, term, tmo, n, toe, chunk_last);
  hipLaunchKernelGGL(k_last_scan<MODE>, dim3(nchunk), dim3(256), 0, st, term, tmo, n, toe, chunk_last, last);
  e = hipGetLastError();
  (void)hipFreeAsync(chunk_last, st);
  return e;
}

static hipError_t launch_keep_steps(const uint8_t *term, const uint8_t *tmo, int64_t n, int64_t M, int toe,
                                    uint8_t *keep, int64_t *ep_steps, hipStream_t st) {
  const int64_t n1 = n - 1;
  if (n1 <= 0) return hipSuccess;
  if (!tmo) {
    hipLaunchKernelGGL(k_keep_steps_counter, dim3(1), dim3(64), 0, st, term, n1, M, toe, keep, ep_steps);
    return hipGetLastError();
  }
  int64_t *last = nullptr;
  hipError_t e = hipMallocAsync((void **)&last, sizeof(int64_t) * n1, st);
  if (e != hipSuccess) return e;
  e = last_flag_scan<0>(term, tmo, n1, toe, last, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_keep_steps, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, term, tmo, n1, toe,
                       last, keep, ep_steps);
    e = hipGetLastError();
  }
  (void)hipFreeAsync(last, st);
  return e;
}

// out[0] = min return, out[1] = max return (doubles), out[2] = number of complete episodes
static hipError_t launch_reward_range(const float *rew, const uint8_t *term, int64_t n, int64_t M, double *trj_lens,
                                      double *out3, hipStream_t st) {
  int64_t *last = nullptr;
  unsigned long long *keys = nullptr;  // [0] min key, [1] max key, [2] count
  hipError_t e = hipMallocAsync((void **)&last, sizeof(int64_t) * n, st);
  if (e != hipSuccess) return e;
  e = hipMallocAsync((void **)&keys, 3 * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const unsigned long long init[3] = {~0ull, 0ull, 0ull};
  e = hipMemcpyAsync(keys, init, sizeof(init), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = last_flag_scan<1>(term, nullptr, n, 0, last, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_episode_walk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rew, term, n, M,
                       last, trj_lens, keys, reinterpret_cast<int64_t *>(keys + 2));
    e = hipGetLastError();
  }
  unsigned long long h[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(h, keys, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFreeAsync(last, st);
  (void)hipFreeAsync(keys, st);
  if (e != hipSuccess) return e;
  auto unkey = [](unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double d;
    memcpy(&d, &u, 8);
    return d;
  };
  out3[0] = unkey(h[0]), out3[1] = unkey(h[1]), out3[2] = (double)h[2];
  return hipSuccess;
}

// *n_traj_host = number of complete trajectories; starts / lengths / returns are written for those only
static hipError_t launch_trajectory_returns(const float *rew, const uint8_t *term, int64_t n, int64_t M,
                                            const float *scale, int64_t *starts, int64_t *lengths, float *returns,
                                            int64_t *n_traj_host, hipStream_t st) {
  const int nchunk = (int)((n + CHUNK - 1) / CHUNK);
  int64_t *last = nullptr, *table = nullptr;  // table: [nchunk] start counts -> offsets, [nchunk] = the count
  hipError_t e = hipMallocAsync((void **)&last, sizeof(int64_t) * n, st);
  if (e != hipSuccess) return e;
  e = hipMallocAsync((void **)&table, sizeof(int64_t) * ((size_t)nchunk + 1), st);
  if (e != hipSuccess) {
    (void)hipFreeAsync(last, st);
    return e;
  }
  e = last_flag_scan<1>(term, nullptr, n, 0, last, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_start_count, dim3(nchunk), dim3(256), 0, st, last, n, M, table);
    hipLaunchKernelGGL(k_chunk_offsets, dim3(1), dim3(256), 0, st, table, nchunk);
    hipLaunchKernelGGL(k_traj_walk, dim3(nchunk), dim3(256), 0, st, rew, term, n, M, scale, last, table, starts,
                       lengths, returns, table + nchunk);
    e = hipGetLastError();
  }
  int64_t h = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&h, table + nchunk, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFreeAsync(last, st);
  (void)hipFreeAsync(table, st);
  if (e == hipSuccess) *n_traj_host = h;
  return e;
}

static hipError_t launch_state_stats(const float *x, int64_t n, int S, double eps, float *mean_f, float *std_f,
                                     hipStream_t st) {
  const int nblk = (int)((n + STAT_ROWS - 1) / STAT_ROWS);
  double *partial = nullptr, *mean = nullptr;
  hipError_t e = hipMallocAsync((void **)&partial, sizeof(double) * (size_t)nblk * S, st);
  if (e != hipSuccess) return e;
  e = hipMallocAsync((void **)&mean, sizeof(double) * S, st);
  if (e != hipSuccess) return e;
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(k_col_partial, dim3(nblk), dim3(256), 0, st, x, n, S, pass ? mean : nullptr, partial);
    hipLaunchKernelGGL(k_col_final, dim3((S + 63) / 64), dim3(64), 0, st, partial, nblk, S, n, pass, eps, mean,
                       mean_f, std_f);
  }
  e = hipGetLastError();
  (void)hipFreeAsync(partial, st);
  (void)hipFreeAsync(mean, st);
  return e;
}

}  // namespace iqlhip

using namespace iqlhip;

// ------------------------------------------------------------ entry points --
extern "C" int iqlhip_prep_keep_mask(const uint8_t *terminals, const uint8_t *timeouts, int64_t n,
                                     int32_t max_episode_steps, int32_t terminate_on_end, uint8_t *keep,
                                     int64_t *ep_steps, void *stream) {
  if (!terminals || !keep || !ep_steps) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (n < 1) return fail(IQLHIP_ERR_INVALID, "n must be >= 1");
  if (!timeouts && max_episode_steps < 1) return fail(IQLHIP_ERR_INVALID, "max_episode_steps must be >= 1");
  HIP_TRY(launch_keep_steps(terminals, timeouts, n, max_episode_steps, terminate_on_end != 0, keep, ep_steps,
                            (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_prep_reward_range(const float *rewards, const uint8_t *terminals, int64_t n,
                                        int32_t max_episode_steps, double *trj_lens, double *min_ret,
                                        double *max_ret, void *stream) {
  if (!rewards || !terminals || !trj_lens || !min_ret || !max_ret) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (n < 1 || max_episode_steps < 1) return fail(IQLHIP_ERR_INVALID, "n and max_episode_steps must be >= 1");
  double out3[3];
  HIP_TRY(launch_reward_range(rewards, terminals, n, max_episode_steps, trj_lens, out3, (hipStream_t)stream));
  if (out3[2] == 0.0) return fail(IQLHIP_ERR_INVALID, "dataset holds no complete episode");
  *min_ret = out3[0], *max_ret = out3[1];
  return 0;
}

extern "C" int iqlhip_prep_modify_reward(float *rewards, int64_t n, const double *trj_lens, int32_t sub_first,
                                         int32_t scale, int32_t sub_one, double min_ret, double max_ret,
                                         int32_t max_episode_steps, void *stream) {
  if (!rewards) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (sub_first < 0 || sub_first > 2) return fail(IQLHIP_ERR_INVALID, "sub_first must be 0, 1 or 2");
  if (sub_first == 2 && !trj_lens) return fail(IQLHIP_ERR_INVALID, "sub_first = 2 needs trj_lens");
  if (n <= 0) return 0;
  RewardOps op;
  op.sub_first = sub_first, op.scale = scale != 0, op.sub_one = sub_one != 0;
  op.min_ret = min_ret, op.range = max_ret - min_ret, op.steps = (float)max_episode_steps;
  hipLaunchKernelGGL(k_modify_reward, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards, n,
                     trj_lens, op);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_prep_state_stats(const float *obs, int64_t n, int32_t state_dim, double eps, float *mean,
                                       float *std, void *stream) {
  if (!obs || !mean || !std) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (n < 1 || state_dim < 1 || state_dim > 256) return fail(IQLHIP_ERR_UNSUPPORTED, "n >= 1, 1 <= state_dim <= 256");
  HIP_TRY(launch_state_stats(obs, n, state_dim, eps, mean, std, (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_replay_pack_normalized(float *rows, int32_t row_stride, int32_t S, int32_t A,
                                             int64_t first_row, int64_t n, const float *obs, const float *act,
                                             const float *rew, const float *next_obs, const float *done,
                                             const float *mean, const float *std, void *stream) {
  if (!rows || !obs || !act || !rew || !next_obs || !done || !mean || !std)
    return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (S <= 0 || A <= 0 || n < 0 || first_row < 0 || row_stride < iqlhip_replay_row_stride(S, A) || (row_stride & 3))
    return fail(IQLHIP_ERR_INVALID, "bad replay geometry S=%d A=%d stride=%d", S, A, row_stride);
  if (n == 0) return 0;
  const int64_t total = n * (int64_t)row_stride;
  int grid = (int)((total + 255) / 256);
  if (grid > 256 * 8) grid = 256 * 8;
  hipLaunchKernelGGL(k_pack_norm, dim3(grid), dim3(256), 0, (hipStream_t)stream, rows, row_stride, S, A, first_row, n,
                     obs, act, rew, next_obs, done, mean, std);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_prep_trajectory_returns(const float *rewards, const uint8_t *terminals, int64_t n,
                                              int32_t max_len, const float *scale, int64_t *starts,
                                              int64_t *lengths, float *returns, int64_t *n_traj, void *stream) {
  if (!rewards || !terminals || !scale || !starts || !lengths || !returns || !n_traj)
    return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (n < 1 || max_len < 1) return fail(IQLHIP_ERR_INVALID, "n and max_len must be >= 1");
  if (max_len > TRAJ_MAX_LEN)
    return fail(IQLHIP_ERR_UNSUPPORTED, "max_len %d is beyond %d", max_len, TRAJ_MAX_LEN);
  int64_t count = 0;
  HIP_TRY(launch_trajectory_returns(rewards, terminals, n, max_len, scale, starts, lengths, returns, &count,
                                    (hipStream_t)stream));
  if (count == 0) return fail(IQLHIP_ERR_INVALID, "dataset holds no complete trajectory");
  *n_traj = count;
  return 0;
}

extern "C" int iqlhip_prep_gather_trajectories(const float *src, int64_t n, int32_t width, const int64_t *starts,
                                               const int64_t *lengths, int64_t n_traj, const int64_t *chosen,
                                               const int64_t *dst_offsets, int64_t m, int64_t total_rows, float *dst,
                                               void *stream) {
  if (!src || !starts || !lengths || !chosen || !dst_offsets || !dst) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (n < 1 || width < 1 || n_traj < 1 || n_traj > n)
    return fail(IQLHIP_ERR_INVALID, "n >= 1, width >= 1, 1 <= n_traj <= n");
  if (m < 1 || m > n_traj || m > 0x7fffffff || total_rows < m || total_rows > n)
    return fail(IQLHIP_ERR_INVALID, "1 <= m <= n_traj, m <= total_rows <= n");
  // blocks per trajectory: about 4096 floats each at the mean trajectory length, 1 .. 16
  int64_t split = (total_rows / m) * width / 4096;
  split = split < 1 ? 1 : (split > 16 ? 16 : split);
  hipLaunchKernelGGL(k_gather_traj, dim3((unsigned)m, (unsigned)split), dim3(256), 0, (hipStream_t)stream, src, n,
                     (int)width, starts, lengths, n_traj, chosen, dst_offsets, total_rows, dst);
  HIP_TRY(hipGetLastError());
  return 0;
}
