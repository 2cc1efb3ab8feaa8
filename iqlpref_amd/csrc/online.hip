// The three kernels of the online phase of algorithms/finetune/iql.py ("fref"): every tick acts with
// exploration noise (fref:681-694), appends the transition to the replay ring (fref:164-180), samples
// from the grown buffer (fref:155-156) and takes one gradient step.  The step is the trainer's; what is
// here is what the tick needs around it, each kernel on its own:
//   k_replay_append       n transitions into the packed rows at (pointer + i) % capacity;
//   k_np_randint_growing  numpy's legacy randint for n_steps consecutive steps whose bound grows;
//   k_explore_epilogue    mean / output of the actor -> noisy, scaled, clamped action.
#include "../../include/iqlhip.h"
#include "common.h"
#include "np_stream.h"

namespace iqlhip {

// ------------------------------------------------------------------ append --
// One thread per 16-byte piece of a row (the stride is a multiple of 4 floats and the rows start on a
// 16-byte boundary): the same columns k_pack writes, padding zeros included, as one float4 store.
__global__ __launch_bounds__(256) void k_replay_append(float *__restrict__ rows, int stride, int S, int A,
                                                        int64_t pointer, int64_t capacity, int64_t n,
                                                        const float *__restrict__ obs, const float *__restrict__ act,
                                                        const float *__restrict__ rew, const float *__restrict__ nxt,
                                                        const float *__restrict__ done) {
  const int NO = round_up(S + A + 2, 4), W = NO + S;  // s' starts on a 16-byte boundary
  const int quads = stride >> 2;
  const int64_t total = n * (int64_t)quads;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / quads;
    const int c0 = (int)(e - i * quads) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      float x = 0.f;
      if (c < S)
        x = obs[i * S + c];
      else if (c < S + A)
        x = act[i * A + (c - S)];
      else if (c == S + A)
        x = rew[i];
      else if (c == S + A + 1)
        x = done[i];
      else if (c >= NO && c < W)
        x = nxt[i * S + (c - NO)];
      v[j] = x;
    }
    const int64_t row = (pointer + i) % capacity;
    *reinterpret_cast<float4 *>(rows + row * stride + c0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

hipError_t launch_replay_append(float *rows, int stride, int S, int A, int64_t pointer, int64_t capacity, int64_t n,
                                const float *obs, const float *act, const float *rew, const float *nxt,
                                const float *done, hipStream_t st) {
  const int64_t total = n * (int64_t)(stride >> 2);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 8) blocks = 256 * 8;  // (the kernel strides over the rest)
  const int grid = (int)blocks;
  hipLaunchKernelGGL(k_replay_append, dim3(grid), dim3(256), 0, st, rows, stride, S, A, pointer, capacity, n, obs, act,
                     rew, nxt, done);
  return hipGetLastError();
}

// ------------------------------------------------------------ growing draw --
// numpy's RandomState.randint(0, hi_t, B) for t = 0 .. n_steps - 1 as ONE stream (np_sampler.hip has what a
// bounded draw does), hi_t = min(hi0 + t growth, cap).  The stream is cut into runs of values that share a
// bound: one step while the bound still grows, everything that is left once it stands (growth 0, or cap
// reached).  A round of 624 words is judged under the bound of the current run; when the run ends inside
// the round, the words behind the one that gave its last value are judged again under the next run's mask
// and threshold -- the loop below comes back with pos just behind that word and the same key.  A run with
// hi == 1 consumes no word and is zeros.  The rounds are np_stream.h's np_twist / np_judge, what np_draw_stream
// itself is made of; with growth 0 this is np_draw_stream, round for round.
struct NpGrowArgs {
  int64_t *out[IQLHIP_MAX_GROUP];
  int64_t hi0[IQLHIP_MAX_GROUP];
  int64_t cap[IQLHIP_MAX_GROUP];
};

__global__ __launch_bounds__(NP_THREADS) void k_np_randint_growing(uint32_t *__restrict__ state, NpGrowArgs a,
                                                                    int growth, int B, int64_t n_steps) {
  __shared__ uint32_t key[MT_N];
  __shared__ int32_t cnt[2][3][NP_WAVES];  // accepted words per (judgement parity, segment, wave)
  __shared__ int32_t cut;                  // pos behind the word that gave the last value of a run
  const int k = blockIdx.x, t = threadIdx.x;
  uint32_t *st = state + (size_t)k * (MT_N + 1);
  int64_t *out = a.out[k];
  const int64_t hi0 = a.hi0[k], cap = a.cap[k], total = n_steps * (int64_t)B;
  NpLane L;
  int pos = np_lane_load(L, st, key);
  int64_t done = 0;  // values written; a run starts on a multiple of B
  int par = 0;
  while (done < total) {
    // the run that starts here: its bound and where it ends
    const int64_t step = done / B;
    int64_t hi = hi0 + step * growth;
    if (hi > cap) hi = cap;
    const int64_t run_end = (growth == 0 || hi >= cap) ? total : (step + 1) * (int64_t)B;
    const uint32_t rng = (uint32_t)(hi - 1);
    if (rng == 0) {  // hi == 1: zeros, no word consumed
      for (int64_t i = done + t; i < run_end; i += NP_THREADS) out[i] = 0;
      done = run_end;
      continue;
    }
    const uint32_t mask = np_mask_of(rng);
    while (done < run_end) {
      if (pos >= MT_N) {
        np_twist(L, key);
        pos = 0;
      }
      const NpJudged J = np_judge(L, cnt[par], pos, rng, mask);
      par ^= 1;
      const int64_t need = run_end - done;
      if (J.a0 && J.pre0 < need) out[done + J.pre0] = (int64_t)J.v0;
      if (J.a1 && J.pre1 < need) out[done + J.pre1] = (int64_t)J.v1;
      if (J.a2 && J.pre2 < need) out[done + J.pre2] = (int64_t)J.v2;
      if (J.got < need) {  // every word of the key consumed
        done += J.got;
        pos = MT_N;
        continue;
      }
      // the need-th accepted word of this round gave the run's last value: the stream goes on behind it
      if (J.a0 && J.pre0 == need - 1) cut = L.e0 + 1;
      if (J.a1 && J.pre1 == need - 1) cut = L.e1 + 1;
      if (J.a2 && J.pre2 == need - 1) cut = L.e2 + 1;
      __syncthreads();
      pos = cut;
      done = run_end;
    }
  }
  if (t == 0) st[MT_N] = (uint32_t)pos;
  np_lane_store(L, st);
}

hipError_t launch_np_randint_growing(uint32_t *state, const int64_t *hi0, const int64_t *cap, int growth, int K,
                                     int batch, int64_t n_steps, int64_t *const *out, hipStream_t st) {
  NpGrowArgs a = {};
  for (int k = 0; k < K; ++k) a.out[k] = out[k], a.hi0[k] = hi0[k], a.cap[k] = cap[k];
  hipLaunchKernelGGL(k_np_randint_growing, dim3(K), dim3(NP_THREADS), 0, st, state, a, growth, batch, n_steps);
  return hipGetLastError();
}

// ------------------------------------------------------ exploration action --
// fref:686-693 behind the actor's forward: `act` holds the tanh output [rows][A] and becomes the action.
//   Gaussian       a = mean + exp(clamp(log_std, -20, 2)) * eps           (Normal.sample, fref:687)
//   deterministic  a = out + clamp(expl_noise * eps, -noise_clip, noise_clip)   (fref:689-692)
//   both           a = clamp(max_action * a, -max_action, max_action)      (fref:693)
// eps: [rows][A] as given, or (NULL) standard normals from the trainer's Philox key: block (row, call,
// column / 4, STREAM_EXPLORE), words (x, y) and (z, w) each one Box-Muller pair
// u1 = (x + 1) 2^-32, u2 = y 2^-32 -> sqrt(-2 ln u1) (cos, sin)(2 pi u2), evaluated in double.
constexpr uint32_t STREAM_EXPLORE = 4;

__global__ __launch_bounds__(256) void k_explore_epilogue(float *__restrict__ act, int64_t rows, int A,
                                                           const float *__restrict__ log_std,
                                                           const float *__restrict__ eps, float expl_noise,
                                                           float noise_clip, float max_action, uint64_t seed,
                                                           uint32_t call) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * A; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / A;
    const int c = (int)(e - row * A);
    float z;
    if (eps) {
      z = eps[e];
    } else {
      const Philox4 r = philox4x32_10((uint32_t)row, call, (uint32_t)(c >> 2), STREAM_EXPLORE, (uint32_t)seed,
                                      (uint32_t)(seed >> 32));
      const uint32_t ua = (c & 2) ? r.z : r.x, ub = (c & 2) ? r.w : r.y;
      const double u1 = ((double)ua + 1.0) * (1.0 / 4294967296.0), u2 = (double)ub * (1.0 / 4294967296.0);
      const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925 * u2;
      z = (float)(rad * ((c & 1) ? sin(ang) : cos(ang)));
    }
    float x = act[e];
    if (log_std) {
      const float ls = fminf(fmaxf(log_std[c], -20.f), 2.f);
      x = x + expf(ls) * z;
    } else {
      x = x + fminf(fmaxf(expl_noise * z, -noise_clip), noise_clip);
    }
    act[e] = fminf(fmaxf(max_action * x, -max_action), max_action);
  }
}

hipError_t launch_explore_epilogue(float *act, int64_t rows, int A, const float *log_std, const float *eps,
                                   float expl_noise, float noise_clip, float max_action, uint64_t seed, uint32_t call,
                                   hipStream_t st) {
  int64_t blocks = (rows * A + 255) / 256;
  if (blocks > 256 * 8) blocks = 256 * 8;  // (the kernel strides over the rest)
  hipLaunchKernelGGL(k_explore_epilogue, dim3((unsigned)blocks), dim3(256), 0, st, act, rows, A, log_std,
                     eps, expl_noise, noise_clip, max_action, seed, call);
  return hipGetLastError();
}

}  // namespace iqlhip
