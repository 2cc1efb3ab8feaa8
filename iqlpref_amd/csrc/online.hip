// The three kernels of the online phase of algorithms/finetune/iql.py ("fref"): every tick acts with
// exploration noise (fref:681-694), appends the transition to the replay ring (fref:164-180), samples
// from the grown buffer (fref:155-156) and takes one gradient step.  The step is the trainer's; what is
// here is what the tick needs around it, each kernel on its own:
//   k_replay_append       n transitions into the packed rows at (pointer + i) % capacity;
//   k_np_randint_growing  numpy's legacy randint for n_steps consecutive steps whose bound grows;
//   k_explore_epilogue    mean / output of the actor -> noisy, scaled, clamped action;
// and, for K seeds that tick side by side, the act and the append of all of them as one launch each:
//   k_replay_append_group one transition into each of K rings;
//   k_explore_group       one actor forward + epilogue per work-group, bit for bit the solo pair's row.
#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"
#include "launchers.h"
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

// ------------------------------------------------- the tick of a seed group --
// One transition into each of K rings: block k writes row pointer[k] % capacity[k] of ring k from
// stage[k] = s | a | r | s' | d (finetune.ReplayBuffer's staging order), the float4 pieces of k_replay_append.
struct AppendGroupArgs {
  float *rows[IQLHIP_MAX_GROUP];
  int64_t row[IQLHIP_MAX_GROUP];  // pointer % capacity
};

__global__ __launch_bounds__(64) void k_replay_append_group(AppendGroupArgs a, int stride, int S, int A,
                                                            const float *__restrict__ stage) {
  const int NO = round_up(S + A + 2, 4), W = NO + S, SW = 2 * S + A + 2;
  const int k = blockIdx.x;
  const float *h = stage + (size_t)k * SW;
  float *dst = a.rows[k] + a.row[k] * stride;
  for (int e = threadIdx.x; e < (stride >> 2); e += 64) {
    const int c0 = e * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      float x = 0.f;
      if (c < S + A + 1)
        x = ldg(h + c);  // s | a | r
      else if (c == S + A + 1)
        x = ldg(h + SW - 1);  // d
      else if (c >= NO && c < W)
        x = ldg(h + S + A + 1 + (c - NO));  // s'
      v[j] = x;
    }
    stg16(dst + c0, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// iqlhip_explore_action for one state row of each of K actors in ONE launch: work-group k runs member k's
// forward on the torch-layout fp32 masters [out][in] where they lie in the parameter arena, then the
// arithmetic of k_explore_epilogue for row 0, and writes row k of out[K][A].  No repacked image, no scratch.
//
// Row k equals what launch_mlp_f32 + k_explore_epilogue write for that one row, bit for bit.  As in
// k_bb_episodes (bb_sim.hip), what fixes an output's bits is the order of operations on ITS accumulator, and
// rows and n-tiles of a mfma_f32_16x16x4f32 tile do not mix: the one live row sits in row 0 of a tile whose
// other rows are zero.  launch_mlp_f32 has two orders and this kernel follows its rule:
//   no width above 256 (k_mlp_f32)   hidden layers: acc = 0; ks = 0 .. nk-1, c = 0 .. 3 in sequence.  Output
//                                    layer (A <= 32: fewer than four n-tiles): partials over ks = w, w + 4, ..
//                                    for w = 0 .. 3 summed ((p0 + p1) + p2) + p3, exact zeros when nk < 4;
//   a width above 256 (k_mlp_wide)   every layer, the output layer too, one chain over ks.
// Then + bias, the activation, and on hidden layers the dropout mask of both kernels: Philox block
// (row 0, call, unit / 4 | layer << 16, STREAM_MLP_DROPOUT), word unit % 4, under the member's seed.
//
// The B fragment of lane (r, q) for n-tile ft and k-step ks is W[16 ft + r][16 ks + 4 q .. + 3]: ONE 16-byte
// load where the rows of W are 16-byte aligned, four scalar loads elsewhere (the first layer: rows of S
// floats); outputs >= N and inputs >= K read as zero, which is the zero padding of the fragment image.
// A layer is a chain of dependent MFMAs fed by weights the update kernel wrote a moment ago on other XCDs, so
// what a wave can do about its latency is keep loads in flight: EXG_PF k-steps x 4 n-tiles of fragments per
// wave during the MFMAs of the run before, all of a wave's fragments at once in the k-split output layer.
// The noise of the epilogue is drawn ahead of the forward: nothing but tanh and the clamp follows the last sum.
constexpr int EXG_THREADS = 256;
constexpr int EXG_MAXW = 1024;  // IQLHIP's widest hidden layer
constexpr int EXG_PF = 4;       // k-steps of B fragments a wave keeps in flight

struct ExploreGroupArgs {
  const float *W[IQLHIP_MAX_GROUP][IQLHIP_MAX_HIDDEN + 1];
  const float *b[IQLHIP_MAX_GROUP][IQLHIP_MAX_HIDDEN + 1];
  const float *log_std[IQLHIP_MAX_GROUP];  // NULL: deterministic policy
  uint64_t seed[IQLHIP_MAX_GROUP];
  uint32_t call[IQLHIP_MAX_GROUP];
  uint32_t drop_thr[IQLHIP_MAX_GROUP];  // 0: no dropout
  float drop_scale[IQLHIP_MAX_GROUP];
  int16_t n_hidden[IQLHIP_MAX_GROUP], hidden[IQLHIP_MAX_GROUP];
};

__device__ __forceinline__ f32x4 exg_load_b(const float *W, int K, int N, int f, int k0, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (f < N) {
    const float *p = W + (size_t)f * K + k0;
    if (vec) {
      if (k0 < K) v = __builtin_bit_cast(f32x4, ldg16(p));  // (K % 4 == 0: the piece lies inside the row)
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (k0 + c < K) v[c] = ldg(p + c);
    }
  }
  return v;
}

__global__ __launch_bounds__(EXG_THREADS) void k_explore_group(const ExploreGroupArgs G, int S, int A,
                                                               const float *__restrict__ s, int s_stride,
                                                               const float *__restrict__ eps, float expl_noise,
                                                               float noise_clip, float max_action,
                                                               float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_x[2][EXG_MAXW];  // the activation row, ping-pong
  __shared__ float s_red[4][32];
  const int m = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int n_layers = G.n_hidden[m] + 1, H = G.hidden[m];
  const bool wide = H > 256;  // (S <= 128 and A <= 32: only the hidden width can be)
  const uint64_t seed = G.seed[m];
  const uint32_t call = G.call[m], drop_thr = G.drop_thr[m];
  const float drop_scale = G.drop_scale[m];

  for (int c = tid; c < round_up(S, 16); c += EXG_THREADS) s_x[0][c] = c < S ? ldg(s + (size_t)m * s_stride + c) : 0.f;
  // the epilogue's standard normal of column tid (k_explore_epilogue, row 0)
  float z = 0.f;
  if (tid < A) {
    const int c = tid;
    if (eps) {
      z = ldg(eps + (size_t)m * A + c);
    } else {
      const Philox4 ph = philox4x32_10(0u, call, (uint32_t)(c >> 2), STREAM_EXPLORE, (uint32_t)seed,
                                       (uint32_t)(seed >> 32));
      const uint32_t ua = (c & 2) ? ph.z : ph.x, ub = (c & 2) ? ph.w : ph.y;
      const double u1 = ((double)ua + 1.0) * (1.0 / 4294967296.0), u2 = (double)ub * (1.0 / 4294967296.0);
      const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925 * u2;
      z = (float)(rad * ((c & 1) ? sin(ang) : cos(ang)));
    }
  }
  __syncthreads();

  float v_out = 0.f;  // column tid of the output layer: sum + bias
  for (int l = 0; l < n_layers; ++l) {
    const bool last = l == n_layers - 1;
    const int K = l == 0 ? S : H, N = last ? A : H;
    const int nk = round_up(K, 16) / 16, ntile = round_up(N, 16) / 16;
    const float *W = G.W[m][l], *bias = G.b[m][l];
    const bool vec = (K & 3) == 0 && ((uintptr_t)W & 15) == 0;
    const float *in = s_x[l & 1];
    float *nxt = s_x[(l + 1) & 1];
    // A fragment: row 0 of the tile is the activation row, rows 1 .. 15 are zero
    auto load_a = [&](int ks) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (r == 0) a = *reinterpret_cast<const f32x4 *>(in + 16 * ks + 4 * q);
      return a;
    };
    if (last && !wide) {  // the k-split output layer of k_mlp_f32
      f32x4 pacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      f32x4 bq[4][2];  // nk <= 16 here: at most four k-steps per wave, all of their fragments in flight at once
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          bq[i][t] = exg_load_b(W, K, t < ntile ? N : 0, 16 * t + r, 16 * (wave + 4 * i) + 4 * q, vec);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ks = wave + 4 * i;
        if (ks >= nk) break;
        const f32x4 af = load_a(ks);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t < ntile) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              pacc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[c], bq[i][t][c], pacc[t], 0, 0, 0);
          }
        }
      }
      if (q == 0) s_red[wave][r] = pacc[0][0], s_red[wave][16 + r] = pacc[1][0];  // row 0 of the tiles
      __syncthreads();
      if (tid < A) {
        float sum = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) sum += s_red[w][tid];
        v_out = sum + ldg(bias + tid);
      }
      break;
    }
    // this wave's n-tiles, four at a time: wave + 4 j + 16 g
    for (int g = 0; 16 * g + wave < ntile; ++g) {
      int f[4];
      f32x4 acc[4], bq[EXG_PF][4];
      float bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tile = wave + 4 * j + 16 * g;
        f[j] = tile < ntile ? 16 * tile + r : N;  // (N: a tile that does not exist loads zeros)
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        bv[j] = f[j] < N ? ldg(bias + f[j]) : 0.f;
      }
      // k-steps in runs of EXG_PF: the fragments of the next run are in flight during the MFMAs of this one
      // (a k-step beyond nk lies beyond K and loads nothing)
#pragma unroll
      for (int u = 0; u < EXG_PF; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[u][j] = exg_load_b(W, K, N, f[j], 16 * u + 4 * q, vec);
      for (int ks0 = 0; ks0 < nk; ks0 += EXG_PF) {
        f32x4 bn[EXG_PF][4];
#pragma unroll
        for (int u = 0; u < EXG_PF; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) bn[u][j] = exg_load_b(W, K, N, f[j], 16 * (ks0 + EXG_PF + u) + 4 * q, vec);
#pragma unroll
        for (int u = 0; u < EXG_PF; ++u) {
          if (ks0 + u >= nk) break;
          const f32x4 af = load_a(ks0 + u);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (wave + 4 * j + 16 * g < ntile)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[c], bq[u][j][c], acc[j], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < EXG_PF; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) bq[u][j] = bn[u][j];
      }
      if (q == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int tile = wave + 4 * j + 16 * g;
          if (tile >= ntile) continue;
          const int col = 16 * tile + r;
          float v = acc[j][0] + bv[j];
          if (last) {  // (wide: A <= 32 columns)
            if (col < N) s_red[0][col] = v;
            continue;
          }
          v = col < N ? fmaxf(v, 0.f) : 0.f;  // zero K padding
          if (drop_thr) {
            const Philox4 ph = philox4x32_10(0u, call, (uint32_t)(col >> 2) | ((uint32_t)l << 16), STREAM_MLP_DROPOUT,
                                             (uint32_t)seed, (uint32_t)(seed >> 32));
            const uint32_t w = (col & 3) == 0 ? ph.x : (col & 3) == 1 ? ph.y : (col & 3) == 2 ? ph.z : ph.w;
            v = w >= drop_thr ? v * drop_scale : 0.f;
          }
          nxt[col] = v;
        }
      }
    }
    __syncthreads();
    if (last && tid < A) v_out = s_red[0][tid];
  }

  if (tid < A) {
    const int c = tid;
    float x = tanhf(v_out);
    const float *log_std = G.log_std[m];
    if (log_std) {
      const float ls = fminf(fmaxf(ldg(log_std + c), -20.f), 2.f);
      x = x + expf(ls) * z;
    } else {
      x = x + fminf(fmaxf(expl_noise * z, -noise_clip), noise_clip);
    }
    stg(out + (size_t)m * A + c, fminf(fmaxf(max_action * x, -max_action), max_action));
  }
}

// actors[k]: member k's actor as iqlhip_explore_action describes it to launch_mlp_f32 (torch-layout weights in
// the arena, dropout_p / dropout_call / dropout_seed the member's); log_std[k] NULL for a deterministic policy.
hipError_t launch_explore_group(const iqlhip_mlp_desc *actors, const float *const *log_std, int K, const float *s,
                                int s_stride, const float *eps, float expl_noise, float noise_clip, float max_action,
                                float *out, hipStream_t st) {
  ExploreGroupArgs G = {};
  for (int k = 0; k < K; ++k) {
    const iqlhip_mlp_desc &d = actors[k];
    for (int l = 0; l < d.n_layers; ++l) G.W[k][l] = d.weights[l], G.b[k][l] = d.biases[l];
    G.log_std[k] = log_std[k], G.seed[k] = d.dropout_seed, G.call[k] = d.dropout_call;
    G.n_hidden[k] = (int16_t)(d.n_layers - 1), G.hidden[k] = (int16_t)d.dims[1];
    G.drop_thr[k] = 0, G.drop_scale[k] = 1.f;
    if (d.dropout_p > 0.f) {  // launch_mlp_f32's threshold and scale
      const double thr = (double)d.dropout_p * 4294967296.0;
      G.drop_thr[k] = thr >= 4294967295.0 ? 0xffffffffu : (thr < 1.0 ? 1u : (uint32_t)thr);
      G.drop_scale[k] = 1.0f / (float)(1.0 - (double)d.dropout_p);
    }
  }
  const int S = actors[0].dims[0], A = actors[0].dims[actors[0].n_layers];
  hipLaunchKernelGGL(k_explore_group, dim3(K), dim3(EXG_THREADS), 0, st, G, S, A, s, s_stride, eps, expl_noise,
                     noise_clip, max_action, out);
  return hipGetLastError();
}

}  // namespace iqlhip

using namespace iqlhip;

// ------------------------------------------------------------ entry points --
// what the append into one ring and into the rings of a group check alike: the packed row
static int replay_geometry_check(int32_t row_stride, int32_t S, int32_t A) {
  if (S <= 0 || A <= 0 || row_stride < iqlhip_replay_row_stride(S, A) || (row_stride & 3))
    return fail(IQLHIP_ERR_INVALID, "bad replay geometry S=%d A=%d stride=%d", S, A, row_stride);
  return 0;
}

extern "C" int iqlhip_replay_append(float *rows, int32_t row_stride, int32_t S, int32_t A, int64_t capacity,
                                    int64_t pointer, int64_t n, const float *obs, const float *act, const float *rew,
                                    const float *next_obs, const float *done, void *stream) {
  if (!rows || !obs || !act || !rew || !next_obs || !done) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (int rc = replay_geometry_check(row_stride, S, A)) return rc;
  if ((uintptr_t)rows & 15) return fail(IQLHIP_ERR_INVALID, "rows must start on a 16-byte boundary");
  if (capacity < 1) return fail(IQLHIP_ERR_INVALID, "capacity = %lld must be >= 1", (long long)capacity);
  if (pointer < 0 || pointer >= capacity)
    return fail(IQLHIP_ERR_INVALID, "pointer = %lld outside 0..%lld", (long long)pointer, (long long)capacity - 1);
  if (n < 1) return fail(IQLHIP_ERR_INVALID, "n = %lld must be >= 1", (long long)n);
  if (n > capacity)
    return fail(IQLHIP_ERR_INVALID, "n = %lld transitions do not fit a ring of %lld rows", (long long)n,
                (long long)capacity);
  int64_t blocks = (n * (int64_t)(row_stride >> 2) + 255) / 256;
  if (blocks > 256 * 8) blocks = 256 * 8;  // (the kernel strides over the rest)
  hipLaunchKernelGGL(k_replay_append, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, rows, row_stride, S, A,
                     pointer, capacity, n, obs, act, rew, next_obs, done);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_replay_append_group(float *const *rows, int32_t row_stride, int32_t S, int32_t A,
                                          const int64_t *capacity, const int64_t *pointer, int32_t K,
                                          const float *stage, void *stream) {
  if (!rows || !capacity || !pointer || !stage) return fail(IQLHIP_ERR_INVALID, "null pointer");
  if (K < 1 || K > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "K = %d: 1..%d rings", K, IQLHIP_MAX_GROUP);
  if (int rc = replay_geometry_check(row_stride, S, A)) return rc;
  for (int k = 0; k < K; ++k) {
    if (!rows[k]) return fail(IQLHIP_ERR_INVALID, "null rows[%d]", k);
    if ((uintptr_t)rows[k] & 15) return fail(IQLHIP_ERR_INVALID, "rows[%d] must start on a 16-byte boundary", k);
    if (capacity[k] < 1) return fail(IQLHIP_ERR_INVALID, "capacity[%d] = %lld must be >= 1", k, (long long)capacity[k]);
    if (pointer[k] < 0 || pointer[k] >= capacity[k])
      return fail(IQLHIP_ERR_INVALID, "pointer[%d] = %lld outside 0..%lld", k, (long long)pointer[k],
                  (long long)capacity[k] - 1);
    for (int j = 0; j < k; ++j)
      if (rows[j] == rows[k]) return fail(IQLHIP_ERR_INVALID, "ring %d listed twice", k);
  }
  AppendGroupArgs a = {};
  for (int k = 0; k < K; ++k) a.rows[k] = rows[k], a.row[k] = pointer[k] % capacity[k];
  hipLaunchKernelGGL(k_replay_append_group, dim3(K), dim3(64), 0, (hipStream_t)stream, a, row_stride, S, A, stage);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int iqlhip_np_randint_growing(uint32_t *state, const int64_t *hi0, const int64_t *cap, int32_t growth,
                                         int32_t K, int32_t batch, int64_t n_steps, int64_t *const *out,
                                         void *stream) {
  if (!state || !hi0 || !cap || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (K < 1 || K > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "K = %d: 1..%d streams", K, IQLHIP_MAX_GROUP);
  if (batch < 1) return fail(IQLHIP_ERR_INVALID, "batch = %d must be >= 1", batch);
  if (n_steps < 0) return fail(IQLHIP_ERR_INVALID, "n_steps = %lld must be >= 0", (long long)n_steps);
  if (growth != 0 && growth != 1) return fail(IQLHIP_ERR_INVALID, "growth = %d must be 0 or 1", growth);
  for (int k = 0; k < K; ++k) {
    if (hi0[k] < 1 || hi0[k] > (int64_t(1) << 32))
      return fail(IQLHIP_ERR_INVALID, "hi0[%d] = %lld outside 1..2^32", k, (long long)hi0[k]);
    if (cap[k] < hi0[k] || cap[k] > (int64_t(1) << 32))
      return fail(IQLHIP_ERR_INVALID, "cap[%d] = %lld outside hi0..2^32", k, (long long)cap[k]);
    if (!out[k]) return fail(IQLHIP_ERR_INVALID, "null out[%d]", k);
  }
  hipStream_t st = (hipStream_t)stream;
  if (int rc = np_check_pos(state, K, st)) return rc;
  if (n_steps == 0) return 0;
  NpGrowArgs a = {};
  for (int k = 0; k < K; ++k) a.out[k] = out[k], a.hi0[k] = hi0[k], a.cap[k] = cap[k];
  hipLaunchKernelGGL(k_np_randint_growing, dim3(K), dim3(NP_THREADS), 0, st, state, a, growth, batch, n_steps);
  HIP_TRY(hipGetLastError());
  return 0;
}
