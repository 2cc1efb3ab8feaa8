// Generic fp32 MLP forward over many rows on the exact-f32 matrix path
// (v_mfma_f32_16x16x4_f32).  Serves nn.Module.forward() of the network
// containers outside the autocast region (ref:452-543, eval_actor ref:306-319)
// and the Markovian reward relabel (ref:719-724, ref:986-991, ref:1176-1178).
//
// Two launches per call:
//   k_mlp_repack  every layer's weights (torch [out][in] or x@W [in][out]) are rewritten once
//                 into the fragment-major image of common.h (zero padded to 16 x 16): a B
//                 fragment is then ONE contiguous 1 KiB read per wave instruction instead of
//                 64 scalar loads with stride K between lanes.
//   k_mlp_f32     one work-group = 64 rows.  The activations live in ONE LDS buffer
//                 [64][lda] (67 KB at width 256: two work-groups per CU); a layer is computed
//                 into registers (wave w owns n-tiles w, w+4, w+8, w+12; four 16-row M tiles
//                 share every B fragment; A fragments are shared by the wave's four n-tiles),
//                 then written back in place behind a barrier.  Per 16-deep k-step a wave issues
//                 4 LDS reads, 4 fragment loads (the next step's, prefetched) and 64 MFMAs.
//
// iqlhip_mlp_set (the post-hoc checkpoint evaluation: M actors x R rows per environment step): the M
// members' images are written ONCE at create, a fixed stride apart in one allocation, and
//   k_mlp_set     grid (row tile, member) runs the same 64-row body (mlp_row_tile) on member m's image,
//                 with the tile's empty 16-row M tiles left out: one launch per step, no repack.
#include <new>

#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"
#include "launchers.h"

namespace iqlhip {

constexpr int MROWS = 64;
constexpr int MAXT = 4;  // n-tiles per wave: widths <= 256

struct MlpArgs {
  int32_t n_layers;
  int32_t dims[IQLHIP_MLP_MAX_LAYERS + 1];
  const float *Wf[IQLHIP_MLP_MAX_LAYERS];  // fragment-major [round16(out)][round16(in)]
  const float *b[IQLHIP_MLP_MAX_LAYERS];
  int32_t hidden_act;  // 0 relu, 1 tanh
  int32_t out_act;     // 0 none, 1 tanh
  int32_t lda;         // LDS row stride (floats)
  // nn.Dropout(p) behind every hidden activation (ref:436-437) in train mode: keep iff the
  // element's Philox word >= drop_thr, kept values times 1 / (1 - p); drop_thr = 0: no dropout
  uint32_t drop_thr;
  float drop_scale;
  uint64_t drop_seed;
  uint32_t drop_call;
};

struct RepackArgs {
  int32_t n_layers;
  int32_t dims[IQLHIP_MLP_MAX_LAYERS + 1];
  const float *W[IQLHIP_MLP_MAX_LAYERS];
  float *Wf[IQLHIP_MLP_MAX_LAYERS];
  int32_t w_in_out;  // 1: W is [in][out]
};

__global__ void k_mlp_repack(const RepackArgs R) {
  using P = Prec<false>;
  const int l = blockIdx.y;
  if (l >= R.n_layers) return;
  const int K = R.dims[l], N = R.dims[l + 1];
  const int Kp = round_up(K, 16), Np = round_up(N, 16);
  const float *W = R.W[l];
  float *Wf = R.Wf[l];
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < Np * Kp; e += gridDim.x * blockDim.x) {
    // consecutive threads read consecutive source elements of the layout at hand
    const int f = R.w_in_out ? e % Np : e / Kp, k = R.w_in_out ? e / Np : e % Kp;
    float v = 0.f;
    if (f < N && k < K) v = R.w_in_out ? W[(size_t)k * N + f] : W[(size_t)f * K + k];
    Wf[fidx<P>(f, k, Kp / 16)] = v;
  }
}

// activation codes of iqlhip_mlp_desc: 0 / 1 are the torch containers' (hidden: relu / tanh; output:
// none / tanh); 8 + i is entry i of reward_models/q_mlp.py:121-130
//   cos, tanh, relu, softplus, sin, leaky_relu, swish, none
__device__ __forceinline__ float act_flax(float v, int i) {
  switch (i) {
    case 0: return cosf(v);
    case 1: return tanhf(v);
    case 2: return fmaxf(v, 0.f);
    case 3: return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v)));  // jax.nn.softplus = logaddexp(x, 0)
    case 4: return sinf(v);
    case 5: return v >= 0.f ? v : 0.01f * v;                  // jax.nn.leaky_relu, slope 0.01
    case 6: return v / (1.f + expf(-v));                      // swish = x * sigmoid(x)
    default: return v;
  }
}
// The kernel is instantiated per activation family (ACT: 0 relu hidden layers, 1 tanh hidden layers,
// 2 anything of the table above).  The epilogues are unrolled 64-fold over register tiles: with the
// whole table inlined at every site the kernel was 0.5 MB of code and every site an instruction-cache
// miss (the relu path spent more time there than in its MFMAs).  The table variant therefore writes
// raw sums to LDS and applies the activation in ONE rolled pass.
template <int ACT>
__device__ __forceinline__ float act_apply(float v, int kind) {  // hidden layers
  if constexpr (ACT == 0) return fmaxf(v, 0.f);
  if constexpr (ACT == 1) return tanhf(v);
  return kind >= 8 ? act_flax(v, kind - 8) : (kind == 0 ? fmaxf(v, 0.f) : tanhf(v));
}
template <int ACT>
__device__ __forceinline__ float out_apply(float v, int kind) {  // output layer
  if constexpr (ACT != 2) return kind == 1 ? tanhf(v) : v;
  return kind >= 8 ? act_flax(v, kind - 8) : (kind == 1 ? tanhf(v) : v);
}

// One 64-row tile through every layer: the body of k_mlp_f32 and of k_mlp_set.  Rows row0 .. row0 + 64 of
// x[n] -> out[n]; the weight images and biases are M.Wf[l] + wofs and M.b[l] + wofs (k_mlp_set: member m's
// copy lies m strides behind member 0's).  MT: how many of the tile's four 16-row M tiles are computed.
// Every (n-tile, M tile) pair has accumulators of its own, so an M tile left out changes nothing in the
// others; the rows of one that is left out must lie at or beyond n.  buf: [16 MT][lda] floats of LDS.
template <int ACT, int MT>
__device__ __forceinline__ void mlp_row_tile(const MlpArgs M, const size_t wofs, const float *__restrict__ x,
                                             const int64_t n, const int64_t row0, const int x_stride,
                                             float *__restrict__ out, const int out_stride, float *buf) {
  using P = Prec<false>;
  constexpr int TROWS = 16 * MT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int lda = M.lda;

  // input rows, zero padded to a multiple of 16 columns
  {
    const int K0 = M.dims[0], K0p = round_up(K0, 16);
    for (int e = tid; e < TROWS * K0p; e += 256) {
      const int rr = e / K0p, c = e - rr * K0p;
      float v = 0.f;
      if (row0 + rr < n && c < K0) v = ldg(x + (size_t)(row0 + rr) * x_stride + c);
      buf[rr * lda + c] = v;
    }
  }
  __syncthreads();

  for (int l = 0; l < M.n_layers; ++l) {
    const int K = M.dims[l], N = M.dims[l + 1];
    const int nk = round_up(K, 16) / 16, ntile = round_up(N, 16) / 16;
    const float *Wf = M.Wf[l] + wofs;
    const float *bias = M.b[l] + wofs;
    const bool last = l == M.n_layers - 1;
    if (last && ntile < 4) {
      // ---- narrow output layer (N < 64, e.g. the reward head N = 1): with n-tiles over waves
      // only `ntile` waves would work through all of K; instead the four waves split the k-steps,
      // every wave accumulates all n-tiles for its share, and the partial tiles meet in LDS ----
      f32x4 pacc[3][MT];
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) pacc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int ks = wave; ks < nk; ks += 4) {
        uint4 a[MT], bq[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bq[t] = ldg16(Wf + frag_off<P>(t < ntile ? t : 0, ks, nk, lane));
#pragma unroll
        for (int m = 0; m < MT; ++m)
          a[m] = *reinterpret_cast<const uint4 *>(buf + (16 * m + r) * lda + 16 * ks + 4 * q);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if (t < ntile) {
#pragma unroll
            for (int m = 0; m < MT; ++m) P::mma(a[m], bq[t], pacc[t][m]);
          }
        }
      }
      __syncthreads();  // the activations have been read: the buffer holds the partial tiles now
      f32x4 *red = reinterpret_cast<f32x4 *>(buf);  // [4 waves][ntile][4 m][64 lanes]
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < ntile)
#pragma unroll
          for (int m = 0; m < MT; ++m) red[((wave * ntile + t) * 4 + m) * 64 + lane] = pacc[t][m];
      __syncthreads();
      for (int e = tid; e < ntile * 4 * 64; e += 256) {
        const int ln = e & 63, m = (e >> 6) & 3, t = e >> 8;
        if (MT < 4 && m >= MT) continue;
        f32x4 sum = red[((0 * ntile + t) * 4 + m) * 64 + ln];
#pragma unroll
        for (int w = 1; w < 4; ++w) sum += red[((w * ntile + t) * 4 + m) * 64 + ln];
        const int ncol = 16 * t + (ln & 15);
        if (ncol < N) {
          const float bvv = ldg(bias + ncol);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int rr = 16 * m + 4 * (ln >> 4) + i;
            if (row0 + rr < n) stg(out + (size_t)(row0 + rr) * out_stride + ncol, out_apply<ACT>(sum[i] + bvv, M.out_act));
          }
        }
      }
      __syncthreads();
      continue;
    }
    // this wave's n-tiles: wave, wave + 4, ... (clamped copies beyond ntile are computed on a
    // valid fragment and dropped: no branches in the load stream)
    int tile[MAXT];
    bool live[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      live[t] = wave + 4 * t < ntile;
      tile[t] = live[t] ? wave + 4 * t : 0;
    }
    f32x4 acc[MAXT][MT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bv[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) bv[t] = ldg(bias + (16 * tile[t] + r < N ? 16 * tile[t] + r : N - 1));
    if (live[0]) {  // wave-uniform: a wave without tiles (narrow layers) skips the k loop
      uint4 bq[MAXT];
#pragma unroll
      for (int t = 0; t < MAXT; ++t) bq[t] = ldg16(Wf + frag_off<P>(tile[t], 0, nk, lane));
      for (int ks = 0; ks < nk; ++ks) {
        uint4 bn[MAXT];  // next k-step's fragments, in flight during this step's MFMAs
        const int kn = ks + 1 < nk ? ks + 1 : ks;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) bn[t] = ldg16(Wf + frag_off<P>(tile[t], kn, nk, lane));
        uint4 a[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
          a[m] = *reinterpret_cast<const uint4 *>(buf + (16 * m + r) * lda + 16 * ks + 4 * q);
        // component-major issue order: the four MFMAs of one (n-tile, M-tile) pair accumulate into
        // the same registers (40-cycle dependent latency vs 32-cycle issue); between two of them the
        // wave issues the other 15 pairs
        float4 af[MT], bf[MAXT];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = __builtin_bit_cast(float4, a[m]);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) bf[t] = __builtin_bit_cast(float4, bq[t]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int t = 0; t < MAXT; ++t) {
            if (live[t]) {
#pragma unroll
              for (int m = 0; m < MT; ++m)
                acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][c], bf[t][c], acc[t][m], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int t = 0; t < MAXT; ++t) bq[t] = bn[t];
      }
    }
    __syncthreads();  // every wave has read its last A fragment: the buffer may be overwritten
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (!live[t]) continue;
      const int ncol = 16 * tile[t] + r;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rr = 16 * m + 4 * q + i;
          float v = acc[t][m][i] + bv[t];
          if constexpr (ACT == 2) {
            buf[rr * lda + ncol] = v;  // raw: the table is applied in the rolled pass below
          } else if (!last) {
            buf[rr * lda + ncol] = ncol < N ? act_apply<ACT>(v, M.hidden_act) : 0.f;  // zero K padding
          } else if (ncol < N && row0 + rr < n) {
            stg(out + (size_t)(row0 + rr) * out_stride + ncol, out_apply<ACT>(v, M.out_act));
          }
        }
      }
    }
    __syncthreads();
    if constexpr (ACT == 2) {
      const int Np = 16 * ntile;
#pragma unroll 1
      for (int e = tid; e < TROWS * Np; e += 256) {
        const int rr = e / Np, c = e - rr * Np;
        const float v = buf[rr * lda + c];
        if (!last) {
          buf[rr * lda + c] = c < N ? act_apply<2>(v, M.hidden_act) : 0.f;
        } else if (c < N && row0 + rr < n) {
          stg(out + (size_t)(row0 + rr) * out_stride + c, out_apply<2>(v, M.out_act));
        }
      }
      __syncthreads();
    }
    if (M.drop_thr && !last) {
      // Dropout of this hidden layer (oracle/philox.py mlp_dropout_keep): one Philox4x32 block per
      // (row, 4 consecutive units); a rolled pass over LDS, the 64-fold unrolled epilogues stay lean
      const int Nq = 4 * ntile;
#pragma unroll 1
      for (int e = tid; e < TROWS * Nq; e += 256) {
        const int rr = e / Nq, cq = e - rr * Nq;
        const uint64_t R = (uint64_t)(row0 + rr);
        const Philox4 ph = philox4x32_10((uint32_t)R, M.drop_call, (uint32_t)cq | ((uint32_t)l << 16),
                                         STREAM_MLP_DROPOUT, (uint32_t)M.drop_seed, (uint32_t)(M.drop_seed >> 32));
        float4 v = *reinterpret_cast<float4 *>(buf + rr * lda + 4 * cq);
        v.x = ph.x >= M.drop_thr ? v.x * M.drop_scale : 0.f;
        v.y = ph.y >= M.drop_thr ? v.y * M.drop_scale : 0.f;
        v.z = ph.z >= M.drop_thr ? v.z * M.drop_scale : 0.f;
        v.w = ph.w >= M.drop_thr ? v.w * M.drop_scale : 0.f;
        *reinterpret_cast<float4 *>(buf + rr * lda + 4 * cq) = v;
      }
      __syncthreads();
    }
  }
}


template <int ACT>
__global__ __launch_bounds__(256, 2) void k_mlp_f32(const MlpArgs M, const float *__restrict__ x, int64_t n,
                                                    int x_stride, float *__restrict__ out, int out_stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  mlp_row_tile<ACT, 4>(M, 0, x, n, (int64_t)blockIdx.x * MROWS, x_stride, out, out_stride,
                       reinterpret_cast<float *>(smem));  // [MROWS][lda]
}

// A frozen set of MLPs of one shape (iqlhip_mlp_set): block (tile, m) takes rows 64 tile .. of member m's R
// rows through member m's weights.  The members' images and biases lie `stride` floats apart in one
// allocation, so S.A describes member 0 and the block adds m strides: no table.  A tile's M tiles that
// hold no row (R = 1: three of four) are not computed.
struct MlpSetArgs {
  MlpArgs A;
  int64_t stride;  // floats between two members
  int32_t R;
};

template <int ACT>
__global__ __launch_bounds__(256, 2) void k_mlp_set(const MlpSetArgs S, const float *__restrict__ x, int x_stride,
                                                    float *__restrict__ out, int out_stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *buf = reinterpret_cast<float *>(smem);
  const size_t m = blockIdx.y, wofs = m * (size_t)S.stride;
  const int64_t row0 = (int64_t)blockIdx.x * MROWS, n = S.R;
  x += m * (size_t)S.R * x_stride, out += m * (size_t)S.R * out_stride;
  const int mt = n - row0 >= MROWS ? 4 : (int)(n - row0 + 15) / 16;  // block-uniform
  if (mt == 1) mlp_row_tile<ACT, 1>(S.A, wofs, x, n, row0, x_stride, out, out_stride, buf);
  else if (mt == 2) mlp_row_tile<ACT, 2>(S.A, wofs, x, n, row0, x_stride, out, out_stride, buf);
  else if (mt == 3) mlp_row_tile<ACT, 3>(S.A, wofs, x, n, row0, x_stride, out, out_stride, buf);
  else mlp_row_tile<ACT, 4>(S.A, wofs, x, n, row0, x_stride, out, out_stride, buf);
}

// Widths beyond 256 (up to 1024; ref:417-449 accepts any hidden_dim): one wave per 16 rows, the
// activations ping-pong between two LDS images [16][lda], every B fragment one contiguous read of the
// fragment-major image.  No register tiling across rows or n-tiles: this variant exists for coverage.
__global__ __launch_bounds__(64) void k_mlp_wide(const MlpArgs M, const float *__restrict__ x, int64_t n, int x_stride,
                                                 float *__restrict__ out, int out_stride) {
  using P = Prec<false>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x, r = lane & 15, q = lane >> 4, lda = M.lda;
  float *in = reinterpret_cast<float *>(smem), *nxt = in + 16 * lda;
  const int64_t row0 = (int64_t)blockIdx.x * 16;
  {
    const int K0 = M.dims[0], K0p = round_up(K0, 16);
    for (int e = lane; e < 16 * K0p; e += 64) {
      const int rr = e / K0p, c = e - rr * K0p;
      float v = 0.f;
      if (row0 + rr < n && c < K0) v = ldg(x + (size_t)(row0 + rr) * x_stride + c);
      in[rr * lda + c] = v;
    }
  }
  __syncthreads();
  for (int l = 0; l < M.n_layers; ++l) {
    const int K = M.dims[l], N = M.dims[l + 1];
    const int nk = round_up(K, 16) / 16, ntile = round_up(N, 16) / 16;
    const float *Wf = M.Wf[l], *bias = M.b[l];
    const bool last = l == M.n_layers - 1;
    for (int nt = 0; nt < ntile; ++nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < nk; ++ks) {
        const uint4 a = *reinterpret_cast<const uint4 *>(in + r * lda + ks * 16 + q * 4);
        const uint4 b = ldg16(Wf + frag_off<P>(nt, ks, nk, lane));
        P::mma(a, b, acc);
      }
      const int col = nt * 16 + r;
      const float bv = col < N ? ldg(bias + col) : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t R = row0 + 4 * q + i;
        float v = acc[i] + bv;
        if (!last) {
          v = col < N ? act_apply<2>(v, M.hidden_act) : 0.f;
          if (M.drop_thr) {  // oracle/philox.py mlp_dropout_keep: block (row, unit / 4 | layer << 16), word unit % 4
            const Philox4 ph = philox4x32_10((uint32_t)R, M.drop_call, (uint32_t)(col >> 2) | ((uint32_t)l << 16),
                                             STREAM_MLP_DROPOUT, (uint32_t)M.drop_seed, (uint32_t)(M.drop_seed >> 32));
            const uint32_t w = (col & 3) == 0 ? ph.x : (col & 3) == 1 ? ph.y : (col & 3) == 2 ? ph.z : ph.w;
            v = w >= M.drop_thr ? v * M.drop_scale : 0.f;
          }
          nxt[(4 * q + i) * lda + col] = v;
        } else if (col < N && R < n) {
          stg(out + (size_t)R * out_stride + col, out_apply<2>(v, M.out_act));
        }
      }
    }
    __syncthreads();
    float *t_ = in;
    in = nxt, nxt = t_;
  }
}

// The fragment-major image on its own, into memory the caller owns (csrc/bb_sim.hip: k_bb_episodes reads one
// image for a whole episode).  Layer l starts mlp_image_offset(d, l) floats into wf; l = n_layers: the total.
size_t mlp_image_offset(const iqlhip_mlp_desc &d, int l) {
  size_t total = 0;
  for (int i = 0; i < l; ++i) total += (size_t)round_up(d.dims[i], 16) * round_up(d.dims[i + 1], 16);
  return total;
}

hipError_t launch_mlp_repack(const iqlhip_mlp_desc &d, float *wf, hipStream_t st) {
  RepackArgs R;
  R.n_layers = d.n_layers;
  for (int i = 0; i <= d.n_layers; ++i) R.dims[i] = d.dims[i];
  for (int i = 0; i < d.n_layers; ++i) R.W[i] = d.weights[i], R.Wf[i] = wf + mlp_image_offset(d, i);
  R.w_in_out = d.w_in_out;
  hipLaunchKernelGGL(k_mlp_repack, dim3(64, d.n_layers), dim3(256), 0, st, R);
  return hipGetLastError();
}

// What k_mlp_f32 / k_mlp_set need to know of a shape: everything of MlpArgs but the weight and bias
// pointers, the kernel instantiation (see act_apply) and the dynamic LDS bytes.  maxd: the widest layer
// that passes through the LDS buffer.
static void mlp_geometry(const iqlhip_mlp_desc &d, MlpArgs &M, int &act, size_t &sm, int &maxd) {
  M.n_layers = d.n_layers;
  maxd = 0;
  for (int i = 0; i <= d.n_layers; ++i) {
    M.dims[i] = d.dims[i];
    if (i < d.n_layers && d.dims[i] > maxd) maxd = d.dims[i];
  }
  M.hidden_act = d.hidden_act, M.out_act = d.out_act;
  act = (d.hidden_act >= 8 || d.out_act >= 8) ? 2 : d.hidden_act;
  const int nt_last = round_up(d.dims[d.n_layers], 16) / 16;
  // the table variant's main-path output layer (>= 4 n-tiles) parks its raw sums in the buffer as well
  if (act == 2 && nt_last >= 4 && d.dims[d.n_layers] > maxd) maxd = d.dims[d.n_layers];
  M.lda = round_up(maxd, 16) + 4;
  M.drop_thr = 0, M.drop_scale = 1.f, M.drop_seed = d.dropout_seed, M.drop_call = d.dropout_call;
  if (d.dropout_p > 0.f) {  // the trainer's fp32 convention (host_plan.h dropout_consts): thr = p 2^32, scale = 1 / (1 - p)
    const double thr = (double)d.dropout_p * 4294967296.0;
    M.drop_thr = thr >= 4294967295.0 ? 0xffffffffu : (thr < 1.0 ? 1u : (uint32_t)thr);
    M.drop_scale = 1.0f / (float)(1.0 - (double)d.dropout_p);
  }
  // the activations [64][lda], or the partial tiles of a k-split output layer (4 waves x <= 3 n-tiles)
  sm = (size_t)MROWS * M.lda * sizeof(float);
  if (nt_last < 4 && sm < (size_t)4 * nt_last * 4 * 64 * 16) sm = (size_t)4 * nt_last * 4 * 64 * 16;
}

hipError_t launch_mlp_f32(const iqlhip_mlp_desc &d, const float *x, int64_t n, int x_stride, float *out,
                          int out_stride, hipStream_t st) {
  MlpArgs M;
  int act, maxd;
  size_t sm;
  mlp_geometry(d, M, act, sm, maxd);
  const size_t total = mlp_image_offset(d, d.n_layers);
  float *wf = nullptr;  // stream-ordered scratch for the fragment-major images (<= 8 x 256 KB)
  hipError_t e = hipMallocAsync((void **)&wf, total * sizeof(float), st);
  if (e != hipSuccess) return e;
  for (int i = 0; i < d.n_layers; ++i) M.Wf[i] = wf + mlp_image_offset(d, i), M.b[i] = d.biases[i];
  e = launch_mlp_repack(d, wf, st);
  if (e != hipSuccess) {
    (void)hipFreeAsync(wf, st);
    return e;
  }
  bool wide = false;
  for (int i = 0; i <= d.n_layers; ++i) wide |= d.dims[i] > 256;
  if (wide) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp_wide), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
    if (e == hipSuccess) {
      int maxw = maxd;
      if (d.dims[d.n_layers] > maxw) maxw = d.dims[d.n_layers];
      M.lda = round_up(maxw, 16) + 4;
      hipLaunchKernelGGL(k_mlp_wide, dim3((unsigned)((n + 15) / 16)), dim3(64), (size_t)2 * 16 * M.lda * sizeof(float),
                         st, M, x, n, x_stride, out, out_stride);
      e = hipGetLastError();
    }
    (void)hipFreeAsync(wf, st);
    return e;
  }
  // (set on every call: the attribute is per device, and a process may drive several)
  auto kern = act == 0 ? k_mlp_f32<0> : act == 1 ? k_mlp_f32<1> : k_mlp_f32<2>;
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          160 * 1024);
  if (e == hipSuccess) {
    const int64_t grid = (n + MROWS - 1) / MROWS;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), sm, st, M, x, n, x_stride, out, out_stride);
    e = hipGetLastError();
  }
  (void)hipFreeAsync(wf, st);
  return e;
}

}  // namespace iqlhip

// ---- iqlhip_mlp_set: M MLPs of one shape, repacked once into one allocation ----
// Member m's block starts m * stride floats into `mem`: the fragment-major images of its layers as
// launch_mlp_repack lays them out, then every layer's bias padded to 16 floats.
struct iqlhip_mlp_set {
  iqlhip::MlpSetArgs S;  // S.A: member 0's pointers
  int act;               // kernel instantiation
  size_t sm;             // dynamic LDS bytes
  int M;
  int device;  // the allocation's, and the one the kernel attribute was set on
  float *mem;
};

namespace iqlhip {

struct BiasArgs {
  int32_t n_layers;
  int32_t dims[IQLHIP_MLP_MAX_LAYERS + 1];
  const float *src[IQLHIP_MLP_MAX_LAYERS];
  float *dst[IQLHIP_MLP_MAX_LAYERS];
};

__global__ void k_mlp_set_bias(const BiasArgs B) {
  const int l = blockIdx.x;
  if (l >= B.n_layers) return;
  const int N = B.dims[l + 1], Np = round_up(N, 16);
  for (int c = threadIdx.x; c < Np; c += blockDim.x) B.dst[l][c] = c < N ? B.src[l][c] : 0.f;
}

// The caller (iqlhip_mlp_set_create) has checked the members: one shape, every width <= 256, no dropout, no null
// pointer.
static hipError_t mlp_set_create(const iqlhip_mlp_desc *const *descs, int M, iqlhip_mlp_set **out, hipStream_t st) {
  const iqlhip_mlp_desc &d0 = *descs[0];
  const int L = d0.n_layers;
  const size_t image = mlp_image_offset(d0, L);
  size_t boff[IQLHIP_MLP_MAX_LAYERS], floats = image;
  for (int l = 0; l < L; ++l) boff[l] = floats, floats += round_up(d0.dims[l + 1], 16);
  const size_t stride = (floats + 63) / 64 * 64;  // members on 256-byte boundaries
  iqlhip_mlp_set *s = new (std::nothrow) iqlhip_mlp_set;
  if (!s) return hipErrorOutOfMemory;
  int maxd;
  mlp_geometry(d0, s->S.A, s->act, s->sm, maxd);
  s->S.stride = (int64_t)stride, s->S.R = 0, s->M = M, s->mem = nullptr;
  hipError_t e = hipGetDevice(&s->device);
  if (e == hipSuccess) e = hipMalloc((void **)&s->mem, stride * (size_t)M * sizeof(float));
  for (int m = 0; m < M && e == hipSuccess; ++m) {
    float *base = s->mem + (size_t)m * stride;
    e = launch_mlp_repack(*descs[m], base, st);
    if (e != hipSuccess) break;
    BiasArgs B;
    B.n_layers = L;
    for (int l = 0; l <= L; ++l) B.dims[l] = d0.dims[l];
    for (int l = 0; l < L; ++l) B.src[l] = descs[m]->biases[l], B.dst[l] = base + boff[l];
    hipLaunchKernelGGL(k_mlp_set_bias, dim3(L), dim3(256), 0, st, B);
    e = hipGetLastError();
  }
  for (int l = 0; l < L; ++l) s->S.A.Wf[l] = s->mem + mlp_image_offset(d0, l), s->S.A.b[l] = s->mem + boff[l];
  if (e == hipSuccess) {  // once, here: the forward is one launch and nothing else
    auto kern = s->act == 0 ? k_mlp_set<0> : s->act == 1 ? k_mlp_set<1> : k_mlp_set<2>;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
  }
  // a snapshot: the sources have been read when this returns
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    if (s->mem) (void)hipFree(s->mem);
    delete s;
    return e;
  }
  *out = s;
  return hipSuccess;
}

}  // namespace iqlhip

using namespace iqlhip;

// ------------------------------------------------------------ entry points --
// what iqlhip_mlp_forward and iqlhip_mlp_set_create check alike in a descriptor: the layer count ...
static int mlp_layers_check(const iqlhip_mlp_desc &d) {
  if (d.n_layers < 1 || d.n_layers > IQLHIP_MLP_MAX_LAYERS)
    return fail(IQLHIP_ERR_INVALID, "n_layers must be in [1, %d]", IQLHIP_MLP_MAX_LAYERS);
  return 0;
}
// ... and the activation codes
static int mlp_act_check(const iqlhip_mlp_desc &d) {
  for (int a : {d.hidden_act, d.out_act})
    if (a < 0 || (a > 1 && a < 8) || a > 15) return fail(IQLHIP_ERR_INVALID, "activation code %d", a);
  return 0;
}

extern "C" int iqlhip_mlp_forward(const iqlhip_mlp_desc *d, const float *x, int64_t n, int32_t x_stride,
                                  float *out, int32_t out_stride, void *stream) {
  if (!d || !x || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n <= 0) return fail(IQLHIP_ERR_INVALID, "n must be positive");
  if (int rc = mlp_layers_check(*d)) return rc;
  for (int i = 0; i <= d->n_layers; ++i)
    if (d->dims[i] <= 0 || d->dims[i] > 1024)
      return fail(IQLHIP_ERR_UNSUPPORTED, "layer width %d outside [1, 1024]", d->dims[i]);
  for (int i = 0; i < d->n_layers; ++i)
    if (!d->weights[i] || !d->biases[i]) return fail(IQLHIP_ERR_INVALID, "null weight pointer");
  if (int rc = mlp_act_check(*d)) return rc;
  if (x_stride < d->dims[0] || out_stride < d->dims[d->n_layers])
    return fail(IQLHIP_ERR_INVALID, "stride smaller than the row width");
  if (!(d->dropout_p < 1.0f)) return fail(IQLHIP_ERR_INVALID, "dropout_p must be < 1");
  if (d->dropout_p > 0.f && n > 0xffffffffLL) return fail(IQLHIP_ERR_UNSUPPORTED, "dropout: n must fit 32 bits");
  HIP_TRY(launch_mlp_f32(*d, x, n, x_stride, out, out_stride, (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_mlp_set_create(const iqlhip_mlp_desc *const *descs, int32_t M, iqlhip_mlp_set **out,
                                     void *stream) {
  if (!descs || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (M < 1 || M > IQLHIP_MLP_SET_MAX)
    return fail(IQLHIP_ERR_INVALID, "M = %d outside [1, %d]", M, IQLHIP_MLP_SET_MAX);
  for (int m = 0; m < M; ++m)
    if (!descs[m]) return fail(IQLHIP_ERR_INVALID, "member %d: null descriptor", m);
  const iqlhip_mlp_desc &d0 = *descs[0];
  if (int rc = mlp_layers_check(d0)) return rc;
  for (int i = 0; i <= d0.n_layers; ++i) {
    if (d0.dims[i] <= 0) return fail(IQLHIP_ERR_INVALID, "layer width %d", d0.dims[i]);
    if (d0.dims[i] > 256)
      return fail(IQLHIP_ERR_UNSUPPORTED, "layer width %d > 256: iqlhip_mlp_forward takes it", d0.dims[i]);
  }
  if (int rc = mlp_act_check(d0)) return rc;
  for (int m = 0; m < M; ++m) {
    const iqlhip_mlp_desc &d = *descs[m];
    bool same = d.n_layers == d0.n_layers && d.w_in_out == d0.w_in_out && d.hidden_act == d0.hidden_act &&
                d.out_act == d0.out_act;
    for (int i = 0; same && i <= d0.n_layers; ++i) same = d.dims[i] == d0.dims[i];
    if (!same) return fail(IQLHIP_ERR_INVALID, "member %d differs from member 0 in shape, activation or layout", m);
    for (int i = 0; i < d.n_layers; ++i)
      if (!d.weights[i] || !d.biases[i]) return fail(IQLHIP_ERR_INVALID, "member %d: null weight pointer", m);
    if (d.dropout_p > 0.f)
      return fail(IQLHIP_ERR_UNSUPPORTED, "member %d: dropout_p > 0 (the set is an eval-mode forward)", m);
  }
  HIP_TRY(mlp_set_create(descs, M, out, (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_mlp_set_destroy(iqlhip_mlp_set *set) {
  if (!set) return fail(IQLHIP_ERR_INVALID, "null set");
  float *mem = set->mem;
  delete set;
  HIP_TRY(hipFree(mem));  // (waits for the work that still reads it)
  return 0;
}

extern "C" int iqlhip_mlp_set_forward(const iqlhip_mlp_set *set, const float *x, int32_t R, int32_t x_stride,
                                      float *out, int32_t out_stride, void *stream) {
  if (!set || !x || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (R < 1) return fail(IQLHIP_ERR_INVALID, "R = %d must be positive", R);
  const int in = set->S.A.dims[0], width = set->S.A.dims[set->S.A.n_layers];
  if (x_stride < in || out_stride < width) return fail(IQLHIP_ERR_INVALID, "stride smaller than the row width");
  int current;
  HIP_TRY(hipGetDevice(&current));  // (no launch, no wait: the set's images live on one device)
  if (current != set->device)
    return fail(IQLHIP_ERR_INVALID, "the set lives on device %d, the current device is %d", set->device, current);
  MlpSetArgs S = set->S;
  S.R = R;
  auto kern = set->act == 0 ? k_mlp_set<0> : set->act == 1 ? k_mlp_set<1> : k_mlp_set<2>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(((int64_t)R + MROWS - 1) / MROWS), (unsigned)set->M), dim3(256), set->sm,
                     (hipStream_t)stream, S, x, x_stride, out, out_stride);
  HIP_TRY(hipGetLastError());
  return 0;
}
