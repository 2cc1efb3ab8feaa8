// Preference-transformer relabel for any depth and width of the general envelope (include/iqlhip.h):
// the layer-wise path beside the one-block streaming kernel of pt.hip, as iql_deep.hip stands
// beside iql_step.hip.  Same quantity (value[:, 0, -1, 0] of PT.__call__ in eval mode,
// reward_models/pref_transformer.py:210-277) and the same rounding points (oracle/relabel_oracle.py
// pt_value_last): q and k rounded to bf16, the q.k sum rounded to bf16, the 1/sqrt(head_dim) scale
// applied and rounded in bf16, fp32 everywhere else.
//
// A one-query streaming kernel cannot run more than one block: every block before the last needs
// the hidden state of EVERY real token.  So a chunk of windows is processed layer by layer, its
// token matrices in the caller's workspace, one window = tp = round_up(2 ql, RT) token rows:
//   embed        tokens s0 a0 s1 a1 .. of the window's real transitions: [s | a] . [Ws ; Wa] + bias
//                + timestep embedding, stacked LayerNorm                                   -> X
//   per block    LN0 + QKV GEMM -> QKV; causal attention per (window, head, query) -> O;
//                X += O . Wo^T + b;  H = relu(LN1(X) . Win^T + b);  X += H . Wout^T + b
//   last block   keys and values of every token, but the query, attention output, MLP and final
//                LayerNorm only for the last action token: its row is gathered (Xl) and the tail
//                runs on one row per window; value head = last row of pref_linear.
// Right alignment: the reference left-pads a window to ql; the pads are never materialised.  A real
// query gets -1e4 added to every pad key (ops.py:6-11, the additive mask) and, after the max
// subtraction, exp of a logit near -1e4 is exactly 0 in fp32, so no pad ever reaches a real token
// at any layer (pt.hip relies on the same fact).  Likewise the causally masked keys (-1e4 fill).
// Tokens are stored from row 0 of the window; rows past 2 len are never read by a real row.
//
// Linears run on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32): a work-group takes RT = 32
// rows and up to 256 output columns (four 16-column tiles per wave, two 16-row tiles each: eight
// independent accumulators), A staged in LDS in 256-deep chunks, B straight from the torch-layout
// weights (16 bytes per lane, L2 resident).
#include <algorithm>

#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"

namespace iqlhip {
namespace ptg {

constexpr int RT = 32;        // token rows per GEMM tile (two MFMA m-tiles)
constexpr int NB = 256;       // output columns per work-group
constexpr int KC = 256;       // depth of one A chunk in LDS
constexpr int LDA = KC + 4;   // its row stride (conflict-free 16-byte fragment reads)
constexpr int THREADS = 256;  // four waves

// the windows of one chunk (pointers already offset to its first window)
struct Chunk {
  const float *obs, *act;
  int64_t n_rows;
  const int64_t *win_start;
  const int32_t *win_len, *win_t0;
  int64_t nw;  // windows in the chunk
  int ql, tp, n_temb;
};

struct Win {
  int64_t start;
  int len, t0;
};

// A window clamped exactly as k_pt_relabel's load_window does: no row of obs / act and no entry of
// the timestep table outside the arrays is ever addressed, whatever the caller hands in; valid
// windows pass through unchanged.
__device__ __forceinline__ Win load_window(const Chunk &c, int64_t w) {
  int l = c.win_len[w];
  const int64_t cap = c.n_rows < (int64_t)c.n_temb ? c.n_rows : (int64_t)c.n_temb;
  l = l > c.ql ? c.ql : l;
  l = (int64_t)l > cap ? (int)cap : l;
  l = l < 1 ? 1 : l;
  int64_t s0 = c.win_start[w];
  s0 = s0 < 0 ? 0 : (s0 > c.n_rows - l ? c.n_rows - l : s0);
  int t = c.win_t0 ? c.win_t0[w] : 0;
  t = t < 0 ? 0 : (t > c.n_temb - l ? c.n_temb - l : t);
  return Win{s0, l, t};
}

enum { EMBED = 0, LN_IN = 1, PLAIN = 2 };

struct Lin {
  const float *a;  // A [rows][lda] (LN_IN / PLAIN)
  int64_t lda;
  const float *w, *b;  // [N][K] torch layout, [N]
  int K, N;
  const float *ln_w, *ln_b;  // LN_IN: LayerNorm of the A rows (K = E); EMBED: stacked LN of the output
  float eps;
  float *y;  // [rows][ldy]
  int64_t ldy;
  int relu, residual;  // y = relu(acc + b) or y += acc + b
  // EMBED: B = [state_wT ; action_wT] ([S + A][E]), per-kind bias, timestep table
  const float *swT, *sb, *awT, *ab, *temb;
  int S, A;
};

// Y = epilogue(A' . W^T + b) for one tile of RT rows x up to NB columns.  tokens != 0: the rows are
// the token rows of the chunk (tp per window) and a tile wholly past a window's 2 len real tokens
// is skipped; tokens == 0: plain rows (one per window, the last-token tail).
template <int MODE>
__global__ __launch_bounds__(THREADS) void k_lin(const Lin p, const Chunk c, int tokens) {
  __shared__ __attribute__((aligned(16))) float at[RT * LDA];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * RT;
  Win win{0, 1, 0};
  int j0 = 0;
  if (tokens) {
    const int64_t w = row0 / c.tp;
    j0 = (int)(row0 - w * c.tp);
    win = load_window(c, w);
    if (j0 >= 2 * win.len) return;  // (uniform over the work-group)
  }
  const int n0 = blockIdx.y * NB;
  const int ntl = (p.N - n0 < NB ? p.N - n0 : NB) / 16;  // n-tiles of this work-group
  const int K = MODE == EMBED ? p.S + p.A : p.K;
  const int E = p.N;  // (EMBED: the output width is embd_dim)

  f32x4 acc[4][2];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s][0] = acc[s][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = K - k0 < KC ? K - k0 : KC;
    const int kcp = round_up(kc, 16);
    __syncthreads();  // the previous chunk is consumed
    for (int e = tid; e < RT * kcp; e += THREADS) {
      const int rr = e / kcp, k = e - rr * kcp;
      float v = 0.f;
      if (k < kc) {
        if (MODE == EMBED) {
          // token j of the window: the state (j even) or action (j odd) of transition j / 2; rows
          // past the real tokens repeat the last one (their results are never read)
          const int j = j0 + rr < 2 * win.len ? j0 + rr : 2 * win.len - 1;
          const int64_t t = win.start + (j >> 1);
          const int kk = k0 + k;
          if (j & 1)
            v = kk >= p.S ? ldg(c.act + t * p.A + (kk - p.S)) : 0.f;
          else
            v = kk < p.S ? ldg(c.obs + t * p.S + kk) : 0.f;
        } else {
          v = ldg(p.a + (row0 + rr) * p.lda + k0 + k);
        }
      }
      at[rr * LDA + k] = v;
    }
    __syncthreads();
    if (MODE == LN_IN) {  // K = E <= KC: one chunk; LayerNorm of each row in place (oracle _ln)
      for (int rr = wave; rr < RT; rr += THREADS / 64) {
        float *x = at + rr * LDA;
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += x[k];
        const float mu = lane_sum<64>(s) / (float)K;
        float v = 0.f;
        for (int k = lane; k < K; k += 64) v += (x[k] - mu) * (x[k] - mu);
        const float sd = sqrtf(lane_sum<64>(v) / (float)K + p.eps);
        for (int k = lane; k < K; k += 64) x[k] = (x[k] - mu) / sd * ldg(p.ln_w + k) + ldg(p.ln_b + k);
      }
      __syncthreads();
    }
    for (int ks = 0; ks < kcp / 16; ++ks) {
      const f32x4 a0 = *reinterpret_cast<const f32x4 *>(at + r * LDA + 16 * ks + 4 * q);
      const f32x4 a1 = *reinterpret_cast<const f32x4 *>(at + (16 + r) * LDA + 16 * ks + 4 * q);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int nt = wave + 4 * s;
        if (nt < ntl) {
          const int n = n0 + 16 * nt + r;
          float bw[4];
          if (MODE == EMBED) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int k = k0 + 16 * ks + 4 * q + i;
              bw[i] = k < p.S ? ldg(p.swT + (size_t)k * E + n)
                              : (k < p.S + p.A ? ldg(p.awT + (size_t)(k - p.S) * E + n) : 0.f);
            }
          } else {
            const float4 b4 = __builtin_bit_cast(float4, ldg16(p.w + (size_t)n * p.K + k0 + 16 * ks + 4 * q));
            bw[0] = b4.x, bw[1] = b4.y, bw[2] = b4.z, bw[3] = b4.w;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i], bw[i], acc[s][0], 0, 0, 0);
            acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i], bw[i], acc[s][1], 0, 0, 0);
          }
        }
      }
    }
  }

  // C layout: acc[s][m][i] = row 16 m + 4 q + i, column n0 + 16 (wave + 4 s) + r
  if (MODE == EMBED) {  // (one work-group column: N = E <= NB)
    __syncthreads();    // every wave is done with the A chunk
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int nt = wave + 4 * s;
      if (nt < ntl) {
        const int n = 16 * nt + r;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int rr = 16 * m + 4 * q + i;
            const int j = j0 + rr < 2 * win.len ? j0 + rr : 2 * win.len - 1;
            const float bias = (j & 1) ? ldg(p.ab + n) : ldg(p.sb + n);
            const float te = ldg(p.temb + (size_t)(win.t0 + (j >> 1)) * E + n);
            at[rr * LDA + n] = (acc[s][m][i] + bias) + te;
          }
      }
    }
    __syncthreads();
    for (int rr = wave; rr < RT; rr += THREADS / 64) {  // stacked_layer_norm
      const float *x = at + rr * LDA;
      float s = 0.f;
      for (int k = lane; k < E; k += 64) s += x[k];
      const float mu = lane_sum<64>(s) / (float)E;
      float v = 0.f;
      for (int k = lane; k < E; k += 64) v += (x[k] - mu) * (x[k] - mu);
      const float sd = sqrtf(lane_sum<64>(v) / (float)E + p.eps);
      float *y = p.y + (row0 + rr) * p.ldy;
      for (int k = lane; k < E; k += 64) stg(y + k, (x[k] - mu) / sd * ldg(p.ln_w + k) + ldg(p.ln_b + k));
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int nt = wave + 4 * s;
      if (nt < ntl) {
        const int n = n0 + 16 * nt + r;
        const float bias = ldg(p.b + n);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float *yp = p.y + (row0 + 16 * m + 4 * q + i) * p.ldy + n;
            float v = acc[s][m][i] + bias;
            if (p.relu) v = fmaxf(v, 0.f);
            if (p.residual) v += ldg(yp);
            stg(yp, v);
          }
      }
    }
  }
}

// Causal attention, one wave per (window, head, query row).  The head's HD features spread over
// HDL lanes, HDL = the largest power of two <= 64 that divides HD (embd_dim 192 makes HD = 3 * 2^k),
// feature d + HDL u in lane d, u < HD / HDL <= 4; the wave's G = 64 / HDL lane groups take keys
// g, g + G, .. of the causal prefix 0..i, each with a lane-local online softmax, and meet at the
// end.  Only real keys are visited: the pads and the future keys contribute exactly 0 (see top).
// last_only: the query is the window's last action token and the output row is the window's.
__global__ __launch_bounds__(THREADS) void k_attn(const float *__restrict__ qkv, float *__restrict__ o,
                                                   const Chunk c, int E, int NH, int last_only) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  int64_t w, orow;
  int h, i;
  if (last_only) {
    w = gw / NH, h = (int)(gw - w * NH);
    if (w >= c.nw) return;
    i = 2 * load_window(c, w).len - 1;
    orow = w;
  } else {
    const int64_t per = (int64_t)NH * c.tp;
    w = gw / per;
    const int rem = (int)(gw - w * per);
    h = rem / c.tp, i = rem - h * c.tp;
    if (w >= c.nw || i >= 2 * load_window(c, w).len) return;
    orow = w * c.tp + i;
  }
  const int HD = E / NH, HDL = (HD & -HD) < 64 ? (HD & -HD) : 64, DPL = HD / HDL, G = 64 / HDL;
  const int g = lane / HDL, col = h * HD + (lane - g * HDL);
  const int ld = 3 * E;
  const float *base = qkv + (size_t)w * c.tp * ld;
  float qv[4], ov[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) qv[u] = u < DPL ? rbf(ldg(base + (size_t)i * ld + col + HDL * u)) : 0.f, ov[u] = 0.f;
  const float sqrt_hd = sqrtf((float)HD);
  float m = -3.0e38f, l = 0.f;
  for (int jb = 0; jb <= i; jb += G) {  // (uniform trip count: the lane sums below span whole groups)
    const int j = jb + g;
    const bool valid = j <= i;
    const float *kr = base + (size_t)(valid ? j : i) * ld + E + col;
    float pr = 0.f;  // bf16 x bf16 products are exact in fp32
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < DPL) pr = fmaf(qv[u], rbf(ldg(kr + HDL * u)), pr);
    pr = lane_sum_rt(pr, HDL);
    const float s = rbf(rbf(pr) / sqrt_hd);  // ops.py:74-79
    if (valid) {
      const float mn = fmaxf(m, s);
      const float c_old = __expf(m - mn), pw = __expf(s - mn);
      l = l * c_old + pw;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < DPL) ov[u] = ov[u] * c_old + pw * ldg(kr + E + HDL * u);
      m = mn;
    }
  }
  for (int off = HDL; off < 64; off <<= 1) {  // the lane groups meet (once per query)
    const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
    const float mn = fmaxf(m, m2), c1 = __expf(m - mn), c2 = __expf(m2 - mn);
    l = l * c1 + l2 * c2;
#pragma unroll
    for (int u = 0; u < 4; ++u) ov[u] = ov[u] * c1 + __shfl_xor(ov[u], off) * c2;
    m = mn;
  }
  if (g == 0) {
    float *op = o + orow * E + col;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < DPL) stg(op + HDL * u, ov[u] / l);
  }
}

// Xl[w] = X[row of the window's last action token]
__global__ __launch_bounds__(THREADS) void k_last_rows(const float *__restrict__ x, float *__restrict__ xl,
                                                        const Chunk c, int E) {
  const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t w = e / E;
  if (w >= c.nw) return;
  const int f = (int)(e - w * E);
  const int last = 2 * load_window(c, w).len - 1;
  stg(xl + e, ldg(x + (w * c.tp + last) * E + f));
}

// out[w] = final LayerNorm of the window's last action token . last row of pref_linear + bias
__global__ __launch_bounds__(THREADS) void k_value_head(const float *__restrict__ xl, const Chunk c, int E,
                                                         const float *lnf_w, const float *lnf_b,
                                                         const float *pw, float pb, float eps,
                                                         float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (w >= c.nw) return;
  float x[4];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = lane + 64 * u;
    x[u] = k < E ? ldg(xl + w * E + k) : 0.f;
    s += x[u];
  }
  const float mu = lane_sum<64>(s) / (float)E;
  float v = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (lane + 64 * u < E) v += (x[u] - mu) * (x[u] - mu);
  const float sd = sqrtf(lane_sum<64>(v) / (float)E + eps);
  float d = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = lane + 64 * u;
    if (k < E) d += ((x[u] - mu) / sd * ldg(lnf_w + k) + ldg(lnf_b + k)) * ldg(pw + k);
  }
  d = lane_sum<64>(d);
  if (lane == 0) stg(out + w, d + pb);
}

// ---- workspace: per window X [tp][E], QKV [tp][3E], O / H [tp][max(E, I)]; per tail row (windows
// rounded up to RT) Xl [E], Ol [E], Hl [max(E, I)] ----
static int64_t tok_floats(const iqlhip_pt_model &m, int tp) {
  const int mx = m.inter_dim > m.embd_dim ? m.inter_dim : m.embd_dim;
  return (int64_t)tp * (4 * m.embd_dim + mx);
}
static int64_t tail_floats(const iqlhip_pt_model &m) {
  const int mx = m.inter_dim > m.embd_dim ? m.inter_dim : m.embd_dim;
  return 2 * m.embd_dim + mx;
}

template <int MODE>
static void lin(const Lin &p, const Chunk &c, int64_t rows, int tokens, hipStream_t st) {
  hipLaunchKernelGGL(k_lin<MODE>, dim3((unsigned)(rows / RT), (unsigned)((p.N + NB - 1) / NB)), dim3(THREADS), 0, st,
                     p, c, tokens);
}

}  // namespace ptg

static int pt_general_tp(int ql) { return round_up(2 * ql, ptg::RT); }

static size_t pt_general_bytes(const iqlhip_pt_model &m, int ql, int64_t nw) {
  const int64_t tail_rows = (nw + ptg::RT - 1) / ptg::RT * ptg::RT;
  return (size_t)(nw * ptg::tok_floats(m, pt_general_tp(ql)) + tail_rows * ptg::tail_floats(m)) * 4;
}

// windows a workspace of `bytes` holds (0: not even one)
static int64_t pt_general_fit(const iqlhip_pt_model &m, int ql, size_t bytes) {
  const int64_t per = ptg::tok_floats(m, pt_general_tp(ql)) + ptg::tail_floats(m);
  const int64_t pad = (ptg::RT - 1) * ptg::tail_floats(m);
  const int64_t fl = (int64_t)(bytes / 4);
  return fl <= pad ? 0 : (fl - pad) / per;
}

static hipError_t launch_pt_general(const iqlhip_pt_model &m, const float *obs, const float *act, int64_t n_rows,
                                    const int64_t *win_start, const int32_t *win_len, const int32_t *win_t0,
                                    int64_t n_win, int ql, float *ws, int64_t chunk, float *out, hipStream_t st) {
  using namespace ptg;
  const int E = m.embd_dim, I = m.inter_dim, NH = m.num_heads, tp = pt_general_tp(ql);
  const int mx = I > E ? I : E;
  const int64_t rows_cap = chunk * tp, tail_cap = (chunk + RT - 1) / RT * RT;
  float *X = ws, *QKV = X + rows_cap * E, *OH = QKV + rows_cap * 3 * E;
  float *Xl = OH + rows_cap * mx, *Ol = Xl + tail_cap * E, *Hl = Ol + tail_cap * E;
  for (int64_t w0 = 0; w0 < n_win; w0 += chunk) {
    Chunk c{obs, act, n_rows, win_start + w0, win_len + w0, win_t0 ? win_t0 + w0 : nullptr,
            n_win - w0 < chunk ? n_win - w0 : chunk, ql, tp, m.n_temb};
    const int64_t rows = c.nw * tp, trows = (c.nw + RT - 1) / RT * RT;
    {
      Lin p{};
      p.N = E, p.ln_w = m.sln_w, p.ln_b = m.sln_b, p.eps = m.eps, p.y = X, p.ldy = E;
      p.swT = m.state_wT, p.sb = m.state_b, p.awT = m.action_wT, p.ab = m.action_b, p.temb = m.temb;
      p.S = m.state_dim, p.A = m.action_dim;
      lin<EMBED>(p, c, rows, 1, st);
    }
    for (int l = 0; l < m.num_layers; ++l) {
      const iqlhip_pt_block &B = m.blocks[l];
      const bool last = l == m.num_layers - 1;
      Lin p{};
      p.eps = m.eps;
      // LN0 + QKV for every token (the last block needs every key and value)
      p.a = X, p.lda = E, p.w = B.qkv_w, p.b = B.qkv_b, p.K = E, p.N = 3 * E, p.ln_w = B.ln0_w, p.ln_b = B.ln0_b;
      p.y = QKV, p.ldy = 3 * E;
      lin<LN_IN>(p, c, rows, 1, st);
      float *xr = X, *orow = OH, *hrow = OH;
      int64_t nrows = rows;
      int tokens = 1;
      if (last) {  // from here on one row per window: its last action token
        hipLaunchKernelGGL(k_last_rows, dim3((unsigned)((c.nw * E + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, X,
                           Xl, c, E);
        hipLaunchKernelGGL(k_attn, dim3((unsigned)((c.nw * NH + 3) / 4)), dim3(THREADS), 0, st, QKV, Ol, c, E, NH, 1);
        xr = Xl, orow = Ol, hrow = Hl, nrows = trows, tokens = 0;
      } else {
        hipLaunchKernelGGL(k_attn, dim3((unsigned)(c.nw * NH * tp / 4)), dim3(THREADS), 0, st, QKV, OH, c, E, NH, 0);
      }
      // X += O . Wo^T + b
      p = Lin{};
      p.eps = m.eps;
      p.a = orow, p.lda = E, p.w = B.attn_out_w, p.b = B.attn_out_b, p.K = E, p.N = E, p.y = xr, p.ldy = E;
      p.residual = 1;
      lin<PLAIN>(p, c, nrows, tokens, st);
      // H = relu(LN1(X) . Win^T + b)   (H overwrites O: the out projection has consumed it)
      p = Lin{};
      p.eps = m.eps;
      p.a = xr, p.lda = E, p.w = B.mlp_in_w, p.b = B.mlp_in_b, p.K = E, p.N = I, p.ln_w = B.ln1_w, p.ln_b = B.ln1_b;
      p.y = hrow, p.ldy = I, p.relu = 1;
      lin<LN_IN>(p, c, nrows, tokens, st);
      // X += H . Wout^T + b
      p = Lin{};
      p.eps = m.eps;
      p.a = hrow, p.lda = I, p.w = B.mlp_out_w, p.b = B.mlp_out_b, p.K = I, p.N = E, p.y = xr, p.ldy = E;
      p.residual = 1;
      lin<PLAIN>(p, c, nrows, tokens, st);
    }
    hipLaunchKernelGGL(k_value_head, dim3((unsigned)((c.nw + 3) / 4)), dim3(THREADS), 0, st, Xl, c, E, m.lnf_w,
                       m.lnf_b, m.pref_w_last, m.pref_b_last, m.eps, out + w0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace iqlhip

using namespace iqlhip;

// ---- entry points: host-only shape checks, then the chunked launches ----
static constexpr size_t PT_GENERAL_BUDGET = size_t(1) << 30;  // workspace of one full chunk

static int pt_general_check(const iqlhip_pt_model *m, int32_t query_length) {
  if (!m) return fail(IQLHIP_ERR_INVALID, "null model");
  if (m->num_layers < 1 || m->num_layers > 8)
    return fail(IQLHIP_ERR_UNSUPPORTED, "num_layers %d: the general path takes 1..8", m->num_layers);
  const int E = m->embd_dim, nh = m->num_heads;
  if (E < 64 || E > 256 || E % 64)
    return fail(IQLHIP_ERR_UNSUPPORTED, "embd_dim %d: must be a multiple of 64 up to 256", E);
  if (nh < 1 || (nh & (nh - 1)) || E / nh < 4)
    return fail(IQLHIP_ERR_UNSUPPORTED, "num_heads %d: must be a power of two with embd_dim / num_heads >= 4", nh);
  if (m->inter_dim < 64 || m->inter_dim > 1024 || m->inter_dim % 64)
    return fail(IQLHIP_ERR_UNSUPPORTED, "inter_dim %d: must be a multiple of 64 up to 1024", m->inter_dim);
  if (m->state_dim < 1 || m->action_dim < 1 || m->state_dim + m->action_dim > 256)
    return fail(IQLHIP_ERR_UNSUPPORTED, "state_dim %d + action_dim %d: must be <= 256", m->state_dim, m->action_dim);
  if (query_length < 1) return fail(IQLHIP_ERR_INVALID, "query_length must be positive");
  if (query_length > 4096) return fail(IQLHIP_ERR_UNSUPPORTED, "query_length %d > 4096", query_length);
  if (m->n_temb < 1) return fail(IQLHIP_ERR_INVALID, "empty timestep table");
  if (!m->blocks) return fail(IQLHIP_ERR_INVALID, "null block array");
  const float *top[] = {m->state_wT, m->state_b, m->action_wT, m->action_b, m->temb, m->sln_w, m->sln_b,
                        m->lnf_w, m->lnf_b, m->pref_w_last};
  for (const float *t : top)
    if (!t) return fail(IQLHIP_ERR_INVALID, "null weight pointer");
  for (int l = 0; l < m->num_layers; ++l) {
    const iqlhip_pt_block &b = m->blocks[l];
    const float *blk[] = {b.ln0_w, b.ln0_b, b.qkv_w, b.qkv_b, b.attn_out_w, b.attn_out_b,
                          b.ln1_w, b.ln1_b, b.mlp_in_w, b.mlp_in_b, b.mlp_out_w, b.mlp_out_b};
    for (const float *t : blk)
      if (!t) return fail(IQLHIP_ERR_INVALID, "null weight pointer in block %d", l);
  }
  return 0;
}

// windows of one full chunk: what 1 GiB holds (at least one), and few enough that the attention
// grid (one wave per head and token row) stays far inside 2^31 work-groups
static int64_t pt_general_cap(const iqlhip_pt_model &m, int ql) {
  int64_t cap = pt_general_fit(m, ql, PT_GENERAL_BUDGET);
  const int64_t grid_cap = ((int64_t)1 << 30) / ((int64_t)m.num_heads * pt_general_tp(ql));
  cap = std::min<int64_t>(cap, std::min<int64_t>(grid_cap, 65536));
  return std::max<int64_t>(cap, 1);
}

extern "C" int iqlhip_pt_general_workspace_bytes(const iqlhip_pt_model *m, int32_t query_length, int64_t n_win,
                                                 size_t *bytes) {
  if (!bytes) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = pt_general_check(m, query_length)) return rc;
  if (n_win <= 0) return fail(IQLHIP_ERR_INVALID, "n_win must be positive");
  *bytes = pt_general_bytes(*m, query_length, std::min(n_win, pt_general_cap(*m, query_length)));
  return 0;
}

extern "C" int iqlhip_pt_relabel_general(const iqlhip_pt_model *m, const float *obs, const float *act,
                                         int64_t n_rows, const int64_t *win_start, const int32_t *win_len,
                                         const int32_t *win_t0, int64_t n_win, int32_t query_length,
                                         void *workspace, size_t workspace_bytes, float *out, void *stream) {
  if (int rc = pt_general_check(m, query_length)) return rc;
  if (!obs || !act || !win_start || !win_len || !out || !workspace) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n_win <= 0 || n_rows <= 0) return fail(IQLHIP_ERR_INVALID, "empty problem");
  if (!win_t0 && query_length > m->n_temb)
    return fail(IQLHIP_ERR_INVALID, "query_length exceeds the timestep table");
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(IQLHIP_ERR_INVALID, "workspace not 16-byte aligned");
  const int64_t chunk = std::min(std::min(n_win, pt_general_cap(*m, query_length)),
                                 pt_general_fit(*m, query_length, workspace_bytes));
  if (chunk < 1)
    return fail(IQLHIP_ERR_INVALID, "workspace of %zu bytes holds no window (one needs %zu)", workspace_bytes,
                pt_general_bytes(*m, query_length, 1));
  HIP_TRY(launch_pt_general(*m, obs, act, n_rows, win_start, win_len, win_t0, n_win, query_length,
                            static_cast<float *>(workspace), chunk, out, (hipStream_t)stream));
  return 0;
}
