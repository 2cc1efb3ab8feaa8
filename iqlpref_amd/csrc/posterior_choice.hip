// The posterior relabel of algorithms/custom_offline/iql_br.py:179-253 after the [S][N] prediction matrix:
// per transition c, n_samps draws of np.random.choice(preds[:, c], n_samps) on numpy's legacy global
// generator -- which is row[randint(0, S, n_samps)], N rows in order being ONE randint stream of
// N * n_samps values -- reduced to their mean or median.  The index matrix never exists in full.
//
// Two kernels per chunk of `rows` transitions, on two streams:
//   k_choice_draw    one work-group continues the MT19937 stream (np_draw_stream, the code of
//                    k_np_randint) for rows * n_samps accepted values, stored as uint16 into one slot of
//                    a ring of CH_RING slots in the caller's workspace; the state goes back to global
//                    memory after every chunk, so chunk c + 1 starts where chunk c stopped;
//   k_choice_reduce  chip-wide, behind an event: a work-group stages the S predictions of a tile of TR
//                    adjacent transitions once (coalesced along the transitions, LDS [TR][S|1] so that
//                    both the staging stores and the random gathers spread over the banks), then one
//                    wave per transition gathers its n_samps values (lane l holds samples l, l + 64, ..)
//                    and reduces them: MEAN = lane sums + butterfly, / n; MEDIAN = rank counting --
//                    every value is broadcast from its lane (v_readlane) and each lane counts how many
//                    precede each of its own in the order (value, sample index), a strict total order, so
//                    exactly one value has rank (n - 1) / 2 and one n / 2.
//   n_samps == 1 needs no tile: k_choice_first reads preds[idx[c]][c], lanes on adjacent transitions.
// The draw of chunk c + CH_RING waits for the reduce of chunk c (its slot); the reduce of the last
// chunks is all that does not hide behind the serial draw.
#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"
#include "np_stream.h"

namespace iqlhip {

constexpr int CH_RING = 4;              // index slots in the workspace
constexpr int64_t CH_VALUES = 1 << 20;  // accepted values per chunk (2 MiB of uint16 per slot)
constexpr int CH_ROW_ALIGN = 32;        // chunk rows: a multiple of the widest tile
constexpr int CH_THREADS = 256, CH_WAVES = CH_THREADS / 64;
constexpr size_t CH_TILE_LDS = 80 * 1024;  // two work-groups per CU

__global__ __launch_bounds__(NP_THREADS) void k_choice_draw(uint32_t *__restrict__ state,
                                                             uint16_t *__restrict__ idx, uint32_t rng,
                                                             uint32_t mask, int64_t total) {
  np_draw_stream<uint16_t>(state, idx, rng, mask, total);
}

// n_samps == 1: out[row0 + r] = preds[idx[r]][row0 + r]
__global__ __launch_bounds__(CH_THREADS) void k_choice_first(const float *__restrict__ preds,
                                                              const uint16_t *__restrict__ idx, int S, int64_t N,
                                                              int64_t row0, int rows, float *__restrict__ out) {
  const int r = blockIdx.x * CH_THREADS + threadIdx.x;
  if (r >= rows) return;
  const int s = min((int)idx[r], S - 1);
  out[row0 + r] = preds[(int64_t)s * N + row0 + r];
}

// K = ceil(n / 64) rounded up to a power of two: samples per lane.  TR: transitions per tile (power of
// two), SP = S | 1: LDS row pitch.  idx: this chunk's [rows][n] indices; row0: its first transition.
template <int K>
__global__ __launch_bounds__(CH_THREADS) void k_choice_reduce(const float *__restrict__ preds,
                                                               const uint16_t *__restrict__ idx, int S, int64_t N,
                                                               int64_t row0, int rows, int n, int tr_log2, int SP,
                                                               int mode, float *__restrict__ out) {
  extern __shared__ float tile[];  // [TR][SP]
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int TR = 1 << tr_log2;
  const int first = blockIdx.x * TR;  // first row of the tile inside the chunk
  const int nr = min(TR, rows - first);
  const float *src = preds + row0 + first;
  for (int e = t; e < S * TR; e += CH_THREADS) {
    const int s = e >> tr_log2, r = e & (TR - 1);
    if (r < nr) tile[r * SP + s] = src[(int64_t)s * N + r];
  }
  __syncthreads();
  for (int r = wave; r < nr; r += CH_WAVES) {
    const uint16_t *ix = idx + (int64_t)(first + r) * n;
    const float *row = tile + r * SP;
    float a[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int j = lane + 64 * i;
      a[i] = j < n ? row[min((int)ix[j], S - 1)] : 0.f;
    }
    float res;
    if (mode == IQLHIP_CHOICE_MEAN) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < K; ++i) s += lane + 64 * i < n ? a[i] : 0.f;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
      res = s / (float)n;
    } else {
      int rank[K];
#pragma unroll
      for (int i = 0; i < K; ++i) rank[i] = 0;
#pragma unroll
      for (int i2 = 0; i2 < K; ++i2) {
        const int m = min(64, n - 64 * i2);  // (wave-uniform) samples held in register i2
        for (int l = 0; l < m; ++l) {
          const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[i2]), l));
          const int jv = l + 64 * i2;
#pragma unroll
          for (int i = 0; i < K; ++i) rank[i] += (v < a[i] || (v == a[i] && jv < lane + 64 * i)) ? 1 : 0;
        }
      }
      const int lo = (n - 1) >> 1, hi = n >> 1;
      float vlo = 0.f, vhi = 0.f;
      bool has_lo = false, has_hi = false;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const bool live = lane + 64 * i < n;
        if (live && rank[i] == lo) vlo = a[i], has_lo = true;
        if (live && rank[i] == hi) vhi = a[i], has_hi = true;
      }
      const uint64_t blo = __ballot(has_lo), bhi = __ballot(has_hi);
      if (blo == 0 || bhi == 0) {  // a NaN among the values: no total order
        res = __int_as_float(0x7fc00000);
      } else {
        const float x = __shfl(vlo, __ffsll((unsigned long long)blo) - 1, 64);
        const float y = __shfl(vhi, __ffsll((unsigned long long)bhi) - 1, 64);
        res = lo == hi ? x : (x + y) * 0.5f;
      }
    }
    if (lane == 0) out[row0 + first + r] = res;
  }
}

// rows of one index slot for this (n, N), before the workspace's own limit
static int64_t choice_slot_rows(int64_t N, int n) {
  const int64_t full = (CH_VALUES / n) / CH_ROW_ALIGN * CH_ROW_ALIGN;  // n <= 1024: >= 1024 rows
  const int64_t all = (N + CH_ROW_ALIGN - 1) / CH_ROW_ALIGN * CH_ROW_ALIGN;
  return full < all ? full : all;
}

static size_t choice_workspace_bytes(int64_t N, int n) {
  return (size_t)CH_RING * (size_t)choice_slot_rows(N, n) * (size_t)n * sizeof(uint16_t);
}

// rows per slot that a workspace of `bytes` allows (0: it holds no tile)
static int64_t choice_fit_rows(int64_t N, int n, size_t bytes) {
  int64_t rows = (int64_t)(bytes / CH_RING / ((size_t)n * sizeof(uint16_t))) / CH_ROW_ALIGN * CH_ROW_ALIGN;
  const int64_t want = choice_slot_rows(N, n);
  return rows < want ? rows : want;
}

// One draw stream and its ring events per host thread and device, kept for the life of the process
// (as the capture stream of api.hip: creating and destroying streams churns the runtime's queues).
struct ChoiceLane {
  hipStream_t stream = nullptr;
  hipEvent_t ready[CH_RING] = {}, freed[CH_RING] = {}, edge = nullptr;
};

static hipError_t choice_lane(ChoiceLane **out) {
  static thread_local ChoiceLane pool[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  ChoiceLane &L = pool[dev];
  if (!L.stream) {
    hipStream_t s = nullptr;
    if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return e;
    if ((e = hipEventCreateWithFlags(&L.edge, hipEventDisableTiming)) != hipSuccess) return e;
    for (int i = 0; i < CH_RING; ++i) {
      if ((e = hipEventCreateWithFlags(&L.ready[i], hipEventDisableTiming)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&L.freed[i], hipEventDisableTiming)) != hipSuccess) return e;
    }
    L.stream = s;  // (set last: a lane whose creation failed half way is built again)
  }
  *out = &L;
  return hipSuccess;
}

template <int K>
static hipError_t launch_reduce(const float *preds, const uint16_t *idx, int S, int64_t N, int64_t row0, int rows,
                                int n, int mode, float *out, hipStream_t st) {
  const int SP = S | 1;
  int tr_log2 = 5;
  while (tr_log2 > 3 && ((size_t)SP << tr_log2) * sizeof(float) > CH_TILE_LDS) --tr_log2;  // S = 2400: 8 rows
  const size_t sm = ((size_t)SP << tr_log2) * sizeof(float);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_choice_reduce<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) return e;
  const int TR = 1 << tr_log2;
  hipLaunchKernelGGL((k_choice_reduce<K>), dim3((unsigned)((rows + TR - 1) / TR)), dim3(CH_THREADS), sm, st, preds,
                     idx, S, N, row0, rows, n, tr_log2, SP, mode, out);
  return hipGetLastError();
}

// slot_rows: rows per ring slot (a multiple of CH_ROW_ALIGN, >= CH_ROW_ALIGN), ws: CH_RING slots of
// slot_rows * n uint16.  `st` is the caller's stream: the reduces run on it, the draws on the draw
// stream between two events, and st waits for the last draw, so the state is final for st's later work.
static hipError_t launch_posterior_choice(uint32_t *state, const float *preds, int S, int64_t N, int n, int mode,
                                          float *out, uint16_t *idx_out, uint16_t *ws, int64_t slot_rows,
                                          hipStream_t st) {
  ChoiceLane *L;
  hipError_t e = choice_lane(&L);
  if (e != hipSuccess) return e;
  hipStream_t ds = L->stream;
  hipEvent_t *ready = L->ready, *freed = L->freed, edge = L->edge;
#define CH_TRY(expr)              \
  do {                            \
    e = (expr);                   \
    if (e != hipSuccess) return e; \
  } while (0)
  const uint32_t rng = (uint32_t)(S - 1), mask = np_mask_of(rng);
  CH_TRY(hipEventRecord(edge, st));  // the state (and whatever st did to out before) is ready
  CH_TRY(hipStreamWaitEvent(ds, edge, 0));
  int64_t c = 0;
  for (int64_t row0 = 0; row0 < N; row0 += slot_rows, ++c) {
    const int slot = (int)(c % CH_RING);
    const int rows = (int)(N - row0 < slot_rows ? N - row0 : slot_rows);
    uint16_t *idx = ws + (size_t)slot * (size_t)slot_rows * (size_t)n;
    if (c >= CH_RING) CH_TRY(hipStreamWaitEvent(ds, freed[slot], 0));
    hipLaunchKernelGGL(k_choice_draw, dim3(1), dim3(NP_THREADS), 0, ds, state, idx, rng, mask, (int64_t)rows * n);
    CH_TRY(hipGetLastError());
    CH_TRY(hipEventRecord(ready[slot], ds));
    CH_TRY(hipStreamWaitEvent(st, ready[slot], 0));
    if (idx_out)
      CH_TRY(hipMemcpyAsync(idx_out + (size_t)row0 * n, idx, (size_t)rows * n * sizeof(uint16_t),
                            hipMemcpyDeviceToDevice, st));
    if (n == 1) {
      hipLaunchKernelGGL(k_choice_first, dim3((unsigned)((rows + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0,
                         st, preds, idx, S, N, row0, rows, out);
      CH_TRY(hipGetLastError());
    } else if (n <= 64) {
      CH_TRY(launch_reduce<1>(preds, idx, S, N, row0, rows, n, mode, out, st));
    } else if (n <= 128) {
      CH_TRY(launch_reduce<2>(preds, idx, S, N, row0, rows, n, mode, out, st));
    } else if (n <= 256) {
      CH_TRY(launch_reduce<4>(preds, idx, S, N, row0, rows, n, mode, out, st));
    } else if (n <= 512) {
      CH_TRY(launch_reduce<8>(preds, idx, S, N, row0, rows, n, mode, out, st));
    } else {
      CH_TRY(launch_reduce<16>(preds, idx, S, N, row0, rows, n, mode, out, st));
    }
    CH_TRY(hipEventRecord(freed[slot], st));
  }
  // (st has waited for every draw through the ready events: the state is final for its later work)
#undef CH_TRY
  return hipSuccess;
}

}  // namespace iqlhip

using namespace iqlhip;

// ------------------------------------------------------------ entry points --
static int choice_check(int32_t S, int64_t N, int32_t n_samps) {
  if (S < 2 || S > 2400) return fail(IQLHIP_ERR_INVALID, "S = %d outside 2..2400", S);
  if (n_samps < 1 || n_samps > 1024) return fail(IQLHIP_ERR_INVALID, "n_samps = %d outside 1..1024", n_samps);
  if (N < 1) return fail(IQLHIP_ERR_INVALID, "N = %lld must be >= 1", (long long)N);
  return 0;
}

extern "C" int iqlhip_posterior_choice_workspace_bytes(int32_t S, int64_t N, int32_t n_samps, size_t *bytes) {
  if (!bytes) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = choice_check(S, N, n_samps)) return rc;
  *bytes = choice_workspace_bytes(N, n_samps);
  return 0;
}

extern "C" int iqlhip_posterior_choice(uint32_t *state, const float *preds, int32_t S, int64_t N, int32_t n_samps,
                                       int32_t mode, float *out, uint16_t *idx_out, void *workspace,
                                       size_t workspace_bytes, void *stream) {
  if (!state || !preds || !out || !workspace) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (int rc = choice_check(S, N, n_samps)) return rc;
  if (mode != IQLHIP_CHOICE_MEAN && mode != IQLHIP_CHOICE_MEDIAN)
    return fail(IQLHIP_ERR_INVALID, "mode %d: IQLHIP_CHOICE_MEAN or IQLHIP_CHOICE_MEDIAN", mode);
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(IQLHIP_ERR_INVALID, "workspace not 16-byte aligned");
  const int64_t slot_rows = choice_fit_rows(N, n_samps, workspace_bytes);
  if (slot_rows < 32)
    return fail(IQLHIP_ERR_INVALID, "workspace of %zu bytes holds no chunk (the full size is %zu)", workspace_bytes,
                choice_workspace_bytes(N, n_samps));
  hipStream_t st = (hipStream_t)stream;
  uint32_t pos = 0;
  HIP_TRY(hipMemcpyAsync(&pos, state + 624, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (pos > 624) return fail(IQLHIP_ERR_INVALID, "pos = %u outside 0..624", pos);
  HIP_TRY(launch_posterior_choice(state, preds, S, N, n_samps, mode, out, idx_out, (uint16_t *)workspace, slot_rows,
                                  st));
  return 0;
}
