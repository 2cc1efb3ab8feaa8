// The training-step driver of libiqlhip.so: the lifecycle of trainers and seed groups, their workspaces, how
// steps reach a stream (StepQueue: pinned argument rings, hipGraph capture, padding, the throttle), the two
// step kinds (run_tuned, deep_run) -- and the entry points that read a trainer's config or arena layout
// (iqlhip_forward, iqlhip_explore_action*, iqlhip_arena_layout, iqlhip_step_cost), the CU-slice streams, the
// error text, ABI version and build tag.  Every other entry point of include/iqlhip.h sits in the .hip file
// of the kernels it launches; what one file calls in another is declared once, in iql_step.h, iql_deep.h or
// launchers.h, which both sides include.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/iqlhip.h"
#include "common.h"
#include "errors.h"
#include "host_plan.h"
#include "iql_deep.h"
#include "iql_step.h"
#include "launchers.h"
#include "step_math.h"

using namespace iqlhip;

// ------------------------------------------------------------------ errors --
static thread_local char g_err[512] = "";
int iqlhip::fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char *iqlhip_last_error(void) { return g_err; }
// One capture-only stream per host thread and device, kept for the life of the process (stream
// capture is thread-local, nothing ever executes on it).  A stream per trainer / group, created and
// destroyed with its owner, churned the runtime's hardware queues: CU-slice streams created after
// such a destroy no longer ran side by side (both halves of the chip serialised).
static hipError_t capture_stream(hipStream_t *out) {
  static thread_local hipStream_t pool[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!pool[dev]) {
    e = hipStreamCreateWithFlags(&pool[dev], hipStreamNonBlocking);
    if (e != hipSuccess) return e;
  }
  *out = pool[dev];
  return hipSuccess;
}

extern "C" int iqlhip_abi_version(void) { return 6; }
// sha256 prefix of csrc/* + include/iqlhip.h, stamped by iqlpref_amd/build.py: the Python side
// refuses a library whose tag does not match the sources it sits beside
#ifndef IQLHIP_BUILD_TAG
#define IQLHIP_BUILD_TAG "untagged"
#endif
static const char g_build_tag[] = "IQLHIP_BUILD_TAG=" IQLHIP_BUILD_TAG;  // marker: build.py reads it from the file
extern "C" const char *iqlhip_build_tag(void) { return g_build_tag + sizeof("IQLHIP_BUILD_TAG=") - 1; }

// ----------------------------------------------------------------- trainer --
static void group_invalidate(struct iqlhip_group *g);

// Bound on the work one caller can leave queued on a stream.  A train_steps call of n steps is
// 3n kernel dispatches (graph nodes or eager launches) and returns without a host wait; a caller
// that loops over such calls (bench.py's long regions, a seed-group sweep) used to be able to
// queue 60,000+ dispatches.  Every WINDOW dispatches the call records an event and, before it
// queues more, waits for the event of TWO windows ago: at most ~3 windows are ever outstanding,
// the device never runs dry (a window is >= 1.5 ms of work), and the host blocks only when it is
// that far ahead.  IQLHIP_MAX_INFLIGHT (dispatches) overrides the window total; 0 disables.
struct Throttle {
  static constexpr int NEV = 2;
  hipEvent_t ev[NEV] = {};
  bool used[NEV] = {};
  int head = 0;
  int64_t since = 0;  // dispatches queued since the last recorded event
  static int64_t window() {
    static const int64_t w = [] {
      const char *e = getenv("IQLHIP_MAX_INFLIGHT");
      const int64_t total = e ? atoll(e) : 6144;
      return total <= 0 ? (int64_t)0 : (total / 3 > 0 ? total / 3 : (int64_t)1);
    }();
    return w;
  }
  // call after `n` dispatches have been queued on `st`
  hipError_t queued(int64_t n, hipStream_t st) {
    const int64_t w = window();
    if (w == 0) return hipSuccess;
    since += n;
    if (since < w) return hipSuccess;
    since = 0;
    hipError_t e;
    if (!ev[head] && (e = hipEventCreateWithFlags(&ev[head], hipEventDisableTiming)) != hipSuccess) return e;
    if (used[head] && (e = hipEventSynchronize(ev[head])) != hipSuccess) return e;  // two windows ago
    if ((e = hipEventRecord(ev[head], st)) != hipSuccess) return e;
    used[head] = true;
    head = (head + 1) % NEV;
    return hipSuccess;
  }
  void destroy() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
  }
};

// Small uploads travel through a ring of N pinned host slots (a pageable source makes hipMemcpyAsync
// host-blocking, which serialised the streams of a SeedGroup); a slot is reused only after the copy that
// read it has completed (its event).
template <int N>
struct PinnedRing {
  char *host[N] = {};
  hipEvent_t ev[N] = {};
  bool used[N] = {};
  int head = 0;
  // the next slot, free to be written: `cap` bytes, allocated on first use
  int next(size_t cap, char **slot) {
    if (!host[head]) {
      HIP_TRY(hipHostMalloc((void **)&host[head], cap, hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&ev[head], hipEventDisableTiming));
    }
    if (used[head]) HIP_TRY(hipEventSynchronize(ev[head]));
    *slot = host[head];
    return 0;
  }
  // the first `bytes` of that slot to `dst`, in one copy
  int send(void *dst, size_t bytes, hipStream_t st) {
    const int slot = head;
    head = (slot + 1) % N;
    HIP_TRY(hipMemcpyAsync(dst, host[slot], bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ev[slot], st));
    used[slot] = true;
    return 0;
  }
  void destroy() {
    for (int k = 0; k < N; ++k) {
      if (ev[k]) (void)hipEventDestroy(ev[k]);
      if (host[k]) (void)hipHostFree(host[k]);
      ev[k] = nullptr, host[k] = nullptr, used[k] = false;
    }
  }
};

// How steps reach a stream, for one trainer (K = 1) or the K members of a group: what the device copies
// of the tuned step's arguments hold, the cached hipGraph of `graph_unroll` steps, the throttle, the
// per-kernel timing of the diagnostic mode and the launch counters.  Both step kinds issue through it.
struct StepQueue {
  PinnedRing<8> arg_ring;  // of [K] DevArgs
  DevArgs dev_args[IQLHIP_MAX_GROUP];  // what the device copies hold (see `continues`) ...
  bool dev_args_valid = false;  // ... and whether the batch of step total_it is already staged for them
  hipGraphExec_t gexec = nullptr;
  int graph_unroll = 0;
  bool graph_counts = false;  // `gexec` holds the counted k_backward (iqlhip_train_steps_valid)
  hipStream_t cap_stream = nullptr;  // capture only (the legacy default stream cannot capture); shared, see capture_stream
  Throttle throttle;
  // per-kernel HIP-event timing (diagnostic mode, eager launches whatever graph_unroll says)
  bool timing = false;
  hipEvent_t ev[5] = {};
  double t_acc[3] = {0, 0, 0};
  double t_empty = 0;  // interval of two back-to-back event records (event overhead)
  int64_t t_n = 0;
  int64_t n_eager = 0, n_graph = 0;  // steps issued as plain launches / graph replays issued (iqlhip_*_launch_counts)

  // K DevArgs through one pinned slot, in one copy to `dst`
  int push(const DevArgs *want, int K, DevArgs *dst, hipStream_t st) {
    char *slot;
    if (int rc = arg_ring.next(sizeof(DevArgs) * K, &slot)) return rc;
    DevArgs *h = reinterpret_cast<DevArgs *>(slot);
    for (int k = 0; k < K; ++k) h[k] = dev_args[k] = want[k];
    return arg_ring.send(dst, sizeof(DevArgs) * K, st);
  }
  // the cached graph holds addresses (descriptors, arguments): whoever moves them drops it
  void drop_graph() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    gexec = nullptr;
  }
  // `gexec` = U x step(cap_stream), a linear chain of kernel nodes; kept until another U or `counts` is asked for
  template <typename Step>
  int ensure_graph(int U, bool counts, Step step) {
    if (gexec && graph_unroll == U && graph_counts == counts) return 0;
    drop_graph();
    hipGraph_t g = nullptr;
    if (!cap_stream) HIP_TRY(capture_stream(&cap_stream));
    HIP_TRY(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int u = 0; u < U && !rc; ++u) rc = step(cap_stream);
    const hipError_t ce = hipStreamEndCapture(cap_stream, &g);
    if ((rc || ce != hipSuccess) && g) (void)hipGraphDestroy(g);
    if (rc) return rc;
    HIP_TRY(ce);
    const hipError_t ie = hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIP_TRY(ie);
    graph_unroll = U, graph_counts = counts;
    return 0;
  }
  // as many replays of the cached graph as fit into steps done .. n
  int replay(int64_t &done, int64_t n, hipStream_t st) {
    for (; done + graph_unroll <= n; done += graph_unroll) {
      HIP_TRY(hipGraphLaunch(gexec, st));
      ++n_graph;
      HIP_TRY(throttle.queued(3 * (int64_t)graph_unroll, st));
    }
    return 0;
  }
  // one step has been issued as plain launches; under timing with ev[0..3] around its three kernels
  // (one event pair per kernel: serialises the stream a little; diagnostic mode only)
  int eager_issued(hipStream_t st) {
    ++n_eager;
    if (!timing) {
      HIP_TRY(throttle.queued(3, st));
      return 0;
    }
    HIP_TRY(hipEventRecord(ev[4], st));  // empty interval: what a record pair costs by itself
    HIP_TRY(hipEventSynchronize(ev[4]));
    for (int k = 0; k < 3; ++k) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      t_acc[k] += ms;
    }
    float ems = 0.f;
    HIP_TRY(hipEventElapsedTime(&ems, ev[3], ev[4]));
    t_empty += ems;
    ++t_n;
    return 0;
  }
  int set_timing(bool enable) {
    timing = enable;
    t_acc[0] = t_acc[1] = t_acc[2] = 0, t_empty = 0, t_n = 0;
    if (timing)
      for (auto &e : ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    return 0;
  }
  void get_timing(double avg_ms[3], int64_t *n) const {
    // event-pair overhead (measured on an empty interval in the same pass) is subtracted
    for (int k = 0; k < 3; ++k) {
      const double v = t_n ? (t_acc[k] - t_empty) / (double)t_n : 0.0;
      avg_ms[k] = v > 0 ? v : 0.0;
    }
    if (n) *n = t_n;
  }
  void launch_counts(int64_t *eager_steps, int64_t *graph_launches) const {
    if (eager_steps) *eager_steps = n_eager;
    if (graph_launches) *graph_launches = n_graph;
  }
  void destroy() {
    drop_graph();
    arg_ring.destroy();
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
    throttle.destroy();
  }
};

// The general step's arguments in device memory, for one trainer (K = 1) or the K members of a group:
//   [K] DeepArgs | [K] DeepCtr | [CAP][K] AdamCoef
// A call is cut into chunks of at most CAP steps; ahead of each, the block, the counters (= the chunk's
// first step) and the Adam coefficients of its steps -- computed HERE in double, as the plain launches
// always had them -- go up in ONE copy from a ring of pinned slots.
struct DeepRing {
  static constexpr int64_t CAP = 1024;
  int K = 0;
  char *dev = nullptr;
  PinnedRing<4> ring;
  size_t head_bytes() const { return (size_t)K * (sizeof(DeepArgs) + sizeof(DeepCtr)); }
  size_t bytes(int64_t n) const { return head_bytes() + (size_t)n * K * sizeof(AdamCoef); }
  DeepArgs *dargs() const { return reinterpret_cast<DeepArgs *>(dev); }
  DeepCtr *dctr() const { return reinterpret_cast<DeepCtr *>(dev + (size_t)K * sizeof(DeepArgs)); }
  AdamCoef *dcoef() const { return reinterpret_cast<AdamCoef *>(dev + head_bytes()); }
  hipError_t init(int k) {
    K = k;
    hipError_t e = hipMalloc((void **)&dev, bytes(CAP));
    return e != hipSuccess ? e : hipMemset(dev, 0, bytes(CAP));
  }
  void destroy() {
    ring.destroy();
    if (dev) (void)hipFree(dev);
    dev = nullptr;
  }
};

// Where a launch of the tuned step finds one trainer's descriptor, arguments, counters and update items
struct Slots {
  TrainerDesc *desc = nullptr;  // device copy of D (kernels read it through L2, not the kernarg segment)
  DevArgs *args = nullptr;
  DevCtr *ctr = nullptr;
  UpdItem *items = nullptr;
  int n_items = 0;
};

// What the tuned three-kernel step of one trainer works on (shapes it is built for: is_deep)
struct TunedTrainer {
  TrainerDesc D;
  bool bf16 = false;
  void *ws = nullptr;
  // `own`: the slots of the trainer's workspace; `cur`: the ones in use -- its row of a group's contiguous
  // arrays while the trainer is a member of one (attach / detach), else `own`
  Slots own, cur;
  // host copy of the update kernel's work items, per trained net: first the items of the lower half of
  // every layer, then the upper half (n_half0 of them in the first part) -- tables are dealt from these
  std::vector<UpdItem> net_items[MAX_TRAIN];
  int n_half0[MAX_TRAIN] = {};
  // a batch_size that is no multiple of 16: the kernels index idx[] and drop_keep[] with their
  // padded row count D.B, the caller's arrays have batch_size rows a step -- copies with D.B rows a step, for
  // one chunk of a call's steps at a time (pad_inputs); grown on demand
  void *pad_idx = nullptr, *pad_keep = nullptr;
  size_t pad_idx_bytes = 0, pad_keep_bytes = 0;
};

struct iqlhip_trainer {
  iqlhip_trainer_config cfg;
  iqlhip_arenas arenas;
  int device = -1;  // where the parameter arena lives
  // one of the two step kinds: the tuned one, or (n_hidden != 2 or another width) the general layer-wise
  // one of iql_deep.hip with the ring its arguments travel through
  TunedTrainer *tuned = nullptr;
  DeepTrainer *deep = nullptr;
  DeepRing deep_ring;
  struct iqlhip_group *group = nullptr;
  float *batch_rows = nullptr;  // [B][stride] staging for iqlhip_train_batch (tuned: a block of the workspace)
  int64_t total_it = 0;
  double lr_q, lr_v, lr_a_base;
  StepQueue queue;  // of the trainer's own calls (K = 1)
};

static_assert(MAX_CRITICS == IQLHIP_MAX_CRITICS, "iql_step.h and iqlhip.h disagree");
static_assert(IQLHIP_N_TENSORS == 2 * DEEP_MAX_LIN * MAX_TRAIN + 1, "offset table size");
static_assert(IQLHIP_MAX_HIDDEN + 1 == DEEP_MAX_LIN, "iql_deep.h and iqlhip.h disagree");
// what both step kinds derive from a config: defaults resolved, net dimensions, dropout constants (host_plan.h)
static StepShape step_shape(const iqlhip_trainer_config &c) {
  return make_step_shape(c.state_dim, c.action_dim, c.n_critics, c.n_hidden, c.dropout_p,
                         c.precision == IQLHIP_PREC_BF16);
}
static int n_critics(const iqlhip_trainer_config &c) { return step_shape(c).E; }
static int n_hidden(const iqlhip_trainer_config &c) { return step_shape(c).NH; }
// which step runs this shape: the tuned three-kernel one or the general layer-wise one
static bool is_deep(const iqlhip_trainer_config &c) {
  // (tests: the general step on a shape the tuned one takes)
  static const bool force_general = getenv("IQLHIP_FORCE_GENERAL") != nullptr;
  return n_hidden(c) != 2 || (c.hidden_dim != 64 && c.hidden_dim != 128 && c.hidden_dim != 256) || force_general;
}

static int check_cfg(const iqlhip_trainer_config *c) {
  if (!c) return fail(IQLHIP_ERR_INVALID, "null config");
  if (c->n_critics < 0 || c->n_critics == 1 || c->n_critics > MAX_CRITICS)
    return fail(IQLHIP_ERR_UNSUPPORTED, "n_critics %d: 0 (= 2) or 2..%d", c->n_critics, MAX_CRITICS);
  if (c->state_dim <= 0 || c->action_dim <= 0) return fail(IQLHIP_ERR_INVALID, "bad dims");
  if (c->n_hidden < 0) return fail(IQLHIP_ERR_INVALID, "n_hidden must be >= 0");
  if (const char *why = nullptr; !deep_shape_ok(*c, n_hidden(*c), &why))
    return fail(IQLHIP_ERR_UNSUPPORTED, "n_hidden %d, hidden_dim %d: %s", n_hidden(*c), c->hidden_dim, why);
  if (c->batch_size < 1) return fail(IQLHIP_ERR_INVALID, "batch_size %d: must be >= 1", c->batch_size);
  if (c->batch_size > (1 << 24)) return fail(IQLHIP_ERR_UNSUPPORTED, "batch_size %d: at most 2^24", c->batch_size);
  if (c->action_dim > 32) return fail(IQLHIP_ERR_UNSUPPORTED, "action_dim %d > 32", c->action_dim);
  if (c->state_dim + c->action_dim > 128) return fail(IQLHIP_ERR_UNSUPPORTED, "state_dim+action_dim > 128");
  // the misc block of k_update sums the per-slab loss partials in its LDS
  if (!is_deep(*c) && (round_up(c->batch_size, 16) / 16) * (n_critics(*c) + 2 + (c->deterministic ? 0 : c->action_dim)) + n_critics(*c) + 2 >
      update_lds_floats())
    return fail(IQLHIP_ERR_UNSUPPORTED, "batch_size %d too large for action_dim %d", c->batch_size,
                c->action_dim);
  if (c->precision != IQLHIP_PREC_FP32 && c->precision != IQLHIP_PREC_BF16)
    return fail(IQLHIP_ERR_INVALID, "precision must be IQLHIP_PREC_FP32 or IQLHIP_PREC_BF16");
  if (c->dropout_p >= 1.0f) return fail(IQLHIP_ERR_INVALID, "dropout_p must be < 1");
  if (c->cosine_t_max <= 0) return fail(IQLHIP_ERR_INVALID, "cosine_t_max must be positive");
  if (c->polyak_form != 0 && c->polyak_form != 1) return fail(IQLHIP_ERR_INVALID, "polyak_form must be 0 or 1");
  return 0;
}

struct Layout {
  int64_t off[IQLHIP_N_TENSORS];
  int64_t n_params, n_target;      // arena elements (with alignment padding)
  int64_t true_params, true_target;  // trained scalars (SURVEY 8d byte model)
};
static Layout make_layout(const iqlhip_trainer_config &c) {
  // every tensor starts on a 128-byte line: rows of the H-wide matrices and the flat layer-1
  // strips are then streamed in whole, aligned lines
  constexpr int64_t ALIGN = 32;
  Layout L;
  int64_t o = 0, cnt = 0;
  const StepShape sh = step_shape(c);
  const int H = c.hidden_dim, NL = sh.NH + 1;
  const int E = sh.E, ntrain = sh.ntrain();
  for (int k = 0; k < IQLHIP_N_TENSORS; ++k) L.off[k] = -1;
  for (int n = 0; n < ntrain; ++n) {
    const int in = sh.in_dim(n), out = sh.out_dim(n);
    for (int l = 0; l < NL; ++l) {
      const int64_t rows = l == NL - 1 ? out : H, cols = l == 0 ? in : H;
      const int64_t sz[2] = {rows * cols, rows};  // W_l [rows][cols], b_l [rows]
      for (int k = 0; k < 2; ++k) {
        o = (o + ALIGN - 1) / ALIGN * ALIGN;
        L.off[(n * NL + l) * 2 + k] = o;
        o += sz[k];
        cnt += sz[k];
      }
    }
    if (n == E - 1) L.n_target = o, L.true_target = cnt;
  }
  if (c.deterministic) {
    L.off[ntrain * NL * 2] = -1;
  } else {
    o = (o + ALIGN - 1) / ALIGN * ALIGN;
    L.off[ntrain * NL * 2] = o;
    o += c.action_dim;
    cnt += c.action_dim;
  }
  L.n_params = o;
  L.true_params = cnt;
  return L;
}

extern "C" int iqlhip_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[IQLHIP_N_TENSORS],
                                   int64_t *n_params, int64_t *n_target) {
  if (int e = check_cfg(cfg)) return e;
  const Layout L = make_layout(*cfg);
  if (offsets) memcpy(offsets, L.off, sizeof(L.off));
  if (n_params) *n_params = L.n_params;
  if (n_target) *n_target = L.n_target;
  return 0;
}

extern "C" int iqlhip_step_cost(const iqlhip_trainer_config *cfg, double *bytes, double *flops) {
  if (int e = check_cfg(cfg)) return e;
  const Layout L = make_layout(*cfg);
  const double B = cfg->batch_size, S = cfg->state_dim, A = cfg->action_dim, H = cfg->hidden_dim;
  // gather + (read p,g,m,v; write g,p,m,v) per trained parameter + target r/w
  if (bytes) *bytes = 4.0 * B * (2 * S + A + 2) + 32.0 * (double)L.true_params + 8.0 * (double)L.true_target;
  if (flops) {
    const double E = n_critics(*cfg), HH = (n_hidden(*cfg) - 1) * H * H;  // hidden-to-hidden matrices
    const double wv = S * H + HH + H, wq = (S + A) * H + HH + H, wa = S * H + HH + H * A;
    const double fwd = 2 * wv + 2 * E * wq + wa;                 // V twice, target+online critics, actor
    const double dw = wv + E * wq + wa;                          // weight gradients
    const double dx = (HH + H) * (E + 1) + (HH + H * A);         // input gradients of every layer but the first
    *flops = 2.0 * B * (fwd + dw + dx);
  }
  return 0;
}

// The update kernel's item table is XCD-major: block b runs on XCD b & 7 (round-robin dispatch), so
// slot i of the table belongs to XCD i & 7, row i >> 3.  `per_xcd` lists what each XCD works on; rows
// are padded with idle slots (net = -1), which gather the next step's batch: they are numbered
// (o0 = index, i0 = count).  `min_depth`: tables of one group share their size.
static std::vector<UpdItem> flatten_table(const std::vector<UpdItem> (&per_xcd)[8], size_t min_depth, size_t *depth_out,
                                          size_t min_idle) {
  size_t depth = 0, n_real = 0;
  for (auto &v : per_xcd) depth = v.size() > depth ? v.size() : depth, n_real += v.size();
  // a table that happens to be (almost) full gets more rows of slots for the batch prefetch: one idle
  // slot per 16 batch rows (a 256-thread slot gathers 16 rows per pass; batch 1024 on 16 slots took four
  // passes of random rows out of a 288 MB buffer each -- the longest chain of the launch)
  while (8 * depth - n_real < min_idle) ++depth;
  if (depth < min_depth) depth = min_depth;
  std::vector<UpdItem> items;
  for (size_t d = 0; d < depth; ++d)
    for (int x = 0; x < 8; ++x) {
      UpdItem pad;
      memset(&pad, 0, sizeof(pad));
      pad.net = -1;
      items.push_back(d < per_xcd[x].size() ? per_xcd[x][d] : pad);
    }
  int n_pad = 0;
  for (auto &it : items)
    if (it.net < 0) it.o0 = n_pad++;
  for (auto &it : items)
    if (it.net < 0) it.i0 = n_pad;
  if (depth_out) *depth_out = depth;
  return items;
}

// Which XCD works on which items.
//   one seed per launch, TwinQ (4 trained nets): network n on XCDs 2n and 2n + 1, each taking half of
//     every layer (the panels a GEMM shares meet in two L2s, the bytes are spread over all eight);
//   one seed, more critics: the nets' items dealt out in order, an eighth of all items per XCD (6 nets
//     on pairs of XCDs left four XCDs with twice the work: E = 4 at batch 1024, round 4);
//   member k of a group launch: a WHOLE network per XCD -- (2n + k) & 7 for four nets: the eight
//     members of a group put one network of every kind on every XCD -- so that its activation / delta
//     panels are fetched from memory into ONE L2 (the balanced one-seed table fetches them into two:
//     2.9 MB of the 13.1 MB a seed's update moved in round 3).
// Measured (round 4, gpurun_out/e1, steps/s with the one-seed table / the whole-network table in every
// member): 8 seeds 219.7k / 223.6k (k_update 17.3 -> 16.7 us), 4 seeds 167.7k / 160.0k, 2 seeds 111.4k /
// 107.7k -- the rotation gives every XCD one network of every kind only for multiples of eight members;
// smaller groups keep the one-seed table.  Dealt in order (E > 2, one seed): E = 4 at batch 1024 35.9k ->
// 37.5k steps/s, E = 8 at batch 256 41.0k -> 42.4k.
static void deal_items(const TunedTrainer *t, int member, int group_size, std::vector<UpdItem> (&per_xcd)[8]) {
  const int NT = t->D.ntrain;
  const bool group = group_size > 1;
  const bool whole = group && group_size % 8 == 0;
  if (whole && NT == 4) {
    for (int n = 0; n < NT; ++n)
      for (auto &it : t->net_items[n]) per_xcd[(2 * n + member) & 7].push_back(it);
    return;
  }
  if (NT == 4) {
    for (int n = 0; n < NT; ++n)
      for (size_t i = 0; i < t->net_items[n].size(); ++i)
        per_xcd[(2 * n + ((int)i < t->n_half0[n] ? 0 : 1)) & 7].push_back(t->net_items[n][i]);
    return;
  }
  size_t total = 0, g = 0;
  for (int n = 0; n < NT; ++n) total += t->net_items[n].size();
  for (int n = 0; n < NT; ++n)
    for (auto &it : t->net_items[n]) {
      const int x = (int)(g * 8 / total);
      per_xcd[(x + (group ? member : 0)) & 7].push_back(it);
      ++g;
    }
  // One seed, more items per XCD than it has CUs (E = 4: 42 on 32): the launch is resident at once and the
  // dispatcher deals an XCD's work-groups over its CUs in order, so rows 32.. of a column land on the CUs of
  // rows 0..: those d CUs carry two work-groups, and what a CU takes in per microsecond bounds a work-group
  // (DESIGN.md section 4).  Put the d lightest items first and the next d lightest last, the heavy layer-2
  // tiles in between: no CU gets two heavy ones.
  if (!group) {
    constexpr size_t CUS_PER_XCD = 32;
    auto weight = [](const UpdItem &it) { return it.layer == 1 ? 3 : (it.layer == 0 ? 2 : 1); };  // layer-2 tile / strip / layer-3 tile
    for (auto &col : per_xcd) {
      if (col.size() <= CUS_PER_XCD || col.size() >= 2 * CUS_PER_XCD) continue;
      const size_t d = col.size() - CUS_PER_XCD;
      std::vector<UpdItem> sorted(col);
      std::stable_sort(sorted.begin(), sorted.end(), [&](const UpdItem &a, const UpdItem &b) { return weight(a) < weight(b); });
      std::vector<UpdItem> out(sorted.begin(), sorted.begin() + d);                 // rows 0 .. d-1: the lightest
      out.insert(out.end(), sorted.begin() + 2 * d, sorted.end());                  // the rest (heaviest) in the middle
      out.insert(out.end(), sorted.begin() + d, sorted.begin() + 2 * d);            // rows 32 ..: the next lightest
      col.swap(out);
    }
  }
}

// The pointer fields of a work item: a function of (net, layer) and the placed descriptor.
static void item_pointers(UpdItem &it, const TrainerDesc &D, int es) {
  if (it.net < 0) return;  // (an idle slot)
  const TrainNet &N = D.net[it.net];
  const int L = it.layer;
  it.wc = N.wc[L], it.tc = N.has_target ? N.tc[L] : nullptr, it.w2ct = (L == 1) ? N.w2ct : nullptr;
  it.w3t = (L == 2) ? N.w3t : nullptr;
  const size_t plane = (size_t)D.H * D.BP * es;
  it.Xsrc = (L == 0) ? D.xT : reinterpret_cast<char *>(D.hT) + (size_t)(it.net * 2 + (L - 1)) * plane;
  it.Zsrc = (L == 0)   ? reinterpret_cast<char *>(D.dz1T) + (size_t)it.net * plane
            : (L == 1) ? reinterpret_cast<char *>(D.dz2T) + (size_t)it.net * plane
                       : reinterpret_cast<char *>(D.dz3T) + (size_t)it.net * D.opmax * D.BP * es;
}

static void tuned_destroy(TunedTrainer *u) {
  if (!u) return;
  (void)hipFree(u->ws);
  (void)hipFree(u->pad_idx);
  (void)hipFree(u->pad_keep);
  delete u;
}

// The tuned step of trainer t (released with it: trainer_release).
static int tuned_create(iqlhip_trainer *t, const StepShape &sh, const Layout &L) {
  const iqlhip_trainer_config *cfg = &t->cfg;
  const iqlhip_arenas *ar = &t->arenas;
  TunedTrainer *u = t->tuned = new (std::nothrow) TunedTrainer();
  if (!u) return fail(IQLHIP_ERR_NOMEM, "host allocation failed");
  u->bf16 = cfg->precision == IQLHIP_PREC_BF16;
  // B: the rows every kernel works on, batch_size rounded up to whole 16-row slabs; rows [batch_size, B) are
  // padding, gathered like the others and kept out of the losses by the counted kernels (D.NB)
  const int S = cfg->state_dim, A = cfg->action_dim, H = cfg->hidden_dim, B = round_up(cfg->batch_size, 16);
  const int es = u->bf16 ? 2 : 4, KM = u->bf16 ? 32 : 16;
  TrainerDesc &D = u->D;
  memset(&D, 0, sizeof(D));
  D.S = S, D.A = A, D.H = H, D.B = B, D.BP = round_up(B, 32), D.NB = cfg->batch_size;
  const int E = sh.E, NT = sh.ntrain();
  D.E = E, D.ntrain = NT, D.nfwd = sh.nfwd(), D.net_v = sh.net_v(), D.net_a = sh.net_a();
  D.out_v = sh.out_v(), D.out_qt = sh.out_qt(), D.out_nv = sh.out_nv(), D.out_mean = sh.out_mean();
  D.two_over_B = 2.0f / (float)B, D.inv_E = 1.0f / (float)E;
  D.OUTW = round_up(D.out_mean + A, 4);
  D.deterministic = cfg->deterministic;
  D.has_dropout = sh.has_dropout;
  D.discount = cfg->discount, D.tau = cfg->tau, D.beta = cfg->beta, D.iql_tau = cfg->iql_tau;
  D.one_m_tau = (float)(1.0 - (double)cfg->tau);
  D.polyak_convex = cfg->polyak_form == 1;
  D.drop_scale = sh.drop.scale, D.drop_thr = sh.drop.thr;
  D.beta1 = cfg->adam_beta1, D.beta2 = cfg->adam_beta2, D.eps = cfg->adam_eps;
  D.t_max = cfg->cosine_t_max;
  D.seed = cfg->seed;
  D.params = ar->params, D.exp_avg = ar->exp_avg, D.exp_avg_sq = ar->exp_avg_sq;
  D.target = ar->target, D.grads = ar->grads;
  D.off_log_std = L.off[NT * 6];
  D.opmax = round_up(A, 16);
  D.xrows = round_up(S + A, 64);
  D.k1max = round_up(S + A, KM);
  const int stride = iqlhip_replay_row_stride(S, A);
  D.stage_stride = stride;
  D.next_off = iqlhip_replay_next_offset(S, A);
  // the idle slots of the update kernel gather the next step's batch; without them (or with
  // IQLHIP_NO_PREFETCH, the A/B of tests/test_gpu_step.py) k_stage runs before every step
  D.prefetch = !getenv("IQLHIP_NO_PREFETCH") ? 1 : 0;  // (every table has idle slots: flatten_table)
  for (int n = 0; n < NT; ++n) {
    TrainNet &N = D.net[n];
    N.in_dim = sh.in_dim(n), N.k1pad = round_up(N.in_dim, KM);
    N.out_dim = sh.out_dim(n), N.out_pad = round_up(N.out_dim, 16);
    N.has_target = n < E;
    for (int k = 0; k < 3; ++k) {
      N.off_w[k] = L.off[n * 6 + 2 * k];
      N.off_b[k] = L.off[n * 6 + 2 * k + 1];
      N.toff_w[k] = N.has_target ? N.off_w[k] : -1;  // target arena = q1,q2 prefix of the layout
      N.toff_b[k] = N.has_target ? N.off_b[k] : -1;
    }
  }
  // update work items (see deal_items / flatten_table): per net, the lower half of every layer first; their
  // pointer fields wait for the workspace (item_pointers)
  for (int n = 0; n < NT; ++n) {
    const TrainNet &N = D.net[n];
    std::vector<UpdItem> half[2];
    auto put = [&](int layer, int o0, int i0) {
      UpdItem it;
      memset(&it, 0, sizeof(it));
      it.net = n, it.layer = layer, it.o0 = o0, it.i0 = i0;
      it.Odim = (layer == 2) ? N.out_dim : H;
      it.Idim = (layer == 0) ? N.in_dim : H;
      it.Opad = (layer == 2) ? N.out_pad : H;
      it.Kw = (layer == 0) ? N.k1pad : H;
      it.has_target = N.has_target;
      it.group = n == D.net_v ? 1 : (n == D.net_a ? 2 : 0);
      it.off_w = N.off_w[layer], it.off_b = N.off_b[layer], it.toff_w = N.toff_w[layer], it.toff_b = N.toff_b[layer];
      half[(layer == 2 && it.Opad <= 64) ? ((i0 / 32) & 1) : (o0 >= it.Opad / 2 ? 1 : 0)].push_back(it);
    };
    for (int o0 = 0; o0 < H; o0 += 64)
      for (int i0 = 0; i0 < H; i0 += 32) put(1, o0, i0);
    for (int o0 = 0; o0 < H; o0 += strip_rows()) put(0, o0, 0);  // layer 1: strips over all in-features
    for (int o0 = 0; o0 < N.out_pad; o0 += 64)
      for (int i0 = 0; i0 < H; i0 += 32) put(2, o0, i0);
    u->n_half0[n] = (int)half[0].size();
    u->net_items[n] = half[0];
    u->net_items[n].insert(u->net_items[n].end(), half[1].begin(), half[1].end());
  }
  std::vector<UpdItem> items;  // the trainer's own table
  {
    std::vector<UpdItem> per_xcd[8];
    deal_items(u, 0, 1, per_xcd);
    // A lone trainer with dropout: its idle slots also draw the next step's masks (draw_keep_plane), B H / 2
    // Philox calls that are pure multiplier time -- on 16 slots at B = H = 256 they were the launch's longest
    // work-groups (k_update 5.6 -> 7.2 us traced).  32 slots keep a TwinQ table (224 tiles) on one work-group
    // per CU.  Group tables stay as they are: the chip is full there and the draws are throughput.
    const size_t rows16 = (size_t)(B + 15) / 16;
    items = flatten_table(per_xcd, 0, nullptr, D.has_dropout && rows16 < 32 ? 32 : rows16);
  }
  // ---- workspace: the one list of its blocks, run once to measure and once to place ----
  auto blocks = [&](WorkspacePlan p) {
    for (int n = 0; n < NT; ++n) {
      TrainNet &N = D.net[n];
      N.wc[0] = p.take<char>((size_t)H * N.k1pad * es);
      N.wc[1] = p.take<char>((size_t)H * H * es);
      N.wc[2] = p.take<char>((size_t)N.out_pad * H * es);
      if (N.has_target) {
        N.tc[0] = p.take<char>((size_t)H * N.k1pad * es);
        N.tc[1] = p.take<char>((size_t)H * H * es);
        N.tc[2] = p.take<char>((size_t)N.out_pad * H * es);
      }
      N.w2ct = p.take<char>((size_t)H * H * es);
      N.w3t = p.take<char>((size_t)H * N.out_pad * es);
    }
    D.xT = p.take<char>((size_t)2 * D.xrows * D.BP * es);
    D.rd = p.take<float>((size_t)B * 2);
    D.actf = p.take<float>((size_t)B * A);
    D.hT = p.take<char>((size_t)NT * 2 * H * D.BP * es);
    D.dz1T = p.take<char>((size_t)NT * H * D.BP * es);
    D.dz2T = p.take<char>((size_t)NT * H * D.BP * es);
    D.dz3T = p.take<char>((size_t)NT * D.opmax * D.BP * es);
    D.outs = p.take<float>((size_t)layer2_parts(H) * B * D.OUTW);
    D.lossp = p.take<float>((size_t)NT * (B / 16));
    D.lsp = p.take<float>((size_t)(B / 16) * A);
    D.ls_snap = p.take<float>((size_t)A);
    // one plane: its only reader is k_forward, its writers (k_stage, k_update's idle slots) run between two forwards
    D.keepb = D.has_dropout ? p.take<uint8_t>((size_t)2 * (B / 4) * H) : nullptr;
    t->batch_rows = p.take<float>((size_t)B * stride);
    D.stage_rows = p.take<float>((size_t)B * stride);
    u->own.args = p.take<DevArgs>(1);
    u->own.ctr = p.take<DevCtr>(1);
    u->own.desc = p.take<TrainerDesc>(1);
    u->own.items = p.take<UpdItem>(items.size());
    return p.end();
  };
  const size_t total = blocks(WorkspacePlan());
  if (hipMalloc(&u->ws, total) != hipSuccess)
    return fail(IQLHIP_ERR_NOMEM, "hipMalloc of %zu workspace bytes failed", total);
  if (hipMemset(u->ws, 0, total) != hipSuccess) return fail(IQLHIP_ERR_HIP, "hipMemset failed");
  blocks(WorkspacePlan(u->ws));
  u->own.n_items = (int)items.size();
  u->cur = u->own;

  for (int n = 0; n < NT; ++n)
    for (auto &it : u->net_items[n]) item_pointers(it, D, es);
  for (auto &it : items) item_pointers(it, D, es);
  if (hipMemcpy(u->own.items, items.data(), items.size() * sizeof(UpdItem), hipMemcpyHostToDevice) != hipSuccess)
    return fail(IQLHIP_ERR_HIP, "hipMemcpy of the work items failed");

  // ---- forward evaluations ----
  const std::vector<EvalSpec> order = eval_order(sh, D.next_off);
  for (int f = 0; f < (int)order.size(); ++f) {
    const auto [net, target, in_off, out_col, slot] = order[f];
    FwdNet &F = D.fwd[f];
    const TrainNet &N = D.net[net];
    F.w1c = target ? N.tc[0] : N.wc[0];
    F.w2c = target ? N.tc[1] : N.wc[1];
    F.w3c = target ? N.tc[2] : N.wc[2];
    const float *base = target ? ar->target : ar->params;
    F.b1 = base + N.off_b[0], F.b2 = base + N.off_b[1], F.b3 = base + N.off_b[2];
    F.in_off = in_off, F.in_dim = N.in_dim, F.k1pad = N.k1pad;
    F.out_dim = N.out_dim, F.out_pad = N.out_pad, F.out_col = out_col;
    F.train_slot = slot;
    F.tanh_out = net == D.net_a;
    F.dropout = (net == D.net_a) && D.has_dropout;
    F.stage = f == 0;
  }
  if (hipMemcpy(u->own.desc, &D, sizeof(TrainerDesc), hipMemcpyHostToDevice) != hipSuccess)
    return fail(IQLHIP_ERR_HIP, "hipMemcpy of the descriptor failed");
  return 0;
}

// Frees a trainer, finished or partly built (iqlhip_trainer_create's owner).
static void trainer_release(iqlhip_trainer *t) {
  t->queue.destroy();
  if (!t->tuned) (void)hipFree(t->batch_rows);  // (tuned: a block of the workspace)
  tuned_destroy(t->tuned);
  deep_destroy(t->deep);
  t->deep_ring.destroy();
  delete t;
}

extern "C" int iqlhip_trainer_create(iqlhip_trainer **out, const iqlhip_trainer_config *cfg,
                                     const iqlhip_arenas *ar) {
  if (!out) return fail(IQLHIP_ERR_INVALID, "null out");
  if (int e = check_cfg(cfg)) return e;
  if (!ar || !ar->params || !ar->exp_avg || !ar->exp_avg_sq || !ar->target)
    return fail(IQLHIP_ERR_INVALID, "null arena pointer");
  HIP_TRY(prepare_step_kernels());
  Owner<iqlhip_trainer, trainer_release> t(new (std::nothrow) iqlhip_trainer());
  if (!t) return fail(IQLHIP_ERR_NOMEM, "host allocation failed");
  t->cfg = *cfg;
  t->arenas = *ar;
  if (hipPointerAttribute_t at; hipPointerGetAttributes(&at, ar->params) == hipSuccess)
    t->device = at.device;
  else
    (void)hipGetLastError();
  t->lr_q = cfg->lr_q, t->lr_v = cfg->lr_v, t->lr_a_base = cfg->lr_actor;
  const StepShape sh = step_shape(*cfg);
  const Layout L = make_layout(*cfg);
  if (is_deep(*cfg)) {
    const size_t rows_bytes = (size_t)cfg->batch_size * iqlhip_replay_row_stride(cfg->state_dim, cfg->action_dim) * 4;
    hipError_t e = deep_create(&t->deep, *cfg, sh, *ar, L.off);
    if (e == hipSuccess) e = hipMalloc((void **)&t->batch_rows, rows_bytes);
    if (e == hipSuccess) e = t->deep_ring.init(1);
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? IQLHIP_ERR_NOMEM : IQLHIP_ERR_HIP, "general step: %s", hipGetErrorString(e));
  } else if (int rc = tuned_create(t.get(), sh, L)) {
    return rc;
  }
  *out = t.release();
  return 0;
}

extern "C" int iqlhip_trainer_destroy(iqlhip_trainer *t) {
  if (!t) return 0;
  if (t->group) return fail(IQLHIP_ERR_INVALID, "trainer is a member of a group: destroy the group first");
  trainer_release(t);
  return 0;
}

extern "C" int iqlhip_trainer_step_kind(iqlhip_trainer *t, int32_t *kind) {
  if (!t || !kind) return fail(IQLHIP_ERR_INVALID, "null argument");
  *kind = t->deep ? 1 : 0;
  return 0;
}

extern "C" int iqlhip_trainer_sync_weights(iqlhip_trainer *t, void *stream) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  if (t->deep) {
    HIP_TRY(deep_sync_weights(t->deep, (hipStream_t)stream));
    return 0;
  }
  HIP_TRY(launch_sync_weights(t->tuned->bf16, t->tuned->cur.desc, (hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_trainer_set_step(iqlhip_trainer *t, int64_t total_it) {
  if (!t || total_it < 0) return fail(IQLHIP_ERR_INVALID, "bad argument");
  // rare (init, load_state_dict): drain every stream first, so that no step in flight on a
  // non-blocking stream can race the counter write below
  HIP_TRY(hipDeviceSynchronize());
  t->total_it = total_it;
  if (t->deep) return 0;  // (the general step's device counter is set with the arguments of every call)
  DevCtr c;
  memset(&c, 0, sizeof(c));
  c.ctr[0] = total_it, c.ctr[1] = total_it;
  HIP_TRY(hipMemcpy(t->tuned->cur.ctr, &c, sizeof(c), hipMemcpyHostToDevice));
  t->queue.dev_args_valid = false;
  if (t->group) group_invalidate(t->group);
  return 0;
}

static double cosine_lr(double base, int64_t t, int64_t t_max) {
  return base * (1.0 + cos(M_PI * (double)t / (double)t_max)) * 0.5;
}

extern "C" int iqlhip_trainer_get_step(iqlhip_trainer *t, int64_t *total_it, double *actor_lr) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  if (total_it) *total_it = t->total_it;
  if (actor_lr) *actor_lr = cosine_lr(t->lr_a_base, t->total_it, t->cfg.cosine_t_max);
  return 0;
}

extern "C" int iqlhip_trainer_set_lr(iqlhip_trainer *t, double lr_q, double lr_v, double lr_a_base) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  t->lr_q = lr_q, t->lr_v = lr_v, t->lr_a_base = lr_a_base;
  return 0;
}

extern "C" int iqlhip_trainer_set_timing(iqlhip_trainer *t, int32_t enable) {
  return t ? t->queue.set_timing(enable != 0) : fail(IQLHIP_ERR_INVALID, "null trainer");
}

extern "C" int iqlhip_trainer_get_timing(iqlhip_trainer *t, double avg_ms[3], int64_t *n) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  t->queue.get_timing(avg_ms, n);
  return 0;
}

extern "C" int iqlhip_trainer_launch_counts(iqlhip_trainer *t, int64_t *eager_steps, int64_t *graph_launches) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  t->queue.launch_counts(eager_steps, graph_launches);
  return 0;
}

// A call continues the previous one when it reads the same replay contents (rows, size,
// generation) with on-device indices and dropout masks, produces no per-step outputs and has the
// same learning rates: nothing in DevArgs that the kernels read differs (base_step / n_steps only
// index idx[], drop_keep[] and losses_out[]), and the last update of the previous call has already
// staged this call's first batch.  Then nothing is sent and k_stage is not launched.
static bool continues(const DevArgs &a, const DevArgs &b) {
  return a.rows == b.rows && a.n_rows == b.n_rows && a.row_stride == b.row_stride &&
         a.generation == b.generation && a.idx_mode == 0 && b.idx_mode == 0 && !a.drop_keep && !b.drop_keep &&
         !a.losses_out && !b.losses_out && !a.n_valid && !b.n_valid && a.lr_q == b.lr_q && a.lr_v == b.lr_v && a.lr_a_base == b.lr_a_base;
}

// What a launch of the tuned step works on: the launch geometry of member 0 and the [K] device arrays of
// a group, or (K = 1) a trainer's own slots -- its slot k of the group's arrays while it is a member of one.
struct StepTarget {
  bool bf16;
  const TrainerDesc &D;
  const TrainerDesc *desc;
  DevArgs *args;
  DevCtr *ctr;
  const UpdItem *items;
  int n_items, K;
};

// one step; ev (optional, 4 events) brackets the three kernels for the per-kernel timing
static int enqueue_step(const StepTarget &x, bool counts, hipStream_t st, hipEvent_t *ev) {
  if (!x.D.prefetch) HIP_TRY(launch_stage(x.bf16, x.D, x.desc, x.args, x.ctr, x.K, st));
  if (ev) HIP_TRY(hipEventRecord(ev[0], st));
  HIP_TRY(launch_forward(x.bf16, x.D, x.desc, x.args, x.ctr, x.K, st));
  if (ev) HIP_TRY(hipEventRecord(ev[1], st));
  // (a padded batch -- the members of a group share the shape -- takes the counted kernels in every call)
  const bool padded = x.D.NB != x.D.B;
  HIP_TRY(launch_backward(x.bf16, x.D, x.desc, x.args, x.ctr, x.K, st, counts || padded));
  if (ev) HIP_TRY(hipEventRecord(ev[2], st));
  HIP_TRY(launch_update(x.bf16, x.desc, x.args, x.ctr, x.items, x.n_items, x.K, st, padded));
  if (ev) HIP_TRY(hipEventRecord(ev[3], st));
  return 0;
}

// The tuned step, for one trainer or the K members of a group: the K DevArgs go up through one pinned slot
// in one copy (skipped when the call continues the last), then the steps run as hipGraphs of `graph_unroll`
// steps and the remainder as plain launches.  `counts`: which k_backward the launches (and the graph) use.
static int run_tuned(StepQueue &q, const StepTarget &x, const DevArgs *want, int64_t n_steps, int graph_unroll,
                     bool counts, hipStream_t st) {
  bool same = x.D.prefetch && q.dev_args_valid && !q.timing, all_philox = true;
  for (int k = 0; k < x.K; ++k) {
    same = same && continues(q.dev_args[k], want[k]);
    all_philox = all_philox && want[k].idx_mode == 0;
  }
  if (!same) {
    if (int rc = q.push(want, x.K, x.args, st)) return rc;
    // the first step's batch (later steps are staged by the update kernel of the step before)
    if (x.D.prefetch) HIP_TRY(launch_stage(x.bf16, x.D, x.desc, x.args, x.ctr, x.K, st));
  }
  // after this call the device holds these arguments and (prefetch, on-device indices) the batch
  // of the step that follows it
  q.dev_args_valid = all_philox;
  int64_t done = 0;
  if (!q.timing && graph_unroll > 0 && n_steps >= graph_unroll) {
    if (int rc = q.ensure_graph(graph_unroll, counts, [&](hipStream_t cs) { return enqueue_step(x, counts, cs, nullptr); }))
      return rc;
    if (int rc = q.replay(done, n_steps, st)) return rc;
  }
  for (; done < n_steps; ++done) {
    if (int rc = enqueue_step(x, counts, st, q.timing ? q.ev : nullptr)) return rc;
    if (int rc = q.eager_issued(st)) return rc;
  }
  return 0;
}

// The general step, for one trainer or the K members of a group.  Per chunk of at most DeepRing::CAP steps:
// the arguments, the counters and the chunk's Adam coefficients go to the device (DeepRing), then the steps
// run as hipGraphs of `graph_unroll` steps (3 graph_unroll kernel nodes, a linear chain captured on one
// stream) and the remainder as plain launches.  Chunks are a multiple of graph_unroll steps long, so only the
// tail of a call runs eagerly.  Everything that differs between a trainer and a group is referenced here.
struct DeepRun {
  iqlhip_trainer *const *tr;
  int K;
  DeepRing *ring;
  const DeepDesc *ddesc;  // [K], device
  StepQueue &q;
};

static int deep_push(const DeepRun &r, const DevArgs *a, int64_t done, int64_t n, hipStream_t st) {
  DeepRing &R = *r.ring;
  const int K = r.K;
  char *slot;
  if (int rc = R.ring.next(R.bytes(DeepRing::CAP), &slot)) return rc;
  DeepArgs *ha = reinterpret_cast<DeepArgs *>(slot);
  DeepCtr *hc = reinterpret_cast<DeepCtr *>(slot + (size_t)K * sizeof(DeepArgs));
  AdamCoef *hk = reinterpret_cast<AdamCoef *>(slot + R.head_bytes());
  for (int k = 0; k < K; ++k) {
    const iqlhip_trainer_config &c = r.tr[k]->cfg;
    const int64_t B = c.batch_size, H = c.hidden_dim, NH = n_hidden(c);
    DeepArgs &x = ha[k];
    memset(&x, 0, sizeof(x));
    x.rows = a[k].rows, x.n_rows = a[k].n_rows, x.row_stride = a[k].row_stride, x.idx_mode = a[k].idx_mode;
    x.idx = a[k].idx ? a[k].idx + done * B : nullptr;
    x.drop_keep = a[k].drop_keep ? a[k].drop_keep + done * NH * B * H : nullptr;
    x.losses_out = a[k].losses_out ? a[k].losses_out + done * 3 : nullptr;
    x.base_step = a[k].base_step + done, x.n_steps = n;
    hc[k].ctr[0] = hc[k].ctr[1] = x.base_step;
    for (int64_t i = 0; i < n; ++i)
      hk[i * K + k] = make_adam_coef(c.adam_beta1, c.adam_beta2, c.adam_eps, a[k].lr_q, a[k].lr_v, a[k].lr_a_base,
                                     c.cosine_t_max, x.base_step + i + 1);
  }
  return R.ring.send(R.dev, R.bytes(n), st);
}

static int deep_run(const DeepRun &r, const DevArgs *a, int64_t n_steps, int graph_unroll, hipStream_t st) {
  StepQueue &q = r.q;
  auto step = [&](hipStream_t s, hipEvent_t *ev) {
    HIP_TRY(deep_step(r.tr[0]->deep, r.ddesc, r.ring->dargs(), r.ring->dctr(), r.ring->dcoef(), r.K, s, ev));
    return 0;
  };
  const int U = q.timing ? 0 : (int)std::min<int64_t>(std::max(graph_unroll, 0), DeepRing::CAP);
  const int64_t cap = U > 0 ? DeepRing::CAP / U * U : DeepRing::CAP;
  for (int64_t done = 0; done < n_steps;) {
    const int64_t n = std::min(cap, n_steps - done);
    if (int rc = deep_push(r, a, done, n, st)) return rc;
    int64_t i = 0;
    if (U > 0 && n >= U) {
      if (int rc = q.ensure_graph(U, false, [&](hipStream_t cs) { return step(cs, nullptr); })) return rc;
      if (int rc = q.replay(i, n, st)) return rc;
    }
    for (; i < n; ++i) {
      if (int rc = step(st, q.timing ? q.ev : nullptr)) return rc;
      if (int rc = q.eager_issued(st)) return rc;
    }
    done += n;
  }
  return 0;
}

// per-step valid-row counts: refused before any launch where the step is not built for them
static int check_counts(const iqlhip_trainer *t0, bool counts, const char *who) {
  // (the counts live on the device: the call cannot tell whether every one of them is the whole batch)
  if (counts && t0->deep)
    return fail(IQLHIP_ERR_UNSUPPORTED,
                "per-step valid-row counts (a short batch) run on the tuned step only (n_hidden 2, hidden_dim 64 / "
                "128 / 256); this %s (n_hidden %d, hidden_dim %d) runs the general layer-wise step",
                who, n_hidden(t0->cfg), t0->cfg.hidden_dim);
  if (counts && t0->tuned->bf16)
    return fail(IQLHIP_ERR_UNSUPPORTED, "per-step valid-row counts (a short batch) are built for precision fp32 only");
  return 0;
}

static int check_view(const iqlhip_replay_view &v, const iqlhip_trainer_config &c) {
  if (v.state_dim != c.state_dim || v.action_dim != c.action_dim)
    return fail(IQLHIP_ERR_INVALID, "replay dims (%d,%d) do not match the trainer (%d,%d)", v.state_dim,
                v.action_dim, c.state_dim, c.action_dim);
  if (v.n_rows <= 0) return fail(IQLHIP_ERR_INVALID, "cannot sample from an empty replay buffer");
  if (v.row_stride != iqlhip_replay_row_stride(v.state_dim, v.action_dim))
    return fail(IQLHIP_ERR_INVALID, "row_stride %d is not the packed layout's (%d)", v.row_stride,
                iqlhip_replay_row_stride(v.state_dim, v.action_dim));
  return 0;
}

// A padded batch on the tuned step (batch_size no multiple of 16: D.NB < D.B).  The caller's idx[] and
// drop_keep[] have batch_size rows a step and the kernels index D.B rows a step, so the steps of a call go
// through copies with D.B rows a step, a chunk of at most pad_chunk() steps at a time: row r < batch_size of a
// step is the caller's, every padding row repeats row 0 of its step (an index the caller gave: in range; a
// mask row: never counted).  Nothing is read beyond the caller's arrays.  On-device indices and masks need
// no copy: a padding row draws the Philox index / mask words of its own row number.
static bool is_padded(const iqlhip_trainer *t) { return t->tuned && t->tuned->D.NB != t->tuned->D.B; }
static int64_t pad_chunk(const iqlhip_trainer *t, bool idx, bool keep) {
  if (!is_padded(t) || (!idx && !keep)) return INT64_MAX;
  const TrainerDesc &D = t->tuned->D;
  const size_t per_step = (idx ? (size_t)D.B * 8 : 0) + (keep ? (size_t)2 * D.B * D.H : 0);
  const size_t budget = (size_t)32 << 20;
  return budget / per_step > 0 ? (int64_t)(budget / per_step) : 1;
}
static int pad_grow(void **buf, size_t *have, size_t want) {
  if (*have >= want) return 0;
  if (*buf) HIP_TRY(hipFree(*buf));  // (waits for the device: nothing in flight reads the old copy)
  *buf = nullptr, *have = 0;
  if (hipMalloc(buf, want) != hipSuccess) return fail(IQLHIP_ERR_NOMEM, "hipMalloc of %zu bytes (padded batch) failed", want);
  *have = want;
  return 0;
}
static int pad_inputs(iqlhip_trainer *t, DevArgs &a, hipStream_t st) {
  if (!is_padded(t)) return 0;
  TunedTrainer *u = t->tuned;
  const int NB = u->D.NB, B = u->D.B, H = u->D.H;
  if (a.idx_mode == 1) {
    if (int rc = pad_grow(&u->pad_idx, &u->pad_idx_bytes, (size_t)a.n_steps * B * 8)) return rc;
    HIP_TRY(launch_pad_rows(a.idx, u->pad_idx, a.n_steps, NB, B, 8, st));
    a.idx = reinterpret_cast<const int64_t *>(u->pad_idx);
  }
  if (a.drop_keep) {
    if (int rc = pad_grow(&u->pad_keep, &u->pad_keep_bytes, (size_t)a.n_steps * 2 * B * H)) return rc;
    HIP_TRY(launch_pad_rows(a.drop_keep, u->pad_keep, a.n_steps * 2, NB, B, H, st));
    a.drop_keep = reinterpret_cast<const uint8_t *>(u->pad_keep);
  }
  return 0;
}

// the arguments of n_steps steps of trainer t from where it stands
static DevArgs make_args(const iqlhip_trainer *t, const iqlhip_replay_view &v, int64_t n_steps, const int64_t *idx,
                         const int32_t *n_valid, const uint8_t *dropout_keep, float *losses_out) {
  DevArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = v.rows, a.n_rows = v.n_rows, a.row_stride = v.row_stride;
  a.generation = v.generation;
  a.idx_mode = idx ? 1 : 0, a.idx = idx;
  a.drop_keep = dropout_keep, a.losses_out = losses_out;
  a.n_valid = n_valid;  // (`continues` is false with counts on either side)
  a.base_step = t->total_it, a.n_steps = n_steps;
  a.lr_q = t->lr_q, a.lr_v = t->lr_v, a.lr_a_base = t->lr_a_base;
  return a;
}

// a trainer's own call (also while it is a member of a group)
static int run_solo(iqlhip_trainer *t, const DevArgs &a, int graph_unroll, hipStream_t st) {
  const bool counts = a.n_valid != nullptr;
  if (int rc = check_counts(t, counts, "trainer")) return rc;
  if (t->deep) {
    iqlhip_trainer *tr[1] = {t};
    return deep_run({tr, 1, &t->deep_ring, deep_desc_dev(t->deep), t->queue}, &a, a.n_steps, graph_unroll, st);
  }
  if (t->group) group_invalidate(t->group);  // this call rewrites the member's slot of the group's arguments
  const TunedTrainer *u = t->tuned;
  const StepTarget x = {u->bf16, u->D, u->cur.desc, u->cur.args, u->cur.ctr, u->cur.items, u->cur.n_items, 1};
  return run_tuned(t->queue, x, &a, a.n_steps, graph_unroll, counts, st);
}

extern "C" int iqlhip_train_steps(iqlhip_trainer *t, const iqlhip_replay_view *view, int64_t n_steps,
                                  const int64_t *idx, const uint8_t *dropout_keep, float *losses_out,
                                  int32_t graph_unroll, void *stream) {
  return iqlhip_train_steps_valid(t, view, n_steps, idx, nullptr, dropout_keep, losses_out, graph_unroll, stream);
}

extern "C" int iqlhip_train_steps_valid(iqlhip_trainer *t, const iqlhip_replay_view *view, int64_t n_steps,
                                        const int64_t *idx, const int32_t *n_valid, const uint8_t *dropout_keep,
                                        float *losses_out, int32_t graph_unroll, void *stream) {
  if (!t || !view || !view->rows) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n_steps < 0) return fail(IQLHIP_ERR_INVALID, "n_steps must be >= 0");
  if (int rc = check_view(*view, t->cfg)) return rc;
  // (one pass, but for a padded batch with injected indices or masks: pad_inputs)
  const int64_t chunk = pad_chunk(t, idx != nullptr, dropout_keep != nullptr);
  const int64_t NB = t->cfg.batch_size, keep_step = (int64_t)n_hidden(t->cfg) * NB * t->cfg.hidden_dim;
  for (int64_t done = 0; done < n_steps;) {
    const int64_t n = std::min(chunk, n_steps - done);
    DevArgs a = make_args(t, *view, n, idx ? idx + done * NB : nullptr, n_valid ? n_valid + done : nullptr,
                          dropout_keep ? dropout_keep + done * keep_step : nullptr,
                          losses_out ? losses_out + done * 3 : nullptr);
    if (int rc = pad_inputs(t, a, (hipStream_t)stream)) return rc;
    if (int rc = run_solo(t, a, graph_unroll, (hipStream_t)stream)) return rc;
    t->total_it += n;
    done += n;
  }
  return 0;
}

extern "C" int iqlhip_train_batch(iqlhip_trainer *t, const float *s, const float *a, const float *r,
                                  const float *s2, const float *d, const uint8_t *dropout_keep,
                                  float *losses_out, void *stream) {
  if (!t || !s || !a || !r || !s2 || !d) return fail(IQLHIP_ERR_INVALID, "null argument");
  const int S = t->cfg.state_dim, A = t->cfg.action_dim, B = t->cfg.batch_size;
  const int stride = iqlhip_replay_row_stride(S, A);
  if (int rc = iqlhip_replay_pack(t->batch_rows, stride, S, A, 0, B, s, a, r, s2, d, stream)) return rc;
  const iqlhip_replay_view rows = {t->batch_rows, B, stride, S, A, 0};
  DevArgs args = make_args(t, rows, 1, nullptr, nullptr, dropout_keep, losses_out);
  args.idx_mode = 2;  // the rows as they lie (a padding row: clamped to the last one)
  if (int rc = pad_inputs(t, args, (hipStream_t)stream)) return rc;
  if (int rc = run_solo(t, args, 0, (hipStream_t)stream)) return rc;
  t->total_it += 1;
  return 0;
}

// ------------------------------------------------------------------ groups --
// K independent trainers (seeds) of one shape stepped by ONE launch sequence: every kernel
// runs with gridDim.y = K and work-group (x, k) does for seed k exactly what work-group x of
// a solo launch does -- the arithmetic of every seed is bit-identical to running it alone.
// One seed at batch 256 is a latency chain on a fraction of the chip; K seeds per launch
// fill it and pay the kernel boundaries once per K seed-steps (the reference runs several
// agents per GPU for the same reason, ensemble_sweeps/launch.sh:12 AGENTS_PER_GPU).
struct iqlhip_group {
  int K = 0;
  int n_items = 0;  // slots of every member's item table (deal_items: a whole network per XCD, rotated by member)
  iqlhip_trainer *tr[IQLHIP_MAX_GROUP] = {};  // (set by attach: none while the group is being built)
  void *mem = nullptr;  // [K] TrainerDesc | [K] DevArgs | [K] DevCtr | [K][n_items] UpdItem
  TrainerDesc *gdesc = nullptr;
  DevArgs *gargs = nullptr;
  DevCtr *gctr = nullptr;
  UpdItem *gitems = nullptr;
  StepQueue queue;  // of the group launches (K members per step)
  // a group of general-step trainers (iql_deep.hip): mem = [K] DeepDesc (the update table is member 0's: one
  // shape, one table); the arguments, counters and Adam coefficients of all members live in `deep_ring`.  The members keep their own
  // workspaces and argument blocks, so one stepped alone between group calls needs no hand-over.
  bool deep = false;
  DeepRing deep_ring;
  DeepDesc *gdeep = nullptr;
};

static void group_invalidate(iqlhip_group *g) { g->queue.dev_args_valid = false; }

static bool same_shape(const iqlhip_trainer_config &a, const iqlhip_trainer_config &b) {
  return a.state_dim == b.state_dim && a.action_dim == b.action_dim && a.hidden_dim == b.hidden_dim &&
         a.batch_size == b.batch_size && a.deterministic == b.deterministic && a.precision == b.precision &&
         n_critics(a) == n_critics(b) && (a.dropout_p > 0.f) == (b.dropout_p > 0.f) &&  // (polyak_form: per seed)
         n_hidden(a) == n_hidden(b);
}

// Member k of g: the trainer steps from its row of the group's arrays from here on (a general-step member
// keeps its own workspace and argument block, so one stepped alone between group calls needs no hand-over).
static void attach(iqlhip_group *g, int k, iqlhip_trainer *t) {
  g->tr[k] = t;
  t->group = g;
  if (g->deep) return;
  t->tuned->cur = {g->gdesc + k, g->gargs + k, g->gctr + k, g->gitems + (size_t)k * g->n_items, g->n_items};
  // the member's slots have moved: its next solo call must send its arguments and stage its first batch
  // again (`continues` would otherwise trust what the OLD slot held -- after a group, whatever the last solo
  // call OUTSIDE it sent), and its own graph holds the old descriptor addresses
  t->queue.dev_args_valid = false;
  t->queue.drop_graph();
}
// Back to its own workspace slots (with the group's current counters): usable on its own.
static void detach(iqlhip_trainer *t) {
  const bool deep = t->group->deep;
  t->group = nullptr;
  if (deep) return;
  TunedTrainer *u = t->tuned;
  (void)hipMemcpy(u->own.ctr, u->cur.ctr, sizeof(DevCtr), hipMemcpyDeviceToDevice);
  u->cur = u->own;
  t->queue.dev_args_valid = false;
  t->queue.drop_graph();
}

// Frees a group, finished or partly built (iqlhip_group_create's owner); its members stay usable.
static void group_release(iqlhip_group *g) {
  (void)hipDeviceSynchronize();
  for (int k = 0; k < g->K; ++k)
    if (g->tr[k]) detach(g->tr[k]);
  g->queue.destroy();
  g->deep_ring.destroy();
  (void)hipFree(g->mem);
  delete g;
}

extern "C" int iqlhip_group_create(iqlhip_group **out, iqlhip_trainer *const *trainers, int32_t n) {
  if (!out || !trainers) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n < 1 || n > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "group size %d: 1..%d", n, IQLHIP_MAX_GROUP);
  for (int k = 0; k < n; ++k) {
    if (!trainers[k]) return fail(IQLHIP_ERR_INVALID, "null trainer");
    if ((trainers[k]->deep != nullptr) != (trainers[0]->deep != nullptr))
      return fail(IQLHIP_ERR_INVALID, "trainer %d: a group holds trainers of the tuned step (n_hidden = 2, hidden_dim "
                  "64 / 128 / 256) or of the general step, not both", k);
    if (trainers[k]->group) return fail(IQLHIP_ERR_INVALID, "trainer %d already belongs to a group", k);
    for (int j = 0; j < k; ++j)
      if (trainers[j] == trainers[k]) return fail(IQLHIP_ERR_INVALID, "trainer %d listed twice", k);
    if (!same_shape(trainers[0]->cfg, trainers[k]->cfg) ||
        (trainers[0]->tuned && trainers[k]->tuned->own.n_items != trainers[0]->tuned->own.n_items))
      return fail(IQLHIP_ERR_INVALID, "trainer %d differs in shape from trainer 0 (dims, batch, precision, "
                  "critics, hidden layers, policy kind and dropout on/off must match)", k);
  }
  Owner<iqlhip_group, group_release> g(new (std::nothrow) iqlhip_group());
  if (!g) return fail(IQLHIP_ERR_NOMEM, "host allocation failed");
  g->K = n, g->deep = trainers[0]->deep != nullptr;
  if (g->deep) {
    hipError_t e = hipDeviceSynchronize();  // members may have steps in flight on other streams
    if (e == hipSuccess) e = hipMalloc(&g->mem, sizeof(DeepDesc) * n);
    g->gdeep = reinterpret_cast<DeepDesc *>(g->mem);
    if (e == hipSuccess) e = g->deep_ring.init(n);
    for (int k = 0; k < n && e == hipSuccess; ++k)
      e = hipMemcpy(g->gdeep + k, &deep_desc(trainers[k]->deep), sizeof(DeepDesc), hipMemcpyHostToDevice);
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? IQLHIP_ERR_NOMEM : IQLHIP_ERR_HIP, "general-step group: %s",
                  hipGetErrorString(e));
  } else {
    // the members' item tables, dealt for a group launch; one size for all
    std::vector<std::vector<UpdItem>> tables(n);
    {
      size_t depth = 0;
      for (int pass = 0; pass < 2; ++pass)
        for (int k = 0; k < n; ++k) {
          std::vector<UpdItem> per_xcd[8];
          deal_items(trainers[k]->tuned, k, n, per_xcd);
          size_t d = 0;
          tables[k] = flatten_table(per_xcd, depth, &d, (size_t)(trainers[k]->tuned->D.B + 15) / 16);
          depth = d > depth ? d : depth;
        }
    }
    const int ni = (int)tables[0].size();
    for (int k = 0; k < n; ++k)
      if ((int)tables[k].size() != ni) return fail(IQLHIP_ERR_INVALID, "item tables of the members differ in size");
    g->n_items = ni;
    // mem = [K] TrainerDesc | [K] DevArgs | [K] DevCtr | [K][n_items] UpdItem
    auto blocks = [&](WorkspacePlan p) {
      g->gdesc = p.take<TrainerDesc>(n);
      g->gargs = p.take<DevArgs>(n);
      g->gctr = p.take<DevCtr>(n);
      g->gitems = p.take<UpdItem>((size_t)ni * n);
      return p.end();
    };
    HIP_TRY(hipDeviceSynchronize());  // members may have steps in flight on other streams
    if (hipMalloc(&g->mem, blocks(WorkspacePlan())) != hipSuccess)
      return fail(IQLHIP_ERR_NOMEM, "hipMalloc of the group descriptors failed");
    blocks(WorkspacePlan(g->mem));
    hipError_t e = hipSuccess;
    for (int k = 0; k < n && e == hipSuccess; ++k) {
      const Slots &m = trainers[k]->tuned->cur;
      e = hipMemcpy(g->gdesc + k, m.desc, sizeof(TrainerDesc), hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipMemcpy(g->gargs + k, m.args, sizeof(DevArgs), hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipMemcpy(g->gctr + k, m.ctr, sizeof(DevCtr), hipMemcpyDeviceToDevice);
      if (e == hipSuccess)
        e = hipMemcpy(g->gitems + (size_t)k * ni, tables[k].data(), sizeof(UpdItem) * ni, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
      return fail(IQLHIP_ERR_HIP, "copying the member descriptors failed: %s", hipGetErrorString(e));
  }
  for (int k = 0; k < n; ++k) attach(g.get(), k, trainers[k]);
  *out = g.release();
  return 0;
}

extern "C" int iqlhip_group_destroy(iqlhip_group *g) {
  if (g) group_release(g);
  return 0;
}

extern "C" int iqlhip_group_train_steps(iqlhip_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                        const int64_t *const *idx, const uint8_t *const *dropout_keep,
                                        float *const *losses_out, int32_t graph_unroll, void *stream) {
  return iqlhip_group_train_steps_valid(g, views, n_steps, idx, nullptr, dropout_keep, losses_out, graph_unroll, stream);
}

extern "C" int iqlhip_group_train_steps_valid(iqlhip_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                              const int64_t *const *idx, const int32_t *const *n_valid,
                                              const uint8_t *const *dropout_keep, float *const *losses_out,
                                              int32_t graph_unroll, void *stream) {
  if (!g || !views) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n_steps < 0) return fail(IQLHIP_ERR_INVALID, "n_steps must be >= 0");
  // any member with counts: the counted k_backward for the whole launch (a member without uses its whole batch)
  bool counts = false;
  for (int k = 0; n_valid && k < g->K; ++k) counts = counts || n_valid[k] != nullptr;
  if (int rc = check_counts(g->tr[0], counts, "group")) return rc;
  for (int k = 0; k < g->K; ++k) {
    if (!views[k].rows) return fail(IQLHIP_ERR_INVALID, "null replay view %d", k);
    if (int rc = check_view(views[k], g->tr[k]->cfg)) return rc;
  }
  const iqlhip_trainer *t0 = g->tr[0];
  // (one pass, but for a padded batch with injected indices or masks: pad_inputs, every member's own copies)
  int64_t chunk = INT64_MAX;
  for (int k = 0; k < g->K; ++k)
    chunk = std::min(chunk, pad_chunk(g->tr[k], idx && idx[k], dropout_keep && dropout_keep[k]));
  const int64_t NB = t0->cfg.batch_size, keep_step = (int64_t)n_hidden(t0->cfg) * NB * t0->cfg.hidden_dim;
  for (int64_t done = 0; done < n_steps;) {
    const int64_t n = std::min(chunk, n_steps - done);
    DevArgs want[IQLHIP_MAX_GROUP];
    for (int k = 0; k < g->K; ++k) {
      iqlhip_trainer *t = g->tr[k];
      want[k] = make_args(t, views[k], n, idx && idx[k] ? idx[k] + done * NB : nullptr,
                          n_valid && n_valid[k] ? n_valid[k] + done : nullptr,
                          dropout_keep && dropout_keep[k] ? dropout_keep[k] + done * keep_step : nullptr,
                          losses_out && losses_out[k] ? losses_out[k] + done * 3 : nullptr);
      if (int rc = pad_inputs(t, want[k], (hipStream_t)stream)) return rc;
      t->queue.dev_args_valid = false;  // a member's own next call starts from scratch
    }
    const int rc = g->deep ? deep_run({g->tr, g->K, &g->deep_ring, g->gdeep, g->queue}, want, n, graph_unroll,
                                      (hipStream_t)stream)
                           : run_tuned(g->queue, {t0->tuned->bf16, t0->tuned->D, g->gdesc, g->gargs, g->gctr, g->gitems,
                                                  g->n_items, g->K},
                                       want, n, graph_unroll, counts, (hipStream_t)stream);
    if (rc) return rc;
    for (int k = 0; k < g->K; ++k) g->tr[k]->total_it += n;
    done += n;
  }
  return 0;
}

extern "C" int iqlhip_group_set_timing(iqlhip_group *g, int32_t enable) {
  return g ? g->queue.set_timing(enable != 0) : fail(IQLHIP_ERR_INVALID, "null group");
}

extern "C" int iqlhip_group_get_timing(iqlhip_group *g, double avg_ms[3], int64_t *n) {
  if (!g) return fail(IQLHIP_ERR_INVALID, "null group");
  g->queue.get_timing(avg_ms, n);
  return 0;
}

extern "C" int iqlhip_group_launch_counts(iqlhip_group *g, int64_t *eager_steps, int64_t *graph_launches) {
  if (!g) return fail(IQLHIP_ERR_INVALID, "null group");
  g->queue.launch_counts(eager_steps, graph_launches);
  return 0;
}

extern "C" int iqlhip_stream_create_cu_slice(void **stream, int32_t slice, int32_t n_slices) {
  if (!stream || n_slices < 1 || slice < 0 || slice >= n_slices)
    return fail(IQLHIP_ERR_INVALID, "stream slice %d of %d", slice, n_slices);
  int dev = 0, cus = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (cus < n_slices) return fail(IQLHIP_ERR_INVALID, "%d slices of %d compute units", n_slices, cus);
  std::vector<uint32_t> mask((cus + 31) / 32, 0u);
  for (int cu = slice; cu < cus; cu += n_slices) mask[cu >> 5] |= 1u << (cu & 31);
  hipStream_t st = nullptr;
  HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  *stream = st;
  return 0;
}
extern "C" int iqlhip_stream_destroy(void *stream) {
  if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return 0;
}

extern "C" int iqlhip_forward(iqlhip_trainer *t, int32_t which, const float *s, const float *a, int64_t n,
                              float *out, void *stream) {
  if (!t || !s || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (n <= 0) return fail(IQLHIP_ERR_INVALID, "n must be positive");
  if ((which == 0 || which == 3) && !a) return fail(IQLHIP_ERR_INVALID, "Q forward needs actions");
  hipStream_t st = (hipStream_t)stream;
  if (t->deep) {
    if (which < 0 || which > 3) return fail(IQLHIP_ERR_INVALID, "which must be 0..3");
    HIP_TRY(deep_infer(t->deep, which, s, a, n, out, st));
    return 0;
  }
  const TunedTrainer *u = t->tuned;
  const int E = u->D.E;
  FwdNet N;
  switch (which) {
    case 0:  // q_1 .. q_E -> out[n][E]
      for (int e = 0; e < E; ++e) {
        N = u->D.fwd[e], N.out_col = e, N.train_slot = -1, N.stage = 0;
        HIP_TRY(launch_infer(u->bf16, u->D, u->cur.desc, N, s, a, n, out, E, st));
      }
      return 0;
    case 1:
      N = u->D.fwd[E], N.out_col = 0, N.train_slot = -1;
      HIP_TRY(launch_infer(u->bf16, u->D, u->cur.desc, N, s, a, n, out, 1, st));
      return 0;
    case 2:  // eval-mode actor: no dropout (ref:299 actor.eval())
      N = u->D.fwd[E + 1], N.out_col = 0, N.train_slot = -1, N.dropout = 0;
      HIP_TRY(launch_infer(u->bf16, u->D, u->cur.desc, N, s, a, n, out, t->cfg.action_dim, st));
      return 0;
    case 3:  // target critics -> out[n][E]
      for (int e = 0; e < E; ++e) {
        N = u->D.fwd[E + 2 + e], N.out_col = e;
        HIP_TRY(launch_infer(u->bf16, u->D, u->cur.desc, N, s, a, n, out, E, st));
      }
      return 0;
    default:
      return fail(IQLHIP_ERR_INVALID, "which must be 0..3");
  }
}

// Diagnostic: attach a device buffer [3][512][8][2] u64 for IQL_STAMPS builds.
extern "C" int iqlhip_trainer_set_debug(iqlhip_trainer *t, void *buf) {
  if (!t) return fail(IQLHIP_ERR_INVALID, "null trainer");
  if (t->deep) return fail(IQLHIP_ERR_UNSUPPORTED, "no stamps in the general step");
  t->tuned->D.dbg = reinterpret_cast<unsigned long long *>(buf);
  HIP_TRY(hipMemcpy(t->tuned->cur.desc, &t->tuned->D, sizeof(TrainerDesc), hipMemcpyHostToDevice));
  t->queue.drop_graph();
  return 0;
}

// ------------------------------------------------------ exploration action --
// The actor of a trainer as launch_mlp_f32 takes it: the fp32 masters of the parameter arena where they lie
// (what every step's update writes: nothing is copied, nothing can go stale), for the tuned and the general
// step alike.  log_std: NULL for a deterministic policy.
static iqlhip_mlp_desc explore_actor(const iqlhip_trainer *t, uint32_t call, const float **log_std) {
  const iqlhip_trainer_config &c = t->cfg;
  const Layout L = make_layout(c);
  const int E = n_critics(c), NL = n_hidden(c) + 1, net = E + 1;
  iqlhip_mlp_desc d;
  memset(&d, 0, sizeof(d));
  d.n_layers = NL;
  d.dims[0] = c.state_dim;
  for (int l = 0; l < NL; ++l) {
    d.dims[l + 1] = l == NL - 1 ? c.action_dim : c.hidden_dim;
    d.weights[l] = t->arenas.params + L.off[(net * NL + l) * 2];
    d.biases[l] = t->arenas.params + L.off[(net * NL + l) * 2 + 1];
  }
  d.w_in_out = 0, d.hidden_act = 0, d.out_act = 1;
  // fref never leaves train mode outside eval_actor: with actor_dropout the exploring forward drops units
  d.dropout_p = c.dropout_p > 0.f ? c.dropout_p : 0.f;
  d.dropout_call = call, d.dropout_seed = c.seed;
  *log_std = c.deterministic ? nullptr : t->arenas.params + L.off[(E + 2) * NL * 2];
  return d;
}

// The actor's forward runs the stand-alone exact-fp32 MLP kernel straight on those masters;
// k_explore_epilogue then turns its output into the action in place.
extern "C" int iqlhip_explore_action(iqlhip_trainer *t, const float *s, int64_t rows, const float *eps,
                                     float expl_noise, float noise_clip, float max_action, uint32_t call,
                                     float *out, void *stream) {
  if (!t || !s || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (rows < 1 || rows > 0xffffffffLL) return fail(IQLHIP_ERR_INVALID, "rows = %lld outside 1..2^32 - 1", (long long)rows);
  const iqlhip_trainer_config &c = t->cfg;
  if (c.precision != IQLHIP_PREC_FP32)
    return fail(IQLHIP_ERR_UNSUPPORTED, "exploration actions need a precision fp32 trainer (the fine-tune flavour "
                                        "runs without autocast)");
  if (!(noise_clip >= 0.f) || !(max_action > 0.f) || !(expl_noise >= 0.f))
    return fail(IQLHIP_ERR_INVALID, "expl_noise and noise_clip must be >= 0, max_action > 0");
  const float *log_std;
  const iqlhip_mlp_desc d = explore_actor(t, call, &log_std);
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch_mlp_f32(d, s, rows, c.state_dim, out, c.action_dim, st));
  HIP_TRY(launch_explore_epilogue(out, rows, c.action_dim, log_std, eps, expl_noise, noise_clip, max_action, c.seed,
                                  call, st));
  return 0;
}

// One state row of each of K trainers: k_explore_group, one work-group per member on the same masters.
extern "C" int iqlhip_explore_action_group(iqlhip_trainer *const *trainers, int32_t K, const float *s,
                                           int32_t s_stride, const float *eps, float expl_noise, float noise_clip,
                                           float max_action, const uint32_t *calls, float *out, void *stream) {
  if (!trainers || !s || !calls || !out) return fail(IQLHIP_ERR_INVALID, "null argument");
  if (K < 1 || K > IQLHIP_MAX_GROUP) return fail(IQLHIP_ERR_INVALID, "K = %d: 1..%d members", K, IQLHIP_MAX_GROUP);
  if (!(noise_clip >= 0.f) || !(max_action > 0.f) || !(expl_noise >= 0.f))
    return fail(IQLHIP_ERR_INVALID, "expl_noise and noise_clip must be >= 0, max_action > 0");
  for (int k = 0; k < K; ++k) {
    if (!trainers[k]) return fail(IQLHIP_ERR_INVALID, "null trainer %d", k);
    const iqlhip_trainer_config &c = trainers[k]->cfg, &c0 = trainers[0]->cfg;
    if (c.precision != IQLHIP_PREC_FP32)
      return fail(IQLHIP_ERR_UNSUPPORTED, "trainer %d: exploration actions need a precision fp32 trainer (the "
                                          "fine-tune flavour runs without autocast)", k);
    if (trainers[k]->device != trainers[0]->device)
      return fail(IQLHIP_ERR_INVALID, "trainer %d lives on device %d, trainer 0 on device %d", k, trainers[k]->device,
                  trainers[0]->device);
    if (c.state_dim != c0.state_dim || c.action_dim != c0.action_dim)
      return fail(IQLHIP_ERR_INVALID, "trainer %d: state_dim %d, action_dim %d differ from trainer 0's %d, %d", k,
                  c.state_dim, c.action_dim, c0.state_dim, c0.action_dim);
  }
  if (s_stride < trainers[0]->cfg.state_dim)
    return fail(IQLHIP_ERR_INVALID, "s_stride = %d below state_dim = %d", s_stride, trainers[0]->cfg.state_dim);
  iqlhip_mlp_desc actors[IQLHIP_MAX_GROUP];
  const float *log_std[IQLHIP_MAX_GROUP];
  for (int k = 0; k < K; ++k) actors[k] = explore_actor(trainers[k], calls[k], &log_std[k]);
  HIP_TRY(launch_explore_group(actors, log_std, K, s, s_stride, eps, expl_noise, noise_clip, max_action, out,
                               (hipStream_t)stream));
  return 0;
}
