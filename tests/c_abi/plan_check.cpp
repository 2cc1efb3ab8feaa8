// Stand-alone check of iqlpref_amd/csrc/host_plan.h (plain C++17, no HIP, no Python): the workspace planner's
// two passes agree and place every block where a hand count puts it, and the shared dropout helper gives the
// constants the trainer descriptors always held.  Exit status 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_plan.h"

using iqlhip::WorkspacePlan;

struct Odd7 {
  char c[7];
};
struct alignas(128) Line {
  char c[128];
};

constexpr int N_REQ = 11;
struct Block {
  char *p;
  size_t bytes;
};
// the one list of requests both passes run: mixed types, sizes around the 256-byte granule
static size_t requests(WorkspacePlan p, Block (&b)[N_REQ]) {
  int i = 0;
  auto take = [&](auto *tag, size_t n) {
    using T = std::remove_pointer_t<decltype(tag)>;
    b[i++] = {reinterpret_cast<char *>(p.take<T>(n)), n * sizeof(T)};
  };
  take((char *)nullptr, 0);        //    0 bytes
  take((char *)nullptr, 1);        //    1
  take((char *)nullptr, 255);      //  255
  take((char *)nullptr, 256);      //  256
  take((char *)nullptr, 257);      //  257
  take((float *)nullptr, 3);       //   12
  take((double *)nullptr, 33);     //  264
  take((uint16_t *)nullptr, 128);  //  256
  take((Odd7 *)nullptr, 37);       //  259
  take((int64_t *)nullptr, 1);     //    8
  take((Line *)nullptr, 3);        //  384
  return p.end();
}
// counted by hand: each block starts where the one before ends, rounded up to 256
static const size_t WANT_OFF[N_REQ] = {0, 0, 256, 512, 768, 1280, 1536, 2048, 2304, 2816, 3072};
static const size_t WANT_TOTAL = 3584;

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  Block m[N_REQ], b[N_REQ];
  const size_t total = requests(WorkspacePlan(), m);
  CHECK(total == WANT_TOTAL);
  for (const Block &x : m) CHECK(x.p == nullptr);  // the measuring pass hands out nothing
  char *base = static_cast<char *>(aligned_alloc(256, total));
  if (!base) return 2;
  const size_t end = requests(WorkspacePlan(base), b);
  CHECK(end == total);
  size_t prev_end = 0;
  for (int i = 0; i < N_REQ; ++i) {
    const size_t off = (size_t)(b[i].p - base);
    CHECK(off == WANT_OFF[i]);
    CHECK(off % 256 == 0);
    CHECK(off >= prev_end);                 // request order, no overlap
    CHECK(off + b[i].bytes <= total);
    CHECK(b[i].bytes == m[i].bytes);
    prev_end = off + b[i].bytes;
    memset(b[i].p, 0x5a, b[i].bytes);       // (every byte of every block is the caller's to write)
  }
  free(base);

  // dropout_p, bf16, bits of the scale, keep threshold: from the expression in iqlhip_trainer_create / deep_create
  // before the helper existed (1 / (1 - p) in float, rounded to bf16 to nearest even under bf16; p * 2^32)
  const struct {
    float p;
    bool bf16;
    uint32_t scale_bits, thr;
  } want[] = {{0.1f, false, 0x3f8e38e4u, 429496736u},
              {0.1f, true, 0x3f8e0000u, 429496736u},
              {0.5f, false, 0x40000000u, 2147483648u},
              {0.5f, true, 0x40000000u, 2147483648u}};
  for (const auto &w : want) {
    const iqlhip::DropoutConsts c = iqlhip::dropout_consts(w.p, w.bf16);
    uint32_t bits;
    memcpy(&bits, &c.scale, 4);
    CHECK(bits == w.scale_bits);
    CHECK(c.thr == w.thr);
    const iqlhip::StepShape s = iqlhip::make_step_shape(17, 6, 0, 0, w.p, w.bf16);
    CHECK(s.has_dropout && s.drop.thr == w.thr && memcmp(&s.drop.scale, &bits, 4) == 0);
  }
  const iqlhip::StepShape none = iqlhip::make_step_shape(17, 6, 0, 0, 0.f, true);
  CHECK(!none.has_dropout && none.drop.thr == 0u && none.drop.scale == 0.f);
  CHECK(none.E == 2 && none.NH == 2);  // the defaults of a zero in the config

  if (failures) return 1;
  printf("ok\n");
  return 0;
}
