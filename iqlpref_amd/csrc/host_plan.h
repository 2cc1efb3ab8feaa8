// Host-only helpers that both trainer constructions (api.hip: the tuned step, iql_deep.hip: the general
// step) build from: the workspace planner, what is derived from a config once, the owner of a partly built
// object and the run-time -> compile-time dispatcher of the kernel selection.  Plain C++17, no HIP include:
// tests/c_abi/plan_check.cpp uses it on its own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

namespace iqlhip {

// One list of requests sizes AND places a workspace.  Driven with no base it measures (take() returns null,
// end() is the total); driven again over the allocation of that size it hands out the pointers.  Every block
// starts on 256 bytes.
class WorkspacePlan {
 public:
  static constexpr size_t ALIGN = 256;
  explicit WorkspacePlan(void *base = nullptr) : base_(static_cast<char *>(base)) {}
  // n elements of T
  template <typename T>
  T *take(size_t n) {
    T *r = base_ ? reinterpret_cast<T *>(base_ + off_) : nullptr;
    off_ += (n * sizeof(T) + ALIGN - 1) / ALIGN * ALIGN;
    return r;
  }
  size_t end() const { return off_; }

 private:
  char *base_;
  size_t off_ = 0;
};

// Inverted dropout as the kernels apply it: keep where a 32-bit draw >= thr, scale what is kept.
struct DropoutConsts {
  float scale;
  uint32_t thr;
};
inline DropoutConsts dropout_consts(float p, bool bf16) {
  DropoutConsts c;
  c.scale = 1.0f / (float)(1.0 - (double)p);
  if (bf16) {  // noise.div_(1-p) happens in bf16 under autocast (ATen _dropout_impl)
    uint32_t u;
    memcpy(&u, &c.scale, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    memcpy(&c.scale, &u, 4);
  }
  const double thr = (double)p * 4294967296.0;
  c.thr = thr >= 4294967295.0 ? 0xffffffffu : (uint32_t)thr;
  return c;
}

// What both step kinds derive from a config: the resolved defaults, the numbering of nets and output
// columns (iql_step.h) and the dropout constants (zero without dropout).
struct StepShape {
  int S, A;
  int E;   // critics: 0 in the config means the reference's TwinQ
  int NH;  // hidden layers: 0 in the config means the reference's default (ref:458-459, 519, 538)
  bool has_dropout;
  DropoutConsts drop;
  int ntrain() const { return E + 2; }
  int nfwd() const { return 2 * E + 3; }
  int net_v() const { return E; }
  int net_a() const { return E + 1; }
  int out_v() const { return E; }
  int out_qt() const { return E + 1; }
  int out_nv() const { return 2 * E + 1; }
  int out_mean() const { return 2 * E + 2; }
  int in_dim(int net) const { return net < E ? S + A : S; }
  int out_dim(int net) const { return net == net_a() ? A : 1; }
};
inline StepShape make_step_shape(int S, int A, int n_critics, int n_hidden, float dropout_p, bool bf16) {
  StepShape s{S, A, n_critics > 0 ? n_critics : 2, n_hidden > 0 ? n_hidden : 2, dropout_p > 0.f, {0.f, 0u}};
  if (s.has_dropout) s.drop = dropout_consts(dropout_p, bf16);
  return s;
}

// The forward evaluations of a step in their order: q_e, v, actor, target q_e, next_v (iql_step.h).
struct EvalSpec {
  int net;
  bool target;
  int in_off;   // float offset of the input inside a replay row
  int out_col;
  int slot;     // trained net whose activation planes the evaluation writes, or -1
};
inline std::vector<EvalSpec> eval_order(const StepShape &s, int next_off) {
  std::vector<EvalSpec> v;
  for (int e = 0; e < s.E; ++e) v.push_back({e, false, 0, e, e});
  v.push_back({s.net_v(), false, 0, s.out_v(), s.net_v()});
  v.push_back({s.net_a(), false, 0, s.out_mean(), s.net_a()});
  for (int e = 0; e < s.E; ++e) v.push_back({e, true, 0, s.out_qt() + e, -1});
  v.push_back({s.net_v(), false, next_off, s.out_nv(), -1});
  return v;
}

// Holds an object under construction: unless release()d it goes to Destroy, the function that also destroys
// a finished one (which therefore takes any partly built state).
template <typename T, void (*Destroy)(T *)>
struct DestroyWith {
  void operator()(T *p) const { Destroy(p); }
};
template <typename T, void (*Destroy)(T *)>
using Owner = std::unique_ptr<T, DestroyWith<T, Destroy>>;

// Kernel selection: f(std::integral_constant<.., V>) for the V of Vs... that equals v; the last one also
// takes every other value (the `else` of a ladder).  Only the listed values are ever instantiated.  CV(x)
// reads the constant inside f, Int / Bool spell a fixed one.
#define CV(x) decltype(x)::value
template <int V>
using Int = std::integral_constant<int, V>;
template <bool V>
using Bool = std::integral_constant<bool, V>;
template <auto V, auto... Rest, typename T, typename F>
inline void with_const(T v, F &&f) {
  if constexpr (sizeof...(Rest) == 0) {
    f(std::integral_constant<decltype(V), V>{});
  } else {
    if (v == V)
      f(std::integral_constant<decltype(V), V>{});
    else
      with_const<Rest...>(v, static_cast<F &&>(f));
  }
}

}  // namespace iqlhip
