// robust.hip — coordinate-wise median and trimmed mean of a round's messages for gfx950, fused with the FedOpt step
// (Yin et al. 2018, "Byzantine-Robust Distributed Learning"; the semantics are pinned in include/flcodec.h).
//
// Per coordinate the C messages' values are sorted across the CLIENT axis in registers and one rule value r comes
// out; then exactly model_fold_kernel's tail: a = fmaf(scale, r, init(dst)), dst = a, opt_step on theta / v.  Every
// source element is read once, dst / theta / v written once; no atomics, no LDS, no grid-wide wait.
//
// The sort: the values become IEEE totalOrder keys on load (k = bits ^ ((bits >> 31) & 0x7fffffff), a signed int32
// whose integer order is the total order: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN; the map is its own
// inverse).  A compare-exchange is v_min_i32 + v_max_i32, so a NaN is a key like any other and nothing is ever
// duplicated or lost.  The network is Batcher's odd-even merge sort for the padded client count P in {4, 8, 16, 32,
// 64} (5 / 19 / 63 / 191 / 543 exchanges), built at compile time into a table and expanded with constant indices, so
// the keys are named registers (no scratch).  Slots past C hold INT32_MAX, which is +NaN's largest payload and sorts
// at or above every real key: real ranks do not move.
//
// Work split: a lane holds P x W keys, W coordinates of every client, with P x W = 64 VGPRs in the three large
// classes: W = 4 (16-B loads) up to P = 16, W = 2 (8-B loads) at P = 32, W = 1 at P = 64.  All P loads of a lane's
// group are issued before the first compare.  Block b serves one chunk of 256 x W elements of one tensor, found from
// the pack's block offsets (pack_entry).  A tensor whose operands are not 4W-byte aligned, and an n % W tail, take
// the same network one coordinate per lane.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>
#include <utility>

#include "flc_device.hpp"
#include "flc_runtime.hpp"

namespace flc {
namespace {

constexpr int kThreads = 256;

// coordinates per lane at P = 32 and P = 64 (1, 2 or 4).  The defaults are the supported build; other values exist
// only to rebuild the widths that lost for tools/robust_probe.py and are not tested
#ifndef FLC_ROBUST_W32
#define FLC_ROBUST_W32 2
#endif
#ifndef FLC_ROBUST_W64
#define FLC_ROBUST_W64 1
#endif
constexpr int robust_width(int P) { return P <= 16 ? 4 : (P == 32 ? FLC_ROBUST_W32 : FLC_ROBUST_W64); }
// tensors per launch: about 256 source pointers in the kernel arguments, at most 32 tensors (the `vec` mask)
constexpr int robust_tensors(int P) { return P <= 8 ? 32 : 256 / P; }

template <int P>
struct RobustPack {
  static constexpr int T = robust_tensors(P);
  float* dst[T];
  float* theta[T];
  float* v[T];
  const float* src[P][T];
  int64_t n[T];
  int blk0[T + 1];
  unsigned vec;  // bit t: tensor t's operands are aligned for the W-wide form
  int nt, ns;
};

struct RobustArgs {  // (uniform scalars)
  int trim, init, opt;  // opt < 0: the fold only
  float scale, beta, lr, beta2, omb, nomb, tau;
};

// ---- Batcher's odd-even merge sort on P inputs as a compile-time table of compare-exchanges --------------------
template <int P>
struct Network {
  static constexpr int kMax = P == 4 ? 5 : P == 8 ? 19 : P == 16 ? 63 : P == 32 ? 191 : 543;
  unsigned char a[kMax] = {}, b[kMax] = {};
  int count = 0;
  constexpr Network() {
    for (int p = 1; p < P; p <<= 1)
      for (int k = p; k >= 1; k >>= 1)
        for (int j = k % p; j + k < P; j += 2 * k)
          for (int i = 0; i < k && i + j + k < P; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
              a[count] = (unsigned char)(i + j);
              b[count] = (unsigned char)(i + j + k);
              ++count;
            }
  }
};
template <int P>
inline constexpr Network<P> kNetwork{};
static_assert(kNetwork<4>.count == 5 && kNetwork<8>.count == 19 && kNetwork<16>.count == 63 &&
              kNetwork<32>.count == 191 && kNetwork<64>.count == 543, "Batcher exchange counts");

__device__ __forceinline__ int total_key(float x) {
  const int b = __float_as_int(x);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

template <int W>
__device__ __forceinline__ void exchange(int (&lo)[W], int (&hi)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const int x = lo[j], y = hi[j];
    lo[j] = min(x, y);
    hi[j] = max(x, y);
  }
}

template <int P, int W, size_t... I>
__device__ __forceinline__ void sort_keys(int (&k)[P][W], std::index_sequence<I...>) {
  // (a braced list evaluates left to right and has no nesting limit, where a 543-term fold expression has one)
  const int order[] = {(exchange<W>(k[kNetwork<P>.a[I]], k[kNetwork<P>.b[I]]), 0)...};
  (void)order;
}

template <int W>
__device__ __forceinline__ void load_w(const float* p, float (&x)[W]) {
  if constexpr (W == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
  } else if constexpr (W == 2) {
    const float2 q = *reinterpret_cast<const float2*>(p);
    x[0] = q.x, x[1] = q.y;
  } else {
    x[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void store_w(float* p, const float (&x)[W]) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  else if constexpr (W == 2) *reinterpret_cast<float2*>(p) = make_float2(x[0], x[1]);
  else *p = x[0];
}

template <int OPT, int W>
__device__ __forceinline__ void step_w(float* theta, float* v, const float (&a)[W], const RobustArgs& g) {
  float th[W];
  load_w<W>(theta, th);
#pragma unroll
  for (int j = 0; j < W; ++j) opt_step<OPT>(th[j], a[j], OPT > 0 ? v + j : nullptr, g.lr, g.beta2, g.omb, g.nomb, g.tau);
  store_w<W>(theta, th);
}

// W consecutive coordinates of tensor t from element e on: load, sort, rule, store, step
template <int P, int W, int RULE>
__device__ __forceinline__ void fold_group(const RobustPack<P>& p, const RobustArgs& g, int t, int64_t e) {
  const int C = p.ns;
  int k[P][W];
  {
    float x[P][W];
#pragma unroll
    for (int m = 0; m < P; ++m)  // every load of the group in flight before the first compare
      if (m < C) load_w<W>(p.src[m][t] + e, x[m]);
#pragma unroll
    for (int m = 0; m < P; ++m)
#pragma unroll
      for (int j = 0; j < W; ++j) k[m][j] = m < C ? total_key(x[m][j]) : INT_MAX;
  }
  float* __restrict__ dst = p.dst[t] + e;
  float a[W];
  if (g.init == 1) {
#pragma unroll
    for (int j = 0; j < W; ++j) a[j] = 0.0f;
  } else {
    load_w<W>(dst, a);
    if (g.init == 0) {
#pragma unroll
      for (int j = 0; j < W; ++j) a[j] = a[j] * g.beta;
    }
  }
  sort_keys<P, W>(k, std::make_index_sequence<(size_t)kNetwork<P>.count>{});
  float r[W];
  if (RULE == FLC_ROBUST_MEDIAN) {
    const int lo = (C - 1) >> 1, hi = C >> 1;  // (uniform; the selects below keep every register index constant)
    int klo[W], khi[W];
#pragma unroll
    for (int j = 0; j < W; ++j) klo[j] = khi[j] = k[0][j];
#pragma unroll
    for (int m = 1; m < P; ++m)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        klo[j] = m == lo ? k[m][j] : klo[j];
        khi[j] = m == hi ? k[m][j] : khi[j];
      }
#pragma unroll
    for (int j = 0; j < W; ++j)
      r[j] = (C & 1) ? key_float(klo[j]) : 0.5f * key_float(klo[j]) + 0.5f * key_float(khi[j]);
  } else {
    const int lo = g.trim, hi = C - g.trim;  // kept ranks [lo, hi), summed ascending from -0 (-0 + x = x for every x)
#pragma unroll
    for (int j = 0; j < W; ++j) r[j] = -0.0f;
#pragma unroll
    for (int m = 0; m < P; ++m)
      if (m >= lo && m < hi) {
#pragma unroll
        for (int j = 0; j < W; ++j) r[j] = r[j] + key_float(k[m][j]);
      }
    const float cnt = (float)(hi - lo);
#pragma unroll
    for (int j = 0; j < W; ++j) r[j] = r[j] / cnt;
  }
#pragma unroll
  for (int j = 0; j < W; ++j) a[j] = fmaf(g.scale, r[j], a[j]);
  store_w<W>(dst, a);
  if (g.opt < 0) return;
  float* theta = p.theta[t] + e;
  float* v = g.opt > 0 ? p.v[t] + e : nullptr;
  if (g.opt == FLC_OPT_AVG) step_w<FLC_OPT_AVG, W>(theta, v, a, g);
  else if (g.opt == FLC_OPT_ADAGRAD) step_w<FLC_OPT_ADAGRAD, W>(theta, v, a, g);
  else if (g.opt == FLC_OPT_YOGI) step_w<FLC_OPT_YOGI, W>(theta, v, a, g);
  else step_w<FLC_OPT_ADAM, W>(theta, v, a, g);
}

template <int P, int RULE>
__global__ __launch_bounds__(kThreads) void robust_fold_kernel(RobustPack<P> p, RobustArgs g) {
  constexpr int W = robust_width(P);
  constexpr int kChunk = kThreads * W;
  const int b = blockIdx.x;
  const int t = pack_entry<RobustPack<P>::T>(p.blk0, p.nt, b);  // (uniform)
  const int64_t n = p.n[t];
  const int64_t c0 = (int64_t)(b - p.blk0[t]) * kChunk;
  const int64_t c1 = c0 + kChunk < n ? c0 + kChunk : n;
  // one coordinate per lane: the whole chunk of an unaligned tensor, or the n % W tail behind the W-wide groups
  int64_t e = c0 + threadIdx.x, step = kThreads;
  if (W > 1 && ((p.vec >> t) & 1u)) {
    e = c0 + W * (int64_t)threadIdx.x;
    step = 1;
    if (e + W <= c1) {
      fold_group<P, W, RULE>(p, g, t, e);
      return;
    }
  }
  for (; e < c1; e += step) fold_group<P, 1, RULE>(p, g, t, e);
}

template <int P>
int launch_class(float* const* dst, const float* const* srcs, int n_src, const int64_t* sizes, int n_tensors, int rule,
                 const RobustArgs& g, float* const* theta, float* const* v, hipStream_t st) {
  constexpr int W = robust_width(P), T = RobustPack<P>::T;
  constexpr unsigned amask = 4u * W - 1u;
  auto aligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & amask) == 0; };
  int t = 0;
  while (t < n_tensors) {
    RobustPack<P> p{};
    p.ns = n_src;
    int blocks = 0;
    for (; t < n_tensors && p.nt < T; ++t) {
      if (sizes[t] == 0) continue;
      const int64_t nb = cdiv(sizes[t], (int64_t)kThreads * W);
      if (blocks + nb > 0x7fffffff) break;  // (the next launch takes it; one tensor alone was checked to fit)
      const int i = p.nt++;
      p.dst[i] = dst[t];
      p.theta[i] = theta ? theta[t] : nullptr;
      p.v[i] = (theta && v) ? v[t] : nullptr;
      p.n[i] = sizes[t];
      bool vec = aligned(dst[t]) && aligned(p.theta[i]) && aligned(p.v[i]);
      for (int m = 0; m < n_src; ++m) {
        p.src[m][i] = srcs[(size_t)m * n_tensors + t];
        vec = vec && aligned(p.src[m][i]);
      }
      if (vec) p.vec |= 1u << i;
      p.blk0[i] = blocks;
      blocks += (int)nb;
    }
    p.blk0[p.nt] = blocks;
    if (blocks == 0) continue;
    if (rule == FLC_ROBUST_MEDIAN)
      FLC_LAUNCH("robust_fold", (robust_fold_kernel<P, FLC_ROBUST_MEDIAN>), dim3(blocks), dim3(kThreads), 0, st, p, g);
    else
      FLC_LAUNCH("robust_fold", (robust_fold_kernel<P, FLC_ROBUST_TRIMMED>), dim3(blocks), dim3(kThreads), 0, st, p, g);
  }
  return FLC_OK;
}

}  // namespace
}  // namespace flc

using namespace flc;

extern "C" {

int flc_robust_fold(float* const* dst, const float* const* srcs, int n_src, const int64_t* sizes, int n_tensors,
                    int rule, int trim, float scale, int init_mode, float beta, float* const* theta, float* const* v,
                    int opt, double lr, double beta2, double tau, void* stream) {
  // everything is checked before anything touches the device
  if (rule != FLC_ROBUST_MEDIAN && rule != FLC_ROBUST_TRIMMED)
    return fail(FLC_EINVAL, "flc_robust_fold: unknown rule %d", rule);
  if (n_src < 1 || n_src > FLC_ROBUST_MAX_SRC)
    return fail(FLC_EINVAL, "flc_robust_fold: n_src must be 1 .. %d (got %d): the client axis is sorted in one launch",
                FLC_ROBUST_MAX_SRC, n_src);
  if (trim < 0 || 2 * (int64_t)trim >= n_src)
    return fail(FLC_EINVAL, "flc_robust_fold: trim must satisfy 0 <= 2 * trim < n_src (trim %d, n_src %d)", trim, n_src);
  if (init_mode < 0 || init_mode > 2) return fail(FLC_EINVAL, "flc_robust_fold: init_mode must be 0, 1 or 2");
  const bool step = theta != nullptr;
  if (step && opt != FLC_OPT_AVG && opt != FLC_OPT_ADAGRAD && opt != FLC_OPT_YOGI && opt != FLC_OPT_ADAM)
    return fail(FLC_EINVAL, "flc_robust_fold: unknown opt %d", opt);
  if (step && opt != FLC_OPT_AVG && !v) return fail(FLC_EINVAL, "flc_robust_fold: v required for an adaptive opt");
  if (n_tensors < 0 || (n_tensors > 0 && (!dst || !sizes || !srcs)))
    return fail(FLC_EINVAL, "flc_robust_fold: bad arguments (n_tensors, dst, sizes, srcs)");
  const bool adaptive = step && opt != FLC_OPT_AVG;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes[t] < 0) return fail(FLC_EINVAL, "flc_robust_fold: negative sizes[%d]", t);
    if (sizes[t] == 0) continue;
    if (sizes[t] > (int64_t)0x7fffffff * kThreads) return fail(FLC_EINVAL, "flc_robust_fold: sizes[%d] too large", t);
    if (!dst[t] || (step && !theta[t]) || (adaptive && !v[t]))
      return fail(FLC_EINVAL, "flc_robust_fold: null pointer for tensor %d", t);
    for (int m = 0; m < n_src; ++m)
      if (!srcs[(size_t)m * n_tensors + t]) return fail(FLC_EINVAL, "flc_robust_fold: null source %d of tensor %d", m, t);
  }
  RobustArgs g{};
  g.trim = trim, g.init = init_mode, g.opt = step ? opt : -1;
  g.scale = scale, g.beta = beta, g.lr = (float)lr, g.beta2 = (float)beta2, g.tau = (float)tau;
  g.omb = (float)(1.0 - beta2), g.nomb = (float)(-(1.0 - beta2));
  hipStream_t st = as_stream(stream);
  float* const* vv = adaptive ? v : nullptr;
  if (n_src <= 4) return launch_class<4>(dst, srcs, n_src, sizes, n_tensors, rule, g, theta, vv, st);
  if (n_src <= 8) return launch_class<8>(dst, srcs, n_src, sizes, n_tensors, rule, g, theta, vv, st);
  if (n_src <= 16) return launch_class<16>(dst, srcs, n_src, sizes, n_tensors, rule, g, theta, vv, st);
  if (n_src <= 32) return launch_class<32>(dst, srcs, n_src, sizes, n_tensors, rule, g, theta, vv, st);
  return launch_class<64>(dst, srcs, n_src, sizes, n_tensors, rule, g, theta, vv, st);
}

}  // extern "C"
