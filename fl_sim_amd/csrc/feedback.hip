// feedback.hip — error feedback for the compressed client messages (gfx950): a client's residual memory e, kept as
// the flat fp32 vector the encoders read.
//
// Per round and message vector (fl_sim_amd/feedback.py, compressed.py):
//   a  = fp32(e + fp32(local - cached))    flc_ef_accumulate, in place in e (a gradient list: a = fp32(e + x))
//   c  = compressors(a)                    the existing encoders with e as their flat input
//   e' = fp32(a - c)                       flc_ef_residual_round (stacked records) / flc_ef_residual_sparse_round
//                                          (sparse records) / flc_ef_residual_dense
// The stacked pipeline's c is nonzero only at the record's K kept indices, and a - (+0) == a bit for bit (a -0
// included), so its residual is K read-modify-writes per client, not a pass over e: one launch covers a round's
// clients (client on grid.y), each thread four consecutive entries of one record (one 16-B load of idx, one 4-B load
// of codes).  A record's indices are unique, so nothing is atomic; an index outside [0, n) — a record an encode that
// failed left behind — is skipped, so nothing is written outside e.  A sparse record (the top-k / rand-k wire,
// compressors.py:284-296) takes the same K-entry pass with its fp32 val field in place of the dequantised codes.
//
// The accumulate has delta_flatten_kernel's shape (delta.hip): a kernel-argument tensor pack, one 4096-element chunk
// of one tensor per 256-thread block, 16-B accesses where the operands and the tensor's slot in e are 16-B aligned
// (local and cached stream past L2: they are touched once; e is loaded and stored plainly: the encoder reads it next).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "flc_device.hpp"
#include "flc_runtime.hpp"

namespace flc {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;
constexpr int64_t kChunk = (int64_t)kThreads * 4 * kUnroll;  // elements per block
constexpr int kMaxT = 48;                                     // tensors per launch (kernel-argument budget)

struct TensorPack {
  const float* l[kMaxT];
  const float* g[kMaxT];
  int64_t off[kMaxT];
  int64_t n[kMaxT];
  int blk0[kMaxT + 1];  // first block of tensor t; blk0[nt] = grid size
  unsigned long long vec;  // bit t: 16-B path for tensor t
  int nt;
};

template <bool SUB>  // SUB: e += l - g; else e += l
__global__ __launch_bounds__(kThreads) void ef_accumulate_kernel(TensorPack p, float* __restrict__ e) {
  const int b = blockIdx.x;
  const int t = pack_entry<kMaxT>(p.blk0, p.nt, b);  // (uniform)
  const float* __restrict__ l = p.l[t];
  const float* __restrict__ g = p.g[t];
  float* __restrict__ o = e + p.off[t];
  const int64_t n = p.n[t];
  const int64_t c0 = (int64_t)(b - p.blk0[t]) * kChunk;
  if ((p.vec >> t) & 1ull) {
    const int64_t n4 = n >> 2;
    float4 d[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i4 = (c0 >> 2) + u * kThreads + threadIdx.x;
      ok[u] = i4 < n4;
      const int64_t j = ok[u] ? 4 * i4 : 0;
      float4 x = ld_stream(l + j);
      if (SUB) {
        const float4 c = ld_stream(g + j);
        x = make_float4(x.x - c.x, x.y - c.y, x.z - c.z, x.w - c.w);
      }
      const float4 m = *reinterpret_cast<const float4*>(o + j);
      d[u] = make_float4(m.x + x.x, m.y + x.y, m.z + x.z, m.w + x.w);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u]) *reinterpret_cast<float4*>(o + 4 * ((c0 >> 2) + u * kThreads + threadIdx.x)) = d[u];
    // the n % 4 tail, by the tensor's last block
    const int64_t tail = n & 3;
    if (c0 + kChunk >= n && (int64_t)threadIdx.x < tail) {
      const int64_t i = (n4 << 2) + threadIdx.x;
      o[i] = o[i] + (SUB ? l[i] - g[i] : l[i]);
    }
    return;
  }
  for (int u = 0; u < 4 * kUnroll; ++u) {
    const int64_t i = c0 + u * kThreads + threadIdx.x;
    if (i < n) o[i] = o[i] + (SUB ? l[i] - g[i] : l[i]);
  }
}

constexpr int kMaxC = 32;            // clients per launch (kernel-argument budget)
constexpr int kPerThread = 4;        // record entries per thread
struct ResidualPack {
  const uint8_t* rec[kMaxC];
  float* e[kMaxC];
};

// es[c][idx[j]] -= stacked_dequant(codes[j]) for the entries j < k of client c = blockIdx.y's record
__global__ __launch_bounds__(kThreads) void ef_residual_round_kernel(ResidualPack p, long long idx_off,
                                                                    long long codes_off, unsigned n, unsigned k,
                                                                    int levels, double step) {
  const int c = blockIdx.y;  // (uniform)
  const uint8_t* __restrict__ rec = p.rec[c];
  float* __restrict__ e = p.e[c];
  const float nrm = *reinterpret_cast<const float*>(rec);
  const unsigned* __restrict__ ix = reinterpret_cast<const unsigned*>(rec + idx_off);
  const uint8_t* __restrict__ cd = rec + codes_off;
  const unsigned j0 = (blockIdx.x * kThreads + threadIdx.x) * kPerThread;  // (k < 2^31: no wrap)
  if (j0 >= k) return;
  unsigned i[kPerThread], code[kPerThread];
  if (j0 + kPerThread <= k) {  // (idx and codes start 16-B aligned in a 16-B aligned record)
    const uint4 iv = *reinterpret_cast<const uint4*>(ix + j0);
    const unsigned cv = *reinterpret_cast<const unsigned*>(cd + j0);
    i[0] = iv.x, i[1] = iv.y, i[2] = iv.z, i[3] = iv.w;
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) code[r] = (cv >> (8 * r)) & 255u;
  } else {
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
      const bool in = j0 + r < k;
      i[r] = in ? ix[j0 + r] : 0xffffffffu;  // (past the record's end: an index no n admits)
      code[r] = in ? cd[j0 + r] : 0u;
    }
  }
  float m[kPerThread];
#pragma unroll
  for (int r = 0; r < kPerThread; ++r) m[r] = i[r] < n ? e[i[r]] : 0.0f;  // (unsigned compare: a negative index too)
#pragma unroll
  for (int r = 0; r < kPerThread; ++r)
    if (i[r] < n) e[i[r]] = m[r] - stacked_dequant(code[r], levels, step, nrm);
}

// es[c][idx[j]] -= val[j] for the entries j < k of client c = blockIdx.y's sparse record (flc_sparse_wire_layout): the
// kernel above with the record's fp32 values (one 16-B load) in place of its codes and norm
__global__ __launch_bounds__(kThreads) void ef_residual_sparse_round_kernel(ResidualPack p, long long idx_off,
                                                                           long long val_off, unsigned n, unsigned k) {
  const int c = blockIdx.y;  // (uniform)
  const uint8_t* __restrict__ rec = p.rec[c];
  float* __restrict__ e = p.e[c];
  const unsigned* __restrict__ ix = reinterpret_cast<const unsigned*>(rec + idx_off);
  const float* __restrict__ vl = reinterpret_cast<const float*>(rec + val_off);
  const unsigned j0 = (blockIdx.x * kThreads + threadIdx.x) * kPerThread;  // (k < 2^31: no wrap)
  if (j0 >= k) return;
  unsigned i[kPerThread];
  float v[kPerThread];
  if (j0 + kPerThread <= k) {  // (idx and val start 16-B aligned in a 16-B aligned record)
    const uint4 iv = *reinterpret_cast<const uint4*>(ix + j0);
    const float4 vv = *reinterpret_cast<const float4*>(vl + j0);
    i[0] = iv.x, i[1] = iv.y, i[2] = iv.z, i[3] = iv.w;
    v[0] = vv.x, v[1] = vv.y, v[2] = vv.z, v[3] = vv.w;
  } else {
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
      const bool in = j0 + r < k;
      i[r] = in ? ix[j0 + r] : 0xffffffffu;  // (past the record's end: an index no n admits)
      v[r] = in ? vl[j0 + r] : 0.0f;
    }
  }
  float m[kPerThread];
#pragma unroll
  for (int r = 0; r < kPerThread; ++r) m[r] = i[r] < n ? e[i[r]] : 0.0f;  // (unsigned compare: a negative index too)
#pragma unroll
  for (int r = 0; r < kPerThread; ++r)
    if (i[r] < n) e[i[r]] = m[r] - v[r];
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void ef_residual_dense_kernel(float* __restrict__ e, const float* __restrict__ c,
                                                                    int64_t n) {
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;
  if (VEC) {
    const int64_t n4 = n >> 2;
    float4 d[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i4 = (c0 >> 2) + u * kThreads + threadIdx.x;
      ok[u] = i4 < n4;
      const int64_t j = ok[u] ? 4 * i4 : 0;
      const float4 m = *reinterpret_cast<const float4*>(e + j), x = ld_stream(c + j);
      d[u] = make_float4(m.x - x.x, m.y - x.y, m.z - x.z, m.w - x.w);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u]) *reinterpret_cast<float4*>(e + 4 * ((c0 >> 2) + u * kThreads + threadIdx.x)) = d[u];
    const int64_t tail = n & 3;
    if (c0 + kChunk >= n && (int64_t)threadIdx.x < tail) {
      const int64_t i = (n4 << 2) + threadIdx.x;
      e[i] = e[i] - c[i];
    }
    return;
  }
  for (int u = 0; u < 4 * kUnroll; ++u) {
    const int64_t i = c0 + u * kThreads + threadIdx.x;
    if (i < n) e[i] = e[i] - c[i];
  }
}

}  // namespace
}  // namespace flc

using namespace flc;

extern "C" {

int flc_ef_accumulate(const float* const* local, const float* const* global, const int64_t* sizes, int n_tensors,
                      float* e, void* stream) {
  if (n_tensors < 0 || (n_tensors > 0 && (!local || !sizes))) return fail(FLC_EINVAL, "flc_ef_accumulate: bad arguments");
  // every tensor checked before the first launch of a chain
  int64_t total_blocks = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes[t] < 0) return fail(FLC_EINVAL, "flc_ef_accumulate: negative size for tensor %d", t);
    if (sizes[t] > 0 && (!local[t] || (global && !global[t]) || !e))
      return fail(FLC_EINVAL, "flc_ef_accumulate: null pointer for tensor %d", t);
    total_blocks += cdiv(sizes[t], kChunk);
    if (total_blocks > 0x7fffffff) return fail(FLC_EINVAL, "flc_ef_accumulate: too many elements");
  }
  hipStream_t st = as_stream(stream);
  int64_t off = 0;
  for (int t0 = 0; t0 < n_tensors; t0 += kMaxT) {
    TensorPack p{};
    int blocks = 0;
    p.nt = 0;
    for (int t = t0; t < std::min(n_tensors, t0 + kMaxT); ++t) {
      if (sizes[t] == 0) continue;
      const int i = p.nt++;
      p.l[i] = local[t];
      p.g[i] = global ? global[t] : nullptr;
      p.off[i] = off;
      p.n[i] = sizes[t];
      p.blk0[i] = blocks;
      // (the 16-B path clamps idle lanes to element 0..3, so it needs n >= 4)
      if (sizes[t] >= 4 && aligned16(local[t]) && (!global || aligned16(global[t])) && aligned16(e + off))
        p.vec |= 1ull << i;
      blocks += (int)cdiv(sizes[t], kChunk);
      off += sizes[t];
    }
    p.blk0[p.nt] = blocks;
    if (blocks == 0) continue;
    if (global)
      FLC_LAUNCH("ef_accumulate", ef_accumulate_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, p, e);
    else
      FLC_LAUNCH("ef_accumulate", ef_accumulate_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, p, e);
  }
  return FLC_OK;
}

// flc_ef_residual_round (sparse_rec false: stacked records) and flc_ef_residual_sparse_round: one argument check, one
// chain of launches of <= kMaxC clients
static int ef_residual_impl(const char* fn, bool sparse_rec, const void* const* records, float* const* es,
                            int n_clients, int64_t n, int64_t k, int levels, void* stream) {
  if (n_clients < 0 || (n_clients > 0 && (!records || !es)) || n < 0 || k < 0)
    return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (n >= (1ll << 31) || k >= (1ll << 31)) return fail(FLC_EINVAL, "%s: n and k must be < 2^31", fn);
  if (k > n) return fail(FLC_EINVAL, "%s: k %lld > n %lld", fn, (long long)k, (long long)n);
  if (!sparse_rec && (levels < 1 || levels > 127)) return fail(FLC_EINVAL, "%s: levels must be in [1, 127]", fn);
  std::vector<std::pair<const float*, int>> owners;
  owners.reserve((size_t)n_clients);
  for (int c = 0; c < n_clients; ++c) {
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
    if (!es[c]) return fail(FLC_EINVAL, "%s: null memory for client %d", fn, c);
    owners.emplace_back(es[c], c);
  }
  std::sort(owners.begin(), owners.end());
  for (size_t i = 1; i < owners.size(); ++i)
    if (owners[i].first == owners[i - 1].first)
      return fail(FLC_EINVAL, "%s: clients %d and %d share a memory", fn,
                  std::min(owners[i - 1].second, owners[i].second), std::max(owners[i - 1].second, owners[i].second));
  if (n_clients == 0 || k == 0) return FLC_OK;
  int64_t off[4];
  if ((sparse_rec ? flc_sparse_wire_layout(n, k, off) : flc_stacked_wire_layout(n, k, off)) == 0)
    return fail(FLC_EINVAL, "%s: bad arguments", fn);
  hipStream_t st = as_stream(stream);
  const double step = 1.0 / (double)(levels < 1 ? 1 : levels);
  const unsigned gx = (unsigned)cdiv(k, (int64_t)kThreads * kPerThread);
  for (int c0 = 0; c0 < n_clients; c0 += kMaxC) {
    const int nc = std::min(n_clients - c0, kMaxC);
    ResidualPack p{};
    for (int c = 0; c < nc; ++c) {
      p.rec[c] = static_cast<const uint8_t*>(records[c0 + c]);
      p.e[c] = es[c0 + c];
    }
    if (sparse_rec)
      FLC_LAUNCH("ef_residual_sparse_round", ef_residual_sparse_round_kernel, dim3(gx, (unsigned)nc), dim3(kThreads), 0,
                 st, p, (long long)off[0], (long long)off[1], (unsigned)n, (unsigned)k);
    else
      FLC_LAUNCH("ef_residual_round", ef_residual_round_kernel, dim3(gx, (unsigned)nc), dim3(kThreads), 0, st, p,
                 (long long)off[1], (long long)off[2], (unsigned)n, (unsigned)k, levels, step);
  }
  return FLC_OK;
}

int flc_ef_residual_round(const void* const* records, float* const* es, int n_clients, int64_t n, int64_t k,
                          int levels, void* stream) {
  return ef_residual_impl("flc_ef_residual_round", false, records, es, n_clients, n, k, levels, stream);
}

int flc_ef_residual_sparse_round(const void* const* records, float* const* es, int n_clients, int64_t n, int64_t k,
                                 void* stream) {
  return ef_residual_impl("flc_ef_residual_sparse_round", true, records, es, n_clients, n, k, 0, stream);
}

int flc_ef_residual_dense(float* e, const float* c, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!e || !c))) return fail(FLC_EINVAL, "flc_ef_residual_dense: bad arguments");
  if (e && e == c) return fail(FLC_EINVAL, "flc_ef_residual_dense: e and c are the same vector");
  if (n == 0) return FLC_OK;
  const int64_t blocks = cdiv(n, kChunk);
  if (blocks > 0x7fffffff) return fail(FLC_EINVAL, "flc_ef_residual_dense: too many elements");
  hipStream_t st = as_stream(stream);
  if (n >= 4 && aligned16(e) && aligned16(c))
    FLC_LAUNCH("ef_residual_dense", ef_residual_dense_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, e, c, n);
  else
    FLC_LAUNCH("ef_residual_dense", ef_residual_dense_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, e, c,
               n);
  return FLC_OK;
}

}  // extern "C"
