// wire.hip — the stacked codec's packed wire and the server-side fold of many clients' wires in one pass (gfx950).
//
// Packed wire (one contiguous, 256-B-aligned record per client; the layout is a function of (n, k) only, so a
// [clients, stride] byte tensor can be all-gathered over RCCL or copied over PCIe as one piece):
//   [0, 4)                     norm       fp32, the kept set's max |value| (compressors.py:344's pnorm at p = inf)
//   [16, 16 + 4k)              idx        int32, ascending
//   [codes, codes + max(k,16)) codes      u8, sign << 7 | level
//   [tiles, tiles + 4(T+1))    tiles      u32 CSR pointers over FLC_TILE-output tiles (T = ceil(n / FLC_TILE))
// The encoder writes it directly (flc_stacked_encode_tiled with the four pointers inside the record).
//
// Fold (flc_stacked_fold_wires): out = fmaf(w_c, decode(wire_c), out) for c = 0 .. m-1 in order, every element,
// every client — the server's sequential fold (nodes.py:1165-1180, _fedopt.py:202-208) in ONE
// pass over `out` instead of one decode-accumulate pass (read + write of 4n bytes) per client.  One 64-lane wave
// per 1024-output tile keeps its slice of the accumulator in registers; per client the tile's kept entries are
// scattered into a 4 KB LDS tile, read back densely (zeros included: fmaf(w, +0, acc) is applied exactly as the
// dense per-client fold applies it), and the scattered slots are cleared again.  All clients' entries of the tile
// are loaded in one batch (a wave prefix over the clients' counts) before the ordered fold; tiles holding more than
// 128 entries over all clients take a per-client loop.  Sparse variant (a fold from +0 with finite weights, the
// aggregation round's case): the accumulator lives in the LDS tile and only the kept entries are fma'd, in client
// order.  fmaf(w, +0, acc) == acc for every element no entry touches, with one exception: an accumulator that is -0
// (a negative fma result below half the smallest subnormal rounds to -0, fmaf(w, v, -0) keeps it when w * v is a
// zero of either sign, and a chained launch carries it in) becomes +0 at the next client whose w has a clear sign bit (w * +0 = +0, and
// +0 + -0 = +0).  So the sparse fold records, per element, the last client that wrote it (a byte in LDS) and, before
// each entry's fma and at the end, replays the skipped clients on a -0 (skip_clients) — the dense chain bit for bit.  Bytes: 4n written (+ 4n read when
// accumulating) + the wires' 5 B per kept entry and tile pointers.
//
// The same kernel with a model as its accumulator (an IO policy): flc_fedopt_fold_records (ModelIO: δ, then the server
// optimiser's step) and flc_avg_and_gradient_records (PairIO: a variance-reduced round's gradients from records, the
// dense parameters folded in the same pass) and flc_fold_record_groups (GroupIO: the launch's records fall into
// groups, each folded in place into its own model — SCAFFOLD's two vectors, IFCA's clusters).
//
// Sparse records (flc_sparse_wire_layout): the plain sparsifiers' wire (top-k and rand-k, compressors.py:284-296) —
// idx, the decoded fp32 values and the tile pointers — as the message's record.  Their fold is the stacked kernel with
// another entry codec (StackedEntry: u8 code + the record's norm; SparseEntry: the fp32 value, no norm): the wave-per-
// tile shape, the single load batch, the per-client loop, the tile-pointer clamps and the -0 rule are shared code.
// flc_fold_sparse_wires (FlatIO), flc_fedopt_fold_sparse_records (ModelIO), flc_fold_sparse_record_groups (GroupIO)
// and flc_avg_and_gradient_sparse_records (PairIO) share the stacked entry points' host code.
//
// Dense records (flc_dense_wire_layout): the dithering quantizers' and the natural compressor's wire — one fp32 norm
// and the packed 2-, 4- or 8-bit codes, or one uint16 per element — as the message's record.  Their fold
// (dense_fold_records_kernel, below the stacked one) shares the IO policies: one wave per tile, the accumulator in
// registers as IO::load lays it out, every record's code words of the tile loaded before the ordered fma chain, each
// code decoded as flc_quant_decode / flc_natural_decode decode it.  flc_fold_dense_wires (FlatIO),
// flc_fedopt_fold_dense_records (ModelIO) and flc_fold_dense_record_groups (GroupIO) are the stacked entry points'
// counterparts, and flc_avg_and_gradient_dense_records (PairIO) is flc_avg_and_gradient_records': a variance-reduced
// round's dense gradient records folded into the gradients, the dense parameters into the model in the same pass.
//
// Mixed rounds (flc_record_kind): every record carries its own descriptor — kind, k, format, levels, bits — or is the
// decoded fp32 vector itself, and mixed_fold_records_kernel (below the entry-fold launcher) folds them in message order
// in one pass with the same IO policies: flc_fedopt_fold_mixed_records (ModelIO), flc_fold_mixed_record_groups
// (GroupIO) and flc_avg_and_gradient_mixed_records (PairIO), through the uniform entry points' host code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>
#include <vector>

#include "flc_device.hpp"
#include "flc_runtime.hpp"

namespace flc {
namespace {

constexpr int kMaxWires = 64;  // clients per launch (more: chained launches, accumulating)

struct WireLayout {
  long long norm, idx, codes, tiles;
};
struct FoldArgs {
  const uint8_t* rec[kMaxWires];  // the c-th client's record in fold order
  float w[kMaxWires];
};

WireLayout wire_layout(int64_t n, int64_t k, size_t* total) {
  WireLayout L;
  L.norm = 0;
  L.idx = 16;
  L.codes = (long long)align_up((size_t)(16 + 4 * k), 16);
  L.tiles = (long long)align_up((size_t)L.codes + (size_t)std::max<int64_t>(k, 16), 16);
  const int64_t ntiles = cdiv(n < 1 ? 1 : n, (int64_t)FLC_TILE);
  *total = align_up((size_t)L.tiles + 4 * (size_t)(ntiles + 1), 256);
  return L;
}

__device__ __forceinline__ unsigned long long lowmask(unsigned j) { return j >= 64u ? ~0ull : ((1ull << j) - 1ull); }

// the dense chain's clients [from, to) with no entry at an element, applied to its accumulator: fmaf(w, +0, a) only
// ever changes a -0, to +0, and only for a w with a clear sign bit (`pos`: one bit per such client of the launch)
__device__ __forceinline__ float skip_clients(float a, unsigned from, unsigned to, unsigned long long pos) {
  return (__float_as_uint(a) == 0x80000000u && (pos & lowmask(to) & ~lowmask(from)) != 0ull) ? 0.0f : a;
}

// Where a tile's accumulator comes from and where it goes.  Lane `lane` owns float4 groups q = lane + 64 u (u < 4)
// of the tile starting at flat element t0.
struct FlatIO {  // one flat vector: out = fold (from +0, or from out itself)
  static constexpr bool kGrouped = false;
  static constexpr bool kSparseForm = true;  // (the host may choose the kernel's sparse form for this accumulator)
  float* out;
  int64_t n;
  int acc_in;
  __device__ __forceinline__ void load(int64_t t0, int lane, float4 acc[4]) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (acc_in) {
        if (e + 4 <= n) {
          v = *reinterpret_cast<const float4*>(out + e);
        } else {
          if (e < n) v.x = out[e];
          if (e + 1 < n) v.y = out[e + 1];
          if (e + 2 < n) v.z = out[e + 2];
        }
      }
      acc[u] = v;
    }
  }
  __device__ __forceinline__ void store(int64_t t0, int lane, const float4 acc[4]) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
      if (e + 4 <= n) {
        *reinterpret_cast<float4*>(out + e) = acc[u];
      } else {
        if (e < n) out[e] = acc[u].x;
        if (e + 1 < n) out[e + 1] = acc[u].y;
        if (e + 2 < n) out[e + 2] = acc[u].z;
      }
    }
  }
};

__device__ __forceinline__ float& comp(float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// A server's model as the fold's accumulator (flc_fedopt_fold_records): the flat element e of the records is
// element e - start[t] of tensor t (the concatenation order of the client's flattened delta).  load: a = δ (· β0
// when `scale`: FedOptServer.update's mul_(betas[0]) first); store: δ = a, then, with OPT >= 0, the server
// optimiser's step on θ (and v) from a — _fedopt.py:202-237 in one pass.  The tile's tensors are walked with a
// uniform index (a tile usually lies inside one tensor); a float4 group inside one 16-B aligned tensor moves as one.
constexpr int kRoundT = 16;  // tensors per launch (kernel-argument budget)
struct ModelTab {
  float* delta[kRoundT];
  float* theta[kRoundT];
  float* v[kRoundT];
  int64_t start[kRoundT + 1];  // flat offsets; start[nt] = end of the launch's range
  int nt;
  unsigned vec;  // bit t: tensor t's operands 16-B aligned and start[t] % 4 == 0
  int scale;
  float beta0, lr, beta2, omb, nomb, tau;
};
template <int OPT>  // OPT < 0: the fold only (δ written, no step)
struct ModelIO {
  static constexpr bool kGrouped = false;
  static constexpr bool kSparseForm = false;  // (its launches take every element through every record's fma)
  ModelTab m;
  __device__ __forceinline__ int first_tensor(int64_t t0) const {
    int t = 0;
#if FLC_PACK_SEARCH_STATIC  // (static offsets: the scalar loads of start issue together, flc_device.hpp pack_entry)
#pragma unroll
    for (int i = 1; i < kRoundT; ++i) t += (i < m.nt && m.start[i] <= t0) ? 1 : 0;
#else
    while (t + 1 < m.nt && m.start[t + 1] <= t0) ++t;
#endif
    return t;
  }
  __device__ __forceinline__ void load(int64_t t0, int lane, float4 acc[4]) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = first_tensor(t0); t < m.nt && m.start[t] < t0 + FLC_TILE; ++t) {
      const int64_t s0 = m.start[t], s1 = m.start[t + 1];
      const float* __restrict__ d = m.delta[t];
      const bool vec = (m.vec >> t) & 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
        if (vec && e >= s0 && e + 4 <= s1) {
          float4 x = *reinterpret_cast<const float4*>(d + (e - s0));
          if (m.scale) x = make_float4(x.x * m.beta0, x.y * m.beta0, x.z * m.beta0, x.w * m.beta0);
          acc[u] = x;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j >= s0 && e + j < s1) {
              const float x = d[e + j - s0];
              comp(acc[u], j) = m.scale ? x * m.beta0 : x;
            }
        }
      }
    }
  }
  __device__ __forceinline__ void store(int64_t t0, int lane, float4 acc[4]) const {
    for (int t = first_tensor(t0); t < m.nt && m.start[t] < t0 + FLC_TILE; ++t) {
      const int64_t s0 = m.start[t], s1 = m.start[t + 1];
      float* __restrict__ d = m.delta[t];
      float* __restrict__ th = m.theta[t];
      float* __restrict__ vv = m.v[t];
      const bool vec = (m.vec >> t) & 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
        if (vec && e >= s0 && e + 4 <= s1) {
          const int64_t o = e - s0;
          *reinterpret_cast<float4*>(d + o) = acc[u];
          if (OPT >= 0) {
            float4 tv = *reinterpret_cast<const float4*>(th + o);
            float4 vq = OPT > 0 ? *reinterpret_cast<const float4*>(vv + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            opt_step<OPT < 0 ? 0 : OPT>(tv.x, acc[u].x, &vq.x, m.lr, m.beta2, m.omb, m.nomb, m.tau);
            opt_step<OPT < 0 ? 0 : OPT>(tv.y, acc[u].y, &vq.y, m.lr, m.beta2, m.omb, m.nomb, m.tau);
            opt_step<OPT < 0 ? 0 : OPT>(tv.z, acc[u].z, &vq.z, m.lr, m.beta2, m.omb, m.nomb, m.tau);
            opt_step<OPT < 0 ? 0 : OPT>(tv.w, acc[u].w, &vq.w, m.lr, m.beta2, m.omb, m.nomb, m.tau);
            *reinterpret_cast<float4*>(th + o) = tv;
            if (OPT > 0) *reinterpret_cast<float4*>(vv + o) = vq;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (e + j >= s0 && e + j < s1) {
              const int64_t o = e + j - s0;
              const float a = comp(acc[u], j);
              d[o] = a;
              if (OPT >= 0) {
                float vi = OPT > 0 ? vv[o] : 0.f;
                opt_step<OPT < 0 ? 0 : OPT>(th[o], a, &vi, m.lr, m.beta2, m.omb, m.nomb, m.tau);
                if (OPT > 0) vv[o] = vi;
              }
            }
          }
        }
      }
    }
  }
};

// A variance-reduced server's round as the fold's accumulator (flc_avg_and_gradient_records): the records are the
// messages' compressed gradients, folded into the server's gradient tensors (load: +0, or the stored partial sum of
// a chained launch; store: the gradient), and in the same pass the tile's slice of the messages' dense parameters is
// folded into the server's parameters (avg_parameters, nodes.py:1134-1163: θ = θ·inertia first, then
// fmaf(w_m, p_m, θ) in message order) — pair_fold_kernel's two chains with the gradient's sources read from records.
// The tensor walk is ModelIO's.
constexpr int kPairSrc = 16;  // dense parameter sources per launch (kernel-argument budget)
struct PairTab {
  float* grad[kRoundT];
  float* param[kRoundT];
  const float* src[kPairSrc][kRoundT];
  int64_t start[kRoundT + 1];
  float w[kPairSrc];
  int nt, ns;
  unsigned gvec;  // bit t: the gradient tensor 16-B aligned and start[t] % 4 == 0
  unsigned pvec;  // bit t: the parameter and every source of it 16-B aligned and start[t] % 4 == 0
  int g_on;       // this launch folds records (else the gradients are neither read nor written)
  int g_acc;      // the gradient chain continues from the stored partial sums
  int p_on;       // this launch folds parameter sources
  int p_scale;    // θ·inertia first (the first parameter launch)
  float inertia;
};
struct PairIO {
  static constexpr bool kGrouped = false;
  static constexpr bool kSparseForm = true;
  PairTab m;
  __device__ __forceinline__ int first_tensor(int64_t t0) const {
    int t = 0;
    while (t + 1 < m.nt && m.start[t + 1] <= t0) ++t;
    return t;
  }
  __device__ __forceinline__ void load(int64_t t0, int lane, float4 acc[4]) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(m.g_on && m.g_acc)) return;
    for (int t = first_tensor(t0); t < m.nt && m.start[t] < t0 + FLC_TILE; ++t) {
      const int64_t s0 = m.start[t], s1 = m.start[t + 1];
      const float* __restrict__ d = m.grad[t];
      const bool vec = (m.gvec >> t) & 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
        if (vec && e >= s0 && e + 4 <= s1) {
          acc[u] = *reinterpret_cast<const float4*>(d + (e - s0));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j >= s0 && e + j < s1) comp(acc[u], j) = d[e + j - s0];
        }
      }
    }
  }
  __device__ __forceinline__ void store(int64_t t0, int lane, float4 acc[4]) const {
    for (int t = first_tensor(t0); t < m.nt && m.start[t] < t0 + FLC_TILE; ++t) {
      const int64_t s0 = m.start[t], s1 = m.start[t + 1];
      float* __restrict__ d = m.grad[t];
      float* __restrict__ th = m.param[t];
      const bool gv = (m.gvec >> t) & 1u, pv = (m.pvec >> t) & 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
        const bool whole = e >= s0 && e + 4 <= s1;
        if (m.g_on) {
          if (gv && whole) {
            *reinterpret_cast<float4*>(d + (e - s0)) = acc[u];
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (e + j >= s0 && e + j < s1) d[e + j - s0] = comp(acc[u], j);
          }
        }
        if (!m.p_on) continue;
        if (pv && whole) {
          const int64_t o = e - s0;
          float4 sv[kPairSrc];
#pragma unroll
          for (int s = 0; s < kPairSrc; ++s)
            if (s < m.ns) sv[s] = *reinterpret_cast<const float4*>(m.src[s][t] + o);
          float4 a = *reinterpret_cast<const float4*>(th + o);
          if (m.p_scale) a = make_float4(a.x * m.inertia, a.y * m.inertia, a.z * m.inertia, a.w * m.inertia);
#pragma unroll
          for (int s = 0; s < kPairSrc; ++s) {
            if (s < m.ns) {
              const float ws = m.w[s];
              a = make_float4(fmaf(ws, sv[s].x, a.x), fmaf(ws, sv[s].y, a.y), fmaf(ws, sv[s].z, a.z),
                              fmaf(ws, sv[s].w, a.w));
            }
          }
          *reinterpret_cast<float4*>(th + o) = a;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (e + j >= s0 && e + j < s1) {
              const int64_t o = e + j - s0;
              float a = m.p_scale ? th[o] * m.inertia : th[o];
              for (int s = 0; s < m.ns; ++s) a = fmaf(m.w[s], m.src[s][t][o], a);
              th[o] = a;
            }
          }
        }
      }
    }
  }
};

// A round whose records fall into groups, each accumulating in place into its own model (flc_fold_record_groups):
// SCAFFOLD's two vectors (θ and c, _scaffold.py:160-169), IFCA's cluster centres (_ifca.py:186-195).  blockIdx.y
// is the launch's group: its records are the [first, first + count) slice of FoldArgs (the host orders a launch's
// records by group), its accumulator the group's own tensors (load: the stored values — add_parameters' in-place
// accumulation, nothing scaled or zeroed; store: the fold).  The tensor walk is ModelIO's.
constexpr int kMaxGroups = 16;  // groups per launch (kernel-argument budget: 2 KB of destination pointers)
struct GroupTab {
  float* dst[kMaxGroups][kRoundT];
  int64_t start[kRoundT + 1];
  unsigned vec[kMaxGroups];  // bit t: the group's tensor t 16-B aligned and start[t] % 4 == 0
  int first[kMaxGroups], count[kMaxGroups];
  int nt;
};
struct GroupIO {
  static constexpr bool kGrouped = true;
  static constexpr bool kSparseForm = true;
  GroupTab m;
  __device__ __forceinline__ int first() const { return m.first[blockIdx.y]; }
  __device__ __forceinline__ int count() const { return m.count[blockIdx.y]; }
  __device__ __forceinline__ int first_tensor(int64_t t0) const {
    int t = 0;
    while (t + 1 < m.nt && m.start[t + 1] <= t0) ++t;
    return t;
  }
  __device__ __forceinline__ void load(int64_t t0, int lane, float4 acc[4]) const {
    const int g = blockIdx.y;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = first_tensor(t0); t < m.nt && m.start[t] < t0 + FLC_TILE; ++t) {
      const int64_t s0 = m.start[t], s1 = m.start[t + 1];
      const float* __restrict__ d = m.dst[g][t];
      const bool vec = (m.vec[g] >> t) & 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
        if (vec && e >= s0 && e + 4 <= s1) {
          acc[u] = *reinterpret_cast<const float4*>(d + (e - s0));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j >= s0 && e + j < s1) comp(acc[u], j) = d[e + j - s0];
        }
      }
    }
  }
  __device__ __forceinline__ void store(int64_t t0, int lane, float4 acc[4]) const {
    const int g = blockIdx.y;
    for (int t = first_tensor(t0); t < m.nt && m.start[t] < t0 + FLC_TILE; ++t) {
      const int64_t s0 = m.start[t], s1 = m.start[t + 1];
      float* __restrict__ d = m.dst[g][t];
      const bool vec = (m.vec[g] >> t) & 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
        if (vec && e >= s0 && e + 4 <= s1) {
          *reinterpret_cast<float4*>(d + (e - s0)) = acc[u];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j >= s0 && e + j < s1) d[e + j - s0] = comp(acc[u], j);
        }
      }
    }
  }
};

// What a kept entry's wire word is and what it decodes to (the fold kernel's entry codec).  Both records keep an
// ascending int32 idx field and the CSR tile pointers; they differ in the word that travels with each index.
struct StackedEntry {  // the stacked record: a u8 code at L.codes + j, dequantised with the record's norm
  static __device__ __forceinline__ float norm(const uint8_t* rec, const WireLayout& L) {
    return *reinterpret_cast<const float*>(rec + L.norm);
  }
  static __device__ __forceinline__ unsigned raw(const uint8_t* rc, const WireLayout& L, unsigned j) {
    return rc[L.codes + j];
  }
  static __device__ __forceinline__ float value(unsigned raw, int levels, double step, float nrm) {
    return stacked_dequant(raw, levels, step, nrm);  // compressors.py:357
  }
};
// The sparse record (flc_sparse_wire_layout: the top-k / rand-k wire of compressors.py:284-296): the decoded fp32
// value itself at L.codes + 4 j (the layout's val field travels in WireLayout::codes), no norm — sparse.hip's
// entry_value<0> at scale 1.
struct SparseEntry {
  static __device__ __forceinline__ float norm(const uint8_t*, const WireLayout&) { return 0.0f; }
  static __device__ __forceinline__ unsigned raw(const uint8_t* rc, const WireLayout& L, unsigned j) {
    return reinterpret_cast<const unsigned*>(rc + L.codes)[j];
  }
  static __device__ __forceinline__ float value(unsigned raw, int, double, float) { return __uint_as_float(raw); }
};

template <bool SPARSE, class IO, class EC = StackedEntry>
__global__ __launch_bounds__(kWave) void stacked_fold_wires_kernel(FoldArgs a, WireLayout L, int nw_all, int levels,
                                                                   double step, int64_t tile0, IO io, unsigned k) {
  __shared__ __attribute__((aligned(16))) float s_tile[FLC_TILE];
  __shared__ __attribute__((aligned(16))) uint8_t s_last[SPARSE ? FLC_TILE : 4];  // sparse: last writer + 1 (0: none)
  float4* tile4 = reinterpret_cast<float4*>(s_tile);
  const int lane = threadIdx.x;
  // the block's records: the whole launch's, or (a grouped launch) its group's slice of them
  int nw = nw_all, rec0 = 0;
  if constexpr (IO::kGrouped) {
    nw = io.count();
    rec0 = io.first();
  }
  const int64_t t = tile0 + blockIdx.x;
  const int64_t t0 = t * FLC_TILE;
  // the tile's slice of the accumulator: lane owns float4 q = lane + 64 u
  float4 acc[4];
  io.load(t0, lane, acc);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    // dense: a zero tile per client; sparse: the accumulator itself lives in the LDS tile
    tile4[lane + u * kWave] = SPARSE ? acc[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (SPARSE) reinterpret_cast<unsigned*>(s_last)[lane + u * kWave] = 0u;
  }
  // client `lane`'s record, entry range in this tile and norm (lanes >= nw: empty)
  const uint8_t* rec = nullptr;
  unsigned lo = 0, cnt = 0;
  float nrm = 0.0f, wl = 0.0f;
  if (lane < nw) {
    rec = a.rec[rec0 + lane];
    wl = a.w[rec0 + lane];
    const unsigned* tiles = reinterpret_cast<const unsigned*>(rec + L.tiles);
    // (clamped to the record's k entries: a malformed or unwritten tile pointer never reads past the record)
    lo = min(tiles[t], k);
    const unsigned hi = min(tiles[t + 1], k);
    cnt = hi > lo ? hi - lo : 0u;
    nrm = EC::norm(rec, L);
  }
  const unsigned long long pos = __ballot(lane < nw && !std::signbit(wl));  // sign-clear weights (sparse: -0 rule)
  const unsigned incl = wave_incl_scan(cnt);
  const unsigned excl = incl - cnt;
  const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, kWave - 1);

  if (total <= 2u * kWave) {
    // fast path: every entry of the tile over all clients in registers (g = lane, lane + 64), one load batch
    int cg[2] = {-1, -1};
    unsigned off[2] = {0u, 0u};
    float val[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned g = (unsigned)lane + (unsigned)(r * kWave);
      int c = -1;
      for (int cc = 0; cc < nw; ++cc) {  // (uniform loop; the client whose range holds g)
        const unsigned ec = (unsigned)__builtin_amdgcn_readlane((int)excl, cc);
        const unsigned nc = (unsigned)__builtin_amdgcn_readlane((int)cnt, cc);
        if (g >= ec && g < ec + nc) c = cc;
      }
      cg[r] = g < total ? c : -1;
    }
    // the owning client's record / range / norm by lane shuffles, then the loads (one batch)
    unsigned idx_raw[2] = {0u, 0u}, code[2] = {0u, 0u};
    float nr[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int src = cg[r] < 0 ? 0 : cg[r];
      const unsigned lo_c = (unsigned)__shfl((int)lo, src, kWave);
      const unsigned ex_c = (unsigned)__shfl((int)excl, src, kWave);
      const unsigned long long rp = (unsigned long long)(uintptr_t)rec;
      const unsigned rlo = (unsigned)__shfl((int)(unsigned)rp, src, kWave);
      const unsigned rhi = (unsigned)__shfl((int)(unsigned)(rp >> 32), src, kWave);
      nr[r] = __shfl(nrm, src, kWave);
      if (cg[r] >= 0) {
        const uint8_t* rc = reinterpret_cast<const uint8_t*>((uintptr_t)(((unsigned long long)rhi << 32) | rlo));
        const unsigned j = lo_c + ((unsigned)lane + (unsigned)(r * kWave) - ex_c);
        idx_raw[r] = reinterpret_cast<const unsigned*>(rc + L.idx)[j];
        code[r] = EC::raw(rc, L, j);
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t o = (int64_t)idx_raw[r] - t0;
      if (cg[r] >= 0 && (o < 0 || o >= FLC_TILE)) cg[r] = -1;  // (a malformed wire: ignored, never out of the tile)
      off[r] = (unsigned)(o < 0 ? 0 : (o >= FLC_TILE ? 0 : o));
      val[r] = EC::value(code[r], levels, step, nr[r]);
    }
    if (SPARSE) {
      // the accumulator in LDS, updated at the kept entries only (see the launch: +0 start, finite weights, so
      // fmaf(w, +0, acc) == acc for every element no entry touches)
      for (int c = 0; c < nw; ++c) {
        const float wc = __shfl(wl, c, kWave);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (cg[r] == c) {
            s_tile[off[r]] = fmaf(wc, val[r], skip_clients(s_tile[off[r]], s_last[off[r]], (unsigned)c, pos));
            s_last[off[r]] = (uint8_t)(c + 1);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = tile4[lane + u * kWave];
    }
    for (int c = 0; c < (SPARSE ? 0 : nw); ++c) {  // the ordered fold
      const float wc = __shfl(wl, c, kWave);
      const bool any = __builtin_amdgcn_readlane((int)cnt, c) != 0;
      if (any) {
        if (cg[0] == c) s_tile[off[0]] = val[0];
        if (cg[1] == c) s_tile[off[1]] = val[1];
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 v = tile4[lane + u * kWave];
          acc[u] = make_float4(fmaf(wc, v.x, acc[u].x), fmaf(wc, v.y, acc[u].y), fmaf(wc, v.z, acc[u].z),
                               fmaf(wc, v.w, acc[u].w));
        }
        __builtin_amdgcn_wave_barrier();
        if (cg[0] == c) s_tile[off[0]] = 0.0f;
        if (cg[1] == c) s_tile[off[1]] = 0.0f;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[u] = make_float4(fmaf(wc, 0.0f, acc[u].x), fmaf(wc, 0.0f, acc[u].y), fmaf(wc, 0.0f, acc[u].z),
                               fmaf(wc, 0.0f, acc[u].w));
      }
    }
  } else {
    // dense tiles (skewed inputs): per client, its entries in rounds of 64, scattered, folded, cleared
    for (int c = 0; c < nw; ++c) {
      const float wc = __shfl(wl, c, kWave);
      const unsigned lo_c = (unsigned)__builtin_amdgcn_readlane((int)lo, c);
      const unsigned n_c = (unsigned)__builtin_amdgcn_readlane((int)cnt, c);
      const float nr_c = __shfl(nrm, c, kWave);
      const unsigned long long rp = (unsigned long long)(uintptr_t)rec;
      const unsigned rlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)rp, c);
      const unsigned rhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(rp >> 32), c);
      const uint8_t* rc = reinterpret_cast<const uint8_t*>((uintptr_t)(((unsigned long long)rhi << 32) | rlo));
      const unsigned* ix = reinterpret_cast<const unsigned*>(rc + L.idx);
      if (SPARSE) {
        for (unsigned j = lo_c + lane; j < lo_c + n_c; j += kWave) {
          const int64_t o = (int64_t)ix[j] - t0;
          if (o >= 0 && o < FLC_TILE) {
            s_tile[o] = fmaf(wc, EC::value(EC::raw(rc, L, j), levels, step, nr_c),
                             skip_clients(s_tile[o], s_last[o], (unsigned)c, pos));
            s_last[o] = (uint8_t)(c + 1);
          }
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        continue;
      }
      for (unsigned j = lo_c + lane; j < lo_c + n_c; j += kWave) {
        const int64_t o = (int64_t)ix[j] - t0;
        if (o >= 0 && o < FLC_TILE) s_tile[o] = EC::value(EC::raw(rc, L, j), levels, step, nr_c);
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 v = tile4[lane + u * kWave];
        acc[u] = make_float4(fmaf(wc, v.x, acc[u].x), fmaf(wc, v.y, acc[u].y), fmaf(wc, v.z, acc[u].z),
                             fmaf(wc, v.w, acc[u].w));
      }
      __builtin_amdgcn_wave_barrier();
      for (unsigned j = lo_c + lane; j < lo_c + n_c; j += kWave) {
        const int64_t o = (int64_t)ix[j] - t0;
        if (o >= 0 && o < FLC_TILE) s_tile[o] = 0.0f;
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (SPARSE) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = tile4[lane + u * kWave];
    }
  }
  if (SPARSE) {  // the clients after each element's last writer
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned lb = reinterpret_cast<const unsigned*>(s_last)[lane + u * kWave];
      acc[u].x = skip_clients(acc[u].x, lb & 0xFFu, 64u, pos);
      acc[u].y = skip_clients(acc[u].y, (lb >> 8) & 0xFFu, 64u, pos);
      acc[u].z = skip_clients(acc[u].z, (lb >> 16) & 0xFFu, 64u, pos);
      acc[u].w = skip_clients(acc[u].w, lb >> 24, 64u, pos);
    }
  }
  io.store(t0, lane, acc);
}

// ---------------------------------------------------------------------------------------------------------------
// Dense records: the dithering quantizers' and the natural compressor's wire as one record per client
//   [0, 4)             norm   fp32 (unused by the natural compressor)
//   [16, 16 + bytes)   codes  `bits` bits per element (2, 4 or 8: sign << (bits-1) | level, element i at bit i * bits),
//                             or one uint16 per element (the natural compressor); bytes = ceil(n * bits / 8)
// padded to 256 B.  The fold reads every client's codes of a tile — four elements per lane and float4 group, the
// accumulator's own layout, so 1/4 .. 1/16 of the dense vector's bytes — and applies the ordered chain
// a = fmaf(w_c, v_c, a) with v_c the decoders' value of the code (dequant<KIND, BITS> in quant.hip, natural_value).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kFmtNatural = 2;  // FLC_WIRE_NATURAL (0 / 1: FLC_Q_STANDARD_DITHER / FLC_Q_NATURAL_DITHER)
constexpr long long kDenseNorm = 0, kDenseCodes = 16;

struct DenseCodec {
  int format, levels, bits;
  int64_t n;
  int logb = 0;  // bucket records (flc_bucket_wire_layout): log2 of the bucket size; 0: one norm for the record
};

// Bucket records: [0, 4 nb) the nb = ceil(n / B) fp32 norms, then the same code stream from the next 16-B boundary.
// The fold reads the norm of (record, e >> log2 B) per quad run of a lane: for B >= 256 the 64 lanes of a run (256
// consecutive elements) read one address, below that a lane's own bucket's.
long long bucket_codes_offset(int64_t n, int logb) {
  return (long long)align_up((size_t)cdiv(n, (int64_t)1 << logb) * sizeof(float), 16);
}

size_t dense_wire_size(int64_t n, int format, int bits) {
  const size_t code_bytes = format == kFmtNatural ? 2 * (size_t)n : ((size_t)n * (size_t)bits + 7) / 8;
  return align_up((size_t)kDenseCodes + code_bytes, 256);
}

// the codes of four consecutive elements (e % 4 == 0): one aligned word of the code stream.  The word of the last
// group of a record may reach into the record's padding (the record ends on a 256-B boundary): those elements lie at
// or beyond n and are never stored.
template <int BITS>
struct Quad {
  typedef uint32_t type;
};
template <>
struct Quad<16> {
  typedef uint2 type;
};
template <int BITS>
__device__ __forceinline__ typename Quad<BITS>::type load_quad(const uint8_t* __restrict__ codes, int64_t e) {
  const uint8_t* p = codes + ((e * BITS) >> 3);
  if constexpr (BITS == 16) return *reinterpret_cast<const uint2*>(p);
  else if constexpr (BITS == 8) return *reinterpret_cast<const uint32_t*>(p);
  else if constexpr (BITS == 4) return (uint32_t)*reinterpret_cast<const uint16_t*>(p);
  else return (uint32_t)*p;
}
template <int BITS>
__device__ __forceinline__ uint32_t quad_code(const typename Quad<BITS>::type& q, int j) {
  if constexpr (BITS == 16) return ((j < 2 ? q.x : q.y) >> (16 * (j & 1))) & 0xffffu;
  else return (q >> (j * BITS)) & ((1u << BITS) - 1u);
}

// KIND 0 / 1: standard / natural dithering with BITS-bit codes; KIND 2: the natural compressor's uint16 codes.
// One wave per FLC_TILE tile; the launch's records in batches of kBatch: the batch's code words are all issued (four
// loads per record and lane), then the ordered chain runs over them — a round of up to kBatch clients is one batch.
// fp32(level value) comes from an LDS table of all 2^(BITS-1) level fields (dequant's (float)level_value, as
// quant_fused_kernel's s_lvt), so a code decodes exactly as flc_quant_decode decodes it, whatever its level field.
// BKT: bucket records — the norm of element e is norms[e >> logb], the codes start at codes_off.
template <int KIND, int BITS, class IO, bool BKT = false>
__global__ __launch_bounds__(kWave) void dense_fold_records_kernel(FoldArgs a, int nw_all, int s, double step,
                                                                   int64_t n, int64_t tile0, IO io, int logb = 0,
                                                                   long long codes_off = kDenseCodes) {
  typedef typename Quad<BITS>::type Q;
  constexpr int kLv = KIND == kFmtNatural ? 1 : (1 << (BITS - 1));
  constexpr int kBatch = BITS == 16 ? 8 : 16;
  __shared__ float s_lvt[kLv];
  const int lane = threadIdx.x;
  if constexpr (KIND != kFmtNatural) {
    for (int i = lane; i < kLv; i += kWave) s_lvt[i] = (float)level_value<KIND>(i, s, step);
    __syncthreads();
  }
  int nw = nw_all, rec0 = 0;
  if constexpr (IO::kGrouped) {
    nw = io.count();
    rec0 = io.first();
  }
  const int64_t t0 = (tile0 + blockIdx.x) * FLC_TILE;
  float4 acc[4];
  io.load(t0, lane, acc);
  for (int c0 = 0; c0 < nw; c0 += kBatch) {
    Q cw[kBatch][4];
    float nr[kBatch][BKT ? 4 : 1];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
#pragma unroll
      for (int u = 0; u < (BKT ? 4 : 1); ++u) nr[i][u] = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u) cw[i][u] = Q{};
      if (c0 + i < nw) {
        const uint8_t* __restrict__ rc = a.rec[rec0 + c0 + i];
        if constexpr (KIND != kFmtNatural && !BKT) nr[i][0] = *reinterpret_cast<const float*>(rc + kDenseNorm);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
          if constexpr (BKT) {
            if (e < n) {
              nr[i][u] = reinterpret_cast<const float*>(rc)[e >> logb];
              cw[i][u] = load_quad<BITS>(rc + codes_off, e);
            }
          } else {
            if (e < n) cw[i][u] = load_quad<BITS>(rc + kDenseCodes, e);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (c0 + i >= nw) continue;  // (uniform)
      const float wc = a.w[rec0 + c0 + i];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float nrm = nr[i][BKT ? u : 0];
        const bool regular = norm_regular(nrm);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t code = quad_code<BITS>(cw[i][u], j);
          if constexpr (KIND == kFmtNatural) {
            v[j] = natural_value(code);
          } else if (!regular) {
            v[j] = code == 0u ? 0.0f : __uint_as_float(0x7fc00000u);
          } else {
            const float lv = s_lvt[code & ((1u << (BITS - 1)) - 1u)];
            const float sv = (code >> (BITS - 1)) ? -lv : lv;  // fp32(lv) * sign, -0 kept
            v[j] = sv * nrm;                                   // compressors.py:357 (rounded before the fma)
          }
        }
        acc[u] = make_float4(fmaf(wc, v[0], acc[u].x), fmaf(wc, v[1], acc[u].y), fmaf(wc, v[2], acc[u].z),
                             fmaf(wc, v[3], acc[u].w));
      }
    }
  }
  io.store(t0, lane, acc);
}

template <class IO>
int launch_dense_fold(const char* name, const DenseCodec& cd, dim3 grid, hipStream_t st, const FoldArgs& a, int nw,
                      int64_t tile0, const IO& io) {
  const double step = 1.0 / (double)(cd.levels < 1 ? 1 : cd.levels);
#define FLC_DF(K, B)                                                                                              \
  do {                                                                                                            \
    FLC_LAUNCH(name, (dense_fold_records_kernel<K, B, IO>), grid, dim3(kWave), 0, st, a, nw, cd.levels, step, cd.n, \
               tile0, io, 0, kDenseCodes);                                                                        \
    return FLC_OK;                                                                                                \
  } while (0)
  if (cd.logb) {  // bucket records (the dithering quantizers only)
    const long long coff = bucket_codes_offset(cd.n, cd.logb);
#define FLC_BF(K, B)                                                                                                \
  do {                                                                                                              \
    FLC_LAUNCH(name, (dense_fold_records_kernel<K, B, IO, true>), grid, dim3(kWave), 0, st, a, nw, cd.levels, step, \
               cd.n, tile0, io, cd.logb, coff);                                                                     \
    return FLC_OK;                                                                                                  \
  } while (0)
    if (cd.format == FLC_Q_STANDARD_DITHER) {
      if (cd.bits == 8) FLC_BF(0, 8);
      if (cd.bits == 4) FLC_BF(0, 4);
      FLC_BF(0, 2);
    }
    if (cd.bits == 8) FLC_BF(1, 8);
    if (cd.bits == 4) FLC_BF(1, 4);
    FLC_BF(1, 2);
#undef FLC_BF
  }
  if (cd.format == kFmtNatural) FLC_DF(2, 16);
  if (cd.format == FLC_Q_STANDARD_DITHER) {
    if (cd.bits == 8) FLC_DF(0, 8);
    if (cd.bits == 4) FLC_DF(0, 4);
    FLC_DF(0, 2);
  }
  if (cd.bits == 8) FLC_DF(1, 8);
  if (cd.bits == 4) FLC_DF(1, 4);
  FLC_DF(1, 2);
#undef FLC_DF
}

// check_quant_args' rule (quant.hip) for a dense record's (format, levels, bits); the natural compressor has 16-bit
// codes and no levels
int check_dense_format(const char* fn, int format, int levels, int bits) {
  if (format == kFmtNatural) {
    if (bits != 16) return fail(FLC_EINVAL, "%s: the natural compressor's codes have 16 bits (got %d)", fn, bits);
    return FLC_OK;
  }
  if (format != FLC_Q_STANDARD_DITHER && format != FLC_Q_NATURAL_DITHER)
    return fail(FLC_EINVAL, "%s: unknown format %d", fn, format);
  if (bits != 2 && bits != 4 && bits != 8) return fail(FLC_EINVAL, "%s: bits must be 2, 4 or 8 (got %d)", fn, bits);
  if (levels < 1 || levels > (1 << (bits - 1)) - 1)
    return fail(FLC_EINVAL, "%s: levels %d does not fit %d-bit codes", fn, levels, bits);
  return FLC_OK;
}

// The sparsifiers' record (flc_sparse_wire_layout): idx int32[k] ascending, val fp32[k] (the decoded values), tiles —
// the stacked record without its norm, its codes widened to the values.  WireLayout::codes is the val field.
WireLayout sparse_wire_layout(int64_t n, int64_t k, size_t* total) {
  WireLayout L;
  L.norm = 0;  // (no norm: SparseEntry reads none)
  L.idx = 0;
  L.codes = (long long)align_up((size_t)(4 * k), 16);
  L.tiles = (long long)align_up((size_t)L.codes + (size_t)(4 * k), 16);
  const int64_t ntiles = cdiv(n < 1 ? 1 : n, (int64_t)FLC_TILE);
  *total = align_up((size_t)L.tiles + 4 * (size_t)(ntiles + 1), 256);
  return L;
}

enum RecordKind { kRecStacked = 0, kRecSparse = 1 };  // the entry records' two codecs (StackedEntry / SparseEntry)

WireLayout record_layout(RecordKind kind, int64_t n, int64_t k, size_t* total) {
  return kind == kRecSparse ? sparse_wire_layout(n, k, total) : wire_layout(n, k, total);
}

// the codec's own argument rule: a stacked record's levels, a sparse record's 1 <= k <= n (the layout's domain)
int check_entry_codec(const char* fn, RecordKind kind, int64_t n, int64_t k, int levels) {
  if (kind == kRecSparse) {
    if (k < 1 || k > n) return fail(FLC_EINVAL, "%s: k %lld outside [1, n = %lld]", fn, (long long)k, (long long)n);
    return FLC_OK;
  }
  if (levels < 1 || levels > 127) return fail(FLC_EINVAL, "%s: levels must be in [1, 127]", fn);
  return FLC_OK;
}

// one launch of the entry-record fold: the kernel by (sparse form, accumulator policy, entry codec)
template <class IO>
int launch_entry_fold(const char* probe, RecordKind kind, bool sparse, dim3 grid, hipStream_t st, const FoldArgs& a,
                      const WireLayout& L, int nw, int levels, double step, int64_t tile0, const IO& io, unsigned k) {
#define FLC_EF(S, EC)                                                                                              \
  do {                                                                                                             \
    FLC_LAUNCH(probe, (stacked_fold_wires_kernel<S, IO, EC>), grid, dim3(kWave), 0, st, a, L, nw, levels, step, tile0, \
               io, k);                                                                                             \
    return FLC_OK;                                                                                                 \
  } while (0)
  if constexpr (IO::kSparseForm) {
    if (sparse && kind == kRecSparse) FLC_EF(true, SparseEntry);
    if (sparse) FLC_EF(true, StackedEntry);
  }
  if (kind == kRecSparse) FLC_EF(false, SparseEntry);
  FLC_EF(false, StackedEntry);
#undef FLC_EF
}

// ---------------------------------------------------------------------------------------------------------------
// Mixed rounds: every record of the launch carries its own descriptor (flc_record_kind, k, format, levels, bits), so a
// round whose clients chose different codecs — or one whose message is the decoded fp32 vector — folds in one pass.
// One wave per tile, the accumulator in registers as IO::load lays it out (the register-accumulator form: every
// record's fma reaches every element, so no -0 replay is needed).  The launch's records are walked in message order as
// RUNS of one class; the class of a run is wave-uniform, so every branch on it is scalar:
//   entry run   stacked and sparse records (any k, any levels): stacked_fold_wires_kernel's dense form with the layout,
//               the entry codec and the levels per lane — one load batch for <= 128 entries over the run's records,
//               else the per-record loop; scattered into the zeroed LDS tile, read back densely, cleared again
//   dense run   dithering records of one code width (any format and levels: the level table is per record) or natural-
//               compressor records: dense_fold_records_kernel's load batch, then the ordered chain
//   flat run    decoded fp32 vectors: the batch's float4 groups loaded, then the ordered chain
// The level tables — one per distinct (format, levels, bits) of the launch, at most kMaxTabs (the host ends a launch
// before a record that would need one more) — are built in LDS once per block; a stacked record's (levels, step) take a
// table entry without LDS values (stacked_dequant evaluates its level in fp64).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMaxTabs = 8;
constexpr int kTabStacked = 3;  // tab_fmt of a stacked record's (levels, step) entry (0 / 1: the dithering formats)
enum MixedClass : uint8_t {
  kClsStacked = 0,
  kClsSparse = 1,
  kClsQ8 = 2,
  kClsQ4 = 3,
  kClsQ2 = 4,
  kClsN16 = 5,
  kClsFlat = 6
};
struct MixedDesc {
  double tab_step[kMaxTabs];  // 1 / levels in fp64, as the uniform entry points pass it
  unsigned k[kMaxWires];      // entries of a stacked or sparse record
  uint8_t cls[kMaxWires];     // MixedClass
  uint8_t tab[kMaxWires];     // the record's table entry (stacked and dithering records)
  uint8_t tab_fmt[kMaxTabs], tab_levels[kMaxTabs], tab_bits[kMaxTabs];
  int ntab;
};

__device__ __forceinline__ int run_class(int cls) { return cls <= kClsSparse ? 0 : cls; }

// wire_layout's / sparse_wire_layout's field offsets from the record's own k
struct EntryOffsets {
  long long idx, codes, tiles;
};
__device__ __forceinline__ EntryOffsets entry_offsets(bool sparse, unsigned k) {
  EntryOffsets o;
  const long long k4 = 4ll * (long long)k;
  if (sparse) {
    o.idx = 0;
    o.codes = (k4 + 15ll) & ~15ll;
    o.tiles = (o.codes + k4 + 15ll) & ~15ll;
  } else {
    o.idx = 16;
    o.codes = (16ll + k4 + 15ll) & ~15ll;
    o.tiles = (o.codes + (long long)(k > 16u ? k : 16u) + 15ll) & ~15ll;
  }
  return o;
}
__device__ __forceinline__ unsigned entry_raw(const uint8_t* rc, bool sparse, const EntryOffsets& o, unsigned j) {
  return sparse ? reinterpret_cast<const unsigned*>(rc + o.codes)[j] : (unsigned)rc[o.codes + j];
}
__device__ __forceinline__ float entry_value(const MixedDesc& d, bool sparse, unsigned slot, unsigned raw, float nrm) {
  if (sparse) return __uint_as_float(raw);
  return stacked_dequant(raw, (int)d.tab_levels[slot], d.tab_step[slot], nrm);  // compressors.py:357
}

// records [r0, r0 + rn) of the launch, all stacked or sparse: lane c holds record r0 + c
__device__ __forceinline__ void mixed_entry_run(const FoldArgs& a, const MixedDesc& d, int r0, int rn, int64_t t,
                                                int64_t t0, int lane, float* s_tile, float4 acc[4]) {
  float4* tile4 = reinterpret_cast<float4*>(s_tile);
  const uint8_t* rec = nullptr;
  unsigned lo = 0, cnt = 0, kk = 0, meta = 0;  // meta: bit 0 sparse, bits 1.. the table entry
  float nrm = 0.0f, wl = 0.0f;
  if (lane < rn) {
    const int r = r0 + lane;
    rec = a.rec[r];
    wl = a.w[r];
    kk = d.k[r];
    const bool sp = d.cls[r] == kClsSparse;
    meta = (sp ? 1u : 0u) | ((unsigned)d.tab[r] << 1);
    const EntryOffsets o = entry_offsets(sp, kk);
    const unsigned* tiles = reinterpret_cast<const unsigned*>(rec + o.tiles);
    // (clamped to the record's own k entries: a malformed or unwritten tile pointer never reads past the record)
    lo = min(tiles[t], kk);
    const unsigned hi = min(tiles[t + 1], kk);
    cnt = hi > lo ? hi - lo : 0u;
    nrm = sp ? 0.0f : *reinterpret_cast<const float*>(rec);
  }
  const unsigned incl = wave_incl_scan(cnt);
  const unsigned excl = incl - cnt;
  const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, kWave - 1);
  const unsigned long long rp = (unsigned long long)(uintptr_t)rec;

  if (total <= 2u * kWave) {
    // every entry of the tile over the run's records in registers (g = lane, lane + 64), one load batch
    int cg[2] = {-1, -1};
    unsigned off[2] = {0u, 0u};
    float val[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned g = (unsigned)lane + (unsigned)(r * kWave);
      int c = -1;
      for (int cc = 0; cc < rn; ++cc) {  // (uniform loop; the record whose range holds g)
        const unsigned ec = (unsigned)__builtin_amdgcn_readlane((int)excl, cc);
        const unsigned nc = (unsigned)__builtin_amdgcn_readlane((int)cnt, cc);
        if (g >= ec && g < ec + nc) c = cc;
      }
      cg[r] = g < total ? c : -1;
    }
    unsigned idx_raw[2] = {0u, 0u}, code[2] = {0u, 0u}, mt[2] = {0u, 0u};
    float nr[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int src = cg[r] < 0 ? 0 : cg[r];
      const unsigned lo_c = (unsigned)__shfl((int)lo, src, kWave);
      const unsigned ex_c = (unsigned)__shfl((int)excl, src, kWave);
      const unsigned k_c = (unsigned)__shfl((int)kk, src, kWave);
      const unsigned rlo = (unsigned)__shfl((int)(unsigned)rp, src, kWave);
      const unsigned rhi = (unsigned)__shfl((int)(unsigned)(rp >> 32), src, kWave);
      mt[r] = (unsigned)__shfl((int)meta, src, kWave);
      nr[r] = __shfl(nrm, src, kWave);
      if (cg[r] >= 0) {
        const uint8_t* rc = reinterpret_cast<const uint8_t*>((uintptr_t)(((unsigned long long)rhi << 32) | rlo));
        const bool sp = mt[r] & 1u;
        const EntryOffsets o = entry_offsets(sp, k_c);
        const unsigned j = lo_c + ((unsigned)lane + (unsigned)(r * kWave) - ex_c);  // (< the record's k: lo, hi clamped)
        idx_raw[r] = reinterpret_cast<const unsigned*>(rc + o.idx)[j];
        code[r] = entry_raw(rc, sp, o, j);
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t o = (int64_t)idx_raw[r] - t0;
      if (cg[r] >= 0 && (o < 0 || o >= FLC_TILE)) cg[r] = -1;  // (a malformed wire: ignored, never out of the tile)
      off[r] = (unsigned)(o < 0 ? 0 : (o >= FLC_TILE ? 0 : o));
      val[r] = entry_value(d, mt[r] & 1u, mt[r] >> 1, code[r], nr[r]);
    }
    for (int c = 0; c < rn; ++c) {  // the ordered fold
      const float wc = __shfl(wl, c, kWave);
      const bool any = __builtin_amdgcn_readlane((int)cnt, c) != 0;
      if (any) {
        if (cg[0] == c) s_tile[off[0]] = val[0];
        if (cg[1] == c) s_tile[off[1]] = val[1];
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 v = tile4[lane + u * kWave];
          acc[u] = make_float4(fmaf(wc, v.x, acc[u].x), fmaf(wc, v.y, acc[u].y), fmaf(wc, v.z, acc[u].z),
                               fmaf(wc, v.w, acc[u].w));
        }
        __builtin_amdgcn_wave_barrier();
        if (cg[0] == c) s_tile[off[0]] = 0.0f;
        if (cg[1] == c) s_tile[off[1]] = 0.0f;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[u] = make_float4(fmaf(wc, 0.0f, acc[u].x), fmaf(wc, 0.0f, acc[u].y), fmaf(wc, 0.0f, acc[u].z),
                               fmaf(wc, 0.0f, acc[u].w));
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  } else {
    // dense tiles: per record, its entries in rounds of 64, scattered, folded, cleared
    for (int c = 0; c < rn; ++c) {
      const float wc = __shfl(wl, c, kWave);
      const unsigned lo_c = (unsigned)__builtin_amdgcn_readlane((int)lo, c);
      const unsigned n_c = (unsigned)__builtin_amdgcn_readlane((int)cnt, c);
      const unsigned k_c = (unsigned)__builtin_amdgcn_readlane((int)kk, c);
      const unsigned mt_c = (unsigned)__builtin_amdgcn_readlane((int)meta, c);
      const float nr_c = __shfl(nrm, c, kWave);
      const unsigned rlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)rp, c);
      const unsigned rhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(rp >> 32), c);
      const uint8_t* rc = reinterpret_cast<const uint8_t*>((uintptr_t)(((unsigned long long)rhi << 32) | rlo));
      const bool sp = mt_c & 1u;
      const EntryOffsets o = entry_offsets(sp, k_c);
      const unsigned* ix = reinterpret_cast<const unsigned*>(rc + o.idx);
      for (unsigned j = lo_c + lane; j < lo_c + n_c; j += kWave) {
        const int64_t e = (int64_t)ix[j] - t0;
        if (e >= 0 && e < FLC_TILE) s_tile[e] = entry_value(d, sp, mt_c >> 1, entry_raw(rc, sp, o, j), nr_c);
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 v = tile4[lane + u * kWave];
        acc[u] = make_float4(fmaf(wc, v.x, acc[u].x), fmaf(wc, v.y, acc[u].y), fmaf(wc, v.z, acc[u].z),
                             fmaf(wc, v.w, acc[u].w));
      }
      __builtin_amdgcn_wave_barrier();
      for (unsigned j = lo_c + lane; j < lo_c + n_c; j += kWave) {
        const int64_t e = (int64_t)ix[j] - t0;
        if (e >= 0 && e < FLC_TILE) s_tile[e] = 0.0f;
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

// records [r0, r0 + rn) of the launch, all dense records of BITS-bit codes (16: the natural compressor's):
// dense_fold_records_kernel's batches, the level table by the record
template <int BITS>
__device__ __forceinline__ void mixed_dense_run(const FoldArgs& a, const MixedDesc& d, int r0, int rn,
                                                const float* s_lvt, int64_t n, int64_t t0, int lane, float4 acc[4]) {
  typedef typename Quad<BITS>::type Q;
  constexpr int kBatch = BITS == 16 ? 8 : 16;
  for (int c0 = 0; c0 < rn; c0 += kBatch) {
    Q cw[kBatch][4];
    float nr[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      nr[i] = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u) cw[i][u] = Q{};
      if (c0 + i < rn) {
        const uint8_t* __restrict__ rc = a.rec[r0 + c0 + i];
        if constexpr (BITS != 16) nr[i] = *reinterpret_cast<const float*>(rc + kDenseNorm);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
          if (e < n) cw[i][u] = load_quad<BITS>(rc + kDenseCodes, e);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (c0 + i >= rn) continue;  // (uniform)
      const float wc = a.w[r0 + c0 + i];
      const float nrm = nr[i];
      const bool regular = norm_regular(nrm);
      const float* lvt = s_lvt + 128 * (int)d.tab[r0 + c0 + i];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t code = quad_code<BITS>(cw[i][u], j);
          if constexpr (BITS == 16) {
            v[j] = natural_value(code);
          } else if (!regular) {
            v[j] = code == 0u ? 0.0f : __uint_as_float(0x7fc00000u);
          } else {
            const float lv = lvt[code & ((1u << (BITS - 1)) - 1u)];
            const float sv = (code >> (BITS - 1)) ? -lv : lv;  // fp32(lv) * sign, -0 kept
            v[j] = sv * nrm;                                   // compressors.py:357 (rounded before the fma)
          }
        }
        acc[u] = make_float4(fmaf(wc, v[0], acc[u].x), fmaf(wc, v[1], acc[u].y), fmaf(wc, v[2], acc[u].z),
                             fmaf(wc, v[3], acc[u].w));
      }
    }
  }
}

// records [r0, r0 + rn) of the launch, all decoded fp32 vectors of n elements
__device__ __forceinline__ void mixed_flat_run(const FoldArgs& a, int r0, int rn, int64_t n, int64_t t0, int lane,
                                               float4 acc[4]) {
  constexpr int kBatch = 4;
  for (int c0 = 0; c0 < rn; c0 += kBatch) {
    float4 fv[kBatch][4];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
#pragma unroll
      for (int u = 0; u < 4; ++u) fv[i][u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 + i < rn) {
        const float* __restrict__ x = reinterpret_cast<const float*>(a.rec[r0 + c0 + i]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t e = t0 + 4 * (int64_t)(lane + u * kWave);
          if (e + 4 <= n) {
            fv[i][u] = *reinterpret_cast<const float4*>(x + e);
          } else {  // (the vector's last elements; those at or beyond n are never stored)
            if (e < n) fv[i][u].x = x[e];
            if (e + 1 < n) fv[i][u].y = x[e + 1];
            if (e + 2 < n) fv[i][u].z = x[e + 2];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (c0 + i >= rn) continue;  // (uniform)
      const float wc = a.w[r0 + c0 + i];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        acc[u] = make_float4(fmaf(wc, fv[i][u].x, acc[u].x), fmaf(wc, fv[i][u].y, acc[u].y),
                             fmaf(wc, fv[i][u].z, acc[u].z), fmaf(wc, fv[i][u].w, acc[u].w));
    }
  }
}

template <class IO>
__global__ __launch_bounds__(kWave) void mixed_fold_records_kernel(FoldArgs a, MixedDesc d, int nw_all, int64_t n,
                                                                   int64_t tile0, IO io) {
  __shared__ __attribute__((aligned(16))) float s_tile[FLC_TILE];
  __shared__ float s_lvt[kMaxTabs * 128];
  float4* tile4 = reinterpret_cast<float4*>(s_tile);
  const int lane = threadIdx.x;
  for (int tb = 0; tb < d.ntab; ++tb) {  // the launch's level tables (dense_fold_records_kernel's s_lvt, one per codec)
    const int fmt = d.tab_fmt[tb], s = d.tab_levels[tb];
    if (fmt == kTabStacked) continue;
    const int nl = 1 << ((int)d.tab_bits[tb] - 1);
    const double step = d.tab_step[tb];
    for (int i = lane; i < nl; i += kWave)
      s_lvt[tb * 128 + i] =
          fmt == FLC_Q_STANDARD_DITHER ? (float)level_value<0>(i, s, step) : (float)level_value<1>(i, s, step);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) tile4[lane + u * kWave] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  // the block's records: the whole launch's, or (a grouped launch) its group's slice of them
  int nw = nw_all, rec0 = 0;
  if constexpr (IO::kGrouped) {
    nw = io.count();
    rec0 = io.first();
  }
  const int64_t t = tile0 + blockIdx.x;
  const int64_t t0 = t * FLC_TILE;
  float4 acc[4];
  io.load(t0, lane, acc);
  int c = rec0;
  const int end = rec0 + nw;
  while (c < end) {
    const int cls = d.cls[c], rcl = run_class(cls);
    int e = c + 1;
    while (e < end && run_class(d.cls[e]) == rcl) ++e;
    if (rcl == 0) mixed_entry_run(a, d, c, e - c, t, t0, lane, s_tile, acc);
    else if (cls == kClsQ8) mixed_dense_run<8>(a, d, c, e - c, s_lvt, n, t0, lane, acc);
    else if (cls == kClsQ4) mixed_dense_run<4>(a, d, c, e - c, s_lvt, n, t0, lane, acc);
    else if (cls == kClsQ2) mixed_dense_run<2>(a, d, c, e - c, s_lvt, n, t0, lane, acc);
    else if (cls == kClsN16) mixed_dense_run<16>(a, d, c, e - c, s_lvt, n, t0, lane, acc);
    else mixed_flat_run(a, c, e - c, n, t0, lane, acc);
    c = e;
  }
  io.store(t0, lane, acc);
}

template <class IO>
int launch_mixed_fold(const char* probe, dim3 grid, hipStream_t st, const FoldArgs& a, const MixedDesc& d, int nw,
                      int64_t n, int64_t tile0, const IO& io) {
  FLC_LAUNCH(probe, (mixed_fold_records_kernel<IO>), grid, dim3(kWave), 0, st, a, d, nw, n, tile0, io);
  return FLC_OK;
}

// A mixed round's descriptor arrays (checked by check_mixed_round) as the impls below take them
struct MixedRound {
  const int32_t* kinds;
  const int64_t* ks;
  const int32_t* formats;
  const int32_t* levels;
  const int32_t* bits;
};

// every record's own argument rule: its uniform entry point's, record by record
int check_mixed_round(const char* fn, const void* const* records, const MixedRound& mx, int n_records, int64_t n) {
  if (n_records > 0 && (!records || !mx.kinds || !mx.ks || !mx.formats || !mx.levels || !mx.bits))
    return fail(FLC_EINVAL, "%s: a null descriptor table", fn);
  if (n <= 0 || n >= (1ll << 31)) return fail(FLC_EINVAL, "%s: n must be in [1, 2^31)", fn);
  for (int c = 0; c < n_records; ++c) {
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
    switch (mx.kinds[c]) {
      case FLC_REC_STACKED:
        if (mx.levels[c] < 1 || mx.levels[c] > 127)
          return fail(FLC_EINVAL, "%s: record %d: levels must be in [1, 127]", fn, c);
        [[fallthrough]];
      case FLC_REC_SPARSE:
        if (mx.ks[c] < 1 || mx.ks[c] > n)
          return fail(FLC_EINVAL, "%s: record %d: k %lld outside [1, n = %lld]", fn, c, (long long)mx.ks[c],
                      (long long)n);
        break;
      case FLC_REC_DENSE:
        if (int rc = check_dense_format(fn, mx.formats[c], mx.levels[c], mx.bits[c])) return rc;
        break;
      case FLC_REC_FLAT:
        break;
      default:
        return fail(FLC_EINVAL, "%s: record %d: unknown kind %d", fn, c, (int)mx.kinds[c]);
    }
  }
  return FLC_OK;
}

// record `c` of the round as entry `pos` of a launch's descriptor; false when it needs a table entry and none is left
bool mixed_take(const MixedRound& mx, int c, MixedDesc* d, int pos) {
  int fmt = -1, lv = 0, bits = 8;
  uint8_t cls = kClsFlat;
  d->k[pos] = 0u;
  switch (mx.kinds[c]) {
    case FLC_REC_STACKED:
      cls = kClsStacked;
      fmt = kTabStacked;
      lv = mx.levels[c];
      d->k[pos] = (unsigned)mx.ks[c];
      break;
    case FLC_REC_SPARSE:
      cls = kClsSparse;
      d->k[pos] = (unsigned)mx.ks[c];
      break;
    case FLC_REC_DENSE:
      if (mx.formats[c] == kFmtNatural) {
        cls = kClsN16;
      } else {
        cls = mx.bits[c] == 8 ? kClsQ8 : mx.bits[c] == 4 ? kClsQ4 : kClsQ2;
        fmt = mx.formats[c];
        lv = mx.levels[c];
        bits = mx.bits[c];
      }
      break;
    default:
      break;
  }
  int slot = 0;
  if (fmt >= 0) {
    for (slot = 0; slot < d->ntab; ++slot)
      if (d->tab_fmt[slot] == fmt && d->tab_levels[slot] == lv && d->tab_bits[slot] == bits) break;
    if (slot == d->ntab) {
      if (d->ntab == kMaxTabs) return false;
      d->tab_fmt[slot] = (uint8_t)fmt;
      d->tab_levels[slot] = (uint8_t)lv;
      d->tab_bits[slot] = (uint8_t)bits;
      d->tab_step[slot] = 1.0 / (double)lv;
      ++d->ntab;
    }
  }
  d->cls[pos] = cls;
  d->tab[pos] = (uint8_t)slot;
  return true;
}

// the launch's records from round position c0: at most `cap`, fewer when the tables run out; their count (>= 1 for
// cap >= 1: one record needs at most one table entry)
int mixed_chunk(const MixedRound& mx, int c0, int cap, MixedDesc* d) {
  *d = MixedDesc{};
  int nw = 0;
  while (nw < cap && mixed_take(mx, c0 + nw, d, nw)) ++nw;
  return nw;
}

// What a round's records are, as every host-side fold below takes it: entry records (stacked or sparse) of one
// (n, k, levels), dense records of one DenseCodec, or (mx) a mixed round, every record by its own descriptor.
struct RoundCodec {
  int64_t n;
  RecordKind kind = kRecStacked;  // the entry codec (neither dense nor mixed)
  int64_t k = 0;
  int levels = 1;
  bool is_dense = false;
  DenseCodec dense{};
  const MixedRound* mx = nullptr;

  static RoundCodec entry(RecordKind kind, int64_t n, int64_t k, int levels) {
    RoundCodec c{n};
    c.kind = kind, c.k = k, c.levels = levels;
    return c;
  }
  static RoundCodec dense_records(int64_t n, int format, int levels, int bits) {
    RoundCodec c{n};
    c.is_dense = true, c.dense = DenseCodec{format, levels, bits, n};
    return c;
  }
  // bucket records (flc_bucket_wire_layout); bucket_bad: the size is not a power of two in [64, 4096] (check fails)
  int64_t bucket_bad = 0;
  static RoundCodec bucket_records(int64_t n, int format, int levels, int bits, int64_t bucket) {
    RoundCodec c = dense_records(n, format, levels, bits);
    const int l = bucket_log2(bucket);
    if (l < 0) c.bucket_bad = bucket ? bucket : -1;
    c.dense.logb = l < 0 ? 6 : l;
    return c;
  }
  static RoundCodec mixed(int64_t n, const MixedRound* mx) {
    RoundCodec c{n};
    c.mx = mx;
    return c;
  }

  // the codec's own argument rule (a mixed round's is check_mixed_round, run by its entry point before anything else)
  int check(const char* fn) const {
    if (mx) return FLC_OK;
    if (is_dense && dense.logb) {
      if (bucket_bad)
        return fail(FLC_EINVAL, "%s: bucket %lld is not a power of two in [64, 4096]", fn, (long long)bucket_bad);
      if (dense.format == kFmtNatural) return fail(FLC_EINVAL, "%s: unknown format %d", fn, dense.format);
    }
    if (is_dense) return check_dense_format(fn, dense.format, dense.levels, dense.bits);
    return check_entry_codec(fn, kind, n, k, levels);
  }
  // bytes of one record of a uniform round (after check)
  size_t record_size() const {
    size_t need = 0;
    if (is_dense && dense.logb)
      return align_up((size_t)bucket_codes_offset(n, dense.logb) + ((size_t)n * (size_t)dense.bits + 7) / 8, 256);
    if (is_dense) return dense_wire_size(n, dense.format, dense.bits);
    record_layout(kind, n, k, &need);
    return need;
  }
  // record `c` of the round as entry `pos` of a launch; false: a mixed launch's level tables are full
  bool take(int c, MixedDesc* d, int pos) const { return !mx || mixed_take(*mx, c, d, pos); }
  // how many records the next launch takes from round position c0: `cap`, fewer where a mixed launch's tables run out
  int chunk(int c0, int cap, MixedDesc* d) const { return mx ? mixed_chunk(*mx, c0, cap, d) : cap; }
  // one launch of the fold: the kernel by the round's codec (`sparse_form`: entry records only; `d`: mixed rounds only)
  template <class IO>
  int launch(const char* probe, bool sparse_form, dim3 grid, hipStream_t st, const FoldArgs& a, const MixedDesc& d,
             int nw, int64_t tile_lo, const IO& io) const {
    if constexpr (!std::is_same_v<IO, FlatIO>) {  // (the wire folds have no mixed form)
      if (mx) return launch_mixed_fold(probe, grid, st, a, d, nw, n, tile_lo, io);
    }
    if (is_dense) return launch_dense_fold(probe, dense, grid, st, a, nw, tile_lo, io);
    size_t need = 0;
    const WireLayout L = record_layout(kind, n, k, &need);
    return launch_entry_fold(probe, kind, sparse_form, grid, st, a, L, nw, levels,
                             1.0 / (double)(levels < 1 ? 1 : levels), tile_lo, io, (unsigned)k);
  }
};

}  // namespace
}  // namespace flc

using namespace flc;

extern "C" {

size_t flc_stacked_wire_layout(int64_t n, int64_t k, int64_t* offsets) {
  if (n <= 0 || k < 0) return 0;
  size_t total = 0;
  const WireLayout L = wire_layout(n, k, &total);
  if (offsets) {
    offsets[0] = L.norm;
    offsets[1] = L.idx;
    offsets[2] = L.codes;
    offsets[3] = L.tiles;
  }
  return total;
}

size_t flc_sparse_wire_layout(int64_t n, int64_t k, int64_t* offsets) {
  if (n < 1 || k < 1 || k > n || n >= (1ll << 31) || k >= (1ll << 31)) return 0;
  size_t total = 0;
  const WireLayout L = sparse_wire_layout(n, k, &total);
  if (offsets) {
    offsets[0] = L.idx;
    offsets[1] = L.codes;  // (val)
    offsets[2] = L.tiles;
  }
  return total;
}

// flc_stacked_fold_wires, flc_fold_sparse_wires and flc_fold_dense_wires: one argument check, one chain of launches
// (a chained launch continues from the stored out), the kernel by the records' codec
static int fold_wires_impl(const char* fn, const char* probe, const RoundCodec& codec, const void* wires,
                           int64_t stride, const int32_t* slots, const float* weights, int n_wires, int accumulate,
                           float* out, void* stream) {
  const int64_t n = codec.n, k = codec.k;
  if (!wires || !slots || !weights || !out || n_wires < 1 || n <= 0 || k < 0)
    return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (codec.is_dense) {
    if (n >= (1ll << 31)) return fail(FLC_EINVAL, "%s: n must be < 2^31", fn);
  } else if (n >= (1ll << 31) || k >= (1ll << 31)) {
    return fail(FLC_EINVAL, "%s: n and k must be < 2^31", fn);
  }
  if (int rc = codec.check(fn)) return rc;
  const size_t need = codec.record_size();
  if (stride < (int64_t)need || stride % 16 != 0)
    return fail(FLC_EINVAL, "%s: stride %lld < record size %zu (or not 16-B aligned)", fn, (long long)stride, need);
  if (!aligned16(wires) || !aligned16(out)) return fail(FLC_EINVAL, "%s: 16-B aligned buffers required", fn);
  for (int c = 0; c < n_wires; ++c)
    if (slots[c] < 0) return fail(FLC_EINVAL, "%s: slot %d is negative", fn, c);
  hipStream_t st = as_stream(stream);
  const int64_t ntiles = cdiv(n, (int64_t)FLC_TILE);
  // Sparse fold (entry records, from +0, finite weights): only the kept entries are fma'd, and a final -0 is resolved
  // as the dense chain would (kernel header).  Otherwise (accumulating into a given vector, or a non-finite weight)
  // every element takes every client's fma.
  bool sparse = !accumulate;
  for (int c = 0; c < n_wires; ++c) sparse = sparse && std::isfinite(weights[c]);
  const MixedDesc none{};
  for (int c0 = 0; c0 < n_wires; c0 += kMaxWires) {
    const int nw = std::min(kMaxWires, n_wires - c0);
    FoldArgs a;
    for (int c = 0; c < kMaxWires; ++c) {
      a.w[c] = c < nw ? weights[c0 + c] : 0.0f;
      a.rec[c] = static_cast<const uint8_t*>(wires) + (c < nw ? (int64_t)slots[c0 + c] * stride : 0);
    }
    const FlatIO io{out, n, (c0 > 0 || accumulate) ? 1 : 0};
    if (int rc = codec.launch(probe, sparse, dim3((unsigned)ntiles), st, a, none, nw, (int64_t)0, io)) return rc;
  }
  return FLC_OK;
}

int flc_stacked_fold_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                           int64_t n, int64_t k, int levels, int accumulate, float* out, void* stream) {
  return fold_wires_impl("flc_stacked_fold_wires", "stacked_fold_wires", RoundCodec::entry(kRecStacked, n, k, levels),
                         wires, stride, slots, weights, n_wires, accumulate, out, stream);
}

int flc_fold_sparse_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                          int64_t n, int64_t k, int accumulate, float* out, void* stream) {
  return fold_wires_impl("flc_fold_sparse_wires", "fold_sparse_wires", RoundCodec::entry(kRecSparse, n, k, 0), wires,
                         stride, slots, weights, n_wires, accumulate, out, stream);
}

// The FedOpt folds (flc_fedopt_fold_records, _sparse_records, _dense_records, _mixed_records): one argument check, one
// chain of launches, the kernel by the round's codec.  `fn` names the entry point in messages, `probe` its launches
// for flc_probe_set.  (A mixed launch ends at 64 records or where its level tables run out.)
static int fedopt_fold_impl(const char* fn, const char* probe, const RoundCodec& codec, const void* const* records,
                            const float* weights, int n_records, float* const* delta, float* const* theta,
                            float* const* v, const int64_t* sizes, int n_tensors, float beta0, int opt, double lr,
                            double beta2, double tau, void* stream) {
  const int64_t n = codec.n, k = codec.k;
  if (n_records < 0 || (n_records > 0 && (!records || !weights)) || n <= 0 || k < 0 || n_tensors < 1 || !delta ||
      !sizes)
    return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (n >= (1ll << 31) || k >= (1ll << 31)) return fail(FLC_EINVAL, "%s: n and k must be < 2^31", fn);
  if (int rc = codec.check(fn)) return rc;
  const bool step_on = theta != nullptr;
  if (step_on && opt != FLC_OPT_AVG && opt != FLC_OPT_ADAGRAD && opt != FLC_OPT_YOGI && opt != FLC_OPT_ADAM)
    return fail(FLC_EINVAL, "%s: unknown optimiser %d", fn, opt);
  if (step_on && opt != FLC_OPT_AVG && !v) return fail(FLC_EINVAL, "%s: v required for adaptive optimisers", fn);
  int64_t total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes[t] < 0) return fail(FLC_EINVAL, "%s: negative size for tensor %d", fn, t);
    if (sizes[t] > 0 && (!delta[t] || (step_on && !theta[t]) || (step_on && opt != FLC_OPT_AVG && !v[t])))
      return fail(FLC_EINVAL, "%s: null pointer for tensor %d", fn, t);
    total += sizes[t];
  }
  if (total != n)
    return fail(FLC_EINVAL, "%s: the tensors hold %lld elements, the records %lld", fn, (long long)total,
                (long long)n);
  for (int c = 0; c < n_records; ++c)
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
  hipStream_t st = as_stream(stream);
  const float omb = (float)(1.0 - beta2), nomb = (float)(-(1.0 - beta2));
  // record chunks in order (the chain continues from the stored δ, the step after the last chunk only); within a
  // chunk, one launch per group of <= kRoundT tensors over the tiles their flat range touches
  int c0 = 0;
  do {
    MixedDesc md;
    const int nw = codec.chunk(c0, std::min(kMaxWires, n_records - c0), &md);
    const bool last = c0 + nw >= n_records;
    FoldArgs a;
    for (int c = 0; c < kMaxWires; ++c) {
      a.w[c] = c < nw ? weights[c0 + c] : 0.0f;
      a.rec[c] = static_cast<const uint8_t*>(c < nw ? records[c0 + c] : nullptr);
    }
    int64_t off = 0;
    int t = 0;
    while (t < n_tensors) {
      ModelTab m{};
      m.scale = c0 == 0;
      m.beta0 = beta0;
      m.lr = (float)lr;
      m.beta2 = (float)beta2;
      m.omb = omb;
      m.nomb = nomb;
      m.tau = (float)tau;
      for (; t < n_tensors && m.nt < kRoundT; ++t) {
        if (sizes[t] == 0) continue;
        const int i = m.nt++;
        m.delta[i] = delta[t];
        m.theta[i] = step_on ? theta[t] : nullptr;
        m.v[i] = (step_on && opt != FLC_OPT_AVG) ? v[t] : nullptr;
        m.start[i] = off;
        const bool vec = off % 4 == 0 && aligned16(m.delta[i]) && (!m.theta[i] || aligned16(m.theta[i])) &&
                         (!m.v[i] || aligned16(m.v[i]));
        if (vec) m.vec |= 1u << i;
        off += sizes[t];
      }
      if (m.nt == 0) break;
      m.start[m.nt] = off;
      const int64_t tile_lo = m.start[0] / FLC_TILE, tile_hi = cdiv(off, (int64_t)FLC_TILE);
      const dim3 grid((unsigned)(tile_hi - tile_lo));
      // (never the sparse form: δ continues from β0·δ, and ModelIO has none)
#define FLC_FR(O)                                                                                       \
  do {                                                                                                  \
    if (int rc = codec.launch(probe, false, grid, st, a, md, nw, tile_lo, ModelIO<O>{m})) return rc;    \
  } while (0)
      if (!step_on || !last) FLC_FR(-1);
      else if (opt == FLC_OPT_AVG) FLC_FR(FLC_OPT_AVG);
      else if (opt == FLC_OPT_ADAGRAD) FLC_FR(FLC_OPT_ADAGRAD);
      else if (opt == FLC_OPT_YOGI) FLC_FR(FLC_OPT_YOGI);
      else FLC_FR(FLC_OPT_ADAM);
#undef FLC_FR
    }
    c0 += nw;
  } while (c0 < n_records);
  return FLC_OK;
}

int flc_fedopt_fold_records(const void* const* records, const float* weights, int n_records, int64_t n, int64_t k,
                            int levels, float* const* delta, float* const* theta, float* const* v,
                            const int64_t* sizes, int n_tensors, float beta0, int opt, double lr, double beta2,
                            double tau, void* stream) {
  return fedopt_fold_impl("flc_fedopt_fold_records", "fedopt_fold_records",
                          RoundCodec::entry(kRecStacked, n, k, levels), records, weights, n_records, delta, theta, v,
                          sizes, n_tensors, beta0, opt, lr, beta2, tau, stream);
}

int flc_fedopt_fold_sparse_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                   int64_t k, float* const* delta, float* const* theta, float* const* v,
                                   const int64_t* sizes, int n_tensors, float beta0, int opt, double lr, double beta2,
                                   double tau, void* stream) {
  return fedopt_fold_impl("flc_fedopt_fold_sparse_records", "fedopt_fold_sparse_records",
                          RoundCodec::entry(kRecSparse, n, k, 0), records, weights, n_records, delta, theta, v, sizes,
                          n_tensors, beta0, opt, lr, beta2, tau, stream);
}

int flc_fedopt_fold_dense_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                  int format, int levels, int bits, float* const* delta, float* const* theta,
                                  float* const* v, const int64_t* sizes, int n_tensors, float beta0, int opt,
                                  double lr, double beta2, double tau, void* stream) {
  return fedopt_fold_impl("flc_fedopt_fold_dense_records", "fedopt_fold_dense_records",
                          RoundCodec::dense_records(n, format, levels, bits), records, weights, n_records, delta, theta,
                          v, sizes, n_tensors, beta0, opt, lr, beta2, tau, stream);
}

int flc_fedopt_fold_bucket_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                   int format, int levels, int bits, int64_t bucket, float* const* delta,
                                   float* const* theta, float* const* v, const int64_t* sizes, int n_tensors,
                                   float beta0, int opt, double lr, double beta2, double tau, void* stream) {
  return fedopt_fold_impl("flc_fedopt_fold_bucket_records", "fedopt_fold_bucket_records",
                          RoundCodec::bucket_records(n, format, levels, bits, bucket), records, weights, n_records,
                          delta, theta, v, sizes, n_tensors, beta0, opt, lr, beta2, tau, stream);
}

// The variance-reduced servers' folds (flc_avg_and_gradient_records, _sparse_records, _dense_records, _mixed_records),
// as fedopt_fold_impl serves the FedOpt folds: one argument check and one chain of launches, the kernel by the round's
// codec
static int avg_and_gradient_impl(const char* fn, const char* probe, const RoundCodec& codec, float* const* params,
                                 float* const* grads, const float* const* param_srcs,
                                 const void* const* grad_records, const float* w_params, const float* w_grads,
                                 int n_src, const int64_t* sizes, int n_tensors, float inertia, void* stream) {
  const int64_t n = codec.n, k = codec.k;
  const bool p_on = param_srcs != nullptr;
  if (n_src < 1 || !grad_records || !w_grads || n <= 0 || k < 0 || n_tensors < 1 || !grads || !sizes ||
      (p_on && (!params || !w_params)))
    return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (n >= (1ll << 31) || k >= (1ll << 31))
    return fail(FLC_EINVAL, "%s: n and k must be < 2^31", fn);
  if (int rc = codec.check(fn)) return rc;
  int64_t total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes[t] < 0) return fail(FLC_EINVAL, "%s: negative size for tensor %d", fn, t);
    if (sizes[t] > 0 && (!grads[t] || (p_on && !params[t])))
      return fail(FLC_EINVAL, "%s: null pointer for tensor %d", fn, t);
    if (p_on && sizes[t] > 0)
      for (int m = 0; m < n_src; ++m)
        if (!param_srcs[(size_t)m * n_tensors + t])
          return fail(FLC_EINVAL, "%s: null source %d of tensor %d", fn, m, t);
    total += sizes[t];
  }
  if (total != n)
    return fail(FLC_EINVAL, "%s: the tensors hold %lld elements, the records %lld", fn,
                (long long)total, (long long)n);
  for (int c = 0; c < n_src; ++c)
    if (!grad_records[c] || !aligned16(grad_records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
  hipStream_t st = as_stream(stream);
  // the gradient chain starts at +0: with finite weights only the kept entries are fma'd (the sparse form, its -0
  // rule as in flc_stacked_fold_wires); a non-finite weight takes every element through every record's fma.  (Dense
  // records carry a code for every element: their fold has no sparse form and needs no -0 replay.)
  bool sparse = true;
  for (int c = 0; c < n_src; ++c) sparse = sparse && std::isfinite(w_grads[c]);
  // launch i of the chain folds the i-th chunk of records (64; a mixed round's ends earlier where its level tables run
  // out — `cuts` holds the chunks' starts) and parameter sources [16 i, 16 i + 16), each chain continuing from its
  // stored partial result; within it, one launch per group of <= kRoundT tensors
  std::vector<int> cuts;
  MixedDesc md;
  for (int c = 0; c < n_src; c += codec.chunk(c, std::min(kMaxWires, n_src - c), &md)) cuts.push_back(c);
  const int r_launches = (int)cuts.size();
  const int p_launches = p_on ? (int)cdiv((int64_t)n_src, (int64_t)kPairSrc) : 0;
  for (int i = 0; i < std::max(r_launches, p_launches); ++i) {
    const int c0 = i < r_launches ? cuts[i] : n_src, s0 = i * kPairSrc;
    const int nw = codec.chunk(c0, i < r_launches ? std::min(kMaxWires, n_src - c0) : 0, &md);
    const int ns = i < p_launches ? std::min(kPairSrc, n_src - s0) : 0;
    FoldArgs a;
    for (int c = 0; c < kMaxWires; ++c) {
      a.w[c] = c < nw ? w_grads[c0 + c] : 0.0f;
      a.rec[c] = static_cast<const uint8_t*>(c < nw ? grad_records[c0 + c] : nullptr);
    }
    int64_t off = 0;
    int t = 0;
    while (t < n_tensors) {
      PairIO io{};
      PairTab& m = io.m;
      m.ns = ns;
      m.g_on = nw > 0;
      m.g_acc = i > 0;
      m.p_on = ns > 0;
      m.p_scale = i == 0;
      m.inertia = inertia;
      for (int s = 0; s < ns; ++s) m.w[s] = w_params[s0 + s];
      for (; t < n_tensors && m.nt < kRoundT; ++t) {
        if (sizes[t] == 0) continue;
        const int j = m.nt++;
        m.grad[j] = grads[t];
        m.param[j] = p_on ? params[t] : nullptr;
        m.start[j] = off;
        if (off % 4 == 0 && aligned16(m.grad[j])) m.gvec |= 1u << j;
        bool pv = off % 4 == 0 && p_on && aligned16(m.param[j]);
        for (int s = 0; s < ns; ++s) {
          m.src[s][j] = param_srcs[(size_t)(s0 + s) * n_tensors + t];
          pv = pv && aligned16(m.src[s][j]);
        }
        if (pv) m.pvec |= 1u << j;
        off += sizes[t];
      }
      if (m.nt == 0) break;
      m.start[m.nt] = off;
      const int64_t tile_lo = m.start[0] / FLC_TILE, tile_hi = cdiv(off, (int64_t)FLC_TILE);
      const dim3 grid((unsigned)(tile_hi - tile_lo));
      if (int rc = codec.launch(probe, sparse, grid, st, a, md, nw, tile_lo, io)) return rc;
    }
  }
  return FLC_OK;
}

int flc_avg_and_gradient_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                 const void* const* grad_records, const float* w_params, const float* w_grads,
                                 int n_src, int64_t n, int64_t k, int levels, const int64_t* sizes, int n_tensors,
                                 float inertia, void* stream) {
  return avg_and_gradient_impl("flc_avg_and_gradient_records", "avg_and_gradient_records",
                               RoundCodec::entry(kRecStacked, n, k, levels), params, grads, param_srcs, grad_records,
                               w_params, w_grads, n_src, sizes, n_tensors, inertia, stream);
}

int flc_avg_and_gradient_sparse_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                        const void* const* grad_records, const float* w_params, const float* w_grads,
                                        int n_src, int64_t n, int64_t k, const int64_t* sizes, int n_tensors,
                                        float inertia, void* stream) {
  return avg_and_gradient_impl("flc_avg_and_gradient_sparse_records", "avg_and_gradient_sparse_records",
                               RoundCodec::entry(kRecSparse, n, k, 0), params, grads, param_srcs, grad_records,
                               w_params, w_grads, n_src, sizes, n_tensors, inertia, stream);
}

int flc_avg_and_gradient_dense_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                       const void* const* grad_records, const float* w_params, const float* w_grads,
                                       int n_src, int64_t n, int format, int levels, int bits, const int64_t* sizes,
                                       int n_tensors, float inertia, void* stream) {
  return avg_and_gradient_impl("flc_avg_and_gradient_dense_records", "avg_and_gradient_dense_records",
                               RoundCodec::dense_records(n, format, levels, bits), params, grads, param_srcs,
                               grad_records, w_params, w_grads, n_src, sizes, n_tensors, inertia, stream);
}

int flc_avg_and_gradient_bucket_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                        const void* const* grad_records, const float* w_params, const float* w_grads,
                                        int n_src, int64_t n, int format, int levels, int bits, int64_t bucket,
                                        const int64_t* sizes, int n_tensors, float inertia, void* stream) {
  return avg_and_gradient_impl("flc_avg_and_gradient_bucket_records", "avg_and_gradient_bucket_records",
                               RoundCodec::bucket_records(n, format, levels, bits, bucket), params, grads, param_srcs,
                               grad_records, w_params, w_grads, n_src, sizes, n_tensors, inertia, stream);
}

// The grouped folds (flc_fold_record_groups, _sparse_record_groups, _dense_record_groups, _mixed_record_groups), as
// fedopt_fold_impl serves the FedOpt folds
static int fold_groups_impl(const char* fn, const char* probe, const RoundCodec& codec, const void* const* records,
                            const float* weights, const int32_t* group_of, int n_records, float* const* dsts,
                            int n_groups, const int64_t* sizes, int n_tensors, void* stream) {
  const int64_t n = codec.n, k = codec.k;
  if (n_records < 0 || (n_records > 0 && (!records || !weights || !group_of)) || n <= 0 || k < 0 || n_groups < 1 ||
      n_tensors < 1 || !dsts || !sizes)
    return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (n >= (1ll << 31) || k >= (1ll << 31)) return fail(FLC_EINVAL, "%s: n and k must be < 2^31", fn);
  if (int rc = codec.check(fn)) return rc;
  int64_t total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes[t] < 0) return fail(FLC_EINVAL, "%s: negative size for tensor %d", fn, t);
    total += sizes[t];
  }
  if (total != n)
    return fail(FLC_EINVAL, "%s: the tensors hold %lld elements, the records %lld", fn, (long long)total,
                (long long)n);
  std::vector<int> members(n_groups, 0);
  for (int c = 0; c < n_records; ++c) {
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
    if (group_of[c] < 0 || group_of[c] >= n_groups)
      return fail(FLC_EINVAL, "%s: record %d names group %d outside [0, %d)", fn, c, (int)group_of[c], n_groups);
    ++members[group_of[c]];
  }
  std::vector<std::pair<uintptr_t, int>> owners;  // (destination, group) of every non-empty tensor
  for (int g = 0; g < n_groups; ++g)
    for (int t = 0; t < n_tensors; ++t) {
      float* d = dsts[(size_t)g * n_tensors + t];
      if (sizes[t] == 0) continue;
      if (!d) {
        if (members[g] > 0) return fail(FLC_EINVAL, "%s: null pointer for tensor %d of group %d", fn, t, g);
        continue;
      }
      owners.emplace_back(reinterpret_cast<uintptr_t>(d), g);
    }
  std::sort(owners.begin(), owners.end());
  for (size_t i = 1; i < owners.size(); ++i)
    if (owners[i].first == owners[i - 1].first && owners[i].second != owners[i - 1].second)
      return fail(FLC_EINVAL, "%s: groups %d and %d share a destination", fn, owners[i - 1].second,
                  owners[i].second);
  if (n_records == 0) return FLC_OK;
  hipStream_t st = as_stream(stream);
  // the records ordered by group, each group's in message order
  std::vector<int> order(n_records);
  for (int c = 0; c < n_records; ++c) order[c] = c;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return group_of[x] < group_of[y]; });
  // launches over the ordered records: each takes <= kMaxWires records of <= kMaxGroups groups (a group cut by a
  // launch's end continues in the next one from its stored results); within it, one launch per <= kRoundT tensors
  int c0 = 0;
  while (c0 < n_records) {
    FoldArgs a;
    GroupIO io{};
    GroupTab& m = io.m;
    int gsel[kMaxGroups];
    int nw = 0, ng = 0;
    MixedDesc md{};
    // Sparse form (only the kept entries are fma'd, a -0 resolved as the dense chain resolves it) whenever every
    // weight of the launch is finite: from ANY stored accumulator a, fmaf(w, +0, a) with a finite w returns a itself
    // unless a is -0 and w's sign bit is clear — exactly skip_clients' rule (NaN stays NaN, ±inf stays ±inf).
    bool sparse = true;
    while (c0 + nw < n_records && nw < kMaxWires) {
      const int c = order[c0 + nw], g = group_of[c];
      const bool opens = ng == 0 || gsel[ng - 1] != g;
      if (opens && ng == kMaxGroups) break;
      if (!codec.take(c, &md, nw)) break;  // (a mixed launch's level tables are full: the next launch)
      if (opens) {
        gsel[ng] = g;
        m.first[ng] = nw;
        m.count[ng] = 0;
        ++ng;
      }
      a.rec[nw] = static_cast<const uint8_t*>(records[c]);
      a.w[nw] = weights[c];
      sparse = sparse && std::isfinite(weights[c]);
      ++m.count[ng - 1];
      ++nw;
    }
    for (int c = nw; c < kMaxWires; ++c) {
      a.rec[c] = nullptr;
      a.w[c] = 0.0f;
    }
    int64_t off = 0;
    int t = 0;
    while (t < n_tensors) {
      m.nt = 0;
      for (int g = 0; g < kMaxGroups; ++g) m.vec[g] = 0u;
      for (; t < n_tensors && m.nt < kRoundT; ++t) {
        if (sizes[t] == 0) continue;
        const int i = m.nt++;
        m.start[i] = off;
        for (int g = 0; g < ng; ++g) {
          m.dst[g][i] = dsts[(size_t)gsel[g] * n_tensors + t];
          if (off % 4 == 0 && aligned16(m.dst[g][i])) m.vec[g] |= 1u << i;
        }
        off += sizes[t];
      }
      if (m.nt == 0) break;
      m.start[m.nt] = off;
      const int64_t tile_lo = m.start[0] / FLC_TILE, tile_hi = cdiv(off, (int64_t)FLC_TILE);
      const dim3 grid((unsigned)(tile_hi - tile_lo), (unsigned)ng);
      if (int rc = codec.launch(probe, sparse, grid, st, a, md, nw, tile_lo, io)) return rc;
    }
    c0 += nw;
  }
  return FLC_OK;
}

int flc_fold_record_groups(const void* const* records, const float* weights, const int32_t* group_of, int n_records,
                           int64_t n, int64_t k, int levels, float* const* dsts, int n_groups, const int64_t* sizes,
                           int n_tensors, void* stream) {
  return fold_groups_impl("flc_fold_record_groups", "fold_record_groups", RoundCodec::entry(kRecStacked, n, k, levels),
                          records, weights, group_of, n_records, dsts, n_groups, sizes, n_tensors, stream);
}

int flc_fold_sparse_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                  int n_records, int64_t n, int64_t k, float* const* dsts, int n_groups,
                                  const int64_t* sizes, int n_tensors, void* stream) {
  return fold_groups_impl("flc_fold_sparse_record_groups", "fold_sparse_record_groups",
                          RoundCodec::entry(kRecSparse, n, k, 0), records, weights, group_of, n_records, dsts, n_groups,
                          sizes, n_tensors, stream);
}

int flc_fold_dense_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                 int n_records, int64_t n, int format, int levels, int bits, float* const* dsts,
                                 int n_groups, const int64_t* sizes, int n_tensors, void* stream) {
  return fold_groups_impl("flc_fold_dense_record_groups", "fold_dense_record_groups",
                          RoundCodec::dense_records(n, format, levels, bits), records, weights, group_of, n_records,
                          dsts, n_groups, sizes, n_tensors, stream);
}

int flc_fold_bucket_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                  int n_records, int64_t n, int format, int levels, int bits, int64_t bucket,
                                  float* const* dsts, int n_groups, const int64_t* sizes, int n_tensors,
                                  void* stream) {
  return fold_groups_impl("flc_fold_bucket_record_groups", "fold_bucket_record_groups",
                          RoundCodec::bucket_records(n, format, levels, bits, bucket), records, weights, group_of,
                          n_records, dsts, n_groups, sizes, n_tensors, stream);
}

// The mixed entry points: the descriptor tables' own check first (check_mixed_round), then the uniform folds' impl
int flc_fedopt_fold_mixed_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                  const int32_t* kinds, const int64_t* ks, const int32_t* formats,
                                  const int32_t* levels, const int32_t* bits, float* const* delta, float* const* theta,
                                  float* const* v, const int64_t* sizes, int n_tensors, float beta0, int opt, double lr,
                                  double beta2, double tau, void* stream) {
  const char* fn = "flc_fedopt_fold_mixed_records";
  const MixedRound mx{kinds, ks, formats, levels, bits};
  if (n_records < 0) return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (int rc = check_mixed_round(fn, records, mx, n_records, n)) return rc;
  return fedopt_fold_impl(fn, "fedopt_fold_mixed_records", RoundCodec::mixed(n, &mx), records, weights, n_records,
                          delta, theta, v, sizes, n_tensors, beta0, opt, lr, beta2, tau, stream);
}

int flc_fold_mixed_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                 int n_records, int64_t n, const int32_t* kinds, const int64_t* ks,
                                 const int32_t* formats, const int32_t* levels, const int32_t* bits, float* const* dsts,
                                 int n_groups, const int64_t* sizes, int n_tensors, void* stream) {
  const char* fn = "flc_fold_mixed_record_groups";
  const MixedRound mx{kinds, ks, formats, levels, bits};
  if (n_records < 0) return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (int rc = check_mixed_round(fn, records, mx, n_records, n)) return rc;
  return fold_groups_impl(fn, "fold_mixed_record_groups", RoundCodec::mixed(n, &mx), records, weights, group_of,
                          n_records, dsts, n_groups, sizes, n_tensors, stream);
}

int flc_avg_and_gradient_mixed_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                       const void* const* grad_records, const float* w_params, const float* w_grads,
                                       int n_src, int64_t n, const int32_t* kinds, const int64_t* ks,
                                       const int32_t* formats, const int32_t* levels, const int32_t* bits,
                                       const int64_t* sizes, int n_tensors, float inertia, void* stream) {
  const char* fn = "flc_avg_and_gradient_mixed_records";
  const MixedRound mx{kinds, ks, formats, levels, bits};
  if (n_src < 1 || !grad_records) return fail(FLC_EINVAL, "%s: bad arguments", fn);
  if (int rc = check_mixed_round(fn, grad_records, mx, n_src, n)) return rc;
  return avg_and_gradient_impl(fn, "avg_and_gradient_mixed_records", RoundCodec::mixed(n, &mx), params, grads,
                               param_srcs, grad_records, w_params, w_grads, n_src, sizes, n_tensors, inertia, stream);
}

size_t flc_dense_wire_layout(int64_t n, int format, int bits, int64_t* offsets) {
  if (n < 1 || n >= (1ll << 31)) return 0;
  if (format == kFmtNatural ? bits != 16
                            : ((format != FLC_Q_STANDARD_DITHER && format != FLC_Q_NATURAL_DITHER) ||
                               (bits != 2 && bits != 4 && bits != 8)))
    return 0;
  if (offsets) {
    offsets[0] = kDenseNorm;
    offsets[1] = kDenseCodes;
  }
  return dense_wire_size(n, format, bits);
}

int flc_fold_dense_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                         int64_t n, int format, int levels, int bits, int accumulate, float* out, void* stream) {
  return fold_wires_impl("flc_fold_dense_wires", "fold_dense_wires", RoundCodec::dense_records(n, format, levels, bits),
                         wires, stride, slots, weights, n_wires, accumulate, out, stream);
}

int flc_fold_bucket_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                          int64_t n, int format, int levels, int bits, int64_t bucket, int accumulate, float* out,
                          void* stream) {
  return fold_wires_impl("flc_fold_bucket_wires", "fold_bucket_wires",
                         RoundCodec::bucket_records(n, format, levels, bits, bucket), wires, stride, slots, weights,
                         n_wires, accumulate, out, stream);
}

}  // extern "C"
