// sketch.hip — the Count Sketch of FetchSGD (Rothchild et al., ICML 2020) with a tiled hash: the one-pass encode, the
// server's median-of-rows estimate (unsketch), the fold / momentum / error state step on tables and the clearing of
// kept coordinates.  gfx950 only.  include/flcodec.h pins the hash; in short, with T = 1024 and NT = cols / T:
//   element i: chunk q = i / cols, source tile p = (i % cols) / T, offset o = i % T, global tile g = i / T;
//   tile map (all rows): (x, y) = philox(q, seed, 0x100), A = (x | 1) % NT, B = y % NT, table tile tau of chunk q
//     receives source tile p = (A tau + B) % NT;
//   in-tile permutation (row j, tile g): (x, y) = philox(g, seed, 0x200 + j), a = (x | 1) % T, b = y % T, offset o
//     lands at (a o + b) % T;
//   sign (row j): bit i & 31 of word (i >> 5) & 3 of philox(i >> 7, seed, 0x300 + j): 32 words per tile.
//
// Both big kernels give a block one table tile tau and a contiguous range of chunks, so every global access is a whole
// coalesced tile and the permutation happens inside LDS: no atomics, a fixed summation order.
//
// tile_words            the random words of one (chunk, tau): the tile map for p, then lanes 0 .. 9 R - 1 of ONE wave
//                       run one Philox call each (8 sign groups and 1 permutation per row) and leave them in LDS, the
//                       permutation with a^-1 mod T (Newton steps) beside it.  A block works in batches of four
//                       chunks: wave w computes the words of chunk w of the NEXT batch while the current batch's loads
//                       are in flight, so a chunk costs each wave a quarter of two Philox calls, not 4 R per element.
// sketch_pass_kernel    reads x ONCE.  Per chunk the source tile goes into LDS as it was loaded (16-B loads, 256
//                       threads x 4 elements, one 16-B LDS store each) and every row GATHERS from it: thread t owns
//                       the cells t, t + 256, t + 512, t + 768 of its table tile and reads offset a^-1 (cell - b) % T.
//                       A wave's 64 consecutive cells read 64 offsets a^-1 apart: a^-1 is odd, so they lie in 64
//                       distinct banks.  (The scatter form of the same permutation would start from the four
//                       consecutive offsets a 16-B load leaves in a lane: offsets 4 a apart, a four-way conflict, and it
//                       needs a tile per row in LDS; the gather needs one.)  The sign is applied at the read from
//                       the row's 32 words.  acc[j][k] += s x, chunks ascending from +0; the tile buffer alternates so
//                       a chunk costs one LDS-only barrier and the later loads stay in flight across it.
// sketch_finish_kernel  per cell the splits' partials in fp64, splits ascending from 0.0, rounded once.  One split:
//                       the pass writes the record itself (the same value) and this launch is skipped.
// sketch_estimate_kernel stages the R weighted tiles (fp32(w_0 S_0), then fmaf(w_c, S_c, .), records ascending) in LDS,
//                       <= 20 KB; per chunk thread t owns offsets t + 256 k (consecutive lanes, consecutive offsets:
//                       cells a apart, conflict-free; 256-B coalesced stores), reads its R cells, applies the signs
//                       and takes the median (v_med3_f32; for five, med3 of e, max of the pair minima, min of the pair
//                       maxima).
// sketch_fold_kernel    elementwise on R cols cells: the same S-bar, then table = S-bar, or u = fmaf(rho, u, S-bar) and
//                       v = v + u.
// sketch_cells_kernel   cell_j(i) of given indices, the one place that maps an element FORWARD to its table tile:
//                       tau = A^-1 (p - B) % NT by Newton steps on the odd multiplier.  It clears u and v at the kept
//                       indices and answers the tests' point queries.
#include <algorithm>

#include "flc_device.hpp"
#include "flc_runtime.hpp"

namespace flc {
namespace {

constexpr int kST = 256;           // threads per block
constexpr int kSNW = kST / kWave;  // waves per block = chunks per batch
constexpr int kTile = 1024;        // T
constexpr int kSMaxRec = 64;       // records per launch
#ifndef FLC_SKETCH_MIN_CPS
#define FLC_SKETCH_MIN_CPS 8       // the fewest chunks a split of the encode takes
#endif
constexpr int kMinCps = FLC_SKETCH_MIN_CPS;
constexpr int kEstMinCps = 4;       // ... a block of the estimate
constexpr int kTargetBlocks = 1024; // blocks a launch aims for when there are chunks enough (4 per CU)

constexpr uint64_t kCtrMap = 0x100, kCtrPerm = 0x200, kCtrSign = 0x300;

// the inverse of an odd a modulo 2^32 (so modulo every smaller power of two): a is its own inverse mod 8, and each
// Newton step x <- x (2 - a x) doubles the correct low bits: 3, 6, 12, 24, 48
__device__ __forceinline__ uint32_t inv_odd(uint32_t a) {
  uint32_t x = a;
#pragma unroll
  for (int s = 0; s < 4; ++s) x *= 2u - a * x;
  return x;
}

template <int R>
struct TileWords {
  uint32_t sign[R][32];  // row j's sign words of the tile's 1024 elements
  uint32_t a[R], b[R], ainv[R];
  uint32_t p;            // the source tile
};

// One wave (all 64 lanes call it, q wave-uniform) fills tw for chunk q and table tile tau.
template <int R>
__device__ __forceinline__ void tile_words(int64_t q, uint32_t tau, uint32_t NT, uint64_t seed, TileWords<R>* tw) {
  static_assert(9 * R <= kWave, "one Philox call per lane");
  const int lane = threadIdx.x & (kWave - 1);
  const U4 m = philox_group((uint64_t)q, seed, kCtrMap);
  const uint32_t p = (((m.x | 1u) & (NT - 1)) * tau + m.y) & (NT - 1);
  const uint64_t g = (uint64_t)q * NT + p;
  if (lane == 0) tw->p = p;
  if (lane < 9 * R) {
    const int j = lane / 9, k = lane - 9 * j;
    if (k < 8) {
      const U4 r = philox_group(g * 8 + (uint64_t)k, seed, kCtrSign + (uint64_t)j);
      tw->sign[j][4 * k + 0] = r.x;
      tw->sign[j][4 * k + 1] = r.y;
      tw->sign[j][4 * k + 2] = r.z;
      tw->sign[j][4 * k + 3] = r.w;
    } else {
      const U4 r = philox_group(g, seed, kCtrPerm + (uint64_t)j);
      const uint32_t a = (r.x | 1u) & (kTile - 1);
      tw->a[j] = a;
      tw->b[j] = r.y & (kTile - 1);
      tw->ainv[j] = inv_odd(a) & (kTile - 1);
    }
  }
}

// v with its sign flipped when bit `bit` (mod 32) of w is set
__device__ __forceinline__ float apply_sign(float v, uint32_t w, uint32_t bit) {
  return __uint_as_float(__float_as_uint(v) ^ (((w >> (bit & 31u)) & 1u) << 31));
}

template <int R>
__global__ __launch_bounds__(kST) void sketch_pass_kernel(const float* __restrict__ x, int64_t n, int64_t cols,
                                                          int64_t nchunks, int64_t cps, uint64_t seed,
                                                          float* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) float s_x[2][kTile];
  __shared__ TileWords<R> s_w[2][kSNW];
  const int t = threadIdx.x, wave = t >> 6;
  const uint32_t NT = (uint32_t)(cols / kTile), tau = blockIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * cps, q1 = std::min<int64_t>(q0 + cps, nchunks);

  float acc[R][4];
#pragma unroll
  for (int j = 0; j < R; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[j][k] = 0.0f;

  if (q0 + wave < q1) tile_words<R>(q0 + wave, tau, NT, seed, &s_w[0][wave]);
  int wb = 0, par = 0;
  for (int64_t qb = q0; qb < q1; qb += kSNW, wb ^= 1) {
    lds_barrier();  // this batch's words are written; the previous batch's are read for the last time
    float4 xv[kSNW];
#pragma unroll
    for (int c = 0; c < kSNW; ++c) {
      xv[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qb + c < q1) {  // (block-uniform)
        const int64_t e = (qb + c) * cols + (int64_t)s_w[wb][c].p * kTile + 4 * t;
        if (e + 4 <= n) {
          xv[c] = ld_stream(x + e);
        } else {  // the vector's last tile: element by element, +0 at and past n
          if (e + 0 < n) xv[c].x = x[e + 0];
          if (e + 1 < n) xv[c].y = x[e + 1];
          if (e + 2 < n) xv[c].z = x[e + 2];
        }
      }
    }
    if (qb + kSNW + wave < q1) tile_words<R>(qb + kSNW + wave, tau, NT, seed, &s_w[wb ^ 1][wave]);
#pragma unroll
    for (int c = 0; c < kSNW; ++c) {
      if (qb + c >= q1) break;  // (block-uniform)
      *reinterpret_cast<float4*>(&s_x[par][4 * t]) = xv[c];
      lds_barrier();  // the tile is in LDS; two chunks back everyone has read this buffer (the barrier between)
      const TileWords<R>& w = s_w[wb][c];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const uint32_t ai = w.ainv[j], b = w.b[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t o = (ai * ((uint32_t)(t + 256 * k) - b)) & (kTile - 1);
          acc[j][k] += apply_sign(s_x[par][o], w.sign[j][o >> 5], o);
        }
      }
      par ^= 1;
    }
  }

  float* d = dst + (int64_t)blockIdx.y * R * cols + (int64_t)tau * kTile + t;
#pragma unroll
  for (int j = 0; j < R; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) d[j * cols + 256 * k] = acc[j][k];
}

__global__ __launch_bounds__(kST) void sketch_finish_kernel(const float* __restrict__ part, int64_t cells, int nsplit,
                                                            float* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x;
  if (i >= cells) return;
  double s = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) s += (double)part[(int64_t)sp * cells + i];
  rec[i] = (float)s;
}

struct SketchPack {
  const float* rec[kSMaxRec];
  float w[kSMaxRec];
};

// S-bar of four consecutive cells from cell index i (a multiple of 4): fp32(w_0 S_0), then fmaf(w_c, S_c, .)
__device__ __forceinline__ float4 fold4(const SketchPack& pk, int nrec, int64_t i, bool cont, float4 v) {
  int c = 0;
  if (!cont) {
    const float4 s = *reinterpret_cast<const float4*>(pk.rec[0] + i);
    const float w = pk.w[0];
    v = make_float4(w * s.x, w * s.y, w * s.z, w * s.w);
    c = 1;
  }
  for (; c < nrec; ++c) {
    const float4 s = *reinterpret_cast<const float4*>(pk.rec[c] + i);
    const float w = pk.w[c];
    v = make_float4(fmaf(w, s.x, v.x), fmaf(w, s.y, v.y), fmaf(w, s.z, v.z), fmaf(w, s.w, v.w));
  }
  return v;
}

__device__ __forceinline__ float med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

template <int R>
__device__ __forceinline__ float median(const float (&e)[R]) {
  if constexpr (R == 1) {
    return e[0];
  } else if constexpr (R == 3) {
    return med3(e[0], e[1], e[2]);
  } else {  // the median of five is the median of e4, the larger pair minimum and the smaller pair maximum
    static_assert(R == 5, "rows 1, 3 or 5");
    const float lo = fmaxf(fminf(e[0], e[1]), fminf(e[2], e[3]));
    const float hi = fminf(fmaxf(e[0], e[1]), fmaxf(e[2], e[3]));
    return med3(e[4], lo, hi);
  }
}

template <int R>
__global__ __launch_bounds__(kST) void sketch_estimate_kernel(SketchPack pk, int nrec, int64_t n, int64_t cols,
                                                              int64_t nchunks, int64_t cps, uint64_t seed,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_t[R][kTile];
  __shared__ TileWords<R> s_w[2][kSNW];
  const int t = threadIdx.x, wave = t >> 6;
  const uint32_t NT = (uint32_t)(cols / kTile), tau = blockIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * cps, q1 = std::min<int64_t>(q0 + cps, nchunks);

  if (q0 + wave < q1) tile_words<R>(q0 + wave, tau, NT, seed, &s_w[0][wave]);
#pragma unroll
  for (int j = 0; j < R; ++j)
    *reinterpret_cast<float4*>(&s_t[j][4 * t]) =
        fold4(pk, nrec, j * cols + (int64_t)tau * kTile + 4 * t, false, make_float4(0.f, 0.f, 0.f, 0.f));

  int wb = 0;
  for (int64_t qb = q0; qb < q1; qb += kSNW, wb ^= 1) {
    lds_barrier();  // the tiles and this batch's words are written; the previous batch's words are read for the last time
    if (qb + kSNW + wave < q1) tile_words<R>(qb + kSNW + wave, tau, NT, seed, &s_w[wb ^ 1][wave]);
#pragma unroll
    for (int c = 0; c < kSNW; ++c) {
      if (qb + c >= q1) break;  // (block-uniform)
      const TileWords<R>& w = s_w[wb][c];
      const int64_t e0 = (qb + c) * cols + (int64_t)w.p * kTile;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t o = (uint32_t)(t + 256 * k);
        float e[R];
#pragma unroll
        for (int j = 0; j < R; ++j)
          e[j] = apply_sign(s_t[j][(w.a[j] * o + w.b[j]) & (kTile - 1)], w.sign[j][o >> 5], o);
        if (e0 + o < n) out[e0 + o] = median<R>(e);
      }
    }
  }
}

// first: S-bar starts at fp32(w_0 S_0); otherwise it continues from the value stored in table (a chained launch)
__global__ __launch_bounds__(kST) void sketch_fold_kernel(SketchPack pk, int nrec, int64_t cells, int first, float rho,
                                                          float* table, float* u, float* v) {
  const int64_t i = ((int64_t)blockIdx.x * kST + threadIdx.x) * 4;
  if (i >= cells) return;
  float4 s = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(table + i);
  s = fold4(pk, nrec, i, !first, s);
  if (!u) {
    *reinterpret_cast<float4*>(table + i) = s;
    return;
  }
  float4 a = *reinterpret_cast<const float4*>(u + i);
  a = make_float4(fmaf(rho, a.x, s.x), fmaf(rho, a.y, s.y), fmaf(rho, a.z, s.z), fmaf(rho, a.w, s.w));
  *reinterpret_cast<float4*>(u + i) = a;
  if (v) {
    const float4 b = *reinterpret_cast<const float4*>(v + i);
    *reinterpret_cast<float4*>(v + i) = make_float4(b.x + a.x, b.y + a.y, b.z + a.z, b.w + a.w);
  }
}

// cell_j(i) within row j's cols cells, and whether s_j(i) is -1
__device__ __forceinline__ uint32_t sketch_cell(int64_t i, int j, int64_t cols, uint64_t seed, bool* neg) {
  const uint32_t NT = (uint32_t)(cols / kTile);
  const int64_t q = i / cols, g = i / kTile;
  const uint32_t p = (uint32_t)((i % cols) / kTile), o = (uint32_t)(i % kTile);
  const U4 m = philox_group((uint64_t)q, seed, kCtrMap);
  const uint32_t A = (m.x | 1u) & (NT - 1);  // (NT == 1: 0, and tau = 0 below)
  const uint32_t tau = (inv_odd(A | 1u) * (p - m.y)) & (NT - 1);
  const U4 r = philox_group((uint64_t)g, seed, kCtrPerm + (uint64_t)j);
  const U4 s = philox_group((uint64_t)(i >> 7), seed, kCtrSign + (uint64_t)j);
  *neg = (pick(s, (int)((i >> 5) & 3)) >> (i & 31)) & 1u;
  return tau * kTile + ((((r.x | 1u) & (kTile - 1)) * o + r.y) & (kTile - 1));
}

// one thread per (index, row): cells_out[e * rows + j] = cell | sign bit (31), and / or u, v cleared there
__global__ __launch_bounds__(kST) void sketch_cells_kernel(const int32_t* __restrict__ idx, int64_t k, int64_t n,
                                                           int rows, int64_t cols, uint64_t seed,
                                                           uint32_t* __restrict__ cells_out, float* u, float* v) {
  const int64_t id = (int64_t)blockIdx.x * kST + threadIdx.x;
  if (id >= k * rows) return;
  const int64_t e = id / rows;
  const int j = (int)(id - e * rows);
  const int64_t i = idx[e];
  if (i < 0 || i >= n) return;  // (an index outside the vector names no cell)
  bool neg;
  const uint32_t cell = sketch_cell(i, j, cols, seed, &neg);
  if (cells_out) cells_out[id] = cell | ((uint32_t)neg << 31);
  if (u) u[j * cols + cell] = 0.0f;
  if (v) v[j * cols + cell] = 0.0f;
}

struct SketchShape {
  int64_t nchunks, cps, ecps;
  int nt, nsplit, esplit;
  size_t bytes;
};

bool table_shape(int rows, int64_t cols) {
  if (rows != 1 && rows != 3 && rows != 5) return false;
  return cols >= (1 << 12) && cols <= (1 << 20) && !(cols & (cols - 1));
}

// The split rule, by (n, cols) alone: a split takes cps = max(kMinCps, ceil(chunks * NT / kTargetBlocks)) chunks.
bool sketch_shape(int64_t n, int rows, int64_t cols, SketchShape* s) {
  if (n < 1 || n >= (int64_t)1 << 31 || !table_shape(rows, cols)) return false;
  s->nt = (int)(cols / kTile);
  s->nchunks = cdiv(n, cols);
  s->cps = std::max<int64_t>(kMinCps, cdiv(s->nchunks * s->nt, kTargetBlocks));
  s->nsplit = (int)cdiv(s->nchunks, s->cps);
  s->ecps = std::max<int64_t>(kEstMinCps, cdiv(s->nchunks * s->nt, kTargetBlocks));
  s->esplit = (int)cdiv(s->nchunks, s->ecps);
  s->bytes = align_up((size_t)rows * cols * sizeof(float), 256);
  return true;
}

int check_sketch_shape(const char* fn, int64_t n, int rows, int64_t cols, SketchShape* s) {
  if (n < 1 || n >= (int64_t)1 << 31) return fail(FLC_EINVAL, "%s: n must be in [1, 2^31)", fn);
  if (!sketch_shape(n, rows, cols, s))
    return fail(FLC_EINVAL, "%s: rows %d must be 1, 3 or 5 and cols %lld a power of two in [2^12, 2^20]", fn, rows,
                (long long)cols);
  return FLC_OK;
}

int check_table_shape(const char* fn, int rows, int64_t cols) {
  if (!table_shape(rows, cols))
    return fail(FLC_EINVAL, "%s: rows %d must be 1, 3 or 5 and cols %lld a power of two in [2^12, 2^20]", fn, rows,
                (long long)cols);
  return FLC_OK;
}

int fill_pack(const char* fn, const void* const* records, const float* weights, int n_records, SketchPack* pk) {
  if (!records || !weights || n_records < 1) return fail(FLC_EINVAL, "%s: null records or weights, or no record", fn);
  if (n_records > kSMaxRec)
    return fail(FLC_EINVAL, "%s: %d records (at most %d per call: fold a longer round with flc_sketch_fold first)", fn,
                n_records, kSMaxRec);
  for (int c = 0; c < n_records; ++c) {
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
    pk->rec[c] = static_cast<const float*>(records[c]);
    pk->w[c] = weights[c];
  }
  return FLC_OK;
}

#define FLC_SKETCH_ROWS(rows, X) \
  switch (rows) {                \
    case 1: X(1); break;         \
    case 3: X(3); break;         \
    default: X(5); break;        \
  }

int launch_estimate(const SketchShape& s, const SketchPack& pk, int nrec, int64_t n, int rows, int64_t cols,
                    uint64_t seed, float* out, hipStream_t st) {
  const dim3 grid((unsigned)s.nt, (unsigned)s.esplit);
#define X(R)                                                                                                     \
  FLC_LAUNCH("sketch_estimate", (sketch_estimate_kernel<R>), grid, dim3(kST), 0, st, pk, nrec, n, cols, s.nchunks, \
             s.ecps, seed, out)
  FLC_SKETCH_ROWS(rows, X)
#undef X
  return FLC_OK;
}

}  // namespace
}  // namespace flc

using namespace flc;

extern "C" {

size_t flc_sketch_wire_layout(int64_t n, int rows, int64_t cols, int64_t* offsets) {
  SketchShape s;
  if (!sketch_shape(n, rows, cols, &s)) return 0;
  if (offsets) offsets[0] = 0;
  return s.bytes;
}

int flc_sketch_splits(int64_t n, int64_t cols) {
  SketchShape s;
  return sketch_shape(n, 1, cols, &s) ? s.nsplit : 0;
}

size_t flc_sketch_workspace_size(int64_t n, int rows, int64_t cols) {
  SketchShape s;
  if (!sketch_shape(n, rows, cols, &s)) return 0;
  return s.nsplit > 1 ? align_up((size_t)s.nsplit * rows * cols * sizeof(float), 256) : 256;
}

int flc_sketch_encode(const float* x, int64_t n, int rows, int64_t cols, uint64_t seed, void* record, float* out,
                      void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "flc_sketch_encode";
  if (!x || !record) return fail(FLC_EINVAL, "%s: null x or record", fn);
  SketchShape s;
  if (int rc = check_sketch_shape(fn, n, rows, cols, &s)) return rc;
  if (!aligned16(x) || !aligned16(record) || !aligned16(out))
    return fail(FLC_EINVAL, "%s: x, record and out must be 16-B aligned", fn);
  const size_t need = flc_sketch_workspace_size(n, rows, cols);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255u))
    return fail(FLC_EINVAL, "%s: workspace %zu < %zu (or null, or not 256-B aligned)", fn, ws_bytes, need);
  hipStream_t st = as_stream(stream);
  float* rec = static_cast<float*>(record);
  float* part = s.nsplit > 1 ? static_cast<float*>(ws) : rec;
  const dim3 grid((unsigned)s.nt, (unsigned)s.nsplit);
#define X(R) \
  FLC_LAUNCH("sketch_pass", (sketch_pass_kernel<R>), grid, dim3(kST), 0, st, x, n, cols, s.nchunks, s.cps, seed, part)
  FLC_SKETCH_ROWS(rows, X)
#undef X
  if (s.nsplit > 1) {
    const int64_t cells = (int64_t)rows * cols;
    FLC_LAUNCH("sketch_finish", sketch_finish_kernel, dim3((unsigned)cdiv(cells, kST)), dim3(kST), 0, st,
               (const float*)part, cells, s.nsplit, rec);
  }
  if (out) {
    SketchPack pk = {};
    pk.rec[0] = rec;
    pk.w[0] = 1.0f;
    return launch_estimate(s, pk, 1, n, rows, cols, seed, out, st);
  }
  return FLC_OK;
}

int flc_sketch_estimate(const void* const* records, const float* weights, int n_records, int64_t n, int rows,
                        int64_t cols, uint64_t seed, float* out, void* stream) {
  const char* fn = "flc_sketch_estimate";
  if (!out || !aligned16(out)) return fail(FLC_EINVAL, "%s: out is null or not 16-B aligned", fn);
  SketchShape s;
  if (int rc = check_sketch_shape(fn, n, rows, cols, &s)) return rc;
  SketchPack pk = {};
  if (int rc = fill_pack(fn, records, weights, n_records, &pk)) return rc;
  return launch_estimate(s, pk, n_records, n, rows, cols, seed, out, as_stream(stream));
}

int flc_sketch_fold(const void* const* records, const float* weights, int n_records, int rows, int64_t cols,
                    float* table, void* stream) {
  const char* fn = "flc_sketch_fold";
  if (!records || !weights || n_records < 1) return fail(FLC_EINVAL, "%s: null records or weights, or no record", fn);
  if (!table || !aligned16(table)) return fail(FLC_EINVAL, "%s: table is null or not 16-B aligned", fn);
  if (int rc = check_table_shape(fn, rows, cols)) return rc;
  for (int c = 0; c < n_records; ++c)
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
  const int64_t cells = (int64_t)rows * cols;
  hipStream_t st = as_stream(stream);
  for (int c0 = 0; c0 < n_records; c0 += kSMaxRec) {  // launches chain, each continuing from the stored S-bar
    const int nc = std::min(kSMaxRec, n_records - c0);
    SketchPack pk = {};
    if (int rc = fill_pack(fn, records + c0, weights + c0, nc, &pk)) return rc;
    FLC_LAUNCH("sketch_fold", sketch_fold_kernel, dim3((unsigned)cdiv(cells / 4, kST)), dim3(kST), 0, st, pk, nc,
               cells, c0 == 0 ? 1 : 0, 0.0f, table, (float*)nullptr, (float*)nullptr);
  }
  return FLC_OK;
}

int flc_sketch_state_step(const void* const* records, const float* weights, int n_records, int rows, int64_t cols,
                          float rho, float* u, float* v, void* stream) {
  const char* fn = "flc_sketch_state_step";
  if (!u || !aligned16(u) || !aligned16(v)) return fail(FLC_EINVAL, "%s: u is null, or u or v not 16-B aligned", fn);
  if (int rc = check_table_shape(fn, rows, cols)) return rc;
  SketchPack pk = {};
  if (int rc = fill_pack(fn, records, weights, n_records, &pk)) return rc;
  const int64_t cells = (int64_t)rows * cols;
  FLC_LAUNCH("sketch_state_step", sketch_fold_kernel, dim3((unsigned)cdiv(cells / 4, kST)), dim3(kST), 0,
             as_stream(stream), pk, n_records, cells, 1, rho, (float*)nullptr, u, v);
  return FLC_OK;
}

static int cells_launch(const char* fn, const int32_t* idx, int64_t k, int64_t n, int rows, int64_t cols,
                        uint64_t seed, uint32_t* cells, float* u, float* v, void* stream) {
  if (!idx || k < 0) return fail(FLC_EINVAL, "%s: null idx or k < 0", fn);
  SketchShape s;
  if (int rc = check_sketch_shape(fn, n, rows, cols, &s)) return rc;
  if (k == 0) return FLC_OK;
  FLC_LAUNCH("sketch_cells", sketch_cells_kernel, dim3((unsigned)cdiv(k * rows, kST)), dim3(kST), 0,
             as_stream(stream), idx, k, n, rows, cols, seed, cells, u, v);
  return FLC_OK;
}

int flc_sketch_clear(const int32_t* idx, int64_t k, int64_t n, int rows, int64_t cols, uint64_t seed, float* u,
                     float* v, void* stream) {
  if (!u && !v) return fail(FLC_EINVAL, "flc_sketch_clear: neither u nor v");
  return cells_launch("flc_sketch_clear", idx, k, n, rows, cols, seed, nullptr, u, v, stream);
}

int flc_sketch_cells(const int32_t* idx, int64_t k, int64_t n, int rows, int64_t cols, uint64_t seed, uint32_t* cells,
                     void* stream) {
  if (!cells) return fail(FLC_EINVAL, "flc_sketch_cells: null cells");
  return cells_launch("flc_sketch_cells", idx, k, n, rows, cols, seed, cells, nullptr, nullptr, stream);
}

}  // extern "C"
