// lowrank.hip — the low-rank (PowerSGD, Vogels et al. 2019) compressor: one power iteration with a CholeskyQR
// orthonormalisation, its record, its decode / residual and the MFMA fold of a round's records.  gfx950 only.
//
// The flat fp32 vector x (n elements) is the row-major matrix M of m = ceil(n / cols) rows and cols columns (elements
// at and past n read as +0).  With Q (cols x r) given:
//   P = M Q;  G = P^T P (fp64);  G = L L^T (fp64 Cholesky, column k dropped when G_kk == 0 or its pivot
//   d_k <= 2^-40 G_kk);  W = L^-1;  P^ = P W^T;  Q' = (M^T P) W^T;  decoded = P^ Q'^T;  q_next = Q' with every dropped
//   column replaced by Q's.
// Record (flc_lowrank_wire_layout): P^ as [m][r] fp32 at 0, Q' as [cols][r] fp32 from the next 16-B boundary, padded
// to 256 B.
//
// lowrank_pass_kernel     reads x ONCE.  A wave owns whole rows (cols / 64 floats per lane as 16-B words: lane l's word
//                         v holds columns 256 v + 4 l .. + 3).  Q sits in LDS, lane-contiguous per (word, component) so
//                         the reads have no bank conflict.  Per row: the lane's chain over its columns (word, then
//                         component, ascending, fmaf from 0), the xor butterfly (1, 2, 4, ..., 32) -> P[i], stored by
//                         lane 0; then, the row still in registers, T[j] = fmaf(x_ij, P[i], T[j]) in the lane's
//                         accumulators and G += P[i]^T P[i] in fp64.  A panel is one block: 4 waves x rpw consecutive
//                         rows each (rpw = 1, 2, 4, 8 by m alone).  At the end the waves' T are added through LDS in
//                         wave order ((w0 + w1) + w2) + w3, G likewise from 0.0, and the panel's partials go to the
//                         workspace.  No atomics.
// lowrank_finish_kernel   every block folds the G partials itself (16 chains, chain c over panels c, c + 16, ...
//                         ascending from 0.0, then the chains in order from 0.0), thread 0 runs the fp64 Cholesky and
//                         forms W.  The first cols / 16 blocks reduce T for 16 columns each (fp64, the same 16-chain
//                         order) and write Q' = T W^T and q_next; the others rescale P -> P^ in place, 1024 rows each.
// lowrank_decode_kernel   Q' in LDS -> registers, the row's P^ wave-uniform, v = P^_0 Q'_0, then fmaf(P^_k, Q'_k, v)
//                         for k ascending; out = acc ? fmaf(w, v, out) : w v;  residual = fp32(x - v).
// lowrank_fold_kernel     out (+)= sum_c sum_k fp32(w_c P^_c[i,k]) Q'_c[j,k] on v_mfma_f32_32x32x2_f32 with the
//                         transposed tile: A = Q' (the instruction's M = output columns), B = the weighted P^ (N =
//                         output rows), so a lane's accumulator group of four is four consecutive columns of one
//                         output row: one 16-B store.  A wave owns 32 rows x 128 columns (four 32 x 32 tiles, 64
//                         accumulator registers); the inner dimension K = C r runs records ascending, k ascending, two
//                         per instruction, an odd K padded with a zero operand; the sum starts from +0 and the stored
//                         value (accumulate) is added last, in one rounding.  The operands are read straight from
//                         L2 (4-B loads: they are (m + cols) r C floats in all and every record's Q' is shared by all
//                         waves).
#include <algorithm>

#include "flc_device.hpp"
#include "flc_runtime.hpp"

namespace flc {
namespace {

constexpr int kLT = 256;           // threads per block
constexpr int kLNW = kLT / kWave;  // waves per block
constexpr int kLChains = 16;       // chains of the partial folds
constexpr int kLFinishRows = 1024; // rows a rescaling block of the finish takes
constexpr int kLFoldMax = 64;      // records per fold launch

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int R> struct VecR;
template <> struct VecR<1> { typedef float T; };
template <> struct VecR<2> { typedef float2 T; };
template <> struct VecR<4> { typedef float4 T; };
template <int R>
__device__ __forceinline__ void ldv(const float* p, float (&o)[R]) {
  const typename VecR<R>::T v = *reinterpret_cast<const typename VecR<R>::T*>(p);
  __builtin_memcpy(o, &v, sizeof(v));
}
template <int R>
__device__ __forceinline__ void stv(float* p, const float (&o)[R]) {
  typename VecR<R>::T v;
  __builtin_memcpy(&v, o, sizeof(v));
  *reinterpret_cast<typename VecR<R>::T*>(p) = v;
}

// the lane-contiguous order of a row's columns: slot = 256 v + 64 c + lane for column 256 v + 4 lane + c
__device__ __forceinline__ int col_slot(int j) { return (j & ~255) + (j & 3) * 64 + ((j >> 2) & 63); }
__device__ __forceinline__ int slot_col(int s) { return (s & ~255) + (s & 63) * 4 + ((s >> 6) & 3); }

// rows per wave of the pass, by m alone: at least 256 panels from 1024 rows up, a T partial per >= 32 rows when large
inline int rows_per_wave(int64_t m) { return m <= 2048 ? 1 : m <= 4096 ? 2 : m <= 8192 ? 4 : 8; }

// one row of M into registers; the tail row element by element, +0 past n
template <int NV>
__device__ __forceinline__ void load_row(const float* x, int64_t e0, int64_t n, int lane, float (&xv)[NV][4]) {
  if (e0 + NV * 256 <= n) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float4 a = *reinterpret_cast<const float4*>(x + e0 + v * 256 + lane * 4);
      xv[v][0] = a.x; xv[v][1] = a.y; xv[v][2] = a.z; xv[v][3] = a.w;
    }
  } else {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t e = e0 + v * 256 + lane * 4 + c;
        xv[v][c] = e < n ? x[e] : 0.0f;
      }
  }
}

template <int COLS, int R>
__global__ __launch_bounds__(kLT) void lowrank_pass_kernel(const float* __restrict__ x, int64_t n, int m, int rpw,
                                                           const float* __restrict__ q, float* __restrict__ p_out,
                                                           float* __restrict__ t_part, double* __restrict__ g_part) {
  constexpr int NV = COLS / 256;
  __shared__ __attribute__((aligned(16))) float s_q[COLS * R];  // Q by slot; at the end the block's T by slot
  __shared__ double s_g[kLNW][R * R];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < COLS; j += kLT) {
    float t[R];
    ldv<R>(q + j * R, t);
    stv<R>(s_q + col_slot(j) * R, t);
  }
  __syncthreads();

  float t[NV][4][R];
  double g[R][R];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int k = 0; k < R; ++k) t[v][c][k] = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int l = 0; l < R; ++l) g[k][l] = 0.0;

  const int row0 = (blockIdx.x * kLNW + wave) * rpw;
  for (int rr = 0; rr < rpw; ++rr) {
    const int i = row0 + rr;
    if (i >= m) break;  // (wave-uniform)
    float xv[NV][4], p[R];
    load_row<NV>(x, (int64_t)i * COLS, n, lane, xv);
#pragma unroll
    for (int k = 0; k < R; ++k) p[k] = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float qv[R];
        ldv<R>(s_q + (v * 256 + c * 64 + lane) * R, qv);
#pragma unroll
        for (int k = 0; k < R; ++k) p[k] = fmaf(xv[v][c], qv[k], p[k]);
      }
#pragma unroll
    for (int k = 0; k < R; ++k)
      for (int o = 1; o < kWave; o <<= 1) p[k] += __shfl_xor(p[k], o, kWave);
    if (lane == 0) stv<R>(p_out + (int64_t)i * R, p);
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < R; ++k) t[v][c][k] = fmaf(xv[v][c], p[k], t[v][c][k]);
#pragma unroll
    for (int k = 0; k < R; ++k)
#pragma unroll
      for (int l = k; l < R; ++l) g[k][l] += (double)p[k] * (double)p[l];
  }

  // the panel's partials: the waves' T through LDS in wave order, G from 0.0 in wave order
  __syncthreads();  // (every wave has read Q for the last time)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < R; ++k)
#pragma unroll
      for (int l = 0; l < R; ++l) s_g[wave][k * R + l] = k <= l ? g[k][l] : g[l][k];
  }
  for (int w = 0; w < kLNW; ++w) {
    if (wave == w) {
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float* sp = s_q + (v * 256 + c * 64 + lane) * R;
          if (w > 0) {
            float a[R];
            ldv<R>(sp, a);
#pragma unroll
            for (int k = 0; k < R; ++k) t[v][c][k] = a[k] + t[v][c][k];
          }
          stv<R>(sp, t[v][c]);
        }
    }
    __syncthreads();
  }
  float4* dst = reinterpret_cast<float4*>(t_part + (int64_t)blockIdx.x * (COLS * R));
  for (int i = threadIdx.x; i < COLS * R / 4; i += kLT) dst[i] = reinterpret_cast<const float4*>(s_q)[i];
  if (threadIdx.x < R * R) {
    double s = 0.0;
    for (int w = 0; w < kLNW; ++w) s += s_g[w][threadIdx.x];
    g_part[(int64_t)blockIdx.x * (R * R) + threadIdx.x] = s;
  }
}

// W = L^-1 of G = L L^T with the drop rule (thread 0, fp64); w: [R][R] row-major, lower triangular
template <int R>
__device__ __forceinline__ void cholesky_inverse(const double (&G)[R][R], double* w, int* drop) {
  double L[R][R], W[R][R];
  bool dr[R];
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int l = 0; l < R; ++l) L[k][l] = W[k][l] = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    double d = G[k][k];
#pragma unroll
    for (int l = 0; l < k; ++l) d -= L[k][l] * L[k][l];
    dr[k] = G[k][k] == 0.0 || d <= 0x1p-40 * G[k][k];
    if (dr[k]) continue;  // (column k of L stays 0: it adds nothing to later columns)
    L[k][k] = sqrt(d);
#pragma unroll
    for (int i = k + 1; i < R; ++i) {
      double s = G[i][k];
#pragma unroll
      for (int l = 0; l < k; ++l) s -= L[i][l] * L[k][l];
      L[i][k] = s / L[k][k];
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    if (dr[k]) continue;
    W[k][k] = 1.0 / L[k][k];
#pragma unroll
    for (int l = 0; l < k; ++l) {
      double s = 0.0;
#pragma unroll
      for (int u = l; u < k; ++u) s += L[k][u] * W[u][l];
      W[k][l] = -s / L[k][k];
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    drop[k] = dr[k];
#pragma unroll
    for (int l = 0; l < R; ++l) w[k * R + l] = W[k][l];
  }
}

// o[k] = fp32(sum_{l <= k} a[l] W[k][l]) in fp64, l ascending from 0.0
template <int R>
__device__ __forceinline__ void apply_w(const double (&a)[R], const double* w, float (&o)[R]) {
#pragma unroll
  for (int k = 0; k < R; ++k) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l <= k; ++l) s += a[l] * w[k * R + l];
    o[k] = (float)s;
  }
}

template <int R>
__global__ __launch_bounds__(kLT) void lowrank_finish_kernel(int cols, int m, int npanels,
                                                             const float* __restrict__ t_part,
                                                             const double* __restrict__ g_part, const float* q_in,
                                                             float* __restrict__ p_io, float* __restrict__ q_out,
                                                             float* q_next) {
  __shared__ double s_c[kLChains][R * R];
  __shared__ double s_w[R * R];
  __shared__ int s_drop[R];
  __shared__ double s_t[kLChains][16][R];
  const int tid = threadIdx.x;
  if (tid < kLChains * R * R) {
    const int chain = tid / (R * R), e = tid % (R * R);
    double a = 0.0;
    for (int p = chain; p < npanels; p += kLChains) a += g_part[(int64_t)p * (R * R) + e];
    s_c[chain][e] = a;
  }
  __syncthreads();
  if (tid < R * R) {
    double a = 0.0;
    for (int c = 0; c < kLChains; ++c) a += s_c[c][tid];
    s_w[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    double G[R][R];
#pragma unroll
    for (int k = 0; k < R; ++k)
#pragma unroll
      for (int l = 0; l < R; ++l) G[k][l] = s_w[k * R + l];
    cholesky_inverse<R>(G, s_w, s_drop);
  }
  __syncthreads();

  const int nqb = cols / 16;
  if ((int)blockIdx.x < nqb) {  // Q' and q_next of 16 slots
    const int chain = tid >> 4, sl = tid & 15, s = blockIdx.x * 16 + sl;
    double a[R];
#pragma unroll
    for (int k = 0; k < R; ++k) a[k] = 0.0;
    for (int p = chain; p < npanels; p += kLChains) {
      float tv[R];
      ldv<R>(t_part + ((int64_t)p * cols + s) * R, tv);
#pragma unroll
      for (int k = 0; k < R; ++k) a[k] += (double)tv[k];
    }
#pragma unroll
    for (int k = 0; k < R; ++k) s_t[chain][sl][k] = a[k];
    __syncthreads();
    if (tid < 16) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        double b = 0.0;
        for (int c = 0; c < kLChains; ++c) b += s_t[c][tid][k];
        a[k] = b;
      }
      float o[R];
      apply_w<R>(a, s_w, o);
      const int j = slot_col(blockIdx.x * 16 + tid);
      stv<R>(q_out + j * R, o);
      if (q_next) {
        float qi[R];
        ldv<R>(q_in + j * R, qi);
#pragma unroll
        for (int k = 0; k < R; ++k) qi[k] = s_drop[k] ? qi[k] : o[k];
        stv<R>(q_next + j * R, qi);
      }
    }
    return;
  }
  const int r0 = ((int)blockIdx.x - nqb) * kLFinishRows;  // P -> P^ in place
  for (int i = r0 + tid; i < r0 + kLFinishRows && i < m; i += kLT) {
    float pv[R], o[R];
    double a[R];
    ldv<R>(p_io + (int64_t)i * R, pv);
#pragma unroll
    for (int k = 0; k < R; ++k) a[k] = (double)pv[k];
    apply_w<R>(a, s_w, o);
    stv<R>(p_io + (int64_t)i * R, o);
  }
}

// out / x / residual may alias each other (the error memory updated in place): a lane reads its elements before it
// writes them
template <int COLS, int R>
__global__ __launch_bounds__(kLT) void lowrank_decode_kernel(const float* __restrict__ ph, const float* __restrict__ qp,
                                                             int64_t n, int m, float w, int acc, float* out,
                                                             const float* x, float* residual) {
  constexpr int NV = COLS / 256;
  __shared__ __attribute__((aligned(16))) float s_q[COLS * R];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < COLS; j += kLT) {
    float t[R];
    ldv<R>(qp + j * R, t);
    stv<R>(s_q + col_slot(j) * R, t);
  }
  __syncthreads();
  float qr[NV][4][R];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) ldv<R>(s_q + (v * 256 + c * 64 + lane) * R, qr[v][c]);

  for (int row = blockIdx.x * kLNW + wave; row < m; row += gridDim.x * kLNW) {
    const int i = __builtin_amdgcn_readfirstlane(row);
    float p[R];
#pragma unroll
    for (int k = 0; k < R; ++k) p[k] = ph[(int64_t)i * R + k];
    float val[NV][4];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = p[0] * qr[v][c][0];
#pragma unroll
        for (int k = 1; k < R; ++k) s = fmaf(p[k], qr[v][c][k], s);
        val[v][c] = s;
      }
    const int64_t e0 = (int64_t)i * COLS;
    const bool full = e0 + COLS <= n;
    if (residual) {
      float xv[NV][4];
      load_row<NV>(x, e0, n, lane, xv);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int64_t e = e0 + v * 256 + lane * 4;
        if (full) {
          *reinterpret_cast<float4*>(residual + e) =
              make_float4(xv[v][0] - val[v][0], xv[v][1] - val[v][1], xv[v][2] - val[v][2], xv[v][3] - val[v][3]);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (e + c < n) residual[e + c] = xv[v][c] - val[v][c];
        }
      }
    }
    if (out) {
      float o[NV][4];
      if (acc) {
        load_row<NV>(out, e0, n, lane, o);
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int c = 0; c < 4; ++c) o[v][c] = fmaf(w, val[v][c], o[v][c]);
      } else {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int c = 0; c < 4; ++c) o[v][c] = w * val[v][c];
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int64_t e = e0 + v * 256 + lane * 4;
        if (full) {
          *reinterpret_cast<float4*>(out + e) = make_float4(o[v][0], o[v][1], o[v][2], o[v][3]);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (e + c < n) out[e + c] = o[v][c];
        }
      }
    }
  }
}

struct LowrankPack {
  const char* rec[kLFoldMax];
  float w[kLFoldMax];
};

// A wave: output rows 32 rg .. + 31 (the instruction's N, lane & 31), columns 128 cg .. + 127 as four tiles (the
// instruction's M).  Step s of the inner dimension takes the global indices 2 s and 2 s + 1 (lane >> 5), index kk
// being (record kk / R, component kk % R).  Accumulator register v of tile t: column 32 t + 8 (v / 4) + 4 (lane >> 5)
// + v % 4 of row lane & 31.
template <int R>
__global__ __launch_bounds__(kLT) void lowrank_fold_kernel(LowrankPack pk, int nrec, int64_t n, int cols, int m,
                                                           int64_t offq, int acc, float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int cgs = cols >> 7;
  const int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kLNW + wave);
  const int rg = tile / cgs, cg = tile - rg * cgs;
  if (rg * 32 >= m) return;  // (wave-uniform; the kernel has no barrier)
  const int half = lane >> 5, l32 = lane & 31;
  const int row = rg * 32 + l32, j0 = cg * 128;
  const bool row_ok = row < m;
  const int64_t erow = (int64_t)row * cols + j0 + 4 * half;

  f32x16 d[4];  // the sum of the launch's terms from +0; the stored value is added last, in one rounding
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) d[t][v] = 0.0f;

  const int K = nrec * R;
  for (int s = 0; 2 * s < K; ++s) {
    const char* rec;
    float wc;
    int k;
    bool ok = true;
    if constexpr (R == 1) {  // the two halves read two records; an odd K ends on a zero operand
      const int ca = 2 * s, cb = 2 * s + 1 < nrec ? 2 * s + 1 : ca;
      rec = half ? pk.rec[cb] : pk.rec[ca];
      wc = half ? pk.w[cb] : pk.w[ca];
      k = 0;
      ok = 2 * s + half < nrec;
    } else {
      const int c = 2 * s / R;
      rec = pk.rec[c];
      wc = pk.w[c];
      k = 2 * s % R + half;
    }
    const float* ph = reinterpret_cast<const float*>(rec);
    const float* qp = reinterpret_cast<const float*>(rec + offq);
    const float b = ok && row_ok ? wc * ph[(int64_t)row * R + k] : 0.0f;
    float a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = ok ? qp[(j0 + t * 32 + l32) * R + k] : 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) d[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b, d[t], 0, 0, 0);
  }

  if (!row_ok) return;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int64_t e = erow + t * 32 + gq * 8;
      if (e + 4 <= n) {
        float4 o = make_float4(d[t][gq * 4 + 0], d[t][gq * 4 + 1], d[t][gq * 4 + 2], d[t][gq * 4 + 3]);
        if (acc) {
          const float4 a = *reinterpret_cast<const float4*>(out + e);
          o = make_float4(a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w);
        }
        *reinterpret_cast<float4*>(out + e) = o;
      } else {
#pragma unroll
        for (int u = 0; u < 3; ++u)
          if (e + u < n) out[e + u] = acc ? out[e + u] + d[t][gq * 4 + u] : d[t][gq * 4 + u];
      }
    }
}

struct LowrankShape {
  int m, npanels, rpw;
  int64_t offq;
  size_t bytes;
};

bool lowrank_shape(int64_t n, int64_t cols, int rank, LowrankShape* s) {
  if (n < 1 || n >= (int64_t)1 << 31) return false;
  if (cols != 256 && cols != 512 && cols != 1024) return false;
  if (rank != 1 && rank != 2 && rank != 4) return false;
  const int64_t m = cdiv(n, cols);
  s->m = (int)m;
  s->rpw = rows_per_wave(m);
  s->npanels = (int)cdiv(m, (int64_t)kLNW * s->rpw);
  s->offq = (int64_t)align_up((size_t)m * rank * sizeof(float), 16);
  s->bytes = align_up((size_t)s->offq + (size_t)cols * rank * sizeof(float), 256);
  return true;
}

int check_lowrank_shape(const char* fn, int64_t n, int64_t cols, int rank, LowrankShape* s) {
  if (n < 1 || n >= (int64_t)1 << 31) return fail(FLC_EINVAL, "%s: n must be in [1, 2^31)", fn);
  if (!lowrank_shape(n, cols, rank, s))
    return fail(FLC_EINVAL, "%s: cols %lld must be 256, 512 or 1024 and rank %d one of 1, 2, 4", fn, (long long)cols,
                rank);
  return FLC_OK;
}

// the kernel instance of a (cols, rank): X(COLS, R) in a function that returns int
#define FLC_LOWRANK_DISPATCH(cols, rank, X)                     \
  switch ((int)(cols) * 8 + (rank)) {                           \
    case 256 * 8 + 1: X(256, 1); break;                         \
    case 256 * 8 + 2: X(256, 2); break;                         \
    case 256 * 8 + 4: X(256, 4); break;                         \
    case 512 * 8 + 1: X(512, 1); break;                         \
    case 512 * 8 + 2: X(512, 2); break;                         \
    case 512 * 8 + 4: X(512, 4); break;                         \
    case 1024 * 8 + 1: X(1024, 1); break;                       \
    case 1024 * 8 + 2: X(1024, 2); break;                       \
    default: X(1024, 4); break;                                 \
  }

int launch_decode(const LowrankShape& s, const char* record, int64_t n, int64_t cols, int rank, float w, int acc,
                  float* out, const float* x, float* residual, hipStream_t st) {
  const float* ph = reinterpret_cast<const float*>(record);
  const float* qp = reinterpret_cast<const float*>(record + s.offq);
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(s.m, kLNW), 1024);
#define X(C, R)                                                                                                      \
  FLC_LAUNCH("lowrank_decode", (lowrank_decode_kernel<C, R>), dim3(grid), dim3(kLT), 0, st, ph, qp, n, s.m, w, acc, \
             out, x, residual)
  FLC_LOWRANK_DISPATCH(cols, rank, X)
#undef X
  return FLC_OK;
}

}  // namespace
}  // namespace flc

using namespace flc;

extern "C" {

size_t flc_lowrank_wire_layout(int64_t n, int64_t cols, int rank, int64_t* offsets) {
  LowrankShape s;
  if (!lowrank_shape(n, cols, rank, &s)) return 0;
  if (offsets) {
    offsets[0] = 0;
    offsets[1] = s.offq;
  }
  return s.bytes;
}

size_t flc_lowrank_workspace_size(int64_t n, int64_t cols, int rank) {
  LowrankShape s;
  if (!lowrank_shape(n, cols, rank, &s)) return 0;
  return align_up((size_t)s.npanels * cols * rank * sizeof(float), 256) +
         align_up((size_t)s.npanels * rank * rank * sizeof(double), 256);
}

int flc_lowrank_encode(const float* x, int64_t n, int64_t cols, int rank, const float* q, void* record, float* q_next,
                       float* out, float* residual, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "flc_lowrank_encode";
  if (!x || !q || !record) return fail(FLC_EINVAL, "%s: null x, q or record", fn);
  LowrankShape s;
  if (int rc = check_lowrank_shape(fn, n, cols, rank, &s)) return rc;
  if (!aligned16(x) || !aligned16(q) || !aligned16(record) || !aligned16(q_next) || !aligned16(out) ||
      !aligned16(residual))
    return fail(FLC_EINVAL, "%s: x, q, record, q_next, out and residual must be 16-B aligned", fn);
  const size_t need = flc_lowrank_workspace_size(n, cols, rank);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255u))
    return fail(FLC_EINVAL, "%s: workspace %zu < %zu (or null, or not 256-B aligned)", fn, ws_bytes, need);
  hipStream_t st = as_stream(stream);
  Carver cv(ws, ws_bytes);
  float* t_part = cv.take<float>((size_t)s.npanels * cols * rank);
  double* g_part = cv.take<double>((size_t)s.npanels * rank * rank);
  char* rec = static_cast<char*>(record);
  float* ph = reinterpret_cast<float*>(rec);
  float* qp = reinterpret_cast<float*>(rec + s.offq);
#define X(C, R)                                                                                                   \
  FLC_LAUNCH("lowrank_pass", (lowrank_pass_kernel<C, R>), dim3(s.npanels), dim3(kLT), 0, st, x, n, s.m, s.rpw, q, \
             ph, t_part, g_part)
  FLC_LOWRANK_DISPATCH(cols, rank, X)
#undef X
  const unsigned grid2 = (unsigned)(cols / 16 + cdiv(s.m, kLFinishRows));
#define X(C, R)                                                                                                      \
  FLC_LAUNCH("lowrank_finish", (lowrank_finish_kernel<R>), dim3(grid2), dim3(kLT), 0, st, (int)cols, s.m, s.npanels, \
             (const float*)t_part, (const double*)g_part, q, ph, qp, q_next)
  FLC_LOWRANK_DISPATCH(cols, rank, X)
#undef X
  if (out || residual) return launch_decode(s, rec, n, cols, rank, 1.0f, 0, out, x, residual, st);
  return FLC_OK;
}

int flc_lowrank_decode(const void* record, int64_t n, int64_t cols, int rank, float weight, int accumulate, float* out,
                       const float* x, float* residual, void* stream) {
  const char* fn = "flc_lowrank_decode";
  if (!record || (!out && !residual) || (residual && !x) || (accumulate && !out))
    return fail(FLC_EINVAL, "%s: null record, neither out nor residual, residual without x, or accumulate without out",
                fn);
  LowrankShape s;
  if (int rc = check_lowrank_shape(fn, n, cols, rank, &s)) return rc;
  if (!aligned16(record) || !aligned16(out) || !aligned16(x) || !aligned16(residual))
    return fail(FLC_EINVAL, "%s: record, out, x and residual must be 16-B aligned", fn);
  return launch_decode(s, static_cast<const char*>(record), n, cols, rank, weight, accumulate ? 1 : 0, out,
                       residual ? x : nullptr, residual, as_stream(stream));
}

int flc_fold_lowrank_records(const void* const* records, const float* weights, int n_records, int64_t n, int64_t cols,
                             int rank, int accumulate, float* out, void* stream) {
  const char* fn = "flc_fold_lowrank_records";
  if (!records || !weights || !out || n_records < 1)
    return fail(FLC_EINVAL, "%s: null records, weights or out, or no record", fn);
  LowrankShape s;
  if (int rc = check_lowrank_shape(fn, n, cols, rank, &s)) return rc;
  if (!aligned16(out)) return fail(FLC_EINVAL, "%s: out must be 16-B aligned", fn);
  for (int c = 0; c < n_records; ++c)
    if (!records[c] || !aligned16(records[c]))
      return fail(FLC_EINVAL, "%s: record %d is null or not 16-B aligned", fn, c);
  hipStream_t st = as_stream(stream);
  const int64_t tiles = cdiv(s.m, 32) * (cols / 128);
  const unsigned grid = (unsigned)cdiv(tiles, kLNW);
  for (int c0 = 0; c0 < n_records; c0 += kLFoldMax) {  // launches chain, each continuing from the stored sums
    const int nc = std::min(kLFoldMax, n_records - c0);
    LowrankPack pk = {};
    for (int c = 0; c < nc; ++c) {
      pk.rec[c] = static_cast<const char*>(records[c0 + c]);
      pk.w[c] = weights[c0 + c];
    }
    const int acc = (c0 > 0 || accumulate) ? 1 : 0;
    switch (rank) {
      case 1:
        FLC_LAUNCH("lowrank_fold", (lowrank_fold_kernel<1>), dim3(grid), dim3(kLT), 0, st, pk, nc, n, (int)cols, s.m,
                   s.offq, acc, out);
        break;
      case 2:
        FLC_LAUNCH("lowrank_fold", (lowrank_fold_kernel<2>), dim3(grid), dim3(kLT), 0, st, pk, nc, n, (int)cols, s.m,
                   s.offq, acc, out);
        break;
      default:
        FLC_LAUNCH("lowrank_fold", (lowrank_fold_kernel<4>), dim3(grid), dim3(kLT), 0, st, pk, nc, n, (int)cols, s.m,
                   s.offq, acc, out);
        break;
    }
  }
  return FLC_OK;
}

}  // extern "C"
