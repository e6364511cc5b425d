// sign.hip — the scaled-sign 1-bit compressor, C(x) = (||x||_1 / d) * sign(x) per bucket (Bernstein et al.'s signSGD
// with the scale of Karimireddy et al.'s EF-signSGD; 1-bit SGD's wire).  gfx950 only.
//
//   scale_b = fp32(S_b / (double)m_b), S_b the fp64 sum of the bucket's fp32 |x| in an order fixed by the bucket size
//             (bucket 0: by n) and the positions, m_b the bucket's true element count (the tail bucket's may be short)
//   bit_i   = the IEEE sign bit of x_i (-0: 1), element i at bit i & 7 of byte i >> 3
//   value   = bit ? -scale_b : scale_b (a zero decodes to +-scale: one bit per element and nothing else)
//
// One pass (sign_encode_kernel): a 512-thread block owns 4096 consecutive elements (the largest bucket), thread t the
// group of 8 at (block * 512 + t) * 8, loaded with two 16-B loads and kept in registers — quant.hip's
// bucket_encode_kernel's split, so a bucket is B / 8 consecutive lanes.  The bits do not depend on the scale: the same
// registers give the lane's byte of the bit stream and its fp64 chain over |x|.
//   bits     every lane's byte goes to its wave's 64 bytes of LDS; after a wave barrier lanes 0..3 of the wave store
//            them as four 16-B words (no byte stores and no atomics reach the stream; no block barrier either).  Lanes
//            past n hold +0: bit 0, so the stream's last 16-B word is zero beyond bit n.
//   S_b      the lane's chain ss = ss + fp64(|v_j|), j = 0..7 from 0.0; an xor butterfly (1, 2, 4, ...: a + b on both
//            partners) over the bucket's min(B / 8, 64) lanes; for B >= 1024 one LDS word per wave, one barrier, and
//            r = 0.0, r += (wave sum) over the bucket's B / 512 waves in wave order.
//   B >= 64  the scale is known in the pass: scales, out (+-scale) and residual (fp32(x - value)) leave from registers.
//   B == 0   (the whole vector) the pass writes the bits and the block's sum (the B = 4096 order) to partials[block];
//            a second launch in the same call (sign_scale_kernel) folds the partials in an order fixed by the block
//            count — thread t the chain over partials t, t + 512, ... ascending, then the butterfly and the waves in
//            order — in every block that needs the scale, so every block gets the same bits; block 0 writes scales[0],
//            and with out / residual the blocks make the elementwise pass over x (grid-stride over 4096-element spans).
//            No grid-wide wait, no ticket, no status word.
#include <algorithm>

#include "flc_device.hpp"
#include "flc_runtime.hpp"

namespace flc {
namespace {

constexpr int kST = 512;             // threads per block
constexpr int kSNW = kST / kWave;    // waves per block
constexpr int kSG = 8;               // elements per thread: one byte of the bit stream
constexpr int kSSpan = kST * kSG;    // elements per block = the largest bucket
constexpr int kScaleGrid = 1024;     // blocks of the whole-vector elementwise pass (each folds the partials once)
static_assert(kSSpan == 4096, "bucket_log2's largest bucket is one block's span");

__device__ __forceinline__ void load8(const float* x, int64_t e0, int valid, float v[kSG]) {
  if (valid == kSG) {
    const float4 a = *reinterpret_cast<const float4*>(x + e0);
    const float4 b = *reinterpret_cast<const float4*>(x + e0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kSG; ++j) v[j] = j < valid ? x[e0 + j] : 0.0f;
  }
}

__device__ __forceinline__ void store8(float* p, int64_t e0, int valid, const float o[kSG]) {
  if (valid == kSG) {
    *reinterpret_cast<float4*>(p + e0) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(p + e0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
  } else {
    for (int j = 0; j < valid; ++j) p[e0 + j] = o[j];
  }
}

__device__ __forceinline__ uint32_t sign_byte(const float v[kSG]) {
  uint32_t b = 0;
#pragma unroll
  for (int j = 0; j < kSG; ++j) b |= (__float_as_uint(v[j]) >> 31) << j;
  return b;
}

// out = +-scale and residual = fp32(x - value) of one group, from the registers that hold x (residual may be x itself:
// the thread has read its elements)
__device__ __forceinline__ void sign_apply(const float v[kSG], float scale, int64_t e0, int valid, float* out,
                                           float* residual) {
  float d[kSG];
#pragma unroll
  for (int j = 0; j < kSG; ++j) d[j] = (__float_as_uint(v[j]) >> 31) ? -scale : scale;
  if (out) store8(out, e0, valid, d);
  if (residual) {
#pragma unroll
    for (int j = 0; j < kSG; ++j) d[j] = v[j] - d[j];
    store8(residual, e0, valid, d);
  }
}

// the block's sum of 512 per-thread doubles in the fixed order: butterfly over `width` lanes, then (lanes > 64) the
// bucket's waves in wave order through s_red after one barrier.  Every thread gets its bucket's sum.
__device__ __forceinline__ double bucket_sum(double ss, int lanes, double* s_red) {
  const int width = lanes < kWave ? lanes : kWave;
  for (int o = 1; o < width; o <<= 1) ss += __shfl_xor(ss, o, kWave);
  if (lanes > kWave) {  // (uniform: a kernel argument)
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (kWave - 1)) == 0) s_red[wave] = ss;
    __syncthreads();
    const int nw = lanes >> 6, w0 = wave & ~(nw - 1);
    double r = 0.0;
    for (int w = 0; w < nw; ++w) r += s_red[w0 + w];
    ss = r;
  }
  return ss;
}

// WHOLE: bucket 0 — logb is 12 (the block's own sum), the sum goes to partials[block], nothing else needs the scale
template <bool WHOLE>
__global__ __launch_bounds__(kST) void sign_encode_kernel(const float* x, int64_t n, int logb,
                                                          float* __restrict__ scales, uint8_t* __restrict__ bits,
                                                          float* out, float* residual, double* __restrict__ partials) {
  __shared__ double s_red[kSNW];
  __shared__ uint4 s_bits[kST / 16];  // the block's 512 bytes of the stream, 64 per wave
  const int64_t e0 = ((int64_t)blockIdx.x * kST + threadIdx.x) * kSG;
  const int valid = e0 >= n ? 0 : (n - e0 < kSG ? (int)(n - e0) : kSG);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  float v[kSG];
  load8(x, e0, valid, v);  // (lanes past n hold +0: bit 0, |x| 0; they take part in the reductions and barriers)

  // the bits: byte -> the wave's LDS line -> four 16-B stores per wave
  reinterpret_cast<uint8_t*>(s_bits)[threadIdx.x] = (uint8_t)sign_byte(v);
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane < 4) {
    const int64_t byte0 = (int64_t)blockIdx.x * kST + wave * kWave + lane * 16;
    if (byte0 < (n + 7) / 8) *reinterpret_cast<uint4*>(bits + byte0) = s_bits[wave * 4 + lane];
  }

  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < kSG; ++j) ss += (double)fabsf(v[j]);
  ss = bucket_sum(ss, 1 << (logb - 3), s_red);
  if constexpr (WHOLE) {
    if (threadIdx.x == 0) partials[blockIdx.x] = ss;
  } else {
    if (!valid) return;
    const int64_t b = e0 >> logb, first = b << logb;
    const int64_t m = n - first < ((int64_t)1 << logb) ? n - first : (int64_t)1 << logb;
    const float scale = (float)(ss / (double)m);
    if (e0 == first) scales[b] = scale;
    sign_apply(v, scale, e0, valid, out, residual);
  }
}

// bucket 0's second launch: every block folds the np partials in the same fixed order; block 0 writes the scale
__global__ __launch_bounds__(kST) void sign_scale_kernel(const float* x, int64_t n, int64_t np,
                                                         const double* __restrict__ partials,
                                                         float* __restrict__ scales, float* out, float* residual) {
  __shared__ double s_red[kSNW];
  double ss = 0.0;
  for (int64_t i = threadIdx.x; i < np; i += kST) ss += partials[i];
  ss = bucket_sum(ss, kST, s_red);
  const float scale = (float)(ss / (double)n);
  if (blockIdx.x == 0 && threadIdx.x == 0) scales[0] = scale;
  if (!out && !residual) return;
  for (int64_t e0 = ((int64_t)blockIdx.x * kST + threadIdx.x) * kSG; e0 < n; e0 += (int64_t)gridDim.x * kSSpan) {
    const int valid = n - e0 < kSG ? (int)(n - e0) : kSG;
    float v[kSG];
    load8(x, e0, valid, v);
    sign_apply(v, scale, e0, valid, out, residual);
  }
}

// v = bit ? -scale : scale, scale = scales[e >> logb] (logb 31: scales[0]);
// out = ACC ? fmaf(w, v, out) : w * v  (w = 1: v itself)
template <bool ACC>
__global__ __launch_bounds__(256) void sign_decode_kernel(const uint8_t* __restrict__ bits, int64_t n, int logb,
                                                          const float* __restrict__ scales, float w,
                                                          float* __restrict__ out) {
  const int64_t ngroups = (n + kSG - 1) / kSG;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * 256) {
    const int64_t e0 = g * kSG;
    const int valid = n - e0 < kSG ? (int)(n - e0) : kSG;
    const float scale = scales[e0 >> logb];  // (a group of 8 lies in one bucket)
    const uint32_t byte = bits[g];
    float o[kSG];
#pragma unroll
    for (int j = 0; j < kSG; ++j) o[j] = ((byte >> j) & 1u) ? -scale : scale;
    if (ACC) {
      float prev[kSG];
      load8(out, e0, valid, prev);
#pragma unroll
      for (int j = 0; j < kSG; ++j) o[j] = fmaf(w, o[j], prev[j]);
    } else {
#pragma unroll
      for (int j = 0; j < kSG; ++j) o[j] = w * o[j];
    }
    store8(out, e0, valid, o);
  }
}

int check_sign_shape(const char* fn, int64_t n, int64_t bucket) {
  if (n < 1 || n >= (int64_t)1 << 31) return fail(FLC_EINVAL, "%s: n must be in [1, 2^31)", fn);
  if (bucket != 0 && bucket_log2(bucket) < 0)
    return fail(FLC_EINVAL, "%s: bucket %lld is not 0 or a power of two in [64, 4096]", fn, (long long)bucket);
  return FLC_OK;
}

}  // namespace
}  // namespace flc

using namespace flc;

extern "C" {

size_t flc_sign_wire_layout(int64_t n, int64_t bucket, int64_t* offsets) {
  if (n < 1 || n >= (1ll << 31) || (bucket != 0 && bucket_log2(bucket) < 0)) return 0;
  const size_t nb = bucket ? (size_t)cdiv(n, bucket) : 1;
  const size_t bits = align_up(nb * sizeof(float), 16);
  if (offsets) {
    offsets[0] = 0;
    offsets[1] = (int64_t)bits;
  }
  return align_up(bits + ((size_t)n + 7) / 8, 256);
}

size_t flc_sign_workspace_size(int64_t n, int64_t bucket) {
  if (n < 1 || n >= (1ll << 31) || bucket != 0) return 0;
  return align_up((size_t)cdiv(n, kSSpan) * sizeof(double), 256);
}

int flc_sign_encode(const float* x, int64_t n, int64_t bucket, float* scales, uint8_t* bits, float* out,
                    float* residual, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "flc_sign_encode";
  if (!x || !scales || !bits) return fail(FLC_EINVAL, "%s: null x, scales or bits", fn);
  if (int rc = check_sign_shape(fn, n, bucket)) return rc;
  if (!aligned16(x) || !aligned16(bits) || (out && !aligned16(out)) || (residual && !aligned16(residual)))
    return fail(FLC_EINVAL, "%s: x, bits, out and residual must be 16-B aligned", fn);
  hipStream_t st = as_stream(stream);
  const unsigned nblk = (unsigned)cdiv(n, kSSpan);
  if (bucket) {
    FLC_LAUNCH("sign_encode", (sign_encode_kernel<false>), dim3(nblk), dim3(kST), 0, st, x, n, bucket_log2(bucket),
               scales, bits, out, residual, (double*)nullptr);
    return FLC_OK;
  }
  const size_t need = flc_sign_workspace_size(n, 0);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 7u))
    return fail(FLC_EINVAL, "%s: workspace %zu < %zu (or null, or not 8-B aligned)", fn, ws_bytes, need);
  double* partials = static_cast<double*>(ws);
  FLC_LAUNCH("sign_encode", (sign_encode_kernel<true>), dim3(nblk), dim3(kST), 0, st, x, n, 12, scales, bits,
             (float*)nullptr, (float*)nullptr, partials);
  const unsigned grid2 = (out || residual) ? std::min<unsigned>(nblk, kScaleGrid) : 1u;
  FLC_LAUNCH("sign_scale", sign_scale_kernel, dim3(grid2), dim3(kST), 0, st, x, n, (int64_t)nblk, partials, scales,
             out, residual);
  return FLC_OK;
}

int flc_sign_decode(const uint8_t* bits, int64_t n, int64_t bucket, const float* scales, float weight, int accumulate,
                    float* out, void* stream) {
  const char* fn = "flc_sign_decode";
  if (!bits || !scales || !out) return fail(FLC_EINVAL, "%s: null bits, scales or out", fn);
  if (int rc = check_sign_shape(fn, n, bucket)) return rc;
  if (!aligned16(out) || !aligned16(bits)) return fail(FLC_EINVAL, "%s: out and bits must be 16-B aligned", fn);
  hipStream_t st = as_stream(stream);
  const int logb = bucket ? bucket_log2(bucket) : 31;  // (n < 2^31: every element reads scales[0])
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(cdiv(n, kSG), 256), 256 * 32);
  if (accumulate)
    FLC_LAUNCH("sign_decode", (sign_decode_kernel<true>), dim3(grid), dim3(256), 0, st, bits, n, logb, scales, weight,
               out);
  else
    FLC_LAUNCH("sign_decode", (sign_decode_kernel<false>), dim3(grid), dim3(256), 0, st, bits, n, logb, scales, weight,
               out);
  return FLC_OK;
}

}  // extern "C"
