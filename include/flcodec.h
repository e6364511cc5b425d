/*
 * flcodec.h — C ABI of the MI355X-native gradient codec + aggregation path for fl-sim.
 *
 * The reference (wenh06/fl-sim) has no native code and no FFI: its codec is the pure-Python class
 * `Compressor` (fl_sim/compressors/compressors.py:35-419) and its aggregation is a set of in-place
 * torch loops on the `Server` (fl_sim/nodes.py:1116-1180, fl_sim/algorithms/fedopt/_fedopt.py:196-265).
 * Every entry point below replaces one branch of those Python functions; the comment on each cites
 * the reference lines it stands in for.  INTEGRATION.md shows the ctypes binding a maintainer adds to
 * the reference (fl_sim_amd/_lib.py is that binding, shipped).
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no framework types; every device pointer is HBM memory of the current
 *     HIP device, every `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - the caller owns every buffer, including the workspace (`*_workspace_size` says how much);
 *     a workspace must be zero-filled once after allocation (flc_workspace_init) and may then be reused
 *     by any number of calls on the same stream (counters reset themselves in-kernel);
 *   - stream-ordered and asynchronous: nothing here synchronises the stream except the host-only RNG
 *     helpers and flc_probe_read; no allocation happens inside a call, so calls can be graph-captured;
 *   - the return value is a status code (FLC_OK = 0); flc_last_error() describes the last failure of
 *     the calling thread;
 *   - element counts are int64_t but a single vector must have fewer than 2^31 elements (index
 *     streams are int32, as the reference's argsort indices fit int32 below that size);
 *   - RNG: every stochastic codec takes (seed, counter) for the counter-based Philox4x32-10 stream
 *     ("philox" mode), or a device array `compat_u` of fp64 uniforms, one per consuming element in
 *     index order ("compat" mode: the exact uniforms Python's `random.random()` would have produced —
 *     see flc_mt_random_doubles).  compat_u == NULL selects philox mode.
 */
#ifndef FLCODEC_H_
#define FLCODEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLC_ABI_VERSION 1

enum flc_status {
  FLC_OK = 0,
  FLC_EINVAL = 1,       /* bad argument (sizes, levels, bits, null pointer) */
  FLC_EHIP = 2,         /* HIP runtime error */
  FLC_EWORKSPACE = 3,   /* workspace too small */
  FLC_EUNSUPPORTED = 4, /* valid request this build does not implement */
  FLC_ECOMM = 5         /* RCCL error, or RCCL could not be loaded */
};

/* dense quantizer families (compressors.py:327-404) */
enum flc_quant_kind {
  FLC_Q_STANDARD_DITHER = 0, /* levels i/s, i = 0..s          (compressors.py:154-182, 327-365) */
  FLC_Q_NATURAL_DITHER = 1   /* levels 0, 2^-(s-1), .., 1/2, 1 (compressors.py:191-221, 367-404) */
};
enum flc_norm_kind { FLC_NORM_INF = 0, FLC_NORM_L2 = 2 };

/* proximal step of FedDR's regularizer (regularizers.py:146-200) */
enum flc_prox_kind { FLC_PROX_NONE = 0, FLC_PROX_L1 = 1, FLC_PROX_SCALE = 2 };

/* server optimiser of FedOptServer.update (_fedopt.py:196-265) */
enum flc_fedopt_kind { FLC_OPT_AVG = 0, FLC_OPT_ADAGRAD = 1, FLC_OPT_YOGI = 2, FLC_OPT_ADAM = 3 };

/* ------------------------------------------------------------------ library */
int flc_abi_version(void);
const char* flc_last_error(void);
/* zero a freshly allocated workspace (once); stream-ordered */
int flc_workspace_init(void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ host RNG (compat mode)
 * Python's `random` and numpy's legacy `RandomState` are both MT19937.  These host functions advance
 * a state exported by `random.getstate()[1]` (624 words + position) or `np.random.get_state()`
 * (624 words, position) exactly as the interpreter would, so the caller can write the advanced state
 * back and the global streams stay in lock-step with the reference (misc.py:196-217 seeds them).  */

/* n draws of random.random() (compressors.py:277, 316, 349, 386) == legacy random_sample (res53) */
int flc_mt_random_doubles(uint32_t* mt_state624, int32_t* mt_pos, double* out, int64_t n);
/* np.random.shuffle(np.arange(D)) then [:K] (compressors.py:285-287): legacy Fisher-Yates with
 * masked-rejection random_interval; writes the first K entries of the shuffled permutation */
int flc_np_shuffle_prefix(uint32_t* mt_state624, int32_t* mt_pos, int64_t D, int64_t K, int32_t* out_idx);

/* ------------------------------------------------------------------ dense quantizer codec
 * x is a [rows, d] row-major fp32 batch: one client delta per row (rows = 1 for compressVector).
 * Wire format per row: one fp32 norm + a packed code stream of `bits` (2, 4 or 8) bits per element,
 *   code = sign << (bits-1) | level, level in 0..s (s < 2^(bits-1)); element i of the flat batch sits
 *   at bit offset i*bits of `codes` (little-endian within a byte).
 * A row whose norm is not finite is encoded as code 0 for x == 0 and code 1 otherwise; it decodes to
 *   +0 / NaN, which is what the reference produces for such rows. */
size_t flc_quant_workspace_size(int64_t rows, int64_t d);
/* per-row ||x||_p: p = inf → max |x| (exact, NaN-propagating), p = 2 → sqrt of an fp64 sum of
 * squares rounded once to fp32 (compressors.py:332, 372; np.linalg.norm) */
int flc_quant_norm(const float* x, int64_t rows, int64_t d, int norm_p, float* norms, void* ws,
                   size_t ws_bytes, void* stream);
/* encode (compressors.py:339-365 / 376-404, the stochastic level choice); `nnz` (device, int64[rows])
 * receives the count of x != 0 per row, the quantity the reference's send-statistics count. */
int flc_quant_encode(const float* x, int64_t rows, int64_t d, int kind, int levels, int bits,
                     const float* norms, uint64_t seed, uint64_t counter, const double* compat_u,
                     uint8_t* codes, int64_t* nnz, void* ws, size_t ws_bytes, void* stream);
/* encode + decode in one pass (compressVector's round trip, compressors.py:339-365 / 376-404): the codes are
 * written exactly as flc_quant_encode writes them and out receives the value flc_quant_decode would give each code
 * (weight 1, no accumulate), computed from the code in registers instead of reading the wire back. */
int flc_quant_encode_decode(const float* x, int64_t rows, int64_t d, int kind, int levels, int bits,
                            const float* norms, uint64_t seed, uint64_t counter, const double* compat_u,
                            uint8_t* codes, int64_t* nnz, float* out, void* ws, size_t ws_bytes, void* stream);
/* philox mode, norm included: the per-row norm (as flc_quant_norm computes it, written to norms), the encode and,
 * with out != NULL, the fused decode.  p = inf with d >= 16384 and a batch of at most #CU x 32768 elements (configs[1]:
 * 10 x 417,482) runs in ONE persistent launch (one 1024-thread block per CU, a grid exchange of the per-row maxima;
 * the co-residency contract of the top-k encoders, flc_topk_status below: check flc_quant_status); otherwise two
 * launches when d >= 2048 (the encode folds the norm partials itself), three below.  The result is the same. */
int flc_quant_encode_auto(const float* x, int64_t rows, int64_t d, int kind, int levels, int bits, int norm_p,
                          uint64_t seed, uint64_t counter, uint8_t* codes, float* norms, int64_t* nnz, float* out,
                          void* ws, size_t ws_bytes, void* stream);
/* a round's messages in one call (philox mode, norm included): message c is the flat vector xs[c] of n elements with
 * its own Philox (seeds[c], counters[c]), its own code stream codes[c] (ceil(n * bits / 8) bytes), norm *norms[c]
 * and, with counts != NULL, nonzero count *counts[c] (device int64, zeroed in the stream by the call); the element
 * index restarts at 0 in every message.  Every output is bit-identical to flc_quant_encode_auto(xs[c], 1, n, ...,
 * seeds[c], counters[c], codes[c], norms[c], counts[c], NULL, ...), whichever launch form that call takes (p = 2
 * keeps flc_quant_norm's partition and traversal per message).  Two ordinary launches per 64 messages for any n — the
 * norm partials over (part, message), the encode over (block, message), each block folding its message's partials —
 * with the message table in the kernel arguments: no grid-wide wait, no status word, nothing copied from the host
 * arrays, capturable into a graph; more than 64 messages chain launches.  xs, seeds, counters, codes, norms and counts
 * are HOST arrays of n_msgs entries.  FLC_EINVAL (nothing launched): a null table or entry (counts itself may be
 * NULL), n_msgs < 1, n < 1 or n >= 2^31, levels not fitting bits, norm_p other than 0 or 2, an xs[c] or codes[c] not
 * 16-B aligned.  FLC_EWORKSPACE: ws_bytes < flc_quant_encode_round_workspace_size(n, n_msgs). */
size_t flc_quant_encode_round_workspace_size(int64_t n, int n_msgs);
int flc_quant_encode_round(const float* const* xs, int n_msgs, int64_t n, int kind, int levels, int bits, int norm_p,
                           const uint64_t* seeds, const uint64_t* counters, uint8_t* const* codes,
                           float* const* norms, int64_t* const* counts, void* ws, size_t ws_bytes, void* stream);
/* flc_quant_encode_round with error feedback in the encode's own pass: message c's input is its error memory es[c],
 * already holding a (flc_ef_accumulate), and the call leaves es[c][i] = fp32(a_i - v_i) for every i < n, v_i the value
 * flc_quant_decode(codes[c], 1, n, kind, levels, bits, norms[c], NULL, 0, .) gives element i.  codes[c], *norms[c]
 * and *counts[c] are bit-identical to flc_quant_encode_round's for xs[c] = es[c], and the memories to that call
 * followed by flc_quant_decode into a fresh vector and flc_ef_residual_dense: every element is subtracted (a zero
 * code's a_i - 0 keeps a_i, -0 included; under a norm of 0, +-inf or NaN any other code gives NaN).  Each thread of
 * the encode launch computes the decoder's value of its codes from registers and stores the residual to the positions
 * it loaded: no decode, no temporary, no further launch.  Launches as flc_quant_encode_round (one norm and one encode
 * launch per 64 messages, capturable); only the encode launch writes a memory, so if a launch cannot be enqueued
 * (FLC_EHIP) the memories of that link of 64 messages and of every later link still hold a, while those of earlier
 * links already hold the residual.  FLC_EINVAL (nothing launched): flc_quant_encode_round's cases, an es[c] that is
 * null or not 16-B aligned, two messages whose memories share elements.  FLC_EWORKSPACE: ws_bytes <
 * flc_quant_encode_round_workspace_size(n, n_msgs). */
int flc_quant_encode_residual_round(float* const* es, int n_msgs, int64_t n, int kind, int levels, int bits,
                                    int norm_p, const uint64_t* seeds, const uint64_t* counters,
                                    uint8_t* const* codes, float* const* norms, int64_t* const* counts, void* ws,
                                    size_t ws_bytes, void* stream);
/* the quantizer workspace's sticky error word (4: a one-launch encode's grid exchange timed out, i.e. its blocks were
 * not all resident — the outputs of that call are invalid); copied to *err_out (device uint64), zeroed with reset */
int flc_quant_status(void* ws, uint64_t* err_out, int reset, void* stream);
/* compat mode: how many uniforms the reference draws for this batch — one per element with x != 0
 * whose y = |x| / norm is not NaN (compressors.py:339-354); norms == NULL counts x != 0 (the natural
 * compressor, compressors.py:307-316).  *count is a device int64. */
int flc_count_consumers(const float* x, int64_t rows, int64_t d, const float* norms, int64_t* count,
                        void* stream);
/* decode: v = fp32(fp32(level_value) * sign) * norm (compressors.py:357/394);
 * out = accumulate ? fmaf(row_weight, v, out) : (row_weights ? row_weight * v : v) */
int flc_quant_decode(const uint8_t* codes, int64_t rows, int64_t d, int kind, int levels, int bits,
                     const float* norms, const float* row_weights, int accumulate, float* out,
                     void* stream);

/* ------------------------------------------------------------------ bucketed dithering
 * The dithering quantizers applied per bucket of `bucket` = B consecutive elements, each bucket with its own norm: the
 * result on a vector of n elements is compressVector (compressors.py:327-365 standard, 367-404 natural dithering)
 * applied to the slices x[0:B], x[B:2B], ..., x[(nb-1)B : n] in order, nb = ceil(n / B), the last slice possibly
 * short.  B is a power of two in [64, 4096]; float32 only; kind, levels and bits as flc_quant_encode; norm_p is
 * FLC_NORM_INF or FLC_NORM_L2.
 *
 * Record layout (flc_bucket_wire_layout): returns the record size (a multiple of 256 B; 0 for bad arguments: a format
 * other than FLC_Q_STANDARD_DITHER / FLC_Q_NATURAL_DITHER — FLC_WIRE_NATURAL has no norm —, bits not 2, 4 or 8, a
 * bucket outside the set above, n < 1 or n >= 2^31) and, if offsets != NULL, the byte offsets of offsets[0] the nb
 * fp32 norms and offsets[1] the packed codes (16-B aligned, ceil(n * bits / 8) bytes, element i at bit offset
 * i * bits: the quantizer codec's code stream; B * bits / 8 >= 16, so every bucket's codes start 16-B aligned).
 * A pure host function. */
size_t flc_bucket_wire_layout(int64_t n, int format, int bits, int64_t bucket, int64_t* offsets);
/* encode one message in philox mode in ONE launch that reads x once (compressors.py:332 / 372 the norm, 339-365 /
 * 376-404 the level choice, per slice): every bucket's norm is computed from values that stay in registers until the
 * level decision.  p = inf: the exact max of the |x| bits, NaN-propagating (flc_quant_norm's); p = 2: fp32(sqrt(S)),
 * S the fp64 sum of the bucket's squares in an order fixed by B and the position in the bucket (elements past n count
 * as +0), never by the grid.  Element e uses Philox word e & 3 of counter group e >> 2, e the index in the whole
 * message, through the tail bucket.  For n a multiple of B and p = inf the norms and codes are those of flc_quant_norm
 * + flc_quant_encode on the [n / B, B] batch with the same (seed, counter).  norms_given != 0: the norms are read
 * from `norms` instead (host-computed reference norms).  norms: nb floats; codes: ceil(n * bits / 8) bytes, 16-B
 * aligned (a record's fields, or any buffers).  nnz (device int64, optional): the message's count of x != 0, zeroed in
 * the stream by the call.  out (optional, n floats, 16-B aligned): the decoder's value of every code, from registers —
 * compressVector's result.  A bucket whose norm is 0, +-inf or NaN encodes code 0 for x == 0 and code 1 otherwise,
 * inside that bucket only.  Algorithmic bytes per element: 4 + bits / 8 + 4 / B (+ 4 with out).  No workspace, no
 * status word, no grid-wide wait: capturable.  FLC_EINVAL (nothing launched): a null x, norms or codes, n < 1 or
 * n >= 2^31, a bad bucket, levels not fitting bits, norm_p other than 0 or 2, x, codes or out not 16-B aligned. */
int flc_bucket_encode(const float* x, int64_t n, int kind, int levels, int bits, int64_t bucket, int norm_p,
                      int norms_given, uint64_t seed, uint64_t counter, float* norms, uint8_t* codes, int64_t* nnz,
                      float* out, void* stream);
/* flc_quant_encode_round's contract for bucket records: message c is xs[c] (n elements) with its own Philox
 * (seeds[c], counters[c]), norms norms[c] (nb floats), codes codes[c] and, with counts != NULL, count *counts[c] (device
 * int64, zeroed in the stream by the call: one memset per run of consecutive slots).  Bit-identical to
 * flc_bucket_encode per message.  One ordinary launch per 64 messages over (block, message) with the message table in
 * the kernel arguments; more messages chain launches.  All tables are HOST arrays of n_msgs entries.  FLC_EINVAL
 * (nothing launched): flc_bucket_encode's cases per message, a null table or entry (counts itself may be NULL),
 * n_msgs < 1. */
int flc_bucket_encode_round(const float* const* xs, int n_msgs, int64_t n, int kind, int levels, int bits,
                            int64_t bucket, int norm_p, int norms_given, const uint64_t* seeds,
                            const uint64_t* counters, float* const* norms, uint8_t* const* codes,
                            int64_t* const* counts, void* stream);
/* decode (compressors.py:357 / 394 per slice): v = fp32(fp32(level_value) * sign) * norms[e / B];
 * out = accumulate ? fmaf(weight, v, out) : weight * v  (weight 1: v itself).  FLC_EINVAL as flc_bucket_encode. */
int flc_bucket_decode(const uint8_t* codes, int64_t n, int kind, int levels, int bits, int64_t bucket,
                      const float* norms, float weight, int accumulate, float* out, void* stream);

/* The folds over bucket records, the four forms every record codec has: flc_fold_dense_wires,
 * flc_fedopt_fold_dense_records, flc_avg_and_gradient_dense_records and flc_fold_dense_record_groups (below) with the
 * records laid out by flc_bucket_wire_layout(n, format, bits, bucket) and the norm of element e read from
 * (record, e / bucket) — the server's weighted aggregation (nodes.py:1165-1180 / _fedopt.py:202-208) fused with the
 * per-slice decode of compressors.py:357 / 394.  Each is bit-identical to decoding every record with flc_bucket_decode
 * and running the dense entry point its counterpart names (flc_quant_decode(accumulate = 1) chains, flc_model_fold,
 * flc_avg_and_gradients, flc_weighted_sum per group).  Arguments, chaining per 64 records and FLC_EINVAL cases as the
 * dense forms, plus a bucket that is not a power of two in [64, 4096] and format FLC_WIRE_NATURAL (no norm). */
int flc_fold_bucket_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                          int64_t n, int format, int levels, int bits, int64_t bucket, int accumulate, float* out,
                          void* stream);
int flc_fedopt_fold_bucket_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                   int format, int levels, int bits, int64_t bucket, float* const* delta,
                                   float* const* theta, float* const* v, const int64_t* sizes, int n_tensors,
                                   float beta0, int opt, double lr, double beta2, double tau, void* stream);
int flc_avg_and_gradient_bucket_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                        const void* const* grad_records, const float* w_params, const float* w_grads,
                                        int n_src, int64_t n, int format, int levels, int bits, int64_t bucket,
                                        const int64_t* sizes, int n_tensors, float inertia, void* stream);
int flc_fold_bucket_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                  int n_records, int64_t n, int format, int levels, int bits, int64_t bucket,
                                  float* const* dsts, int n_groups, const int64_t* sizes, int n_tensors,
                                  void* stream);

/* ------------------------------------------------------------------ natural compressor
 * (compressors.py:302-325).  Wire: one uint16 per element, 0 = zero, else sign << 15 | (e + 150)
 * for the chosen power of two 2^e, e in [-149, 127]. */
size_t flc_natural_workspace_size(int64_t n);  /* needed in compat mode only */
int flc_natural_encode(const float* x, int64_t n, uint64_t seed, uint64_t counter,
                       const double* compat_u, uint16_t* codes, int64_t* nnz, void* ws, size_t ws_bytes,
                       void* stream);
int flc_natural_decode(const uint16_t* codes, int64_t n, float weight, int accumulate, float* out,
                       void* stream);
/* a round's messages in one call (philox mode only; compat mode's sequential uniforms stay with flc_natural_encode;
 * compressors.py:302-325): message c is the flat vector xs[c] of n elements with its own Philox (seeds[c],
 * counters[c]) and its own code stream codes[c] (2n bytes); the element index restarts at 0 in every message, so
 * codes[c] is bit-identical to flc_natural_encode(xs[c], n, seeds[c], counters[c], NULL, codes[c], NULL, ...).  The
 * compressor has no norm: ONE ordinary streaming launch per 64 messages over (block of 8192 elements, message), no
 * workspace, no counts (the send count is 9/32 n whatever the data), no grid-wide wait and no status word; the message
 * table travels in the kernel arguments, so nothing is copied from the host arrays and the call is capturable; more
 * than 64 messages chain launches.  Code bytes past 2n are never written.  xs, seeds, counters and codes are HOST
 * arrays of n_msgs entries.  FLC_EINVAL (nothing launched): a null table or entry, n_msgs < 1, n < 1 or n >= 2^31, an
 * xs[c] or codes[c] not 16-B aligned. */
int flc_natural_encode_round(const float* const* xs, int n_msgs, int64_t n, const uint64_t* seeds,
                             const uint64_t* counters, uint16_t* const* codes, void* stream);
/* flc_natural_encode_round with error feedback in the encode's own pass: message c's input is its error memory es[c],
 * already holding a (flc_ef_accumulate), and the call leaves es[c][i] = fp32(a_i - v_i) for every i < n, v_i the value
 * flc_natural_decode(codes[c], n, 1, 0, .) gives element i.  codes[c] is bit-identical to flc_natural_encode_round's
 * for xs[c] = es[c], and the memories to that call followed by flc_natural_decode into a fresh vector and
 * flc_ef_residual_dense: every element is subtracted (a zero code's a_i - 0 keeps a_i, -0 included; a NaN's code
 * 0x7fff gives a_i - NaN, +-inf gives a_i - (+-inf)).  Each thread computes the decoder's value of the codes it has
 * just formed and stores the residual to the positions it loaded (plain stores: the next round's accumulate reads
 * them): no decode, no temporary, no further launch.  Elements at or past n are never written.  Only the encode
 * launch writes a memory, so if a launch cannot be enqueued (FLC_EHIP) the memories of that link of 64 messages and
 * of every later link still hold a, while those of earlier links already hold the residual.  FLC_EINVAL (nothing
 * launched): flc_natural_encode_round's cases, an es[c] that is null or not 16-B aligned, two messages whose
 * memories [es[c], es[c] + n) share elements. */
int flc_natural_encode_residual_round(float* const* es, int n_msgs, int64_t n, const uint64_t* seeds,
                                      const uint64_t* counters, uint16_t* const* codes, void* stream);

/* ------------------------------------------------------------------ top-k sparsifier
 * (compressors.py:293-296): keeps the k largest *signed* values (NaN largest, -0 == +0); among values
 * equal to the k-th largest the highest indices are kept (the order of a stable ascending argsort).
 * Output: idx[k] ascending, val[k] the kept values bit-for-bit.  Requires 0 < k < n.
 *
 * Co-residency: the top-k and stacked encoders are ONE persistent launch of one 1024-thread block per CU
 * whose blocks hand work to each other through flags in the workspace, so every block of the launch must
 * be resident at once.  Launches of these encoders on one device are serialised by the library (stream
 * order, or an event chain across streams; not inside a stream capture); kernels of other libraries or
 * processes that occupy CUs for long stretches can delay a block past the bounded spin, which the kernel
 * records in the workspace's sticky error word instead of hanging.  flc_topk_status reads that word:
 * 0 = every call since the last reset was exact; otherwise bits 1 (digit not found), 2 (count mismatch),
 * 4 (exchange spin timeout) mean the kept set of some call may be wrong.  Check it after calls that may
 * have shared the device (fl_sim_amd does when FLC_TOPK_CHECK=1, and the GPU tests after every test). */
/* *err_out (device uint64) = the workspace's sticky error word; reset != 0 clears it (stream-ordered) */
int flc_topk_status(void* ws, uint64_t* err_out, int reset, void* stream);
/* Diagnostics of the select (the result never depends on them; tests use them to assert which path a call took).
 * flc_topk_select_plan: host only (no device call when cus > 0; cus == 0 reads the current device's CU count).
 * Fills out[FLC_PLAN_WORDS] with the numbers the select uses for a call over n elements keeping k: clients == 0
 * for the single-client entry points (flc_topk_encode*, flc_stacked_encode*), clients >= 1 for the batched ones. */
enum {
  FLC_PLAN_S = 0,        /* sample keys */
  FLC_PLAN_RANK_LO = 1,  /* the floor is the sample's rank_lo-th largest key */
  FLC_PLAN_RANK_HI = 2,  /* the ceiling its rank_hi-th largest (0: no ceiling) */
  FLC_PLAN_TAKE_ALL = 3, /* 1: no sample, every element is a candidate */
  FLC_PLAN_G = 4,        /* blocks per select */
  FLC_PLAN_M = 5,        /* elements per block range */
  FLC_PLAN_OVF = 6,      /* candidates per block kept in HBM beyond LDS_CAP (0: none) */
  FLC_PLAN_LIST_CAP = 7, /* in-bin keys a block may publish before the select falls to histogram rounds */
  FLC_PLAN_COMPACT = 8,  /* 1: the floor / ceiling start from the compact sample */
  FLC_PLAN_CAP = 9,      /* candidates per block kept in LDS */
  FLC_PLAN_LIST_ALL = 10,/* in-bin keys of all blocks resolved locally */
  FLC_PLAN_HIST_BITS = 11, /* log2 of the band histogram's bins */
  FLC_PLAN_FAST_RANK = 12, /* the fast pick runs while rank_lo <= this */
  FLC_PLAN_CHUNK = 13,   /* batched: clients per launch (their headers are reused by the next launch) */
  FLC_PLAN_CUS = 14,     /* the CU count used */
  FLC_PLAN_WORDS = 16
};
int flc_topk_select_plan(int64_t n, int64_t k, int clients, int cus, int64_t* out);
/* The state words the last call on `ws` left for select `client` (0 for a single-client workspace; the client's
 * place in its launch for a batched one), copied to the HOST array out16 in the order of FLC_SEL_*; synchronises
 * the stream once. */
enum {
  FLC_SEL_CALL = 0, FLC_SEL_ERR = 1, FLC_SEL_C = 2, FLC_SEL_FALLBACK = 3, FLC_SEL_T = 4, FLC_SEL_MAXKEY = 5,
  FLC_SEL_ROUNDS = 6, FLC_SEL_T_LO = 7, FLC_SEL_T_HI = 8, FLC_SEL_NEED = 9, FLC_SEL_TIES = 10, FLC_SEL_STRICT = 11,
  FLC_SEL_SAMPLE_PATH = 12 /* 0 fast pick, 1 general radix pick, 2 take-all */
};
int flc_topk_select_stats(const void* ws, size_t ws_bytes, int client, uint64_t* out16, void* stream);
/* Test hook (host only, no device): the batched encoders' pinned table ring (a ring of 32 host slots whose reuse
 * waits for an event recorded after every 8th slot's use, or drains the device) driven by `n_ops` triples
 * (kind, slot, stream id): kind 0 stages the next slot and writes (slot, wait 0 none / 1 event / 2 drain, event slot)
 * to `out`; kind 1 marks `slot` done on stream `stream id` (> 0).  Returns the triples written, or -1. */
int flc_ring_selftest(const int32_t* ops, int n_ops, int32_t* out, int n_out);
size_t flc_topk_workspace_size(int64_t n, int64_t k);
int flc_topk_encode(const float* x, int64_t n, int64_t k, int32_t* idx, float* val, void* ws,
                    size_t ws_bytes, void* stream);
/* Tile pointers (CSR row pointers over FLC_TILE-output tiles) of an ascending index stream:
 * tiles[t] = first j with idx[j] >= t * FLC_TILE, t = 0 .. ceil(n / FLC_TILE); the encoders' *_tiled
 * variants emit them alongside the wire (so that a decoder needs no index pass), flc_tile_index forms
 * them from idx alone. */
#define FLC_TILE 1024
int flc_tile_index(const int32_t* idx, int64_t k, int64_t n, uint32_t* tiles, void* stream);
/* flc_topk_encode_tiled writes a sparse record (flc_sparse_wire_layout(n, k), below) when idx, val and tiles are the
 * three pointers inside it. */
int flc_topk_encode_tiled(const float* x, int64_t n, int64_t k, int32_t* idx, float* val, uint32_t* tiles,
                          void* ws, size_t ws_bytes, void* stream);
/* dense decode of an ascending sparse stream of unique indices below n: v[idx[j]] = fl(scale * val[j]), v = +0
 * elsewhere (compressors.py:289-291, 294-295); then, over the whole vector (the fused aggregation),
 *   out = accumulate ? fmaf(weight, v, out) : (weight != 1 ? fl(weight * v) : v)
 * An unkept position takes the weight like a kept one: -0 under a negative weight, NaN under an infinite or NaN one.
 * 0 <= k <= n: k == 0 (idx and val may be NULL) decodes the all-zero vector and still writes every element of out,
 * k == n keeps every element.  Nothing outside out[0, n) is written.  Workspace: a per-tile index of the stream. */
size_t flc_sparse_decode_workspace_size(int64_t n);
int flc_sparse_decode(const int32_t* idx, const float* val, int64_t k, float scale, int64_t n,
                      float weight, int accumulate, float* out, void* ws, size_t ws_bytes, void* stream);
int flc_sparse_decode_tiled(const int32_t* idx, const float* val, int64_t k, float scale, int64_t n,
                            float weight, int accumulate, float* out, const uint32_t* tiles, void* stream);

/* ------------------------------------------------------------------ stacked top-k -> 8-bit dither
 * Top-k of x (as above), then standard dithering with s = levels (<= 127), p = inf, of the k kept
 * values: the pipeline TopK(x) followed by StandardDithering on the k-sparse result.
 * Wire: idx[k] int32 ascending, codes[k] (sign << 7 | level), norm[1] fp32. */
int flc_stacked_encode(const float* x, int64_t n, int64_t k, int levels, uint64_t seed,
                       uint64_t counter, const double* compat_u, int32_t* idx, uint8_t* codes,
                       float* norm, void* ws, size_t ws_bytes, void* stream);
int flc_stacked_encode_tiled(const float* x, int64_t n, int64_t k, int levels, uint64_t seed,
                             uint64_t counter, const double* compat_u, int32_t* idx, uint8_t* codes,
                             float* norm, uint32_t* tiles, void* ws, size_t ws_bytes, void* stream);
/* dense decode: v[idx[j]] = fp32(fp32(lv) * sign) * norm with lv = level * (1 / levels) in fp64 and lv = 1 at level ==
 * levels (compressors.py:157, 357; a set sign bit with level 0 gives -0), v = +0 elsewhere; a norm that is 0, negative,
 * +-inf or NaN decodes code 0 to +0 and every other code to NaN.  The output rule over the whole vector, 0 <= k <= n
 * and the extent are flc_sparse_decode's. */
int flc_stacked_decode(const int32_t* idx, const uint8_t* codes, int64_t k, int levels,
                       const float* norm, int64_t n, float weight, int accumulate, float* out,
                       void* ws, size_t ws_bytes, void* stream);  /* ws: flc_sparse_decode_workspace_size */
int flc_stacked_decode_tiled(const int32_t* idx, const uint8_t* codes, int64_t k, int levels,
                             const float* norm, int64_t n, float weight, int accumulate, float* out,
                             const uint32_t* tiles, void* stream);

/* Packed wire: one client's stacked wire as ONE contiguous record whose layout depends on (n, k) only, so that
 * a [clients, stride] byte buffer moves as one piece (RCCL all-gather, PCIe copy).  Returns the record size
 * (a multiple of 256 B; 0 for bad arguments) and, if offsets != NULL, the byte offsets of
 * offsets[0] norm (fp32), [1] idx (int32[k]), [2] codes (u8[max(k,16)]), [3] tiles (u32[ceil(n/FLC_TILE)+1]).
 * flc_stacked_encode_tiled writes a record when given those four pointers inside it. */
size_t flc_stacked_wire_layout(int64_t n, int64_t k, int64_t* offsets);
/* Fold of many clients' wires into one vector in ONE pass over out (the server's weighted aggregation,
 * nodes.py:1165-1180 / _fedopt.py:202-208, fused with the decode):
 *   out = (accumulate ? out : +0);  for c = 0 .. n_wires-1:  out = fmaf(weights[c], decode(record slots[c]), out)
 * elementwise, in that order — bit-identical to n_wires flc_stacked_decode_tiled(weight, accumulate=1) calls on a
 * zeroed (or the given) out.  wires: records of `stride` bytes (>= flc_stacked_wire_layout(n, k), 16-B multiple),
 * record index slots[c] holds client c; slots and weights are HOST arrays.  Replaces SURVEY §8(e)'s dense reduce
 * when the records are all-gathered: every rank folds all clients in client order, so the result does not depend on
 * the number of GPUs. */
int flc_stacked_fold_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights,
                           int n_wires, int64_t n, int64_t k, int levels, int accumulate, float* out, void* stream);
/* A compressed FedOpt round's server update in ONE pass (replaces FedOptServer.update, _fedopt.py:196-240, when each
 * client message carries its delta as a packed stacked record — the codec's call site, fl_sim_amd/compressed.py):
 * over the flat concatenation of the model's tensors (element e of the records = element e - offset_t of tensor t,
 * the order FedOptClient.communicate's delta list flattens in),
 *   a = delta * beta0;  for c = 0 .. n_records-1:  a = fmaf(weights[c], decode(records[c]), a);  delta = a;
 *   then, if theta != NULL, the optimiser's step on theta (and v): avg theta = fmaf(lr, a, theta); adagrad / yogi /
 *   adam as flc_model_fold (every rounding where torch's CPU ops round).
 * Bit-identical to decoding every record densely (flc_stacked_decode_tiled) and running flc_model_fold with
 * init_mode 0 and the step.  records: HOST array of n_records device pointers to records of the
 * flc_stacked_wire_layout(n, k) layout (16-B aligned; any device memory the stream's device can read, e.g. each client's
 * own); delta / theta / v: HOST arrays of n_tensors device pointers (v only for adaptive optimisers; pinned host
 * memory mapped into the device's address space works too), sizes summing to n.  theta == NULL: the fold alone. */
int flc_fedopt_fold_records(const void* const* records, const float* weights, int n_records, int64_t n, int64_t k,
                            int levels, float* const* delta, float* const* theta, float* const* v,
                            const int64_t* sizes, int n_tensors, float beta0, int opt, double lr, double beta2,
                            double tau, void* stream);
/* A round whose records fall into groups, each group accumulating in place into its own model, in ONE pass: the
 * server side of a compressed SCAFFOLD round (the groups are its two vectors: theta += lr/|msgs| * parameters_delta,
 * c += 1/N * control_variates_delta; replaces SCAFFOLDServer.update, scaffold/_scaffold.py:160-169, when the clients
 * send both deltas as packed stacked records in place of _scaffold.py:210-222) and of a compressed IFCA round (the
 * groups are the clusters: center += 1/cluster_size * delta; replaces ifca/_ifca.py:186-195 over the messages of
 * _ifca.py:228-240).  For every group g, tensor t and element e of tensor t (flat element start_t + e of the records):
 *   a = dsts[g * n_tensors + t][e];
 *   for c = 0 .. n_records-1 with group_of[c] == g, in that order:  a = fmaf(weights[c], decode(records[c]), a);
 *   dsts[g * n_tensors + t][e] = a
 * — add_parameters' in-place accumulation (nodes.py:1116-1132): nothing scaled, nothing zeroed.  A group without a
 * record is neither read nor written (its pointers may be NULL).  Bit-identical to decoding every record densely
 * (flc_stacked_decode_tiled) and calling flc_weighted_sum(init_mode 2) per tensor: -0 and +-inf accumulators, empty
 * tiles and weights of either sign or zero included; a NaN accumulator stays NaN.  records / weights / group_of / dsts
 * / sizes: HOST arrays; records of the flc_stacked_wire_layout(n, k) layout, 16-B aligned; sizes summing to n.  One
 * launch (grid = tiles x groups) for n_records <= 64 over all groups, <= 16 groups with records and n_tensors <= 16;
 * beyond that launches chain, each continuing from the stored results, the order within a group kept.  FLC_EINVAL
 * (nothing launched): a null or misaligned record, a group_of outside [0, n_groups), sizes not summing to n, n or
 * k >= 2^31, levels outside [1, 127], a null destination of a non-empty tensor in a group that has records, the same
 * destination in two groups. */
int flc_fold_record_groups(const void* const* records, const float* weights, const int32_t* group_of, int n_records,
                           int64_t n, int64_t k, int levels, float* const* dsts /* [n_groups][n_tensors] */,
                           int n_groups, const int64_t* sizes, int n_tensors, void* stream);

/* ------------------------------------------------------------------ sparse records (top-k / rand-k wire)
 * One client's top-k or rand-k wire (compressors.py:284-296) as ONE contiguous record, the plain sparsifiers'
 * counterpart of the stacked record above: what a message carries in place of the 4 n bytes of the decoded vector
 * compressVector returns.  Returns the record size (a multiple of 256 B; 0 for bad arguments: n < 1, k < 1, k > n, n or
 * k >= 2^31) and, if offsets != NULL, the byte offsets of
 * offsets[0] idx (int32[k], ascending), [1] val (fp32[k]: the DECODED values, so for rand-k already scale * x[idx],
 * compressors.py:290-291), [2] tiles (u32[ceil(n/FLC_TILE)+1], the stacked record's CSR pointers); every field 16-B
 * aligned.  The layout depends on (n, k) only.  decode(record) is flc_sparse_decode_tiled(idx, val, k, scale = 1, n,
 * ..., tiles).  flc_topk_encode_tiled and flc_topk_encode_batch write a record when given the three pointers inside it;
 * a rand-k record is its ascending index set, flc_sparse_gather's values and flc_tile_index's (or the key select's)
 * tiles. */
size_t flc_sparse_wire_layout(int64_t n, int64_t k, int64_t* offsets);
/* flc_stacked_fold_wires' contract over sparse records (the server's weighted aggregation, nodes.py:1165-1180 /
 * _fedopt.py:202-208, fused with the decode of compressors.py:289-291 / 294-295):
 *   out = (accumulate ? out : +0);  for c = 0 .. n_wires-1:  out = fmaf(weights[c], decode(record slots[c]), out)
 * elementwise, in that order — bit-identical to n_wires flc_sparse_decode_tiled(scale 1, weight = w_c, accumulate = 1)
 * calls on a zeroed (or the given) out: fmaf(w, +0, a) on the elements no entry names (a -0 accumulator included),
 * +-inf and NaN accumulators, weights of either sign, zero or denormal, kept values that are -0, denormal, +-inf or NaN.
 * The stacked fold's kernel with the fp32 value as its entry codec: one wave per tile, one load batch for tiles of
 * <= 128 entries over all clients, every tile pointer clamped to k, an index outside its tile ignored.  wires, stride,
 * slots, weights and the chaining past 64 records as flc_stacked_fold_wires'.  FLC_EINVAL (nothing launched): its
 * cases, with k outside [1, n] in place of the levels. */
int flc_fold_sparse_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                          int64_t n, int64_t k, int accumulate, float* out, void* stream);
/* flc_fedopt_fold_records' contract over sparse records (replaces FedOptServer.update, _fedopt.py:196-240, when each
 * client message carries its delta as a sparse record in place of compressors.py:284-296's decoded vector):
 *   a = delta * beta0;  for c = 0 .. n_records-1:  a = fmaf(weights[c], decode(records[c]), a);  delta = a;
 *   then, if theta != NULL, the optimiser's step (avg / adagrad / yogi / adam, as flc_model_fold).
 * Bit-identical to decoding every record densely (flc_sparse_decode_tiled) and running flc_model_fold with init_mode 0
 * and the step.  Arguments as flc_fedopt_fold_records' without levels; k in [1, n]. */
int flc_fedopt_fold_sparse_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                   int64_t k, float* const* delta, float* const* theta, float* const* v,
                                   const int64_t* sizes, int n_tensors, float beta0, int opt, double lr, double beta2,
                                   double tau, void* stream);
/* flc_fold_record_groups' contract over sparse records (add_parameters' in-place accumulation per group,
 * nodes.py:1116-1132; SCAFFOLD's two vectors, _scaffold.py:160-169, IFCA's clusters, _ifca.py:186-195): bit-identical
 * to decoding every record densely and calling flc_weighted_sum(init_mode 2) per group and tensor.  Arguments, chaining
 * and FLC_EINVAL cases as flc_fold_record_groups' without levels; k in [1, n]. */
int flc_fold_sparse_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                  int n_records, int64_t n, int64_t k, float* const* dsts /* [n_groups][n_tensors] */,
                                  int n_groups, const int64_t* sizes, int n_tensors, void* stream);

/* ------------------------------------------------------------------ dense records (dithering / natural wire)
 * One client's dithering or natural-compressor wire as ONE contiguous record, the dense quantizers' counterpart of the
 * stacked record above: what a message carries in place of the decoded vector compressVector returns
 * (compressors.py:357 / 394 standard / natural dithering, 302-325 the natural compressor).
 * `format`: FLC_Q_STANDARD_DITHER or FLC_Q_NATURAL_DITHER with bits in {2, 4, 8} (the quantizer codec's code width), or
 * FLC_WIRE_NATURAL with bits = 16 (the natural compressor's uint16 codes; `levels` is then ignored).
 * Returns the record size (a multiple of 256 B; 0 for bad arguments: another format, bits that do not match it,
 * n < 1 or n >= 2^31) and, if offsets != NULL, the byte offsets of offsets[0] the norm (fp32; unused by the natural
 * compressor) and offsets[1] the codes (16-B aligned; ceil(n * bits / 8) bytes, 2n for the natural compressor).  The
 * layout depends on (n, format, bits) only, so a [clients, stride] block moves as one piece.  The encoders write a
 * record when given those pointers inside it: flc_quant_encode (norms = the record's norm field, written by
 * flc_quant_norm or by the caller), flc_quant_encode_auto with out == NULL, flc_quant_encode_round (a round's records
 * in one call), flc_natural_encode. */
enum flc_dense_wire_format { FLC_WIRE_NATURAL = 2 /* beside FLC_Q_STANDARD_DITHER = 0, FLC_Q_NATURAL_DITHER = 1 */ };
size_t flc_dense_wire_layout(int64_t n, int format, int bits, int64_t* offsets);
/* flc_stacked_fold_wires' contract over dense records (the server's weighted aggregation, nodes.py:1165-1180 /
 * _fedopt.py:202-208, fused with the decode of compressors.py:357 / 394 / 302-325):
 *   out = (accumulate ? out : +0);  for c = 0 .. n_wires-1:  out = fmaf(weights[c], decode(record slots[c]), out)
 * elementwise, in that order — bit-identical to n_wires flc_quant_decode(row_weights = w_c, accumulate = 1) calls
 * (flc_natural_decode(weight = w_c, accumulate = 1) for FLC_WIRE_NATURAL) on a zeroed (or the given) out: a norm that is
 * 0, +-inf, NaN or negative decodes code 0 to +0 and every other code to NaN, a negative zero level to -0.  One pass
 * over out; the records' codes are read once (bits / 32 of the dense vectors' bytes).  wires: records of `stride`
 * bytes (>= flc_dense_wire_layout(n, format, bits), a 16-B multiple), record index slots[c] holds client c; slots and
 * weights are HOST arrays; more than 64 records chain launches.  FLC_EINVAL (nothing launched): a null pointer,
 * bits that do not match the format, levels that do not fit bits (1 <= levels < 2^(bits-1)), n >= 2^31, a short or
 * misaligned stride, a negative slot. */
int flc_fold_dense_wires(const void* wires, int64_t stride, const int32_t* slots, const float* weights, int n_wires,
                         int64_t n, int format, int levels, int bits, int accumulate, float* out, void* stream);
/* flc_fedopt_fold_records' contract over dense records (replaces FedOptServer.update, _fedopt.py:196-240, when each
 * client message carries its delta as a dense record in place of compressors.py:357 / 394 / 302-325's decoded vector):
 *   a = delta * beta0;  for c = 0 .. n_records-1:  a = fmaf(weights[c], decode(records[c]), a);  delta = a;
 *   then, if theta != NULL, the optimiser's step (avg / adagrad / yogi / adam, as flc_model_fold).
 * Bit-identical to decoding every record densely (flc_quant_decode / flc_natural_decode) and running flc_model_fold
 * with init_mode 0 and the step.  Arguments as flc_fedopt_fold_records', (format, levels, bits) as above. */
int flc_fedopt_fold_dense_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                  int format, int levels, int bits, float* const* delta, float* const* theta,
                                  float* const* v, const int64_t* sizes, int n_tensors, float beta0, int opt,
                                  double lr, double beta2, double tau, void* stream);
/* flc_fold_record_groups' contract over dense records (add_parameters' in-place accumulation per group,
 * nodes.py:1116-1132, of messages that carry compressors.py:357 / 394 / 302-325's codes): bit-identical to decoding
 * every record densely and calling flc_weighted_sum(init_mode 2) per group and tensor.  Arguments, chaining and
 * FLC_EINVAL cases as flc_fold_record_groups', (format, levels, bits) as above. */
int flc_fold_dense_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                 int n_records, int64_t n, int format, int levels, int bits,
                                 float* const* dsts /* [n_groups][n_tensors] */, int n_groups, const int64_t* sizes,
                                 int n_tensors, void* stream);

/* ------------------------------------------------------------------ mixed rounds (every record its own codec)
 * A round whose clients chose different codecs — another K, another code width, another record kind, or a client that
 * sends the decoded vector compressVector returns (compressors.py:267-410) — in ONE pass: each record carries its own
 * descriptor in parallel HOST arrays of n_records entries,
 *   records[c]  device pointer to the record, 16-B aligned; for FLC_REC_FLAT the fp32 vector of n elements
 *   kinds[c]    flc_record_kind: FLC_REC_STACKED (flc_stacked_wire_layout(n, ks[c]), levels[c] in [1, 127]),
 *               FLC_REC_SPARSE (flc_sparse_wire_layout(n, ks[c])), FLC_REC_DENSE (flc_dense_wire_layout(n, formats[c],
 *               bits[c]) with levels[c], as flc_fold_dense_wires takes them), FLC_REC_FLAT
 *   ks[c]       the K of a stacked or sparse record, in [1, n]; ignored otherwise
 *   formats[c], levels[c], bits[c]   a dense record's; levels[c] a stacked record's too; ignored otherwise.
 * Every element follows  a = init;  for c in message order:  a = fmaf(w_c, v_c[e], a)  with v_c[e] what record c's own
 * decoder gives at e (stacked_dequant of the code byte, the sparse value, the dithering level times the norm, the
 * natural compressor's power of two, the flat vector's element; +0 where a stacked or sparse record has no entry):
 * bit-identical to decoding every record into a zeroed vector (flc_stacked_decode_tiled / flc_sparse_decode_tiled /
 * flc_quant_decode / flc_natural_decode) and running the dense entry point named below — -0 accumulators, weights of
 * either sign or zero, subnormal products, a norm that is 0, +-inf, NaN or negative (code 0 -> +0, any other code ->
 * NaN) and empty tiles included.  One wave per FLC_TILE tile keeps the accumulator in registers and walks the records in
 * message order as runs of one class (stacked / sparse entries scattered through an LDS tile; dense codes of one width;
 * flat vectors), every tile pointer clamped to the record's own k.  Launches chain per 64 records (and per 8 distinct
 * (format, levels, bits) / stacked levels), each continuing from the stored results.
 * FLC_EINVAL (nothing launched): a null table or entry, an unknown kind, a record that is not 16-B aligned, k outside
 * [1, n] (stacked, sparse), levels outside [1, 127] (stacked), a (format, levels, bits) flc_fold_dense_wires refuses,
 * n >= 2^31, and every refusal of the uniform counterpart. */
enum flc_record_kind { FLC_REC_STACKED = 0, FLC_REC_SPARSE = 1, FLC_REC_DENSE = 2, FLC_REC_FLAT = 3 };
/* flc_fedopt_fold_records' contract over a mixed round (replaces FedOptServer.update, _fedopt.py:196-240, when the
 * clients' messages carry their deltas under different codecs):
 *   a = delta * beta0;  for c = 0 .. n_records-1:  a = fmaf(weights[c], decode_c(records[c]), a);  delta = a;
 *   then, if theta != NULL, the optimiser's step (avg / adagrad / yogi / adam, as flc_model_fold), on the last launch.
 * Bit-identical to decoding every record and running flc_model_fold with init_mode 0 and the step.  Arguments as
 * flc_fedopt_fold_records', the descriptor arrays in place of (k, levels). */
int flc_fedopt_fold_mixed_records(const void* const* records, const float* weights, int n_records, int64_t n,
                                  const int32_t* kinds, const int64_t* ks, const int32_t* formats,
                                  const int32_t* levels, const int32_t* bits, float* const* delta, float* const* theta,
                                  float* const* v, const int64_t* sizes, int n_tensors, float beta0, int opt, double lr,
                                  double beta2, double tau, void* stream);
/* flc_fold_record_groups' contract over a mixed round (add_parameters' in-place accumulation per group,
 * nodes.py:1116-1132; SCAFFOLD's two vectors, scaffold/_scaffold.py:160-169 over the messages of _scaffold.py:210-222,
 * IFCA's clusters, ifca/_ifca.py:186-195 over the messages of _ifca.py:228-240): the records of a group, and the
 * groups, may differ in codec.  Bit-identical to decoding every record and calling flc_weighted_sum(init_mode 2) per
 * group and tensor.  Arguments, chaining and FLC_EINVAL cases as flc_fold_record_groups', the descriptor arrays in place
 * of (k, levels). */
int flc_fold_mixed_record_groups(const void* const* records, const float* weights, const int32_t* group_of,
                                 int n_records, int64_t n, const int32_t* kinds, const int64_t* ks,
                                 const int32_t* formats, const int32_t* levels, const int32_t* bits,
                                 float* const* dsts /* [n_groups][n_tensors] */, int n_groups, const int64_t* sizes,
                                 int n_tensors, void* stream);
/* flc_avg_and_gradient_records' contract over a mixed round of gradients (replaces fedprox/_fedprox.py:163-167 and
 * 208-217, fedpd/_fedpd.py:197-202 and 252-275, proxskip/_proxskip.py:212-216 and 265-276, pfedmac/_pfedmac.py:158-162
 * and 203-212, nodes.py:1134-1180, when the messages carry their gradients under different codecs):
 *   params[t] = params[t] * inertia, then fmaf(w_params[m], param_srcs[m * n_tensors + t], .) for m in order
 *               (param_srcs == NULL: params is neither read nor written — update_gradients alone);
 *   grads[t]  = +0, then fmaf(w_grads[m], decode_m(grad_records[m])[e], .) for m in order;
 * bit-identical to decoding every record and calling flc_avg_and_gradients.  Arguments and chaining as
 * flc_avg_and_gradient_records', the descriptor arrays in place of (k, levels). */
int flc_avg_and_gradient_mixed_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                       const void* const* grad_records, const float* w_params, const float* w_grads,
                                       int n_src, int64_t n, const int32_t* kinds, const int64_t* ks,
                                       const int32_t* formats, const int32_t* levels, const int32_t* bits,
                                       const int64_t* sizes, int n_tensors, float inertia, void* stream);

/* ------------------------------------------------------------------ multi-GPU exchange (RCCL over xGMI)
 * For callers outside torch; one process per GPU.  RCCL is the NCCL API on ROCm, looked
 * up on first use: $FLC_RCCL_LIB if set, else an RCCL already loaded in the process (inside a torch process, torch's
 * own, whatever its soname), else librccl.so.1.  The round's exchange is either
 *   flc_rccl_reduce: sum of the ranks' fp32 partial sums to `root` (the dense round; the cross-rank summation order is
 *     RCCL's, so the result matches one device to 1e-6 * sum|w_i d_i|), or
 *   flc_rccl_allgather: every rank's block of packed wire records to every rank (recv = nranks * bytes_per_rank, rank
 *     order), then flc_stacked_fold_wires over all clients in client order (bit-identical to one device at any N).
 * flc_comm_unique_id on one rank, its flc_comm_id_bytes() bytes shipped to the others out of band, then
 * flc_comm_init on every rank (collective; `device` >= 0: the communicator's HIP device, made current for the call
 * only — the calling thread's current device is restored).  Collectives are
 * stream-ordered and asynchronous like every other call. */
size_t flc_comm_id_bytes(void);
/* Where the RCCL symbols were found on first use (loads RCCL if not yet loaded): "env" (FLC_RCCL_LIB), "global" (the
 * process's global namespace, e.g. torch's RCCL loaded RTLD_GLOBAL), "loaded" (an already-loaded librccl* object),
 * "dlopen" (librccl.so.1), or "none" (not found; every flc_comm_* / flc_rccl_* call then fails with FLC_ECOMM). */
const char* flc_comm_rccl_origin(void);
int flc_comm_unique_id(void* id_out);
int flc_comm_init(const void* id, int nranks, int rank, int device, void** comm_out);
int flc_comm_size(void* comm, int* nranks, int* rank);
int flc_comm_destroy(void* comm);
int flc_rccl_reduce(const float* send, float* recv, int64_t n, int root, void* comm, void* stream);
int flc_rccl_allreduce(const float* send, float* recv, int64_t n, void* comm, void* stream);
int flc_rccl_allgather(const void* send, void* recv, int64_t bytes_per_rank, void* comm, void* stream);

/* ------------------------------------------------------------------ adaptive random compressor
 * (compressors.py:297-301): ind = np.random.choice(np.arange(n), size=1, p=|x| / sum|x|); out = 0,
 * out[ind] = x[ind].  Bit-exact with numpy: S in numpy's order (8192-element buffers folded in order, each
 * by pairwise_sum), p = fp32(|x| / S), the strictly sequential fp64 cumsum, cdf / cdf[-1] and
 * searchsorted(u, side='right').  Two calls, because numpy validates p before it draws u:
 *   flc_adaptive_prepare writes the check to *status (device int32): 0 ok, 1 "probabilities contain NaN",
 *     2 "probabilities do not sum to 1" (|sum p - 1| > 3.4526698e-4);
 *   flc_adaptive_select (same stream, same x and workspace) takes u in [0, 1) (compat mode: the legacy
 *     np.random.random_sample() draw, see flc_mt_random_doubles) and writes out and *index (device int64);
 *     it writes nothing when the status is non-zero.  x must be 16-byte aligned; 0 < n < 2^31. */
size_t flc_adaptive_workspace_size(int64_t n);
int flc_adaptive_prepare(const float* x, int64_t n, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int flc_adaptive_select(const float* x, int64_t n, double u, int64_t* index, float* out, void* ws, size_t ws_bytes,
                        void* stream);
/* the same on a float64 x (the reference keeps it float64): S an fp64 sum of the same buffers and trees, p = |x| / S
 * in fp64, the tolerance sqrt(eps64) = 1.4901161e-8; same workspace size */
int flc_adaptive_prepare_f64(const double* x, int64_t n, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int flc_adaptive_select_f64(const double* x, int64_t n, double u, int64_t* index, double* out, void* ws,
                            size_t ws_bytes, void* stream);
/* the last select's walk on this workspace, as 4 device int32: special chunks (a binade crossing or near an edge),
 * special maps taken, chunks re-run sequentially, 1 if the exact sequential chain ran instead (diagnostics: the
 * result never depends on them) */
int flc_adaptive_stats(const void* ws, size_t ws_bytes, int64_t n, int32_t* stats, void* stream);

/* the stacked encoder fused with the client delta (f1): x = local - global formed in the encoder's HBM pass
 * (FedOptClient.communicate, _fedopt.py:294-297: clone + add_(alpha=-1) per parameter tensor, then the flatten the
 * codec's flat input needs, nodes.py:300-302) — the flat delta is never written.  local, global and sizes are HOST
 * arrays (of device pointers / element counts, like flc_delta_flatten); tensors must be 4-B aligned; the element
 * order is the concatenation.  The output is bit-identical to flc_stacked_encode_tiled of the flattened delta.
 * The workspace holds the encoder's plus a tensor table (copied from the host arrays, so not graph-capturable). */
size_t flc_stacked_encode_delta_workspace_size(int64_t n, int64_t k, int n_tensors);
int flc_stacked_encode_delta(const float* const* local, const float* const* global, const int64_t* sizes,
                             int n_tensors, int64_t k, int levels, uint64_t seed, uint64_t counter, int32_t* idx,
                             uint8_t* codes, float* norm, uint32_t* tiles, void* ws, size_t ws_bytes, void* stream);

/* the stacked encoder over many clients of one round in one launch (the clients a rank encodes before the fold,
 * nodes.py:706-713 / _fedopt.py:295-308 once per client): client c's packet is bit-identical to
 * flc_stacked_encode_tiled(xs[c], n, k, levels, seeds[c], counter, ...) into idx[c], codes[c], norm[c], tiles[c]
 * (tiles may be NULL: no tile pointers; the four pointers of a wire record make client c's record).  All clients
 * have the same n and k; xs, seeds, idx, codes, norm and tiles are HOST arrays of n_clients entries (device
 * pointers / seeds).  The device's CUs are split among up to #CU clients per launch (one independent select of
 * #CU / clients blocks each, its own header, no exchange across clients); more clients run in further launches on
 * the stream.  The workspace is used afresh by every call (its headers are zeroed in the stream), so it needs no
 * zeroing by the caller, but must not be shared with single-client calls.  flc_topk_status(ws) reports the errors
 * of every client's select.  The client table is copied from the host arrays into the workspace, so the call is not
 * graph-capturable (like flc_stacked_encode_delta). */
size_t flc_stacked_encode_batch_workspace_size(int64_t n, int64_t k, int n_clients);
int flc_stacked_encode_batch(const float* const* xs, int n_clients, int64_t n, int64_t k, int levels,
                             const uint64_t* seeds, uint64_t counter, int32_t* const* idx, uint8_t* const* codes,
                             float* const* norm, uint32_t* const* tiles, void* ws, size_t ws_bytes, void* stream);

/* plain top-k of many clients in one launch (compressors.py:293-296 per client): client c's (idx, val, tiles) equal
 * flc_topk_encode_tiled(xs[c], n, k, ...); arrays and workspace as in flc_stacked_encode_batch (the two share a
 * workspace size).  The three pointers inside a sparse record (flc_sparse_wire_layout(n, k)) make client c's record: a
 * round's records in one call. */
size_t flc_topk_encode_batch_workspace_size(int64_t n, int64_t k, int n_clients);
int flc_topk_encode_batch(const float* const* xs, int n_clients, int64_t n, int64_t k, int32_t* const* idx,
                          float* const* val, uint32_t* const* tiles, void* ws, size_t ws_bytes, void* stream);

/* the batched encoder fused with the clients' deltas (f1 for a round's clients): client c's packet is
 * bit-identical to flc_stacked_encode_delta(local + c * n_tensors, global, sizes, ...) with seeds[c].  local is a HOST
 * array of n_clients * n_tensors device pointers, client-major (client c's tensors at [c * n_tensors, (c+1) *
 * n_tensors)); global (n_tensors, shared by every client: the round's global model) and sizes are HOST arrays as in
 * flc_stacked_encode_delta; outputs, seeds and the workspace as in flc_stacked_encode_batch. */
size_t flc_stacked_encode_delta_batch_workspace_size(int64_t n, int64_t k, int n_clients, int n_tensors);
int flc_stacked_encode_delta_batch(const float* const* local, const float* const* global, const int64_t* sizes,
                                   int n_tensors, int n_clients, int64_t k, int levels, const uint64_t* seeds,
                                   uint64_t counter, int32_t* const* idx, uint8_t* const* codes, float* const* norm,
                                   uint32_t* const* tiles, void* ws, size_t ws_bytes, void* stream);

/* a round's messages in one batched encode, each with its own Philox (seed, counter) — sampled clients, whose
 * compressors have advanced differently — and the send counts made by the encode itself: client c's packet is
 * bit-identical to flc_stacked_encode_tiled(xs[c], n, k, levels, seeds[c], counters[c], ...) (the delta form: to
 * flc_stacked_encode_delta of client c's tensors), and counts[c] (counts may be NULL: no counts; else a HOST array
 * of n_clients device pointers, none NULL) receives what flc_count_nonzero_at_batch would write for the packet: one
 * device int64, the kept entries with !(value == 0) (a kept NaN counts), zeroed and added to in the stream by the
 * encode's own launches.  counters is a HOST array of n_clients entries (NULL: FLC_EINVAL).  Everything else as in
 * flc_stacked_encode_batch / flc_stacked_encode_delta_batch, which are the all-counters-equal, no-count case of the
 * same code; the workspace is flc_stacked_encode_batch_workspace_size(n, k, n_clients) for the flat form and
 * flc_stacked_encode_delta_batch_workspace_size(n, k, n_clients, n_tensors) for the delta form.  The flat form may
 * be captured into a graph (its table then travels in kernel arguments). */
int flc_stacked_encode_round(const float* const* xs, int n_clients, int64_t n, int64_t k, int levels,
                             const uint64_t* seeds, const uint64_t* counters, int32_t* const* idx,
                             uint8_t* const* codes, float* const* norm, uint32_t* const* tiles, int64_t* const* counts,
                             void* ws, size_t ws_bytes, void* stream);
int flc_stacked_encode_delta_round(const float* const* local, const float* const* global, const int64_t* sizes,
                                   int n_tensors, int n_clients, int64_t k, int levels, const uint64_t* seeds,
                                   const uint64_t* counters, int32_t* const* idx, uint8_t* const* codes,
                                   float* const* norm, uint32_t* const* tiles, int64_t* const* counts, void* ws,
                                   size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ top-k by magnitude (selection order)
 * compressors.py:293-296 keeps the K largest *signed* values (`out[np.argsort(out)[:-K]] = 0`); that is
 * FLC_ORDER_SIGNED, the order of every entry point above.  FLC_ORDER_MAGNITUDE keeps the K largest |x| instead (the
 * top-k of Aji & Heafield, Deep Gradient Compression and Stich et al.): the kept index set is exactly the signed
 * select's on |x| — a NaN of either sign is the largest magnitude, -0 == +0, +v and -v tie, and among the entries tied
 * with the K-th largest magnitude the highest indices are kept — and each kept value is x's own, sign included, bit
 * for bit.  The stacked pipeline's second stage is unchanged and runs on the kept values: norm = max|kept| = max|x|,
 * the Philox word by element id, the code's sign bit the kept value's own sign.  flc_topk_select_stats reports the
 * signed select's diagnostics on |x|; flc_topk_select_plan and every workspace size do not depend on the order.
 *
 * Each `_ord` entry is the entry of the same name with `order` after k; the entries above are its order = 0 case.
 * Any other order returns FLC_EINVAL and launches nothing. */
enum { FLC_ORDER_SIGNED = 0, FLC_ORDER_MAGNITUDE = 1 };
/* compressors.py:293-296 by |x| (order 1): the sparse record of flc_topk_encode_tiled; tiles may be NULL */
int flc_topk_encode_tiled_ord(const float* x, int64_t n, int64_t k, int order, int32_t* idx, float* val,
                              uint32_t* tiles, void* ws, size_t ws_bytes, void* stream);
/* compressors.py:293-296 by |x| per client: flc_topk_encode_batch */
int flc_topk_encode_batch_ord(const float* const* xs, int n_clients, int64_t n, int64_t k, int order,
                              int32_t* const* idx, float* const* val, uint32_t* const* tiles, void* ws, size_t ws_bytes,
                              void* stream);
/* compressors.py:293-296 by |x|, then 327-365 on the kept values: flc_stacked_encode_tiled; tiles may be NULL */
int flc_stacked_encode_tiled_ord(const float* x, int64_t n, int64_t k, int order, int levels, uint64_t seed,
                                 uint64_t counter, const double* compat_u, int32_t* idx, uint8_t* codes, float* norm,
                                 uint32_t* tiles, void* ws, size_t ws_bytes, void* stream);
/* the same on the client delta local - global formed in the read pass (|local - global|: the magnitude is taken after
 * the subtraction): flc_stacked_encode_delta */
int flc_stacked_encode_delta_ord(const float* const* local, const float* const* global, const int64_t* sizes,
                                 int n_tensors, int64_t k, int order, int levels, uint64_t seed, uint64_t counter,
                                 int32_t* idx, uint8_t* codes, float* norm, uint32_t* tiles, void* ws, size_t ws_bytes,
                                 void* stream);
/* a round's clients in one launch, compressors.py:293-296 by |x| per client: flc_stacked_encode_round and
 * flc_stacked_encode_delta_round (one order for the whole call) */
int flc_stacked_encode_round_ord(const float* const* xs, int n_clients, int64_t n, int64_t k, int order, int levels,
                                 const uint64_t* seeds, const uint64_t* counters, int32_t* const* idx,
                                 uint8_t* const* codes, float* const* norm, uint32_t* const* tiles,
                                 int64_t* const* counts, void* ws, size_t ws_bytes, void* stream);
int flc_stacked_encode_delta_round_ord(const float* const* local, const float* const* global, const int64_t* sizes,
                                       int n_tensors, int n_clients, int64_t k, int order, int levels,
                                       const uint64_t* seeds, const uint64_t* counters, int32_t* const* idx,
                                       uint8_t* const* codes, float* const* norm, uint32_t* const* tiles,
                                       int64_t* const* counts, void* ws, size_t ws_bytes, void* stream);
/* compressors.py:293-296 by |x| in float64: flc_topk_dense_f64 (declared with the float64 forms below) */
int flc_topk_dense_f64_ord(const double* x, int64_t n, int64_t k, int order, double* out, void* ws, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------ other compressors
 * identical (compressors.py:273-275): out = +x;  lazy (276-283): out = x / p (fp32 division);
 * rand-k (284-292): out = 0, out[idx[j]] = scale * x[idx[j]] (idx in any order, unique). */
int flc_copy(const float* x, int64_t n, float* out, void* stream);
int flc_scale_div(const float* x, int64_t n, float p, float* out, void* stream);
int flc_randk_apply(const float* x, int64_t n, const int32_t* idx, int64_t k, float scale, float* out,
                    void* stream);
/* rand-k index set in philox mode (no host round trip): keys[e] = the Philox word of element e >> 2, as a positive
 * fp32 bit pattern; the K largest keys (flc_topk_encode_tiled on keys) are a uniformly random K-subset, ascending.
 * keys must be 16-B aligned. */
int flc_randk_keys(int64_t n, uint64_t seed, uint64_t counter, float* keys, void* stream);
/* rand-k's kept values without the dense vector (compressors.py:289-291 at the kept indices only): val[j] = scale *
 * x[idx[j]], one fp32 multiply — bit-equal to what flc_randk_apply scatters to out[idx[j]]; the val field of a sparse
 * record (flc_sparse_wire_layout).  An index outside [0, n) writes +0 and reads nothing.  FLC_EINVAL: a null pointer,
 * n < 1, k < 0, n or k >= 2^31.  k == 0: nothing launched. */
int flc_sparse_gather(const float* x, int64_t n, const int32_t* idx, int64_t k, float scale, float* val, void* stream);

/* ------------------------------------------------------------------ float64 inputs (f64.hip)
 * The reference runs every compressor on whatever dtype x has (compressors.py:267-410): on a float64 vector
 * ``np.zeros_like(x)``, ``x / P``, ``D / K * x[i]``, ``math.log2(abs(x[i]))``, ``np.linalg.norm(x, p)`` and the level
 * arithmetic all stay float64.  These are the float64 forms of the entry points above (a fp64 vector in, a fp64
 * vector out; buffers 16-B aligned).  Uniforms as for float32: compat_u = one double per consumer in index order
 * (the reference's random.random() calls; count them with flc_count_consumers_f64), or Philox (compat_u == NULL).
 *   flc_copy_f64 / flc_scale_div_f64 / flc_randk_apply_f64   IDENTICAL, LAZY (x / p), RANDK (scale * x[idx[j]])
 *   flc_natural_f64        natural compression (compressors.py:302-318): codes (uint16 per element: 0 zero,
 *                          0x7fff NaN, else sign << 15 | (e + 1075)) and / or the decoded vector; either may be NULL
 *   flc_quant_norm_f64     p = inf: max |x|; p = 2: sqrt of an fp64 sum of squares (fixed order)
 *   flc_quant_f64          standard / natural dithering (compressors.py:339-357, 376-393) with the given norm:
 *                          8-bit codes (sign << 7 | level) and / or the decoded vector lv * sign * norm; nnz =
 *                          count(x != 0) when non-NULL.  A norm that is not a positive finite double encodes as the
 *                          float32 codec's does (code 0 for x == 0, else 1) and decodes code 0 to +0, any other to NaN
 *   flc_natural_decode_f64 / flc_quant_decode_f64   the decoded vectors of those codes (natural: fields 1..2099,
 *                          2^(field - 1075), 2^1024 being +-inf; dithering: the level tables of flc_quant_kind in fp64,
 *                          standard lv = i * (1 / levels) with lv[levels] = 1)
 *   flc_topk_dense_f64     out = x on the K largest (ties: the highest indices), +0 elsewhere (293-296), 0 < k < n
 * Workspace: flc_f64_workspace_size(n, k) bytes (compat mode, the norm and top-k with that k; not needed by the
 * element-wise forms or by the Philox-mode encoders). */
int flc_copy_f64(const double* x, int64_t n, double* out, void* stream);
int flc_scale_div_f64(const double* x, int64_t n, double p, double* out, void* stream);
int flc_randk_apply_f64(const double* x, int64_t n, const int32_t* idx, int64_t k, double scale, double* out,
                        void* stream);
size_t flc_f64_workspace_size(int64_t n, int64_t k);  /* k: flc_topk_dense_f64's k, else 0 */
int flc_count_consumers_f64(const double* x, int64_t n, const double* norm, int64_t* count, void* ws, size_t ws_bytes,
                            void* stream);
int flc_natural_f64(const double* x, int64_t n, uint64_t seed, uint64_t counter, const double* compat_u,
                    uint16_t* codes, double* out, void* ws, size_t ws_bytes, void* stream);
int flc_natural_decode_f64(const uint16_t* codes, int64_t n, double* out, void* stream);
int flc_quant_norm_f64(const double* x, int64_t n, int norm_p, double* norm, void* ws, size_t ws_bytes, void* stream);
int flc_quant_f64(const double* x, int64_t n, int kind, int levels, const double* norm, uint64_t seed,
                  uint64_t counter, const double* compat_u, uint8_t* codes, double* out, int64_t* nnz, void* ws,
                  size_t ws_bytes, void* stream);
int flc_quant_decode_f64(const uint8_t* codes, int64_t n, int kind, int levels, const double* norm, double* out,
                         void* stream);
int flc_topk_dense_f64(const double* x, int64_t n, int64_t k, double* out, void* ws, size_t ws_bytes, void* stream);
/* the float64 workspace's sticky error word (4: flc_topk_dense_f64's grid-synchronised select timed out at a barrier,
 * i.e. its blocks were not all resident — the output of that call is invalid), as flc_topk_status reports the float32
 * encoders'; copied to *err_out (device uint64), zeroed with reset */
int flc_f64_status(void* ws, uint64_t* err_out, int reset, void* stream);
/* the select state the last flc_topk_dense_f64(x, n, k, ...) left in `ws` and that call's band geometry, copied to
 * the HOST array out[FLC_STATS64_WORDS]; synchronises the stream once (diagnostics, as flc_topk_select_stats) */
enum {
  FLC_STATS64_FB = 0,    /* 1: T came from the exact passes over x */
  FLC_STATS64_ERR = 1, FLC_STATS64_NBIN = 2, FLC_STATS64_T = 3, FLC_STATS64_NEED = 4, FLC_STATS64_TIES = 5,
  FLC_STATS64_ITHR = 6,
  FLC_STATS64_S = 7, FLC_STATS64_R_LO = 8, FLC_STATS64_R_HI = 9, /* sample keys, floor / ceiling ranks */
  FLC_STATS64_ON = 10,   /* 1: the sampled band runs for this (n, k) */
  FLC_STATS64_SAMPLE = 11, /* the sample size cap */
  FLC_STATS64_WORDS = 16
};
int flc_topk_stats_f64(const void* ws, size_t ws_bytes, int64_t n, int64_t k, int64_t* out, void* stream);

/* ------------------------------------------------------------------ client delta
 * FedOptClient.communicate (_fedopt.py:294-297): delta_t = clone(local_t) then add_(global_t, alpha=-1), i.e.
 * local_t - global_t per element, for each parameter tensor t; plus the flatten the codec's flat input needs.
 * out[off_t + i] = local[t][i] - global[t][i], off_t = sizes[0] + ... + sizes[t-1].  local, global and sizes are
 * HOST arrays (of device pointers / element counts); empty tensors are allowed. */
int flc_delta_flatten(const float* const* local, const float* const* global, const int64_t* sizes, int n_tensors,
                      float* out, void* stream);
/* the number of nonzero deltas local - global (as flc_delta_flatten forms them; NaN counts) at the k flat indices idx
 * of the concatenation — the count a standard-dithering stage's send statistics take from its input (compressors.py
 * 339-365: one entry per nonzero element) when the delta itself is never formed (flc_stacked_encode_delta).  count: one
 * device int64, written stream-ordered. */
int flc_delta_count_nonzero_at(const float* const* local, const float* const* global, const int64_t* sizes,
                               int n_tensors, const int32_t* idx, int64_t k, int64_t* count, void* stream);
/* the same count (compressors.py:339-365, one send entry per nonzero dithering input) for many clients whose deltas
 * are already flat — a round's deferred compressed messages: counts[c] = the number of nonzero xs[c][idx[c][j]], j < k
 * (NaN counts), every x of n elements, every idx of k in-range indices (a stacked record's kept indices).  xs, idx
 * and counts are HOST arrays of device pointers; each count one device int64, written stream-ordered. */
int flc_count_nonzero_at_batch(const float* const* xs, const int32_t* const* idx, int n_clients, int64_t n,
                               int64_t k, int64_t* const* counts, void* stream);

/* ------------------------------------------------------------------ error feedback
 * A client's residual memory e for a biased compressor (fl_sim_amd/feedback.py): per round and message vector
 *   a = fp32(e + fp32(local - cached));  c = compressors(a);  e' = fp32(a - c)
 * with e the flat fp32 vector the encoders read as their input (zero at the start).
 *
 * flc_ef_accumulate: e[off_t + i] = e[off_t + i] + (local[t][i] - global[t][i]) in place, off_t = sizes[0] + ... +
 * sizes[t-1]: two roundings per element, nothing contracted; global == NULL: e[off_t + i] + local[t][i] (a gradient
 * list).  Bit-identical to flc_delta_flatten into a fresh vector d followed by e = e + d; NaN, +-inf, -0 and denormals
 * as IEEE addition gives them.  local, global and sizes are HOST arrays (as flc_delta_flatten's); empty tensors are
 * allowed; more than 48 tensors chain launches.  FLC_EINVAL (nothing launched): null tables, a negative size, a null
 * pointer for a non-empty tensor (a null e included). */
int flc_ef_accumulate(const float* const* local, const float* const* global /* NULL: nothing subtracted */,
                      const int64_t* sizes, int n_tensors, float* e, void* stream);
/* The residual of a round's stacked records: for every client c and entry j < k of records[c] (the
 * flc_stacked_wire_layout(n, k) layout), es[c][idx[j]] -= decode(codes[j]) with the record's norm — the decoders' own
 * dequantisation.  Bit-identical to flc_stacked_decode_tiled(weight 1, accumulate 0) into a zeroed c_dense followed by
 * es[c] = es[c] - c_dense: an element no entry names is untouched (x - (+0) == x, a -0 included), a zero code leaves
 * its element as it is, a norm that is 0, +-inf or NaN turns the elements of nonzero codes into NaN.  One launch for
 * up to 32 clients (more chain); a record's indices are unique, so nothing is atomic.  An entry whose index lies
 * outside [0, n) is skipped: a record that a failed encode left behind writes nothing outside its memory.  records and
 * es are HOST arrays of device pointers.  FLC_EINVAL (nothing launched): n_clients < 0, null tables with n_clients >
 * 0, a null or not 16-B aligned record, a null memory, the same memory for two clients, n or k >= 2^31, k > n, levels
 * outside [1, 127].  n_clients == 0 or k == 0: the tables are checked, nothing is launched. */
int flc_ef_residual_round(const void* const* records, float* const* es, int n_clients, int64_t n, int64_t k,
                          int levels, void* stream);
/* The residual of a round's sparse records (flc_sparse_wire_layout(n, k): top-k's and rand-k's messages,
 * compressors.py:284-296): es[c][idx[j]] -= val[j] for every client c and entry j < k.  Bit-identical to
 * flc_sparse_decode_tiled(scale 1, weight 1, accumulate 0) into a zeroed c_dense followed by flc_ef_residual_dense: an
 * element no entry names keeps its bits (a -0 included).  The launch bound (32 clients, more chain), the skipped
 * out-of-range indices and the FLC_EINVAL cases are flc_ef_residual_round's, without levels. */
int flc_ef_residual_sparse_round(const void* const* records, float* const* es, int n_clients, int64_t n, int64_t k,
                                 void* stream);
/* e[i] = e[i] - c[i], i < n: the residual of a message that carries its decoded flat vector c (every compressor but
 * the stacked pipeline).  16-B accesses when both pointers are 16-B aligned, 4-B otherwise; the same bits either way.
 * FLC_EINVAL: n < 0, a null pointer with n > 0, e == c. */
int flc_ef_residual_dense(float* e, const float* c, int64_t n, void* stream);

/* ------------------------------------------------------------------ aggregation
 * weighted sum of client tensors into dst, in message order, one fmaf per message per element:
 *   init_mode 0: dst = dst * beta   (avg_parameters' inertia, nodes.py:1158-1159;
 *                                   FedOptServer.update's betas[0], _fedopt.py:203)
 *   init_mode 1: dst = 0            (update_gradients, nodes.py:1173-1174)
 *   init_mode 2: dst unchanged      (add_parameters, nodes.py:1131-1132)
 *   then for m in 0..n_src-1: dst = fmaf(weights[m], srcs[m][i], dst)   (nodes.py:1132, 1178; _fedopt.py:204-208)
 * srcs and weights are HOST arrays of device pointers / fp32 weights (n_src >= 0). */
int flc_weighted_sum(const float* const* srcs, const float* weights, int n_src, int64_t n, int init_mode,
                     float beta, float* dst, void* stream);
/* a whole model in ONE launch (a model is many small tensors; two launches per tensor are launch-bound): for each
 * tensor t, dst[t] = init(dst[t]) then fmaf(weights[m], srcs[m * n_tensors + t], .) for m in message order — exactly
 * flc_weighted_sum per tensor — and, with theta != NULL, flc_fedopt_step on (theta[t], dst[t], v[t]) with the folded
 * dst[t] as the delta: FedOptServer.update in one pass (_fedopt.py:196-265).  Host arrays of device pointers;
 * n_src <= 16 (a longer message list: flc_weighted_sum, which chains); 16 tensors per launch, more in further launches
 * (tensor order).  v may be NULL for opt = avg. */
int flc_model_fold(float* const* dst, const float* const* srcs, const float* weights, int n_src, const int64_t* sizes,
                   int n_tensors, int init_mode, float beta, float* const* theta, float* const* v, int opt, double lr,
                   double beta2, double tau, void* stream);
/* avg_parameters (nodes.py:1134-1163) and update_gradients (nodes.py:1165-1180) of one round in ONE launch — what
 * the variance-reduced servers run back to back (fedprox/_fedprox.py:163-167, fedpd/_fedpd.py:197-202,
 * proxskip/_proxskip.py:212-216, pfedmac/_pfedmac.py:158-162):
 *   params[t] = params[t] * inertia, then fmaf(w_params[m], param_srcs[m][t], .) for m in order;
 *   grads[t]  = +0, then fmaf(w_grads[m], grad_srcs[m][t], .) for m in order;
 * bit-identical to flc_model_fold(init 0, beta = inertia) of the parameters followed by flc_model_fold(init 1) of the
 * gradients.  param_srcs / grad_srcs: HOST arrays [n_src][n_tensors] of device pointers; params / grads / sizes HOST
 * arrays of n_tensors; more than 16 messages chain launches (each continuing the stored partial results). */
int flc_avg_and_gradients(float* const* params, float* const* grads, const float* const* param_srcs,
                          const float* const* grad_srcs, const float* w_params, const float* w_grads, int n_src,
                          const int64_t* sizes, int n_tensors, float inertia, void* stream);
/* The same round when every message carries its gradients as a packed stacked record (the codec's call site for the
 * variance-reduced algorithms, fl_sim_amd/compressed.py: CompressedGradientsClientMixin; replaces
 * fedprox/_fedprox.py:163-167 and 208-217, fedpd/_fedpd.py:197-202 and 252-275, proxskip/_proxskip.py:212-216 and
 * 265-276, pfedmac/_pfedmac.py:158-162 and 203-212, nodes.py:1134-1180).  Over the flat concatenation of the model's
 * tensors (element e of a record = element e - start_t of tensor t, the order the client flattens its gradient list):
 *   params[t] = params[t] * inertia, then fmaf(w_params[m], param_srcs[m * n_tensors + t], .) for m in order
 *               (exactly flc_avg_and_gradients' parameters; param_srcs == NULL: params is not touched — that form is
 *               update_gradients alone);
 *   grads[t]  = +0, then fmaf(w_grads[m], decode(grad_records[m])[e], .) for m in order;
 * bit-identical to decoding every record densely (flc_stacked_decode_tiled) and calling flc_avg_and_gradients — -0
 * results, empty tiles and weights of either sign or zero included.  One wave per FLC_TILE-element tile decodes the
 * tile's slice of every record into the gradient and folds the same slice of the dense parameter sources.
 * grad_records: HOST array of n_src device pointers to records of the flc_stacked_wire_layout(n, k) layout (16-B
 * aligned); params / grads / sizes: HOST arrays of n_tensors, sizes summing to n.  One launch for n_src <= 16 and
 * n_tensors <= 16; records chain per 64, parameter sources per 16, tensors per 16 (each later launch continues the
 * stored partial results). */
int flc_avg_and_gradient_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                 const void* const* grad_records, const float* w_params, const float* w_grads,
                                 int n_src, int64_t n, int64_t k, int levels, const int64_t* sizes, int n_tensors,
                                 float inertia, void* stream);
/* flc_avg_and_gradient_records' contract when every message carries its gradients as a sparse record
 * (flc_sparse_wire_layout(n, k); replaces the same reference lines: fedprox/_fedprox.py:163-167, fedpd/_fedpd.py:197-202,
 * proxskip/_proxskip.py:212-216, pfedmac/_pfedmac.py:158-162, nodes.py:1134-1180): bit-identical to decoding every
 * record densely (flc_sparse_decode_tiled) and calling flc_avg_and_gradients.  Arguments and chaining as
 * flc_avg_and_gradient_records' without levels; k in [1, n]. */
int flc_avg_and_gradient_sparse_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                        const void* const* grad_records, const float* w_params, const float* w_grads,
                                        int n_src, int64_t n, int64_t k, const int64_t* sizes, int n_tensors,
                                        float inertia, void* stream);
/* flc_avg_and_gradient_records' contract when every message carries its gradients as a dense record
 * (flc_dense_wire_layout(n, format, bits): the dithering quantizers' and the natural compressor's wire; replaces
 * nodes.py:1134-1180 — avg_parameters and update_gradients — over compressors.py:357 / 394 / 302-325's decoded vectors,
 * for fedprox/_fedprox.py:163-167, fedpd/_fedpd.py:197-202, proxskip/_proxskip.py:212-216, pfedmac/_pfedmac.py:158-162):
 *   params[t] = params[t] * inertia, then fmaf(w_params[m], param_srcs[m * n_tensors + t], .) for m in order
 *               (param_srcs == NULL: params is neither read nor written — update_gradients alone);
 *   grads[t]  = +0, then fmaf(w_grads[m], decode(grad_records[m])[e], .) for m in order;
 * bit-identical to decoding every record densely (flc_quant_decode; flc_natural_decode for FLC_WIRE_NATURAL) and calling
 * flc_avg_and_gradients: every element takes every record's fma (a dense record holds a code for every element, so
 * there is no sparse form), a norm that is 0, +-inf, NaN or negative decodes as flc_fold_dense_wires states.  The
 * records' codes are read once (bits / 32 of the decoded vectors' bytes) and no decoded vector is ever written.
 * Arguments and chaining as flc_avg_and_gradient_records' (records per 64, parameter sources per 16, tensors per 16),
 * (format, levels, bits) and their FLC_EINVAL cases as flc_fold_dense_wires'. */
int flc_avg_and_gradient_dense_records(float* const* params, float* const* grads, const float* const* param_srcs,
                                       const void* const* grad_records, const float* w_params, const float* w_grads,
                                       int n_src, int64_t n, int format, int levels, int bits,
                                       const int64_t* sizes, int n_tensors, float inertia, void* stream);
/* FedDyn's and pFedMe's server updates on a whole model, one pass per <= 16 tensors and <= 16 messages
 * (theta = the model, aux = the per-element second state; srcs[m * n_tensors + t] = message m's tensor t):
 *   FLC_SRV_FEDDYN (feddyn/_feddyn.py:172-184): h = aux, for each message in order h = fmaf(c, fl(src - theta0), h)
 *     with c = fp32(-mu / num_clients); with `fold`, theta = the avg_parameters fold of theta0 in the same pass
 *     (init_mode 0: theta0 * inertia first, then fmaf(weights[m], src, .) in order); line 184's result is discarded
 *     by the reference, so nothing follows.  Without `fold` only h is updated (theta read-only: the chained form).
 *   FLC_SRV_PFEDME (pfedme/_pfedme.py:166-175): with `fold`, a = the avg fold of theta0 (init_mode 0, or 2 when the
 *     round has no message: avg_parameters returns early), then theta = fmaf(fp32(1 - c), theta0, fl(a * fp32(c)))
 *     with c = beta; without `fold` (no sources: the fold ran in chained flc_model_fold launches and aux holds the
 *     saved theta0) theta = fmaf(fp32(1 - c), aux, fl(theta * fp32(c))). */
enum flc_server_kind { FLC_SRV_FEDDYN = 1, FLC_SRV_PFEDME = 2 };
int flc_model_fold_server(float* const* theta, float* const* aux, const float* const* srcs, const float* weights,
                          int n_src, const int64_t* sizes, int n_tensors, int kind, int fold, int init_mode,
                          float inertia, double c, void* stream);
/* the rest of FedOptServer.update after the delta average (_fedopt.py:212-265):
 *   avg:     theta = fmaf(lr, delta, theta)
 *   adagrad: v = v + delta^2;                               theta += lr * delta / (sqrt(v) + tau)
 *   yogi:    v = v - (1-beta2) * delta^2 * sign(v - delta^2); theta += ...
 *   adam:    v = v * beta2 + (1-beta2) * delta^2;            theta += ... */
int flc_fedopt_step(float* theta, const float* delta, float* v, int64_t n, int opt, double lr, double beta2,
                    double tau, void* stream);

/* the rest of FedDRServer.update once x_tilde holds its sample-weighted fold (flc_weighted_sum, init_mode 2,
 * _feddr.py:172-180), one pass:
 *   y = fmaf(alpha, theta - y, y)                       (_feddr.py:166-170)
 *   theta = prox(cx * x_til + cy * y)                   (_feddr.py:182-190; cx = coeff/eta, cy = 1/(N+1) in fp32)
 *   prox: NONE (NullRegularizer); L1: sign(t) * max(|t| - prox_c, 0) (L1Norm); SCALE: t * prox_c (L2NormSquared,
 *   prox_c = 1/(1+2 coeff); L2Norm: NONE, then the host scales by max(0, 1 - 1/||theta||) with flc_weighted_sum). */
int flc_feddr_combine(float* theta, float* y, const float* x_til, int64_t n, float alpha, float cx, float cy,
                      int prox, float prox_c, void* stream);
/* the same three on float64 models and messages (the reference's torch ops keep them float64: add_ with alpha is one
 * fp64 fma per element, the scalars stay Python doubles, sqrt is IEEE): weights, beta, lr, beta2, tau, alpha, cx, cy
 * and prox_c are used as given */
int flc_weighted_sum_f64(const double* const* srcs, const double* weights, int n_src, int64_t n, int init_mode,
                         double beta, double* dst, void* stream);
int flc_fedopt_step_f64(double* theta, const double* delta, double* v, int64_t n, int opt, double lr, double beta2,
                        double tau, void* stream);
int flc_feddr_combine_f64(double* theta, double* y, const double* x_til, int64_t n, double alpha, double cx, double cy,
                          int prox, double prox_c, void* stream);

/* ------------------------------------------------------------------ measurement
 * Record HIP events around every launch of the kernel named `kernel_name` (NULL disables);
 * flc_probe_read synchronises those events and returns the summed duration and launch count, then
 * clears the record. Used by bench.py for the live roofline figure. */
int flc_probe_set(const char* kernel_name);
int flc_probe_read(double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* FLCODEC_H_ */
