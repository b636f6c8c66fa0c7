/* abz_summary.h -- what the posterior calls share (abz_summary.hip, abz_wquantile.hip, abz_hist.hip, abz_sample.hip, abz_adjust.hip, abz_adjust_hcorr.hip
 * and their entry points in abz_api.hip): the view of a population, the two sources the gathers read their values from, the current
 * row and the integer mass of a position, a thread's share of a tile and the in-tile pairing of the sums, the tally of the masses
 * and its verdict, and the calls' buffer in the context. */
#pragma once
#include "abz_ctx.h"
#include "abz_device.h"

struct SumPop {
  const uint32_t* bits;     /* NULL: classic storage, slot0 is the row array */
  const double* slot0;
  const double* slot1;
  const double* wns;        /* NULL: unit weights */
  int64_t N;
  int ld, d;
};

static inline SumPop sum_pop(abcdez_ctx* ctx, const uint32_t* bits, int64_t N, const double* slot0, const double* slot1, const double* wns) {
  SumPop p{};
  p.bits = bits; p.slot0 = slot0; p.slot1 = bits ? slot1 : slot0; p.wns = wns; p.N = N;
  p.ld = ctx->h_model.ld; p.d = ctx->h_model.d;
  return p;
}
/* the current row of position i: the slot its bit names */
__device__ inline const double* sum_row(const SumPop& p, int64_t i) {
  const uint32_t b = p.bits ? packed_bit(p.bits, i) : 0u;
  return (b ? p.slot1 : p.slot0) + (size_t)i * (size_t)p.ld;
}

#define ABZ_COLS_MAX_M 256  /* columns of a ColView at most (the second-moment pass keeps 4 x m x 4 sums in LDS) */
#define ABZ_ADJUST_MAX_C 256  /* blob columns of a regression adjustment at most (abz_adjust.hip stages 256 x 8 coefficients in LDS) */
#define WQ_CB 16            /* weighted quantiles: columns per chunk, 128 bytes of a row */
#define H_RC 8              /* histograms, range: columns per launch (64 bytes of a row; 16 spill scalar registers) */

/* ---- the value sources.  The posterior calls were welded to their values in exactly five kernels, the ones that READ them
 * (sum_first, sum_second, wq_gather, hist_range, hist_bin); everything behind those (tree finish, radix passes, LDS histograms,
 * read-backs, refusals) works on sums, keys, masses and bin codes in the calls' buffer.  The five and their drivers are templates
 * over a source S, passed to the kernels by value, which says where the values are and nothing else:
 *   S.N, S.wns               the positions and their weights (NULL: unit weights); sum_weight and sum_mass below read them
 *   S.row(i)                 the start of row i
 *   S.value(row, k)          the value of column k of a row
 *   S.cols()                 the number of columns, MAX_COLS at most
 *   S::CB, KC, WAVES, HOLD_ROWS   the tuning of the two moment passes (abz_summary.hip): columns per thread and trip of the
 *                            first pass, columns k streamed per trip of the second, the waves per SIMD asked of the compiler
 *                            (0: no hint), whether a thread keeps the addresses of its 8 rows in registers or recomputes them
 * One kernel text per gather is what makes a summary of a matrix bit for bit the summary of the same numbers in a population. */

/* the population's parameter rows, push_p-cast: the row of position i is in the slot its bit names.  push_p stands between every
 * load and its use, which keeps few loads of a trip in flight: the moment passes take 8 resp. 4 + 4 columns per trip and hold the
 * addresses of a thread's 8 rows (each costs a read of the packed bits) in 16 registers, with no occupancy asked for. */
struct PopSource : SumPop {
  const abz_model* M;
  static constexpr int MAX_COLS = ABZ_MAX_D, CB = 8, KC = 4, WAVES = 0;
  static constexpr bool HOLD_ROWS = true;
  __host__ __device__ int cols() const { return d; }
  __device__ const double* row(int64_t i) const { return sum_row(*this, i); }
  __device__ double value(const double* r, int k) const { return abz_push_p(&M->prior[k], r[k]); }
};
static inline PopSource pop_source(abcdez_ctx* ctx, const SumPop& p) { return PopSource{p, (const abz_model*)ctx->d_model}; }

/* a dense per-particle matrix X[N][ldx] (its first m columns are the values, taken as they are) under the population's weights:
 * the summaries of ANY such matrix (include/abcdez_spec.h, "posterior summaries", column summaries).  The use it was made for is
 * the posterior predictive check: X = the simulated data behind the particles (the reference's blobs, docs/src/index.md:298-324,
 * rebuilt on the device by abcdez_blob_eval), summarised per observation without moving N x n_blob doubles to the host, bit for
 * bit abcdez_amd/summary.py's summary_reference of the downloaded matrix.  As with the population a thread reads runs of CONTIGUOUS
 * doubles of its row (16 in the quantile gather, 4 and 2 + 4 per trip in the moment passes, whose trips walk along the row so
 * that every line fetched is used while it is still in the caches); no thread group walks down a column of the row-major matrix.
 * Without push_p between load and use the compiler keeps every load of a trip in flight, and three waves per SIMD need the
 * registers: the moment passes take fewer columns per trip than the population's and recompute the row address from the position. */
struct ColView {
  const double* X;
  const double* wns;        /* NULL: unit weights */
  int64_t N;
  int ldx, m;
  static constexpr int MAX_COLS = ABZ_COLS_MAX_M, CB = 4, KC = 2, WAVES = 3;
  static constexpr bool HOLD_ROWS = false;
  __host__ __device__ int cols() const { return m; }
  __device__ const double* row(int64_t i) const { return X + (size_t)i * (size_t)ldx; }
  __device__ double value(const double* r, int k) const { return r[k]; }
};

/* histograms: a requested column, its range and the two scales (abz_hist.hip) */
struct HistCol { double lo, hi, scale, scale2; int32_t col, pad; };

/* ---- device side.  `s` below is anything that has the fields N and wns: a SumPop or a source */
template <class S>
__device__ inline double sum_weight(const S& s, int64_t i) { return s.wns ? s.wns[i] : 1.0; }
/* the integer mass of position i, b = abz_stratum_bits(N): the resampler's fixed point, or 2^b each without weights */
template <class S>
__device__ inline unsigned long long sum_mass(const S& s, int64_t i, int b) {
  return s.wns ? abz_weight_fix(s.wns[i], (uint32_t)s.N) : (1ull << b);
}
/* one block = one tile of ABZ_TILE positions, thread t owns the positions m*512 + 2t + c of its tile (m < 4, c < 2): position
 * q < 8 of thread t in the tile at `base` */
__device__ inline int64_t tile_pos(int64_t base, int q) { return base + (q >> 1) * 512 + 2 * threadIdx.x + (q & 1); }
/* the weights of the thread's 8 positions, 0.0 where the position does not count or lies past N: w[q] > 0.0 is the test, the
 * rows of the others are never read.  Returns the number that count. */
template <class S>
__device__ inline int tile_weights(const S& s, int64_t base, double (&w)[8]) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t i = tile_pos(base, q);
    double wv = 0.0;
    if (i < s.N) wv = sum_weight(s, i);
    const bool live = wv > 0.0;
    w[q] = live ? wv : 0.0;
    c += live;
  }
  return c;
}
/* the rows of the thread's 8 positions, w = their tile_weights: the addresses kept in registers (NULL where the position does not
 * count: never looked up), or recomputed from the position at every use -- the source's HOLD_ROWS.  live(q): position q counts,
 * asked of what is in registers anyway (the address or the weight; the other test costs the population's first pass 16
 * registers); rows[q] only where it does. */
template <class S, bool HOLD = S::HOLD_ROWS>
struct TileRows {
  const double* r[8];
  __device__ TileRows(const S& s, int64_t base, const double (&w)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = w[q] > 0.0 ? s.row(tile_pos(base, q)) : nullptr;
  }
  __device__ bool live(int q) const { return r[q] != nullptr; }
  __device__ const double* operator[](int q) const { return r[q]; }
};
template <class S>
struct TileRows<S, false> {
  const S& s;
  int64_t base;
  const double (&w)[8];
  __device__ TileRows(const S& s_, int64_t base_, const double (&w_)[8]) : s(s_), base(base_), w(w_) {}
  __device__ bool live(int q) const { return w[q] > 0.0; }
  __device__ const double* operator[](int q) const { return s.row(tile_pos(base, q)); }
};
/* slot t's eight terms and the wave's 64 slots: the in-tile pairing of tile_sum_kernel; every lane gets the wave's sum.  Every
 * bit-for-bit claim of the moment passes and of the regression adjustment rests on this one order. */
__device__ inline double tile_wave_tree(const double (&e)[8]) {
  double s = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s = s + shfl_xor_f64(s, off);
  return s;
}
/* every lane gets the sum over its wavefront */
__device__ inline unsigned long long sum_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
/* block tally of the masses: every thread brings the low halves, the high halves and the number of its masses >= 1; wave sums ->
 * LDS -> one global atomic per block and word, tot[0] += low halves, tot[1] += high halves, tot[2] += n_mass, when the block
 * counted anything.  Both sums of fewer than 2^31 halves below 2^32 are exact.  Must be reached by every thread of the block. */
__device__ inline void sum_mass_tally(unsigned long long lo, unsigned long long hi, unsigned long long cnt,
                                      unsigned long long* __restrict__ tot) {
  __shared__ unsigned long long s_tot[3];
  const int t = threadIdx.x;
  if (t < 3) s_tot[t] = 0ull;
  __syncthreads();
  lo = sum_wave_sum_u64(lo); hi = sum_wave_sum_u64(hi); cnt = sum_wave_sum_u64(cnt);
  if ((t & 63) == 0 && cnt) { atomicAdd(&s_tot[0], lo); atomicAdd(&s_tot[1], hi); atomicAdd(&s_tot[2], cnt); }
  __syncthreads();
  if (t < 3 && s_tot[2]) atomicAdd(&tot[t], s_tot[t]);
}
/* M = hi 2^32 + lo from the tally; false: M reaches 2^63, which is the case iff hi + (lo >> 32) reaches 2^31 */
__host__ __device__ inline bool sum_mass_total(unsigned long long lo, unsigned long long hi, unsigned long long* M) {
  const unsigned long long top = hi + (lo >> 32);
  if (top >= (1ull << 31)) return false;
  *M = (top << 32) | (lo & 0xFFFFFFFFull);
  return true;
}

/* ---- host side (abz_summary.hip) */
/* ctx->sum_ws holds at least `bytes` afterwards; the contents do not survive a growth */
int sum_ws_reserve(abcdez_ctx* ctx, size_t bytes);
/* the two refusals of the totals under the name of `call` (no mass, or M reaches 2^63): sets the error and returns -1 */
int sum_mass_refuse(const char* call, bool too_heavy);
/* the verdict on a tally: fills *M_out and *n_mass, or refuses */
int sum_mass_verdict(const char* call, unsigned long long lo, unsigned long long hi, unsigned long long cnt, uint64_t* M_out,
                     int64_t* n_mass);

/* the upper levels of the tile tree for `ntrees` trees of n partials each, parts[b n .. (b + 1) n) -> out[b] (sum_finish_kernel,
 * enqueued on the context's stream; no division) */
int abz_sum_finish(abcdez_ctx*, const double* parts, int64_t n, double* out, unsigned ntrees);

int abz_posterior_moments_impl(abcdez_ctx*, const SumPop&, int want_second, double* mean, double* S, double* W, double* Q, int64_t* n_pos);
int abz_posterior_quantiles_impl(abcdez_ctx*, const SumPop&, int k, const double* probs, int n_probs, double* q_out);
int abz_posterior_wquantiles_impl(abcdez_ctx*, const SumPop&, int k0, int nk, const double* probs, int n_probs, double* q_out, uint64_t* M,
                                  int64_t* n_mass);
int abz_posterior_histograms_impl(abcdez_ctx*, const SumPop&, const int32_t* cols, int n_cols, int bins, const double* range,
                                  const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1, uint64_t* tallies1,
                                  uint64_t* mass2, uint64_t* outside2, uint64_t* M, int64_t* n_mass);
int abz_posterior_sample_impl(abcdez_ctx*, const SumPop&, int64_t n, uint32_t draw, const double* delta, const uint64_t* stamp,
                              uint32_t* idx_out, double* P_out, double* theta_out, double* delta_out, uint64_t* stamp_out, uint64_t* M,
                              int64_t* n_mass);
/* the same three calls over a dense matrix, each next to its driver (abz_summary.hip, abz_wquantile.hip, abz_hist.hip) */
int abz_columns_moments_impl(abcdez_ctx*, const ColView&, int want_second, double* mean, double* S, double* W, double* Q, int64_t* n_pos);
int abz_columns_wquantiles_impl(abcdez_ctx*, const ColView&, int k0, int nk, const double* probs, int n_probs, double* q_out, uint64_t* M,
                                int64_t* n_mass);
int abz_columns_histograms_impl(abcdez_ctx*, const ColView&, const int32_t* cols, int n_cols, int bins, const double* range,
                                const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1, uint64_t* tallies1,
                                uint64_t* mass2, uint64_t* outside2, uint64_t* M, int64_t* n_mass);
/* abz_adjust.hip: s_mean[c], x_mean[d], target[c], beta[c d], S_sx_out[c d] are HOST arrays, Sb and Y DEVICE matrices */
int abz_adjust_cross_impl(abcdez_ctx*, const SumPop&, const double* Sb, int lds, const int32_t* cols, int c, const double* s_mean,
                          const double* x_mean, double* S_sx_out);
int abz_adjust_apply_impl(abcdez_ctx*, const SumPop&, const double* Sb, int lds, const int32_t* cols, int c, const double* target,
                          const double* beta, double* Y, int ldy);
/* abz_adjust_hcorr.hip: tf_kind[d], tf_lo_hi[d][2], gamma[c d], m[d] are HOST arrays too, U, Z and Y DEVICE matrices; U == NULL: u is the
 * population's push_p-cast parameters; gamma == NULL: no correction; tf_kind == NULL: no transform */
int abz_adjust_transform_impl(abcdez_ctx*, const SumPop&, const int32_t* tf_kind, const double* tf_lo_hi, double* U, int ldu);
int abz_adjust_cross_dense_impl(abcdez_ctx*, const ColView&, const double* Sb, int lds, const int32_t* cols, int c, const double* s_mean,
                                const double* x_mean, double* S_out);
int abz_adjust_logres_impl(abcdez_ctx*, const SumPop&, const double* U, int ldu, const double* Sb, int lds, const int32_t* cols, int c,
                           const double* s_mean, const double* x_mean, const double* beta, double* Z, int ldz);
int abz_adjust_apply_scaled_impl(abcdez_ctx*, const SumPop&, const double* U, int ldu, const double* Sb, int lds, const int32_t* cols, int c,
                                 const double* target, const double* beta, const double* s_mean, const double* x_mean, const double* gamma,
                                 const double* m, const int32_t* tf_kind, const double* tf_lo_hi, double* Y, int ldy);
