/* abz_summary.h -- what the posterior calls share (abz_summary.hip, abz_wquantile.hip, abz_hist.hip, abz_sample.hip, abz_columns.hip,
 * abz_adjust.hip and their entry points in abz_api.hip): the view of a population, the current row and the integer mass of a position, the tally
 * of the masses and its verdict, the calls' buffer in the context, and the drivers of the passes that do not depend on where the
 * values come from (the population's parameter rows, or any dense per-particle matrix: abz_columns.hip). */
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

/* a dense per-particle matrix X[N][ldx] (its first m columns are the values) under the population's weights: what
 * abz_columns.hip summarises -- the simulated data behind the particles (posterior predictive), taken as they are (no push_p) */
struct ColView {
  const double* X;
  const double* wns;        /* NULL: unit weights */
  int64_t N;
  int ldx, m;
};

#define ABZ_COLS_MAX_M 256  /* columns of a ColView at most (the second-moment pass keeps 4 x m x 4 sums in LDS) */
#define ABZ_ADJUST_MAX_C 256  /* blob columns of a regression adjustment at most (abz_adjust.hip stages 256 x 8 coefficients in LDS) */
#define WQ_CB 16            /* weighted quantiles: columns per chunk, 128 bytes of a row */
#define H_RC 8              /* histograms, range: columns per launch (64 bytes of a row; 16 spill scalar registers) */

/* histograms: a requested column, its range and the two scales (abz_hist.hip) */
struct HistCol { double lo, hi, scale, scale2; int32_t col, pad; };

/* ---- device side */
/* the current row of position i: the slot its bit names */
__device__ inline const double* sum_row(const SumPop& p, int64_t i) {
  const uint32_t b = p.bits ? packed_bit(p.bits, i) : 0u;
  return (b ? p.slot1 : p.slot0) + (size_t)i * (size_t)p.ld;
}
/* the integer mass of position i, b = abz_stratum_bits(N): the resampler's fixed point, or 2^b each without weights */
__device__ inline unsigned long long sum_mass(const SumPop& p, int64_t i, int b) {
  return p.wns ? abz_weight_fix(p.wns[i], (uint32_t)p.N) : (1ull << b);
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

/* ---- the launches that read the values.  Every other pass of the three calls (tree finish, radix passes, LDS histograms) works
 * on what these leave in the buffer, so a call over another source of values brings its own gathers and shares the driver. */
struct SumMomentsGather {   /* sum_first_kernel / sum_second_kernel and their twins: one block per tile of ABZ_TILE positions */
  virtual void first(hipStream_t s, unsigned nt, double* parts, unsigned long long* n_pos) const = 0;
  virtual void second(hipStream_t s, unsigned nt, const double* mean, double* parts) const = 0;
};
struct SumWqGather {        /* wq_gather_kernel and its twin: the columns c0 .. c0 + ncols - 1 of the call's range */
  virtual void gather(hipStream_t s, unsigned nb, int c0, int ncols, unsigned long long* keys, unsigned long long* mass,
                      int first_chunk, unsigned long long* parts, unsigned long long* tot) const = 0;
};
struct SumHistGather {      /* hist_range_kernel / hist_bin_kernel and their twins */
  virtual void range(hipStream_t s, unsigned nb, const HistCol* cols, int c0, int ncols, unsigned long long* krange) const = 0;
  virtual void bin(hipStream_t s, unsigned nb, const HistCol* cols, int nc, int bins, int bins2, int64_t Nld,
                   unsigned long long* mass, uint16_t* idx1, uint8_t* idx2, unsigned long long* tot) const = 0;
};
/* the drivers: `call` names the entry point in the refusals, d = the number of columns the source has */
int abz_moments_drive(abcdez_ctx*, const char* call, int64_t N, int d, const SumMomentsGather&, int want_second, double* mean,
                      double* S, double* W, double* Q, int64_t* n_pos);
int abz_wquantiles_drive(abcdez_ctx*, const char* call, int64_t N, int nk, const SumWqGather&, const double* probs, int n_probs,
                         double* q_out, uint64_t* M, int64_t* n_mass);
int abz_histograms_drive(abcdez_ctx*, const char* call, int64_t N, int d, const SumHistGather&, const int32_t* cols, int n_cols,
                         int bins, const double* range, const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1,
                         uint64_t* tallies1, uint64_t* mass2, uint64_t* outside2, uint64_t* M, int64_t* n_mass);

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
/* abz_columns.hip */
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
