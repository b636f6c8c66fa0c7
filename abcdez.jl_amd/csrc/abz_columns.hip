/*
 * abz_columns.hip -- the posterior summaries of ANY dense per-particle matrix under the population's weights (include/abcdez_spec.h,
 * "posterior summaries", column summaries / posterior predictive): X[N][ldx], the first m columns are the values, wns[N] the
 * weights (NULL: unit weights).  The use it was made for is the posterior predictive check: X = the simulated data behind the
 * particles (the reference's blobs, docs/src/index.md:298-324, rebuilt on the device by abcdez_blob_eval), summarised per
 * observation without moving N x n_blob doubles to the host.
 *
 * The arithmetic is that of abz_summary.hip, abz_wquantile.hip and abz_hist.hip, value for value -- the same tile tree over the
 * positions, abz_summary_term1 / term2, the resampler's integer masses, abz_hist_bin -- so the results are bit for bit
 * abcdez_amd/summary.py's summary_reference of the downloaded matrix.  Only the launches that READ the values live here, twins of
 * the population's gathers with two differences: the row of position i is X + i ldx (no slot bit), and the value is taken as it
 * is (no push_p).  Everything behind them (tree finish, radix passes, LDS histograms, the read-backs and the refusals) is the
 * drivers' of abz_summary.h; the scratch is the summaries' buffer, so a select enqueued ahead and every other state of the context
 * survive the calls.
 *   first moments    one block = one tile, thread t owns the positions m*512 + 2t + c; columns in blocks of 4 per thread
 *   second moments   4 centred columns j of the thread's 8 rows in registers, the columns k >= j stream past 2 at a time
 *   wq gather        order keys of up to 16 columns of a row per thread, masses, totals, per-block (v_1, m_(1), v_n)
 *   hist range/bin   smallest and largest key of 8 columns a launch; one read of the row for every requested column's bins
 * As in the population's gathers a thread reads runs of CONTIGUOUS doubles of its row (16 in the quantile gather, 4 and 2 + 4 per
 * trip in the moment passes, whose trips walk along the row so that every line fetched is used while it is still in the caches);
 * no thread group walks down a column of the row-major matrix.  The moment passes keep no row pointers (the address is recomputed
 * from the position) and fewer columns per trip than their twins: without push_p between load and use the compiler keeps every
 * load of a trip in flight, and three waves per SIMD need the registers.  Rows of positions that do not count (w <= 0, or no
 * mass) are never read.
 */
#include <string.h>

#include "abz_ctx.h"
#include "abz_device.h"
#include "abz_summary.h"

#define COL_CB 4            /* first pass: columns per thread and trip */
#define COL_JB 4            /* second pass: columns j held per thread */
#define COL_KC 2            /* second pass: columns k streamed per trip */

typedef unsigned long long u64;

__device__ inline const double* col_row(const ColView& v, int64_t i) { return v.X + (size_t)i * (size_t)v.ldx; }
/* the integer mass of position i, b = abz_stratum_bits(N): the resampler's fixed point, or 2^b each without weights */
__device__ inline u64 col_mass(const ColView& v, int64_t i, int b) {
  return v.wns ? abz_weight_fix(v.wns[i], (uint32_t)v.N) : (1ull << b);
}
/* position q < 8 of thread t in the tile at `base` */
__device__ inline int64_t col_pos(int64_t base, int q) { return base + (q >> 1) * 512 + 2 * threadIdx.x + (q & 1); }
/* the weights of the 8 positions of thread t in its tile, 0.0 where the position does not count or lies past N: the rows of
 * those are never read (w[q] > 0.0 is the test; the row address is recomputed from the position, not kept in registers) */
__device__ inline int col_owned(const ColView& v, int64_t base, double (&w)[8]) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t i = col_pos(base, q);
    double wv = 0.0;
    if (i < v.N) wv = v.wns ? v.wns[i] : 1.0;
    const bool live = wv > 0.0;
    w[q] = live ? wv : 0.0;
    c += live;
  }
  return c;
}
/* slot t's eight terms and the wave's 64 slots: the in-tile pairing of tile_sum_kernel; every lane gets the wave's sum */
__device__ inline double col_wave_tree(const double (&e)[8]) {
  double s = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s = s + shfl_xor_f64(s, off);
  return s;
}

/* ---- first moments: parts[(k) nt + tile] = tile sum of w x_k (k < m), parts[(m) nt + tile] of w, parts[(m+1) nt + tile] of w w */
__global__ __launch_bounds__(ABZ_BLOCK, 3) void col_first_kernel(const ColView v, double* __restrict__ parts, u64* __restrict__ n_pos) {
  __shared__ double s_w[COL_CB][4];
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t nt = gridDim.x, tile = blockIdx.x;
  double w[8];
  const u64 c = sum_wave_sum_u64((u64)col_owned(v, tile * ABZ_TILE, w));
  if ((t & 63) == 0 && c) atomicAdd(n_pos, c);
  {
    double e[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = w[q];
    const double sw = col_wave_tree(e);
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = w[q] * w[q];
    const double sq = col_wave_tree(e);
    if ((t & 63) == 0) { s_w[0][wave] = sw; s_w[1][wave] = sq; }
    __syncthreads();
    if (t < 2) parts[(size_t)(v.m + t) * nt + tile] = (s_w[t][0] + s_w[t][1]) + (s_w[t][2] + s_w[t][3]);
    __syncthreads();
  }
  for (int cb = 0; cb < v.m; cb += COL_CB) {                     /* block-uniform */
    double e[COL_CB][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int a = 0; a < COL_CB; ++a) {
        const int k = cb + a;
        double x = 0.0;
        if (w[q] > 0.0 && k < v.m) x = abz_summary_term1(w[q], col_row(v, col_pos(tile * ABZ_TILE, q))[k]);
        e[a][q] = x;
      }
    }
#pragma unroll
    for (int a = 0; a < COL_CB; ++a) {
      const double s = col_wave_tree(e[a]);
      if ((t & 63) == 0) s_w[a][wave] = s;
    }
    __syncthreads();
    if (t < COL_CB && cb + t < v.m) parts[(size_t)(cb + t) * nt + tile] = (s_w[t][0] + s_w[t][1]) + (s_w[t][2] + s_w[t][3]);
    __syncthreads();
  }
}

/* ---- second central moments: parts[pair(j, k) nt + tile], pair(j, k) = j m - j (j - 1) / 2 + (k - j), j <= k < m */
__global__ __launch_bounds__(ABZ_BLOCK, 3) void col_second_kernel(const ColView v, const double* __restrict__ mean,
                                                               double* __restrict__ parts) {
  __shared__ double s_acc[COL_JB * ABZ_COLS_MAX_M][4];           /* (a, k) -> the four waves' sums */
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t nt = gridDim.x, tile = blockIdx.x;
  const int d = v.m;
  double w[8];
  (void)col_owned(v, tile * ABZ_TILE, w);
  for (int jb = 0; jb < d; jb += COL_JB) {                       /* block-uniform */
    double cj[COL_JB][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int a = 0; a < COL_JB; ++a) {
        const int j = jb + a;
        cj[a][q] = (w[q] > 0.0 && j < d) ? col_row(v, col_pos(tile * ABZ_TILE, q))[j] - mean[j] : 0.0;
      }
    }
    for (int kb = jb; kb < d; kb += COL_KC) {
      double ck[COL_KC][8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int b = 0; b < COL_KC; ++b) {
          const int k = kb + b;
          ck[b][q] = (w[q] > 0.0 && k < d) ? col_row(v, col_pos(tile * ABZ_TILE, q))[k] - mean[k] : 0.0;
        }
      }
#pragma unroll
      for (int a = 0; a < COL_JB; ++a) {
#pragma unroll
        for (int b = 0; b < COL_KC; ++b) {
          const int j = jb + a, k = kb + b;
          if (j <= k && k < d) {                                 /* block-uniform */
            double e[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) e[q] = w[q] > 0.0 ? w[q] * (cj[a][q] * ck[b][q]) : 0.0;   /* abz_summary_term2 on centred values */
            const double s = col_wave_tree(e);
            if ((t & 63) == 0) s_acc[a * d + k][wave] = s;
          }
        }
      }
    }
    __syncthreads();
    for (int idx = t; idx < COL_JB * d; idx += ABZ_BLOCK) {
      const int a = idx / d, k = idx - a * d, j = jb + a;
      if (j < d && k >= j) {
        const size_t pair = (size_t)j * d - (size_t)j * (j - 1) / 2 + (size_t)(k - j);
        parts[pair * nt + tile] = (s_acc[idx][0] + s_acc[idx][1]) + (s_acc[idx][2] + s_acc[idx][3]);
      }
    }
    __syncthreads();
  }
}

/* ---- weighted quantiles, gather: keys[c N + i] for the counting positions (others are never read: their mass is 0), mass[i],
 * the totals tot[0 .. 2] (first chunk only) and parts[(c nb + block) 3 + {0, 1, 2}] = (smallest key, smallest mass at it,
 * largest key) of the block's positions; the columns k_first .. k_first + ncols - 1 of X */
__global__ __launch_bounds__(ABZ_BLOCK) void col_wq_gather_kernel(const ColView v, int k_first, int ncols, u64* __restrict__ keys,
                                                                  u64* __restrict__ mass, int first_chunk, u64* __restrict__ parts,
                                                                  u64* __restrict__ tot) {
  __shared__ u64 s_kmin[WQ_CB], s_m1[WQ_CB], s_kmax[WQ_CB];
  const int t = threadIdx.x;
  u64 kmin[WQ_CB], m1[WQ_CB], kmax[WQ_CB];
#pragma unroll
  for (int c = 0; c < WQ_CB; ++c) { kmin[c] = ~0ull; m1[c] = ~0ull; kmax[c] = 0ull; }
  if (t < WQ_CB) { s_kmin[t] = ~0ull; s_m1[t] = ~0ull; s_kmax[t] = 0ull; }
  u64 lo = 0, hi = 0, cnt = 0;
  const int b = abz_stratum_bits((uint32_t)v.N);
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < v.N; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    const u64 m = col_mass(v, i, b);
    if (first_chunk) mass[i] = m;
    if (m < 1) continue;
    lo += m & 0xFFFFFFFFull; hi += m >> 32; cnt += 1;
    const double* row = col_row(v, i) + k_first;
#pragma unroll
    for (int c = 0; c < WQ_CB; ++c) {
      if (c < ncols) {
        const u64 key = f64_order_key(row[c]);
        keys[(size_t)c * (size_t)v.N + (size_t)i] = key;
        if (key < kmin[c] || (key == kmin[c] && m < m1[c])) { kmin[c] = key; m1[c] = m; }
        if (key > kmax[c]) kmax[c] = key;
      }
    }
  }
  if (first_chunk) sum_mass_tally(lo, hi, cnt, tot);                   /* kernel-uniform */
  __syncthreads();
#pragma unroll
  for (int c = 0; c < WQ_CB; ++c) {
    if (c < ncols && cnt) { atomicMin(&s_kmin[c], kmin[c]); atomicMax(&s_kmax[c], kmax[c]); }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < WQ_CB; ++c) {
    if (c < ncols && kmin[c] == s_kmin[c] && m1[c] != ~0ull) atomicMin(&s_m1[c], m1[c]);
  }
  __syncthreads();
  if (t < ncols) {
    u64* o = parts + ((size_t)t * gridDim.x + blockIdx.x) * 3;
    o[0] = s_kmin[t]; o[1] = s_m1[t]; o[2] = s_kmax[t];
  }
}

/* ---- histograms, range: krange[2 c + {0, 1}] = (smallest, largest) order key of requested column c over the counting positions,
 * for the columns c0 .. c0 + ncols - 1 of the list */
__global__ __launch_bounds__(ABZ_BLOCK) void col_hist_range_kernel(const ColView v, const HistCol* __restrict__ cols, int c0, int ncols,
                                                                   u64* __restrict__ krange) {
  __shared__ u64 s_kmin[H_RC], s_kmax[H_RC];
  __shared__ int s_col[H_RC];
  const int t = threadIdx.x;
  if (t < H_RC) { s_kmin[t] = ~0ull; s_kmax[t] = 0ull; s_col[t] = t < ncols ? cols[c0 + t].col : 0; }
  __syncthreads();
  u64 kmin[H_RC], kmax[H_RC];
#pragma unroll
  for (int c = 0; c < H_RC; ++c) { kmin[c] = ~0ull; kmax[c] = 0ull; }
  const int b = abz_stratum_bits((uint32_t)v.N);
  bool any = false;
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < v.N; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    if (col_mass(v, i, b) < 1) continue;
    any = true;
    const double* row = col_row(v, i);
#pragma unroll
    for (int c = 0; c < H_RC; ++c) {
      if (c < ncols) {
        const u64 key = f64_order_key(row[s_col[c]]);
        if (key < kmin[c]) kmin[c] = key;
        if (key > kmax[c]) kmax[c] = key;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < H_RC; ++c) {
    if (c < ncols && any) { atomicMin(&s_kmin[c], kmin[c]); atomicMax(&s_kmax[c], kmax[c]); }
  }
  __syncthreads();
  if (t < ncols && s_kmax[t] >= s_kmin[t]) {
    atomicMin(&krange[2 * (c0 + t)], s_kmin[t]);
    atomicMax(&krange[2 * (c0 + t) + 1], s_kmax[t]);
  }
}

/* ---- histograms, bin: mass[i] for i < Nld (0 beyond N), idx1[c Nld + i] and idx2[c Nld + i] (when idx2) for the counting
 * positions (255 in idx2: outside); tot[0 .. 2] the tally of the masses */
__global__ __launch_bounds__(ABZ_BLOCK) void col_hist_bin_kernel(const ColView v, const HistCol* __restrict__ cols, int nc, int bins,
                                                                 int bins2, int64_t Nld, u64* __restrict__ mass,
                                                                 uint16_t* __restrict__ idx1, uint8_t* __restrict__ idx2,
                                                                 u64* __restrict__ tot) {
  const int t = threadIdx.x;
  u64 lo = 0, hi = 0, cnt = 0;
  const int b = abz_stratum_bits((uint32_t)v.N);
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < Nld; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    const u64 m = i < v.N ? col_mass(v, i, b) : 0ull;
    mass[i] = m;
    if (m < 1) continue;
    lo += m & 0xFFFFFFFFull; hi += m >> 32; cnt += 1;
    const double* row = col_row(v, i);
    for (int c = 0; c < nc; ++c) {
      const HistCol h = cols[c];
      const double x = row[h.col];
      idx1[(size_t)c * (size_t)Nld + (size_t)i] = (uint16_t)abz_hist_bin(x, h.lo, h.hi, h.scale, bins);
      if (idx2) {
        const int32_t b2 = abz_hist_bin(x, h.lo, h.hi, h.scale2, bins2);
        idx2[(size_t)c * (size_t)Nld + (size_t)i] = (uint8_t)(b2 >= bins2 ? 255u : (uint32_t)b2);
      }
    }
  }
  sum_mass_tally(lo, hi, cnt, tot);
}

/* ================================================================ host side: the gathers handed to the drivers of abz_summary.h */
struct ColMomentsGather : SumMomentsGather {
  ColView v;
  void first(hipStream_t s, unsigned nt, double* parts, u64* n_pos) const override {
    hipLaunchKernelGGL(col_first_kernel, dim3(nt), dim3(ABZ_BLOCK), 0, s, v, parts, n_pos);
  }
  void second(hipStream_t s, unsigned nt, const double* mean, double* parts) const override {
    hipLaunchKernelGGL(col_second_kernel, dim3(nt), dim3(ABZ_BLOCK), 0, s, v, mean, parts);
  }
};
struct ColWqGather : SumWqGather {
  ColView v;
  int k0;
  void gather(hipStream_t s, unsigned nb, int c0, int ncols, u64* keys, u64* mass, int first_chunk, u64* parts, u64* tot) const override {
    hipLaunchKernelGGL(col_wq_gather_kernel, dim3(nb), dim3(ABZ_BLOCK), 0, s, v, k0 + c0, ncols, keys, mass, first_chunk, parts, tot);
  }
};
struct ColHistGather : SumHistGather {
  ColView v;
  void range(hipStream_t s, unsigned nb, const HistCol* cols, int c0, int ncols, u64* krange) const override {
    hipLaunchKernelGGL(col_hist_range_kernel, dim3(nb), dim3(ABZ_BLOCK), 0, s, v, cols, c0, ncols, krange);
  }
  void bin(hipStream_t s, unsigned nb, const HistCol* cols, int nc, int bins, int bins2, int64_t Nld, u64* mass, uint16_t* idx1,
           uint8_t* idx2, u64* tot) const override {
    hipLaunchKernelGGL(col_hist_bin_kernel, dim3(nb), dim3(ABZ_BLOCK), 0, s, v, cols, nc, bins, bins2, Nld, mass, idx1, idx2, tot);
  }
};

int abz_columns_moments_impl(abcdez_ctx* ctx, const ColView& v, int want_second, double* mean, double* S, double* W, double* Q,
                             int64_t* n_pos) {
  ColMomentsGather g;
  g.v = v;
  return abz_moments_drive(ctx, "columns_moments", v.N, v.m, g, want_second, mean, S, W, Q, n_pos);
}

int abz_columns_wquantiles_impl(abcdez_ctx* ctx, const ColView& v, int k0, int nk, const double* probs, int n_probs, double* q_out,
                                uint64_t* M, int64_t* n_mass) {
  ColWqGather g;
  g.v = v; g.k0 = k0;
  return abz_wquantiles_drive(ctx, "columns_wquantiles", v.N, nk, g, probs, n_probs, q_out, M, n_mass);
}

int abz_columns_histograms_impl(abcdez_ctx* ctx, const ColView& v, const int32_t* cols, int n_cols, int bins, const double* range,
                                const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1, uint64_t* tallies1,
                                uint64_t* mass2, uint64_t* outside2, uint64_t* M, int64_t* n_mass) {
  ColHistGather g;
  g.v = v;
  return abz_histograms_drive(ctx, "columns_histograms", v.N, v.m, g, cols, n_cols, bins, range, pairs, n_pairs, bins2, lo_hi, mass1,
                              tallies1, mass2, outside2, M, n_mass);
}
