/*
 * abz_summary.hip -- posterior summaries of the population where it lives (include/abcdez_spec.h, "posterior summaries"):
 *   weighted mean, second central moments, W = sum(Wns), Q = sum(Wns.^2), #(Wns > 0), marginal type-7 quantiles
 * -- what every test of the reference extracts from a result (test/runtests.jl:159-162) of the tuple of
 * src/abcdez_smc.jl:388-393 / src/abcdez_mc.jl:166-171, without moving the rows to the host.
 *
 * Every sum is the fixed tile tree over the POSITIONS (tile_sum_kernel's pairing inside a tile of 2048, levels 1-2 above it),
 * so the results are bit for bit those of the numpy restatement in abcdez_amd/summary.py.  One block = one tile; thread t owns
 * the positions m*512 + 2t + c of its tile (m < 4, c < 2), reads their rows straight from the packed storage (current slot
 * from the position's bit) and applies push_p per component.  The two moment passes are templates over the value source of
 * abz_summary.h, so the same text summarises any dense per-particle matrix (the column summaries, abz_columns_moments_impl);
 * the columns per trip below are the population's, a matrix takes 4 and 2.
 *   first-moment pass   columns in blocks of 8 per thread (64 doubles of terms in registers), d + 2 partials per tile
 *   second-moment pass  4 centred columns j of the thread's 8 rows stay in registers while the columns k >= j stream past 4 at
 *                       a time from the rows the block has just pulled into the caches; d (d + 1) / 2 partials per tile, no
 *                       term vector in memory, no launch per pair
 *   finish              one block per tree (levels 1-2); the first pass's finish also divides by W
 *   column gather       push_p-cast column k + the mask (Wns > 0) for the exact rank select of abz_population.hip
 * The calls keep a buffer of their own and put the select's device state back: a run continued after a summary is
 * bit-identical to one without it.
 */
#include <string.h>

#include <string>
#include <vector>

#include "abz_ctx.h"
#include "abz_device.h"
#include "abz_summary.h"

int abz_select_impl(abcdez_ctx*, const double*, const uint8_t*, int64_t, int64_t, double*, double*, int64_t*);

#define ABZ_SUM_JB 4        /* second pass: columns j held per thread; the columns per trip are the source's (S::CB, S::KC) */

/* ---- first moments: parts[(k) nt + tile] = tile sum of w x_k (k < d), parts[(d) nt + tile] of w, parts[(d+1) nt + tile] of w w */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK, S::WAVES) void sum_first_kernel(const S src, double* __restrict__ parts,
                                                                        unsigned long long* __restrict__ n_pos) {
  __shared__ double s_w[S::CB][4];
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t nt = gridDim.x, tile = blockIdx.x;
  const int d = src.cols();
  double w[8];
  const unsigned long long c = sum_wave_sum_u64((unsigned long long)tile_weights(src, tile * ABZ_TILE, w));
  const TileRows<S> row(src, tile * ABZ_TILE, w);
  if ((t & 63) == 0 && c) atomicAdd(n_pos, c);
  {
    double e[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = w[q];
    const double sw = tile_wave_tree(e);
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = w[q] * w[q];
    const double sq = tile_wave_tree(e);
    if ((t & 63) == 0) { s_w[0][wave] = sw; s_w[1][wave] = sq; }
    __syncthreads();
    if (t < 2) parts[(size_t)(d + t) * nt + tile] = (s_w[t][0] + s_w[t][1]) + (s_w[t][2] + s_w[t][3]);
    __syncthreads();
  }
  for (int cb = 0; cb < d; cb += S::CB) {                        /* block-uniform */
    double e[S::CB][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int a = 0; a < S::CB; ++a) {
        const int k = cb + a;
        double v = 0.0;
        if (row.live(q) && k < d) v = abz_summary_term1(w[q], src.value(row[q], k));
        e[a][q] = v;
      }
    }
#pragma unroll
    for (int a = 0; a < S::CB; ++a) {
      const double s = tile_wave_tree(e[a]);
      if ((t & 63) == 0) s_w[a][wave] = s;
    }
    __syncthreads();
    if (t < S::CB && cb + t < d) parts[(size_t)(cb + t) * nt + tile] = (s_w[t][0] + s_w[t][1]) + (s_w[t][2] + s_w[t][3]);
    __syncthreads();
  }
}

/* ---- second central moments: parts[pair(j, k) nt + tile], pair(j, k) = j d - j (j - 1) / 2 + (k - j), j <= k < d */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK, S::WAVES) void sum_second_kernel(const S src, const double* __restrict__ mean,
                                                                         double* __restrict__ parts) {
  __shared__ double s_acc[ABZ_SUM_JB * S::MAX_COLS][4];          /* (a, k) -> the four waves' sums */
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t nt = gridDim.x, tile = blockIdx.x;
  const int d = src.cols();
  double w[8];
  (void)tile_weights(src, tile * ABZ_TILE, w);
  const TileRows<S> row(src, tile * ABZ_TILE, w);
  for (int jb = 0; jb < d; jb += ABZ_SUM_JB) {                   /* block-uniform */
    double cj[ABZ_SUM_JB][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int a = 0; a < ABZ_SUM_JB; ++a) {
        const int j = jb + a;
        cj[a][q] = (row.live(q) && j < d) ? src.value(row[q], j) - mean[j] : 0.0;
      }
    }
    for (int kb = jb; kb < d; kb += S::KC) {
      double ck[S::KC][8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int b = 0; b < S::KC; ++b) {
          const int k = kb + b;
          ck[b][q] = (row.live(q) && k < d) ? src.value(row[q], k) - mean[k] : 0.0;
        }
      }
#pragma unroll
      for (int a = 0; a < ABZ_SUM_JB; ++a) {
#pragma unroll
        for (int b = 0; b < S::KC; ++b) {
          const int j = jb + a, k = kb + b;
          if (j <= k && k < d) {                                 /* block-uniform */
            double e[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) e[q] = row.live(q) ? w[q] * (cj[a][q] * ck[b][q]) : 0.0;   /* abz_summary_term2 on centred values */
            const double s = tile_wave_tree(e);
            if ((t & 63) == 0) s_acc[a * d + k][wave] = s;
          }
        }
      }
    }
    __syncthreads();
    for (int idx = t; idx < ABZ_SUM_JB * d; idx += ABZ_BLOCK) {
      const int a = idx / d, k = idx - a * d, j = jb + a;
      if (j < d && k >= j) {
        const size_t pair = (size_t)j * d - (size_t)j * (j - 1) / 2 + (size_t)(k - j);
        parts[pair * nt + tile] = (s_acc[idx][0] + s_acc[idx][1]) + (s_acc[idx][2] + s_acc[idx][3]);
      }
    }
    __syncthreads();
  }
}

/* ---- the upper levels of the tile tree, one block per tree (tree_finish_kernel's level-1 / level-2 logic for any number of
 * trees): tree b sums parts[b n .. (b + 1) n).  n == 1: that partial IS the sum (one tile, no further level).  The first
 * n_div trees are then divided by tree div_by (mean_k = T(w x_k) / W): those blocks finish that tree as well. */
struct SumFinishArgs {
  const double* parts;
  int64_t n;                /* partials per tree, <= 2048 * 2048 */
  double* out;
  int n_div, div_by;
};
__device__ inline double sum_finish_tile(const double* __restrict__ x, int64_t n, int64_t base, double* s_w) {
  const int t = threadIdx.x;
  double e[8];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int64_t k = base + m * 512 + 2 * t;
    e[2 * m] = k < n ? x[k] : 0.0;
    e[2 * m + 1] = k + 1 < n ? x[k + 1] : 0.0;
  }
  const double s = tile_wave_tree(e);
  __syncthreads();                                     /* s_w is reused from tile to tile */
  if ((t & 63) == 0) s_w[t >> 6] = s;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);        /* every thread gets the tile's sum */
}
__device__ inline double sum_finish_tree(const double* __restrict__ x, int64_t n, double* s_w, double* s_l1) {
  if (n == 1) return x[0];
  const int64_t nt = (n + ABZ_TILE - 1) / ABZ_TILE;
  if (nt == 1) return sum_finish_tile(x, n, 0, s_w);
  for (int64_t tile = 0; tile < nt; ++tile) {
    const double v = sum_finish_tile(x, n, tile * ABZ_TILE, s_w);
    if (threadIdx.x == 0) s_l1[tile] = v;
  }
  __syncthreads();
  const double r = sum_finish_tile(s_l1, nt, 0, s_w);
  __syncthreads();                                     /* s_l1 may be filled again by the caller's next tree */
  return r;
}
__global__ __launch_bounds__(ABZ_BLOCK) void sum_finish_kernel(const SumFinishArgs a) {
  __shared__ double s_w[4];
  __shared__ double s_l1[ABZ_TILE];
  const int b = blockIdx.x;
  double r = sum_finish_tree(a.parts + (size_t)b * a.n, a.n, s_w, s_l1);
  if (b < a.n_div) r = r / sum_finish_tree(a.parts + (size_t)a.div_by * a.n, a.n, s_w, s_l1);
  if (threadIdx.x == 0) a.out[b] = r;
}

/* ---- column k of P and the mask (Wns > 0), dense, for the rank select */
__global__ __launch_bounds__(ABZ_BLOCK) void sum_column_kernel(const abz_model* __restrict__ M, const SumPop p, int k,
                                                               double* __restrict__ col, uint8_t* __restrict__ mask,
                                                               unsigned long long* __restrict__ n_pos) {
  const int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + threadIdx.x;
  bool live = false;
  if (i < p.N) {
    live = sum_weight(p, i) > 0.0;
    double v = 0.0;
    if (live) v = abz_push_p(&M->prior[k], sum_row(p, i)[k]);
    col[i] = v;
    mask[i] = (uint8_t)live;
  }
  const unsigned long long c = sum_wave_sum_u64(live);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_pos, c);
}

/* ================================================================ host side */
int sum_ws_reserve(abcdez_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->sum_ws_bytes) return 0;
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (ctx->sum_ws) ABZ_HIP_CHECK(hipFree(ctx->sum_ws));
  ctx->sum_ws = nullptr; ctx->sum_ws_bytes = 0;
  const size_t want = abz_align(bytes + bytes / 8, 1 << 20);
  ABZ_HIP_CHECK(hipMalloc(&ctx->sum_ws, want));
  ctx->sum_ws_bytes = want;
  return 0;
}
int sum_mass_refuse(const char* call, bool too_heavy) {
  abz_set_error(std::string(call) + (too_heavy ? ": the total mass reaches 2^63 -- the weights are not normalised (sum(Wns) must be about 1)"
                                               : ": no particle has a positive weight that carries mass"));
  return -1;
}
int sum_mass_verdict(const char* call, unsigned long long lo, unsigned long long hi, unsigned long long cnt, uint64_t* M_out,
                     int64_t* n_mass) {
  unsigned long long M = 0;
  if (cnt < 1) return sum_mass_refuse(call, false);
  if (!sum_mass_total(lo, hi, &M)) return sum_mass_refuse(call, true);
  *M_out = M;
  *n_mass = (int64_t)cnt;
  return 0;
}

int abz_sum_finish(abcdez_ctx* ctx, const double* parts, int64_t n, double* out, unsigned ntrees) {
  SumFinishArgs f{parts, n, out, 0, 0};
  hipLaunchKernelGGL(sum_finish_kernel, dim3(ntrees), dim3(ABZ_BLOCK), 0, ctx->stream, f);
  ABZ_HIP_CHECK(hipGetLastError());
  return 0;
}

/* the moments of a source; `call` names the entry point in the refusal */
template <class Src>
static int moments_drive(abcdez_ctx* ctx, const char* call, const Src& src, int want_second, double* mean, double* S, double* W, double* Q,
                         int64_t* n_pos) {
  const int64_t N = src.N;
  const int d = src.cols();
  const size_t nt = (size_t)((N + ABZ_TILE - 1) / ABZ_TILE);
  const size_t npairs = (size_t)d * (size_t)(d + 1) / 2;
  const size_t ntrees = want_second && npairs > (size_t)d + 2 ? npairs : (size_t)d + 2;
  /* [ n_pos | first results d + 2 | second results npairs | partials ntrees x nt ] */
  const size_t o_res1 = 256, o_res2 = o_res1 + abz_align(((size_t)d + 2) * 8), o_parts = o_res2 + abz_align(npairs * 8);
  int rc = sum_ws_reserve(ctx, o_parts + ntrees * nt * 8);
  if (rc) return rc;
  char* base = (char*)ctx->sum_ws;
  unsigned long long* d_npos = (unsigned long long*)base;
  double* res1 = (double*)(base + o_res1);
  double* res2 = (double*)(base + o_res2);
  double* parts = (double*)(base + o_parts);

  ABZ_HIP_CHECK(hipMemsetAsync(d_npos, 0, 8, ctx->stream));
  hipLaunchKernelGGL(sum_first_kernel<Src>, dim3((unsigned)nt), dim3(ABZ_BLOCK), 0, ctx->stream, src, parts, d_npos);
  SumFinishArgs f{parts, (int64_t)nt, res1, d, d};
  hipLaunchKernelGGL(sum_finish_kernel, dim3((unsigned)(d + 2)), dim3(ABZ_BLOCK), 0, ctx->stream, f);
  ABZ_HIP_CHECK(hipGetLastError());
  std::vector<double> h1((size_t)d + 2);
  unsigned long long h_npos = 0;
  ABZ_HIP_CHECK(hipMemcpyAsync(h1.data(), res1, ((size_t)d + 2) * 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipMemcpyAsync(&h_npos, d_npos, 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (h_npos < 1) { abz_set_error(std::string(call) + ": no particle has a positive weight"); return -1; }
  memcpy(mean, h1.data(), (size_t)d * 8);
  *W = h1[d]; *Q = h1[d + 1]; *n_pos = (int64_t)h_npos;
  if (!want_second) return 0;

  hipLaunchKernelGGL(sum_second_kernel<Src>, dim3((unsigned)nt), dim3(ABZ_BLOCK), 0, ctx->stream, src, (const double*)res1, parts);
  SumFinishArgs g{parts, (int64_t)nt, res2, 0, 0};
  hipLaunchKernelGGL(sum_finish_kernel, dim3((unsigned)npairs), dim3(ABZ_BLOCK), 0, ctx->stream, g);
  ABZ_HIP_CHECK(hipGetLastError());
  std::vector<double> h2(npairs);
  ABZ_HIP_CHECK(hipMemcpyAsync(h2.data(), res2, npairs * 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  size_t pair = 0;
  for (int j = 0; j < d; ++j)
    for (int k = j; k < d; ++k, ++pair) S[(size_t)j * d + k] = S[(size_t)k * d + j] = h2[pair];
  return 0;
}

int abz_posterior_moments_impl(abcdez_ctx* ctx, const SumPop& p, int want_second, double* mean, double* S, double* W, double* Q,
                               int64_t* n_pos) {
  return moments_drive(ctx, "posterior_moments", pop_source(ctx, p), want_second, mean, S, W, Q, n_pos);
}
int abz_columns_moments_impl(abcdez_ctx* ctx, const ColView& v, int want_second, double* mean, double* S, double* W, double* Q,
                             int64_t* n_pos) {
  return moments_drive(ctx, "columns_moments", v, want_second, mean, S, W, Q, n_pos);
}

int abz_posterior_quantiles_impl(abcdez_ctx* ctx, const SumPop& p, int k, const double* probs, int n_probs, double* q_out) {
  const int64_t N = p.N;
  /* [ n_pos | column N x f64 | mask N x u8 ] */
  const size_t o_col = 256, o_mask = o_col + abz_align((size_t)N * 8);
  int rc = sum_ws_reserve(ctx, o_mask + abz_align((size_t)N));
  if (rc) return rc;
  char* base = (char*)ctx->sum_ws;
  unsigned long long* d_npos = (unsigned long long*)base;
  double* col = (double*)(base + o_col);
  uint8_t* mask = (uint8_t*)(base + o_mask);
  ABZ_HIP_CHECK(hipMemsetAsync(d_npos, 0, 8, ctx->stream));
  hipLaunchKernelGGL(sum_column_kernel, dim3((unsigned)((N + ABZ_BLOCK - 1) / ABZ_BLOCK)), dim3(ABZ_BLOCK), 0, ctx->stream,
                     (const abz_model*)ctx->d_model, p, k, col, mask, d_npos);
  ABZ_HIP_CHECK(hipGetLastError());
  /* the select keeps state between calls (its binning window on the device, which arrays it belongs to) and returns through the
   * scalar area, where a select enqueued ahead of the next generation may be waiting: all of it is put back below */
  unsigned long long h_npos = 0, scal[ABZ_S_SCALARS];
  ABZ_HIP_CHECK(hipMemcpyAsync(&h_npos, d_npos, 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipMemcpyAsync(scal, ctx->d_scal, sizeof(scal), hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (h_npos < 1) { abz_set_error("posterior_quantiles: no particle has a positive weight"); return -1; }
  const bool clean = ctx->sel_clean;
  const void *sd = ctx->sel_delta, *sa = ctx->sel_alive;
  const int64_t sn = ctx->sel_N;
  const int64_t n = (int64_t)h_npos;
  for (int q = 0; q < n_probs && rc == 0; ++q) {
    double g, a = 0.0, b = 0.0;
    int64_t n_le;
    /* every select seeds its binning window from the column's extrema: the window a select leaves behind ends at its own rank
     * (made for the shrinking quantiles of the generations), and a later, larger probability would find all its keys clamped
     * into the last bin and leave them to the one finishing block (measured at 2^22 positions: 4 ms per select instead of 0.4, gather and read-back included) */
    ctx->sel_clean = false;
    const int64_t j = abz_quantile_type7_index(n, probs[q], &g);
    rc = abz_select_impl(ctx, col, mask, N, j - 1, &a, &b, &n_le);
    if (n == 1) b = a;
    if (rc == 0) q_out[q] = abz_quantile_type7(a, b, g);
  }
  ctx->sel_clean = clean; ctx->sel_delta = sd; ctx->sel_alive = sa; ctx->sel_N = sn;
  if (hipMemcpyAsync(ctx->d_scal, scal, sizeof(scal), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    if (rc == 0) { abz_set_error("posterior_quantiles: could not restore the select's device state"); rc = -2; }
  }
  return rc;
}
