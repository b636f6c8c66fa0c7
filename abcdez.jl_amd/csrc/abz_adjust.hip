/*
 * abz_adjust.hip -- the regression-adjusted posterior (include/abcdez_spec.h, "posterior summaries", REGRESSION ADJUSTMENT): the
 * local-linear ABC adjustment of Beaumont, Zhang and Balding (2002), theta*_i = theta_i - beta^T (s_i - s_obs), where the population
 * and the simulated data behind it live.  Two passes relate the two halves of a result that the other posterior calls summarise
 * alone -- the parameter rows x (push_p-cast, from the packed population or abcdemc's row array: sum_row) and the blob rows s
 * (Sb + i lds, rebuilt on the device by abcdez_blob_eval, taken as they are):
 *   cross   S_sx[j][k] = T(w_i ((s_ij - smean_j) (x_ik - xmean_k))), the rectangular kin of sum_second_kernel:
 *           one block = one tile, thread t owns the positions m*512 + 2t + c; 4 centred blob columns of the thread's 8 rows stay in
 *           registers while the centred parameter columns stream past one at a time (two would spill at three waves per SIMD);
 *           the 4 x d sums of the j-block are collected in LDS, c d partials per tile, the tree levels above the tile by the
 *           summaries' finishing launch
 *   apply   y_ik = x_ik - sum_j beta_jk (s_ij - t_j), j ascending: one thread per position (the shape of every row reader here: a
 *           thread walks contiguous doubles of ITS rows, so every line it pulls is used while it is in the caches, and no lane
 *           group walks down a column of a row-major matrix); 8 accumulators per thread, beta staged through LDS in chunks of 8
 *           columns k so that a wavefront reads beta_jk as one broadcast; the order over j is fixed, so the mapping is invisible
 * The cross kernel's text lives in abz_adjust.h, a template over the value sources of abz_summary.h: here it runs over the population,
 * in abz_adjust_hcorr.hip (transforms, heteroscedastic correction) over a dense matrix.
 * The host solves for beta between the two (c x c, a few thousand operations).  Both calls only read the population and the blobs;
 * their scratch is the summaries' buffer, so a select enqueued ahead and every other state of the context survive them.  Rows of
 * positions that do not count (w <= 0) are never read; their rows of Y are +0.0.
 */
#include <string.h>

#include <string>

#include "abz_adjust.h"

/* ---- apply: Y[i][k] = x_ik - sum_j beta[j][k] (s_ij - t_j) for the counting positions, +0.0 for the others; k < d */
__global__ __launch_bounds__(ABZ_BLOCK) void adj_apply_kernel(const abz_model* __restrict__ M, const SumPop p, const AdjBlobs b,
                                                              const double* __restrict__ target, const double* __restrict__ beta,
                                                              double* __restrict__ Y, int ldy) {
  __shared__ double s_beta[ABZ_ADJUST_MAX_C * ADJ_KA];           /* [j][a]: beta[j][k0 + a] of the chunk */
  __shared__ double s_t[ABZ_ADJUST_MAX_C];
  __shared__ int s_col[ABZ_ADJUST_MAX_C];
  const int t = threadIdx.x;
  const int d = p.d, c = b.c;
  const int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t;
  for (int j = t; j < c; j += ABZ_BLOCK) { s_t[j] = target[j]; s_col[j] = b.cols[j]; }
  const bool inside = i < p.N;
  bool live = false;
  if (inside) live = sum_weight(p, i) > 0.0;
  const double* srow = nullptr;
  const double* xrow = nullptr;
  if (live) { srow = adj_srow(b, i); xrow = sum_row(p, i); }
  double* yrow = inside ? Y + (size_t)i * (size_t)ldy : nullptr;
  for (int k0 = 0; k0 < d; k0 += ADJ_KA) {                       /* block-uniform */
    __syncthreads();                                             /* the chunk before has been read (first trip: s_t, s_col are in) */
    for (int idx = t; idx < c * ADJ_KA; idx += ABZ_BLOCK) {
      const int j = idx / ADJ_KA, a = idx - j * ADJ_KA;
      s_beta[idx] = k0 + a < d ? beta[(size_t)j * d + k0 + a] : 0.0;
    }
    __syncthreads();
    if (live) {
      double acc[ADJ_KA];
#pragma unroll
      for (int a = 0; a < ADJ_KA; ++a) acc[a] = 0.0;
#pragma unroll 4
      for (int j = 0; j < c; ++j) {
        const double ds = srow[s_col[j]] - s_t[j];
#pragma unroll
        for (int a = 0; a < ADJ_KA; ++a) acc[a] = acc[a] + s_beta[j * ADJ_KA + a] * ds;
      }
#pragma unroll
      for (int a = 0; a < ADJ_KA; ++a)
        if (k0 + a < d) yrow[k0 + a] = abz_push_p(&M->prior[k0 + a], xrow[k0 + a]) - acc[a];
    } else if (inside) {
#pragma unroll
      for (int a = 0; a < ADJ_KA; ++a)
        if (k0 + a < d) yrow[k0 + a] = 0.0;
    }
  }
}

/* ================================================================ host side */
int abz_adjust_cross_impl(abcdez_ctx* ctx, const SumPop& p, const double* Sb, int lds, const int32_t* cols, int c, const double* s_mean,
                          const double* x_mean, double* S_sx_out) {
  return adj_cross_run(ctx, pop_source(ctx, p), Sb, lds, cols, c, s_mean, x_mean, S_sx_out);
}

int abz_adjust_apply_impl(abcdez_ctx* ctx, const SumPop& p, const double* Sb, int lds, const int32_t* cols, int c, const double* target,
                          const double* beta, double* Y, int ldy) {
  const int d = p.d;
  if (!adj_all_finite(target, (size_t)c)) { abz_set_error("adjust: the target is not finite"); return -1; }
  if (!adj_all_finite(beta, (size_t)c * (size_t)d)) { abz_set_error("adjust: a regression coefficient is not finite"); return -1; }
  AdjStage st;
  const int i_cols = st.add_cols(cols, c), i_t = st.add(target, (size_t)c * 8), i_beta = st.add(beta, (size_t)c * (size_t)d * 8);
  int rc = st.commit(ctx, 0);
  if (rc) return rc;
  const AdjBlobs b{Sb, st.at<int32_t>(i_cols), lds, c};
  hipLaunchKernelGGL(adj_apply_kernel, dim3((unsigned)((p.N + ABZ_BLOCK - 1) / ABZ_BLOCK)), dim3(ABZ_BLOCK), 0, ctx->stream,
                     (const abz_model*)ctx->d_model, p, b, st.at<double>(i_t), st.at<double>(i_beta), Y, ldy);
  ABZ_HIP_CHECK(hipGetLastError());
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}
