/*
 * abz_adjust_hcorr.hip -- bounded transforms and the heteroscedastic correction of the regression adjustment (include/abcdez_spec.h,
 * "REGRESSION ADJUSTMENT": TRANSFORM, HETEROSCEDASTIC CORRECTION; library version 680).  Per-particle passes over the two matrices
 * the plain method (abz_adjust.hip) already holds, every one in the shape of its apply: one thread per position, walking contiguous
 * doubles of ITS rows, the coefficients staged through LDS in chunks of columns k so that a wavefront reads them as one broadcast.
 *   transform  population -> U[N][d] = abz_adjust_forward of the push_p-cast parameters
 *   cross      S_su resp. S_sz over a dense matrix: the cross kernel of abz_adjust.h over the ColView source, the same text as S_sx
 *   logres     Z[i][k] = abz_log(e e), e = (u_ik - xmean_k) - sum_j beta_jk (s_ij - smean_j)
 *   scaled     Y[i][k] = back(m_k + e exp(-0.5 sum_j gamma_jk (s_ij - t_j))): two accumulator sets per thread, the beta sum centred
 *              on smean and the gamma sum centred on t, ADJ_KS = 4 columns per trip -- 8 accumulators and 2 x 256 x 4 coefficients
 *              in LDS, the plain apply's budget (two sets of 8 would double both and halve the workgroups per CU by LDS); without
 *              gamma the plain apply's arithmetic, the back-transform fused into the store
 * u comes from a value source: the population (no transform) or the dense U.  Rows of positions that do not count are never read;
 * their rows of U, Z and Y are +0.0.  Z is not read by the scaled pass, so Y may be written over it.
 */
#include <string.h>

#include <string>

#include "abz_adjust.h"

#define ADJ_KS 4            /* scaled apply: parameter columns k per thread and trip (two accumulators each) */

/* the transforms: kind[d] and lo_hi[d][2] (DEVICE arrays); kind == NULL: every transform is the identity */
struct AdjTf {
  const int32_t* kind;
  const double* lo_hi;
};
__device__ inline double adj_back(const AdjTf& tf, int k, double v) {
  return tf.kind ? abz_adjust_back(tf.kind[k], tf.lo_hi[2 * k], tf.lo_hi[2 * k + 1], v) : v;
}

/* ---- transform: U[i][k] = forward_k(x_ik) for the counting positions, +0.0 for the others; k < d */
__global__ __launch_bounds__(ABZ_BLOCK) void adj_transform_kernel(const PopSource src, const AdjTf tf, double* __restrict__ U, int ldu) {
  const int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + threadIdx.x;
  if (i >= src.N) return;
  const int d = src.cols();
  double* urow = U + (size_t)i * (size_t)ldu;
  if (sum_weight(src, i) > 0.0) {
    const double* xrow = src.row(i);
    for (int k = 0; k < d; ++k) urow[k] = abz_adjust_forward(tf.kind[k], tf.lo_hi[2 * k], tf.lo_hi[2 * k + 1], src.value(xrow, k));
  } else {
    for (int k = 0; k < d; ++k) urow[k] = 0.0;
  }
}

/* ---- log residuals: Z[i][k] = abz_log(e e), e = (u_ik - x_mean[k]) - sum_j beta[j][k] (s_ij - s_mean[j]); +0.0 where w <= 0 */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK) void adj_logres_kernel(const S src, const AdjBlobs b, const double* __restrict__ s_mean,
                                                               const double* __restrict__ x_mean, const double* __restrict__ beta,
                                                               double* __restrict__ Z, int ldz) {
  __shared__ double s_beta[ABZ_ADJUST_MAX_C * ADJ_KA];           /* [j][a]: beta[j][k0 + a] of the chunk */
  __shared__ double s_sm[ABZ_ADJUST_MAX_C];
  __shared__ int s_col[ABZ_ADJUST_MAX_C];
  const int t = threadIdx.x;
  const int d = src.cols(), c = b.c;
  const int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t;
  for (int j = t; j < c; j += ABZ_BLOCK) { s_sm[j] = s_mean[j]; s_col[j] = b.cols[j]; }
  const bool inside = i < src.N;
  bool live = false;
  if (inside) live = sum_weight(src, i) > 0.0;
  const double* srow = nullptr;
  const double* urow = nullptr;
  if (live) { srow = adj_srow(b, i); urow = src.row(i); }
  double* zrow = inside ? Z + (size_t)i * (size_t)ldz : nullptr;
  for (int k0 = 0; k0 < d; k0 += ADJ_KA) {                       /* block-uniform */
    __syncthreads();                                             /* the chunk before has been read (first trip: s_sm, s_col are in) */
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
        const double ds = srow[s_col[j]] - s_sm[j];
#pragma unroll
        for (int a = 0; a < ADJ_KA; ++a) acc[a] = acc[a] + s_beta[j * ADJ_KA + a] * ds;
      }
#pragma unroll
      for (int a = 0; a < ADJ_KA; ++a)
        if (k0 + a < d) zrow[k0 + a] = abz_adjust_logres(abz_adjust_residual(src.value(urow, k0 + a), x_mean[k0 + a], acc[a]));
    } else if (inside) {
#pragma unroll
      for (int a = 0; a < ADJ_KA; ++a)
        if (k0 + a < d) zrow[k0 + a] = 0.0;
    }
  }
}

/* ---- scaled apply.  HCORR: Y[i][k] = back_k(m[k] + e exp(-0.5 a2)), e as above, a2 = sum_j gamma[j][k] (s_ij - t_j); otherwise
 * Y[i][k] = back_k(u_ik - sum_j beta[j][k] (s_ij - t_j)), the plain apply behind a transform.  +0.0 where w <= 0. */
struct AdjScaled {
  const double *s_mean, *target, *beta, *gamma, *x_mean, *m;     /* DEVICE; s_mean, gamma, x_mean, m only with HCORR */
};
template <class S, bool HCORR>
__global__ __launch_bounds__(ABZ_BLOCK) void adj_scaled_kernel(const S src, const AdjBlobs b, const AdjScaled g, const AdjTf tf,
                                                               double* __restrict__ Y, int ldy) {
  __shared__ double s_beta[ABZ_ADJUST_MAX_C * ADJ_KS];           /* [j][a]: beta[j][k0 + a] of the chunk */
  __shared__ double s_gamma[HCORR ? ABZ_ADJUST_MAX_C * ADJ_KS : 1];
  __shared__ double s_t[ABZ_ADJUST_MAX_C];
  __shared__ double s_sm[HCORR ? ABZ_ADJUST_MAX_C : 1];
  __shared__ int s_col[ABZ_ADJUST_MAX_C];
  const int t = threadIdx.x;
  const int d = src.cols(), c = b.c;
  const int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t;
  for (int j = t; j < c; j += ABZ_BLOCK) {
    s_t[j] = g.target[j]; s_col[j] = b.cols[j];
    if (HCORR) s_sm[j] = g.s_mean[j];
  }
  const bool inside = i < src.N;
  bool live = false;
  if (inside) live = sum_weight(src, i) > 0.0;
  const double* srow = nullptr;
  const double* urow = nullptr;
  if (live) { srow = adj_srow(b, i); urow = src.row(i); }
  double* yrow = inside ? Y + (size_t)i * (size_t)ldy : nullptr;
  for (int k0 = 0; k0 < d; k0 += ADJ_KS) {                       /* block-uniform */
    __syncthreads();                                             /* the chunk before has been read (first trip: s_t, s_sm, s_col are in) */
    for (int idx = t; idx < c * ADJ_KS; idx += ABZ_BLOCK) {
      const int j = idx / ADJ_KS, a = idx - j * ADJ_KS;
      s_beta[idx] = k0 + a < d ? g.beta[(size_t)j * d + k0 + a] : 0.0;
      if (HCORR) s_gamma[idx] = k0 + a < d ? g.gamma[(size_t)j * d + k0 + a] : 0.0;
    }
    __syncthreads();
    if (live) {
      double acc1[ADJ_KS], acc2[ADJ_KS];
#pragma unroll
      for (int a = 0; a < ADJ_KS; ++a) { acc1[a] = 0.0; acc2[a] = 0.0; }
#pragma unroll 4
      for (int j = 0; j < c; ++j) {
        const double s = srow[s_col[j]];
        const double dt = s - s_t[j];
        if (HCORR) {
          const double dm = s - s_sm[j];
#pragma unroll
          for (int a = 0; a < ADJ_KS; ++a) {
            acc1[a] = acc1[a] + s_beta[j * ADJ_KS + a] * dm;
            acc2[a] = acc2[a] + s_gamma[j * ADJ_KS + a] * dt;
          }
        } else {
#pragma unroll
          for (int a = 0; a < ADJ_KS; ++a) acc1[a] = acc1[a] + s_beta[j * ADJ_KS + a] * dt;
        }
      }
#pragma unroll
      for (int a = 0; a < ADJ_KS; ++a) {
        const int k = k0 + a;
        if (k < d) {
          const double u = src.value(urow, k);
          const double v = HCORR ? abz_adjust_scaled(g.m[k], abz_adjust_residual(u, g.x_mean[k], acc1[a]), acc2[a]) : u - acc1[a];
          yrow[k] = adj_back(tf, k, v);
        }
      }
    } else if (inside) {
#pragma unroll
      for (int a = 0; a < ADJ_KS; ++a)
        if (k0 + a < d) yrow[k0 + a] = 0.0;
    }
  }
}

/* ================================================================ host side */
static unsigned adj_blocks(int64_t N) { return (unsigned)((N + ABZ_BLOCK - 1) / ABZ_BLOCK); }

int abz_adjust_transform_impl(abcdez_ctx* ctx, const SumPop& p, const int32_t* tf_kind, const double* tf_lo_hi, double* U, int ldu) {
  const int d = p.d;
  AdjStage st;
  const int i_kind = st.add(tf_kind, (size_t)d * 4), i_lh = st.add(tf_lo_hi, (size_t)d * 16);
  int rc = st.commit(ctx, 0);
  if (rc) return rc;
  const AdjTf tf{st.at<int32_t>(i_kind), st.at<double>(i_lh)};
  hipLaunchKernelGGL(adj_transform_kernel, dim3(adj_blocks(p.N)), dim3(ABZ_BLOCK), 0, ctx->stream, pop_source(ctx, p), tf, U, ldu);
  ABZ_HIP_CHECK(hipGetLastError());
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int abz_adjust_cross_dense_impl(abcdez_ctx* ctx, const ColView& v, const double* Sb, int lds, const int32_t* cols, int c,
                                const double* s_mean, const double* x_mean, double* S_out) {
  return adj_cross_run(ctx, v, Sb, lds, cols, c, s_mean, x_mean, S_out);
}

/* the dense source of u for the population p: U[N][ldu] under p's weights */
static ColView adj_dense(const SumPop& p, const double* U, int ldu) { return ColView{U, p.wns, p.N, ldu, p.d}; }

int abz_adjust_logres_impl(abcdez_ctx* ctx, const SumPop& p, const double* U, int ldu, const double* Sb, int lds, const int32_t* cols,
                           int c, const double* s_mean, const double* x_mean, const double* beta, double* Z, int ldz) {
  const int d = p.d;
  if (!adj_all_finite(s_mean, (size_t)c) || !adj_all_finite(x_mean, (size_t)d)) {
    abz_set_error("adjust: a mean of the simulated data or of the parameters is not finite");
    return -1;
  }
  if (!adj_all_finite(beta, (size_t)c * (size_t)d)) { abz_set_error("adjust: a regression coefficient is not finite"); return -1; }
  AdjStage st;
  const int i_cols = st.add_cols(cols, c), i_sm = st.add(s_mean, (size_t)c * 8), i_xm = st.add(x_mean, (size_t)d * 8),
            i_beta = st.add(beta, (size_t)c * (size_t)d * 8);
  int rc = st.commit(ctx, 0);
  if (rc) return rc;
  const AdjBlobs b{Sb, st.at<int32_t>(i_cols), lds, c};
  const dim3 grid(adj_blocks(p.N)), block(ABZ_BLOCK);
  if (U)
    hipLaunchKernelGGL(adj_logres_kernel<ColView>, grid, block, 0, ctx->stream, adj_dense(p, U, ldu), b, st.at<double>(i_sm),
                       st.at<double>(i_xm), st.at<double>(i_beta), Z, ldz);
  else
    hipLaunchKernelGGL(adj_logres_kernel<PopSource>, grid, block, 0, ctx->stream, pop_source(ctx, p), b, st.at<double>(i_sm),
                       st.at<double>(i_xm), st.at<double>(i_beta), Z, ldz);
  ABZ_HIP_CHECK(hipGetLastError());
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

template <class S>
static void adj_scaled_launch(abcdez_ctx* ctx, const S& src, const AdjBlobs& b, const AdjScaled& g, const AdjTf& tf, double* Y, int ldy) {
  const dim3 grid(adj_blocks(src.N)), block(ABZ_BLOCK);
  if (g.gamma)
    hipLaunchKernelGGL((adj_scaled_kernel<S, true>), grid, block, 0, ctx->stream, src, b, g, tf, Y, ldy);
  else
    hipLaunchKernelGGL((adj_scaled_kernel<S, false>), grid, block, 0, ctx->stream, src, b, g, tf, Y, ldy);
}

int abz_adjust_apply_scaled_impl(abcdez_ctx* ctx, const SumPop& p, const double* U, int ldu, const double* Sb, int lds, const int32_t* cols,
                                 int c, const double* target, const double* beta, const double* s_mean, const double* x_mean,
                                 const double* gamma, const double* m, const int32_t* tf_kind, const double* tf_lo_hi, double* Y, int ldy) {
  const int d = p.d;
  const size_t cd = (size_t)c * (size_t)d;
  if (!adj_all_finite(target, (size_t)c)) { abz_set_error("adjust: the target is not finite"); return -1; }
  if (!adj_all_finite(beta, cd) || (gamma && !adj_all_finite(gamma, cd))) {
    abz_set_error("adjust: a regression coefficient is not finite");
    return -1;
  }
  if (gamma && (!adj_all_finite(s_mean, (size_t)c) || !adj_all_finite(x_mean, (size_t)d) || !adj_all_finite(m, (size_t)d))) {
    abz_set_error("adjust: a mean of the simulated data or of the parameters is not finite");
    return -1;
  }
  AdjStage st;
  const int i_cols = st.add_cols(cols, c), i_t = st.add(target, (size_t)c * 8), i_beta = st.add(beta, cd * 8);
  const int i_sm = st.add(gamma ? s_mean : nullptr, (size_t)c * 8), i_xm = st.add(gamma ? x_mean : nullptr, (size_t)d * 8);
  const int i_gamma = st.add(gamma, cd * 8), i_m = st.add(gamma ? m : nullptr, (size_t)d * 8);
  const int i_kind = st.add(tf_kind, (size_t)d * 4), i_lh = st.add(tf_kind ? tf_lo_hi : nullptr, (size_t)d * 16);
  int rc = st.commit(ctx, 0);
  if (rc) return rc;
  const AdjBlobs b{Sb, st.at<int32_t>(i_cols), lds, c};
  const AdjScaled g{st.at<double>(i_sm), st.at<double>(i_t), st.at<double>(i_beta), st.at<double>(i_gamma), st.at<double>(i_xm),
                    st.at<double>(i_m)};
  const AdjTf tf{st.at<int32_t>(i_kind), st.at<double>(i_lh)};
  if (U)
    adj_scaled_launch(ctx, adj_dense(p, U, ldu), b, g, tf, Y, ldy);
  else
    adj_scaled_launch(ctx, pop_source(ctx, p), b, g, tf, Y, ldy);
  ABZ_HIP_CHECK(hipGetLastError());
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}
