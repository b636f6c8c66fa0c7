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
 * The host solves for beta between the two (c x c, a few thousand operations).  Both calls only read the population and the blobs;
 * their scratch is the summaries' buffer, so a select enqueued ahead and every other state of the context survive them.  Rows of
 * positions that do not count (w <= 0) are never read; their rows of Y are +0.0.
 */
#include <float.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "abz_ctx.h"
#include "abz_device.h"
#include "abz_summary.h"

#define ADJ_JB 4            /* cross: blob columns j held per thread */
#define ADJ_KC 1            /* cross: parameter columns k streamed per trip */
#define ADJ_KA 8            /* apply: parameter columns k (accumulators) per thread and trip */

/* the blob matrix Sb[N][lds] and the c chosen columns (DEVICE array) */
struct AdjBlobs {
  const double* Sb;
  const int32_t* cols;
  int lds, c;
};

/* bit q of the result = the slot of the current row of position q of the thread (tile_pos) where w[q] > 0.0: the population's
 * rows without 8 row pointers in registers */
__device__ inline uint32_t adj_slots(const SumPop& p, int64_t base, const double (&w)[8]) {
  uint32_t slots = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (w[q] > 0.0 && p.bits && packed_bit(p.bits, tile_pos(base, q))) slots |= 1u << q;
  return slots;
}
__device__ inline const double* adj_xrow(const SumPop& p, int64_t i, uint32_t slot) {
  return (slot ? p.slot1 : p.slot0) + (size_t)i * (size_t)p.ld;
}
__device__ inline const double* adj_srow(const AdjBlobs& b, int64_t i) { return b.Sb + (size_t)i * (size_t)b.lds; }

/* ---- cross moments: parts[(j d + k) nt + tile] = tile sum of w (s_j - smean_j) (x_k - xmean_k), j < c, k < d */
__global__ __launch_bounds__(ABZ_BLOCK, 3) void adj_cross_kernel(const abz_model* __restrict__ M, const SumPop p, const AdjBlobs b,
                                                                 const double* __restrict__ s_mean, const double* __restrict__ x_mean,
                                                                 double* __restrict__ parts) {
  __shared__ double s_acc[ADJ_JB * ABZ_MAX_D][4];                /* (a, k) -> the four waves' sums */
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t nt = gridDim.x, tile = blockIdx.x;
  const int d = p.d, c = b.c;
  double w[8];
  (void)tile_weights(p, tile * ABZ_TILE, w);
  const uint32_t slots = adj_slots(p, tile * ABZ_TILE, w);
  for (int jb = 0; jb < c; jb += ADJ_JB) {                       /* block-uniform */
    double cj[ADJ_JB][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int a = 0; a < ADJ_JB; ++a) {
        const int j = jb + a;
        cj[a][q] = (w[q] > 0.0 && j < c) ? adj_srow(b, tile_pos(tile * ABZ_TILE, q))[b.cols[j]] - s_mean[j] : 0.0;
      }
    }
    for (int kb = 0; kb < d; kb += ADJ_KC) {
      double ck[ADJ_KC][8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int g = 0; g < ADJ_KC; ++g) {
          const int k = kb + g;
          ck[g][q] = (w[q] > 0.0 && k < d)
                         ? abz_push_p(&M->prior[k], adj_xrow(p, tile_pos(tile * ABZ_TILE, q), (slots >> q) & 1u)[k]) - x_mean[k]
                         : 0.0;
        }
      }
#pragma unroll
      for (int a = 0; a < ADJ_JB; ++a) {
#pragma unroll
        for (int g = 0; g < ADJ_KC; ++g) {
          const int j = jb + a, k = kb + g;
          if (j < c && k < d) {                                  /* block-uniform */
            double e[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) e[q] = w[q] > 0.0 ? w[q] * (cj[a][q] * ck[g][q]) : 0.0;   /* abz_summary_term2 on centred values */
            const double s = tile_wave_tree(e);
            if ((t & 63) == 0) s_acc[a * d + k][wave] = s;
          }
        }
      }
    }
    __syncthreads();
    for (int idx = t; idx < ADJ_JB * d; idx += ABZ_BLOCK) {
      const int a = idx / d, k = idx - a * d, j = jb + a;
      if (j < c) parts[((size_t)j * d + k) * nt + tile] = (s_acc[idx][0] + s_acc[idx][1]) + (s_acc[idx][2] + s_acc[idx][3]);
    }
    __syncthreads();
  }
}

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
static bool adj_all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(fabs(v[i]) <= DBL_MAX)) return false;
  return true;
}
/* cols (identity when NULL) and the host vectors a pass needs, into the summaries' buffer: [ cols c x i32 | a | b | room ]; the
 * device addresses come back in *d_cols, *d_a, *d_b, *d_room.  The host copies must live until the call's synchronisation. */
static int adj_stage(abcdez_ctx* ctx, const int32_t* cols, int c, std::vector<int32_t>& h_cols, const double* a, size_t na, const double* b,
                     size_t nb, size_t room_bytes, const int32_t** d_cols, const double** d_a, const double** d_b, char** d_room) {
  const size_t o_a = abz_align((size_t)c * 4), o_b = o_a + abz_align(na * 8), o_room = o_b + abz_align(nb * 8);
  int rc = sum_ws_reserve(ctx, o_room + room_bytes);
  if (rc) return rc;
  char* base = (char*)ctx->sum_ws;
  h_cols.resize((size_t)c);
  for (int j = 0; j < c; ++j) h_cols[(size_t)j] = cols ? cols[j] : j;
  ABZ_HIP_CHECK(hipMemcpyAsync(base, h_cols.data(), (size_t)c * 4, hipMemcpyHostToDevice, ctx->stream));
  ABZ_HIP_CHECK(hipMemcpyAsync(base + o_a, a, na * 8, hipMemcpyHostToDevice, ctx->stream));
  ABZ_HIP_CHECK(hipMemcpyAsync(base + o_b, b, nb * 8, hipMemcpyHostToDevice, ctx->stream));
  *d_cols = (const int32_t*)base; *d_a = (const double*)(base + o_a); *d_b = (const double*)(base + o_b); *d_room = base + o_room;
  return 0;
}

int abz_adjust_cross_impl(abcdez_ctx* ctx, const SumPop& p, const double* Sb, int lds, const int32_t* cols, int c, const double* s_mean,
                          const double* x_mean, double* S_sx_out) {
  const int d = p.d;
  if (!adj_all_finite(s_mean, (size_t)c) || !adj_all_finite(x_mean, (size_t)d)) {
    abz_set_error("adjust: a mean of the simulated data or of the parameters is not finite");
    return -1;
  }
  const size_t nt = (size_t)((p.N + ABZ_TILE - 1) / ABZ_TILE), ntrees = (size_t)c * (size_t)d;
  /* room: [ results c d | partials c d x nt ] */
  const size_t o_parts = abz_align(ntrees * 8);
  std::vector<int32_t> h_cols;
  const int32_t* d_cols;
  const double *d_smean, *d_xmean;
  char* room;
  int rc = adj_stage(ctx, cols, c, h_cols, s_mean, (size_t)c, x_mean, (size_t)d, o_parts + ntrees * nt * 8, &d_cols, &d_smean, &d_xmean, &room);
  if (rc) return rc;
  double* res = (double*)room;
  double* parts = (double*)(room + o_parts);
  const AdjBlobs b{Sb, d_cols, lds, c};
  hipLaunchKernelGGL(adj_cross_kernel, dim3((unsigned)nt), dim3(ABZ_BLOCK), 0, ctx->stream, (const abz_model*)ctx->d_model, p, b, d_smean,
                     d_xmean, parts);
  ABZ_HIP_CHECK(hipGetLastError());
  rc = abz_sum_finish(ctx, parts, (int64_t)nt, res, (unsigned)ntrees);
  if (rc) return rc;
  ABZ_HIP_CHECK(hipMemcpyAsync(S_sx_out, res, ntrees * 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int abz_adjust_apply_impl(abcdez_ctx* ctx, const SumPop& p, const double* Sb, int lds, const int32_t* cols, int c, const double* target,
                          const double* beta, double* Y, int ldy) {
  const int d = p.d;
  if (!adj_all_finite(target, (size_t)c)) { abz_set_error("adjust: the target is not finite"); return -1; }
  if (!adj_all_finite(beta, (size_t)c * (size_t)d)) { abz_set_error("adjust: a regression coefficient is not finite"); return -1; }
  std::vector<int32_t> h_cols;
  const int32_t* d_cols;
  const double *d_target, *d_beta;
  char* room;
  int rc = adj_stage(ctx, cols, c, h_cols, target, (size_t)c, beta, (size_t)c * (size_t)d, 0, &d_cols, &d_target, &d_beta, &room);
  if (rc) return rc;
  const AdjBlobs b{Sb, d_cols, lds, c};
  hipLaunchKernelGGL(adj_apply_kernel, dim3((unsigned)((p.N + ABZ_BLOCK - 1) / ABZ_BLOCK)), dim3(ABZ_BLOCK), 0, ctx->stream,
                     (const abz_model*)ctx->d_model, p, b, d_target, d_beta, Y, ldy);
  ABZ_HIP_CHECK(hipGetLastError());
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}
