/* abz_adjust.h -- what the two translation units of the regression adjustment share (abz_adjust.hip: the plain method, version 670;
 * abz_adjust_hcorr.hip: bounded transforms and the heteroscedastic correction, version 680): the view of the blob matrix, the tuning
 * constants, the staging of a pass's host vectors in the summaries' buffer, and the CROSS pass, a template over the value sources
 * of abz_summary.h like the gathers of the posterior calls: one kernel text gives S_sx of the population's push_p-cast parameters
 * and S_sz (or S_su) of a dense N x d matrix, which is what makes the second regression bit for bit the first one's arithmetic. */
#pragma once
#include <float.h>
#include <math.h>

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
__device__ inline const double* adj_srow(const AdjBlobs& b, int64_t i) { return b.Sb + (size_t)i * (size_t)b.lds; }

/* bit q of the result = the slot of the current row of position q of the thread (tile_pos) where w[q] > 0.0: the population's
 * rows without 8 row pointers in registers.  A dense matrix has one slot. */
__device__ inline uint32_t adj_slots(const SumPop& p, int64_t base, const double (&w)[8]) {
  uint32_t slots = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (w[q] > 0.0 && p.bits && packed_bit(p.bits, tile_pos(base, q))) slots |= 1u << q;
  return slots;
}
__device__ inline uint32_t adj_slots(const ColView&, int64_t, const double (&)[8]) { return 0u; }
__device__ inline const double* adj_xrow(const SumPop& p, int64_t i, uint32_t slot) {
  return (slot ? p.slot1 : p.slot0) + (size_t)i * (size_t)p.ld;
}
__device__ inline const double* adj_xrow(const ColView& v, int64_t i, uint32_t) { return v.row(i); }

/* ---- cross moments: parts[(j d + k) nt + tile] = tile sum of w (s_j - smean_j) (x_k - xmean_k), j < c, k < d = src.cols():
 * one block = one tile, thread t owns the positions m*512 + 2t + c; 4 centred blob columns of the thread's 8 rows stay in registers
 * while the centred value columns stream past one at a time (two would spill at three waves per SIMD); the 4 x d sums of the
 * j-block are collected in LDS, c d partials per tile, the tree levels above the tile by the summaries' finishing launch */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK, 3) void adj_cross_kernel(const S src, const AdjBlobs b, const double* __restrict__ s_mean,
                                                                 const double* __restrict__ x_mean, double* __restrict__ parts) {
  __shared__ double s_acc[ADJ_JB * ABZ_MAX_D][4];                /* (a, k) -> the four waves' sums */
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t nt = gridDim.x, tile = blockIdx.x;
  const int d = src.cols(), c = b.c;
  double w[8];
  (void)tile_weights(src, tile * ABZ_TILE, w);
  const uint32_t slots = adj_slots(src, tile * ABZ_TILE, w);
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
                         ? src.value(adj_xrow(src, tile_pos(tile * ABZ_TILE, q), (slots >> q) & 1u), k) - x_mean[k]
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

/* ================================================================ host side */
static inline bool adj_all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(fabs(v[i]) <= DBL_MAX)) return false;
  return true;
}
/* the host vectors a pass needs, laid out in the summaries' buffer behind one another (256-byte aligned) with `room` bytes after
 * them: add() every vector, commit() reserves and enqueues the copies, at() gives the device address of a vector.  The host
 * copies must live until the call's synchronisation. */
struct AdjStage {
  struct Item { const void* host; size_t bytes, off; };
  std::vector<Item> items;
  std::vector<int32_t> h_cols;
  size_t end = 0;
  char* base = nullptr;
  int add(const void* host, size_t bytes) {
    items.push_back(Item{host, bytes, end});
    end += abz_align(bytes);
    return (int)items.size() - 1;
  }
  /* cols (identity when NULL) */
  int add_cols(const int32_t* cols, int c) {
    h_cols.resize((size_t)c);
    for (int j = 0; j < c; ++j) h_cols[(size_t)j] = cols ? cols[j] : j;
    return add(h_cols.data(), (size_t)c * 4);
  }
  int commit(abcdez_ctx* ctx, size_t room_bytes) {
    int rc = sum_ws_reserve(ctx, end + room_bytes);
    if (rc) return rc;
    base = (char*)ctx->sum_ws;
    for (const Item& it : items)
      if (it.host && it.bytes) ABZ_HIP_CHECK(hipMemcpyAsync(base + it.off, it.host, it.bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
  template <class T>
  const T* at(int item) const { return items[(size_t)item].host ? (const T*)(base + items[(size_t)item].off) : nullptr; }
  char* room() const { return base + end; }
};

/* the cross pass over a value source: S_out[c][src.cols()] (HOST), one synchronisation */
template <class S>
int adj_cross_run(abcdez_ctx* ctx, const S& src, const double* Sb, int lds, const int32_t* cols, int c, const double* s_mean,
                  const double* x_mean, double* S_out) {
  const int d = src.cols();
  if (!adj_all_finite(s_mean, (size_t)c) || !adj_all_finite(x_mean, (size_t)d)) {
    abz_set_error("adjust: a mean of the simulated data or of the parameters is not finite");
    return -1;
  }
  const size_t nt = (size_t)((src.N + ABZ_TILE - 1) / ABZ_TILE), ntrees = (size_t)c * (size_t)d;
  /* room: [ results c d | partials c d x nt ] */
  const size_t o_parts = abz_align(ntrees * 8);
  AdjStage st;
  const int i_cols = st.add_cols(cols, c), i_sm = st.add(s_mean, (size_t)c * 8), i_xm = st.add(x_mean, (size_t)d * 8);
  int rc = st.commit(ctx, o_parts + ntrees * nt * 8);
  if (rc) return rc;
  double* res = (double*)st.room();
  double* parts = (double*)(st.room() + o_parts);
  const AdjBlobs b{Sb, st.at<int32_t>(i_cols), lds, c};
  hipLaunchKernelGGL(adj_cross_kernel<S>, dim3((unsigned)nt), dim3(ABZ_BLOCK), 0, ctx->stream, src, b, st.at<double>(i_sm),
                     st.at<double>(i_xm), parts);
  ABZ_HIP_CHECK(hipGetLastError());
  rc = abz_sum_finish(ctx, parts, (int64_t)nt, res, (unsigned)ntrees);
  if (rc) return rc;
  ABZ_HIP_CHECK(hipMemcpyAsync(S_out, res, ntrees * 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}
