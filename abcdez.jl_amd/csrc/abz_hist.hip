/*
 * abz_hist.hip -- marginal and pairwise histograms of the population where it lives (include/abcdez_spec.h, "posterior summaries",
 * histograms): every counting position adds its integer mass abz_weight_fix(w_i, N) to the bin of abz_hist_bin.  Sums of integers
 * only, so the 64-bit atomics below have no order to get wrong and the result is bit for bit the literal restatement in
 * abcdez_amd/summary.py (hist_reference).
 *
 *   range   (automatic ranges only) smallest and largest order key of every requested column over the counting positions,
 *           8 columns a launch, each launch reads its own columns of the current rows
 *   setup   per column (lo, hi) -- given, or from the keys, a constant column widened by 0.5 -- and the two scales
 *   bin     one thread per position reads its current row ONCE and writes the mass (8 B), per requested column the 1-D bin as
 *           u16 (bins, bins + 1, bins + 2 = under, over, NaN) and, when pairs are asked for, the 2-D bin as u8 (255 = outside),
 *           both column-major; M and n_mass by integer reduction
 *   1-D     LDS histograms of 64-bit masses, bins + 3 cells a column, as many columns per workgroup as fit H1_CELLS: the masses
 *           are read once per column group (once in all for 32 columns at 64 bins)
 *   pairs   a workgroup holds the masses and the u8 column j of its positions in registers while up to HB_K columns k stream
 *           past, one LDS histogram per pair (j, k) of the batch; bins2^2 cells a pair, H2_CELLS in all.  A pair that does not fit
 *           (bins2 > 90) is cut into row ranges of b_j, one batch each.
 * Non-empty LDS cells are flushed with global 64-bit integer atomics into zeroed outputs.  The host reads [M, n_mass, error |
 * lo, hi | 1-D cells] and the 2-D cells after ONE synchronisation; no state survives the call.  Only range and bin read values: they
 * are templates over the value source of abz_summary.h, and the same driver serves a dense per-particle matrix
 * (abz_columns_histograms_impl).
 */
#include <string.h>

#include <string>
#include <vector>

#include "abz_ctx.h"
#include "abz_device.h"
#include "abz_summary.h"

#define HB_K 16               /* pairs (columns k) per batch */
#define H1_CELLS 5120         /* 40 KB: 1-D cells per workgroup */
#define H2_CELLS 8192         /* 64 KB: 2-D cells per workgroup */
/* H_RC (abz_summary.h): range, columns per launch (64 bytes of a row; 16 spill scalar registers) */
#define H_VEC 4               /* positions per thread and tile in the two histogram passes */
#define H_TILE (ABZ_BLOCK * H_VEC)
#define H_PAD 16              /* the column stride is a multiple of this: 4 x u16 and 4 x u8 loads stay aligned */
#define H_RANGE_BLOCKS 1024
#define H_BIN_BLOCKS 4096
#define H_PASS_BLOCKS 128     /* pairs: blocks per batch at most */
#define H_PASS_WORKGROUPS 2048 /* both histogram passes: workgroups in all, about */
#define H_OUTSIDE 255u

typedef unsigned long long u64;

/* HistCol (abz_summary.h): a requested column, its range and the two scales */
struct HistBatch { int32_t cj, n, r0, r1; int32_t ck[HB_K]; int32_t pair[HB_K]; };

/* ---- range: krange[2 c + {0, 1}] = (smallest, largest) order key of requested column c over the counting positions, for the
 * columns c0 .. c0 + ncols - 1 of the list */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK) void hist_range_kernel(const S p, const HistCol* __restrict__ cols, int c0, int ncols,
                                                              u64* __restrict__ krange) {
  __shared__ u64 s_kmin[H_RC], s_kmax[H_RC];
  __shared__ int s_col[H_RC];
  const int t = threadIdx.x;
  if (t < H_RC) { s_kmin[t] = ~0ull; s_kmax[t] = 0ull; s_col[t] = t < ncols ? cols[c0 + t].col : 0; }
  __syncthreads();
  u64 kmin[H_RC], kmax[H_RC];
#pragma unroll
  for (int c = 0; c < H_RC; ++c) { kmin[c] = ~0ull; kmax[c] = 0ull; }
  const int b = abz_stratum_bits((uint32_t)p.N);
  bool any = false;
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < p.N; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    if (sum_mass(p, i, b) < 1) continue;
    any = true;
    const double* row = p.row(i);
#pragma unroll
    for (int c = 0; c < H_RC; ++c) {
      if (c < ncols) {
        const u64 key = f64_order_key(p.value(row, s_col[c]));
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

/* ---- setup: the range and the scales of every requested column; hdr[3] = nc - c for the first column c whose automatic range
 * cannot be used (0: none) */
__global__ __launch_bounds__(ABZ_BLOCK) void hist_setup_kernel(HistCol* __restrict__ cols, int nc, int automatic,
                                                              const u64* __restrict__ krange, int bins, int bins2,
                                                              double* __restrict__ lohi, u64* __restrict__ hdr) {
  for (int c = threadIdx.x; c < nc; c += ABZ_BLOCK) {
    double lo = cols[c].lo, hi = cols[c].hi;
    if (automatic) {
      lo = f64_from_order_key_dev(krange[2 * c]);
      hi = f64_from_order_key_dev(krange[2 * c + 1]);
      if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
      const double w = hi - lo;
      const double big = 0x1.fffffffffffffp1023;
      if (!(lo < hi) || !(lo >= -big) || !(hi <= big) || !(w <= big))   /* NaN fails every comparison */
        atomicMax(&hdr[3], (u64)(nc - c));
    }
    cols[c].lo = lo; cols[c].hi = hi;
    cols[c].scale = abz_hist_scale(lo, hi, bins);
    cols[c].scale2 = abz_hist_scale(lo, hi, bins2 > 0 ? bins2 : 1);
    lohi[2 * c] = lo; lohi[2 * c + 1] = hi;
  }
}

/* ---- bin: mass[i] for i < Nld (0 beyond N), idx1[c Nld + i] and idx2[c Nld + i] (when idx2) for the counting positions;
 * tot[0] = sum of the low 32 bits of the masses, tot[1] = sum of the high 32 bits, tot[2] = n_mass */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK) void hist_bin_kernel(const S p, const HistCol* __restrict__ cols, int nc, int bins, int bins2,
                                                            int64_t Nld, u64* __restrict__ mass, uint16_t* __restrict__ idx1,
                                                            uint8_t* __restrict__ idx2, u64* __restrict__ tot) {
  const int t = threadIdx.x;
  u64 lo = 0, hi = 0, cnt = 0;
  const int b = abz_stratum_bits((uint32_t)p.N);
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < Nld; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    const u64 m = i < p.N ? sum_mass(p, i, b) : 0ull;
    mass[i] = m;
    if (m < 1) continue;
    lo += m & 0xFFFFFFFFull; hi += m >> 32; cnt += 1;
    const double* row = p.row(i);
    for (int c = 0; c < nc; ++c) {
      const HistCol h = cols[c];
      const double x = p.value(row, h.col);
      idx1[(size_t)c * (size_t)Nld + (size_t)i] = (uint16_t)abz_hist_bin(x, h.lo, h.hi, h.scale, bins);
      if (idx2) {
        const int32_t b2 = abz_hist_bin(x, h.lo, h.hi, h.scale2, bins2);
        idx2[(size_t)c * (size_t)Nld + (size_t)i] = (uint8_t)(b2 >= bins2 ? H_OUTSIDE : (uint32_t)b2);
      }
    }
  }
  sum_mass_tally(lo, hi, cnt, tot);
}

/* the four masses of a thread's positions i .. i + 3 (i a multiple of 4, the array 16-byte aligned) */
__device__ inline void hist_load_mass(const u64* __restrict__ mass, int64_t i, u64 m[H_VEC]) {
  const ulonglong2 a = *(const ulonglong2*)(mass + i), c = *(const ulonglong2*)(mass + i + 2);
  m[0] = a.x; m[1] = a.y; m[2] = c.x; m[3] = c.y;
}

/* ---- 1-D: out[(c0 + c) (bins + 3) + cell] += mass for the columns c0 = blockIdx.y G .. of the list; grid (blocks, groups) */
__global__ __launch_bounds__(ABZ_BLOCK) void hist_1d_kernel(const u64* __restrict__ mass, const uint16_t* __restrict__ idx1,
                                                           int64_t Nld, int nc, int G, int bins, u64* __restrict__ out) {
  __shared__ u64 s_hist[H1_CELLS];
  const int t = threadIdx.x, c0 = blockIdx.y * G, stride = bins + 3;
  const int n = nc - c0 < G ? nc - c0 : G;
  const int cells = n * stride;                      /* <= H1_CELLS: G = H1_CELLS / stride on the host */
  for (int j = t; j < cells; j += ABZ_BLOCK) s_hist[j] = 0ull;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * H_TILE; base < Nld; base += (int64_t)gridDim.x * H_TILE) {
    const int64_t i = base + (int64_t)t * H_VEC;
    if (i >= Nld) continue;
    u64 m[H_VEC];
    hist_load_mass(mass, i, m);
    if (!(m[0] | m[1] | m[2] | m[3])) continue;
    for (int c = 0; c < n; ++c) {
      const uint2 v = *(const uint2*)(idx1 + (size_t)(c0 + c) * (size_t)Nld + (size_t)i);
      const uint32_t bin[H_VEC] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16};
      int cur = -1;                                  /* a thread's run of positions in one bin costs one atomic */
      u64 acc = 0;
#pragma unroll
      for (int j = 0; j < H_VEC; ++j) {
        if (!m[j]) continue;
        const int cell = c * stride + (int)(bin[j] < (uint32_t)stride ? bin[j] : (uint32_t)stride - 1u);
        if (cell == cur) { acc += m[j]; continue; }
        if (cur >= 0) atomicAdd(&s_hist[cur], acc);
        cur = cell; acc = m[j];
      }
      if (cur >= 0) atomicAdd(&s_hist[cur], acc);
    }
  }
  __syncthreads();
  u64* o = out + (size_t)c0 * (size_t)stride;
  for (int j = t; j < cells; j += ABZ_BLOCK) {
    const u64 v = s_hist[j];
    if (v) atomicAdd(&o[j], v);
  }
}

/* ---- pairs: batch blockIdx.y = column cj of the list against the columns ck[0 .. n), rows r0 <= b_j < r1 of the cell space:
 * out[pair[q] bins2^2 + b_j bins2 + b_k] += mass; grid (blocks, batches) */
__global__ __launch_bounds__(ABZ_BLOCK) void hist_pair_kernel(const u64* __restrict__ mass, const uint8_t* __restrict__ idx2,
                                                             int64_t Nld, const HistBatch* __restrict__ batches, int bins2,
                                                             u64* __restrict__ out) {
  __shared__ u64 s_hist[H2_CELLS];
  const int t = threadIdx.x;
  const HistBatch* __restrict__ bt = batches + blockIdx.y;
  const int n = bt->n, r0 = bt->r0, r1 = bt->r1;
  const int seg = (r1 - r0) * bins2;                 /* n seg <= H2_CELLS: the host's batching */
  const int cells = n * seg;
  for (int j = t; j < cells; j += ABZ_BLOCK) s_hist[j] = 0ull;
  __syncthreads();
  const uint8_t* cj = idx2 + (size_t)bt->cj * (size_t)Nld;
  for (int64_t base = (int64_t)blockIdx.x * H_TILE; base < Nld; base += (int64_t)gridDim.x * H_TILE) {
    const int64_t i = base + (int64_t)t * H_VEC;
    if (i >= Nld) continue;
    u64 m[H_VEC];
    hist_load_mass(mass, i, m);
    if (!(m[0] | m[1] | m[2] | m[3])) continue;
    const uint32_t vj = *(const uint32_t*)(cj + i);
    int row[H_VEC];                                  /* (b_j - r0) bins2, or -1: no mass, outside, or another batch's rows */
    bool any = false;
#pragma unroll
    for (int j = 0; j < H_VEC; ++j) {
      const int bj = (int)((vj >> (8 * j)) & 255u);
      const bool ok = m[j] != 0ull && bj >= r0 && bj < r1;
      row[j] = ok ? (bj - r0) * bins2 : -1;
      any |= ok;
    }
    if (!any) continue;
    uint32_t vk[HB_K];                               /* all loads of the batch in flight before the first atomic */
#pragma unroll
    for (int q = 0; q < HB_K; ++q)
      vk[q] = q < n ? *(const uint32_t*)(idx2 + (size_t)bt->ck[q] * (size_t)Nld + (size_t)i) : 0xFFFFFFFFu;
#pragma unroll
    for (int q = 0; q < HB_K; ++q) {
      if (q < n) {
        int cur = -1;
        u64 acc = 0;
#pragma unroll
        for (int j = 0; j < H_VEC; ++j) {
          const uint32_t bk = (vk[q] >> (8 * j)) & 255u;
          if (row[j] < 0 || bk >= (uint32_t)bins2) continue;
          const int cell = q * seg + row[j] + (int)bk;
          if (cell == cur) { acc += m[j]; continue; }
          if (cur >= 0) atomicAdd(&s_hist[cur], acc);
          cur = cell; acc = m[j];
        }
        if (cur >= 0) atomicAdd(&s_hist[cur], acc);
      }
    }
  }
  __syncthreads();
  const size_t per = (size_t)bins2 * (size_t)bins2;
  for (int j = t; j < cells; j += ABZ_BLOCK) {
    const u64 v = s_hist[j];
    if (!v) continue;
    const int q = j / seg, rem = j - q * seg;
    atomicAdd(&out[(size_t)bt->pair[q] * per + (size_t)r0 * (size_t)bins2 + (size_t)rem], v);
  }
}

/* ================================================================ host side */
/* the histograms of a source; `call` names the entry point in the refusals */
template <class S>
static int histograms_drive(abcdez_ctx* ctx, const char* call, const S& src, const int32_t* cols, int nc, int bins, const double* range,
                            const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1, uint64_t* tallies1,
                            uint64_t* mass2, uint64_t* outside2, uint64_t* M_out, int64_t* n_mass) {
  const int64_t N = src.N;
  const int d = src.cols();
  /* the blob the host uploads: [ columns | key ranges | batches ] */
  std::vector<int> pos((size_t)d, -1);
  std::vector<HistCol> hc((size_t)nc);
  for (int c = 0; c < nc; ++c) {
    hc[c] = HistCol{};
    hc[c].col = cols ? cols[c] : c;
    if (range) { hc[c].lo = range[2 * c]; hc[c].hi = range[2 * c + 1]; }
    pos[hc[c].col] = c;
  }
  std::vector<HistBatch> batches;
  if (n_pairs > 0) {
    const int per = bins2 * bins2;
    int B = per <= H2_CELLS ? H2_CELLS / per : 1;
    B = B > HB_K ? HB_K : B;
    const int R = per <= H2_CELLS ? bins2 : H2_CELLS / bins2;              /* rows of b_j per batch */
    std::vector<std::vector<std::pair<int, int>>> by_j((size_t)nc);      /* column j of the list -> (column k, pair index) */
    for (int q = 0; q < n_pairs; ++q) by_j[pos[pairs[2 * q]]].push_back({pos[pairs[2 * q + 1]], q});
    for (int j = 0; j < nc; ++j) {
      const auto& v = by_j[j];
      for (size_t a = 0; a < v.size(); a += (size_t)B) {
        for (int r0 = 0; r0 < bins2; r0 += R) {
          HistBatch bt{};
          bt.cj = j; bt.r0 = r0; bt.r1 = r0 + R < bins2 ? r0 + R : bins2;
          bt.n = (int)(v.size() - a < (size_t)B ? v.size() - a : (size_t)B);
          for (int q = 0; q < bt.n; ++q) { bt.ck[q] = v[a + q].first; bt.pair[q] = v[a + q].second; }
          batches.push_back(bt);
        }
      }
    }
  }
  const size_t nbt = batches.size();
  const size_t b_cols = abz_align((size_t)nc * sizeof(HistCol)), b_kr = abz_align((size_t)nc * 16),
               b_bt = abz_align(nbt * sizeof(HistBatch));
  std::vector<char> blob(b_cols + b_kr + b_bt, 0);
  memcpy(blob.data(), hc.data(), (size_t)nc * sizeof(HistCol));
  for (int c = 0; c < nc; ++c) {
    const u64 init[2] = {~0ull, 0ull};
    memcpy(blob.data() + b_cols + (size_t)c * 16, init, 16);
  }
  if (nbt) memcpy(blob.data() + b_cols + b_kr, batches.data(), nbt * sizeof(HistBatch));

  const int stride = bins + 3;
  const int64_t Nld = (N + H_PAD - 1) / H_PAD * H_PAD;
  const size_t n_m1 = (size_t)nc * (size_t)stride, n_m2 = (size_t)n_pairs * (size_t)bins2 * (size_t)bins2;
  /* [ header 4 x u64 | lo, hi | 1-D cells | 2-D cells || blob | mass | idx1 | idx2 ]: the part before || is zeroed and read back */
  const size_t o_lohi = 256, o_m1 = o_lohi + abz_align((size_t)nc * 16), o_m2 = o_m1 + abz_align(n_m1 * 8),
               o_blob = o_m2 + abz_align(n_m2 * 8), o_mass = o_blob + blob.size(), o_idx1 = o_mass + abz_align((size_t)Nld * 8),
               o_idx2 = o_idx1 + abz_align((size_t)nc * (size_t)Nld * 2),
               o_end = o_idx2 + (n_pairs > 0 ? abz_align((size_t)nc * (size_t)Nld) : 0);
  int rc = sum_ws_reserve(ctx, o_end);
  if (rc) return rc;
  char* base = (char*)ctx->sum_ws;
  u64* hdr = (u64*)base;
  double* lohi = (double*)(base + o_lohi);
  u64* m1 = (u64*)(base + o_m1);
  u64* m2 = (u64*)(base + o_m2);
  HistCol* dcols = (HistCol*)(base + o_blob);
  u64* krange = (u64*)(base + o_blob + b_cols);
  const HistBatch* dbt = (const HistBatch*)(base + o_blob + b_cols + b_kr);
  u64* mass = (u64*)(base + o_mass);
  uint16_t* idx1 = (uint16_t*)(base + o_idx1);
  uint8_t* idx2 = n_pairs > 0 ? (uint8_t*)(base + o_idx2) : nullptr;

  ABZ_HIP_CHECK(hipMemsetAsync(base, 0, o_blob, ctx->stream));
  ABZ_HIP_CHECK(hipMemcpyAsync(base + o_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
  const int64_t nb64 = (N + ABZ_BLOCK - 1) / ABZ_BLOCK;
  if (!range) {
    const int nb = (int)(nb64 < H_RANGE_BLOCKS ? nb64 : H_RANGE_BLOCKS);
    for (int c0 = 0; c0 < nc; c0 += H_RC)
      hipLaunchKernelGGL(hist_range_kernel<S>, dim3((unsigned)nb), dim3(ABZ_BLOCK), 0, ctx->stream, src, (const HistCol*)dcols, c0,
                         nc - c0 < H_RC ? nc - c0 : H_RC, krange);
  }
  hipLaunchKernelGGL(hist_setup_kernel, dim3(1), dim3(ABZ_BLOCK), 0, ctx->stream, dcols, nc, range ? 0 : 1, (const u64*)krange, bins,
                     bins2, lohi, hdr);
  {
    const int64_t nbl = (Nld + ABZ_BLOCK - 1) / ABZ_BLOCK;
    const int nb = (int)(nbl < H_BIN_BLOCKS ? nbl : H_BIN_BLOCKS);
    hipLaunchKernelGGL(hist_bin_kernel<S>, dim3((unsigned)nb), dim3(ABZ_BLOCK), 0, ctx->stream, src, (const HistCol*)dcols, nc, bins,
                       bins2, Nld, mass, idx1, idx2, hdr);
  }
  const int64_t tiles = (Nld + H_TILE - 1) / H_TILE;
  {
    const int G = H1_CELLS / stride < nc ? H1_CELLS / stride : nc;        /* >= 1: bins + 3 <= 4099 */
    const int groups = (nc + G - 1) / G;
    int64_t want = (H_PASS_WORKGROUPS + groups - 1) / groups;               /* about 2048 workgroups in all, as for the pairs */
    want = want < 1 ? 1 : want;
    const int nb = (int)(tiles < want ? tiles : want);
    hipLaunchKernelGGL(hist_1d_kernel, dim3((unsigned)nb, (unsigned)groups), dim3(ABZ_BLOCK), 0, ctx->stream, (const u64*)mass,
                       (const uint16_t*)idx1, Nld, nc, G, bins, m1);
  }
  for (size_t b0 = 0; b0 < nbt; b0 += 32768) {                            /* gridDim.y stays below 65536 */
    const size_t nby = nbt - b0 < 32768 ? nbt - b0 : 32768;
    int64_t want = (int64_t)((H_PASS_WORKGROUPS + nbt - 1) / nbt);        /* about 2048 workgroups in all */
    want = want < 1 ? 1 : want > H_PASS_BLOCKS ? H_PASS_BLOCKS : want;
    const int nb = (int)(tiles < want ? tiles : want);
    hipLaunchKernelGGL(hist_pair_kernel, dim3((unsigned)nb, (unsigned)nby), dim3(ABZ_BLOCK), 0, ctx->stream, (const u64*)mass,
                       (const uint8_t*)idx2, Nld, dbt + b0, bins2, m2);
  }
  ABZ_HIP_CHECK(hipGetLastError());
  std::vector<u64> h((o_m1 + n_m1 * 8) / 8);
  ABZ_HIP_CHECK(hipMemcpyAsync(h.data(), base, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (n_m2) ABZ_HIP_CHECK(hipMemcpyAsync(mass2, m2, n_m2 * 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  uint64_t Mv = 0;
  int64_t nm = 0;
  if (sum_mass_verdict(call, h[0], h[1], h[2], &Mv, &nm)) return -1;
  if (h[3]) {
    const int c = nc - (int)h[3];
    abz_set_error(std::string(call) + ": the automatic range of column " + std::to_string(hc[c].col) +
                  " is not usable (a NaN or an infinity among the counting rows, or hi - lo not finite): pass a range");
    return -1;
  }
  *M_out = Mv;
  *n_mass = nm;
  memcpy(lo_hi, h.data() + o_lohi / 8, (size_t)nc * 16);
  for (int c = 0; c < nc; ++c) {
    const u64* src = h.data() + o_m1 / 8 + (size_t)c * (size_t)stride;
    memcpy(mass1 + (size_t)c * (size_t)bins, src, (size_t)bins * 8);
    for (int q = 0; q < 3; ++q) tallies1[3 * c + q] = src[bins + q];
  }
  const size_t per = (size_t)bins2 * (size_t)bins2;
  for (int q = 0; q < n_pairs; ++q) {                                     /* every counting position is in a cell or outside */
    uint64_t in = 0;
    for (size_t e = 0; e < per; ++e) in += mass2[(size_t)q * per + e];
    outside2[q] = Mv - in;
  }
  return 0;
}

int abz_posterior_histograms_impl(abcdez_ctx* ctx, const SumPop& p, const int32_t* cols, int nc, int bins, const double* range,
                                  const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1, uint64_t* tallies1,
                                  uint64_t* mass2, uint64_t* outside2, uint64_t* M_out, int64_t* n_mass) {
  return histograms_drive(ctx, "posterior_histograms", pop_source(ctx, p), cols, nc, bins, range, pairs, n_pairs, bins2, lo_hi, mass1,
                          tallies1, mass2, outside2, M_out, n_mass);
}
int abz_columns_histograms_impl(abcdez_ctx* ctx, const ColView& v, const int32_t* cols, int nc, int bins, const double* range,
                                const int32_t* pairs, int n_pairs, int bins2, double* lo_hi, uint64_t* mass1, uint64_t* tallies1,
                                uint64_t* mass2, uint64_t* outside2, uint64_t* M_out, int64_t* n_mass) {
  return histograms_drive(ctx, "columns_histograms", v, cols, nc, bins, range, pairs, n_pairs, bins2, lo_hi, mass1, tallies1, mass2,
                          outside2, M_out, n_mass);
}
