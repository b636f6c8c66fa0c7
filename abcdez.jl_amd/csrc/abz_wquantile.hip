/*
 * abz_wquantile.hip -- weighted marginal quantiles of the population where it lives (include/abcdez_spec.h, "posterior summaries",
 * weighted quantiles): every position carries the integer mass abz_weight_fix(w_i, N) of the resampler, the quantile is a rank
 * select over the cumulated masses.  Everything is integer sums, minima and maxima, so no evaluation order exists and the result
 * is bit for bit the literal restatement in abcdez_amd/summary.py.
 *
 * Columns are handled in chunks of up to WQ_CB (their keys fit 128 bytes of a row), probabilities in batches of WQ_PB:
 *   gather    order key (uint64) of every counting position and column of the chunk, the masses, M = sum of the masses,
 *             n_mass, and per block and column (smallest key, smallest mass at it, largest key)
 *   targets   per column: v_1, m_(1), v_n from the blocks' partials; H = m_(1) + t per probability
 *   8 x pass  most significant digit first, 8 bits a pass: histogram of MASS per digit among the keys that still match the
 *             prefix of a probability.  Prefixes of equal length are equal or disjoint, so a key matches at most one of the
 *             distinct prefixes ("slots", <= WQ_PB of them) and costs one LDS atomic; a workgroup flushes its non-empty bins
 *             to the global histogram.  `scan` then moves every probability one digit down and renumbers the slots.
 *   close     per slot: smallest mass among the keys equal to the selected one, largest counting key below it
 *   final     the interpolation, into the result array on the device
 * Nothing is read by the host until the very end: one copy of [M, n_mass | results], one synchronisation per call.  The select
 * of the generations (abz_select_impl) is not involved and no state survives the call.  Only the gather reads values: it is a
 * template over the value source of abz_summary.h, and the same driver serves a dense per-particle matrix (abz_columns_wquantiles_impl).
 */
#include <string.h>

#include <vector>

#include "abz_ctx.h"
#include "abz_device.h"
#include "abz_summary.h"

#define WQ_PB 16            /* probabilities per batch: one 256-bin histogram each, 32 KB of LDS */
/* WQ_CB (abz_summary.h): columns per chunk, 128 bytes of a row */
#define WQ_ITEMS 8          /* positions per thread and tile in the passes */
#define WQ_TILE (ABZ_BLOCK * WQ_ITEMS)
#define WQ_MAX_BLOCKS 2048  /* gather: blocks (and partials per column) */
#define WQ_PASS_BLOCKS 128  /* passes: blocks per column */
#define WQ_KEY_BYTES ((size_t)512 << 20)   /* the chunk's keys stay below this */

typedef unsigned long long u64;

struct WqState {            /* one per column of the chunk */
  u64 prefix[WQ_PB];        /* slot -> the key bits decided so far, right-aligned */
  u64 hrem[WQ_PB];          /* probability -> H minus the mass of the keys below its prefix */
  u64 mmin[WQ_PB];          /* slot -> smallest mass among the keys equal to the selected one */
  u64 vprev[WQ_PB];         /* slot -> largest counting key below the selected one */
  u64 kmin, m1, kmax;       /* v_1, m_(1), v_n as keys */
  int32_t slot_of[WQ_PB];   /* probability -> slot */
  int32_t top[WQ_PB];       /* probability -> no S_k exceeds H: q = v_n */
  int32_t nslots, pad;
};

struct WqProbs { double p[WQ_PB]; int n; };

/* ---- gather: keys[c N + i] for the counting positions (others are never read: their mass is 0), mass[i], the totals
 * tot[0] = sum of the low 32 bits of the masses, tot[1] = sum of the high 32 bits, tot[2] = n_mass (first chunk only), and
 * parts[(c nb + block) 3 + {0, 1, 2}] = (smallest key, smallest mass at it, largest key) of the block's positions; the columns
 * k_first .. k_first + ncols - 1 of the source */
template <class S>
__global__ __launch_bounds__(ABZ_BLOCK) void wq_gather_kernel(const S p, int k_first, int ncols, u64* __restrict__ keys,
                                                             u64* __restrict__ mass, int first_chunk, u64* __restrict__ parts,
                                                             u64* __restrict__ tot) {
  __shared__ u64 s_kmin[WQ_CB], s_m1[WQ_CB], s_kmax[WQ_CB];
  const int t = threadIdx.x;
  u64 kmin[WQ_CB], m1[WQ_CB], kmax[WQ_CB];
#pragma unroll
  for (int c = 0; c < WQ_CB; ++c) { kmin[c] = ~0ull; m1[c] = ~0ull; kmax[c] = 0ull; }
  if (t < WQ_CB) { s_kmin[t] = ~0ull; s_m1[t] = ~0ull; s_kmax[t] = 0ull; }
  u64 lo = 0, hi = 0, cnt = 0;
  const int b = abz_stratum_bits((uint32_t)p.N);
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < p.N; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    const u64 m = sum_mass(p, i, b);
    if (first_chunk) mass[i] = m;
    if (m < 1) continue;
    lo += m & 0xFFFFFFFFull; hi += m >> 32; cnt += 1;
    const double* row = p.row(i);
#pragma unroll
    for (int c = 0; c < WQ_CB; ++c) {
      if (c < ncols) {
        const u64 key = f64_order_key(p.value(row, k_first + c));
        keys[(size_t)c * (size_t)p.N + (size_t)i] = key;
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

/* ---- targets: one block per column.  (v_1, m_(1), v_n) from the blocks' partials, then per probability
 * t = min(floor(p (double)(M - m_(1))), M - m_(1)), H = m_(1) + t; every probability starts in slot 0 with an empty prefix */
__global__ __launch_bounds__(ABZ_BLOCK) void wq_targets_kernel(WqState* __restrict__ st, const u64* __restrict__ parts, int nb,
                                                              const u64* __restrict__ tot, const WqProbs pr) {
  __shared__ u64 s_kmin, s_m1, s_kmax;
  const int t = threadIdx.x, c = blockIdx.x;
  const u64* pc = parts + (size_t)c * nb * 3;
  if (t == 0) { s_kmin = ~0ull; s_m1 = ~0ull; s_kmax = 0ull; }
  __syncthreads();
  u64 kmin = ~0ull, m1 = ~0ull, kmax = 0ull;
  for (int j = t; j < nb; j += ABZ_BLOCK) {
    const u64 a = pc[3 * j], m = pc[3 * j + 1], z = pc[3 * j + 2];
    if (a < kmin || (a == kmin && m < m1)) { kmin = a; m1 = m; }
    if (z > kmax) kmax = z;
  }
  atomicMin(&s_kmin, kmin); atomicMax(&s_kmax, kmax);
  __syncthreads();
  if (kmin == s_kmin) atomicMin(&s_m1, m1);
  __syncthreads();
  WqState* s = st + c;
  if (t == 0) { s->kmin = s_kmin; s->m1 = s_m1; s->kmax = s_kmax; s->nslots = 1; s->pad = 0; }
  if (t < WQ_PB) {
    const u64 Mtot = tot[0] + (tot[1] << 32);
    const u64 span = Mtot - s_m1;
    u64 tt = 0;
    if (t < pr.n) {
      const double x = abz_floor(pr.p[t] * (double)span);
      tt = x >= 0x1p63 ? span : (u64)x;
      if (tt > span) tt = span;
    }
    s->prefix[t] = 0; s->hrem[t] = s_m1 + tt; s->mmin[t] = ~0ull; s->vprev[t] = 0ull; s->slot_of[t] = 0; s->top[t] = 0;
  }
}

/* ---- one radix pass: hist[(c WQ_PB + slot) 256 + digit] += mass over the keys of column c whose bits above `shift + 8` are
 * the slot's prefix; grid (blocks, columns), a block strides over tiles of WQ_TILE positions */
__global__ __launch_bounds__(ABZ_BLOCK) void wq_pass_kernel(const WqState* __restrict__ st, const u64* __restrict__ keys,
                                                           const u64* __restrict__ mass, int64_t N, int shift, u64* __restrict__ hist) {
  __shared__ u64 s_hist[WQ_PB * 256];
  __shared__ u64 s_prefix[WQ_PB];
  const int t = threadIdx.x, c = blockIdx.y;
  const WqState* s = st + c;
  const int nslots = s->nslots;
  if (t < WQ_PB) s_prefix[t] = t < nslots ? s->prefix[t] : ~0ull;
  for (int j = t; j < nslots * 256; j += ABZ_BLOCK) s_hist[j] = 0ull;
  __syncthreads();
  const u64* kc = keys + (size_t)c * (size_t)N;
  int cur = -1;                       /* a thread's run of positions in one bin costs one atomic */
  u64 acc = 0;
  for (int64_t base = (int64_t)blockIdx.x * WQ_TILE; base < N; base += (int64_t)gridDim.x * WQ_TILE) {
    u64 k[WQ_ITEMS], m[WQ_ITEMS];
#pragma unroll
    for (int j = 0; j < WQ_ITEMS; ++j) {
      const int64_t i = base + j * ABZ_BLOCK + t;
      m[j] = i < N ? mass[i] : 0ull;
      k[j] = m[j] ? kc[i] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < WQ_ITEMS; ++j) {
      if (!m[j]) continue;
      const u64 hi = shift >= 56 ? 0ull : k[j] >> (shift + 8);
      int slot = -1;
      for (int q = 0; q < nslots; ++q)
        if (s_prefix[q] == hi) slot = q;
      if (slot < 0) continue;
      const int bin = slot * 256 + (int)((k[j] >> shift) & 255ull);
      if (bin == cur) { acc += m[j]; continue; }
      if (cur >= 0) atomicAdd(&s_hist[cur], acc);
      cur = bin; acc = m[j];
    }
  }
  if (cur >= 0) atomicAdd(&s_hist[cur], acc);
  __syncthreads();
  u64* hc = hist + (size_t)c * WQ_PB * 256;
  for (int j = t; j < nslots * 256; j += ABZ_BLOCK) {
    const u64 v = s_hist[j];
    if (v) atomicAdd(&hc[j], v);
  }
}

/* ---- scan: one block per column.  Per slot the inclusive sums of its 256 bins; per probability the smallest digit whose
 * inclusive sum exceeds hrem (none in the first pass: H >= M, the quantile is v_n); the probabilities' new prefixes are
 * renumbered into slots and the histogram is cleared for the next pass */
__global__ __launch_bounds__(ABZ_BLOCK) void wq_scan_kernel(WqState* __restrict__ st, u64* __restrict__ hist, int np) {
  __shared__ u64 s_inc[WQ_PB * 256];
  __shared__ u64 s_new[WQ_PB], s_pre[WQ_PB];
  const int t = threadIdx.x, c = blockIdx.x, lane = t & 63, wave = t >> 6;
  WqState* s = st + c;
  u64* hc = hist + (size_t)c * WQ_PB * 256;
  const int nslots = s->nslots;
  for (int slot = wave; slot < nslots; slot += ABZ_BLOCK / 64) {          /* wave-uniform */
    u64 h[4], run = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { run += hc[slot * 256 + 4 * lane + j]; h[j] = run; }
    u64 inc = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    const u64 below = inc - run;
#pragma unroll
    for (int j = 0; j < 4; ++j) s_inc[slot * 256 + 4 * lane + j] = below + h[j];
  }
  __syncthreads();
  if (t < WQ_PB) {
    u64 np_prefix = ~0ull;
    if (t < np) {
      const int slot = s->slot_of[t];
      const u64* inc = s_inc + slot * 256;
      const u64 hrem = s->hrem[t];
      int lo = 0, hi = 256;                                                /* first digit with inc > hrem, 256: none */
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (inc[mid] > hrem) hi = mid; else lo = mid + 1;
      }
      if (lo >= 256) { s->top[t] = 1; lo = 255; }
      np_prefix = (s->prefix[slot] << 8) | (u64)lo;
      s->hrem[t] = hrem - (lo ? inc[lo - 1] : 0ull);
    }
    s_new[t] = np_prefix;
  }
  __syncthreads();
  if (t == 0) {
    int n = 0;
    for (int q = 0; q < np; ++q) {
      int slot = -1;
      for (int j = 0; j < n; ++j)
        if (s_pre[j] == s_new[q]) slot = j;
      if (slot < 0) { slot = n; s_pre[n++] = s_new[q]; }
      s->slot_of[q] = slot;
    }
    for (int j = 0; j < n; ++j) s->prefix[j] = s_pre[j];
    s->nslots = n;
  }
  for (int j = t; j < nslots * 256; j += ABZ_BLOCK) hc[j] = 0ull;
}

/* ---- closing pass: per slot (prefix = the selected key v_k) the smallest mass among the keys equal to it and the largest
 * counting key below it; grid (blocks, columns) */
__global__ __launch_bounds__(ABZ_BLOCK) void wq_close_kernel(WqState* __restrict__ st, const u64* __restrict__ keys,
                                                            const u64* __restrict__ mass, int64_t N) {
  __shared__ u64 s_mm[WQ_PB], s_vp[WQ_PB], s_prefix[WQ_PB];
  const int t = threadIdx.x, c = blockIdx.y;
  WqState* s = st + c;
  const int nslots = s->nslots;
  if (t < WQ_PB) { s_mm[t] = ~0ull; s_vp[t] = 0ull; s_prefix[t] = t < nslots ? s->prefix[t] : 0ull; }
  __syncthreads();
  u64 pre[WQ_PB], mm[WQ_PB], vp[WQ_PB];
#pragma unroll
  for (int q = 0; q < WQ_PB; ++q) { pre[q] = s_prefix[q]; mm[q] = ~0ull; vp[q] = 0ull; }
  const u64* kc = keys + (size_t)c * (size_t)N;
  for (int64_t i = (int64_t)blockIdx.x * ABZ_BLOCK + t; i < N; i += (int64_t)gridDim.x * ABZ_BLOCK) {
    const u64 m = mass[i];
    if (!m) continue;
    const u64 k = kc[i];
#pragma unroll
    for (int q = 0; q < WQ_PB; ++q) {
      if (q < nslots) {
        if (k == pre[q] && m < mm[q]) mm[q] = m;
        if (k < pre[q] && k > vp[q]) vp[q] = k;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < WQ_PB; ++q) {
    if (q < nslots) {
      if (mm[q] != ~0ull) atomicMin(&s_mm[q], mm[q]);
      if (vp[q]) atomicMax(&s_vp[q], vp[q]);
    }
  }
  __syncthreads();
  if (t < nslots) {
    if (s_mm[t] != ~0ull) atomicMin(&s->mmin[t], s_mm[t]);
    if (s_vp[t]) atomicMax(&s->vprev[t], s_vp[t]);
  }
}

/* ---- the interpolation: res[c n_total + q0 + q]; grid = columns */
__global__ void wq_final_kernel(const WqState* __restrict__ st, int np, double* __restrict__ res, int n_total, int q0) {
  const int t = threadIdx.x, c = blockIdx.x;
  const WqState* s = st + c;
  if (t >= np) return;
  double q;
  if (s->top[t]) {
    q = f64_from_order_key_dev(s->kmax);
  } else {
    const int slot = s->slot_of[t];
    const double vk = f64_from_order_key_dev(s->prefix[slot]);
    const u64 hb = s->hrem[t], mm = s->mmin[slot];
    if (hb >= mm) {                                   /* the crossing is not in the first element of the tie group: v_k-1 = v_k */
      q = abz_quantile_type7(vk, vk, 0.0);
    } else {
      const double g = (double)hb / (double)mm;
      q = abz_quantile_type7(f64_from_order_key_dev(s->vprev[slot]), vk, g);
    }
  }
  res[(size_t)c * n_total + q0 + t] = q;
}

/* ================================================================ host side */
/* the columns k0 .. k0 + nk - 1 of a source; `call` names the entry point in the refusals */
template <class S>
static int wquantiles_drive(abcdez_ctx* ctx, const char* call, const S& src, int k0, int nk, const double* probs, int n_probs,
                            double* q_out, uint64_t* M_out, int64_t* n_mass) {
  const int64_t N = src.N;
  size_t fit = WQ_KEY_BYTES / ((size_t)N * 8);                         /* columns whose keys fit the chunk */
  fit = fit < 1 ? 1 : fit > WQ_CB ? WQ_CB : fit;
  const int ncc = (int)fit < nk ? (int)fit : nk;
  const int64_t nb64 = (N + ABZ_BLOCK - 1) / ABZ_BLOCK;
  const int nb = (int)(nb64 < WQ_MAX_BLOCKS ? nb64 : WQ_MAX_BLOCKS);
  const int64_t nt64 = (N + WQ_TILE - 1) / WQ_TILE;
  const int npb = (int)(nt64 < WQ_PASS_BLOCKS ? nt64 : WQ_PASS_BLOCKS);
  /* [ totals 3 x u64 | results nk x n_probs | states | histograms | partials | mass | keys ] */
  const size_t n_res = (size_t)nk * (size_t)n_probs;
  const size_t o_res = 256, o_st = o_res + abz_align(n_res * 8), o_hist = o_st + abz_align((size_t)ncc * sizeof(WqState)),
               o_parts = o_hist + (size_t)ncc * WQ_PB * 256 * 8, o_mass = o_parts + abz_align((size_t)ncc * nb * 3 * 8),
               o_keys = o_mass + abz_align((size_t)N * 8);
  int rc = sum_ws_reserve(ctx, o_keys + (size_t)ncc * (size_t)N * 8);
  if (rc) return rc;
  char* base = (char*)ctx->sum_ws;
  u64* tot = (u64*)base;
  double* res = (double*)(base + o_res);
  WqState* st = (WqState*)(base + o_st);
  u64* hist = (u64*)(base + o_hist);
  u64* parts = (u64*)(base + o_parts);
  u64* mass = (u64*)(base + o_mass);
  u64* keys = (u64*)(base + o_keys);

  ABZ_HIP_CHECK(hipMemsetAsync(base, 0, o_parts, ctx->stream));        /* totals, results, states, histograms */
  for (int c0 = 0; c0 < nk; c0 += ncc) {
    const int nc = nk - c0 < ncc ? nk - c0 : ncc;
    hipLaunchKernelGGL(wq_gather_kernel<S>, dim3((unsigned)nb), dim3(ABZ_BLOCK), 0, ctx->stream, src, k0 + c0, nc, keys, mass,
                       c0 == 0 ? 1 : 0, parts, tot);
    for (int q0 = 0; q0 < n_probs; q0 += WQ_PB) {
      WqProbs pr{};
      pr.n = n_probs - q0 < WQ_PB ? n_probs - q0 : WQ_PB;
      for (int q = 0; q < pr.n; ++q) pr.p[q] = probs[q0 + q];
      hipLaunchKernelGGL(wq_targets_kernel, dim3((unsigned)nc), dim3(ABZ_BLOCK), 0, ctx->stream, st, (const u64*)parts, nb,
                         (const u64*)tot, pr);
      for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(wq_pass_kernel, dim3((unsigned)npb, (unsigned)nc), dim3(ABZ_BLOCK), 0, ctx->stream, (const WqState*)st,
                           (const u64*)keys, (const u64*)mass, N, shift, hist);
        hipLaunchKernelGGL(wq_scan_kernel, dim3((unsigned)nc), dim3(ABZ_BLOCK), 0, ctx->stream, st, hist, pr.n);
      }
      hipLaunchKernelGGL(wq_close_kernel, dim3((unsigned)npb, (unsigned)nc), dim3(ABZ_BLOCK), 0, ctx->stream, st, (const u64*)keys,
                         (const u64*)mass, N);
      hipLaunchKernelGGL(wq_final_kernel, dim3((unsigned)nc), dim3(64), 0, ctx->stream, (const WqState*)st, pr.n,
                         res + (size_t)c0 * n_probs, n_probs, q0);
    }
  }
  ABZ_HIP_CHECK(hipGetLastError());
  std::vector<u64> h(o_res / 8 + n_res);                                 /* totals and results are contiguous: one copy */
  ABZ_HIP_CHECK(hipMemcpyAsync(h.data(), base, o_res + n_res * 8, hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (sum_mass_verdict(call, h[0], h[1], h[2], M_out, n_mass)) return -1;
  memcpy(q_out, h.data() + o_res / 8, n_res * 8);
  return 0;
}

int abz_posterior_wquantiles_impl(abcdez_ctx* ctx, const SumPop& p, int k0, int nk, const double* probs, int n_probs, double* q_out,
                                  uint64_t* M_out, int64_t* n_mass) {
  return wquantiles_drive(ctx, "posterior_wquantiles", pop_source(ctx, p), k0, nk, probs, n_probs, q_out, M_out, n_mass);
}
int abz_columns_wquantiles_impl(abcdez_ctx* ctx, const ColView& v, int k0, int nk, const double* probs, int n_probs, double* q_out,
                                uint64_t* M_out, int64_t* n_mass) {
  return wquantiles_drive(ctx, "columns_wquantiles", v, k0, nk, probs, n_probs, q_out, M_out, n_mass);
}
