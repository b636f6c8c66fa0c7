/*
 * abz_sample.hip -- n equally weighted draws from the population where it lives (include/abcdez_spec.h, "posterior summaries",
 * POSTERIOR SAMPLE): n strata over the total integer mass M of the resampler's fixed point, one Philox point per stratum, the
 * position under the point, and the gather of that position's current row (push_p-cast), distance and blob stamp.  Integers only:
 * the indices are bit for bit those of the literal restatement in abcdez_amd/summary.py (sample_reference).
 *
 *   count    (weights only) sum of the masses as two 32-bit halves -- so that a total of 2^63 or more is seen, never wrapped -- and
 *            n_mass
 *   scan     (weights only) the resampler's three scan kernels (abz_population.hip, abz_wfix_scan_enqueue) on this call's buffers:
 *            exclusive tile offsets and the inclusive sums C
 *   setup    one thread: M, q = M div n, r = M mod n and the refusal flag, on the device -- no host round trip before the search
 *   search   one thread per stratum: the point, then the tile whose offsets bracket it (binary search over the offsets: 16 KB at
 *            2^22 positions), then the position among that tile's 2048 inclusive sums (16 KB).  Neighbouring strata land in
 *            neighbouring tiles, so a wavefront's 22 steps stay in a few cache lines; without weights idx = R >> b, no scan
 *   gather   a lane group per sampled row, 16 bytes per lane and load, the slot bit of the SOURCE position selects the row; P (dense
 *            n x d, push_p per dimension), the internal rows, distances and stamps leave in the same pass
 * Every scratch word lives in the summaries' buffer (sum_ws_reserve): neither ctx->ws nor the device scalars are touched, so a select
 * armed ahead survives the call.  The host reads [M, n_mass, flag] after ONE synchronisation and reports the refusals then; on a
 * refusal the search and the gather write nothing.
 */
#include <string>

#include "abz_ctx.h"
#include "abz_device.h"
#include "abz_dispatch.h"
#include "abz_summary.h"

#define SMP_COUNT_BLOCKS 1024
#define SMP_LANES_MAX 16     /* lanes per sampled row at most: 256 contiguous bytes per load of a group */

typedef unsigned long long u64;

/* header words (u64) at the front of the buffer; [0, SMP_H_N) is zeroed per call and read back */
enum { SMP_H_LO = 0, SMP_H_HI = 1, SMP_H_NMASS = 2, SMP_H_M = 3, SMP_H_Q = 4, SMP_H_R = 5, SMP_H_FLAG = 6, SMP_H_N = 8 };
enum { SMP_OK = 0, SMP_TOO_HEAVY = 1, SMP_NO_MASS = 2, SMP_TOO_MANY = 3 };

/* ---- count: hdr[LO] += low halves, hdr[HI] += high halves of the masses, hdr[NMASS] += #(m >= 1) */
__global__ __launch_bounds__(ABZ_BLOCK) void sample_count_kernel(const double* __restrict__ wns, uint32_t N, u64* __restrict__ hdr) {
  u64 lo = 0, hi = 0, cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * ABZ_BLOCK + threadIdx.x; i < N; i += (uint64_t)gridDim.x * ABZ_BLOCK) {
    const u64 m = abz_weight_fix(wns[i], N);
    lo += m & 0xFFFFFFFFull; hi += m >> 32; cnt += m ? 1u : 0u;
  }
  sum_mass_tally(lo, hi, cnt, hdr);
}

/* ---- setup: M, q, r and the flag.  unit_b >= 0: no weight array, every position has the mass 2^unit_b */
__global__ void sample_setup_kernel(u64* __restrict__ hdr, uint32_t N, u64 n, int unit_b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  u64 lo = hdr[SMP_H_LO], hi = hdr[SMP_H_HI], n_mass = hdr[SMP_H_NMASS];
  if (unit_b >= 0) { lo = 0; hi = (u64)N << (unit_b - 32); n_mass = N; }     /* b >= 32 for every N < 2^31: N 2^b as its high half */
  u64 flag = SMP_OK, M = 0, q = 0, r = 0;
  if (n_mass < 1) flag = SMP_NO_MASS;
  else if (!sum_mass_total(lo, hi, &M)) flag = SMP_TOO_HEAVY;
  else if (n > M) flag = SMP_TOO_MANY;
  else { q = M / n; r = M % n; }
  hdr[SMP_H_NMASS] = n_mass; hdr[SMP_H_M] = M; hdr[SMP_H_Q] = q; hdr[SMP_H_R] = r; hdr[SMP_H_FLAG] = flag;
}

/* ---- search: idx[s] = the smallest position i with C_i > R_s.  cum == NULL: unit masses 2^unit_b */
__global__ __launch_bounds__(ABZ_BLOCK) void sample_search_kernel(const u64* __restrict__ hdr, const u64* __restrict__ tile_off,
                                                                 const u64* __restrict__ cum, uint32_t N, uint32_t nt, uint32_t n,
                                                                 uint64_t seed, uint32_t draw, int unit_b, uint32_t* __restrict__ idx) {
  if (hdr[SMP_H_FLAG] != SMP_OK) return;
  const uint64_t g = (uint64_t)blockIdx.x * ABZ_BLOCK + threadIdx.x;
  if (g >= n) return;
  const uint32_t s = (uint32_t)g;
  const u64 R = abz_sample_point(seed, s, draw, hdr[SMP_H_Q], hdr[SMP_H_R]);
  uint32_t i;
  if (!cum) {
    i = (uint32_t)(R >> unit_b);
  } else {
    uint32_t lo = 0, hi = nt;              /* the number of tiles whose offset is <= R; at least 1: tile_off[0] = 0 */
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (tile_off[mid] <= R) lo = mid + 1; else hi = mid;
    }
    const uint32_t tl = lo ? lo - 1 : 0u;  /* the tile: its offset <= R < the next tile's offset (or M) */
    lo = tl * ABZ_SCAN_TILE;
    hi = lo + ABZ_SCAN_TILE < N ? lo + ABZ_SCAN_TILE : N;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (cum[mid] > R) hi = mid; else lo = mid + 1;
    }
    i = lo;
  }
  idx[s] = i < N ? i : N - 1u;             /* (R < M makes i < N; the bound is for the memory the gather reads) */
}

/* ---- gather: G lanes per sampled row s, lane j moves the 16-byte pieces j, j + G, .. of the current row of idx[s] */
__global__ __launch_bounds__(ABZ_BLOCK) void sample_gather_kernel(const abz_model* __restrict__ M, const u64* __restrict__ hdr,
                                                                 const SumPop p, const uint32_t* __restrict__ idx, uint32_t n, int G,
                                                                 const double* __restrict__ delta, const uint64_t* __restrict__ stamp,
                                                                 double* __restrict__ P_out, double* __restrict__ theta_out,
                                                                 double* __restrict__ delta_out, uint64_t* __restrict__ stamp_out) {
  if (hdr[SMP_H_FLAG] != SMP_OK) return;
  const uint64_t g = (uint64_t)blockIdx.x * ABZ_BLOCK + threadIdx.x;
  const uint64_t s = g / (uint64_t)G;
  const int j = (int)(g % (uint64_t)G);
  if (s >= n) return;
  const uint32_t src = idx[s];
  if (src >= (uint64_t)p.N) return;
  const double* __restrict__ row = sum_row(p, src);
  double* __restrict__ po = P_out + (size_t)s * (size_t)p.d;
  double* __restrict__ to = theta_out ? theta_out + (size_t)s * (size_t)p.ld : nullptr;
  if (p.ld == 1) {
    const double v = row[0];
    po[0] = abz_push_p(&M->prior[0], v);
    if (to) to[0] = v;
  } else {
    for (int c = j; 2 * c < p.ld; c += G) {            /* ld is a power of two >= 2: rows are 16-byte aligned */
      const double2 v = *reinterpret_cast<const double2*>(row + 2 * c);
      if (to) *reinterpret_cast<double2*>(to + 2 * c) = v;
      if (2 * c < p.d) po[2 * c] = abz_push_p(&M->prior[2 * c], v.x);
      if (2 * c + 1 < p.d) po[2 * c + 1] = abz_push_p(&M->prior[2 * c + 1], v.y);
    }
  }
  if (j == 0) {
    if (delta_out) delta_out[s] = delta[src];
    if (stamp_out) stamp_out[s] = stamp[src];
  }
}

/* ================================================================ host side */
int abz_posterior_sample_impl(abcdez_ctx* ctx, const SumPop& p, int64_t n, uint32_t draw, const double* delta, const uint64_t* stamp,
                              uint32_t* idx_out, double* P_out, double* theta_out, double* delta_out, uint64_t* stamp_out,
                              uint64_t* M_out, int64_t* n_mass) {
  const double* wns = p.wns;
  const uint32_t Nu = (uint32_t)p.N, nu = (uint32_t)n;
  const int b = abz_stratum_bits(Nu);
  if (!wns) {                              /* everything is known here: refuse before anything is enqueued */
    u64 M = 0;
    if (!sum_mass_total(0, (u64)Nu << (b - 32), &M)) {               /* N 2^b as its high half, as in sample_setup_kernel */
      abz_set_error("posterior_sample: the total mass reaches 2^63 (N 2^b with N = " + std::to_string((long long)p.N) + ")");
      return -1;
    }
    if ((u64)n > M) { abz_set_error("posterior_sample: n exceeds the total mass M"); return -1; }
  }
  const uint32_t nt = (Nu + ABZ_SCAN_TILE - 1) / ABZ_SCAN_TILE;
  /* [ header | last_pos || tile offsets | tile_lp | C ]: only the header is zeroed and read back */
  const size_t o_tile = 256, o_lp = o_tile + abz_align((size_t)nt * 8), o_cum = o_lp + abz_align((size_t)nt * 4),
               o_end = o_cum + abz_align((size_t)Nu * 8);
  int rc = sum_ws_reserve(ctx, wns ? o_end : o_tile);
  if (rc) return rc;
  char* base = (char*)ctx->sum_ws;
  u64* hdr = (u64*)base;
  u64* last_pos = hdr + SMP_H_N;
  u64* tile = (u64*)(base + o_tile);
  uint32_t* tile_lp = (uint32_t*)(base + o_lp);
  u64* cum = wns ? (u64*)(base + o_cum) : nullptr;

  ABZ_HIP_CHECK(hipMemsetAsync(base, 0, o_tile, ctx->stream));
  if (wns) {
    const uint32_t nb64 = (Nu + ABZ_BLOCK - 1) / ABZ_BLOCK;
    hipLaunchKernelGGL(sample_count_kernel, dim3(nb64 < SMP_COUNT_BLOCKS ? nb64 : SMP_COUNT_BLOCKS), dim3(ABZ_BLOCK), 0, ctx->stream,
                       wns, Nu, hdr);
    abz_wfix_scan_enqueue(ctx, wns, Nu, tile, tile_lp, last_pos, cum);
  }
  hipLaunchKernelGGL(sample_setup_kernel, dim3(1), dim3(64), 0, ctx->stream, hdr, Nu, (u64)n, wns ? -1 : b);
  hipLaunchKernelGGL(sample_search_kernel, dim3(abz_grid((uint64_t)nu)), dim3(ABZ_BLOCK), 0, ctx->stream, (const u64*)hdr,
                     (const u64*)tile, (const u64*)cum, Nu, nt, nu, ctx->h_model.seed, draw, wns ? -1 : b, idx_out);
  int G = p.ld / 2;
  G = G < 1 ? 1 : G > SMP_LANES_MAX ? SMP_LANES_MAX : G;
  hipLaunchKernelGGL(sample_gather_kernel, dim3(abz_grid((uint64_t)nu * (uint64_t)G)), dim3(ABZ_BLOCK), 0, ctx->stream,
                     (const abz_model*)ctx->d_model, (const u64*)hdr, p, (const uint32_t*)idx_out, nu, G, delta, stamp, P_out, theta_out,
                     delta_out, stamp_out);
  ABZ_HIP_CHECK(hipGetLastError());
  u64 h[SMP_H_N];
  ABZ_HIP_CHECK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  ABZ_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  switch (h[SMP_H_FLAG]) {
    case SMP_OK: break;
    case SMP_NO_MASS: return sum_mass_refuse("posterior_sample", false);
    case SMP_TOO_HEAVY: return sum_mass_refuse("posterior_sample", true);
    default: abz_set_error("posterior_sample: n exceeds the total mass M"); return -1;
  }
  *M_out = h[SMP_H_M];
  *n_mass = (int64_t)h[SMP_H_NMASS];
  return 0;
}
