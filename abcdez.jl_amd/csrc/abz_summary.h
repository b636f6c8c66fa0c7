/* abz_summary.h -- what the posterior-summary translation units share (abz_summary.hip, abz_wquantile.hip): the view of a
 * population and the calls' buffer in the context. */
#pragma once
#include "abz_ctx.h"

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

/* ctx->sum_ws holds at least `bytes` afterwards (abz_summary.hip); the contents do not survive a growth */
int sum_ws_reserve(abcdez_ctx* ctx, size_t bytes);
