// dfm_ss_lane.h — what the one-lane-per-column kernels of the state-space pass
// share (ss_sim_kernel of dfm_ss_sim.hip, ss_news_kernel of dfm_ss_news.hip):
// a lane's vector lives in an LDS column, element k at [k * 64 + lane].
#pragma once
#include "dfm_common.h"

namespace dfm {

// v + sum_{k<n} a[k] x[64 k] (NEG: v - sum), the products added in the order of k: a from the
// staged record or the constants (a broadcast read), x a lane's column.  Eight
// pairs are read before their multiply-adds run, so a round costs one LDS
// latency, not eight: the chain of a lane is serial and nothing else hides it.
template <bool NEG>
DFM_DEV double sim_dot(double v, const double *a, const double *x, int n) {
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double av[8], xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      av[q] = a[k + q];
      xv[q] = x[(k + q) * 64];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) v = fma(NEG ? -av[q] : av[q], xv[q], v);
  }
  for (; k < n; ++k) v = fma(NEG ? -a[k] : a[k], x[k * 64], v);
  return v;
}

}  // namespace dfm
