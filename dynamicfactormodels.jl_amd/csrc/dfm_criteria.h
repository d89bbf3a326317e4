// dfm_criteria.h — the seven criteria of src/criteria.jl:17-53, their sweep
// over k = 1..kmax, the first arg-min of a row and PCp's sigma^2, stated once
// for host code, device code and a plain C++ compiler (tests/c_harness).
// Codes 0..6 = PCp1, PCp2, PCp3, ICp1, ICp2, ICp3, BIC.
#pragma once
#include <math.h>
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DFM_HD __host__ __device__ inline
#else
#define DFM_HD inline
#endif

namespace dfm {

DFM_HD int ceil_half(int m) { return (m + 1) / 2; }   // max_factor_number, src/DynamicFactorModel.jl:101

// Criterion `code` at k factors: V = V(k), sigma2 = PCp's V(ceil(m/2)) of the
// unrestricted fit, c = (N + T) / (N T), m = min(T, N).
DFM_HD double criterion(int code, double V, int k, double sigma2, int64_t T, int64_t N) {
  const double c = (double)(N + T) / ((double)N * (double)T), m = (double)(T < N ? T : N);
  switch (code) {
    case 0: return V + k * sigma2 * c * log(1.0 / c);
    case 1: return V + k * sigma2 * c * log(m);
    case 2: return V + k * sigma2 * log(m) / m;
    case 3: return log(V) + k * c * log(1.0 / c);
    case 4: return log(V) + k * c * log(m);
    case 5: return log(V) + k * log(m) / m;
    case 6: return V + k * log((double)T) / T;
  }
  return NAN;
}

// The first-minimum rule, indmin (src/DynamicFactorModel.jl:65): a later value
// replaces the least so far only when strictly smaller, so ties keep the
// earlier k and NaN never wins (a row of NaN keeps k = 1).
DFM_HD bool below(double v, double least) { return v < least; }

// 1-based k of the first minimum of row[0..n-1]
DFM_HD int first_argmin(const double *row, int n) {
  int best = 0;
  double least = row[0];
  for (int k = 1; k < n; ++k)
    if (below(row[k], least)) { least = row[k]; best = k; }
  return best + 1;
}

// out[code * kmax + k - 1] for k = 1..kmax from the descending eigenvalues and
// the trace: V(k) = (trace - sum_{i <= k} ev[i]) / (N T), subtracted in order.
// argmin (7 ints, or nullptr): first_argmin of every row, kept while the table
// is written (a kernel selects out of registers, not out of the table).
DFM_HD void criteria_sweep(const double *ev, int kmax, double trace, double sigma2, int64_t T, int64_t N,
                           double *out, int *argmin = nullptr) {
  const double NT = (double)N * (double)T;
  double cum = trace, least[7] = {};
  for (int k = 1; k <= kmax; ++k) {
    cum -= ev[k - 1];
    const double V = cum / NT;
#ifdef __clang__
#pragma unroll
#endif
    for (int code = 0; code < 7; ++code) {
      const double v = criterion(code, V, k, sigma2, T, N);
      out[code * kmax + k - 1] = v;
      if (argmin && (k == 1 || below(v, least[code]))) { least[code] = v; argmin[code] = k; }
    }
  }
}

// PCp's sigma^2 = sum_{j >= ceil(m/2)} ev[j] / (N T) of a descending spectrum, in
// two summation orders whose bits differ; a call site keeps the one it has.
// (a) a total minus the top ceil(m/2) values, subtracted in ascending index order
DFM_HD double sigma2_minus_top(double total, const double *ev, int m, double NT) {
  for (int j = 0; j < ceil_half(m); ++j) total -= ev[j];
  return total / NT;
}
// ... the total being the spectrum summed in ascending index order
DFM_HD double sigma2_total_minus_top(const double *ev, int m, double NT) {
  double s = 0.0;
  for (int j = 0; j < m; ++j) s += ev[j];
  return sigma2_minus_top(s, ev, m, NT);
}
// (b) the tail summed from index m - 1 down to h (h = 0: the trace, small end first)
DFM_HD double tail_sum(const double *ev, int m, int h) {
  double s = 0.0;
  for (int j = m - 1; j >= h; --j) s += ev[j];
  return s;
}
DFM_HD double sigma2_tail(const double *ev, int m, double NT) { return tail_sum(ev, m, ceil_half(m)) / NT; }

}  // namespace dfm
