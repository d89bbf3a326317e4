// dfm_fact_plan.h — the one statement of the factored solver's first filter: its degree, whether a Rayleigh-Ritz step
// stands in front of it, and for every H.Z product of it the kernel that runs it and the formats in which Z and HZ
// pass between the products and the Horner steps.  Plain C++, no HIP: eig_run_fact2_t builds one FilterPlan per solve
// and walks it, and tests/c_harness/fact_plan_host.cpp checks the rule with a host compiler alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace dfm {

// Filter schedule.  From a warm start (the base fit's eigenvectors): a degree-6 filter on [0, max(theta_p, 0.2
// theta_k)] after the first Rayleigh-Ritz step, degree 2 on [0, theta_p] after the later ones.  C3 (tools/
// eig_proto.py, the CPU model of this loop; tools/c3_excess.py, the convergence excess measured on the GPU): with
// degree 2 throughout the first filter gains only ~3e3 in the eigenvalue bound (theta_16 ~ 0.8e3 far below lambda_17
// ~ 8e3) against ~5e4 for the later ones, and replicates retire at the 4th (96 %) or 5th Rayleigh-Ritz step after
// 7.09 products; with this schedule every replicate of the CPU model retires at the 2nd step after 7 products — two
// Rayleigh-Ritz passes and the straggler tail fewer, two more Chebyshev passes.  Cold starts (no warm vectors:
// expanding windows) keep degree 2 on [0, theta_p].
constexpr int kChebWarmD0 = 6, kChebD = 2;
constexpr int kFilterDMax = 8;   // = kChebDMax (dfm_eig.h; asserted in dfm_fact.hip)
constexpr double kChebWarmBeta = 0.2;
// A warm start whose first filter has middle steps (degree >= 3) skips the first Rayleigh-Ritz step: the filter is a
// polynomial in G*, so span(p(G*) Q0 Bm) = span(p(G*) Q0) for any invertible Bm and the next Rayleigh-Ritz step, which
// reads only the span, loses nothing; the interval end is kWarmFixBeta lambda_k of the BASE fit, one number for the
// whole job (model-only: the same in every batch, lane and shard).  The guards' branch of filter_end (theta_p) is not
// taken over: it needs a product, an end short of lambda_{p+1} only slows the filter, and in the CPU model it never
// binds (theta_p / theta_k of a step on the start block <= 0.022 at C3, <= 0.095 at T = 120, N = 300, against the 0.2
// it must exceed).  Gone per solve: step 0's y2, eig_small, pv and ap2; one more middle Horner step instead.  The
// guard columns are orthonormalised once against the warm vectors (q0_guards_kernel): with raw random guards the
// filtered block's condition number is ~4e7 (CPU model) and the Cholesky of its Gram matrix fails.  The first
// Rayleigh-Ritz step diagonalises a projected matrix that no earlier step has pre-rotated; its kJacobiSweeps = 2
// sweeps still suffice (CPU model: the same retirement as with 4; measured, a cap of 4 there: 47 replicate-steps in
// 205 k fewer, eig_small +0.05 ms per C3 step, profiles/r07_c3_ab.txt).  That step runs as loop step 1 (itc = 2 in
// ap2): decide_converged's previous-residual record needs no initialisation for it — the stagnation test that reads
// the record is guarded by itc > 2, and loop step 2 reads the slot ((itc - 1) & 1) that loop step 1 wrote.
constexpr double kWarmFixBeta = 0.21;
constexpr int Q0G_PMAX = 32;   // the widest block q0_guards_kernel takes (eig_run_factored: p <= 32)

// The A/B switches of the factored solver (environment; production sets none).  D0 and BETA are read once per
// process, the others at every solve, so one process can run both sides of each.
//
//   switch               default  set to  restores / selects                                        measured
//   DFM_FACT_D0          6        2..8    the first filter's degree cap (1)
//   DFM_FACT_BETA        0.2      x       its interval factor behind a first Rayleigh-Ritz step
//   DFM_FACT_STEP0       off      1       the Rayleigh-Ritz step in front of the first filter       profiles/r07_c3_ab.txt
//   DFM_FACT_F32         on       0       fp64 middle products (2)                                  profiles/r08_c3_ab.txt
//   DFM_FACT_SPLIT       on       0       the fp32 launches, bit for bit (3)                        profiles/r15_c3_ab.txt
//   DFM_FACT_SPLIT_LAST  on       0       the fp64 last product, bit for bit (4)                    profiles/r19_c3_ab.txt
//   DFM_FACT_SPLIT3      on       0       six terms in every split product, bit for bit (7)         profiles/r21_c3_ab.txt
//   DFM_AP2_PROBE        on       0       ap2's one-pass form throughout (5)                        profiles/r10_c3_ab.txt
//   DFM_FACT_PF          stored   0       the NOPF middle steps (6)                                 profiles/r10_c3_ab.txt
//
// Precedence (plan_first_filter): SPLIT_LAST and SPLIT3 act only where SPLIT is on, SPLIT only where F32 is on and the model
// holds the split H, F32 and PF only on a solve that starts with the filter (STEP0 off, a warm start, degree >= 3,
// maxit >= 2), F32 only under the eigenvalue rule (tol < 0) with H32, a finite hmax > 0 and T >= 16.
// (1) The filter amplifies wanted eigenvalue lambda_1 over lambda_k by about T_d(x_1) / T_d(x_k) ~ (x_1 / x_k)^d,
//     x = 2 lambda / b - 1 (x_k = 9 at b = 0.2 lambda_k): the filtered block's condition number.  Its degree is capped
//     so that stays below ~1e6 (CholQR2 keeps every wanted direction in fp64): C3's lambda_1 / lambda_8 = 1.6 allows 6
//     (the cap); a panel with one dominant factor (C2's base fit: lambda_1 / lambda_4 = 50) gets 3.
// (2) Under the eigenvalue rule the middle products of a filter-only step — 1 .. d0 - 1 of its d0 — run in fp32
//     (gemmh_zrm_f32_kernel).  The filter only has to deliver a good subspace: the Rayleigh-Ritz step behind it and
//     the Kato-Temple stopping rule stay fp64 and measure the true residual, the eigenvalue error is quadratic in the
//     subspace error, and the rounding noise (relative to the idiosyncratic part H Z alone: PF bB, EL a and F'F stay
//     fp64) is damped by the product that follows.  The CPU model (tools/eig_proto.py, F32 / NOISE) retires the same
//     replicates at the same steps with 64 times the fp32 noise in those products; in the last product it degrades at
//     16 times the noise.  The strict and subspace rules keep fp64 throughout: they bound the eigenvector residual,
//     which is linear in the subspace error (the model needs more products there).
// (3) Where the model holds the split H they run as six bf16 MFMA terms (gemmh_zrm_split_kernel, dfm_gemm.hip): as
//     accurate as the fp32 kernel, on the 16 times faster bf16 matrix path.
// (4) With them product d0 runs on the same kernel, through its fp64-row epilogue, on planes from the last middle
//     step.  The argument is that of (2); the model moves no replicate up to four times fp32's
//     noise and one in 400 at eight, and the split kernel's error is 0.82 of fp32's.
// (5) ap2 decides before it writes (boot_ap2_kernel's probe) on the Rayleigh-Ritz steps it >= first_poll: every step
//     of a warm solve (C3: 97 % retire at the first one and, under eigenvalue-only statistics, leave without V0, Qn
//     and their MFMAs).  The earlier steps of a cold solve keep the one-pass form: everybody goes on there and the
//     second read of Q and Y would be pure cost.  The bits do not depend on it.
// (6) Middle steps read stored PF (boot_prep_kernel writes it).  The NOPF instances (boot_cheb_mid_kernel) take it
//     from PV's rows instead, for a step that filters V0 = Q0 with kw >= r and F = fscale * warm[:, :r].  Measured at
//     C3 they move 0.30 GB less per launch and take 0.19 ms off a 9.34 ms step (prep -0.10, the five middle steps
//     -0.09: the pass is bound by its load latency, not its bytes) — 2.3 times the parent's run-to-run spread, short
//     of the 3 times this project asks of a change, so the stored form stays the default.  The middle steps behind a
//     first Rayleigh-Ritz step (PV = P'D (Q Bm), boot_pv_kernel) have no such identity and always read stored PF.
// (7) The error of product sp is damped by every Horner step behind it, so the accuracy of (3) is needed only near the
//     end of the filter: the split products sp <= d0 - 2 run as three terms, (m,h) (h,m) (h,h), on planes h and m
//     alone (>= 16 significand bits; gemmh_zrm_split_kernel's TERMS), and the pass in front of each writes only those
//     two planes.  The CPU model (tools/eig_proto.py, TERMS=) moves no replicate in 1 200 with them, nor with operands
//     of 14 bits there; three terms in product d0 - 1 hold only down to 16 bits and in product d0 not at all, so
//     those two keep six.
struct FactSwitches {
  int d0_cap = kChebWarmD0;
  double beta = kChebWarmBeta;
  bool keep_step0 = false, f32_off = false, split_off = false, split_last_off = false, ap2_probe_off = false;
  bool pf_stored = true, split3_off = false;
};
inline FactSwitches read_fact_switches() {
  auto env = [](const char *name, const char *unset) { const char *e = getenv(name); return e ? e : unset; };
  static const int d0_cap = std::max(kChebD, std::min(kFilterDMax, atoi(env("DFM_FACT_D0", "6"))));
  static const double beta = atof(env("DFM_FACT_BETA", "0.2"));
  auto is_zero = [&](const char *name) { return atoi(env(name, "1")) == 0; };
  FactSwitches s;
  s.d0_cap = d0_cap;
  s.beta = beta;
  s.keep_step0 = atoi(env("DFM_FACT_STEP0", "0")) != 0;
  s.f32_off = is_zero("DFM_FACT_F32");
  s.split_off = is_zero("DFM_FACT_SPLIT");
  s.split_last_off = is_zero("DFM_FACT_SPLIT_LAST");
  s.split3_off = is_zero("DFM_FACT_SPLIT3");
  s.ap2_probe_off = is_zero("DFM_AP2_PROBE");
  s.pf_stored = !(*env("DFM_FACT_PF", "") && is_zero("DFM_FACT_PF"));   // (an empty value leaves it stored)
  return s;
}

// What a pass leaves Z in for the next product: fp64 chunks, float chunks (Z32, in the first half of Z's region) or
// the three bf16 planes of gemmh_zrm_split_kernel's Zs (dfm_internal.h) — all in the replicate-major 16-row chunk
// layout (zrm_ix) at the fp64 replicate stride
enum class ZFmt { F64, F32, Split };
// What a product leaves HZ in for the Horner step behind it: fp64 rows, column-interleaved (gathered by idx), or
// float chunks in Z's layout, not yet scaled by hmax (HZ32)
enum class HzFmt { Rows64, Chunk32 };
// The kernel of one product: gemmh_zrm_kernel, gemmh_zrm_f32_kernel, gemmh_zrm_split_kernel<false> and <true>
enum class HzProduct { F64, F32, Split, SplitRows };
constexpr ZFmt operand_of(HzProduct k) {
  return k == HzProduct::F64 ? ZFmt::F64 : k == HzProduct::F32 ? ZFmt::F32 : ZFmt::Split;
}
constexpr HzFmt result_of(HzProduct k) {
  return k == HzProduct::F64 || k == HzProduct::SplitRows ? HzFmt::Rows64 : HzFmt::Chunk32;
}

struct FilterPlanIn {   // what the solver knows before its first launch
  bool warm = false, has_H32 = false, has_Hs = false;
  int kw = 0, k = 0, p = 0, P = 16, r = 0, T = 0, maxit = 0;
  double tol = 0.0, spread = 0.0, lamk = 0.0, fscale = 0.0, hmax = 0.0;
};

// Step 0 of the solve: products 1 .. d0, the middle Horner step sp (1 <= sp < d0) behind product sp, the last Horner
// step behind product d0.  Without skip0 a Rayleigh-Ritz step consumes product 1 and everything is fp64.
struct FilterPlan {
  int d0 = kChebD;
  bool warm_started = false;   // the warm schedule: degree d0, polls from the first Rayleigh-Ritz step
  bool mid = false;            // d0 >= 3: the first filter has middle Horner steps (boot_cheb_mid_kernel)
  bool skip0 = false;          // ... and, from a warm start, no Rayleigh-Ritz step in front of it
  bool nopf = false;           // ... whose middle steps take PF from PV's rows (6)
  bool stg_ok = false;         // y2 and the Horner steps stage F / EL[idx] rows through LDS (P = 16, even r <= 8)
  ZFmt z0 = ZFmt::F64;                       // what boot_prep_kernel leaves Z0 in
  HzProduct product[kFilterDMax + 1] = {};   // [1 .. d0]
  HzFmt mid_in[kFilterDMax + 1] = {};        // [1 .. d0 - 1]: what middle step sp reads ...
  ZFmt mid_out[kFilterDMax + 1] = {};        // ... and the Z it writes
  // The split products' refinement (7): the plane pairs product sp adds up (6, or 3 on planes h and m alone; 0 for a
  // product that is not split) and the planes of the Split Z that prep (z0_planes) and middle step sp (mid_planes[sp])
  // write for the product behind them (3 or 2; 0 where that Z is not split)
  int terms[kFilterDMax + 1] = {};           // [1 .. d0]
  int z0_planes = 0;
  int mid_planes[kFilterDMax + 1] = {};      // [1 .. d0 - 1]
  int pad_rows = 0;              // round_up(T, 16) - T: the rows of Z's last chunk past T
  bool zero_zpad = false;        // ... which no pass of step 0 writes in the fp64 Z: zeroed behind product d0
  int products_f32 = 0;          // per replicate: products not run in fp64 (gemm_products_f32 / nb) ...
  int products_split_last = 0;   // ... and last products run split (gemm_products_split_last / nb)
  int products_split3 = 0;       // ... and those of products_f32 run as three terms (gemm_products_split3 / nb)

  // does prep or a middle step write fp64 Z chunks (whole ones, their pad rows zero)?
  bool writes_z64() const {
    bool w = z0 == ZFmt::F64;
    for (int sp = 1; sp < d0; ++sp) w = w || mid_out[sp] == ZFmt::F64;
    return w;
  }
  // The chain: every product reads the format the pass before it wrote, every Horner step reads what its product
  // wrote, the last one fp64 rows; a middle step fed fp64 rows writes fp64 (the instances that exist); and somebody
  // writes the fp64 Z's pad rows, which the later fp64 products read.  A split product of three terms is fed exactly
  // two planes and one of six terms three; nothing else has terms or planes.
  static constexpr int planes_of(HzProduct k, int terms) {
    return operand_of(k) != ZFmt::Split ? (terms == 0 ? 0 : -1) : terms == 6 ? 3 : terms == 3 ? 2 : -1;
  }
  bool consistent() const {
    if (d0 < kChebD || d0 > kFilterDMax || mid != (d0 >= 3)) return false;
    ZFmt z = z0;
    int planes = z0_planes;
    for (int sp = 1; sp < d0; ++sp) {
      const HzFmt hz = result_of(product[sp]);
      if (operand_of(product[sp]) != z || mid_in[sp] != hz || planes_of(product[sp], terms[sp]) != planes) return false;
      if (hz == HzFmt::Rows64 && mid_out[sp] != ZFmt::F64) return false;
      z = mid_out[sp];
      planes = mid_planes[sp];
    }
    return operand_of(product[d0]) == z && result_of(product[d0]) == HzFmt::Rows64 &&
           planes_of(product[d0], terms[d0]) == planes && (pad_rows == 0 || zero_zpad || writes_z64());
  }
};

inline int first_filter_degree(double spread, int cap) {
  const double ratio = std::max(1.0001, 1.1 * spread);
  const int d = (int)std::floor(std::log(1e6) / std::log(ratio));
  return std::max(kChebD, std::min(cap, d));
}

inline FilterPlan plan_first_filter(const FilterPlanIn &in, const FactSwitches &sw) {
  FilterPlan pl;
  pl.warm_started = in.warm && in.kw >= in.k && in.spread >= 1.0;
  pl.d0 = pl.warm_started ? first_filter_degree(in.spread, sw.d0_cap) : kChebD;
  pl.mid = pl.d0 >= 3;
  pl.skip0 = pl.warm_started && pl.mid && in.maxit >= 2 && kWarmFixBeta * in.lamk > 0.0 && in.p <= Q0G_PMAX &&
             !sw.keep_step0;
  pl.stg_ok = in.P == 16 && in.r <= 8 && (in.r & 1) == 0 && ((in.p + 1) & ~1) <= 16;
  pl.nopf = pl.skip0 && in.fscale > 0.0 && in.kw >= in.r && !sw.pf_stored;
  // the kernel of the middle products and of the last one (2 - 4) ...
  HzProduct middle = HzProduct::F64, last = HzProduct::F64;
  if (pl.skip0 && in.tol < 0.0 && in.has_H32 && std::isfinite(in.hmax) && in.hmax > 0.0 && in.T >= 16 && !sw.f32_off) {
    middle = HzProduct::F32;
    if (in.has_Hs && !sw.split_off) {
      middle = HzProduct::Split;
      if (!sw.split_last_off) last = HzProduct::SplitRows;
    }
  }
  // ... and the formats between them follow from the kernels
  for (int sp = 1; sp <= pl.d0; ++sp) {
    pl.product[sp] = sp < pl.d0 ? middle : last;
    pl.products_f32 += pl.product[sp] == HzProduct::F32 || pl.product[sp] == HzProduct::Split;
    pl.products_split_last += pl.product[sp] == HzProduct::SplitRows;
  }
  pl.z0 = operand_of(pl.product[1]);
  for (int sp = 1; sp < pl.d0; ++sp) {
    pl.mid_in[sp] = result_of(pl.product[sp]);
    pl.mid_out[sp] = operand_of(pl.product[sp + 1]);
  }
  // ... three terms in the split products two or more short of the last (7), and the planes each one is fed
  for (int sp = 1; sp <= pl.d0; ++sp) {
    if (operand_of(pl.product[sp]) != ZFmt::Split) continue;
    pl.terms[sp] = pl.product[sp] == HzProduct::Split && sp <= pl.d0 - 2 && !sw.split3_off ? 3 : 6;
    pl.products_split3 += pl.terms[sp] == 3;
    (sp == 1 ? pl.z0_planes : pl.mid_planes[sp - 1]) = FilterPlan::planes_of(pl.product[sp], pl.terms[sp]);
  }
  pl.pad_rows = (16 - (in.T & 15)) & 15;
  pl.zero_zpad = pl.pad_rows != 0 && !pl.writes_z64();
  return pl;
}

}  // namespace dfm
