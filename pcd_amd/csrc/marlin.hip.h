// K9, the data-parallel algebra of Marlin's AHP rounds 2 and 3 on gfx950: the differences x - w^i behind r(alpha, .) on H, and the
// rational sumcheck's numerator a and denominator b in one pass over its twelve input vectors.  (The transposed mat-vec of t(X) sits
// beside the witness map's mat-vecs in inst_field.hip: it shares their small-coefficient sums.)
//
// Vectors are C-ABI Montgomery words (x R, R = 2^(32 ABI_WORDS)) as in a pcdhip_buf, and, as in poly.hip.h, the kernels compute on the
// words as read wherever the step is linear: unpack32 takes x R as a plain integer, a product with a constant brought to the right
// power of R' = 2^(28 N) once on the host lands on the scale that the next step needs, and pack32 of a canonical value on the scale R
// IS the ABI image.  Scales below are the factor an integer carries over the field element it stands for; a Montgomery product of
// integers on the scales s and t is on the scale s t / R'.
#pragma once
#include "poly.hip.h"

namespace pcd {

// ---- r(alpha, .) on H: out_i = x - w^i (ABI words), i < n; the batch inversion of poly.hip.h with the scale x^n - 1 follows.
// A lane owns MARLIN_LAG_E consecutive i: it takes w^(first i) from the transform's resident power table `tw` (tw_len powers of w;
// beyond the table -- a mixed-radix domain keeps only the n / m powers of its row transform -- times (w^tw_len)^(i / tw_len), a power
// with an exponent below m <= 49) and steps by w.  Everything is on the scale R: x as read, w^i R = mul(w^i R', R).
constexpr int MARLIN_LAG_E = 8;
template <class F>
__global__ void __launch_bounds__(256) marlin_lagrange_diffs(const uint32_t* __restrict__ tw, uint32_t tw_len, const F w, const F w_len,
                                                             const PolyAbiElt<F> x_abi, uint64_t n, uint32_t* __restrict__ out) {
  constexpr int AW = F::ABI_WORDS;
  const uint64_t lo = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * MARLIN_LAG_E;
  if (lo >= n) return;
  const int cnt = (int)(n - lo < (uint64_t)MARLIN_LAG_E ? n - lo : (uint64_t)MARLIN_LAG_E);
  F cout;
#pragma unroll
  for (int i = 0; i < F::N; i++) cout.v[i] = F::Params::cout(i);
  F wi = tw ? F::load(tw + (size_t)(lo % tw_len) * F::WORDS) : F::one();  // (no table: the domain of one element)
  if (tw && lo >= tw_len) wi = wi * w_len.pow_u64(lo / tw_len);
  wi = wi * cout;
  const F x = F::unpack32(x_abi.w);
#pragma unroll 1
  for (int k = 0; k < cnt; k++) {
    (x - wi).canonical().pack32(out + (lo + k) * AW);
    wi = wi * w;
  }
}

// ---- the rational sumcheck.  For i < n and the three matrices M = A, B, C:
//   d_M = alpha beta - alpha row_M[i] - beta col_M[i] + row_col_M[i]        (row_col given: the vector taken as it stands)
//   d_M = (beta - row_M[i]) (alpha - col_M[i])                              (row_col null)
//   b_i = d_A d_B d_C        a_i = c_A val_A[i] d_B d_C + c_B val_B[i] d_A d_C + c_C val_C[i] d_A d_B
// One matrix at a time: (a, b) <- (a d_M + u_M b, b d_M) with u_M = c_M val_M, from (u_A, d_A).  a and b stay on the scale R
// throughout, so d_B, d_C and u_B, u_C are formed on the scale R' -- the inputs as read against constants that the host brings to the
// power of R' each product needs (cin = R'^2 / R, k3 = R'^3 / R^2) -- and d_A, u_A on the scale R.  17 products per element with
// row_col (2 + 1, then twice 3 + 1 + 3), 15 without (2 + 1, then twice 2 + 1 + 3).  The two later matrices share ONE loop body and
// the two forms of d one kernel (a uniform branch): 14 product sites in all instead of the 32 of two straight-line kernels of 16
// products -- every site is a 1 458-multiply-add body at 753 bits, and the compile time of that object follows their number.
template <class F>
struct MarlinSumcheckConsts {
  F alpha_p, beta_p, ab_r;   // d_A with row_col: alpha, beta on the scale R', alpha beta on R
  F alpha_r, beta_r;         // without: alpha, beta on the scale R (the ABI words unpacked)
  F alpha_2, beta_2, ab_p;   // d_B, d_C with row_col: alpha, beta on the scale R'^2 / R, alpha beta on R'
  F k3;                      // ... and without: R'^3 / R^2
  F c[3];                    // c_A on the scale R', c_B and c_C on R'^2 / R
};
struct MarlinSumcheckIn { const uint32_t *row[3], *col[3], *rc[3], *val[3]; };

// the constants of a call from its field elements (C-ABI words): once, on the host
template <class F>
inline MarlinSumcheckConsts<F> marlin_sumcheck_consts(const uint32_t* alpha_abi, const uint32_t* beta_abi, const uint32_t* coeff_abi) {
  constexpr int AW = F::ABI_WORDS;
  F cin;
  for (int i = 0; i < F::N; i++) cin.v[i] = F::Params::cin(i);
  MarlinSumcheckConsts<F> k;
  k.alpha_p = F::from_abi(alpha_abi);
  k.beta_p = F::from_abi(beta_abi);
  k.alpha_r = F::unpack32(alpha_abi);
  k.beta_r = F::unpack32(beta_abi);
  k.ab_r = k.alpha_p * k.beta_r;
  k.ab_p = k.alpha_p * k.beta_p;
  k.alpha_2 = k.alpha_p * cin;
  k.beta_2 = k.beta_p * cin;
  k.k3 = cin * cin;
  k.c[0] = F::from_abi(coeff_abi);
  k.c[1] = F::from_abi(coeff_abi + AW) * cin;
  k.c[2] = F::from_abi(coeff_abi + 2 * AW) * cin;
  return k;
}

// element i of a and b (also callable on the host, where a stand-alone check of the scales runs it)
template <class F>
PCD_HD void marlin_sumcheck_element(const MarlinSumcheckConsts<F>& k, const MarlinSumcheckIn& in, uint64_t i, uint32_t* a_out, uint32_t* b_out) {
  constexpr int AW = F::ABI_WORDS;
  const bool rc = in.rc[0] != nullptr;
  F cin;
#pragma unroll
  for (int j = 0; j < F::N; j++) cin.v[j] = F::Params::cin(j);
  const F row0 = F::unpack32(in.row[0] + i * AW), col0 = F::unpack32(in.col[0] + i * AW);
  F b;
  if (rc) b = k.ab_r - k.alpha_p * row0 - k.beta_p * col0 + F::unpack32(in.rc[0] + i * AW);
  else b = ((k.beta_r - row0) * cin) * (k.alpha_r - col0);
  F a = k.c[0] * F::unpack32(in.val[0] + i * AW);
#pragma unroll 1
  for (int m = 1; m < 3; m++) {
    const F row = F::unpack32(in.row[m] + i * AW), col = F::unpack32(in.col[m] + i * AW);
    F d;
    if (rc) d = k.ab_p - k.alpha_2 * row - k.beta_2 * col + F::unpack32(in.rc[m] + i * AW) * cin;
    else d = ((k.beta_r - row) * k.k3) * (k.alpha_r - col);
    const F u = (m == 1 ? k.c[1] : k.c[2]) * F::unpack32(in.val[m] + i * AW);
    a = a * d + u * b;
    b = b * d;
  }
  a.canonical().pack32(a_out + i * AW);
  b.canonical().pack32(b_out + i * AW);
}

template <class F>
__global__ void __launch_bounds__(256) marlin_sumcheck_ab(const MarlinSumcheckConsts<F> k, const MarlinSumcheckIn in, uint64_t n,
                                                          uint32_t* __restrict__ a_out, uint32_t* __restrict__ b_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) marlin_sumcheck_element<F>(k, in, i, a_out, b_out);
}

}  // namespace pcd
