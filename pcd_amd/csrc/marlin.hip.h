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

// ---- K10, the index's arithmetisation: the row / col / row_col / val evaluations on K of the three constraint matrices, one launch.
// Lane k of matrix M (blockIdx.y) owns entry k of M in the index's order -- row by row, ascending column inside a row, which is how the
// host lays the CSR out before the upload -- and writes, as ABI words,
//   row_k = w^pi(c)   col_k = w^r   row_col_k = row_k col_k   val_k = v w^pi(c) / |H|          for k < nnz_M,
//   row_k = col_k = row_col_k = 1,  val_k = 0                                                   for nnz_M <= k < |K|.
// r: the row that holds entry k, found in the resident row pointers -- the largest r with rp[r] <= k, which steps over runs of empty
// rows (their pointers are equal, and the search keeps the last of them that is not beyond k).  pi = reindex_by_subdomain in the
// lane; with period == 1 (|X| = |H|) every column is an instance column, so the quotient by period - 1 is never formed.  w^j from the
// transform's resident powers, as in marlin_lagrange_diffs: beyond the table of a mixed-radix H, times (w^tw_len)^(j / tw_len).
// Scales: the table holds w^j R'; times cout = R it is w^j R, the ABI image (row, col).  row_col = (w^pi(c) R') (w^r R) / R'.
// val = (v R as read) (w^pi(c) / |H| R') / R', the second factor one product with the host's constant h_inv = R' / |H|.
// Product sites: the power beyond the table (pow_u64's two and one more; never taken by a radix-2 H), one for the three products with
// a constant (a loop: cout, cout, h_inv), row_col and val.
template <class F>
struct MarlinIndexArgs {
  const uint64_t* rp[3];     // rows + 1 entries each
  const uint32_t* col[3];    // nnz_M column indices, the index's order
  const uint32_t* coeff[3];  // nnz_M coefficients, ABI words
  uint32_t* out[3][4];       // row, col, row_col, val: k_n elements each, ABI words
  uint32_t nnz[3];
  uint32_t rows, k_n;
  uint32_t x_n, period;      // |X| and |H| / |X|
  const uint32_t* tw;        // tw_len resident powers of w (device image); null for |H| = 1
  uint32_t tw_len;
  F w_len;                   // w^tw_len
  F h_inv;                   // 1 / |H| on the scale R'
  PolyAbiElt<F> one_abi;     // the ABI words of 1
};

template <class F>
PCD_DEV F marlin_domain_power(const uint32_t* __restrict__ tw, uint32_t tw_len, const F& w_len, uint32_t j) {
  if (!tw) return F::one();
  F p = F::load(tw + (size_t)(j % tw_len) * F::WORDS);
  if (j >= tw_len) p = p * w_len.pow_u64(j / tw_len);
  return p;
}

template <class F>
__global__ void __launch_bounds__(256) marlin_index_arith(const MarlinIndexArgs<F> a) {
  constexpr int AW = F::ABI_WORDS;
  const uint32_t M = blockIdx.y;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.k_n) return;
  uint32_t* const row_out = a.out[M][0] + (size_t)k * AW;
  uint32_t* const col_out = a.out[M][1] + (size_t)k * AW;
  uint32_t* const rc_out = a.out[M][2] + (size_t)k * AW;
  uint32_t* const val_out = a.out[M][3] + (size_t)k * AW;
  if (k >= a.nnz[M]) {
#pragma unroll
    for (int i = 0; i < AW; i++) { row_out[i] = a.one_abi.w[i]; col_out[i] = a.one_abi.w[i]; rc_out[i] = a.one_abi.w[i]; val_out[i] = 0; }
    return;
  }
  // the row of entry k: rp[lo] <= k < rp[hi] throughout (rp[0] = 0, rp[rows] = nnz > k)
  const uint64_t* __restrict__ rp = a.rp[M];
  uint32_t lo = 0, hi = a.rows;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (rp[mid] <= k) lo = mid; else hi = mid;
  }
  const uint32_t c = a.col[M][k];
  uint32_t j;
  if (a.period == 1 || c < a.x_n) j = c * a.period;
  else { const uint32_t i = c - a.x_n; j = i + i / (a.period - 1) + 1; }
  F cout;
#pragma unroll
  for (int i = 0; i < F::N; i++) cout.v[i] = F::Params::cout(i);
  F wj = F::zero(), wh = F::zero(), col_r = F::zero();
#pragma unroll 1
  for (int s = 0; s < 3; s++) {  // s = 0: col = w^r R;  1: row = w^j R;  2: wh = w^j / |H| on the scale R'
    const F p = s == 2 ? wj : marlin_domain_power<F>(a.tw, a.tw_len, a.w_len, s == 0 ? lo : j);
    const F o = p * (s == 2 ? a.h_inv : cout);
    if (s == 0) { col_r = o; o.canonical().pack32(col_out); }
    else if (s == 1) { wj = p; o.canonical().pack32(row_out); }
    else wh = o;
  }
  (wj * col_r).canonical().pack32(rc_out);
  (F::unpack32(a.coeff[M] + (size_t)k * AW) * wh).canonical().pack32(val_out);
}

// ---- K11, round 1 and the first sumcheck.
// The pointwise core of the first sumcheck's quotient: for i < n
//   q_i = r_i (za_i (eta_A + eta_C zb_i) + eta_B zb_i) - t_i z_i
// from five vectors read once as ABI words (the scale R), one store.  Scales: u = eta_C zb + eta_A on R' (eta_C brought to R'^2 / R on
// the host, eta_A to R'), s = za u + eta_B zb on R (eta_B on R'), d = r s - t z on R^2 / R' -- t and z are both as read, so their
// product cannot land on R by a constant's scale -- and q = d cin on R, the ABI image.  The five products of the formula are one
// product and two fused pairs (Fp::dot2: two products under ONE reduction each), the sixth brings d to the scale R: four product
// sites, six products' multiply-adds, four reductions.  Every load of element i precedes its store and no pointer is declared
// restrict, so q_out may be any one of the inputs (or several, when those are the same vector).
template <class F>
struct MarlinSumcheck1Consts { F eta_a, eta_b, eta_c2; };  // eta_A, eta_B on the scale R', eta_C on R'^2 / R
template <class F>
inline MarlinSumcheck1Consts<F> marlin_sumcheck1_consts(const uint32_t* eta_abi) {
  constexpr int AW = F::ABI_WORDS;
  F cin;
  for (int i = 0; i < F::N; i++) cin.v[i] = F::Params::cin(i);
  MarlinSumcheck1Consts<F> k;
  k.eta_a = F::from_abi(eta_abi);
  k.eta_b = F::from_abi(eta_abi + AW);
  k.eta_c2 = F::from_abi(eta_abi + 2 * AW) * cin;
  return k;
}
// element i of q (host and device, like marlin_sumcheck_element)
template <class F>
PCD_HD void marlin_sumcheck1_element(const MarlinSumcheck1Consts<F>& k, const uint32_t* za, const uint32_t* zb, const uint32_t* r,
                                     const uint32_t* t, const uint32_t* z, uint64_t i, uint32_t* q_out) {
  constexpr int AW = F::ABI_WORDS;
  F cin;
#pragma unroll
  for (int j = 0; j < F::N; j++) cin.v[j] = F::Params::cin(j);
  const F b = F::unpack32(zb + i * AW);
  const F u = k.eta_c2 * b + k.eta_a;
  const F s = F::dot2(F::unpack32(za + i * AW), u, k.eta_b, b);
  const F d = F::dot2(F::unpack32(r + i * AW), s, F::unpack32(t + i * AW).neg(), F::unpack32(z + i * AW));
  (d * cin).canonical().pack32(q_out + i * AW);
}
template <class F>
__global__ void __launch_bounds__(256) marlin_sumcheck1_q(const MarlinSumcheck1Consts<F> k, const uint32_t* za, const uint32_t* zb,
                                                          const uint32_t* r, const uint32_t* t, const uint32_t* z, uint64_t n,
                                                          uint32_t* q_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) marlin_sumcheck1_element<F>(k, za, zb, r, t, z, i, q_out);
}

// z on H at reindex_by_subdomain's places, a gather without arithmetic: lane k < h_n finds the variable c with pi(c) = k -- k / period
// on the subdomain X (k a multiple of period), else x_n + (k - k / period - 1) -- and copies its ABI words; c >= num_cols reads as 0.
// period == 1 (X = H): every k is on X, out[k] = z[k].
template <int AW>
__global__ void __launch_bounds__(256) marlin_place_assignment(const uint32_t* __restrict__ z, uint64_t num_cols, uint64_t x_n,
                                                               uint64_t period, uint64_t h_n, uint32_t* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= h_n) return;
  const uint64_t c = k % period == 0 ? k / period : x_n + (k - k / period - 1);
  const uint32_t* src = z + c * AW;
  uint32_t* dst = out + k * AW;
#pragma unroll
  for (int i = 0; i < AW; i++) dst[i] = c < num_cols ? src[i] : 0u;
}

// out_i = a_i + b_i (sub == 0) or a_i - b_i for i < n, ABI words: linear, so the words are summed as read.  out may be a or b.
template <class F>
__global__ void __launch_bounds__(256) marlin_vec_addsub(const uint32_t* a, const uint32_t* b, uint64_t n, int sub, uint32_t* out) {
  constexpr int AW = F::ABI_WORDS;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const F x = F::unpack32(a + i * AW), y = F::unpack32(b + i * AW);
  (sub ? x - y : x + y).canonical().pack32(out + i * AW);
}

// p <- p + blind(X) (X^n - 1) for blind of k coefficients (ABI words, on the device), over the touched coefficients only: lane l owns
// index l < k (p_l - blind_l) or n + (l - k) (p + blind_(l - k)) when the two windows are apart (k <= n), and index l < n + k when
// they overlap.  The caller has zeroed p beyond its old length.
template <class F>
__global__ void __launch_bounds__(256) marlin_add_vanishing_multiple(uint32_t* p, const uint32_t* __restrict__ blind, uint64_t k, uint64_t n) {
  constexpr int AW = F::ABI_WORDS;
  const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t lanes = k <= n ? 2 * k : n + k;
  if (l >= lanes) return;
  const uint64_t idx = (k <= n && l >= k) ? n + (l - k) : l;
  F acc = F::unpack32(p + idx * AW);
  if (idx < k) acc = acc - F::unpack32(blind + idx * AW);
  if (idx >= n && idx - n < k) acc = acc + F::unpack32(blind + (idx - n) * AW);
  acc.canonical().pack32(p + idx * AW);
}

// ---- K12, the second sumcheck.
// The pointwise core of its quotient: q_i = a_i - b_i f_i for i < n, a and b those of marlin_sumcheck_ab, from thirteen vectors read
// once as ABI words and one store; a and b stay in registers.  The body up to the end of the loop is marlin_sumcheck_element's, line
// for line, and on purpose a second copy of it: factored into a function that both kernels call (a and b handed back by reference,
// or as a pair by value), the compiler's report for marlin_sumcheck_ab itself changed -- at 298 bits 108 -> 102 and 122 VGPRs, at 753
// bits ScratchSize 0 -> 1300 bytes a lane and 2 -> 1 waves per SIMD -- so K9's kernel stays as it was and this one has its own text.
// Scales: the loop leaves a and b on R, and f is read on R, so b f would land on R^2 / R' and no constant can mend that inside the
// one product.  Instead f' = f cin is on R (R'^2 / R) / R' = R', then b f' is on R R' / R' = R beside a, and q = a - b f' is the ABI
// image once canonical.  Two products beyond marlin_sumcheck_ab's: 19 with row_col, 17 without, at 16 product sites (its 14 and
// these two).  The two are a chain -- no sum of two products stands in the formula -- so Fp::dot2 has nothing to fuse here:
// dot2(a, R, -b, f) cin would be three products' multiply-adds under the same two reductions.  f is loaded behind the loop, so that
// nothing of it is held across the loop's products; every load of element i still precedes the store and q_out is not declared
// restrict, so q_out may be f.
// element i of q (host and device, like marlin_sumcheck_element)
template <class F>
PCD_HD void marlin_sumcheck2_element(const MarlinSumcheckConsts<F>& k, const MarlinSumcheckIn& in, const uint32_t* f, uint64_t i,
                                     uint32_t* q_out) {
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
  const F fp = F::unpack32(f + i * AW) * cin;
  (a - b * fp).canonical().pack32(q_out + i * AW);
}
template <class F>
__global__ void __launch_bounds__(256) marlin_sumcheck2_q(const MarlinSumcheckConsts<F> k, const MarlinSumcheckIn in, const uint32_t* f,
                                                          uint64_t n, uint32_t* q_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) marlin_sumcheck2_element<F>(k, in, f, i, q_out);
}

}  // namespace pcd
