// One object per scalar field (compile with -DPCD_FIELD_IDX=0..3): the K9 kernels whose products are inlined (marlin.hip.h) -- the
// differences behind r(alpha, .) on H, the rational sumcheck, the K10 arithmetisation of the index, and K11's first sumcheck with the
// small kernels of round 1.  A unit of its own so that their 753-bit bodies compile beside the
// field objects; inst_field.hip puts the entries into its FieldEntry.
#include "common.h"
#include <string.h>

#include "marlin.hip.h"

namespace pcd {

#if PCD_FIELD_IDX == 0
typedef Fp<F298A, true> FTP;
#elif PCD_FIELD_IDX == 1
typedef Fp<F298B, true> FTP;
#elif PCD_FIELD_IDX == 2
typedef Fp<F753A, true> FTP;
#elif PCD_FIELD_IDX == 3
typedef Fp<F753B, true> FTP;
#else
#error "PCD_FIELD_IDX must be 0..3"
#endif

#define PCD_CAT_(a, b) a##b
#define PCD_CAT(a, b) PCD_CAT_(a, b)

// out_i = x - w^i for i < n (ABI words) and vh_abi = x^n - 1, formed on the host.  domain_consts = FftTables::consts of the domain
// (DomainConsts and MixedConsts both start with its generator), tw = its tw_len resident powers; both null for n == 1
hipError_t PCD_CAT(pcd_marlin_diffs_, PCD_FIELD_IDX)(hipStream_t st, const void* domain_consts, const uint32_t* tw, uint32_t tw_len,
                                                     const uint32_t* x_abi, uint64_t n, uint32_t* out, uint32_t* vh_abi) {
  FTP w = FTP::one();
  if (domain_consts) memcpy(&w, domain_consts, sizeof w);
  PolyAbiElt<FTP> x;
  memcpy(x.w, x_abi, sizeof x.w);
  (FTP::from_abi(x_abi).pow_u64(n) - FTP::one()).to_abi(vh_abi);
  const uint64_t lanes = (n + MARLIN_LAG_E - 1) / MARLIN_LAG_E;
  hipLaunchKernelGGL(marlin_lagrange_diffs<FTP>, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, tw, tw_len, w,
                     tw ? w.pow_u64(tw_len) : FTP::one(), x, n, out);
  return hipGetLastError();
}

hipError_t PCD_CAT(pcd_marlin_sumcheck_ab_, PCD_FIELD_IDX)(hipStream_t st, const uint32_t* alpha_abi, const uint32_t* beta_abi,
                                                           const uint32_t* coeff_abi, const uint32_t* const row[3], const uint32_t* const col[3],
                                                           const uint32_t* const rc[3], const uint32_t* const val[3], uint64_t n,
                                                           uint32_t* a_out, uint32_t* b_out) {
  if (n == 0) return hipSuccess;
  const MarlinSumcheckConsts<FTP> k = marlin_sumcheck_consts<FTP>(alpha_abi, beta_abi, coeff_abi);
  MarlinSumcheckIn in;
  for (int m = 0; m < 3; m++) { in.row[m] = row[m]; in.col[m] = col[m]; in.rc[m] = rc[0] ? rc[m] : nullptr; in.val[m] = val[m]; }
  hipLaunchKernelGGL(marlin_sumcheck_ab<FTP>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, k, in, n, a_out, b_out);
  return hipGetLastError();
}

// K10: the twelve evaluation vectors on K of an index.  1 / |H| comes from the domain's constants (slot 4 of DomainConsts and of
// MixedConsts, device image); |H| = 1 has no tables and w = 1 / |H| = 1
hipError_t PCD_CAT(pcd_marlin_index_arith_, PCD_FIELD_IDX)(hipStream_t st, const void* domain_consts, const uint32_t* tw, uint32_t tw_len,
                                                           const MarlinIndexIn& in) {
  if (in.k_n == 0) return hipSuccess;
  MarlinIndexArgs<FTP> a;
  for (int m = 0; m < 3; m++) {
    a.rp[m] = in.rp[m]; a.col[m] = in.col[m]; a.coeff[m] = in.coeff[m]; a.nnz[m] = in.nnz[m];
    for (int q = 0; q < 4; q++) a.out[m][q] = in.out[m][q];
  }
  a.rows = in.rows; a.k_n = in.k_n; a.x_n = in.x_n; a.period = in.period;
  a.tw = tw; a.tw_len = tw ? tw_len : 1;
  FTP w = FTP::one();
  a.h_inv = FTP::one();
  if (domain_consts) {
    memcpy(&w, domain_consts, sizeof w);
    memcpy(&a.h_inv, (const char*)domain_consts + 4 * sizeof(FTP), sizeof a.h_inv);
  }
  a.w_len = tw ? w.pow_u64(tw_len) : FTP::one();
  FTP::one().to_abi(a.one_abi.w);
  hipLaunchKernelGGL(marlin_index_arith<FTP>, dim3((in.k_n + 255) / 256, 3), dim3(256), 0, st, a);
  return hipGetLastError();
}

// K11: the first sumcheck's q in one launch (q_out may be one of the inputs), and the three small kernels of round 1 -- the placement
// of the assignment on H, out = a +- b, p += blind (X^n - 1); all vectors ABI words on the device, eta in ABI words on the host
hipError_t PCD_CAT(pcd_marlin_sumcheck1_q_, PCD_FIELD_IDX)(hipStream_t st, const uint32_t* eta_abi, const uint32_t* za, const uint32_t* zb,
                                                           const uint32_t* r, const uint32_t* t, const uint32_t* z, uint64_t n,
                                                           uint32_t* q_out) {
  if (n == 0) return hipSuccess;
  const MarlinSumcheck1Consts<FTP> k = marlin_sumcheck1_consts<FTP>(eta_abi);
  hipLaunchKernelGGL(marlin_sumcheck1_q<FTP>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, k, za, zb, r, t, z, n, q_out);
  return hipGetLastError();
}
hipError_t PCD_CAT(pcd_marlin_place_, PCD_FIELD_IDX)(hipStream_t st, const uint32_t* z, uint64_t num_cols, uint64_t x_n, uint64_t h_n,
                                                     uint32_t* out) {
  if (h_n == 0) return hipSuccess;
  hipLaunchKernelGGL(marlin_place_assignment<FTP::ABI_WORDS>, dim3((uint32_t)((h_n + 255) / 256)), dim3(256), 0, st, z, num_cols, x_n,
                     h_n / x_n, h_n, out);
  return hipGetLastError();
}
hipError_t PCD_CAT(pcd_marlin_addsub_, PCD_FIELD_IDX)(hipStream_t st, const uint32_t* a, const uint32_t* b, uint64_t n, int sub, uint32_t* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(marlin_vec_addsub<FTP>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a, b, n, sub, out);
  return hipGetLastError();
}
hipError_t PCD_CAT(pcd_marlin_add_vanishing_, PCD_FIELD_IDX)(hipStream_t st, uint32_t* p, const uint32_t* blind, uint64_t k, uint64_t n) {
  if (k == 0) return hipSuccess;
  const uint64_t lanes = k <= n ? 2 * k : n + k;
  hipLaunchKernelGGL(marlin_add_vanishing_multiple<FTP>, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, p, blind, k, n);
  return hipGetLastError();
}

}  // namespace pcd
