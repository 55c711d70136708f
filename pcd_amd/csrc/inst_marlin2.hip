// One object per scalar field (compile with -DPCD_FIELD_IDX=0..3): K12's marlin_sumcheck2_q (marlin.hip.h), the second sumcheck's
// q = a - b f in one launch.  A unit of its own beside inst_marlin.hip: the kernel carries the rational sumcheck's 14 product sites and
// two more, and at 753 bits that body is as long to compile as the whole of inst_marlin.hip -- the two objects of a field build side by
// side instead of one behind the other.  inst_field.hip puts the entry into its FieldEntry.
#include "common.h"

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

// q_out_i = a_i - b_i f_i for i < n; the twelve vectors and the constants as for pcd_marlin_sumcheck_ab_; q_out may be f
hipError_t PCD_CAT(pcd_marlin_sumcheck2_q_, PCD_FIELD_IDX)(hipStream_t st, const uint32_t* alpha_abi, const uint32_t* beta_abi,
                                                           const uint32_t* coeff_abi, const uint32_t* const row[3], const uint32_t* const col[3],
                                                           const uint32_t* const rc[3], const uint32_t* const val[3], const uint32_t* f,
                                                           uint64_t n, uint32_t* q_out) {
  if (n == 0) return hipSuccess;
  const MarlinSumcheckConsts<FTP> k = marlin_sumcheck_consts<FTP>(alpha_abi, beta_abi, coeff_abi);
  MarlinSumcheckIn in;
  for (int m = 0; m < 3; m++) { in.row[m] = row[m]; in.col[m] = col[m]; in.rc[m] = rc[0] ? rc[m] : nullptr; in.val[m] = val[m]; }
  hipLaunchKernelGGL(marlin_sumcheck2_q<FTP>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, k, in, f, n, q_out);
  return hipGetLastError();
}

}  // namespace pcd
