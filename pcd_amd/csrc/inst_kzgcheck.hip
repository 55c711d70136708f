// One object per curve (compile with -DPCD_CURVE_IDX=0..3): K14's two kernels (kzg_check.hip.h), the scalar collapse over the curve's
// scalar field and the hand-over of the short MSMs' results to the pairing over its G1.  A unit of its own, as inst_polyopen.hip is: the
// 753-bit instantiations compile beside the other objects, and no other unit changes for them.  capi_kzg.hip calls the two entries by
// curve (the scalar collapse by field: curve c serves the field pcdhip_curve_scalar_field(c)).
#include "common.h"
#include "kzg_check.hip.h"

namespace pcd {

#if PCD_CURVE_IDX == 0
typedef G1_MNT4_298 G1T;
#elif PCD_CURVE_IDX == 1
typedef G1_MNT6_298 G1T;
#elif PCD_CURVE_IDX == 2
typedef G1_MNT4_753 G1T;
#elif PCD_CURVE_IDX == 3
typedef G1_MNT6_753 G1T;
#else
#error "PCD_CURVE_IDX must be 0..3"
#endif

#define PCD_CAT_(a, b) a##b
#define PCD_CAT(a, b) PCD_CAT_(a, b)

namespace {
typedef Fp<typename G1T::FR> FRT;  // (the product inlined at 298 bits, one copy per code object at 753)
}

// left: E x N canonical scalars, right: E x P (device memory)
hipError_t PCD_CAT(pcd_kzg_check_scalars_, PCD_CURVE_IDX)(hipStream_t st, const KzgCheckTables& t, uint32_t* left, uint32_t* right) {
  const uint64_t lanes = (uint64_t)t.E * (2ull + t.n_shift + 2ull * t.m + 2ull * t.P);
  if (lanes == 0) return hipSuccess;
  if (lanes >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((kzg_check_scalars_kernel<FRT>), dim3((uint32_t)((lanes + 63) / 64)), dim3(64), 0, st, t, left, right);
  return hipGetLastError();
}

// jac: n Jacobian points (device image), even ones negated on the way; out_z null: whole Jacobian points in the C-ABI image into out
hipError_t PCD_CAT(pcd_kzg_check_pairs_, PCD_CURVE_IDX)(hipStream_t st, const uint32_t* jac, uint32_t n, uint32_t* out, uint32_t* out_z) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((kzg_check_pairs_kernel<G1T>), dim3((n + 63) / 64), dim3(64), 0, st, jac, n, out, out_z);
  return hipGetLastError();
}

}  // namespace pcd
