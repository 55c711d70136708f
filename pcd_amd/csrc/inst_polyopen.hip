// One object per scalar field (compile with -DPCD_FIELD_IDX=0..3): K13's three kernels (poly.hip.h poly_open_tiles,
// poly_open_carry_scan, poly_open_div_tiles), the divisions of a round's openings batched over parts.  A unit of its own, as
// inst_marlin2.hip is: at 753 bits it compiles beside k9_% and k12_% instead of behind inst_field.hip, whose kernels keep their code.
// inst_field.hip puts the two entries into its FieldEntry.
#include "common.h"
#include <string.h>

#include "poly.hip.h"

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

namespace {
typedef PolyCfg<FTP> PC;
uint64_t open_tiles(uint64_t len) { return std::max<uint64_t>(1, (len + PC::TILE - 1) / PC::TILE); }
}  // namespace

// tiles and carries of every part, z^TILE of every point (device image)
size_t PCD_CAT(pcd_poly_open_scratch_words_, PCD_FIELD_IDX)(uint32_t n_parts, uint32_t n_points, uint64_t max_len) {
  return (2 * (size_t)n_parts * open_tiles(max_len) + n_points) * FTP::WORDS;
}

hipError_t PCD_CAT(pcd_poly_open_, PCD_FIELD_IDX)(hipStream_t st, const PolyOpenPart* parts_dev, const PolyOpenTerm* terms_dev,
                                                  const uint32_t* elts_abi_dev, const uint32_t* points_abi_dev, uint32_t n_parts,
                                                  uint32_t n_points, uint64_t max_len, uint32_t* scratch, uint32_t* values_abi_dev,
                                                  uint32_t* launches) {
  if (launches) *launches = 0;
  if (n_parts == 0) return hipSuccess;
  if (n_parts > 65535 || max_len == 0 || max_len >= (1ull << 31)) return hipErrorInvalidValue;
  const uint64_t K = open_tiles(max_len);
  uint32_t* tiles = scratch;
  uint32_t* carries = scratch + (size_t)n_parts * K * FTP::WORDS;
  uint32_t* zt = carries + (size_t)n_parts * K * FTP::WORDS;
  const dim3 grid((uint32_t)K, n_parts);
  hipLaunchKernelGGL(poly_open_tiles<FTP>, grid, dim3(PC::B), 0, st, parts_dev, terms_dev, elts_abi_dev, points_abi_dev, tiles, (uint32_t)K, zt);
  hipLaunchKernelGGL(poly_open_carry_scan<FTP>, dim3(1, n_parts), dim3(PC::CB), 0, st, parts_dev, tiles, (uint32_t)K, zt, carries, values_abi_dev);
  uint32_t n = 2;
  if (max_len > 1) {
    hipLaunchKernelGGL(poly_open_div_tiles<FTP>, grid, dim3(PC::B), 0, st, parts_dev, elts_abi_dev, points_abi_dev, carries, (uint32_t)K);
    n = 3;
  }
  if (launches) *launches = n;
  (void)n_points;
  return hipGetLastError();
}

}  // namespace pcd
