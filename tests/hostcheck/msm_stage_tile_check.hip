// Stand-alone host program (tests/test_msm_coarse_staged_host.py, tests/test_gpu_msm_coarse_staged.py): prints what the tile rule of the
// staged write pass of the partition sort (pcd_amd/csrc/msm.hip.h: msm_stage_tile, msm_stage_lds_bytes) returns on the host, with the
// constants it is built from -- the function is __host__ __device__ and msm_run calls this very code before its launches.  No GPU is touched.
//   msm_stage_tile_check                    ->  "const budget tile_min tile_max w_max min_run bin_shift sign_at g_at g_bits idx_at idx_bits"
//                                               then one line per (W = 1 .. 64, nbins = 1, 2, 4 .. 8192): "W nbins tile lds_bytes"
//   msm_stage_tile_check <W> <nbins> ...    ->  the same line for the given pairs only (any values)
// tile = 0: no tile fits (msm_run launches the direct write pass); lds_bytes = the footprint at the chosen tile, or at tile_min when none fits
#include <cstdio>
#include <cstdlib>

#include "../../pcd_amd/csrc/msm.hip.h"

static void line(int W, uint32_t nbins) {
  const uint32_t tile = pcd::msm_stage_tile(W, nbins);
  printf("%d %u %u %zu\n", W, nbins, tile, pcd::msm_stage_lds_bytes(tile ? tile : pcd::MSM_STAGE_TILE_MIN, W, nbins));
}

int main(int argc, char** argv) {
  printf("const %zu %u %u %d %u %d %d %d %d %d %d\n", pcd::MSM_STAGE_LDS_BUDGET, pcd::MSM_STAGE_TILE_MIN, pcd::MSM_STAGE_TILE_MAX, pcd::MSM_STAGE_W_MAX,
         pcd::MSM_STAGE_MIN_RUN, pcd::MSM_BIN_SHIFT, pcd::MSM_STAGE_SIGN_AT, pcd::MSM_STAGE_G_AT, pcd::MSM_STAGE_G_BITS, pcd::MSM_STAGE_IDX_AT,
         pcd::MSM_STAGE_IDX_BITS);
  if (argc > 1) {
    for (int i = 1; i + 1 < argc; i += 2) line(atoi(argv[i]), (uint32_t)strtoul(argv[i + 1], nullptr, 10));
    return 0;
  }
  for (int W = 1; W <= 64; W++)
    for (uint32_t nbins = 1; nbins <= 8192; nbins <<= 1) line(W, nbins);
  return 0;
}
