// Stand-alone host program (tests/test_msm_bin_staged_host.py, tests/test_gpu_msm_bin_staged.py): prints the constants of the staged per-bin
// sort of the partition sort (pcd_amd/csrc/msm.hip.h: msm_bin_sort_staged_kernel) as the host code that launches it sees them.  No GPU is touched.
//   msm_bin_stage_check  ->  "const cap block per lds_bytes bin_shift"
#include <cstdio>

#include "../../pcd_amd/csrc/msm.hip.h"

int main() {
  printf("const %u %d %d %zu %d\n", pcd::MSM_BIN_STAGE_CAP, pcd::MSM_BIN_STAGE_BLOCK, pcd::MSM_BIN_STAGE_PER, pcd::msm_bin_stage_lds_bytes(),
         pcd::MSM_BIN_SHIFT);
  return 0;
}
