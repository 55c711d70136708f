// Stand-alone host program (tests/test_gpu_msm_epilogue.py::test_plan_function_on_host): prints what the chunk rule of the MSM accumulation
// (pcd_amd/csrc/msm.hip.h: msm_plan_chunk, msm_plan_rounds and the packed plan word every lane evaluates on the device) returns on the
// host -- the functions are __host__ __device__, so this is the code the kernels run.  No GPU is touched.
//   msm_plan_check <lanes> <lo> <hi> <M>...   ->   one line per M: "M chunk rounds chunk_of_word word_lanes word_lo word_hi"
#include <cstdio>
#include <cstdlib>

#include "../../pcd_amd/csrc/msm.hip.h"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const uint32_t lanes = (uint32_t)strtoul(argv[1], nullptr, 10), lo = (uint32_t)strtoul(argv[2], nullptr, 10), hi = (uint32_t)strtoul(argv[3], nullptr, 10);
  const uint64_t word = pcd::msm_plan_word(lanes, lo, hi);
  for (int i = 4; i < argc; i++) {
    const uint32_t M = (uint32_t)strtoul(argv[i], nullptr, 10);
    printf("%u %u %llu %u %u %u %u\n", M, pcd::msm_plan_chunk(M, lanes, lo, hi), (unsigned long long)pcd::msm_plan_rounds(M, lanes, hi),
           pcd::msm_chunk_of_plan(M, word), (uint32_t)(word & 0xFFFFFu), (uint32_t)(word >> 20) & 255u, (uint32_t)(word >> 28) & 255u);
  }
  return 0;
}
