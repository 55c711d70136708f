// Stand-alone host program (tests/test_msm_short_batch_host.py): prints what the host-side planner of the batched short MSM
// (pcd_amd/csrc/msm_short.hip.h: msm_short_batch_plan, and msm_short_plan per item beside it) returns -- the code the library runs before
// its launches.  No GPU is touched.
//   msm_short_batch_plan_check <per_wave: 64 | 32 | 21> <groups> <n>...
//   ->  "plan span entries parts folds err_words table_words scratch_words jac_words"
//       one line per item:   "item j n single_parts"                                 (single_parts: msm_short_plan's, 0 for n == 0)
//       one line per entry:  "entry e offset n part0 parts row0 out_slot scalars"    (scalars: the pointer as a number)
//       "part_item e..."  and  "fold_item e..."                                      (the two lists of the table)
// Item j is given offset j, out_slot 100 + j and the scalar pointer 4096 * (j + 1), so an entry says which item it came from.
#include <cstdio>
#include <cstdlib>

#include "../../pcd_amd/csrc/msm_short.hip.h"

template <class G>
int run(int groups, int argc, char** argv) {
  using namespace pcd;
  static_assert(sizeof(MsmShortBatchItem) == 32, "entry size");
  std::vector<MsmShortBatchIn> items;
  for (int i = 3; i < argc; i++) {
    const uint32_t j = (uint32_t)items.size();
    items.push_back({(const uint32_t*)(uintptr_t)(4096u * (j + 1)), j, (uint32_t)strtoul(argv[i], nullptr, 10), 100u + j});
  }
  // the view of a vector with `groups` window copies (c = 8 as a stand-in: only span depends on it) or a plain one
  const MsmBasesView bv = {nullptr, 4096u, 0u, groups > 1 ? 8 : 0, groups, nullptr};
  const MsmShortBatchPlan pl = msm_short_batch_plan<G>(bv, items.data(), items.size());
  printf("plan %u %u %u %u %zu %zu %zu %d\n", pl.span, pl.entries, pl.parts, pl.folds, pl.err_words, pl.table_words, pl.scratch_words,
         (int)Jac<typename G::F>::WORDS);
  if (pl.table.size() != pl.table_words) return 3;
  for (size_t j = 0; j < items.size(); j++) printf("item %zu %u %u\n", j, items[j].n, items[j].n ? msm_short_plan<G>(bv, items[j].n).parts : 0u);
  const MsmShortBatchItem* ent = (const MsmShortBatchItem*)pl.table.data();
  for (uint32_t e = 0; e < pl.entries; e++)
    printf("entry %u %u %u %u %u %u %u %llu\n", e, ent[e].offset, ent[e].n, ent[e].part0, ent[e].parts, ent[e].row0, ent[e].out_slot,
           (unsigned long long)(uintptr_t)ent[e].scalars);
  printf("part_item");
  for (uint32_t p = 0; p < pl.parts; p++) printf(" %u", pl.table[pl.part_item_off() + p]);
  printf("\nfold_item");
  for (uint32_t f = 0; f < pl.folds; f++) printf(" %u", pl.table[pl.fold_item_off() + f]);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int per_wave = atoi(argv[1]), groups = atoi(argv[2]);
  static_assert(pcd::MsmItems<pcd::G1_MNT4_298>::PER_WAVE == 64 && pcd::MsmItems<pcd::G2_MNT4_298>::PER_WAVE == 32 &&
                pcd::MsmItems<pcd::G2_MNT6_298>::PER_WAVE == 21, "one group per lane split");
  if (per_wave == 64) return run<pcd::G1_MNT4_298>(groups, argc, argv);
  if (per_wave == 32) return run<pcd::G2_MNT4_298>(groups, argc, argv);
  if (per_wave == 21) return run<pcd::G2_MNT6_298>(groups, argc, argv);
  return 2;
}
