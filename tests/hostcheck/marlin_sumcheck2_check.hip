// TEST HARNESS ONLY (never part of libpcdhip.so): K12's element function marlin_sumcheck2_element (marlin.hip.h) -- q = a - b f of the
// second sumcheck, the body of the kernel marlin_sumcheck2_q -- compiled for the HOST and run over case lists from a file, so that its
// scales are checked where no device is.  tests/test_marlin_sumcheck2_host.py builds it, writes the cases and compares the words.
//   marlin_sumcheck2_check <field 0..3> <cases file> <output file>
// The cases file is a sequence of lists, all of 64-bit little-endian words: n, have_row_col, then alpha, beta, c_A, c_B, c_C and the
// thirteen vectors row_A row_B row_C col_A .. col_C row_col_A .. row_col_C val_A .. val_C f of n elements each, every element as its
// C-ABI Montgomery limbs (row_col is present but not read when have_row_col is 0).  The output file gets the n elements of q of every
// list, one list behind the other.  Prints "ok <lists> <elements>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pcd_amd/csrc/common.h"

#include "../../pcd_amd/csrc/marlin.hip.h"
using namespace pcd;

template <class F>
static int run(FILE* in, FILE* out) {
  constexpr int AW = F::ABI_WORDS, L = AW / 2;
  long lists = 0, elements = 0;
  uint64_t head[2];
  while (fread(head, 8, 2, in) == 2) {
    const size_t n = head[0];
    std::vector<uint64_t> consts(5 * L), vecs(13 * n * L), q(n * L);
    if (fread(consts.data(), 8, consts.size(), in) != consts.size()) return 2;
    if (!vecs.empty() && fread(vecs.data(), 8, vecs.size(), in) != vecs.size()) return 2;
    const uint32_t* c = (const uint32_t*)consts.data();
    const MarlinSumcheckConsts<F> k = marlin_sumcheck_consts<F>(c, c + AW, c + 2 * AW);
    auto vec = [&](int j) { return (const uint32_t*)(vecs.data() + (size_t)j * n * L); };
    MarlinSumcheckIn si;
    for (int m = 0; m < 3; m++) { si.row[m] = vec(m); si.col[m] = vec(3 + m); si.rc[m] = head[1] ? vec(6 + m) : nullptr; si.val[m] = vec(9 + m); }
    for (size_t i = 0; i < n; i++) marlin_sumcheck2_element<F>(k, si, vec(12), i, (uint32_t*)q.data());
    if (n && fwrite(q.data(), 8, q.size(), out) != q.size()) return 2;
    lists++;
    elements += (long)n;
  }
  printf("ok %ld %ld\n", lists, elements);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s <field 0..3> <cases file> <output file>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  int rc = 2;
  switch (atoi(argv[1])) {
    case 0: rc = run<Fp<F298A, true>>(in, out); break;
    case 1: rc = run<Fp<F298B, true>>(in, out); break;
    case 2: rc = run<Fp<F753A, true>>(in, out); break;
    case 3: rc = run<Fp<F753B, true>>(in, out); break;
    default: fprintf(stderr, "no such field\n");
  }
  fclose(in);
  return fclose(out) == 0 ? rc : 2;
}
