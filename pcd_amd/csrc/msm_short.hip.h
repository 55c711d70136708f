// Short MSMs without buckets: bit-plane sums over the resident copies of a base vector.
//
// A resident vector already holds what makes buckets unnecessary for a handful of pairs: copy g is 2^(span g) P_i (affine, (0,0) for
// the identity) with span = c Wg, Wg = ceil(W / groups) -- or, for a plain vector (groups == 1), span = the scalar bits.  With the
// canonical scalar in plain binary (no signed digits)
//     sum_i k_i P_i = sum_{b < span} 2^b B_b,    B_b = sum over (i < n, g < groups) with bit (span g + b) of k_i set, of copy_g[offset + i]
// so the work is one mixed addition per set bit, spread over span x parts one-wave workgroups, and a chain of `span` doublings behind
// them -- nothing that grows with 2^c.  Stream-ordered launches, no workgroup waits for another:
//   msm_short_planes    grid (span, parts), one wave each: item t walks its share of the n * groups candidates of plane b, adds the
//                       ones whose bit is set and whose base is finite, the wave sums its items by a log-depth tree through LDS:
//                       one Jacobian point per (b, part).  The workgroups of plane 0 also check that every scalar is reduced.
//   msm_short_fold      (parts > 1 only) grid (span): the `parts` partials of plane b summed by one wave, the same tree.
//   msm_short_combine   one workgroup: R = sum_b 2^b B_b.  The doublings are inherent (span of them in series), the additions are not:
//                       item j first runs Horner over its own run of w = ceil(span / items) planes, C_j = sum_d 2^d B_(j w + d) -- all
//                       items at once -- and one item then chains R = 2^w R + C_j: span doublings but only span / w + w additions deep.
// All three compute in the lane-split form the other latency-bound kernels use (MsmItems: 2 / 3 lanes per Fq2 / Fq3 point).  The group
// law is the complete one of ec.hip.h (EC::madd / EC::add fall back to a doubling for equal operands and return the identity for
// opposite ones), so duplicate bases, P next to -P and empty planes need no special case.
// The bodies of the three kernels are device functions; "the batched form" at the end of this file runs them for k MSMs over one vector
// at once behind a descriptor table.  The single kernels do not go through the table: their arguments stay kernel arguments.
#pragma once
#include <string.h>

#include <vector>

#include "msm.hip.h"

namespace pcd {

constexpr uint32_t MSM_SHORT_MAX_N = 1024;  // pairs per call (PCDHIP_E_SIZE_UNSUPPORTED beyond)
constexpr uint32_t MSM_SHORT_E = 4;         // candidates per item of a plane's workgroup: a lane's serial chain is at most this long

struct MsmShortPlan {
  uint32_t span = 0;   // bit planes
  uint32_t parts = 0;  // workgroups per plane
  size_t err_words = 0, scratch_words = 0;  // scratch: [0] the error word, [1 .. parts] one per part, then span * parts Jacobian points
};
template <class G>
MsmShortPlan msm_short_plan(const MsmBasesView& bv, uint32_t n) {
  MsmShortPlan pl;
  const int bits = G::FR::BITS;
  if (bv.groups > 1) {
    const int W = msm_num_windows(bits, bv.c), Wg = (W + bv.groups - 1) / bv.groups;
    pl.span = (uint32_t)(bv.c * Wg);
  } else {
    pl.span = (uint32_t)bits;
  }
  const uint32_t per_wg = MsmItems<G>::PER_WAVE * MSM_SHORT_E;
  pl.parts = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)n * (uint32_t)bv.groups + per_wg - 1) / per_wg));
  pl.err_words = ((size_t)pl.parts + 1 + 3) & ~(size_t)3;
  pl.scratch_words = pl.err_words + (size_t)pl.span * pl.parts * Jac<typename G::F>::WORDS;
  return pl;
}

// the tree of a one-wave workgroup: the sending half of every level posts its points in LDS
template <class G>
struct MsmShortTree {
  typedef MsmItems<G> IT;
  typedef typename IT::GA GA;
  typedef typename GA::F F;
  static constexpr uint32_t PW = IT::PER_WAVE;
  static constexpr uint32_t HALF = PW > 32 ? 32 : 16;  // largest power of two below PW (64, 32 or 21 items a wave)
  static_assert(PW > HALF && PW <= 2 * HALF, "one level must cover every item");
  static constexpr uint32_t LDS_WORDS = HALF * Jac<typename G::F>::WORDS;
  // every lane of the workgroup calls this; afterwards item 0 holds the sum of the live items' points
  PCD_DEV static void sum(Jac<F>& acc, uint32_t* lds, bool live, uint32_t it) {
    constexpr int JW = Jac<typename G::F>::WORDS;
    for (uint32_t s = HALF; s > 0; s >>= 1) {
      if (live && it >= s && it < 2 * s) acc.store(lds + (size_t)(it - s) * JW);
      __syncthreads();
      if (live && it < s && it + s < PW) acc = EC<GA>::add(acc, Jac<F>::load(lds + (size_t)it * JW));
      __syncthreads();
    }
  }
};

// The bodies of the three launches, shared by the single kernels (arguments in SGPRs) and the batched ones (arguments read from a
// descriptor table): every lane of a one-wave workgroup calls them, `tree` is the workgroup's MsmShortTree<G>::LDS_WORDS words of LDS.
//
// planes: plane b, workgroup `part` of `parts` of one MSM; err_parts / partial are that MSM's own words and rows
template <class G>
PCD_DEV void msm_short_planes_body(uint32_t* tree, const uint32_t* __restrict__ bases, uint32_t n_total, uint32_t offset, uint32_t groups,
                                   const uint32_t* __restrict__ inf_bits, const uint32_t* __restrict__ scalars, uint32_t n, uint32_t span,
                                   int scalar_bits, uint32_t* __restrict__ err_parts, uint32_t* __restrict__ partial, uint32_t b, uint32_t part,
                                   uint32_t parts) {
  typedef MsmShortTree<G> T;
  typedef typename T::IT IT;
  typedef typename T::GA GA;
  typedef typename T::F F;
  constexpr int NS = G::FR::N32;
  constexpr int JW = Jac<typename G::F>::WORDS;
  constexpr uint32_t PW = T::PW;
  if (b == 0) {
    // a scalar must be a reduced canonical value: the rule of the digit pass (msm_scalar_too_wide), applied to EVERY scalar of the call,
    // also those whose base is the point at infinity
    bool wide = false;
    for (uint32_t i = part * 64u + threadIdx.x; i < n; i += parts * 64u) {
      uint32_t s[NS];
#pragma unroll
      for (int k = 0; k < NS; k++) s[k] = scalars[(size_t)i * NS + k];
      wide |= msm_scalar_too_wide<NS>(s, scalar_bits);
    }
    const bool any = __ballot(wide) != 0ull;
    if (threadIdx.x == 0) err_parts[part] = any ? 1u : 0u;
  }
  const bool live = !IT::idle();
  const uint32_t it = IT::local();
  Jac<F> acc = Jac<F>::infinity();
  if (live) {
    const uint32_t total = n * groups;  // (n <= MSM_SHORT_MAX_N, groups <= the windows of a scalar: far below 2^32)
    for (uint32_t j = part * PW + it; j < total; j += parts * PW) {
      const uint32_t g = j / n, i = j - g * n;
      const uint32_t bit = span * g + b, word = bit >> 5;
      if (word >= (uint32_t)NS) continue;  // the last copy may cover positions past the scalar's top word
      if (!((scalars[(size_t)i * NS + word] >> (bit & 31u)) & 1u)) continue;
      if (msm_base_is_inf(inf_bits, offset + i)) continue;
      acc = EC<GA>::madd(acc, Aff<F>::load(bases + ((size_t)g * n_total + offset + i) * MsmBaseStride<G>::value));
    }
  }
  T::sum(acc, tree, live, it);
  if (live && it == 0) acc.store(partial + ((size_t)b * parts + part) * JW);
}

// fold: row[0] = sum over p < parts of row[p], `row` the partials of one plane of one MSM
template <class G>
PCD_DEV void msm_short_fold_body(uint32_t* tree, uint32_t* __restrict__ row, uint32_t parts) {
  typedef MsmShortTree<G> T;
  typedef typename T::IT IT;
  typedef typename T::GA GA;
  typedef typename T::F F;
  constexpr int JW = Jac<typename G::F>::WORDS;
  const bool live = !IT::idle();
  const uint32_t it = IT::local();
  Jac<F> acc = Jac<F>::infinity();
  if (live)
    for (uint32_t p = it; p < parts; p += T::PW) acc = EC<GA>::add(acc, Jac<F>::load(row + (size_t)p * JW));
  T::sum(acc, tree, live, it);  // (its first barrier stands between every item's reads of the row and the store below)
  if (live && it == 0) acc.store(row);
}

// combine: out = sum_b 2^b B_b with B_b at rows + b * row_stride_words; the rows are used as scratch.  *err_word = any of
// err_parts[0 .. parts), which is also what every lane gets back
template <class G>
PCD_DEV bool msm_short_combine_body(uint32_t* __restrict__ rows, size_t row_stride_words, uint32_t span, const uint32_t* err_parts, uint32_t parts,
                                    uint32_t* err_word, uint32_t* __restrict__ out) {
  typedef MsmItems<G> IT;
  typedef typename IT::GA GA;
  typedef typename GA::F F;
  typedef EC<GA> E;
  bool raised;
  {
    bool any = false;
    for (uint32_t p = threadIdx.x; p < parts; p += 64u) any |= err_parts[p] != 0u;
    raised = __ballot(any) != 0ull;
    if (threadIdx.x == 0) *err_word = raised ? 1u : 0u;
  }
  const bool live = !IT::idle();
  const uint32_t it = IT::local();
  const uint32_t w = (span + IT::PER_WAVE - 1) / IT::PER_WAVE;  // planes per item
  const uint32_t runs = (span + w - 1) / w;                      // <= PER_WAVE
  if (live && it < runs) {
    const uint32_t lo = it * w, hi = min(lo + w, span);
    Jac<F> c = Jac<F>::load(rows + (size_t)(hi - 1) * row_stride_words);
    for (uint32_t b = hi - 1; b-- > lo;) {
      c = E::dbl(c);
      c = E::add(c, Jac<F>::load(rows + (size_t)b * row_stride_words));
    }
    c.store(rows + (size_t)lo * row_stride_words);  // (row lo belongs to this item's run: nobody else reads it before the barrier)
  }
  __syncthreads();
  if (!live || it != 0) return raised;
  Jac<F> r = Jac<F>::load(rows + (size_t)(runs - 1) * w * row_stride_words);
  for (uint32_t j = runs - 1; j-- > 0;) {
    for (uint32_t d = 0; d < w; d++) r = E::dbl(r);
    r = E::add(r, Jac<F>::load(rows + (size_t)j * w * row_stride_words));
  }
  r.store(out);
  return raised;
}

template <class G>
__global__ void __launch_bounds__(64) msm_short_planes_kernel(const uint32_t* __restrict__ bases, uint32_t n_total, uint32_t offset, uint32_t groups,
                                                              const uint32_t* __restrict__ inf_bits, const uint32_t* __restrict__ scalars, uint32_t n,
                                                              uint32_t span, int scalar_bits, uint32_t* __restrict__ err_parts,
                                                              uint32_t* __restrict__ partial) {
  __shared__ uint32_t tree[MsmShortTree<G>::LDS_WORDS];
  msm_short_planes_body<G>(tree, bases, n_total, offset, groups, inf_bits, scalars, n, span, scalar_bits, err_parts, partial, blockIdx.x, blockIdx.y,
                           gridDim.y);
}

// partial[b * parts] = sum over p < parts of partial[b * parts + p]
template <class G>
__global__ void __launch_bounds__(64) msm_short_fold_kernel(uint32_t* __restrict__ partial, uint32_t parts) {
  __shared__ uint32_t tree[MsmShortTree<G>::LDS_WORDS];
  msm_short_fold_body<G>(tree, partial + (size_t)blockIdx.x * parts * Jac<typename G::F>::WORDS, parts);
}

// out = sum_b 2^b B_b with B_b at rows + b * row_stride_words; the rows are used as scratch.  err[0] = any of err[1 .. parts]
template <class G>
__global__ void __launch_bounds__(64) msm_short_combine_kernel(uint32_t* __restrict__ rows, size_t row_stride_words, uint32_t span,
                                                               uint32_t* __restrict__ err, uint32_t parts, uint32_t* __restrict__ out) {
  if (blockIdx.x != 0) return;
  (void)msm_short_combine_body<G>(rows, row_stride_words, span, err + 1, parts, err, out);
}

// scalars_dev: n canonical scalars; scratch: msm_short_plan(...).scratch_words u32 words; out_dev: one Jacobian point (device image).
// scratch[0] is the error word afterwards: non-zero when a scalar was not a reduced canonical value.  1 <= n <= MSM_SHORT_MAX_N.
template <class G>
hipError_t msm_short_run(hipStream_t st, const MsmBasesView& bv, const uint32_t* scalars_dev, uint32_t n, uint32_t* scratch, uint32_t* out_dev) {
  constexpr int JW = Jac<typename G::F>::WORDS;
  if (n == 0 || n > MSM_SHORT_MAX_N || (uint64_t)bv.offset + n > bv.n_total) return hipErrorInvalidValue;
  const MsmShortPlan pl = msm_short_plan<G>(bv, n);
  uint32_t* partial = scratch + pl.err_words;
  hipLaunchKernelGGL((msm_short_planes_kernel<G>), dim3(pl.span, pl.parts), dim3(64), 0, st, bv.dptr, bv.n_total, bv.offset, (uint32_t)bv.groups,
                     bv.inf_bits, scalars_dev, n, pl.span, (int)G::FR::BITS, scratch + 1, partial);
  PCD_HIP_TRY(hipGetLastError());
  if (pl.parts > 1) {
    hipLaunchKernelGGL((msm_short_fold_kernel<G>), dim3(pl.span), dim3(64), 0, st, partial, pl.parts);
    PCD_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL((msm_short_combine_kernel<G>), dim3(1), dim3(64), 0, st, partial, (size_t)pl.parts * JW, pl.span, scratch, pl.parts, out_dev);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- the batched form
// k independent short MSMs over ONE resident vector as one chain of at most three launches: what a commit round's hiding MSMs are (two
// coefficients each, a dozen of them).  One after the other they cost k serial combine chains on one wave each; side by side they cost one.
// `span` depends on the handle alone, so it is the same for every MSM of the call -- which is why a call takes one handle.  The kernels
// are the bodies above behind a descriptor table in device memory, one entry per MSM with n > 0; the entry's index is uniform over the
// workgroup, so the table is read by scalar loads.  Grids (64 lanes, no workgroup waits for another):
//   planes   (P, span), P = the sum of the MSMs' own `parts`: a part -> entry list gives workgroup x its MSM.  (Parts on x, planes on y:
//            y is capped at 65535 and P is not.)  Never k x max parts: one 1024-pair MSM next to 63 two-pair ones gets 13 + 63 parts.
//   fold     (entries with parts > 1, span), launched only when there is such an entry
//   combine  (entries): one wave per MSM
// An MSM with n == 0 owns no entry, no workgroup and no scratch, and its result slot is NOT written by these launches: the caller zeroes it
// beforehand (all-zero words are the identity, Z = 0).
struct MsmShortBatchIn {     // one MSM of the call, as the host states it
  const uint32_t* scalars;   // its n canonical scalars (device memory)
  uint32_t offset;           // its first base
  uint32_t n;                // pairs, 0 .. MSM_SHORT_MAX_N
  uint32_t out_slot;         // its Jacobian point goes to out + out_slot * out_stride_words
};
struct MsmShortBatchItem {   // one table entry (device memory; 32 bytes)
  const uint32_t* scalars;
  uint32_t offset, n;
  uint32_t part0, parts;     // its workgroups of a plane are part0 .. part0 + parts - 1 of the call's P
  uint32_t row0;             // its span * parts partial rows start at Jacobian point row0 of the row area: row (b, p) is row0 + b * parts + p
  uint32_t out_slot;
};
static_assert(sizeof(MsmShortBatchItem) == 32, "the table is staged as u32 words");

// Scratch of a call, in u32 words: the error words -- [0] the call's, [1 .. 1 + entries) one per entry, then one per part -- | the table:
// entries, the part -> entry list, the list of entries to fold (staged from `table` by one copy) | the rows: span * P Jacobian points.
struct MsmShortBatchPlan {
  uint32_t span = 0, entries = 0, parts = 0, folds = 0;  // parts: P
  size_t err_words = 0, table_words = 0, scratch_words = 0;
  std::vector<uint32_t> table;                           // table_words words: the host image of the middle section
  size_t part_item_off() const { return (size_t)entries * (sizeof(MsmShortBatchItem) / 4); }  // (words from the table's start)
  size_t fold_item_off() const { return part_item_off() + parts; }
};
template <class G>
MsmShortBatchPlan msm_short_batch_plan(const MsmBasesView& bv, const MsmShortBatchIn* items, size_t k) {
  MsmShortBatchPlan pl;
  pl.span = msm_short_plan<G>(bv, 1).span;
  std::vector<MsmShortBatchItem> ent;
  std::vector<uint32_t> part_item, fold_item;
  uint64_t parts = 0;
  for (size_t j = 0; j < k; j++) {
    if (items[j].n == 0) continue;
    const uint32_t pj = msm_short_plan<G>(bv, items[j].n).parts;
    const uint32_t e = (uint32_t)ent.size();
    ent.push_back({items[j].scalars, items[j].offset, items[j].n, (uint32_t)parts, pj, (uint32_t)(parts * pl.span), items[j].out_slot});
    part_item.insert(part_item.end(), pj, e);
    if (pj > 1) fold_item.push_back(e);
    parts += pj;
  }
  pl.entries = (uint32_t)ent.size();
  pl.parts = (uint32_t)parts;
  pl.folds = (uint32_t)fold_item.size();
  pl.err_words = ((size_t)1 + pl.entries + pl.parts + 3) & ~(size_t)3;
  pl.table_words = (pl.fold_item_off() + pl.folds + 3) & ~(size_t)3;
  pl.scratch_words = pl.err_words + pl.table_words + (size_t)pl.span * pl.parts * Jac<typename G::F>::WORDS;
  pl.table.assign(pl.table_words, 0u);
  if (pl.entries) memcpy(pl.table.data(), ent.data(), ent.size() * sizeof(MsmShortBatchItem));
  if (pl.parts) memcpy(pl.table.data() + pl.part_item_off(), part_item.data(), part_item.size() * 4);
  if (pl.folds) memcpy(pl.table.data() + pl.fold_item_off(), fold_item.data(), fold_item.size() * 4);
  return pl;
}

template <class G>
__global__ void __launch_bounds__(64) msm_short_batch_planes_kernel(const uint32_t* __restrict__ bases, uint32_t n_total, uint32_t groups,
                                                                    const uint32_t* __restrict__ inf_bits, const MsmShortBatchItem* __restrict__ table,
                                                                    const uint32_t* __restrict__ part_item, uint32_t span, int scalar_bits,
                                                                    uint32_t* __restrict__ err, uint32_t* __restrict__ err_parts,
                                                                    uint32_t* __restrict__ rows) {
  __shared__ uint32_t tree[MsmShortTree<G>::LDS_WORDS];
  const uint32_t x = blockIdx.x, b = blockIdx.y;
  const MsmShortBatchItem e = table[part_item[x]];
  if (x == 0 && b == 0 && threadIdx.x == 0) err[0] = 0u;  // the call's word: raised by the combine launch, behind this one on the stream
  msm_short_planes_body<G>(tree, bases, n_total, e.offset, groups, inf_bits, e.scalars, e.n, span, scalar_bits, err_parts + e.part0,
                           rows + (size_t)e.row0 * Jac<typename G::F>::WORDS, b, x - e.part0, e.parts);
}

template <class G>
__global__ void __launch_bounds__(64) msm_short_batch_fold_kernel(const MsmShortBatchItem* __restrict__ table, const uint32_t* __restrict__ fold_item,
                                                                  uint32_t* __restrict__ rows) {
  __shared__ uint32_t tree[MsmShortTree<G>::LDS_WORDS];
  const MsmShortBatchItem e = table[fold_item[blockIdx.x]];
  msm_short_fold_body<G>(tree, rows + ((size_t)e.row0 + (size_t)blockIdx.y * e.parts) * Jac<typename G::F>::WORDS, e.parts);
}

// err_items[j] = entry j's error word; err[0] is raised when any entry's is (every raising workgroup stores the same 1)
template <class G>
__global__ void __launch_bounds__(64) msm_short_batch_combine_kernel(const MsmShortBatchItem* __restrict__ table, uint32_t* __restrict__ rows,
                                                                     uint32_t span, uint32_t* __restrict__ err, uint32_t* __restrict__ err_items,
                                                                     const uint32_t* __restrict__ err_parts, uint32_t* __restrict__ out,
                                                                     size_t out_stride_words) {
  constexpr int JW = Jac<typename G::F>::WORDS;
  const MsmShortBatchItem e = table[blockIdx.x];
  const bool raised = msm_short_combine_body<G>(rows + (size_t)e.row0 * JW, (size_t)e.parts * JW, span, err_parts + e.part0, e.parts,
                                                err_items + blockIdx.x, out + (size_t)e.out_slot * out_stride_words);
  if (raised && threadIdx.x == 0) err[0] = 1u;
}

// scratch: msm_short_batch_plan(...).scratch_words u32 words (device); *table_host receives the table's host image, which the staging copy
// reads: it must stay as it is until that copy has run.  bv: the view at offset 0.  *launches = kernels launched: 0 (no MSM with n > 0:
// nothing is touched, scratch[0] included), 2 or 3.
template <class G>
hipError_t msm_short_batch_run(hipStream_t st, const MsmBasesView& bv, const MsmShortBatchIn* items, size_t k, uint32_t* scratch,
                               std::vector<uint32_t>* table_host, uint32_t* out_dev, size_t out_stride_words, uint32_t* launches) {
  *launches = 0;
  if (bv.offset != 0) return hipErrorInvalidValue;
  for (size_t j = 0; j < k; j++)
    if (items[j].n > MSM_SHORT_MAX_N || (uint64_t)items[j].offset + items[j].n > bv.n_total) return hipErrorInvalidValue;
  MsmShortBatchPlan pl = msm_short_batch_plan<G>(bv, items, k);
  if (pl.entries == 0) return hipSuccess;
  if ((uint64_t)pl.span * pl.parts >= (1ull << 32)) return hipErrorInvalidValue;  // (row0 is a 32-bit count of points)
  table_host->swap(pl.table);
  uint32_t* err_items = scratch + 1;
  uint32_t* err_parts = err_items + pl.entries;
  uint32_t* table_dev = scratch + pl.err_words;
  uint32_t* rows = table_dev + pl.table_words;
  const MsmShortBatchItem* table = (const MsmShortBatchItem*)table_dev;
  PCD_HIP_TRY(hipMemcpyAsync(table_dev, table_host->data(), pl.table_words * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL((msm_short_batch_planes_kernel<G>), dim3(pl.parts, pl.span), dim3(64), 0, st, bv.dptr, bv.n_total, (uint32_t)bv.groups, bv.inf_bits,
                     table, table_dev + pl.part_item_off(), pl.span, (int)G::FR::BITS, scratch, err_parts, rows);
  PCD_HIP_TRY(hipGetLastError());
  ++*launches;
  if (pl.folds) {
    hipLaunchKernelGGL((msm_short_batch_fold_kernel<G>), dim3(pl.folds, pl.span), dim3(64), 0, st, table, table_dev + pl.fold_item_off(), rows);
    PCD_HIP_TRY(hipGetLastError());
    ++*launches;
  }
  hipLaunchKernelGGL((msm_short_batch_combine_kernel<G>), dim3(pl.entries), dim3(64), 0, st, table, rows, pl.span, scratch, err_items, err_parts, out_dev,
                     out_stride_words);
  PCD_HIP_TRY(hipGetLastError());
  ++*launches;
  return hipSuccess;
}

}  // namespace pcd
