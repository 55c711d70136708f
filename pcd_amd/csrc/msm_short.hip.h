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
#pragma once
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

template <class G>
__global__ void __launch_bounds__(64) msm_short_planes_kernel(const uint32_t* __restrict__ bases, uint32_t n_total, uint32_t offset, uint32_t groups,
                                                              const uint32_t* __restrict__ inf_bits, const uint32_t* __restrict__ scalars, uint32_t n,
                                                              uint32_t span, int scalar_bits, uint32_t* __restrict__ err_parts,
                                                              uint32_t* __restrict__ partial) {
  typedef MsmShortTree<G> T;
  typedef typename T::IT IT;
  typedef typename T::GA GA;
  typedef typename T::F F;
  constexpr int NS = G::FR::N32;
  constexpr int JW = Jac<typename G::F>::WORDS;
  constexpr uint32_t PW = T::PW;
  __shared__ uint32_t tree[T::LDS_WORDS];
  const uint32_t b = blockIdx.x, part = blockIdx.y, parts = gridDim.y;
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

// partial[b * parts] = sum over p < parts of partial[b * parts + p]
template <class G>
__global__ void __launch_bounds__(64) msm_short_fold_kernel(uint32_t* __restrict__ partial, uint32_t parts) {
  typedef MsmShortTree<G> T;
  typedef typename T::IT IT;
  typedef typename T::GA GA;
  typedef typename T::F F;
  constexpr int JW = Jac<typename G::F>::WORDS;
  __shared__ uint32_t tree[T::LDS_WORDS];
  uint32_t* row = partial + (size_t)blockIdx.x * parts * JW;
  const bool live = !IT::idle();
  const uint32_t it = IT::local();
  Jac<F> acc = Jac<F>::infinity();
  if (live)
    for (uint32_t p = it; p < parts; p += T::PW) acc = EC<GA>::add(acc, Jac<F>::load(row + (size_t)p * JW));
  T::sum(acc, tree, live, it);  // (its first barrier stands between every item's reads of the row and the store below)
  if (live && it == 0) acc.store(row);
}

// out = sum_b 2^b B_b with B_b at rows + b * row_stride_words; the rows are used as scratch.  err[0] = any of err[1 .. parts]
template <class G>
__global__ void __launch_bounds__(64) msm_short_combine_kernel(uint32_t* __restrict__ rows, size_t row_stride_words, uint32_t span,
                                                               uint32_t* __restrict__ err, uint32_t parts, uint32_t* __restrict__ out) {
  typedef MsmItems<G> IT;
  typedef typename IT::GA GA;
  typedef typename GA::F F;
  typedef EC<GA> E;
  if (blockIdx.x != 0) return;
  {
    bool any = false;
    for (uint32_t p = threadIdx.x; p < parts; p += 64u) any |= err[1 + p] != 0u;
    const bool raised = __ballot(any) != 0ull;
    if (threadIdx.x == 0) err[0] = raised ? 1u : 0u;
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
  if (!live || it != 0) return;
  Jac<F> r = Jac<F>::load(rows + (size_t)(runs - 1) * w * row_stride_words);
  for (uint32_t j = runs - 1; j-- > 0;) {
    for (uint32_t d = 0; d < w; d++) r = E::dbl(r);
    r = E::add(r, Jac<F>::load(rows + (size_t)j * w * row_stride_words));
  }
  r.store(out);
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

}  // namespace pcd
