// K7, the open side of KZG10 / MarlinKZG10 (ark-poly-commit `KZG10::open`, `MarlinKZG10::open`): division of a polynomial by
// (X - z), evaluation of k polynomials at one point, and the linear combination of k polynomials, on gfx950.
//
// Coefficients are C-ABI Montgomery words (x R, R = 2^(32 ABI_WORDS)), low degree first, as in a pcdhip_buf.  The kernels never
// convert them: unpack32 reads x R as a plain integer, and since every step below is LINEAR in the coefficients (only the point z,
// brought into the device image once per lane, enters a product), the results come out scaled by the same R -- pack32 of the
// canonical representative IS the ABI image of the result.  A coefficient costs its Horner product and nothing else; the canonical
// words the MSM wants (x itself) cost one product more, fused into the store.
//
// Division.  p(X) = q(X)(X - z) + v with h_i = sum_{j >= i} p_j z^(j - i): h_i = p_i + z h_(i+1), q_(i-1) = h_i, v = h_0.
// A suffix scan with a constant multiplier, in three stream-ordered launches (no inter-workgroup waiting):
//   1. poly_tile_eval   -- every tile of TILE = B x E coefficients reduces to T_k = sum_j p_(lo_k + j) z^j;
//   2. poly_carry_scan  -- one workgroup scans the T_k with the multiplier z^TILE: the carry-in C_k = h at the tile's end, and v;
//   3. poly_div_tile    -- every tile again, from its carry-in: q.
// Inside a tile a lane owns E consecutive coefficients (a local Horner), the B lanes combine (value, multiplier) pairs over log2(B)
// steps whose multiplier is the same power of z in every lane (it squares once per step).  Tiles are staged through LDS, so the
// global reads (and the shifted-by-one quotient stores) are contiguous word streams.
#pragma once
#include "ec.hip.h"

namespace pcd {

template <class F>
struct PolyAbiElt { uint32_t w[F::ABI_WORDS]; };

// B lanes, E coefficients per lane (PolyCfg<F>::B, ::E): 298-bit tiles of 1024 (LDS 40 + 11 KB), 753-bit tiles of 512 (48 + 14 KB)
template <class F>
struct PolyCfg {
  static constexpr int B = F::N <= 11 ? 256 : 128;
  static constexpr int E = 4;
  static constexpr uint32_t TILE = (uint32_t)B * E;
  static constexpr int CB = 256;  // lanes of the carry scan
};

// stage `cnt` elements (ABI words) starting at element `lo` of p into LDS, zeros up to the tile's end
template <class F, int B>
PCD_DEV void poly_stage_in(const uint32_t* __restrict__ p, uint64_t lo, uint32_t cnt, uint32_t tile, uint32_t* st) {
  constexpr int AW = F::ABI_WORDS;
  const uint32_t words = cnt * AW;
  const uint32_t* src = p + lo * AW;
  for (uint32_t w = threadIdx.x; w < tile * AW; w += B) st[w] = w < words ? src[w] : 0u;
}

// tree reduction over the B lanes of (h, segment multiplier m): lane 0 ends with sum_t h_t m^t; m ends as m^B
template <class F, int B>
PCD_DEV F poly_block_reduce(F h, F& m, uint32_t* red) {
  const uint32_t t = threadIdx.x;
  for (int d = 1; d < B; d <<= 1) {
    if ((t & (2 * d - 1)) == (uint32_t)d) h.store(red + (size_t)t * F::WORDS);
    __syncthreads();
    if ((t & (2 * d - 1)) == 0) h = h + m * F::load(red + (size_t)(t + d) * F::WORDS);
    __syncthreads();
    m = m.sqr();
  }
  return h;
}

// inclusive suffix scan: lane t ends with sum_{u >= t} h_u m^(u - t)
template <class F, int B>
PCD_DEV F poly_block_suffix_scan(F h, F m, uint32_t* red) {
  const uint32_t t = threadIdx.x;
  for (int d = 1; d < B; d <<= 1) {
    h.store(red + (size_t)t * F::WORDS);
    __syncthreads();
    if (t + d < (uint32_t)B) h = h + m * F::load(red + (size_t)(t + d) * F::WORDS);
    __syncthreads();
    if (2 * d < B) m = m.sqr();
  }
  return h;
}

// local Horner over a lane's E staged coefficients: h <- sum_e p_e z^e + z^E h
template <class F, int E>
PCD_DEV F poly_lane_horner(const uint32_t* st, F h, bool h_zero, const F& z) {
  constexpr int AW = F::ABI_WORDS;
  const uint32_t base = threadIdx.x * E;
#pragma unroll 1
  for (int e = E - 1; e >= 0; e--) {
    const F x = F::unpack32(st + (size_t)(base + e) * AW);
    h = (h_zero && e == E - 1) ? x : x + z * h;
  }
  return h;
}

// phase 1, batched over the polynomials of `descs` (blockIdx.y): tiles[y * tiles_stride + k] = T_k (device image).  Block (0, 0)
// also leaves z^TILE in zt for the carry scan.
template <class F>
__global__ void __launch_bounds__(PolyCfg<F>::B) poly_tile_eval(const PolyDesc* __restrict__ descs, const PolyAbiElt<F> z_abi,
                                                                uint32_t* __restrict__ tiles, uint32_t tiles_stride, uint32_t* __restrict__ zt) {
  constexpr int B = PolyCfg<F>::B, E = PolyCfg<F>::E;
  constexpr uint32_t TILE = PolyCfg<F>::TILE;
  __shared__ __attribute__((aligned(16))) uint32_t st[TILE * F::ABI_WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t red[B * F::WORDS];
  const PolyDesc d = descs[blockIdx.y];
  const uint64_t lo = (uint64_t)blockIdx.x * TILE;
  if (blockIdx.x > 0 && lo >= d.len) return;  // (whole workgroup; tile 0 of an empty polynomial runs and yields 0)
  const uint32_t cnt = lo >= d.len ? 0u : (uint32_t)(d.len - lo < TILE ? d.len - lo : TILE);
  poly_stage_in<F, B>(d.p, lo, cnt, TILE, st);
  const F z = F::from_abi(z_abi.w);
  F m = z;
#pragma unroll
  for (int e = 1; e < E; e++) m = m * z;  // z^E
  __syncthreads();
  F h = poly_lane_horner<F, E>(st, F::zero(), true, z);
  h = poly_block_reduce<F, B>(h, m, red);
  if (threadIdx.x == 0) {
    h.store(tiles + ((size_t)blockIdx.y * tiles_stride + blockIdx.x) * F::WORDS);
    if (blockIdx.x == 0 && blockIdx.y == 0) m.store(zt);  // m = (z^E)^B
  }
}

// phase 2, one workgroup per polynomial: lane t owns the tiles [t c, t c + c) (c = ceil(K / CB)), a Horner in Z = z^TILE from the
// top, a suffix scan of the lanes with Z^c, then the walk down that writes the carry-in of every tile (carries may be null) and,
// from lane 0, v = h_0 as an ABI Montgomery element.
template <class F>
__global__ void __launch_bounds__(PolyCfg<F>::CB) poly_carry_scan(const PolyDesc* __restrict__ descs, const uint32_t* __restrict__ tiles,
                                                                  uint32_t tiles_stride, const uint32_t* __restrict__ zt,
                                                                  uint32_t* __restrict__ carries, uint32_t* __restrict__ values_abi) {
  constexpr int CB = PolyCfg<F>::CB;
  constexpr uint32_t TILE = PolyCfg<F>::TILE;
  __shared__ __attribute__((aligned(16))) uint32_t red[CB * F::WORDS];
  const PolyDesc d = descs[blockIdx.y];
  const uint32_t K = (uint32_t)((d.len + TILE - 1) / TILE);
  const uint32_t c = (K + CB - 1) / CB;
  const uint32_t lo = min(K, threadIdx.x * c), hi = min(K, lo + c);
  const uint32_t* T = tiles + (size_t)blockIdx.y * tiles_stride * F::WORDS;
  const F Z = K > 1 ? F::load(zt) : F::one();
  F h = F::zero();
  for (uint32_t k = hi; k-- > lo;) h = F::load(T + (size_t)k * F::WORDS) + Z * h;
  h = poly_block_suffix_scan<F, CB>(h, Z.pow_u64(c), red);
  h.store(red + (size_t)threadIdx.x * F::WORDS);  // (the scan ends on a barrier behind its last reads of red)
  __syncthreads();
  F cin = threadIdx.x + 1 < (uint32_t)CB ? F::load(red + (size_t)(threadIdx.x + 1) * F::WORDS) : F::zero();
  for (uint32_t k = hi; k-- > lo;) {
    if (carries) cin.store(carries + ((size_t)blockIdx.y * tiles_stride + k) * F::WORDS);
    cin = F::load(T + (size_t)k * F::WORDS) + Z * cin;
  }
  if (threadIdx.x == 0) cin.canonical().pack32(values_abi + (size_t)blockIdx.y * F::ABI_WORDS);
}

// phase 3 (one polynomial): every tile from its carry-in; q_(i-1) = h_i for the tile's i >= 1, as ABI Montgomery words or, with
// CANON, as canonical words (x = (x R) (R' / R) / R': one product with the constant cin * 1).
template <class F, bool CANON>
__global__ void __launch_bounds__(PolyCfg<F>::B) poly_div_tile(const uint32_t* __restrict__ p, uint64_t len, const PolyAbiElt<F> z_abi,
                                                               const uint32_t* __restrict__ carries, uint32_t* __restrict__ q) {
  constexpr int B = PolyCfg<F>::B, E = PolyCfg<F>::E, AW = F::ABI_WORDS;
  constexpr uint32_t TILE = PolyCfg<F>::TILE;
  __shared__ __attribute__((aligned(16))) uint32_t st[TILE * AW];
  __shared__ __attribute__((aligned(16))) uint32_t red[B * F::WORDS];
  const uint64_t lo = (uint64_t)blockIdx.x * TILE;
  const uint32_t cnt = (uint32_t)(len - lo < TILE ? len - lo : TILE);
  poly_stage_in<F, B>(p, lo, cnt, TILE, st);
  const F z = F::from_abi(z_abi.w);
  F m = z;
#pragma unroll
  for (int e = 1; e < E; e++) m = m * z;
  const F C = F::load(carries + (size_t)blockIdx.x * F::WORDS);
  const bool top = threadIdx.x == B - 1;
  __syncthreads();
  F h = poly_lane_horner<F, E>(st, top ? C : F::zero(), !top, z);
  h = poly_block_suffix_scan<F, B>(h, m, red);
  h.store(red + (size_t)threadIdx.x * F::WORDS);  // (every lane is past the scan's last barrier, which ended all reads of red)
  __syncthreads();
  F hin = top ? C : F::load(red + (size_t)(threadIdx.x + 1) * F::WORDS);
  F kc = F::zero();
  if constexpr (CANON) {
    F cin, one_raw = F::zero();
#pragma unroll
    for (int i = 0; i < F::N; i++) cin.v[i] = F::Params::cin(i);
    one_raw.v[0] = 1;
    kc = cin * one_raw;
  }
  const uint32_t base = threadIdx.x * E;
#pragma unroll 1
  for (int e = E - 1; e >= 0; e--) {
    uint32_t* s = st + (size_t)(base + e) * AW;
    hin = F::unpack32(s) + z * hin;
    if constexpr (CANON) (hin * kc).canonical().pack32(s);
    else hin.canonical().pack32(s);
  }
  __syncthreads();
  // element lo + i lands at q[lo + i - 1]: one contiguous run of words from q + (lo - 1) AW (element 0 of the polynomial is v)
  const uint32_t skip = lo == 0 ? AW : 0;
  for (uint32_t w = threadIdx.x + skip; w < cnt * AW; w += B) q[lo * AW + w - AW] = st[w];
}

// out_i = sum_j c_j p_(j,i), i < n_out (an input shorter than i + 1 contributes nothing); ABI Montgomery in and out.  The k
// coefficients enter the device image once per workgroup, through LDS, B at a time.  out may alias an input.
template <class F>
__global__ void __launch_bounds__(256) poly_lincomb(const PolyDesc* __restrict__ descs, const uint32_t* __restrict__ coeffs_abi,
                                                    uint32_t k, uint64_t n_out, uint32_t* out) {
  constexpr int B = 256, AW = F::ABI_WORDS;
  __shared__ __attribute__((aligned(16))) uint32_t cs[B * F::WORDS];
  const uint64_t i = (uint64_t)blockIdx.x * B + threadIdx.x;
  F acc = F::zero();
  for (uint32_t j0 = 0; j0 < k; j0 += B) {
    __syncthreads();
    if (j0 + threadIdx.x < k) F::from_abi(coeffs_abi + (size_t)(j0 + threadIdx.x) * AW).store(cs + (size_t)threadIdx.x * F::WORDS);
    __syncthreads();
    const uint32_t je = min(k, j0 + B);
    for (uint32_t j = j0; j < je; j++) {
      const PolyDesc d = descs[j];
      if (i < d.len) acc = acc + F::load(cs + (size_t)(j - j0) * F::WORDS) * F::unpack32(d.p + i * AW);
    }
  }
  if (i < n_out) acc.canonical().pack32(out + i * AW);
}

// ---- K7 commit side (ark-poly-commit `KZG10::commit`): the canonical scalars of k polynomials for their MSMs, and their trimmed lengths.
// One lane per coefficient, one polynomial per blockIdx.y.  x = (x R) (R' / R) / R' is one product with the constant kc = cin * 1 (as in
// poly_div_tile<F, true>), which the host forms once and passes by value.  Coefficients at i >= cap are reduced and inspected only: they
// have no base, but they still count for the trimmed length, from which the caller makes its size checks after the fact.  Nothing at
// i >= len is read.  trimmed[y] is raised by one atomicMax per workgroup that holds a non-zero coefficient.
constexpr int POLY_COMMIT_B = 256;
template <class F>
__global__ void __launch_bounds__(POLY_COMMIT_B) poly_commit_scalars(const PolyCommitDesc* __restrict__ descs, const F kc,
                                                                     uint32_t* __restrict__ trimmed) {
  constexpr int B = POLY_COMMIT_B, AW = F::ABI_WORDS;
  __shared__ uint32_t top;
  const PolyCommitDesc d = descs[blockIdx.y];
  const uint64_t lo = (uint64_t)blockIdx.x * B;
  if (lo >= d.len) return;  // (whole workgroup)
  if (threadIdx.x == 0) top = 0;
  __syncthreads();
  const uint64_t i = lo + threadIdx.x;
  uint32_t mine = 0;
  if (i < d.len) {
    const F x = (F::unpack32(d.p + i * AW) * kc).canonical();
    if (!x.is_raw_zero()) mine = (uint32_t)i + 1;
    if (i < d.cap) x.pack32(d.out + i * AW);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mine = max(mine, (uint32_t)__shfl_xor((int)mine, s, 64));
  if ((threadIdx.x & 63) == 0 && mine) atomicMax(&top, mine);
  __syncthreads();
  if (threadIdx.x == 0 && top) atomicMax(trimmed + blockIdx.y, top);
}

// ---- K8, vector algebra for Marlin's AHP rounds: batch inversion (ark-ff `batch_inversion[_and_mul]`), the pointwise product, division
// by the vanishing polynomial X^n - 1 (ark-poly `divide_by_vanishing_poly`).  ABI Montgomery words in and out, as above.
//
// Batch inversion: Montgomery's trick at two levels.  A tile of B x E elements is staged through LDS; a lane owns E consecutive
// elements, replaces zeros by one (remembered in a bit mask), and leaves its running products P_k = x_0 .. x_k in the slots of the
// x_k.  The lane products are inverted -- one inv_gcd per lane (LANE_INV), or one per workgroup over a prefix and a suffix product scan
// of the lanes -- and the walk back down turns slot k into inv * P_(k-1) and inv into inv * x_k, with x_k read again from `in` (the lines
// the workgroup has just staged; nothing of the tile is stored before the walk has ended, so out may be in).  3 (E - 1) products per
// lane besides the inversion's share.
// The R factors: unpack32 reads x R as the device image of x rho, rho = R / R'.  P_k carries rho^(k+1), the inverse of the lane product
// rho^-E, so inv * P_(k-1) is the device image of x_k^-1 / rho: the integer x_k^-1 R'^2 / R.  The constant K = scale R^2 / R' folded
// into the lane inverse once (unpack32(scale R) * cout, cout = R; cout * cout without a scale) makes that scale x_k^-1 R, the ABI image.
#ifndef PCD_BINV_LANE_INV
#define PCD_BINV_LANE_INV 1
#endif
template <class F, bool LANE_INV = (PCD_BINV_LANE_INV != 0)>
struct BinvCfg {  // LDS: the tile in ABI words + one pad word per lane (+ B elements for the scans)
  static constexpr int B = LANE_INV ? 64 : 128;
  static constexpr int E = LANE_INV ? (F::N <= 11 ? 16 : 8) : (F::N <= 11 ? 8 : 4);
  static constexpr uint32_t TILE = (uint32_t)B * E;
};

template <class F, bool LANE_INV>
__global__ void __launch_bounds__((BinvCfg<F, LANE_INV>::B)) poly_batch_inv_tile(const uint32_t* in, uint64_t n, const PolyAbiElt<F> scale_abi,
                                                                               int has_scale, uint32_t* out) {
  typedef BinvCfg<F, LANE_INV> Cfg;
  constexpr int B = Cfg::B, E = Cfg::E, AW = F::ABI_WORDS;
  constexpr uint32_t TILE = Cfg::TILE, CHUNK = (uint32_t)E * AW;  // a lane's chunk starts at t (CHUNK + 1): odd stride, no bank shared
  __shared__ __attribute__((aligned(16))) uint32_t st[TILE * AW + B];
  __shared__ __attribute__((aligned(16))) uint32_t red[LANE_INV ? 1 : B * F::WORDS];
  const uint32_t t = threadIdx.x;
  const uint64_t lo = (uint64_t)blockIdx.x * TILE;
  const uint32_t cnt = (uint32_t)(n - lo < TILE ? n - lo : TILE);
  const uint32_t* src = in + lo * AW;
  for (uint32_t w = t; w < TILE * AW; w += B) st[w + w / CHUNK] = w < cnt * AW ? src[w] : 0u;
  F cout;
#pragma unroll
  for (int i = 0; i < F::N; i++) cout.v[i] = F::Params::cout(i);
  const F K = (has_scale ? F::unpack32(scale_abi.w) : cout) * cout;
  __syncthreads();
  uint32_t* mine = st + (size_t)t * (CHUNK + 1);
  uint32_t zmask = 0;
  F run = F::one();
#pragma unroll 1
  for (int k = 0; k < E; k++) {
    uint32_t* s = mine + k * AW;
    F x = F::unpack32(s);
    if (x.is_zero()) { zmask |= 1u << k; x = F::one(); }
    run = k == 0 ? x : run * x;
    run.canonical().pack32(s);
  }
  F inv;
  if constexpr (LANE_INV) {
    inv = run.inv() * K;
  } else {
    // 1 / L_t = (1 / total) * (L_0 .. L_(t-1)) * (L_(t+1) .. L_(B-1)): an inclusive prefix and an inclusive suffix product scan of the
    // lanes through the one array, each lane keeping its neighbour's value
    F pre = run, suf = run;
    for (int d = 1; d < B; d <<= 1) {
      pre.store(red + (size_t)t * F::WORDS);
      __syncthreads();
      if (t >= (uint32_t)d) pre = pre * F::load(red + (size_t)(t - d) * F::WORDS);
      __syncthreads();
    }
    pre.store(red + (size_t)t * F::WORDS);
    __syncthreads();
    const F below = t > 0 ? F::load(red + (size_t)(t - 1) * F::WORDS) : F::one();
    __syncthreads();
    for (int d = 1; d < B; d <<= 1) {
      suf.store(red + (size_t)t * F::WORDS);
      __syncthreads();
      if (t + d < (uint32_t)B) suf = suf * F::load(red + (size_t)(t + d) * F::WORDS);
      __syncthreads();
    }
    suf.store(red + (size_t)t * F::WORDS);
    __syncthreads();
    const F above = t + 1 < (uint32_t)B ? F::load(red + (size_t)(t + 1) * F::WORDS) : F::one();
    __syncthreads();
    if (t == B - 1) (pre.inv() * K).store(red);
    __syncthreads();
    inv = F::load(red) * below * above;
  }
  const uint32_t* again = src + (size_t)t * CHUNK;
#pragma unroll 1
  for (int k = E - 1; k >= 0; k--) {
    uint32_t* s = mine + k * AW;
    const bool z = (zmask >> k) & 1u;  // (a zero, or the padding behind the vector's end: never read again)
    const F y = k > 0 ? inv * F::unpack32(s - AW) : inv;
    if (k > 0) inv = inv * (z ? F::one() : F::unpack32(again + k * AW));
    (z ? F::zero() : y.canonical()).pack32(s);
  }
  __syncthreads();
  uint32_t* dst = out + lo * AW;
  for (uint32_t w = t; w < cnt * AW; w += B) dst[w] = st[w + w / CHUNK];
}

// out_i = a_i b_i, i < n.  ABI: from_abi puts one operand into the device image, the other is read as it stands (b R), so the product is
// a b R, the ABI image.  !ABI: device image in and out (the pointwise step of the polynomial product, between its transforms).
template <class F, bool ABI>
__global__ void __launch_bounds__(256) poly_vec_mul(const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if constexpr (ABI) (F::from_abi(a + i * F::ABI_WORDS) * F::unpack32(b + i * F::ABI_WORDS)).canonical().pack32(out + i * F::ABI_WORDS);
  else (F::load(a + i * F::WORDS) * F::load(b + i * F::WORDS)).store(out + i * F::WORDS);
}

// p = q (X^n - 1) + r: q_j = sum_{i >= 1, j + i n < len} p_(j + i n) for j < q_len = len - n, r_j = p_j + q_j for j < min(len, n)
// (r may be null).  Lane j walks its column with stride n: one streaming pass for len <= a few n, len / n terms per lane in general.
template <class F>
__global__ void __launch_bounds__(256) poly_div_vanishing(const uint32_t* __restrict__ p, uint64_t len, uint64_t n, uint32_t* __restrict__ q,
                                                          uint32_t* __restrict__ r) {
  constexpr int AW = F::ABI_WORDS;
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t q_len = len > n ? len - n : 0, r_len = len < n ? len : n;
  if (j >= q_len && j >= r_len) return;
  F acc = F::zero();
  for (uint64_t i = j + n; i < len; i += n) acc = acc + F::unpack32(p + i * AW);
  if (j < q_len) acc.canonical().pack32(q + j * AW);
  if (r && j < r_len) (acc + F::unpack32(p + j * AW)).canonical().pack32(r + j * AW);
}

// ---- K13, a round's openings (MarlinKZG10 `open_combinations` / `batch_open`): the three launches of the division above, batched over
// PARTS (common.h PolyOpenPart), every part with its own terms, point, output slice and store scale.  grid (tiles of the longest part,
// parts); a workgroup whose tile lies beyond its part's len leaves at once (whole workgroup).
//
// Launch 1 forms the part's tile in LDS as the linear combination of its terms and reduces it to T_k as poly_tile_eval does.  The B lanes
// take the tile in E rounds of B consecutive elements: per round one accumulator per lane, and per term one contiguous run of B elements
// staged through `sub` (which shares its storage with the reduction's `red`: the two are never live together).  The coefficients enter the
// device image CS at a time through `cs`; a part of at most CS terms converts them once per workgroup.  The combined tile, reduced and
// packed into `st`, is at once the Horner input and -- for a part with a workspace vector -- what is stored as ABI words for launch 3.
template <class F>
struct PolyOpenCfg {
  static constexpr int CS = F::N <= 11 ? 32 : 8;  // (753 bits: st 48 KB + red 13.5 KB + cs 0.9 KB stays below 64 KB)
};

template <class F>
__global__ void __launch_bounds__(PolyCfg<F>::B) poly_open_tiles(const PolyOpenPart* __restrict__ parts, const PolyOpenTerm* __restrict__ terms,
                                                                 const uint32_t* __restrict__ elts_abi, const uint32_t* __restrict__ points_abi,
                                                                 uint32_t* __restrict__ tiles, uint32_t tiles_stride, uint32_t* __restrict__ zt) {
  constexpr int B = PolyCfg<F>::B, E = PolyCfg<F>::E, AW = F::ABI_WORDS, CS = PolyOpenCfg<F>::CS;
  constexpr uint32_t TILE = PolyCfg<F>::TILE;
  static_assert(F::WORDS >= AW, "sub fits into red");
  __shared__ __attribute__((aligned(16))) uint32_t st[TILE * AW];
  __shared__ __attribute__((aligned(16))) uint32_t red[B * F::WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t cs[CS * F::WORDS];
  uint32_t* sub = red;
  const PolyOpenPart d = parts[blockIdx.y];
  const uint64_t lo = (uint64_t)blockIdx.x * TILE;
  if (lo >= d.len) return;  // (whole workgroup; len >= 1, so tile 0 of every part runs)
  const uint32_t cnt = (uint32_t)(d.len - lo < TILE ? d.len - lo : TILE);
  const uint32_t t = threadIdx.x;
  if (!d.work) {  // one term, coefficient 1: the item's own words
    poly_stage_in<F, B>(terms[d.term_lo].p, lo, cnt, TILE, st);
  } else {
    const bool once = d.n_terms <= (uint32_t)CS;
#pragma unroll 1
    for (int e = 0; e < E; e++) {
      const uint64_t elo = lo + (uint64_t)e * B;  // this round: elements [elo, elo + B)
      F acc = F::zero();
#pragma unroll 1
      for (uint32_t j0 = 0; j0 < d.n_terms; j0 += CS) {
        const uint32_t je = min(d.n_terms, j0 + CS);
        if (!once || e == 0) {
          __syncthreads();  // (the previous chunk's products have read cs)
          if (j0 + t < je) {
            const uint32_t c = terms[d.term_lo + j0 + t].coeff;
            (c == POLY_OPEN_ONE ? F::one() : F::from_abi(elts_abi + (size_t)c * AW)).store(cs + (size_t)t * F::WORDS);
          }
        }
#pragma unroll 1
        for (uint32_t j = j0; j < je; j++) {
          const PolyOpenTerm tm = terms[d.term_lo + j];
          if (elo >= tm.len) continue;  // (uniform: the term ends below this round)
          const uint32_t have = (uint32_t)(tm.len - elo < (uint64_t)B ? tm.len - elo : (uint64_t)B);
          const uint32_t* src = tm.p + elo * AW;
          __syncthreads();  // (cs is written; the previous term's products have read sub)
          for (uint32_t w = t; w < (uint32_t)B * AW; w += B) sub[w] = w < have * AW ? src[w] : 0u;
          __syncthreads();
          acc = acc + F::load(cs + (size_t)(j - j0) * F::WORDS) * F::unpack32(sub + (size_t)t * AW);
        }
      }
      acc.canonical().pack32(st + ((size_t)e * B + t) * AW);  // (zero at and beyond the part's len: no term reaches there)
    }
    __syncthreads();
    uint32_t* dst = d.work + lo * AW;
    for (uint32_t w = t; w < cnt * AW; w += B) dst[w] = st[w];
  }
  const F z = F::from_abi(points_abi + (size_t)d.point * AW);
  F m = z;
#pragma unroll
  for (int e = 1; e < E; e++) m = m * z;  // z^E
  __syncthreads();  // (st is whole; sub is no longer read, red may be written)
  F h = poly_lane_horner<F, E>(st, F::zero(), true, z);
  h = poly_block_reduce<F, B>(h, m, red);
  if (t == 0) {
    h.store(tiles + ((size_t)blockIdx.y * tiles_stride + blockIdx.x) * F::WORDS);
    if (blockIdx.x == 0 && d.first_of_point) m.store(zt + (size_t)d.point * F::WORDS);  // m = (z^E)^B, once per POINT
  }
}

// Launch 2: poly_carry_scan with the multiplier z^TILE read per part (a sibling, so that the kernel above keeps its code as it is).
// values_abi[y] = part y at its point.
template <class F>
__global__ void __launch_bounds__(PolyCfg<F>::CB) poly_open_carry_scan(const PolyOpenPart* __restrict__ parts, const uint32_t* __restrict__ tiles,
                                                                       uint32_t tiles_stride, const uint32_t* __restrict__ zt,
                                                                       uint32_t* __restrict__ carries, uint32_t* __restrict__ values_abi) {
  constexpr int CB = PolyCfg<F>::CB;
  constexpr uint32_t TILE = PolyCfg<F>::TILE;
  __shared__ __attribute__((aligned(16))) uint32_t red[CB * F::WORDS];
  const PolyOpenPart d = parts[blockIdx.y];
  const uint32_t K = (uint32_t)((d.len + TILE - 1) / TILE);
  const uint32_t c = (K + CB - 1) / CB;
  const uint32_t lo = min(K, threadIdx.x * c), hi = min(K, lo + c);
  const uint32_t* T = tiles + (size_t)blockIdx.y * tiles_stride * F::WORDS;
  const F Z = K > 1 ? F::load(zt + (size_t)d.point * F::WORDS) : F::one();
  F h = F::zero();
  for (uint32_t k = hi; k-- > lo;) h = F::load(T + (size_t)k * F::WORDS) + Z * h;
  h = poly_block_suffix_scan<F, CB>(h, Z.pow_u64(c), red);
  h.store(red + (size_t)threadIdx.x * F::WORDS);
  __syncthreads();
  F cin = threadIdx.x + 1 < (uint32_t)CB ? F::load(red + (size_t)(threadIdx.x + 1) * F::WORDS) : F::zero();
  for (uint32_t k = hi; k-- > lo;) {
    cin.store(carries + ((size_t)blockIdx.y * tiles_stride + k) * F::WORDS);
    cin = F::load(T + (size_t)k * F::WORDS) + Z * cin;
  }
  if (threadIdx.x == 0) cin.canonical().pack32(values_abi + (size_t)blockIdx.y * F::ABI_WORDS);
}

// Launch 3: poly_div_tile<F, true> per part, from the part's own carries row, point and source.  The canonical store's constant is
// kc * scale (kc = cin * 1 as there), formed by lane 0 and handed round through LDS: scaling the quotient by a challenge costs no product
// beyond the one the canonical store pays anyway.
template <class F>
__global__ void __launch_bounds__(PolyCfg<F>::B) poly_open_div_tiles(const PolyOpenPart* __restrict__ parts, const uint32_t* __restrict__ elts_abi,
                                                                     const uint32_t* __restrict__ points_abi, const uint32_t* __restrict__ carries,
                                                                     uint32_t tiles_stride) {
  constexpr int B = PolyCfg<F>::B, E = PolyCfg<F>::E, AW = F::ABI_WORDS;
  constexpr uint32_t TILE = PolyCfg<F>::TILE;
  __shared__ __attribute__((aligned(16))) uint32_t st[TILE * AW];
  __shared__ __attribute__((aligned(16))) uint32_t red[B * F::WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t ks[F::WORDS];
  const PolyOpenPart d = parts[blockIdx.y];
  const uint64_t lo = (uint64_t)blockIdx.x * TILE;
  if (lo >= d.len || d.len <= 1) return;  // (whole workgroup; a constant has no quotient)
  const uint32_t cnt = (uint32_t)(d.len - lo < TILE ? d.len - lo : TILE);
  poly_stage_in<F, B>(d.src, lo, cnt, TILE, st);
  if (threadIdx.x == 0) {
    F cin, one_raw = F::zero();
#pragma unroll
    for (int i = 0; i < F::N; i++) cin.v[i] = F::Params::cin(i);
    one_raw.v[0] = 1;
    F kc = cin * one_raw;
    if (d.scale != POLY_OPEN_ONE) kc = kc * F::from_abi(elts_abi + (size_t)d.scale * AW);
    kc.store(ks);
  }
  const F z = F::from_abi(points_abi + (size_t)d.point * AW);
  F m = z;
#pragma unroll
  for (int e = 1; e < E; e++) m = m * z;
  const F C = F::load(carries + ((size_t)blockIdx.y * tiles_stride + blockIdx.x) * F::WORDS);
  const bool top = threadIdx.x == B - 1;
  __syncthreads();
  F h = poly_lane_horner<F, E>(st, top ? C : F::zero(), !top, z);
  h = poly_block_suffix_scan<F, B>(h, m, red);
  h.store(red + (size_t)threadIdx.x * F::WORDS);
  __syncthreads();
  F hin = top ? C : F::load(red + (size_t)(threadIdx.x + 1) * F::WORDS);
  const F kc = F::load(ks);
  const uint32_t base = threadIdx.x * E;
#pragma unroll 1
  for (int e = E - 1; e >= 0; e--) {
    uint32_t* s = st + (size_t)(base + e) * AW;
    hin = F::unpack32(s) + z * hin;
    (hin * kc).canonical().pack32(s);
  }
  __syncthreads();
  const uint32_t skip = lo == 0 ? AW : 0;
  for (uint32_t w = threadIdx.x + skip; w < cnt * AW; w += B) d.q[lo * AW + w - AW] = st[w];
}

}  // namespace pcd
