// K14: the two kernels of the MarlinKZG10 check that are its own (capi_kzg.hip kzg_check_run runs them between points_in, the batched
// short MSM and the pairing): the collapse of a round's tables onto the column scalars of the two MSMs, and the hand-over of the MSMs'
// Jacobian results to the pairing.
//
// The vector of a check, N = 2 + n_shift + 2 m + P points, in this order (the resident part first):
//   [0] g   [1] gamma_g   [2 + k] S_k, k < n_shift   [2 + n_shift + i] comm_i   [2 + n_shift + m + i] shifted_i   [2 + n_shift + 2 m + o] W_o
// Equation e of E takes row e of an E x P randomizer matrix rho: the caller's randomizers (E = 1, combined mode) or the identity matrix
// (E = P, per-opening mode).  Its left scalars over the vector and its right scalars over the W range:
//   g          - sum_o rho_o value_o            comm_i     sum_o rho_o a_(o,i)
//   gamma_g    - sum_o rho_o random_v_o         shifted_i  sum_o rho_o s_(o,i)
//   S_k        - sum_o sum_{i : k(i) = k} rho_o s_(o,i) v_(o,i)
//   W_o          rho_o z_o                      right: W_o -> rho_o
#pragma once
#include "ec.hip.h"

namespace pcd {

// a call's tables on the device: C-ABI words as the host has them (Montgomery, R = 2^(32 N32)), the randomizers canonical
struct KzgCheckTables {
  const uint32_t* a;            // P x m
  const uint32_t* s;            // P x m; null: no degree-bound term anywhere
  const uint32_t* v;            // P x m, read only where s != 0; null with s
  const int32_t* shift_index;   // m; null with s
  const uint32_t* z;            // P
  const uint32_t* value;        // P
  const uint32_t* random_v;     // P; null: none
  const uint32_t* randomizers;  // P canonical scalars; null: per-opening mode
  uint32_t m, P, n_shift, E;
};

// One lane per (column, equation), a loop over the openings.  Nothing is converted on the way in: the Montgomery product of the plain
// words x and y is x y / R' (R' = 2^(28 N), the device image's radix), so with rho canonical (plain) and a = a' R in the ABI image
//   rho (x) a = rho a' R / R',      (rho (x) s) (x) v = rho s' v' R^2 / R'^2
// and one product with cin = R'^2 / R per ABI factor at the END of the sum leaves the plain integer rho a' (rho s' v'): a column costs one
// product per term, two for a shift power's, and writes canonical words where the MSM reads them.
// (the body of a lane: column c < N + P of equation e; host-callable, as the field code is)
template <class F>
PCD_HD void kzg_check_column(const KzgCheckTables& t, uint32_t e, uint32_t c, uint32_t* __restrict__ left, uint32_t* __restrict__ right) {
  constexpr int AW = F::ABI_WORDS;
  const uint32_t m = t.m, P = t.P, ns = t.n_shift;
  const uint32_t N = 2u + ns + 2u * m + P;
  // the openings with a non-zero randomizer in row e, and that randomizer as plain words
  const uint32_t o_lo = t.randomizers ? 0u : e, o_hi = t.randomizers ? P : e + 1u;
  auto rho = [&](uint32_t o) {
    if (t.randomizers) return F::unpack32(t.randomizers + (size_t)o * AW);
    F one = F::zero();
    one.v[0] = 1u;
    return one;
  };
  auto elt = [&](const uint32_t* table, size_t idx) { return F::unpack32(table + idx * AW); };
  if (c >= N) {  // the right side: row e of the matrix itself
    const uint32_t o = c - N;
    uint32_t* out = right + ((size_t)e * P + o) * AW;
    for (int k = 0; k < AW; k++) out[k] = t.randomizers ? t.randomizers[(size_t)o * AW + k] : (k == 0 && o == e ? 1u : 0u);
    return;
  }
  F acc = F::zero();
  int factors = 1;  // ABI factors per term
  bool negate = false;
  if (c == 0u) {
    for (uint32_t o = o_lo; o < o_hi; o++) acc = acc + rho(o) * elt(t.value, o);
    negate = true;
  } else if (c == 1u) {
    if (t.random_v)
      for (uint32_t o = o_lo; o < o_hi; o++) acc = acc + rho(o) * elt(t.random_v, o);
    negate = true;
  } else if (c < 2u + ns) {
    const int32_t k = (int32_t)(c - 2u);
    if (t.s)
      for (uint32_t o = o_lo; o < o_hi; o++) {
        const F r = rho(o);
        for (uint32_t i = 0; i < m; i++) {
          if (t.shift_index[i] != k) continue;
          const F s = elt(t.s, (size_t)o * m + i);
          if (s.is_raw_zero()) continue;  // (v is read only where s != 0)
          acc = acc + (r * s) * elt(t.v, (size_t)o * m + i);
        }
      }
    factors = 2;
    negate = true;
  } else if (c < 2u + ns + 2u * m) {
    const uint32_t j = c - 2u - ns;
    const uint32_t* table = j < m ? t.a : t.s;
    const uint32_t i = j < m ? j : j - m;
    if (table)
      for (uint32_t o = o_lo; o < o_hi; o++) acc = acc + rho(o) * elt(table, (size_t)o * m + i);
  } else {
    const uint32_t o = c - 2u - ns - 2u * m;
    if (o >= o_lo && o < o_hi) acc = rho(o) * elt(t.z, o);
  }
  F cin;
  for (int i = 0; i < F::N; i++) cin.v[i] = F::Params::cin(i);
  for (int f = 0; f < factors; f++) acc = acc * cin;
  if (negate) acc = acc.neg();
  acc.canonical().pack32(left + ((size_t)e * N + c) * AW);
}
template <class F>
__global__ void __launch_bounds__(64) kzg_check_scalars_kernel(KzgCheckTables t, uint32_t* __restrict__ left, uint32_t* __restrict__ right) {
  const uint32_t cols = 2u + t.n_shift + 2u * t.m + 2u * t.P;
  const uint32_t id = blockIdx.x * 64u + threadIdx.x;
  if (id >= t.E * cols) return;
  kzg_check_column<F>(t, id / cols, id % cols, left, right);
}

// The 2 E results of the batched short MSM (Jacobian, device image; 2 e the left side of equation e, 2 e + 1 its right side) as the
// pairing takes them, the left sides negated: e(-L, h) e(R, beta_h) == 1.  With out_z the wave-per-pairing form -- (X, Y) into the G1
// array, Z into the Z array, no inversion, an identity as (0 : 1 : 0) -- and without it whole Jacobian points in the C-ABI image, which
// to_affine then normalises for the lane-per-pairing kernels.
template <class G>
__global__ void __launch_bounds__(64) kzg_check_pairs_kernel(const uint32_t* __restrict__ jac, uint32_t n, uint32_t* __restrict__ out,
                                                             uint32_t* __restrict__ out_z) {
  typedef typename G::F F;
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  Jac<F> p = Jac<F>::load(jac + (size_t)i * Jac<F>::WORDS);
  if (p.is_inf()) p = Jac<F>::infinity();
  else if ((i & 1u) == 0u) p.Y = p.Y.neg();
  if (out_z) {
    const Aff<F> xy = {p.X, p.Y};
    xy.to_abi(out + (size_t)i * Aff<F>::ABI_WORDS);
    p.Z.to_abi(out_z + (size_t)i * F::ABI_WORDS);
  } else {
    p.to_abi(out + (size_t)i * Jac<F>::ABI_WORDS);
  }
}

}  // namespace pcd
