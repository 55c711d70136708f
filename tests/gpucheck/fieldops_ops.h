// TEST HARNESS ONLY (never part of libpcdhip.so): ONE element of one field / Lz / tower / accumulator-step operation on RAW device
// images (28-bit limbs, any representative the operation's contract allows), written once as __host__ __device__ code so that the host
// build (tests/hostcheck/hostcheck.hip, with the 128-bit column check) and the gfx950 build (fieldops_check.hip, one element per lane)
// run exactly the same case lists.  The expected values are Python integers (tests/field_reference.py), never another build of this.
#pragma once
#include "../../pcd_amd/csrc/ec.hip.h"

namespace fieldops {
using namespace pcd;

enum FieldOp {
  F_MUL = 0, F_SQR, F_ADD, F_SUB, F_NEG, F_DBL, F_MUL_SMALL, F_MUL_SMALL_VAR, F_INV_GCD, F_INV_FERMAT, F_MUL_INV, F_CANONICAL, F_IS_ZERO,
  F_EQ, F_TO_ABI, F_ABI_ROUNDTRIP, F_TO_WORDS, F_WORDS_ROUNDTRIP, F_SIGNED_SUM, F_OPS
};
enum LzOp { L_MUL = 0, L_DOT2, L_DOT4, L_SQR, L_SCALE_CARRY, L_CARRY, L_SUB0, L_SUB2, L_SHL, L_OPS };
enum TowerOp { T_MUL = 0, T_SQR, T_INV, T_OPS };
enum StepOp { S_MADD_LZ = 0, S_MADD_X, S_MADD_X_PLAIN, S_MADD_JAC, S_OPS };
constexpr int SIGNED_SUM_MAX_TERMS = 16;

// words per element of the operands: a, b (F_SIGNED_SUM: k terms of N words, and k int32 coefficients); the result is always N words
template <class F> PCD_HD int field_a_words(int op, uint32_t k) { return op == F_SIGNED_SUM ? (int)k * F::N : F::N; }
template <class F> PCD_HD int field_b_words(int op, uint32_t k) { return op == F_SIGNED_SUM ? (int)k : F::N; }

// Every operation that holds field products is ONE non-inlined body per field variant (operands by reference, like Fp::dot_call), shared by
// the operations that use it: the inlined variant of a 753-bit field would otherwise put seventeen 27-limb products into one kernel.
#define FO_BODY __host__ __device__ __noinline__ static
template <class F>
struct FieldBodies {
  static constexpr int N = F::N;
  FO_BODY void mul(F& o, const F& x, const F& y) { o = x * y; }
  FO_BODY void sqr(F& o, const F& x) { o = x.sqr(); }
  FO_BODY void inv_gcd(F& o, const F& x) { o = x.inv_gcd(); }
  FO_BODY void inv_fermat(F& o, const F& x) { o = x.inv_fermat(); }
  FO_BODY void to_abi(uint32_t* w, const F& x) { x.to_abi(w); }
  FO_BODY void from_abi(F& o, const uint32_t* w) { o = F::from_abi(w); }
  FO_BODY void to_words(uint32_t* w, const F& x) { x.to_canonical_words(w); }
  FO_BODY void from_words(F& o, const uint32_t* w) { o = F::from_canonical_words(w); }
  FO_BODY void signed_sum(F& o, const uint32_t* a, const uint32_t* b, uint32_t k) {
    int64_t s[N];
    for (int i = 0; i < N; i++) s[i] = 0;
    for (uint32_t t = 0; t < k; t++)
      for (int i = 0; i < N; i++) s[i] += (int64_t)(int32_t)b[t] * (int64_t)a[(size_t)t * N + i];
    o = F::from_signed_sum(s);
  }
};
#undef FO_BODY

template <class F>
PCD_HD void field_op(int op, const uint32_t* a, const uint32_t* b, uint32_t k, uint32_t* out) {
  constexpr int N = F::N;
  typedef FieldBodies<F> FB;
  F r = F::zero();
  if (op == F_SIGNED_SUM) {
    FB::signed_sum(r, a, b, k);
    r.store(out);
    return;
  }
  const F x = F::load(a), y = F::load(b);
  uint32_t w[N];
  for (int i = 0; i < N; i++) w[i] = 0;
  switch (op) {
    case F_MUL: FB::mul(r, x, y); break;
    case F_SQR: FB::sqr(r, x); break;
    case F_ADD: r = x + y; break;
    case F_SUB: r = x - y; break;
    case F_NEG: r = x.neg(); break;
    case F_DBL: r = x.dbl(); break;
    case F_MUL_SMALL: r = x.mul_small(k); break;
    case F_MUL_SMALL_VAR: r = x.mul_small_var(k); break;
    case F_INV_GCD: FB::inv_gcd(r, x); break;
    case F_INV_FERMAT: FB::inv_fermat(r, x); break;
    case F_MUL_INV: { F t; FB::inv_gcd(t, x); FB::mul(r, x, t); r = r.canonical(); break; }   // (Fp::inv() is inv_gcd)
    case F_CANONICAL: r = x.canonical(); break;
    case F_IS_ZERO: r.v[0] = x.is_zero() ? 1u : 0u; break;
    case F_EQ: r.v[0] = (x == y) ? 1u : 0u; r.v[1] = (x != y) ? 1u : 0u; break;
    case F_TO_ABI: FB::to_abi(w, x); r = F::load(w); break;
    case F_ABI_ROUNDTRIP: FB::to_abi(w, x); FB::from_abi(r, w); break;
    case F_TO_WORDS: FB::to_words(w, x); r = F::load(w); break;
    case F_WORDS_ROUNDTRIP: FB::to_words(w, x); FB::from_words(r, w); break;
    default: break;
  }
  r.store(out);
}

// ops: eight Lz images (a0 b0 a1 b1 a2 b2 a3 b3) of N signed words each; the result is N words (a field element, or an Lz image)
template <class F>
PCD_HD void lz_op(int op, const int32_t* ops, int32_t k, uint32_t* out) {
  constexpr int N = F::N;
  typedef typename F::Lz L;
  L o[8];
  for (int j = 0; j < 8; j++)
    for (int i = 0; i < N; i++) o[j].v[i] = ops[j * N + i];
  F r = F::zero();
  L l = o[0];
  bool is_lz = false;
  switch (op) {
    case L_MUL: r = F::lz_mul(o[0], o[1]); break;
    case L_DOT2: r = F::lz_dot2(o[0], o[1], o[2], o[3]); break;
    case L_DOT4: r = F::lz_dot4(o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]); break;
    case L_SQR: r = F::lz_sqr(o[0]); break;
    case L_SCALE_CARRY: l = F::lz_scale_carry(o[0], k); is_lz = true; break;
    case L_CARRY: l = F::lz_carry(o[0]); is_lz = true; break;
    case L_SUB0: l = F::template lz_sub<0>(o[0], o[1]); is_lz = true; break;
    case L_SUB2: l = F::template lz_sub<2>(o[0], o[1]); is_lz = true; break;
    case L_SHL: l = F::lz_shl(o[0], k); is_lz = true; break;
    default: break;
  }
  for (int i = 0; i < N; i++) out[i] = is_lz ? (uint32_t)l.v[i] : r.v[i];
}

template <class T>
PCD_HD void tower_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const T x = T::load(a), y = T::load(b);
  T r = T::zero();
  switch (op) {
    case T_MUL: r = x * y; break;
    case T_SQR: r = x.sqr(); break;
    case T_INV: r = x.inv(); break;
    default: break;
  }
  r.store(out);
}

// One accumulator record: X || Y || ZZ || ZZZ (raw images) || identity flag; `steps` mixed additions of the affine points q[0 .. steps).
// S_MADD_JAC: the Jacobian record X || Y || Z || identity flag of EC::madd (what the 27-limb G1 / Fq3 groups accumulate in).
template <class G> PCD_HD int step_words(int op) { return (op == S_MADD_JAC ? 3 : 4) * G::F::WORDS + 1; }
template <class G>
PCD_HD void madd_steps(int op, const uint32_t* acc, const uint32_t* q, int steps, uint32_t* out) {
  typedef typename G::F F;
  typedef EC<G> E;
  constexpr int W = F::WORDS;
  if (op == S_MADD_LZ) {
    if constexpr (LazyCapable<F>::value) {
      typename E::AccLz a;
      for (int i = 0; i < W; i++) a.X.v[i] = (int32_t)acc[i];
      a.Y = F::load(acc + W); a.ZZ = F::load(acc + 2 * W); a.ZZZ = F::load(acc + 3 * W); a.inf = acc[4 * W] != 0;
      for (int s = 0; s < steps; s++) a = E::madd_lz(a, Aff<F>::load(q + (size_t)s * 2 * W));
      for (int i = 0; i < W; i++) out[i] = (uint32_t)a.X.v[i];
      a.Y.store(out + W); a.ZZ.store(out + 2 * W); a.ZZZ.store(out + 3 * W); out[4 * W] = a.inf ? 1u : 0u;
    }
    return;
  }
  if (op == S_MADD_JAC) {   // (only the groups with non-inlined arithmetic accumulate in Jacobian coordinates: msm.hip.h MsmUseXyzz)
    if constexpr (!F::Base::INLINE_ARITH) {
      Jac<F> a = Jac<F>::load(acc);
      if (acc[3 * W] != 0) a = Jac<F>::infinity();
      for (int s = 0; s < steps; s++) a = E::madd(a, Aff<F>::load(q + (size_t)s * 2 * W));
      a.store(out); out[3 * W] = a.is_inf() ? 1u : 0u;
    }
    return;
  }
  typename E::AccX a = {F::load(acc), F::load(acc + W), F::load(acc + 2 * W), F::load(acc + 3 * W)};
  if (acc[4 * W] != 0) a = E::x_infinity();
  for (int s = 0; s < steps; s++) {
    const Aff<F> p = Aff<F>::load(q + (size_t)s * 2 * W);
    a = op == S_MADD_X ? E::madd_x(a, p) : E::madd_x_plain(a, p);
  }
  a.X.store(out); a.Y.store(out + W); a.ZZ.store(out + 2 * W); a.ZZZ.store(out + 3 * W); out[4 * W] = a.is_inf() ? 1u : 0u;
}

// the plain towers the product computes G2 coordinates in: Fq2 over fields 0 and 2 (MNT4), Fq3 over fields 1 and 3 (MNT6)
typedef G2_MNT4_298::F Tower0;
typedef G2_MNT6_298::F Tower1;
typedef G2_MNT4_753::F Tower2;
typedef G2_MNT6_753::F Tower3;

}  // namespace fieldops
