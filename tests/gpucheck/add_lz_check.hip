// TEST HARNESS ONLY (never part of libpcdhip.so): EC::add_lz -- the full addition of two lazily reduced XYZZ accumulators -- on the GPU
// against the device's plain Jacobian EC::add, operation by operation, under RANDOM LANE MASKS: every lane draws its own case each round,
// so the rare branches (an identity on either side, equal points -> the doubling branch, opposite points -> the identity) are taken by
// some lanes of a wave while the others add normally or sit the round out.  Both forms are rational identities in the coordinates, so
// they are compared as points: X_a Z_b^2 = X_b Z_a^2 and Y_a Z_b^3 = Y_b Z_a^3 as values mod p.
// Compiled by tests/test_gpu_add_lz.py (hipcc, gfx950) into a temporary shared library.
#include <cstdio>
#include "../../pcd_amd/csrc/ec.hip.h"
using namespace pcd;

template <class B> __device__ B al_rnd(uint32_t& s) {
  B r;
  for (int i = 0; i < B::N; i++) { s = s * 1664525u + 1013904223u; r.v[i] = (s >> 4) & 0x0FFFFFFFu; }
  r.v[B::N - 1] &= 0xFFFFu;  // < 2^(28 (N-1) + 16) < p
  return r;
}
template <class F> __device__ bool al_same(const F& a0, const F& b0) {
  const F a = a0.canonical(), b = b0.canonical();
  bool ok = true;
  for (int i = 0; i < F::N; i++) ok &= a.v[i] == b.v[i];
  return ok;
}
template <class F> __device__ bool al_same_pt(const Jac<F>& a, const Jac<F>& b) {
  if (a.is_inf() || b.is_inf()) return a.is_inf() == b.is_inf();
  const F za = a.Z.sqr(), zb = b.Z.sqr();
  return al_same(a.X * zb, b.X * za) && al_same(a.Y * zb * b.Z, b.Y * za * a.Z);
}
// the representative in [p, 2p) of a value, and a record with every coordinate at the upper end of its range (X + 6p: below 16p for X < 10p)
template <class F> __device__ F al_upper(const F& f) {
  F c = f.canonical(), r;
  uint32_t carry = 0;
  for (int i = 0; i < F::N; i++) {
    const uint32_t x = c.v[i] + F::Params::mod(i) + carry;
    r.v[i] = i < F::N - 1 ? (x & 0x0FFFFFFFu) : x;
    carry = i < F::N - 1 ? (x >> 28) : 0;
  }
  return r;
}
template <class G> __device__ typename EC<G>::AccLz al_edge(const typename EC<G>::AccLz& a) {
  typedef typename G::F F;
  if (a.inf) return a;
  typename EC<G>::AccLz r = a;
  typename F::Lz t;
  for (int i = 0; i < F::N; i++) t.v[i] = a.X.v[i] + (int32_t)F::Params::mod4(i) + (int32_t)F::Params::mod2(i);
  r.X = F::lz_carry(t);
  r.Y = al_upper(a.Y); r.ZZ = al_upper(a.ZZ); r.ZZZ = al_upper(a.ZZZ);
  return r;
}

// cases: 0, 1 random pair   2 operands after madd_lz steps (X unreduced)   3 the same at the edge of the format   4 equal points, other Z
//        5 opposite points   6 an identity on the left / the right / both   7 sits the round out
//        8 chain of 32, output as the left operand   9 chain of 32, output as the right operand (incoming records alternately at the edge)
constexpr int AL_CASES = 10;
template <class G>
__global__ void __launch_bounds__(64) al_check(uint32_t* bad, int rounds, uint32_t seed) {
  typedef typename G::F F;
  typedef EC<G> E;
  typedef Jac<F> J;
  typedef typename E::AccLz Lz;
  const uint32_t lane = blockIdx.x * 64 + threadIdx.x;
  uint32_t s = seed ^ (0x9E3779B9u * (lane + 1u));
  for (int it = 0; it < rounds; it++) {
    s = s * 1664525u + 1013904223u;
    const uint32_t choice = (s >> 8) % (uint32_t)AL_CASES;
    F c[6];
    for (int k = 0; k < 6; k++) c[k] = al_rnd<F>(s);
    if (choice == 7) continue;
    J ja = {c[0], c[1], c[2]}, jb = {c[3], c[4], c[5]};
    if (choice == 4) { const F l = c[3], ll = l.sqr(); jb = {ja.X * ll, ja.Y * ll * l, ja.Z * l}; }
    if (choice == 5) { const F l = c[3], ll = l.sqr(); jb = {ja.X * ll, (ja.Y * ll * l).neg(), ja.Z * l}; }
    if (choice == 6) { if (it % 3 != 1) ja = J::infinity(); if (it % 3 != 0) jb = J::infinity(); }
    Lz la = E::lz_from(ja), lb = E::lz_from(jb);
    if (choice == 2 || choice == 3) {
      for (int k = 0; k < 3; k++) {
        const Aff<F> q = {al_rnd<F>(s), al_rnd<F>(s)}, q2 = {al_rnd<F>(s), al_rnd<F>(s)};
        la = E::madd_lz(la, q); ja = E::madd(ja, q);
        lb = E::madd_lz(lb, q2); jb = E::madd(jb, q2);
      }
    }
    if (choice == 3 || (choice == 4 && (it & 1))) { la = al_edge<G>(la); lb = al_edge<G>(lb); }
    const int steps = choice >= 8 ? 32 : 1;
    bool ok = true;
    for (int st = 0; st < steps; st++) {
      const Lz got = E::add_lz(la, lb);
      const J want = E::add(ja, jb);
      ok &= al_same_pt(E::lz_to_jac(got), want) && got.inf == want.is_inf();
      if (steps > 1) {  // feed the sum back on one side, a fresh record on the other
        const J fresh = {al_rnd<F>(s), al_rnd<F>(s), al_rnd<F>(s)};
        Lz lf = E::lz_from(fresh);
        if (st & 1) lf = al_edge<G>(lf);
        if (choice == 8) { la = got; ja = want; lb = lf; jb = fresh; }
        else { lb = got; jb = want; la = lf; ja = fresh; }
      }
    }
    if (!ok) atomicAdd(bad + choice, 1);
    atomicAdd(bad + AL_CASES + choice, 1);  // how often each case ran
  }
  atomicAdd(bad + 2 * AL_CASES, 1);  // lanes that ran to the end
}

template <class G> static int al_run(int rounds, uint32_t seed, uint32_t* out) {
  constexpr size_t BYTES = (2 * AL_CASES + 1) * 4;
  uint32_t* bad;
  if (hipMalloc(&bad, BYTES) != hipSuccess) return -1;
  (void)hipMemset(bad, 0, BYTES);
  hipLaunchKernelGGL((al_check<G>), dim3(8), dim3(64), 0, 0, bad, rounds, seed);
  const hipError_t e = hipDeviceSynchronize();
  (void)hipMemcpy(out, bad, BYTES, hipMemcpyDeviceToHost);
  (void)hipFree(bad);
  return e == hipSuccess ? 0 : -2;
}
// which: 0 MNT4-298 G1, 1 MNT6-298 G1.  out[0..9] = mismatches per case, out[10..19] = runs per case, out[20] = lanes that finished
extern "C" int gc_add_lz_check(int which, int rounds, uint32_t seed, uint32_t* out) {
  switch (which) {
    case 0: return al_run<G1_MNT4_298>(rounds, seed, out);
    case 1: return al_run<G1_MNT6_298>(rounds, seed, out);
  }
  return -3;
}
