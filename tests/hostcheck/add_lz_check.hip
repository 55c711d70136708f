// TEST HARNESS ONLY (never part of libpcdhip.so): EC::add_lz -- the full addition of two lazily reduced XYZZ accumulators (ec.hip.h) --
// compiled for the HOST with the 128-bit column check on (-DPCD_LZ_CHECK: every column sum of every lazily reduced product and square is
// recomputed in 128 bits and the program aborts where the 64-bit accumulator differs) and compared with the plain Jacobian EC::add on the
// affine image.  tests/test_add_lz_host.py builds it and feeds it curve points from the oracle.
//   add_lz_check <curve: 0 MNT4-298 G1, 1 MNT6-298 G1> <file of n affine points, C-ABI image> <n>
// prints one line "ok <checks> <mismatches>" (exit status 1 with mismatches).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pcd_amd/csrc/ec.hip.h"
using namespace pcd;

static uint32_t g_seed = 0x2545F491u;
template <class F> static F rnd_field() {  // raw limbs below 2^(28 (N-1) + 16) < p: some field element
  F r;
  for (int i = 0; i < F::N; i++) { g_seed = g_seed * 1664525u + 1013904223u; r.v[i] = (g_seed >> 4) & 0x0FFFFFFFu; }
  r.v[F::N - 1] &= 0xFFFFu;
  if (r.is_zero()) r = F::one();
  return r;
}
// the representative in [p, 2p) of a value (the upper end of what a reduced coordinate may be)
template <class F> __attribute__((noinline)) static F upper(const F& f) {
  F c = f.canonical(), r;
  uint32_t carry = 0;
  for (int i = 0; i < F::N; i++) {
    const uint32_t x = c.v[i] + F::Params::mod(i) + carry;
    r.v[i] = i < F::N - 1 ? (x & 0x0FFFFFFFu) : x;
    carry = i < F::N - 1 ? (x >> 28) : 0;
  }
  return r;
}

template <class G>
struct Check {
  typedef typename G::F F;
  typedef EC<G> E;
  typedef Jac<F> J;
  typedef typename E::AccLz Lz;
  long checks = 0, bad = 0;

  // (the templates of ec.hip.h are force-inlined: one out-of-line copy of each operation keeps this program small enough to compile quickly)
#define NOINL __attribute__((noinline)) static
  NOINL Lz add_lz(const Lz& a, const Lz& b) { return E::add_lz(a, b); }
  NOINL Lz madd_lz(const Lz& a, const Aff<F>& b) { return E::madd_lz(a, b); }
  NOINL Lz lz_from(const J& a) { return E::lz_from(a); }
  NOINL J lz_to_jac(const Lz& a) { return E::lz_to_jac(a); }
  NOINL J add(const J& a, const J& b) { return E::add(a, b); }
  NOINL J madd(const J& a, const Aff<F>& b) { return E::madd(a, b); }
  NOINL J dbl(const J& a) { return E::dbl(a); }
  NOINL Aff<F> to_affine(const J& a) { return E::to_affine(a); }
  NOINL F canon(const F& a) { return a.canonical(); }
  NOINL F mul(const F& a, const F& b) { return a * b; }

  static bool same_value(const F& a, const F& b) {
    const F x = canon(a), y = canon(b);
    bool ok = true;
    for (int i = 0; i < F::N; i++) ok &= x.v[i] == y.v[i];
    return ok;
  }
  void expect(const Lz& got, const J& want, const char* what) {
    checks++;
    const Aff<F> a = to_affine(lz_to_jac(got)), b = to_affine(want);
    const bool fmt = got.inf || (format_ok(got));
    if (!(same_value(a.x, b.x) && same_value(a.y, b.y) && got.inf == want.is_inf() && fmt)) {
      if (bad < 10) fprintf(stderr, "mismatch: %s\n", what);
      bad++;
    }
  }
  // the stated format: X carried (limbs 0 .. N-2 in [0, 2^28)) with value below 16p, Y / ZZ / ZZZ normalised limbs below 2p
  static bool below(const int64_t* v, int mult) {  // value of the limbs < mult * p: the borrow out of value - mult p
    __int128 borrow = 0;
    for (int i = 0; i < F::N; i++) {
      __int128 d = (__int128)v[i] - (__int128)mult * F::Params::mod(i) + borrow;
      borrow = d >> 28;  // arithmetic shift: floor
    }
    return borrow < 0;
  }
  NOINL bool format_ok(const Lz& a) {
    int64_t x[F::N];
    for (int i = 0; i < F::N; i++) { x[i] = a.X.v[i]; if (i < F::N - 1 && (a.X.v[i] < 0 || a.X.v[i] >= (1 << 28))) return false; }
    if (a.X.v[F::N - 1] < 0 || !below(x, 16)) return false;
    const F* c[3] = {&a.Y, &a.ZZ, &a.ZZZ};
    for (int k = 0; k < 3; k++) {
      int64_t y[F::N];
      for (int i = 0; i < F::N; i++) { y[i] = c[k]->v[i]; if (c[k]->v[i] >= (1u << 28)) return false; }
      if (!below(y, 2)) return false;
    }
    return true;
  }

  NOINL J scaled(const Aff<F>& p, const F& z) {  // (x z^2 : y z^3 : z)
    const F zz = mul(z, z);
    return {mul(p.x, zz), mul(mul(p.y, zz), z), z};
  }
  // the same record with every coordinate at the upper end of its stated range: X + 4p + 2p (below 16p for X < 10p), the others in [p, 2p)
  NOINL Lz at_edge(const Lz& a) {
    if (a.inf) return a;
    Lz r = a;
    typename F::Lz t;
    for (int i = 0; i < F::N; i++) t.v[i] = a.X.v[i] + (int32_t)F::Params::mod4(i) + (int32_t)F::Params::mod2(i);
    r.X = F::lz_carry(t);
    r.Y = upper(a.Y); r.ZZ = upper(a.ZZ); r.ZZZ = upper(a.ZZZ);
    return r;
  }

  int run(const std::vector<Aff<F>>& pts) {
    const int n = (int)pts.size();
    const Lz inf = E::lz_infinity();
    const J jinf = J::infinity();
    // 1. every ordered pair of distinct points under fresh random Z on both sides
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) {
        if (i == j) continue;
        const J a = scaled(pts[i], rnd_field<F>()), b = scaled(pts[j], rnd_field<F>());
        expect(add_lz(lz_from(a), lz_from(b)), add(a, b), "random pair");
      }
    // 2. the special cases, with different representations of the same point on the two sides
    expect(add_lz(inf, inf), jinf, "inf + inf");
    for (int i = 0; i < n; i++) {
      const J a = scaled(pts[i], rnd_field<F>()), a2 = scaled(pts[i], rnd_field<F>());
      const Lz la = lz_from(a), la2 = lz_from(a2);
      expect(add_lz(la, inf), a, "P + inf");
      expect(add_lz(inf, la), a, "inf + P");
      expect(add_lz(la, la), dbl(a), "P + P (same record)");
      expect(add_lz(la, la2), dbl(a), "P + P (other Z)");
      expect(add_lz(at_edge(la), at_edge(la2)), dbl(a), "P + P (edge records)");
      expect(add_lz(la, lz_from(E::neg(a2))), jinf, "P + (-P)");
      expect(add_lz(at_edge(la), at_edge(lz_from(E::neg(a2)))), jinf, "P + (-P) (edge records)");
    }
    // 3. operands as the accumulation leaves them: X unreduced after a chain of madd_lz steps; and the same records pushed to the upper
    //    end of the format (X just below 16p, Y / ZZ / ZZZ in [p, 2p)) on either side and on both
    for (int i = 0; i + 8 <= n; i++) {
      for (int len = 2; len <= 4; len++) {
        Lz la = inf, lb = inf;
        J ja = jinf, jb = jinf;
        for (int k = 0; k < len; k++) {
          la = madd_lz(la, pts[i + k]); ja = madd(ja, pts[i + k]);
          lb = madd_lz(lb, pts[i + 4 + k]); jb = madd(jb, pts[i + 4 + k]);
        }
        const J want = add(ja, jb);
        expect(add_lz(la, lb), want, "madd chains");
        expect(add_lz(at_edge(la), lb), want, "madd chains, left at the edge");
        expect(add_lz(la, at_edge(lb)), want, "madd chains, right at the edge");
        expect(add_lz(at_edge(la), at_edge(lb)), want, "madd chains, both at the edge");
        expect(add_lz(at_edge(la), madd_lz(inf, pts[i])), add(ja, J{pts[i].x, pts[i].y, F::one()}), "edge + affine record");
      }
    }
    // 4. chains of 32 additions: the output feeds the next step as the left operand, and separately as the right one; every second
    //    incoming record is pushed to the edge of the format.  Then the pattern of the first reduction level (run += B, acc += run) with
    //    empty buckets in between, which takes the doubling branch.
    for (int start = 0; start + 33 <= n; start += 7) {
      Lz left = madd_lz(inf, pts[start]), right = left;
      J want = {pts[start].x, pts[start].y, F::one()};
      for (int k = 1; k <= 32; k++) {
        Lz b = madd_lz(madd_lz(inf, pts[start + k]), pts[(start + 3 * k) % n]);
        const J jb = madd(J{pts[start + k].x, pts[start + k].y, F::one()}, pts[(start + 3 * k) % n]);
        if (k & 1) b = at_edge(b);
        left = add_lz(left, b);
        right = add_lz(b, right);
        want = add(want, jb);
        expect(left, want, "chain, output as left operand");
        expect(right, want, "chain, output as right operand");
      }
      Lz run = inf, acc = inf;
      J jrun = jinf, jacc = jinf;
      for (int k = 0; k < 32; k++) {
        if (k % 3 != 1) { run = add_lz(run, madd_lz(inf, pts[start + k])); jrun = madd(jrun, pts[start + k]); }
        acc = add_lz(acc, run); jacc = add(jacc, jrun);
        expect(acc, jacc, "running sums");
      }
    }
    printf("ok %ld %ld\n", checks, bad);
    return bad ? 1 : 0;
  }
};

template <class G>
static int run_curve(const char* path, int n) {
  typedef typename G::F F;
  std::vector<uint32_t> raw((size_t)n * Aff<F>::ABI_WORDS);
  FILE* f = fopen(path, "rb");
  if (!f || fread(raw.data(), 4, raw.size(), f) != raw.size()) { fprintf(stderr, "cannot read %s\n", path); return 2; }
  fclose(f);
  std::vector<Aff<F>> pts;
  for (int i = 0; i < n; i++) pts.push_back(Aff<F>::from_abi(raw.data() + (size_t)i * Aff<F>::ABI_WORDS));
  Check<G> c;
  return c.run(pts);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int curve = atoi(argv[1]), n = atoi(argv[3]);
  if (n < 40) return 2;
  switch (curve) {
    case 0: return run_curve<G1_MNT4_298>(argv[2], n);
    case 1: return run_curve<G1_MNT6_298>(argv[2], n);
  }
  return 2;
}
