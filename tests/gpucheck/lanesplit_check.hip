// TEST HARNESS ONLY (never part of libpcdhip.so): the LANE-SPLIT extension fields of pcd_amd/csrc/fp.hip.h (Fp2S: two lanes per element,
// Fp3S: three) and the group law of ec.hip.h in them, one operation per item on RAW limb images, against Python integers
// (tests/field_reference.py; tests/test_gpu_lanesplit_ops.py drives it).  These forms exist in the gfx950 build only (PCD_DEV).
// Layout: workgroups of 64 lanes (the mailbox is per lane of one wave); an item is L = 2 / 3 adjacent lanes, item i of a block sits at
// lanes L i .. L i + L - 1 (L = 3: lane 63 of every wave idles).  The host passes one active flag per item: an inactive item returns at
// once, so the collective operations (partner exchange, both() / all3(), the mailbox posts) run under a ragged exec mask.  Memory images
// are the product's own, c0 || c1 (|| c2), read with F::load and written with F::store (the role addressing is part of what is tested).
// The host pre-fills the output with a sentinel; `ran` counts the LANES that finished.
// type / group numbers (the coordinate field of group g is type g):
//   0  Fp2S<Fp<F298A, true>>   G2Cfg2S<F298A, .., true>    SplitOfTail of the MNT4-298 G2
//   1  Fp3S<Fp<F298B, true>>   G2Cfg3S<F298B, .., true>    AccOf / SplitOfTail of the MNT6-298 G2
//   2  Fp2S<Fp<F753A, false>>  G2Cfg2S<F753A, .., false>   the single-item kernels of the MNT4-753 G2
//   3  Fp3S<Fp<F753B, false>>  G2Cfg3S<F753B, .., false>   the single-item kernels of the MNT6-753 G2
//   4  type 2 over the mailbox field   G2Cfg2SMB<F753A>    AccOf / SplitOfTail of the MNT4-753 G2
//   5  type 3 over the mailbox field   G2Cfg3SMB<F753B>    AccOf / SplitOfTail of the MNT6-753 G2
// One source, three translation units (-DLANESPLIT_PART=0..2, tests/gpucheck/Makefile) so that they compile side by side: 0 the 298-bit
// types and the entry points, 1 the two forms over F753A, 2 the two forms over F753B.
#include <vector>
#include "../../pcd_amd/csrc/ec.hip.h"
#ifndef LANESPLIT_PART
#error "compile with -DLANESPLIT_PART=0..2"
#endif
using namespace pcd;

enum TowerOp { T_MUL = 0, T_SQR, T_ADD, T_SUB, T_NEG, T_DBL, T_MUL_SMALL, T_MUL_BY_A, T_IS_ZERO, T_IS_RAW_ZERO, T_EQ, T_ONE, T_FROM_ABI, T_ABI_ROUNDTRIP, T_OPS };
enum GroupOp { S_MADD_X = 0, S_MADD_JAC, J_ADD, J_DBL, X_ROUNDTRIP, G_OPS };
constexpr uint32_t SENTINEL = 0xA5A5A5A5u;

template <int ID> struct GroupOf;
template <> struct GroupOf<0> { typedef G2Cfg2S<F298A, F298B, PCD_MNT4_298_A_SMALL, PCD_MNT4_298_NR_SMALL, 0, true> type; };
template <> struct GroupOf<1> { typedef G2Cfg3S<F298B, F298A, PCD_MNT6_298_A_SMALL, PCD_MNT6_298_NR_SMALL, 1, true> type; };
template <> struct GroupOf<2> { typedef G2Cfg2S<F753A, F753B, PCD_MNT4_753_A_SMALL, PCD_MNT4_753_NR_SMALL, 2, false> type; };
template <> struct GroupOf<3> { typedef G2Cfg3S<F753B, F753A, PCD_MNT6_753_A_SMALL, PCD_MNT6_753_NR_SMALL, 3, false> type; };
template <> struct GroupOf<4> { typedef G2Cfg2SMB<F753A, F753B, PCD_MNT4_753_A_SMALL, PCD_MNT4_753_NR_SMALL, 2> type; };
template <> struct GroupOf<5> { typedef G2Cfg3SMB<F753B, F753A, PCD_MNT6_753_A_SMALL, PCD_MNT6_753_NR_SMALL, 3> type; };

// words per item.  Towers: a, b and out are one element image each (T_FROM_ABI / T_ABI_ROUNDTRIP: the first ABI_WORDS <= WORDS words of a
// hold a C-ABI image, and T_ABI_ROUNDTRIP writes one into the first ABI_WORDS words of out; the rest keeps the sentinel).  Groups: p is X || Y || ZZ || ZZZ || flag (S_MADD_X) or X || Y || Z || flag;
// q is `steps` affine points (the two chains), one Jacobian record (J_ADD) or unused; out is always four coordinate slots (the fourth
// stays untouched for a Jacobian result) and one identity flag PER LANE of the item.
template <class T> static int tower_words() { return T::WORDS; }
template <class T> static int group_p_words(int op) { return (op == S_MADD_X ? 4 : 3) * T::WORDS + 1; }
template <class T> static int group_q_words(int op, int steps) { return op <= S_MADD_JAC ? steps * 2 * T::WORDS : op == J_ADD ? 3 * T::WORDS + 1 : 0; }
template <class T> static int group_out_words() { return 4 * T::WORDS + T::LANES; }

// the item of this lane, or -1: lanes past the last whole item of the wave, items past the list, inactive items
template <int L> __device__ __forceinline__ int my_item(int n_items, const uint8_t* active) {
  constexpr int PER = 64 / L;
  if ((int)threadIdx.x >= PER * L) return -1;
  const int item = (int)blockIdx.x * PER + (int)threadIdx.x / L;
  if (item >= n_items || active[item] == 0) return -1;
  return item;
}
template <class T> __device__ __forceinline__ unsigned my_role() { return (threadIdx.x & 63u) % (unsigned)T::LANES; }

template <class G, int OP>
__global__ void __launch_bounds__(64) tower_kernel(const uint32_t* a, const uint32_t* b, uint32_t k, int n_items, const uint8_t* active, uint32_t* out, uint32_t* ran) {
  typedef typename G::F T;
  typedef typename T::Base F;
  const int item = my_item<T::LANES>(n_items, active);
  if (item < 0) return;
  a += (size_t)item * T::WORDS; b += (size_t)item * T::WORDS; out += (size_t)item * T::WORDS;
  if constexpr (OP == T_FROM_ABI) { T::from_abi(a).store(out); }
  else if constexpr (OP == T_ABI_ROUNDTRIP) { T::from_abi(a).to_abi(out); }
  else if constexpr (OP == T_ONE) { T::one().store(out); }
  else {
    const T x = T::load(a), y = T::load(b);
    T r = T::zero();
    if constexpr (OP == T_MUL) r = x * y;
    else if constexpr (OP == T_SQR) r = x.sqr();
    else if constexpr (OP == T_ADD) r = x + y;
    else if constexpr (OP == T_SUB) r = x - y;
    else if constexpr (OP == T_NEG) r = x.neg();
    else if constexpr (OP == T_DBL) r = x.dbl();
    else if constexpr (OP == T_MUL_SMALL) r = x.mul_small(k);
    else if constexpr (OP == T_MUL_BY_A) r = G::mul_by_a(x);
    else if constexpr (OP == T_IS_ZERO) r.c.v[0] = x.is_zero() ? 1u : 0u;          // (word 0 of every lane's own coefficient slot)
    else if constexpr (OP == T_IS_RAW_ZERO) r.c.v[0] = x.is_raw_zero() ? 1u : 0u;
    else if constexpr (OP == T_EQ) { r.c.v[0] = (x == y) ? 1u : 0u; r.c.v[1] = (x != y) ? 1u : 0u; }
    r.store(out);
  }
  atomicAdd(ran, 1u);
}

template <class G, int OP>
__global__ void __launch_bounds__(64) group_kernel(const uint32_t* p, const uint32_t* q, int steps, int n_items, const uint8_t* active, uint32_t* out, uint32_t* ran) {
  typedef typename G::F T;
  typedef EC<G> E;
  typedef Jac<T> J;
  constexpr int W = T::WORDS;
  const int item = my_item<T::LANES>(n_items, active);
  if (item < 0) return;
  out += (size_t)item * (4 * W + T::LANES);
  uint32_t* flag = out + 4 * W + my_role<T>();
  if constexpr (OP == S_MADD_X) {
    p += (size_t)item * (4 * W + 1); q += (size_t)item * steps * 2 * W;
    typename E::AccX a = {T::load(p), T::load(p + W), T::load(p + 2 * W), T::load(p + 3 * W)};
    if (p[4 * W] != 0) a = E::x_infinity();
    for (int s = 0; s < steps; s++) a = E::madd_x(a, Aff<T>::load(q + (size_t)s * 2 * W));
    a.X.store(out); a.Y.store(out + W); a.ZZ.store(out + 2 * W); a.ZZZ.store(out + 3 * W);
    *flag = a.is_inf() ? 1u : 0u;
  } else {
    p += (size_t)item * (3 * W + 1);
    J a = J::load(p);
    if (p[3 * W] != 0) a = J::infinity();
    if constexpr (OP == S_MADD_JAC) {
      q += (size_t)item * steps * 2 * W;
      for (int s = 0; s < steps; s++) a = E::madd(a, Aff<T>::load(q + (size_t)s * 2 * W));
    } else if constexpr (OP == J_ADD) {
      q += (size_t)item * (3 * W + 1);
      J c = J::load(q);
      if (q[3 * W] != 0) c = J::infinity();
      a = E::add(a, c);
    } else if constexpr (OP == J_DBL) {
      a = E::dbl(a);
    } else {
      a = E::x_to_jac(E::x_from(a));
    }
    a.store(out);
    *flag = a.is_inf() ? 1u : 0u;
  }
  atomicAdd(ran, 1u);
}

// the operands, the active flags, the sentinel-filled output and the lane counter on the device around one launch
struct Run {
  uint32_t *a = nullptr, *b = nullptr, *out = nullptr, *ran = nullptr;
  uint8_t* act = nullptr;
  size_t out_words;
  bool ok = true;
  Run(const void* ha, size_t a_words, const void* hb, size_t b_words, const uint8_t* hact, int n_items, size_t out_words_) : out_words(out_words_) {
    ok = hipMalloc(&a, (a_words + 1) * 4) == hipSuccess && hipMalloc(&b, (b_words + 1) * 4) == hipSuccess && hipMalloc(&act, (size_t)n_items) == hipSuccess &&
         hipMalloc(&out, (out_words + 1) * 4) == hipSuccess && hipMalloc(&ran, 4) == hipSuccess;
    if (!ok) return;
    const std::vector<uint32_t> fill(out_words + 1, SENTINEL);
    ok = hipMemcpy(a, ha, a_words * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(b, hb, b_words * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(act, hact, (size_t)n_items, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(out, fill.data(), (out_words + 1) * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(ran, 0, 4) == hipSuccess;
  }
  int finish(uint32_t* hout, uint32_t* hran) {
    int rc = ok ? 0 : -2;
    if (ok && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = -3;
    if (rc == 0 && (hipMemcpy(hout, out, out_words * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hran, ran, 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = -4;
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(act); (void)hipFree(out); (void)hipFree(ran);
    return rc;
  }
};
template <int L> static dim3 blocks(int n_items) { return dim3((unsigned)((n_items + 64 / L - 1) / (64 / L))); }

template <class G, int OP>
static int launch_tower(const uint32_t* a, const uint32_t* b, uint32_t k, int n, const uint8_t* act, uint32_t* out, uint32_t* ran) {
  typedef typename G::F T;
  Run r(a, (size_t)n * T::WORDS, b, (size_t)n * T::WORDS, act, n, (size_t)n * T::WORDS);
  if (r.ok) hipLaunchKernelGGL((tower_kernel<G, OP>), blocks<T::LANES>(n), dim3(64), 0, 0, r.a, r.b, k, n, r.act, r.out, r.ran);
  return r.finish(out, ran);
}
template <class G>
static int run_tower(int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, const uint8_t* act, uint32_t* out, uint32_t* ran) {
  switch (op) {
#define LS_CASE(OP) case OP: return launch_tower<G, OP>(a, b, k, n, act, out, ran);
    LS_CASE(T_MUL) LS_CASE(T_SQR) LS_CASE(T_ADD) LS_CASE(T_SUB) LS_CASE(T_NEG) LS_CASE(T_DBL) LS_CASE(T_MUL_SMALL) LS_CASE(T_MUL_BY_A)
    LS_CASE(T_IS_ZERO) LS_CASE(T_IS_RAW_ZERO) LS_CASE(T_EQ) LS_CASE(T_ONE) LS_CASE(T_FROM_ABI) LS_CASE(T_ABI_ROUNDTRIP)
#undef LS_CASE
    default: return -1;
  }
}
template <class G, int OP>
static int launch_group(const uint32_t* p, const uint32_t* q, int steps, int n, const uint8_t* act, uint32_t* out, uint32_t* ran) {
  typedef typename G::F T;
  Run r(p, (size_t)n * group_p_words<T>(OP), q, (size_t)n * group_q_words<T>(OP, steps), act, n, (size_t)n * group_out_words<T>());
  if (r.ok) hipLaunchKernelGGL((group_kernel<G, OP>), blocks<T::LANES>(n), dim3(64), 0, 0, r.a, r.b, steps, n, r.act, r.out, r.ran);
  return r.finish(out, ran);
}
template <class G>
static int run_group(int op, const uint32_t* p, const uint32_t* q, int steps, int n, const uint8_t* act, uint32_t* out, uint32_t* ran) {
  switch (op) {
    case S_MADD_X: return launch_group<G, S_MADD_X>(p, q, steps, n, act, out, ran);
    case S_MADD_JAC: return launch_group<G, S_MADD_JAC>(p, q, steps, n, act, out, ran);
    case J_ADD: return launch_group<G, J_ADD>(p, q, steps, n, act, out, ran);
    case J_DBL: return launch_group<G, J_DBL>(p, q, steps, n, act, out, ran);
    case X_ROUNDTRIP: return launch_group<G, X_ROUNDTRIP>(p, q, steps, n, act, out, ran);
    default: return -1;
  }
}
// words per item of the three arrays of one call, so that the caller can size (and check) its buffers: what[0] = 0 towers, 1 groups
template <class G>
static void words_of(int what, int op, int steps, int* w3) {
  typedef typename G::F T;
  if (what == 0) { w3[0] = w3[1] = w3[2] = tower_words<T>(); }
  else { w3[0] = group_p_words<T>(op); w3[1] = group_q_words<T>(op, steps); w3[2] = group_out_words<T>(); }
}

// each part's entry points (id: the type / group number above, of the two this part holds)
#define LS_PART_ENTRIES(SUFFIX, ID_A, ID_B)                                                                                                                  \
  int ls_tower_##SUFFIX(int id, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, const uint8_t* act, uint32_t* out, uint32_t* ran) {          \
    return id == ID_A ? run_tower<GroupOf<ID_A>::type>(op, a, b, k, n, act, out, ran) : run_tower<GroupOf<ID_B>::type>(op, a, b, k, n, act, out, ran);       \
  }                                                                                                                                                          \
  int ls_group_##SUFFIX(int id, int op, const uint32_t* p, const uint32_t* q, int steps, int n, const uint8_t* act, uint32_t* out, uint32_t* ran) {           \
    return id == ID_A ? run_group<GroupOf<ID_A>::type>(op, p, q, steps, n, act, out, ran) : run_group<GroupOf<ID_B>::type>(op, p, q, steps, n, act, out, ran); \
  }
#define LS_PART_DECLS(SUFFIX)                                                                                                                       \
  int ls_tower_##SUFFIX(int id, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, const uint8_t* act, uint32_t* out, uint32_t* ran); \
  int ls_group_##SUFFIX(int id, int op, const uint32_t* p, const uint32_t* q, int steps, int n, const uint8_t* act, uint32_t* out, uint32_t* ran);

#if LANESPLIT_PART == 0
LS_PART_DECLS(753a)
LS_PART_DECLS(753b)
LS_PART_ENTRIES(298, 0, 1)
extern "C" int gc_split_tower_ops(int type, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n_items, const uint8_t* active, uint32_t* out, uint32_t* ran) {
  if (n_items <= 0 || op < 0 || op >= T_OPS || type < 0 || type > 5) return -1;
  if (type < 2) return ls_tower_298(type, op, a, b, k, n_items, active, out, ran);
  return (type & 1) == 0 ? ls_tower_753a(type, op, a, b, k, n_items, active, out, ran) : ls_tower_753b(type, op, a, b, k, n_items, active, out, ran);
}
extern "C" int gc_split_group_ops(int group, int op, const uint32_t* p, const uint32_t* q, int steps, int n_items, const uint8_t* active, uint32_t* out, uint32_t* ran) {
  if (n_items <= 0 || op < 0 || op >= G_OPS || group < 0 || group > 5 || (op <= S_MADD_JAC && steps <= 0)) return -1;
  if (group < 2) return ls_group_298(group, op, p, q, steps, n_items, active, out, ran);
  return (group & 1) == 0 ? ls_group_753a(group, op, p, q, steps, n_items, active, out, ran) : ls_group_753b(group, op, p, q, steps, n_items, active, out, ran);
}
// words per item of (first operand, second operand, output) of one call: what = 0 gc_split_tower_ops, 1 gc_split_group_ops; and the sentinel
extern "C" int gc_split_words(int what, int id, int op, int steps, int* w3) {
  if (what < 0 || what > 1 || id < 0 || id > 5 || op < 0 || op >= (what == 0 ? (int)T_OPS : (int)G_OPS)) return -1;
  switch (id) {
    case 0: words_of<GroupOf<0>::type>(what, op, steps, w3); break;
    case 1: words_of<GroupOf<1>::type>(what, op, steps, w3); break;
    case 2: words_of<GroupOf<2>::type>(what, op, steps, w3); break;
    case 3: words_of<GroupOf<3>::type>(what, op, steps, w3); break;
    case 4: words_of<GroupOf<4>::type>(what, op, steps, w3); break;
    default: words_of<GroupOf<5>::type>(what, op, steps, w3); break;
  }
  return 0;
}
extern "C" uint32_t gc_split_sentinel() { return SENTINEL; }
#elif LANESPLIT_PART == 1
LS_PART_ENTRIES(753a, 2, 4)
#else
LS_PART_ENTRIES(753b, 3, 5)
#endif
