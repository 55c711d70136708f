// TEST HARNESS ONLY (never part of libpcdhip.so): the gfx950 build of the field arithmetic of pcd_amd/csrc/fp.hip.h and of the lazily
// reduced addition steps of ec.hip.h, operation by operation on RAW limb images, one element per lane in blocks of 64 lanes (the
// mailbox variant's LDS slots are per lane of one wave).  The per-element code is tests/gpucheck/fieldops_ops.h, shared with the host
// build; the expected values are Python integers (tests/field_reference.py).  Every kernel counts the elements it processed in `ran`.
// variant: 0 the inlined products (all fields), 1 the non-inlined mul_call / sqr_call bodies, 2 the LDS mailbox form (753-bit fields).
// Built by __graft_entry__.build() (hipcc, gfx950) into tests/gpucheck/libgpucheck_fp.so; tests/test_gpu_field_ops.py drives it.
// One source, five translation units (-DFIELDOPS_PART=0..4, tests/gpucheck/Makefile) so that they compile side by side: 0 the 298-bit fields,
// their Lz family and towers; 1 / 2 the three variants and the tower of the 753-bit fields A / B; 3 the accumulator steps of the 298-bit
// groups; 4 those of the 753-bit G1 groups in their mailbox form.
#include "fieldops_ops.h"
#ifndef FIELDOPS_PART
#error "compile with -DFIELDOPS_PART=0..4"
#endif
using namespace pcd;
using namespace fieldops;

template <class F>
__global__ void __launch_bounds__(64) field_kernel(int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  field_op<F>(op, a + (size_t)i * field_a_words<F>(op, k), b + (size_t)i * field_b_words<F>(op, k), k, out + (size_t)i * F::N);
  atomicAdd(ran, 1u);
}
template <class F>
__global__ void __launch_bounds__(64) lz_kernel(int op, const int32_t* ops, int32_t k, int n, uint32_t* out, uint32_t* ran) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  lz_op<F>(op, ops + (size_t)i * 8 * F::N, k, out + (size_t)i * F::N);
  atomicAdd(ran, 1u);
}
template <class T>
__global__ void __launch_bounds__(64) tower_kernel(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  tower_op<T>(op, a + (size_t)i * T::WORDS, b + (size_t)i * T::WORDS, out + (size_t)i * T::WORDS);
  atomicAdd(ran, 1u);
}
template <class G>
__global__ void __launch_bounds__(64) step_kernel(int op, const uint32_t* acc, const uint32_t* q, int steps, int n, uint32_t* out, uint32_t* ran) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  madd_steps<G>(op, acc + (size_t)i * step_words<G>(op), q + (size_t)i * steps * 2 * G::F::WORDS, steps, out + (size_t)i * step_words<G>(op));
  atomicAdd(ran, 1u);
}

// two input vectors and one output vector of words on the device around one launch; the element counter comes back in *ran
struct Run {
  uint32_t *a = nullptr, *b = nullptr, *out = nullptr, *ran = nullptr;
  size_t out_words;
  bool ok = true;
  Run(const void* ha, size_t a_words, const void* hb, size_t b_words, size_t out_words_) : out_words(out_words_) {
    ok = hipMalloc(&a, (a_words + 1) * 4) == hipSuccess && hipMalloc(&b, (b_words + 1) * 4) == hipSuccess &&
         hipMalloc(&out, (out_words + 1) * 4) == hipSuccess && hipMalloc(&ran, 4) == hipSuccess;
    if (!ok) return;
    ok = hipMemcpy(a, ha, a_words * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(b, hb, b_words * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(out, 0, out_words * 4) == hipSuccess && hipMemset(ran, 0, 4) == hipSuccess;
  }
  int finish(uint32_t* hout, uint32_t* hran) {
    int rc = ok ? 0 : -2;
    if (ok && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = -3;
    if (rc == 0 && (hipMemcpy(hout, out, out_words * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hran, ran, 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = -4;
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(out); (void)hipFree(ran);
    return rc;
  }
};
static dim3 blocks(int n) { return dim3((unsigned)((n + 63) / 64)); }

template <class F>
static int run_field(int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran) {
  Run r(a, (size_t)n * field_a_words<F>(op, k), b, (size_t)n * field_b_words<F>(op, k), (size_t)n * F::N);
  if (r.ok) hipLaunchKernelGGL((field_kernel<F>), blocks(n), dim3(64), 0, 0, op, r.a, r.b, k, n, r.out, r.ran);
  return r.finish(out, ran);
}
template <class F>
static int run_lz(int op, const int32_t* ops, int32_t k, int n, uint32_t* out, uint32_t* ran) {
  Run r(ops, (size_t)n * 8 * F::N, ops, 0, (size_t)n * F::N);
  if (r.ok) hipLaunchKernelGGL((lz_kernel<F>), blocks(n), dim3(64), 0, 0, op, (const int32_t*)r.a, k, n, r.out, r.ran);
  return r.finish(out, ran);
}
template <class T>
static int run_tower(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran) {
  Run r(a, (size_t)n * T::WORDS, b, (size_t)n * T::WORDS, (size_t)n * T::WORDS);
  if (r.ok) hipLaunchKernelGGL((tower_kernel<T>), blocks(n), dim3(64), 0, 0, op, r.a, r.b, n, r.out, r.ran);
  return r.finish(out, ran);
}
template <class G>
static int run_step(int op, const uint32_t* acc, const uint32_t* q, int steps, int n, uint32_t* out, uint32_t* ran) {
  if (op == S_MADD_LZ && !LazyCapable<typename G::F>::value) return -1;
  if (op == fieldops::S_MADD_JAC && G::F::Base::INLINE_ARITH) return -1;
  Run r(acc, (size_t)n * step_words<G>(op), q, (size_t)n * steps * 2 * G::F::WORDS, (size_t)n * step_words<G>(op));
  if (r.ok) hipLaunchKernelGGL((step_kernel<G>), blocks(n), dim3(64), 0, 0, op, r.a, r.b, steps, n, r.out, r.ran);
  return r.finish(out, ran);
}

// the parts' entry points, each defined in one translation unit
int fo_field_753(int field, int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran);
int fo_tower_753(int field, int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran);
int fo_step_753(int curve, int op, const uint32_t* acc, const uint32_t* q, int steps, int n, uint32_t* out, uint32_t* ran);

#if FIELDOPS_PART == 0
extern "C" int gc_field_ops(int field, int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran) {
  if (n <= 0 || op < 0 || op >= F_OPS || (op == F_SIGNED_SUM && (k == 0 || k > SIGNED_SUM_MAX_TERMS))) return -1;
  if (field == 0 && variant == 0) return run_field<Fp<F298A, true>>(op, a, b, k, n, out, ran);
  if (field == 1 && variant == 0) return run_field<Fp<F298B, true>>(op, a, b, k, n, out, ran);
  if ((field == 2 || field == 3) && variant >= 0 && variant < 3) return fo_field_753(field, variant, op, a, b, k, n, out, ran);
  return -1;
}
extern "C" int gc_lz_ops(int field, int op, const int32_t* ops, int32_t k, int n, uint32_t* out, uint32_t* ran) {
  if (n <= 0 || op < 0 || op >= L_OPS) return -1;
  if (field == 0) return run_lz<Fp<F298A, true>>(op, ops, k, n, out, ran);
  if (field == 1) return run_lz<Fp<F298B, true>>(op, ops, k, n, out, ran);
  return -1;
}
extern "C" int gc_tower_ops(int field, int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran) {
  if (n <= 0 || op < 0 || op >= T_OPS) return -1;
  if (field == 0) return run_tower<Tower0>(op, a, b, n, out, ran);
  if (field == 1) return run_tower<Tower1>(op, a, b, n, out, ran);
  if (field == 2 || field == 3) return fo_tower_753(field, op, a, b, n, out, ran);
  return -1;
}
#elif FIELDOPS_PART == 1 || FIELDOPS_PART == 2
#if FIELDOPS_PART == 1
typedef F753A PartP; typedef Tower2 PartT;
int fo_field_753b(int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran);
int fo_tower_753b(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran);
#else
typedef F753B PartP; typedef Tower3 PartT;
#endif
static int part_field(int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran) {
  if (variant == 0) return run_field<Fp<PartP, true>>(op, a, b, k, n, out, ran);
  if (variant == 1) return run_field<Fp<PartP, false>>(op, a, b, k, n, out, ran);
  return run_field<Fp<PartP, false, true>>(op, a, b, k, n, out, ran);
}
#if FIELDOPS_PART == 1
int fo_field_753(int field, int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran) {
  return field == 2 ? part_field(variant, op, a, b, k, n, out, ran) : fo_field_753b(variant, op, a, b, k, n, out, ran);
}
int fo_tower_753(int field, int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran) {
  return field == 2 ? run_tower<PartT>(op, a, b, n, out, ran) : fo_tower_753b(op, a, b, n, out, ran);
}
#else
int fo_field_753b(int variant, int op, const uint32_t* a, const uint32_t* b, uint32_t k, int n, uint32_t* out, uint32_t* ran) {
  return part_field(variant, op, a, b, k, n, out, ran);
}
int fo_tower_753b(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out, uint32_t* ran) { return run_tower<PartT>(op, a, b, n, out, ran); }
#endif
#elif FIELDOPS_PART == 3
extern "C" int gc_madd_step(int curve, int grp, int op, const uint32_t* acc, const uint32_t* q, int steps, int n, uint32_t* out, uint32_t* ran) {
  if (n <= 0 || steps <= 0 || op < 0 || op >= S_OPS) return -1;
  switch (curve * 2 + grp - 1) {
    case 0: return run_step<G1_MNT4_298>(op, acc, q, steps, n, out, ran);
    case 1: return run_step<G2_MNT4_298>(op, acc, q, steps, n, out, ran);
    case 2: return run_step<G1_MNT6_298>(op, acc, q, steps, n, out, ran);
    case 3: return run_step<G2_MNT6_298>(op, acc, q, steps, n, out, ran);
    case 4: case 6: return op == S_MADD_JAC || op == S_MADD_X_PLAIN ? fo_step_753(curve, op, acc, q, steps, n, out, ran) : -1;
    default: return -1;
  }
}
#else
// the 27-limb G1 groups in the mailbox form their accumulation runs (ec.hip.h AccOf): EC::madd on a Jacobian record, and madd_x_plain (PCD_XYZZ_753)
int fo_step_753(int curve, int op, const uint32_t* acc, const uint32_t* q, int steps, int n, uint32_t* out, uint32_t* ran) {
  if (curve == 2) return run_step<G1CfgMB<F753A, F753B, PCD_MNT4_753_A_SMALL, 2>>(op, acc, q, steps, n, out, ran);
  return run_step<G1CfgMB<F753B, F753A, PCD_MNT6_753_A_SMALL, 3>>(op, acc, q, steps, n, out, ran);
}
#endif
