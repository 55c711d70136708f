// What the capi_*.hip units of libpcdhip.so share among themselves (common.h is what they share with the inst_*.hip units): the static
// facts about the four fields and curves, the error plumbing of the C ABI, the workspace slots, the one host-side field dispatch, and
// the helpers that cross a unit boundary -- each declared here once, under the unit that defines it.
#pragma once
#include <string.h>

#include <algorithm>
#include <new>

#include "common.h"

namespace pcd {

const int kFieldLimbs[4] = {5, 5, 12, 12};
const int kCurveFq[4] = {0, 1, 2, 3};
const int kCurveFr[4] = {1, 0, 3, 2};
const int kCurveG2Deg[4] = {2, 3, 2, 3};

inline bool valid_curve(int c) { return c >= 0 && c < 4; }
inline bool valid_field(int f) { return f >= 0 && f < 4; }
inline bool valid_group(int g) { return g == 1 || g == 2; }

// nothing may throw across the C ABI: bodies that use std containers run inside guarded()
template <class Fn>
int guarded(Fn&& body) {
  try { return body(); }
  catch (const std::bad_alloc&) { return PCDHIP_E_OOM; }
  catch (...) { return PCDHIP_E_HIP; }
}

inline int fail(pcdhip_ctx* ctx, hipError_t e) {
  if (ctx) { try { ctx->last_hip_error = hipGetErrorString(e); } catch (...) {} }
  if (e == hipErrorOutOfMemory) return PCDHIP_E_OOM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return PCDHIP_E_NO_DEVICE;
  if (e == hipErrorInvalidValue) return PCDHIP_E_ARG;
  return PCDHIP_E_HIP;
}
#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(ctx, e_); } while (0)
#define BIND() do { hipError_t e_ = hipSetDevice(ctx->device); if (e_ != hipSuccess) return fail(ctx, e_); } while (0)

enum { AUX_FFT_X = 0, AUX_FFT_TMP, AUX_A, AUX_B, AUX_C, AUX_Z, AUX_CSR_RP, AUX_CSR_COL, AUX_CSR_COEF, AUX_SCAL, AUX_OUT,
       AUX_G16, AUX_Z_CANON, AUX_H_CANON, AUX_MISC, AUX_FB_TABLE, AUX_FB_JAC, AUX_FB_OUT };

// Evaluation domain as ark-poly `GeneralEvaluationDomain::new(min_size)` picks it: radix-2 when 2^ceil(log2 min_size)
// fits the field's 2-adicity, otherwise the mixed-radix size 2^a q^b (b <= 2) of `best_mixed_domain_size`.
struct Dom { uint32_t n, m; int a; };

// The one host-side dispatch from a field id (0..3) to the library's host-callable field template: `fn` is a generic callable that gets
// a FieldTag and names the field as `typename decltype(tag)::type` (no allocation, nothing virtual: the four calls are instantiated here).
template <class T> struct FieldTag { typedef T type; };
template <class Fn>
void with_host_field(int field_id, Fn&& fn) {
  switch (field_id) {
    case 0: fn(FieldTag<Fp<F298A, false>>()); break;
    case 1: fn(FieldTag<Fp<F298B, false>>()); break;
    case 2: fn(FieldTag<Fp<F753A, false>>()); break;
    default: fn(FieldTag<Fp<F753B, false>>()); break;
  }
}

// ---- capi_core.hip
typedef hipError_t (*G1ScaleFn)(hipStream_t, const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t*);
G1ScaleFn g1_scale_entry(int curve_id);

// ---- capi_msm.hip
hipError_t zero_flagged(hipStream_t st, uint32_t* pts_dev, uint8_t* flags_dev, const uint8_t* flags_host, size_t n, size_t point_bytes);
void shard_range(size_t n, size_t g, size_t parts, size_t* lo, size_t* hi);
int bases_upload_single(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xy, const uint8_t* inf, size_t n, pcdhip_bases** out);
int msm_common(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint32_t* scalars_dev, size_t n, uint64_t* out_xyz,
               bool out_on_device = false);
int ensure_side_streams(pcdhip_ctx* ctx);
int drop_side_streams(pcdhip_ctx* ctx, bool partial);
bool pipe_pending(const pcdhip_ctx* ctx);
void drain_peers(pcdhip_ctx* ctx);

// ---- capi_msm_short.hip (the caller has bound the device; PCDHIP_E_ARG for a sharded handle or a range beyond the vector)
int msm_short_common(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint32_t* scalars_dev, size_t n, uint64_t* out_xyz);
// the same without the copy to the host and its wait: one Jacobian point in the device image at out_dev (device memory), 1 <= n <=
// MSM_SHORT_MAX_N; for scalars known to be reduced (the error word is not read)
int msm_short_async(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint32_t* scalars_dev, size_t n, uint32_t* out_dev);
int msm_short_host(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars, size_t n, uint64_t* out_xyz);
// k independent short MSMs over one handle as ONE chain of at most three launches on the context's stream (msm_short.hip.h, "the batched
// form"): item j's Jacobian point (device image) lands at out_dev + items[j].out_slot * out_stride_words; the slot of an item with n == 0
// is left as it is (the caller has zeroed it).  Asynchronous, no host wait: the descriptor table is staged by one hipMemcpyAsync into
// ctx->short_ws, whose first word is the call's error word afterwards (*err_dev, optional).  Any k; *launches (optional) = kernels launched
int msm_short_batch_async(pcdhip_ctx* ctx, const pcdhip_bases* bases, const MsmShortBatchIn* items, size_t k, uint32_t* out_dev,
                          size_t out_stride_words, const uint32_t** err_dev = nullptr, uint32_t* launches = nullptr);

// ---- capi_fft.hip
int pick_domain(int field_id, size_t min_size, Dom* d);
int split_domain(int field_id, size_t n, Dom* d);  // n = m * 2^a with m in {1, q, q^2}?  PCDHIP_E_ARG for 0 and n >= 2^31, else E_SIZE_UNSUPPORTED
int get_tables(pcdhip_ctx* ctx, int field_id, int log_n, const FftTables** out);
int get_mixed_tables(pcdhip_ctx* ctx, int field_id, const Dom& d, const FftTables** out);
int domain_transform(pcdhip_ctx* ctx, int field_id, const Dom& d, uint32_t* v, uint32_t* tmp, int inverse, int coset, float* pass_ms,
                     int* npasses);

// ---- capi_witness.hip
size_t csr_bytes(const pcdhip_csr* m, const FieldEntry& fe, size_t off[6]);
int validate_csr(const pcdhip_csr* m, size_t num_cols);
int upload_csr_to(pcdhip_ctx* ctx, const pcdhip_csr* m, const FieldEntry& fe, size_t num_cols, char* d, DevCsr* out);
int upload_csr(pcdhip_ctx* ctx, int slot, const pcdhip_csr* m, const FieldEntry& fe, size_t num_cols, DevCsr* out);
int upload_three(pcdhip_ctx* ctx, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, const FieldEntry& fe, size_t num_vars,
                 DevCsr out[3]);
int witness_chain_dev(pcdhip_ctx* ctx, int field_id, const DevCsr& mat, int k, const uint32_t* z_dev, size_t num_inputs, const Dom& d, int slot,
                      bool transforms = true);
int witness_finish_dev(pcdhip_ctx* ctx, int field_id, const Dom& d, const uint32_t* b_at = nullptr, const uint32_t* c_at = nullptr);
int witness_map_dev(pcdhip_ctx* ctx, int field_id, const DevCsr mats[3], const uint32_t* z_dev, size_t num_inputs, Dom* dom_out,
                    hipEvent_t after_spmv = nullptr);

// ---- capi_setup.hip
struct HostCsrT {
  std::vector<uint64_t> rp;
  std::vector<uint32_t> col;
  std::vector<uint64_t> coeff;
  pcdhip_csr view;
};
int transpose_csr(const pcdhip_csr* m, size_t cols, size_t limbs, HostCsrT* t, const uint32_t* perm = nullptr, size_t rows_out = 0);

// ---- capi_verify.hip
void negate_point(int curve_id, int group_id, uint64_t* xy);
bool scalars_reduced(int fr, const uint64_t* x, size_t count);  // every element's limbs, as an integer, below the modulus of field `fr`
void scalar_lincomb(int fr, const uint64_t* const* a, const uint64_t* const* b, size_t n, uint64_t* out);

}  // namespace pcd

// the prepared verifying key (capi_verify.hip): the one handle type that the inst_*.hip units never see, hence not in common.h
struct pcdhip_pvk {
  int curve_id = 0;
  size_t num_inputs = 0;
  std::vector<uint64_t> alpha, beta, neg_gamma, neg_delta, gamma_abc, alpha_beta /* e(alpha, beta) */, gt_one;
  std::vector<uint8_t> gamma_abc_inf;
  pcdhip_bases* abc = nullptr;  // gamma_abc_g1 resident (no precomputed copies; used when there are too many inputs for window tables)
  // prepared inputs (fixed_base.hip.h): gamma_abc_g1 in the C-ABI image with flagged points zeroed, then one window table per
  // gamma_abc_g1[j], j >= 1 -- one device block; null when the key has more than PVK_TABLE_INPUTS inputs
  uint32_t* abc_dev = nullptr;
  size_t abc_tables_off = 0;  // u32 words from abc_dev to the tables
};
constexpr size_t PVK_TABLE_INPUTS = 256;

// the prepared verifier key of the MarlinKZG10 check (capi_kzg_check.hip), likewise unseen by the inst_*.hip units
struct pcdhip_kzg_vk {
  int curve_id = 0;
  size_t n_shift = 0;
  bool has_gamma = false;
  // the check's vector in the device image, room for the short MSM's limit of points: g, gamma_g, the shift powers (resident), then a
  // call's commitments, shifted commitments and witnesses.  `vec` is the handle the short MSM takes: its n and its infinity bitmap are
  // set per call (the bitmap arrives with the call's upload); head_inf = the bits of the resident part
  uint32_t* vec_dev = nullptr;
  pcdhip_bases vec = {};
  std::vector<uint32_t> head_inf;
  // one block laid out once for the most equations a call may have: (h, beta_h) per equation, resident | the pairing's G1 slots | their
  // Z | Miller values | GT results | Jacobian points in the C-ABI image (lane-per-pairing mode) -- byte offsets
  void* pair = nullptr;
  size_t o_g2 = 0, o_g1 = 0, o_z = 0, o_f = 0, o_gt = 0, o_jac = 0;
  void* scratch = nullptr;  // a call's upload, its column scalars and MSM results; grows to the largest call seen
  size_t scratch_bytes = 0;
  std::vector<uint64_t> stage;   // the host image of the last call's upload (it outlives the staging copy)
  std::vector<uint64_t> gt_one;
};
