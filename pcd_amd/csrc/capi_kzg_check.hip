// ------------------------------------------------------------------------------------------------ K14: the MarlinKZG10 check on device
// (include/pcdhip.h states the equation.)  A prepared verifier key keeps g, gamma_g and the shift powers resident in the device image, in
// front of a range for a call's fresh points, and h, beta_h beside the pairing's slots; a call is one staged upload, the launches of
// kzg_check.hip.h around points_in, the batched short MSM and the pairing, one download and ONE wait -- the rule of verify_prepared_vm.
#include "capi_internal.h"
#include "kzg_check.hip.h"
#include "msm_short.hip.h"

using namespace pcd;

namespace pcd {
#define PCD_K14_DECL(c)                                                                                             \
  hipError_t pcd_kzg_check_scalars_##c(hipStream_t, const KzgCheckTables&, uint32_t* left, uint32_t* right);        \
  hipError_t pcd_kzg_check_pairs_##c(hipStream_t, const uint32_t* jac, uint32_t n, uint32_t* out, uint32_t* out_z);
PCD_K14_DECL(0) PCD_K14_DECL(1) PCD_K14_DECL(2) PCD_K14_DECL(3)
#undef PCD_K14_DECL
}  // namespace pcd

namespace {
constexpr size_t CHECK_MAX_OPENINGS = 64;          // E <= 64 equations: the pairing slots of a key are laid out once
constexpr size_t CHECK_MAX_POINTS = MSM_SHORT_MAX_N;  // the short MSM's limit
enum { AUX_CHECK_SCALARS = AUX_FB_OUT + 4 };       // (capi_kzg.hip's AUX_OPEN: pcdhip_kzg_check_scalars runs while no call of K7 / K13 does)

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
bool abi_is_zero(const uint64_t* x, size_t limbs) { uint64_t o = 0; for (size_t i = 0; i < limbs; i++) o |= x[i]; return o == 0; }

hipError_t scalars_entry(int curve_id, hipStream_t st, const KzgCheckTables& t, uint32_t* left, uint32_t* right) {
  switch (curve_id) {
    case 0: return pcd_kzg_check_scalars_0(st, t, left, right);
    case 1: return pcd_kzg_check_scalars_1(st, t, left, right);
    case 2: return pcd_kzg_check_scalars_2(st, t, left, right);
    default: return pcd_kzg_check_scalars_3(st, t, left, right);
  }
}
hipError_t pairs_entry(int curve_id, hipStream_t st, const uint32_t* jac, uint32_t n, uint32_t* out, uint32_t* out_z) {
  switch (curve_id) {
    case 0: return pcd_kzg_check_pairs_0(st, jac, n, out, out_z);
    case 1: return pcd_kzg_check_pairs_1(st, jac, n, out, out_z);
    case 2: return pcd_kzg_check_pairs_2(st, jac, n, out, out_z);
    default: return pcd_kzg_check_pairs_3(st, jac, n, out, out_z);
  }
}

// The tables of a call as the C ABI states them, and what the argument checks have found.
struct CheckArgs {
  int fr = 0;
  size_t m = 0, P = 0, n_shift = 0;
  const int32_t* shift_index = nullptr;
  const uint64_t *points = nullptr, *coeffs = nullptr, *scoeffs = nullptr, *values = nullptr, *random_v = nullptr, *item_values = nullptr,
                 *randomizers = nullptr;
  size_t E() const { return randomizers ? 1 : P; }
  size_t N() const { return 2 + n_shift + 2 * m + P; }
};
// -> PCDHIP_OK, PCDHIP_E_SIZE_UNSUPPORTED or PCDHIP_E_ARG; on the host, before anything is queued.  has_shifted: the call brought
// shifted commitments (the scalar collapse alone has no points and passes true)
int check_args(const CheckArgs& c, bool has_shifted) {
  if (c.P > CHECK_MAX_OPENINGS || c.m > CHECK_MAX_POINTS || c.n_shift > CHECK_MAX_POINTS || c.N() > CHECK_MAX_POINTS) return PCDHIP_E_SIZE_UNSUPPORTED;
  const size_t L = (size_t)kFieldLimbs[c.fr], cells = c.P * c.m;
  if (!scalars_reduced(c.fr, c.points, c.P) || !scalars_reduced(c.fr, c.values, c.P) || !scalars_reduced(c.fr, c.coeffs, cells)) return PCDHIP_E_ARG;
  if (c.random_v && !scalars_reduced(c.fr, c.random_v, c.P)) return PCDHIP_E_ARG;
  if (c.randomizers && !scalars_reduced(c.fr, c.randomizers, c.P)) return PCDHIP_E_ARG;
  if (!c.scoeffs) return PCDHIP_OK;
  if (!scalars_reduced(c.fr, c.scoeffs, cells)) return PCDHIP_E_ARG;
  for (size_t x = 0; x < cells; x++) {
    if (abi_is_zero(c.scoeffs + x * L, L)) continue;
    const size_t i = x % c.m;
    if (!has_shifted || !c.item_values || !c.shift_index || c.shift_index[i] < 0 || (size_t)c.shift_index[i] >= c.n_shift) return PCDHIP_E_ARG;
    if (!scalars_reduced(c.fr, c.item_values + x * L, 1)) return PCDHIP_E_ARG;
  }
  return PCDHIP_OK;
}
// where the tables sit in a call's upload, in bytes from `base` (256-byte aligned parts; an absent table has no room)
struct TableLayout { size_t a, s, v, idx, z, value, rv, rnd, end; };
TableLayout table_layout(const CheckArgs& c, size_t base) {
  const size_t eb = (size_t)kFieldLimbs[c.fr] * 8, cells = up256(c.P * c.m * eb), row = up256(c.P * eb);
  TableLayout t;
  t.a = base;
  t.s = t.a + cells;
  t.v = t.s + (c.scoeffs ? cells : 0);
  t.idx = t.v + (c.scoeffs ? cells : 0);
  t.z = t.idx + (c.scoeffs ? up256(c.m * 4) : 0);
  t.value = t.z + row;
  t.rv = t.value + row;
  t.rnd = t.rv + (c.random_v ? row : 0);
  t.end = t.rnd + (c.randomizers ? row : 0);
  return t;
}
// the host image of the tables (zeroed by the caller); an item value is copied only where s != 0 -- nothing else of that table is read
void stage_tables(const CheckArgs& c, const TableLayout& t, char* h) {
  const size_t L = (size_t)kFieldLimbs[c.fr], eb = L * 8, cells = c.P * c.m;
  if (cells) memcpy(h + t.a, c.coeffs, cells * eb);
  if (c.scoeffs) {
    if (cells) memcpy(h + t.s, c.scoeffs, cells * eb);
    for (size_t x = 0; x < cells; x++)
      if (!abi_is_zero(c.scoeffs + x * L, L)) memcpy(h + t.v + x * eb, c.item_values + x * L, eb);
    for (size_t i = 0; i < c.m; i++) ((int32_t*)(h + t.idx))[i] = c.shift_index ? c.shift_index[i] : -1;
  }
  memcpy(h + t.z, c.points, c.P * eb);
  memcpy(h + t.value, c.values, c.P * eb);
  if (c.random_v) memcpy(h + t.rv, c.random_v, c.P * eb);
  if (c.randomizers) memcpy(h + t.rnd, c.randomizers, c.P * eb);
}
KzgCheckTables device_tables(const CheckArgs& c, const TableLayout& t, const char* d) {
  auto at = [&](size_t off, bool present) { return present ? (const uint32_t*)(d + off) : nullptr; };
  KzgCheckTables k;
  k.a = at(t.a, true);
  k.s = at(t.s, c.scoeffs);
  k.v = at(t.v, c.scoeffs);
  k.shift_index = (const int32_t*)at(t.idx, c.scoeffs);
  k.z = at(t.z, true);
  k.value = at(t.value, true);
  k.random_v = at(t.rv, c.random_v);
  k.randomizers = at(t.rnd, c.randomizers);
  k.m = (uint32_t)c.m; k.P = (uint32_t)c.P; k.n_shift = (uint32_t)c.n_shift; k.E = (uint32_t)c.E();
  return k;
}
int curve_of_scalar_field(int fr) { return kCurveFr[fr]; }  // (the map is an involution: {1, 0, 3, 2})

// the key's per-call scratch: grown here, never shrunk (a key that has seen its largest call allocates nothing again)
int vk_scratch(pcdhip_ctx* ctx, pcdhip_kzg_vk* vk, size_t bytes) {
  if (bytes <= vk->scratch_bytes) return PCDHIP_OK;
  TRY(hipStreamSynchronize(ctx->stream));
  if (vk->scratch) { TRY(hipFree(vk->scratch)); vk->scratch = nullptr; vk->scratch_bytes = 0; }
  TRY(hipMalloc(&vk->scratch, bytes));
  vk->scratch_bytes = bytes;
  return PCDHIP_OK;
}
void gt_one(int curve_id, uint64_t* out /* zeroed */) {
  with_host_field(kCurveFq[curve_id], [&](auto fq) { decltype(fq)::type::one().to_abi((uint32_t*)out); });
}

// Everything of pcdhip_kzg_check_combinations behind its argument checks.
int kzg_check_run(pcdhip_ctx* ctx, pcdhip_kzg_vk* vk, const CheckArgs& c, const uint64_t* comm_xy, const uint8_t* comm_inf, const uint64_t* shifted_xy,
                  const uint8_t* shifted_inf, const uint64_t* w_xy, const uint8_t* w_inf, int* ok) {
  const int cid = vk->curve_id;
  const GroupEntry& ge = group_entry(cid, 1);
  const PairingEntry& pe = pairing_entry(cid);
  const size_t m = c.m, P = c.P, E = c.E(), N = c.N(), head = 2 + c.n_shift, fresh = 2 * m + P;
  const size_t l1 = (size_t)pcdhip_point_limbs(cid, 1), ab = l1 * 8, eb = (size_t)kFieldLimbs[c.fr] * 8;
  const size_t jw = (size_t)ge.point_words / 2 * 3, stride = (size_t)ge.base_stride_words;
  // the upload: fresh points (C-ABI) | the vector's infinity bitmap | the tables;  behind it: left scalars | right scalars | MSM results
  const size_t o_pts = 0, o_bits = o_pts + up256(fresh * ab);
  const TableLayout tl = table_layout(c, o_bits + up256(CHECK_MAX_POINTS / 8));
  const size_t up_bytes = tl.end, o_left = up_bytes, o_right = o_left + up256(E * N * eb), o_msm = o_right + up256(E * P * eb);
  int rc = vk_scratch(ctx, vk, o_msm + up256(2 * E * jw * 4));
  if (rc) return rc;
  char* d = (char*)vk->scratch;
  vk->stage.assign(up_bytes / 8, 0);
  char* h = (char*)vk->stage.data();
  uint32_t* bits = (uint32_t*)(h + o_bits);
  memcpy(bits, vk->head_inf.data(), vk->head_inf.size() * 4);
  // a flagged point, and one whose coordinates are all zero, stays (0, 0) and has its bit set: the planes skip it
  auto place = [&](size_t slot, const uint64_t* xy, const uint8_t* inf, size_t j) {
    if (!xy || (inf && inf[j]) || abi_is_zero(xy + j * l1, l1)) { bits[(head + slot) >> 5] |= 1u << ((head + slot) & 31); return; }
    memcpy(h + o_pts + slot * ab, xy + j * l1, ab);
  };
  for (size_t i = 0; i < m; i++) { place(i, comm_xy, comm_inf, i); place(m + i, shifted_xy, shifted_inf, i); }
  for (size_t o = 0; o < P; o++) place(2 * m + o, w_xy, w_inf, o);
  stage_tables(c, tl, h);
  hipStream_t st = ctx->stream;
  const bool vm = ctx->pairing_vm;
  if (vm && !ctx->vm_block[cid]) TRY(pe.vm_upload(st, &ctx->vm_block[cid], &ctx->vm_tables[cid]));  // (once per context; prepare has done it)
  TRY(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
  uint32_t launches = 0;
  TRY(ge.points_in(st, (const uint32_t*)(d + o_pts), (uint32_t)fresh, vk->vec.dptr + head * stride));
  launches++;
  uint32_t* left = (uint32_t*)(d + o_left);
  uint32_t* right = (uint32_t*)(d + o_right);
  uint32_t* msm_out = (uint32_t*)(d + o_msm);
  TRY(scalars_entry(cid, st, device_tables(c, tl, d), left, right));
  launches++;
  // 2 E short MSMs over the key's vector: item 2 e the left side of equation e, 2 e + 1 its right side (in per-opening mode W_e alone)
  vk->vec.n = N;
  vk->vec.inf_bits = (uint32_t*)(d + o_bits);
  const size_t sw = eb / 4;
  std::vector<MsmShortBatchIn> items(2 * E);
  for (size_t e = 0; e < E; e++) {
    items[2 * e] = {left + e * N * sw, 0u, (uint32_t)N, (uint32_t)(2 * e)};
    if (c.randomizers) items[2 * e + 1] = {right, (uint32_t)(head + 2 * m), (uint32_t)P, 1u};
    else items[2 * e + 1] = {right + (e * P + e) * sw, (uint32_t)(head + 2 * m + e), 1u, (uint32_t)(2 * e + 1)};
  }
  uint32_t chain = 0;  // (the scalars are reduced by construction: the error word is not read)
  rc = msm_short_batch_async(ctx, &vk->vec, items.data(), items.size(), msm_out, jw, nullptr, &chain);
  if (rc) return rc;
  launches += chain;
  // the pairing's slots of the key's block: g2 (h, beta_h per equation, resident) | g1 | z | Miller values | GT | Jacobian C-ABI points
  char* pb = (char*)vk->pair;
  uint32_t* g1 = (uint32_t*)(pb + vk->o_g1);
  uint32_t* g1z = (uint32_t*)(pb + vk->o_z);
  if (vm) {
    TRY(pairs_entry(cid, st, msm_out, (uint32_t)(2 * E), g1, g1z));
    launches++;
  } else {  // the lane-per-pairing kernels take affine points: one normalisation launch more, no wait
    uint32_t* jac_abi = (uint32_t*)(pb + vk->o_jac);
    TRY(pairs_entry(cid, st, msm_out, (uint32_t)(2 * E), jac_abi, nullptr));
    TRY(ge.to_affine(st, jac_abi, (uint32_t)(2 * E), g1));
    launches += 2;
  }
  TRY(pe.multi_pairing(st, g1, vm ? g1z : nullptr, (const uint32_t*)(pb + vk->o_g2), (uint32_t)E, 2, (uint32_t*)(pb + vk->o_f), (uint32_t*)(pb + vk->o_gt),
                       vm ? &ctx->vm_tables[cid] : nullptr));
  launches += 2;
  const size_t gw = vk->gt_one.size();
  std::vector<uint64_t> gt(E * gw);
  TRY(hipMemcpyAsync(gt.data(), pb + vk->o_gt, E * gw * 8, hipMemcpyDeviceToHost, st));
  TRY(hipStreamSynchronize(st));
  ctx->kzg_check_plan[0] = E;
  ctx->kzg_check_plan[1] = N;
  ctx->kzg_check_plan[2] = launches;
  ctx->kzg_check_plan[3] = 1;
  for (size_t e = 0; e < E; e++) ok[e] = memcmp(&gt[e * gw], vk->gt_one.data(), gw * 8) == 0 ? 1 : 0;
  return PCDHIP_OK;
}
}  // namespace

extern "C" {

int pcdhip_kzg_vk_prepare(pcdhip_ctx* ctx, int curve_id, const uint64_t* g_xy, const uint64_t* gamma_g_xy, const uint64_t* h_xy,
                          const uint64_t* beta_h_xy, const uint64_t* shift_powers_xy, size_t n_shift, pcdhip_kzg_vk** out) {
  return guarded([&]() -> int {
  if (!ctx || !valid_curve(curve_id) || !g_xy || !h_xy || !beta_h_xy || (n_shift && !shift_powers_xy) || !out) return PCDHIP_E_ARG;
  *out = nullptr;
  if (n_shift > CHECK_MAX_POINTS - 2) return PCDHIP_E_SIZE_UNSUPPORTED;
  BIND();
  const GroupEntry& ge = group_entry(curve_id, 1);
  const PairingEntry& pe = pairing_entry(curve_id);
  const size_t l1 = (size_t)pcdhip_point_limbs(curve_id, 1), l2 = (size_t)pcdhip_point_limbs(curve_id, 2), ab = l1 * 8, head = 2 + n_shift;
  const size_t slots = 2 * CHECK_MAX_OPENINGS;
  pcdhip_kzg_vk* vk = new pcdhip_kzg_vk();
  vk->curve_id = curve_id;
  vk->n_shift = n_shift;
  vk->has_gamma = gamma_g_xy != nullptr;
  vk->gt_one.assign((size_t)pe.gt_words / 2, 0);
  gt_one(curve_id, vk->gt_one.data());
  vk->o_g2 = 0;
  vk->o_g1 = vk->o_g2 + up256(slots * l2 * 8);
  vk->o_z = vk->o_g1 + up256(slots * ab);
  vk->o_f = vk->o_z + up256(slots * ab / 2);
  vk->o_gt = vk->o_f + up256(slots * (size_t)pe.gt_internal_words * 4);
  vk->o_jac = vk->o_gt + up256(CHECK_MAX_OPENINGS * (size_t)pe.gt_words * 4);
  const size_t pair_bytes = vk->o_jac + up256(slots * ab / 2 * 3);
  // the head of the vector in the C-ABI image, its flags, and (h, beta_h) once per equation
  std::vector<uint64_t> pts(head * l1, 0), g2s(slots * l2);
  vk->head_inf.assign(CHECK_MAX_POINTS / 32, 0u);
  auto place = [&](size_t slot, const uint64_t* xy) {
    if (!xy || abi_is_zero(xy, l1)) { vk->head_inf[slot >> 5] |= 1u << (slot & 31); return; }
    memcpy(&pts[slot * l1], xy, ab);
  };
  place(0, g_xy);
  place(1, gamma_g_xy);
  for (size_t k = 0; k < n_shift; k++) place(2 + k, shift_powers_xy + k * l1);
  for (size_t e = 0; e < CHECK_MAX_OPENINGS; e++) {
    memcpy(&g2s[2 * e * l2], h_xy, l2 * 8);
    memcpy(&g2s[(2 * e + 1) * l2], beta_h_xy, l2 * 8);
  }
  auto fail_with = [&](int rc) { pcdhip_kzg_vk_free(ctx, vk); return rc; };
  auto tryh = [&](hipError_t e) { return e == hipSuccess ? PCDHIP_OK : fail(ctx, e); };
  int rc = tryh(hipMalloc((void**)&vk->vec_dev, CHECK_MAX_POINTS * (size_t)ge.base_stride_words * 4));
  rc = rc ? rc : tryh(hipMalloc(&vk->pair, pair_bytes));
  // room for a Marlin-sized round from the start (21 items, 2 openings, both optional tables); larger calls grow it once
  rc = rc ? rc : vk_scratch(ctx, vk, std::max<size_t>(up256(head * ab), 1u << 20));
  if (rc) return fail_with(rc);
  vk->vec.curve_id = curve_id; vk->vec.group_id = 1; vk->vec.n = head; vk->vec.dptr = vk->vec_dev; vk->vec.c = 0; vk->vec.groups = 1;
  hipStream_t st = ctx->stream;
  rc = tryh(hipMemsetAsync(vk->vec_dev, 0, CHECK_MAX_POINTS * (size_t)ge.base_stride_words * 4, st));
  rc = rc ? rc : tryh(hipMemcpyAsync(vk->scratch, pts.data(), head * ab, hipMemcpyHostToDevice, st));
  rc = rc ? rc : tryh(ge.points_in(st, (const uint32_t*)vk->scratch, (uint32_t)head, vk->vec_dev));
  rc = rc ? rc : tryh(hipMemcpyAsync((char*)vk->pair + vk->o_g2, g2s.data(), slots * l2 * 8, hipMemcpyHostToDevice, st));
  rc = rc ? rc : tryh(hipStreamSynchronize(st));
  if (!rc && ctx->pairing_vm && !ctx->vm_block[curve_id]) rc = tryh(pe.vm_upload(st, &ctx->vm_block[curve_id], &ctx->vm_tables[curve_id]));
  if (rc) return fail_with(rc);
  *out = vk;
  return PCDHIP_OK;
  });
}

void pcdhip_kzg_vk_free(pcdhip_ctx* ctx, pcdhip_kzg_vk* vk) {
  if (!vk) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  if (vk->vec_dev) (void)hipFree(vk->vec_dev);
  if (vk->pair) (void)hipFree(vk->pair);
  if (vk->scratch) (void)hipFree(vk->scratch);
  delete vk;
}

int pcdhip_kzg_check_scalars(pcdhip_ctx* ctx, int field_id, size_t n_shift, size_t m, const int32_t* shift_index, size_t n_openings,
                             const uint64_t* points_mont, const uint64_t* coeffs_mont, const uint64_t* shifted_coeffs_mont,
                             const uint64_t* values_mont, const uint64_t* random_v_mont, const uint64_t* item_values_mont,
                             const uint64_t* randomizers_canonical, uint64_t* left_canonical, uint64_t* right_canonical) {
  return guarded([&]() -> int {
  const size_t P = n_openings;
  if (!ctx || !valid_field(field_id) || (P && (!points_mont || !values_mont || !left_canonical || !right_canonical || (m && !coeffs_mont))))
    return PCDHIP_E_ARG;
  if (P == 0) return PCDHIP_OK;
  CheckArgs c;
  c.fr = field_id; c.m = m; c.P = P; c.n_shift = n_shift; c.shift_index = shift_index;
  c.points = points_mont; c.coeffs = coeffs_mont; c.scoeffs = m ? shifted_coeffs_mont : nullptr; c.values = values_mont; c.random_v = random_v_mont;
  c.item_values = item_values_mont; c.randomizers = randomizers_canonical;
  int rc = check_args(c, true);
  if (rc) return rc;
  BIND();
  const size_t eb = (size_t)kFieldLimbs[field_id] * 8, E = c.E(), N = c.N();
  const TableLayout tl = table_layout(c, 0);
  const size_t o_left = tl.end, o_right = o_left + up256(E * N * eb), total = o_right + up256(E * P * eb);
  TRY(ctx->aux_ws.ensure(AUX_CHECK_SCALARS, total));
  char* d = (char*)ctx->aux_ws.buf[AUX_CHECK_SCALARS];
  std::vector<uint64_t> host(tl.end / 8, 0);
  stage_tables(c, tl, (char*)host.data());
  TRY(hipMemcpyAsync(d, host.data(), tl.end, hipMemcpyHostToDevice, ctx->stream));
  TRY(scalars_entry(curve_of_scalar_field(field_id), ctx->stream, device_tables(c, tl, d), (uint32_t*)(d + o_left), (uint32_t*)(d + o_right)));
  std::vector<uint64_t> back((E * N + E * P) * eb / 8);
  TRY(hipMemcpyAsync(back.data(), d + o_left, E * N * eb, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipMemcpyAsync(back.data() + E * N * eb / 8, d + o_right, E * P * eb, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  memcpy(left_canonical, back.data(), E * N * eb);
  memcpy(right_canonical, back.data() + E * N * eb / 8, E * P * eb);
  return PCDHIP_OK;
  });
}

int pcdhip_kzg_check_combinations(pcdhip_ctx* ctx, pcdhip_kzg_vk* vk, size_t m, const uint64_t* comm_xy, const uint8_t* comm_inf,
                                  const uint64_t* shifted_xy, const uint8_t* shifted_inf, const int32_t* shift_index, size_t n_openings,
                                  const uint64_t* points_mont, const uint64_t* coeffs_mont, const uint64_t* shifted_coeffs_mont,
                                  const uint64_t* values_mont, const uint64_t* random_v_mont, const uint64_t* item_values_mont, const uint64_t* w_xy,
                                  const uint8_t* w_inf, const uint64_t* randomizers_canonical, int* ok) {
  return guarded([&]() -> int {
  const size_t P = n_openings;
  if (!ctx || !vk || !ok || (m && !comm_xy) || (P && (!points_mont || !values_mont || !w_xy || (m && !coeffs_mont)))) return PCDHIP_E_ARG;
  if (P == 0) { *ok = 1; return PCDHIP_OK; }  // (true without a launch: one verdict in either mode)
  CheckArgs c;
  c.fr = kCurveFr[vk->curve_id]; c.m = m; c.P = P; c.n_shift = vk->n_shift; c.shift_index = shift_index;
  c.points = points_mont; c.coeffs = coeffs_mont; c.scoeffs = m ? shifted_coeffs_mont : nullptr; c.values = values_mont; c.random_v = random_v_mont;
  c.item_values = item_values_mont; c.randomizers = randomizers_canonical;
  int rc = check_args(c, shifted_xy != nullptr);
  if (rc) return rc;
  if (random_v_mont && !vk->has_gamma) return PCDHIP_E_ARG;
  BIND();
  int verdicts[CHECK_MAX_OPENINGS];
  rc = kzg_check_run(ctx, vk, c, comm_xy, comm_inf, shifted_xy, shifted_inf, w_xy, w_inf, verdicts);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }  // (an error partway: nothing of this call still reads the key's staging image)
  for (size_t e = 0; e < c.E(); e++) ok[e] = verdicts[e];
  return PCDHIP_OK;
  });
}

int pcdhip_kzg_check_combinations_last_plan(pcdhip_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return PCDHIP_E_ARG;
  for (int i = 0; i < 4; i++) out[i] = ctx->kzg_check_plan[i];
  return PCDHIP_OK;
}

}  // extern "C"
