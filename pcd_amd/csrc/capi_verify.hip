// Pairings, the prepared verifying key and the Groth16 verifications of libpcdhip.so.
#include "capi_internal.h"

using namespace pcd;

namespace {
// groups x per pairs -> groups GT elements
// g1_z (nullable; honoured by the wave-per-pairing kernels only -- callers pass it only while ctx->pairing_vm): Z of Jacobian G1 points
int pairing_groups(pcdhip_ctx* ctx, int curve_id, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                   const uint8_t* g2_inf, size_t groups, size_t per, uint64_t* gt_out, const uint64_t* g1_z = nullptr) {
  const size_t n_pairs = groups * per;
  if (!ctx || !valid_curve(curve_id) || (n_pairs && (!g1_xy || !g2_xy)) || !gt_out || n_pairs >= (1u << 24) || (groups && !per)) return PCDHIP_E_ARG;
  BIND();
  const PairingEntry& pe = pairing_entry(curve_id);
  const size_t w1 = (size_t)pcdhip_point_limbs(curve_id, 1) * 8, w2 = (size_t)pcdhip_point_limbs(curve_id, 2) * 8;
  const size_t gb = (size_t)pe.gt_words * 4, gi = (size_t)pe.gt_internal_words * 4;
  const size_t gt_off = n_pairs * (w1 + w2 + gi), z_off = gt_off + std::max<size_t>(groups, 1) * gb, flag_off = z_off + n_pairs * (w1 / 2);
  TRY(ctx->aux_ws.ensure(AUX_MISC, flag_off + 2 * n_pairs + 256));
  char* d = (char*)ctx->aux_ws.buf[AUX_MISC];
  uint32_t* g1d = (uint32_t*)d;
  uint32_t* g2d = (uint32_t*)(d + n_pairs * w1);
  uint32_t* scr = (uint32_t*)(d + n_pairs * (w1 + w2));
  uint32_t* out = (uint32_t*)(d + gt_off);
  if (n_pairs) {
    TRY(hipMemcpyAsync(g1d, g1_xy, n_pairs * w1, hipMemcpyHostToDevice, ctx->stream));
    TRY(hipMemcpyAsync(g2d, g2_xy, n_pairs * w2, hipMemcpyHostToDevice, ctx->stream));
    // flagged infinities -> (0, 0)
    TRY(zero_flagged(ctx->stream, g1d, (uint8_t*)d + flag_off, g1_inf, n_pairs, w1));
    TRY(zero_flagged(ctx->stream, g2d, (uint8_t*)d + flag_off + n_pairs, g2_inf, n_pairs, w2));
  }
  if (!ctx->vm_block[curve_id] && ctx->pairing_vm) TRY(pe.vm_upload(ctx->stream, &ctx->vm_block[curve_id], &ctx->vm_tables[curve_id]));
  uint32_t* g1zd = nullptr;
  if (g1_z && n_pairs) {
    g1zd = (uint32_t*)(d + z_off);
    TRY(hipMemcpyAsync(g1zd, g1_z, n_pairs * (w1 / 2), hipMemcpyHostToDevice, ctx->stream));
  }
  TRY(pe.multi_pairing(ctx->stream, g1d, g1zd, g2d, (uint32_t)groups, (uint32_t)per, scr, out, ctx->pairing_vm ? &ctx->vm_tables[curve_id] : nullptr));
  TRY(hipMemcpyAsync(gt_out, out, groups * gb, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
}  // namespace

namespace pcd {
// Are all `count` scalars (`into_repr()` images of field `fr`) reduced, i.e. < r?  On the host, before anything is enqueued: the window
// tables read nwin * 8 bits of a scalar and drop the rest, the MSM refuses only what is wider than r, and either computes x + r as x --
// so a public input >= r is a second encoding of another statement and is refused as an argument, not answered with a verdict.
// (A limb compare with the modulus: it holds for the C-ABI Montgomery image as well, which pcdhip_groth16_prove checks r and s with.)
bool scalars_reduced(int fr, const uint64_t* x, size_t count) {
  bool ok = true;
  with_host_field(fr, [&](auto f) {
    typedef typename decltype(f)::type B;
    typedef typename B::Params P;
    B m;
    for (int i = 0; i < B::N; i++) m.v[i] = P::mod(i);
    uint32_t r[P::N32];
    m.pack32(r);
    const uint32_t* w = (const uint32_t*)x;
    for (size_t s = 0; s < count && ok; s++, w += P::N32) {
      int i = P::N32 - 1;
      while (i >= 0 && w[i] == r[i]) i--;
      ok = i >= 0 && w[i] < r[i];
    }
  });
  return ok;
}
}  // namespace pcd

namespace {
// acc_i = gamma_abc[0] + sum_j x_ij gamma_abc[j] for k proofs (Jacobian C-ABI image -> affine + flags), through the resident bases
// acc_z (nullable): when given, non-empty on return iff the accumulations came back in Jacobian form -- (X, Y) in acc_a, Z in acc_z -- which
// happens with window tables and the wave-per-pairing kernels on (they take Jacobian G1 points: no inversion anywhere in a verification)
int prepare_inputs(pcdhip_ctx* ctx, const pcdhip_pvk* pvk, size_t k, const uint64_t* public_inputs, std::vector<uint64_t>* acc_a, std::vector<uint8_t>* acc_inf,
                   std::vector<uint64_t>* acc_z = nullptr) {
  const int cid = pvk->curve_id;
  const size_t l1 = (size_t)pcdhip_point_limbs(cid, 1), sl = (size_t)kFieldLimbs[kCurveFr[cid]], ni = pvk->num_inputs;
  std::vector<uint64_t> acc_j(k * (l1 / 2 * 3)), scal(ni * sl);
  acc_a->assign(k * l1, 0);
  acc_inf->assign(k, 0);
  if (pvk->abc_dev) {  // window tables: every proof's accumulation in one launch, no doubling chains
    const GroupEntry& ge = group_entry(cid, 1);
    const size_t jw = (size_t)ge.point_words / 2 * 3, sb = (ni - 1) * sl * 8;
    // Jacobian accumulations only when the wave-per-pairing kernels will take them: 3 pairings per proof, PCD_VM_MAX_PAIRS per launch
    // (beyond, the lane-per-pairing kernels want affine points: a batch of 1366+ proofs used to fail here)
    const bool jac = acc_z && ctx->pairing_vm && 3 * k <= PCD_VM_MAX_PAIRS;
    TRY(ctx->aux_ws.ensure(AUX_FB_JAC, k * (64 * jw * 4 + sb + l1 * 8 + l1 * 4 + 1) + 64));
    char* d = (char*)ctx->aux_ws.buf[AUX_FB_JAC];
    uint32_t* scratch = (uint32_t*)d;
    uint32_t* scal_d = (uint32_t*)(d + k * 64 * jw * 4);
    uint32_t* out_d = (uint32_t*)((char*)scal_d + k * sb);
    uint32_t* z_d = (uint32_t*)((char*)out_d + k * l1 * 8);
    uint8_t* inf_d = (uint8_t*)z_d + k * l1 * 4;
    if (sb) TRY(hipMemcpyAsync(scal_d, public_inputs, k * sb, hipMemcpyHostToDevice, ctx->stream));
    TRY(ge.fb_inputs(ctx->stream, pvk->abc_dev + pvk->abc_tables_off, pvk->abc_dev, (uint32_t)ni, scal_d, (uint32_t)k, scratch, out_d, inf_d, jac ? z_d : nullptr, 1));
    if (jac) { acc_z->assign(k * (l1 / 2), 0); TRY(hipMemcpyAsync(acc_z->data(), z_d, k * l1 * 4, hipMemcpyDeviceToHost, ctx->stream)); }
    TRY(hipMemcpyAsync(acc_a->data(), out_d, k * l1 * 8, hipMemcpyDeviceToHost, ctx->stream));
    TRY(hipMemcpyAsync(acc_inf->data(), inf_d, k, hipMemcpyDeviceToHost, ctx->stream));
    TRY(hipStreamSynchronize(ctx->stream));
    return PCDHIP_OK;
  }
  for (size_t i = 0; i < k; i++) {
    std::fill(scal.begin(), scal.end(), 0);
    scal[0] = 1;
    if (ni > 1) memcpy(&scal[sl], public_inputs + i * (ni - 1) * sl, (ni - 1) * sl * 8);
    int rc = pcdhip_msm(ctx, pvk->abc, 0, scal.data(), ni, &acc_j[i * (l1 / 2 * 3)]);
    if (rc) return rc;
  }
  return pcdhip_to_affine(ctx, cid, 1, acc_j.data(), k, acc_a->data(), acc_inf->data());
}
// The prepared verification on the wave-per-pairing kernels as ONE trip to the device: a single upload (public inputs, the proofs'
// points, -gamma, -delta, Z = 1), the input accumulation writing its Jacobian result straight into the middle pair's slot, the Miller
// loops, the final exponentiations, one download.  (As separate calls -- prepare_inputs, then pairing_groups -- the same work was
// fourteen stream operations and two synchronisations: 0.33 ms in front of a 1.1 ms Miller loop.)
int verify_prepared_vm(pcdhip_ctx* ctx, const pcdhip_pvk* pvk, size_t k, const uint64_t* public_inputs, const uint64_t* proofs, const uint8_t* proofs_inf,
                       int* ok) {
  const int cid = pvk->curve_id;
  const PairingEntry& pe = pairing_entry(cid);
  const GroupEntry& ge = group_entry(cid, 1);
  const size_t l1 = (size_t)pcdhip_point_limbs(cid, 1), l2 = (size_t)pcdhip_point_limbs(cid, 2), pl = 2 * l1 + l2, lz = l1 / 2;
  const size_t sl = (size_t)kFieldLimbs[kCurveFr[cid]], ni = pvk->num_inputs, np = 3 * k;
  const size_t w1 = l1 * 8, w2 = l2 * 8, wz = lz * 8, sb = (ni - 1) * sl * 8, jw = (size_t)ge.point_words / 2 * 3;
  const size_t gb = (size_t)pe.gt_words * 4, gi = (size_t)pe.gt_internal_words * 4, gw = pvk->alpha_beta.size();
  // the upload: [g1 | g2 | z | scalars], 16-byte aligned parts; behind it on the device: Miller values, GT results, accumulation scratch
  auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_g1 = 0, o_g2 = o_g1 + up16(np * w1), o_z = o_g2 + up16(np * w2), o_sc = o_z + up16(np * wz), up_bytes = o_sc + up16(k * sb);
  const size_t o_f = up_bytes, o_gt = o_f + up16(np * gi), o_scr = o_gt + up16(k * gb), o_inf = o_scr + up16(k * 64 * jw * 4), total = o_inf + up16(k) + 256;
  TRY(ctx->aux_ws.ensure(AUX_MISC, total));
  char* d = (char*)ctx->aux_ws.buf[AUX_MISC];
  std::vector<uint64_t> host(up_bytes / 8, 0);
  char* h = (char*)host.data();
  for (size_t i = 0; i < k; i++) {
    const uint64_t* pr = proofs + i * pl;
    const bool ia = proofs_inf && proofs_inf[3 * i], ib = proofs_inf && proofs_inf[3 * i + 1], ic = proofs_inf && proofs_inf[3 * i + 2];
    // (a flagged infinity stays (0, 0), which is how the kernels know it)
    if (!ia) memcpy(h + o_g1 + (3 * i) * w1, pr, w1);
    if (!ic) memcpy(h + o_g1 + (3 * i + 2) * w1, pr + l1 + l2, w1);
    if (!ib) memcpy(h + o_g2 + (3 * i) * w2, pr + l1, w2);
    memcpy(h + o_g2 + (3 * i + 1) * w2, pvk->neg_gamma.data(), w2);
    memcpy(h + o_g2 + (3 * i + 2) * w2, pvk->neg_delta.data(), w2);
    memcpy(h + o_z + (3 * i) * wz, pvk->gt_one.data(), wz);       // Z = 1 (the first coefficient of GT's one) for the proof's own points
    memcpy(h + o_z + (3 * i + 2) * wz, pvk->gt_one.data(), wz);
  }
  if (sb) memcpy(h + o_sc, public_inputs, k * sb);
  TRY(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!ctx->vm_block[cid]) TRY(pe.vm_upload(ctx->stream, &ctx->vm_block[cid], &ctx->vm_tables[cid]));
  uint32_t* g1d = (uint32_t*)(d + o_g1);
  uint32_t* g1zd = (uint32_t*)(d + o_z);
  // acc_i -> pair 3 i + 1, Jacobian: (X, Y) into the G1 array, Z into the Z array (an infinite accumulation has Z = 0)
  TRY(ge.fb_inputs(ctx->stream, pvk->abc_dev + pvk->abc_tables_off, pvk->abc_dev, (uint32_t)ni, (const uint32_t*)(d + o_sc), (uint32_t)k, (uint32_t*)(d + o_scr),
                   g1d + w1 / 4, (uint8_t*)(d + o_inf), g1zd + wz / 4, 3));
  TRY(pe.multi_pairing(ctx->stream, g1d, g1zd, (const uint32_t*)(d + o_g2), (uint32_t)k, 3, (uint32_t*)(d + o_f), (uint32_t*)(d + o_gt), &ctx->vm_tables[cid]));
  std::vector<uint64_t> gt(k * gw);
  TRY(hipMemcpyAsync(gt.data(), d + o_gt, k * gb, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < k; i++) ok[i] = memcmp(&gt[i * gw], pvk->alpha_beta.data(), gw * 8) == 0 ? 1 : 0;
  return PCDHIP_OK;
}
}  // namespace

namespace pcd {
// y -> -y of an affine point in the C-ABI image, on the host (the library's own host-callable field templates)
void negate_point(int curve_id, int group_id, uint64_t* xy) {
  const size_t deg = group_id == 1 ? 1 : (size_t)kCurveG2Deg[curve_id];
  bool zero = true;  // the point at infinity (zero coordinates) stays what it is
  for (size_t k = 0; k < (size_t)pcdhip_point_limbs(curve_id, group_id); k++) zero = zero && xy[k] == 0;
  if (zero) return;
  with_host_field(kCurveFq[curve_id], [&](auto fq) {
    typedef typename decltype(fq)::type B;
    uint32_t* y = (uint32_t*)xy + deg * B::ABI_WORDS;
    for (size_t c = 0; c < deg; c++) B::from_abi(y + c * B::ABI_WORDS).neg().to_abi(y + c * B::ABI_WORDS);
  });
}
// canonical scalars: out = sum_i a_i * b_i mod r  (b_i == nullptr: plain sum); `words` u32 words each
void scalar_lincomb(int fr, const uint64_t* const* a, const uint64_t* const* b, size_t n, uint64_t* out) {
  with_host_field(fr, [&](auto f) {
    typedef typename decltype(f)::type B;
    B acc = B::zero();
    for (size_t i = 0; i < n; i++) {
      B x = B::from_canonical_words((const uint32_t*)a[i]);
      if (b && b[i]) x = x * B::from_canonical_words((const uint32_t*)b[i]);
      acc = acc + x;
    }
    acc.to_canonical_words((uint32_t*)out);
  });
}
}  // namespace pcd

extern "C" {

int pcdhip_pairing_set_mode(pcdhip_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 1) return PCDHIP_E_ARG;
  ctx->pairing_vm = mode == 0;
  return PCDHIP_OK;
}
int pcdhip_multi_pairing(pcdhip_ctx* ctx, int curve_id, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                         const uint8_t* g2_inf, size_t n_pairs, uint64_t* gt_out) {
  // (one group holding every pair; with no pair at all the empty product still goes through the final exponentiation)
  if (n_pairs == 0) {
    if (!ctx || !valid_curve(curve_id) || !gt_out) return PCDHIP_E_ARG;
    BIND();
    const PairingEntry& pe = pairing_entry(curve_id);
    TRY(ctx->aux_ws.ensure(AUX_MISC, (size_t)pe.gt_words * 4 + 256));
    uint32_t* out = (uint32_t*)ctx->aux_ws.buf[AUX_MISC];
    if (!ctx->vm_block[curve_id] && ctx->pairing_vm) TRY(pe.vm_upload(ctx->stream, &ctx->vm_block[curve_id], &ctx->vm_tables[curve_id]));
    TRY(pe.multi_pairing(ctx->stream, out, nullptr, out, 1, 0, out, out, ctx->pairing_vm ? &ctx->vm_tables[curve_id] : nullptr));
    TRY(hipMemcpyAsync(gt_out, out, (size_t)pe.gt_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    TRY(hipStreamSynchronize(ctx->stream));
    return PCDHIP_OK;
  }
  return pairing_groups(ctx, curve_id, g1_xy, g1_inf, g2_xy, g2_inf, 1, n_pairs, gt_out);
}

// ---- prepared verifying key (ark-groth16 `prepare_verifying_key` / `SNARK::process_vk`; reference call sites
// src/ec_cycle_pcd/mod.rs:71,371,445,495,553) and the verifications that use it
int pcdhip_process_vk(pcdhip_ctx* ctx, int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                      const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t num_inputs, pcdhip_pvk** out) {
  return guarded([&]() -> int {
  if (!ctx || !valid_curve(curve_id) || !alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1 || num_inputs < 1 || !out) return PCDHIP_E_ARG;
  BIND();
  *out = nullptr;
  const size_t l1 = (size_t)pcdhip_point_limbs(curve_id, 1), l2 = (size_t)pcdhip_point_limbs(curve_id, 2);
  const PairingEntry& pe = pairing_entry(curve_id);
  pcdhip_pvk* pvk = new pcdhip_pvk();
  pvk->curve_id = curve_id; pvk->num_inputs = num_inputs;
  pvk->alpha.assign(alpha_g1, alpha_g1 + l1);
  pvk->beta.assign(beta_g2, beta_g2 + l2);
  pvk->neg_gamma.assign(gamma_g2, gamma_g2 + l2);
  pvk->neg_delta.assign(delta_g2, delta_g2 + l2);
  negate_point(curve_id, 2, pvk->neg_gamma.data());
  negate_point(curve_id, 2, pvk->neg_delta.data());
  pvk->gamma_abc.assign(gamma_abc_g1, gamma_abc_g1 + num_inputs * l1);
  pvk->gamma_abc_inf.assign(num_inputs, 0);
  if (gamma_abc_inf) pvk->gamma_abc_inf.assign(gamma_abc_inf, gamma_abc_inf + num_inputs);
  pvk->alpha_beta.assign(pe.gt_words / 2, 0);
  pvk->gt_one.assign(pe.gt_words / 2, 0);
  const int saved = ctx->precompute;
  ctx->precompute = 0;
  int rc = bases_upload_single(ctx, curve_id, 1, gamma_abc_g1, gamma_abc_inf, num_inputs, &pvk->abc);  // (device 0 of a multi-device context)
  ctx->precompute = saved;
  if (!rc && num_inputs <= PVK_TABLE_INPUTS) {
    const GroupEntry& ge = group_entry(curve_id, 1);
    const size_t abi_w = (size_t)ge.point_abi_words;
    const size_t tab_w = ge.fb_table_words;   // one table + the Jacobians of its doubling chain
    const size_t head = (num_inputs * abi_w + num_inputs / 4 + 64 + 3) / 4 * 4;   // points, then the flag bytes, 16-byte aligned
    hipError_t e = hipMalloc((void**)&pvk->abc_dev, (head + std::max<size_t>(num_inputs - 1, 1) * tab_w) * 4);
    if (e != hipSuccess) {  // no room for the window tables (up to 1.3 GB for a 753-bit key): the plain resident vector serves (MSM path)
      (void)hipGetLastError();
      pvk->abc_dev = nullptr;
    }
  }
  if (!rc && pvk->abc_dev) {
    const GroupEntry& ge = group_entry(curve_id, 1);
    const size_t abi_w = (size_t)ge.point_abi_words;
    const size_t head = (num_inputs * abi_w + num_inputs / 4 + 64 + 3) / 4 * 4;
    pvk->abc_tables_off = head;
    hipError_t e = hipMemcpyAsync(pvk->abc_dev, gamma_abc_g1, num_inputs * abi_w * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = zero_flagged(ctx->stream, pvk->abc_dev, (uint8_t*)(pvk->abc_dev + num_inputs * abi_w), gamma_abc_inf, num_inputs, abi_w * 4);
    if (e == hipSuccess) e = ge.fb_tables(ctx->stream, pvk->abc_dev, (uint32_t)num_inputs, pvk->abc_dev + head);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { pcdhip_pvk_free(ctx, pvk); return fail(ctx, e); }
  }
  rc = rc ? rc : pcdhip_multi_pairing(ctx, curve_id, alpha_g1, nullptr, beta_g2, nullptr, 1, pvk->alpha_beta.data());  // e(alpha, beta), once
  rc = rc ? rc : pcdhip_multi_pairing(ctx, curve_id, nullptr, nullptr, nullptr, nullptr, 0, pvk->gt_one.data());
  if (rc) { pcdhip_pvk_free(ctx, pvk); return rc; }
  *out = pvk;
  return PCDHIP_OK;
  });
}
void pcdhip_pvk_free(pcdhip_ctx* ctx, pcdhip_pvk* pvk) {
  if (!pvk) return;
  pcdhip_bases_free(ctx, pvk->abc);
  if (pvk->abc_dev) { if (ctx) (void)hipSetDevice(ctx->device); (void)hipFree(pvk->abc_dev); }
  delete pvk;
}

// `verify_with_processed_vk` for n proofs under one key: e(A, B) e(acc, -gamma) e(C, -delta) == e(alpha, beta) -- three Miller
// loops and one final exponentiation per proof, every Miller loop of the batch in one launch, one lane per proof for the products
// and final exponentiations.
int pcdhip_groth16_verify_prepared(pcdhip_ctx* ctx, const pcdhip_pvk* pvk, size_t n_proofs, const uint64_t* public_inputs_canonical,
                                   const uint64_t* proofs, const uint8_t* proofs_inf, int* ok) {
  return guarded([&]() -> int {
  if (!ctx || !pvk || (n_proofs && (!proofs || !ok)) || (pvk->num_inputs > 1 && n_proofs && !public_inputs_canonical) || n_proofs >= (1u << 20))
    return PCDHIP_E_ARG;
  if (n_proofs == 0) return PCDHIP_OK;
  if (pvk->num_inputs > 1 && !scalars_reduced(kCurveFr[pvk->curve_id], public_inputs_canonical, n_proofs * (pvk->num_inputs - 1))) return PCDHIP_E_ARG;
  BIND();
  const int cid = pvk->curve_id;
  const size_t l1 = (size_t)pcdhip_point_limbs(cid, 1), l2 = (size_t)pcdhip_point_limbs(cid, 2), pl = 2 * l1 + l2, k = n_proofs;
  if (ctx->pairing_vm && pvk->abc_dev && 3 * k <= PCD_VM_MAX_PAIRS) return verify_prepared_vm(ctx, pvk, k, public_inputs_canonical, proofs, proofs_inf, ok);
  std::vector<uint64_t> acc_a, acc_z;
  std::vector<uint8_t> acc_inf;
  int rc = prepare_inputs(ctx, pvk, k, public_inputs_canonical, &acc_a, &acc_inf, &acc_z);
  if (rc) return rc;
  const size_t gw = pvk->alpha_beta.size(), lz = l1 / 2;
  std::vector<uint64_t> gt(k * gw), g1s(3 * k * l1), g2s(3 * k * l2), g1z;
  if (!acc_z.empty()) {  // Z = 1 (the first coefficient of GT's one) for the proof's own points, the accumulation's Z for the middle pair
    g1z.resize(3 * k * lz);
    for (size_t i = 0; i < 3 * k; i++) memcpy(&g1z[i * lz], i % 3 == 1 ? &acc_z[(i / 3) * lz] : pvk->gt_one.data(), lz * 8);
  }
  std::vector<uint8_t> inf1(3 * k, 0), inf2(3 * k, 0);
  for (size_t i = 0; i < k; i++) {
    const uint64_t* pr = proofs + i * pl;
    memcpy(&g1s[(3 * i) * l1], pr, l1 * 8);
    memcpy(&g1s[(3 * i + 1) * l1], &acc_a[i * l1], l1 * 8);
    memcpy(&g1s[(3 * i + 2) * l1], pr + l1 + l2, l1 * 8);
    memcpy(&g2s[(3 * i) * l2], pr + l1, l2 * 8);
    memcpy(&g2s[(3 * i + 1) * l2], pvk->neg_gamma.data(), l2 * 8);
    memcpy(&g2s[(3 * i + 2) * l2], pvk->neg_delta.data(), l2 * 8);
    inf1[3 * i + 1] = acc_inf[i];
    if (proofs_inf) { inf1[3 * i] = proofs_inf[3 * i]; inf2[3 * i] = proofs_inf[3 * i + 1]; inf1[3 * i + 2] = proofs_inf[3 * i + 2]; }
  }
  rc = pairing_groups(ctx, cid, g1s.data(), inf1.data(), g2s.data(), inf2.data(), k, 3, gt.data(), g1z.empty() ? nullptr : g1z.data());
  if (rc) return rc;
  for (size_t i = 0; i < k; i++) ok[i] = memcmp(&gt[i * gw], pvk->alpha_beta.data(), gw * 8) == 0 ? 1 : 0;
  return PCDHIP_OK;
  });
}

// All n proofs at once with ONE final exponentiation: with caller-supplied challenges rho_i (128 bits each, two
// u64 limbs per proof; the library has no RNG) the n equations are raised to rho_i and multiplied,
//   prod_i e(rho_i A_i, B_i) * e(sum_i rho_i acc_i, -gamma) * e(sum_i rho_i C_i, -delta) * e(-(sum_i rho_i) alpha, beta) == 1,
// n + 3 Miller loops in one launch and one final exponentiation.  Sound up to 2^-128 over the choice of rho (a batch that contains an
// invalid proof passes with that probability); when it reports failure, pcdhip_groth16_verify_prepared tells which proof is bad.
int pcdhip_groth16_verify_batch_rlc(pcdhip_ctx* ctx, const pcdhip_pvk* pvk, size_t n_proofs, const uint64_t* public_inputs_canonical,
                                    const uint64_t* proofs, const uint8_t* proofs_inf, const uint64_t* rho, int* all_ok) {
  return guarded([&]() -> int {
  if (!ctx || !pvk || !all_ok || (n_proofs && (!proofs || !rho)) || (pvk->num_inputs > 1 && n_proofs && !public_inputs_canonical) || n_proofs >= (1u << 16))
    return PCDHIP_E_ARG;
  *all_ok = 1;
  if (n_proofs == 0) return PCDHIP_OK;
  for (size_t i = 0; i < n_proofs; i++) if (!(rho[2 * i] | rho[2 * i + 1])) return PCDHIP_E_ARG;  // zero is not a challenge
  if (pvk->num_inputs > 1 && !scalars_reduced(kCurveFr[pvk->curve_id], public_inputs_canonical, n_proofs * (pvk->num_inputs - 1))) { *all_ok = 0; return PCDHIP_E_ARG; }
  // While the batch's 3k Miller loops find a SIMD each (one wave per pairing: pairing_vm.hip.h) the k verifications side by side take the
  // time of one -- less than the scalings of the combination cost (k = 8: 5.5 against 17 ms on MNT4-298) -- and their answer is the
  // deterministic one.  The random linear combination is for batches that would otherwise queue on the chip.
  if (ctx->pairing_vm && 3 * n_proofs <= 1024) {
    std::vector<int> each(n_proofs, 0);
    int rc = pcdhip_groth16_verify_prepared(ctx, pvk, n_proofs, public_inputs_canonical, proofs, proofs_inf, each.data());
    if (rc) return rc;
    for (size_t i = 0; i < n_proofs; i++) if (!each[i]) *all_ok = 0;
    return PCDHIP_OK;
  }
  BIND();
  const int cid = pvk->curve_id, fr = kCurveFr[cid];
  const size_t l1 = (size_t)pcdhip_point_limbs(cid, 1), l2 = (size_t)pcdhip_point_limbs(cid, 2), pl = 2 * l1 + l2, k = n_proofs;
  const size_t sl = (size_t)kFieldLimbs[fr], ni = pvk->num_inputs, j1 = l1 / 2 * 3;
  // challenges as full-width canonical scalars (zero is not a challenge)
  std::vector<uint64_t> rw(k * sl, 0);
  for (size_t i = 0; i < k; i++) { rw[i * sl] = rho[2 * i]; rw[i * sl + 1] = rho[2 * i + 1]; if (!(rho[2 * i] | rho[2 * i + 1])) return PCDHIP_E_ARG; }
  // scalars of the gamma_abc combination: s_0 = sum rho_i, s_j = sum_i rho_i x_ij
  std::vector<uint64_t> s(ni * sl, 0);
  std::vector<const uint64_t*> pa(k), pb(k);
  for (size_t i = 0; i < k; i++) pa[i] = &rw[i * sl];
  scalar_lincomb(fr, pa.data(), nullptr, k, &s[0]);
  for (size_t j = 1; j < ni; j++) {
    for (size_t i = 0; i < k; i++) pb[i] = public_inputs_canonical + (i * (ni - 1) + (j - 1)) * sl;
    scalar_lincomb(fr, pa.data(), pb.data(), k, &s[j * sl]);
  }
  std::vector<uint64_t> sacc_j(j1), sacc(l1);
  uint8_t sacc_inf = 0;
  int rc = pcdhip_msm(ctx, pvk->abc, 0, s.data(), ni, sacc_j.data());
  rc = rc ? rc : pcdhip_to_affine(ctx, cid, 1, sacc_j.data(), 1, sacc.data(), &sacc_inf);
  if (rc) return rc;
  // rho_i A_i, rho_i C_i and (sum rho) alpha: 2k + 1 one-lane products in one launch
  const size_t np = 2 * k + 1;
  std::vector<uint64_t> pts(np * l1), ks(np * sl), prod(np * j1);
  for (size_t i = 0; i < k; i++) {
    const uint64_t* pr = proofs + i * pl;
    memcpy(&pts[i * l1], pr, l1 * 8);
    memcpy(&pts[(k + i) * l1], pr + l1 + l2, l1 * 8);
    if (proofs_inf && proofs_inf[3 * i]) memset(&pts[i * l1], 0, l1 * 8);
    if (proofs_inf && proofs_inf[3 * i + 2]) memset(&pts[(k + i) * l1], 0, l1 * 8);
    memcpy(&ks[i * sl], &rw[i * sl], sl * 8);
    memcpy(&ks[(k + i) * sl], &rw[i * sl], sl * 8);
  }
  memcpy(&pts[2 * k * l1], pvk->alpha.data(), l1 * 8);
  memcpy(&ks[2 * k * sl], &s[0], sl * 8);
  {
    const size_t in_b = np * l1 * 8, k_b = np * sl * 8, out_b = np * j1 * 8;
    TRY(ctx->aux_ws.ensure(AUX_MISC, in_b + k_b + out_b + 64));
    char* d = (char*)ctx->aux_ws.buf[AUX_MISC];
    TRY(hipMemcpyAsync(d, pts.data(), in_b, hipMemcpyHostToDevice, ctx->stream));
    TRY(hipMemcpyAsync(d + in_b, ks.data(), k_b, hipMemcpyHostToDevice, ctx->stream));
    TRY(g1_scale_entry(cid)(ctx->stream, (const uint32_t*)d, (const uint32_t*)(d + in_b), (uint32_t)(sl * 2), (uint32_t)np, (uint32_t*)(d + in_b + k_b)));
    TRY(hipMemcpyAsync(prod.data(), d + in_b + k_b, out_b, hipMemcpyDeviceToHost, ctx->stream));
    TRY(hipStreamSynchronize(ctx->stream));
  }
  std::vector<uint64_t> sc_j(j1), ra(k * l1), sc(l1), sal(l1);
  std::vector<uint8_t> ra_inf(k, 0);
  uint8_t sc_inf = 0, sal_inf = 0;
  rc = pcdhip_points_sum(ctx, cid, 1, &prod[k * j1], k, sc_j.data());
  rc = rc ? rc : pcdhip_to_affine(ctx, cid, 1, sc_j.data(), 1, sc.data(), &sc_inf);
  rc = rc ? rc : pcdhip_to_affine(ctx, cid, 1, prod.data(), k, ra.data(), ra_inf.data());
  rc = rc ? rc : pcdhip_to_affine(ctx, cid, 1, &prod[2 * k * j1], 1, sal.data(), &sal_inf);
  if (rc) return rc;
  negate_point(cid, 1, sal.data());
  // the k + 3 pairs of the single product
  const size_t nq = k + 3;
  std::vector<uint64_t> g1s(nq * l1), g2s(nq * l2), gt(pvk->gt_one.size());
  std::vector<uint8_t> inf1(nq, 0), inf2(nq, 0);
  for (size_t i = 0; i < k; i++) {
    memcpy(&g1s[i * l1], &ra[i * l1], l1 * 8);
    memcpy(&g2s[i * l2], proofs + i * pl + l1, l2 * 8);
    inf1[i] = ra_inf[i];
    if (proofs_inf) inf2[i] = proofs_inf[3 * i + 1];
  }
  memcpy(&g1s[k * l1], sacc.data(), l1 * 8);       memcpy(&g2s[k * l2], pvk->neg_gamma.data(), l2 * 8);       inf1[k] = sacc_inf;
  memcpy(&g1s[(k + 1) * l1], sc.data(), l1 * 8);   memcpy(&g2s[(k + 1) * l2], pvk->neg_delta.data(), l2 * 8);   inf1[k + 1] = sc_inf;
  memcpy(&g1s[(k + 2) * l1], sal.data(), l1 * 8);  memcpy(&g2s[(k + 2) * l2], pvk->beta.data(), l2 * 8);        inf1[k + 2] = sal_inf;
  rc = pairing_groups(ctx, cid, g1s.data(), inf1.data(), g2s.data(), inf2.data(), 1, nq, gt.data());
  if (rc) return rc;
  *all_ok = memcmp(gt.data(), pvk->gt_one.data(), gt.size() * 8) == 0 ? 1 : 0;
  return PCDHIP_OK;
  });
}

// ark-groth16 `Groth16::verify` for n proofs under one key (reference call site mod.rs:239, once per prior message of a merge node):
// process_vk once, then the prepared verification.  Deterministic: ok[i] per proof.
int pcdhip_groth16_verify_batch(pcdhip_ctx* ctx, int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                                const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t num_inputs,
                                size_t n_proofs, const uint64_t* public_inputs_canonical, const uint64_t* proofs, const uint8_t* proofs_inf,
                                int* ok) {
  if (!ctx || !valid_curve(curve_id) || !alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1 || num_inputs < 1 ||
      (num_inputs > 1 && n_proofs && !public_inputs_canonical) || (n_proofs && (!proofs || !ok)) || n_proofs >= (1u << 20))
    return PCDHIP_E_ARG;
  if (n_proofs == 0) return PCDHIP_OK;
  // (the prepared verification checks this as well; here it saves building the key's tables for a call that is refused)
  if (num_inputs > 1 && !scalars_reduced(kCurveFr[curve_id], public_inputs_canonical, n_proofs * (num_inputs - 1))) return PCDHIP_E_ARG;
  pcdhip_pvk* pvk = nullptr;
  int rc = pcdhip_process_vk(ctx, curve_id, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, gamma_abc_inf, num_inputs, &pvk);
  if (rc) return rc;
  rc = pcdhip_groth16_verify_prepared(ctx, pvk, n_proofs, public_inputs_canonical, proofs, proofs_inf, ok);
  pcdhip_pvk_free(ctx, pvk);
  return rc;
}

int pcdhip_groth16_verify(pcdhip_ctx* ctx, int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                          const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t num_inputs,
                          const uint64_t* public_inputs_canonical, const uint64_t* proof, const uint8_t* proof_inf, int* ok) {
  if (!proof || !ok) return PCDHIP_E_ARG;
  *ok = 0;
  return pcdhip_groth16_verify_batch(ctx, curve_id, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, gamma_abc_inf, num_inputs, 1,
                                     public_inputs_canonical, proof, proof_inf, ok);
}

}  // extern "C"
