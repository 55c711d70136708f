// ------------------------------------------------------------------------------------------------ K7: KZG10 open side
// (poly.hip.h: division by (X - z), evaluation, linear combination; then the witness MSMs and the pairing check)
#include "capi_internal.h"

using namespace pcd;

namespace {
enum { AUX_POLY = AUX_FB_OUT + 1, AUX_POLY_Q, AUX_POLY_R };  // descriptors | values | tile scratch;  the two quotients of an opening

// descriptors of k polynomials of one field (lens[j] <= their buffers' n, below 2^31) -> the field, or -1 when they do not qualify
int poly_descs(const pcdhip_buf* const* polys, const size_t* lens, size_t k, std::vector<PolyDesc>* d, uint64_t* max_len) {
  int f = -1;
  *max_len = 0;
  d->resize(k);
  for (size_t j = 0; j < k; j++) {
    const pcdhip_buf* b = polys[j];
    if (!b || lens[j] > b->n || lens[j] >= (1ull << 31) || (j && b->field_id != f)) return -1;
    f = b->field_id;
    (*d)[j] = {b->dptr, (uint64_t)lens[j]};
    *max_len = std::max<uint64_t>(*max_len, lens[j]);
  }
  return f;
}
// the k values land on the device at *values_dev (ABI Montgomery); with div (k == 1) the quotient goes to q_out as well
int poly_eval_run(pcdhip_ctx* ctx, int f, const std::vector<PolyDesc>& d, uint64_t max_len, const uint64_t* z_mont, uint32_t** values_dev,
                  const PolyDesc* div = nullptr, uint32_t* q_out = nullptr, int q_canonical = 0) {
  const FieldEntry& fe = field_entry(f);
  const size_t k = d.size();
  const size_t db = (k * sizeof(PolyDesc) + 255) & ~(size_t)255, vb = (k * fe.abi_words * 4 + 255) & ~(size_t)255;
  TRY(ctx->aux_ws.ensure(AUX_POLY, db + vb + fe.poly_scratch_words((uint32_t)k, max_len) * 4));
  char* base = (char*)ctx->aux_ws.buf[AUX_POLY];
  TRY(hipMemcpyAsync(base, d.data(), k * sizeof(PolyDesc), hipMemcpyHostToDevice, ctx->stream));
  *values_dev = (uint32_t*)(base + db);
  TRY(fe.poly_eval(ctx->stream, (const PolyDesc*)base, (uint32_t)k, max_len, (const uint32_t*)z_mont, (uint32_t*)(base + db + vb), *values_dev,
                   div, q_out, q_canonical));
  return PCDHIP_OK;
}
// p / (X - z) as canonical scalars in the workspace slot (len - 1 of them), p(z) to the host
int kzg_divide(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, const uint64_t* z_mont, int slot, uint32_t** q_dev, uint64_t* value_mont) {
  const FieldEntry& fe = field_entry(p->field_id);
  TRY(ctx->aux_ws.ensure(slot, std::max<size_t>(len, 1) * fe.abi_words * 4));
  *q_dev = (uint32_t*)ctx->aux_ws.buf[slot];
  const std::vector<PolyDesc> d = {{p->dptr, (uint64_t)len}};
  uint32_t* vals = nullptr;
  int rc = poly_eval_run(ctx, p->field_id, d, len, z_mont, &vals, &d[0], *q_dev, 1);
  if (rc) return rc;
  TRY(hipMemcpyAsync(value_mont, vals, (size_t)fe.abi_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
// the witness MSM over the bases' prefix; an empty quotient gives the point at infinity (Z = 0).  Upstream skips the quotient's
// leading zeros before its MSM: not needed here, a zero scalar drops out of the buckets.
int kzg_witness(pcdhip_ctx* ctx, const pcdhip_bases* bases, const uint32_t* q_dev, size_t n, uint64_t* out_xyz) {
  if (n == 0) {
    memset(out_xyz, 0, (size_t)pcdhip_point_limbs(bases->curve_id, bases->group_id) / 2 * 3 * 8);
    return PCDHIP_OK;
  }
  if (n <= ctx->msm_short_max) return msm_short_common(ctx, bases, 0, q_dev, n, out_xyz);  // pcdhip_msm_set_short: no buckets for a few pairs
  return msm_common(ctx, bases, 0, q_dev, n, out_xyz);
}
void mont_to_canonical(int fr, const uint64_t* in, uint64_t* out) {
  with_host_field(fr, [&](auto f) { decltype(f)::type::from_abi((const uint32_t*)in).to_canonical_words((uint32_t*)out); });
}
// the one of GT in the C-ABI image (tower order: its first base-field coefficient is 1, the others 0), as the pairing writes it
void gt_one(int curve_id, uint64_t* out /* zeroed */) {
  with_host_field(kCurveFq[curve_id], [&](auto fq) { decltype(fq)::type::one().to_abi((uint32_t*)out); });
}
}  // namespace

extern "C" {

int pcdhip_poly_eval(pcdhip_ctx* ctx, const pcdhip_buf* const* polys, const size_t* lens, size_t k, const uint64_t* z_mont,
                     uint64_t* out_mont) {
  return guarded([&]() -> int {
  if (!ctx || !z_mont || (k && (!polys || !lens || !out_mont)) || k > 65535) return PCDHIP_E_ARG;
  if (k == 0) return PCDHIP_OK;
  std::vector<PolyDesc> d;
  uint64_t max_len = 0;
  const int f = poly_descs(polys, lens, k, &d, &max_len);
  if (f < 0) return PCDHIP_E_ARG;
  BIND();
  uint32_t* vals = nullptr;
  int rc = poly_eval_run(ctx, f, d, max_len, z_mont, &vals);
  if (rc) return rc;
  TRY(hipMemcpyAsync(out_mont, vals, k * kFieldLimbs[f] * 8, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
  });
}

int pcdhip_poly_lincomb(pcdhip_ctx* ctx, const pcdhip_buf* const* polys, const size_t* lens, const uint64_t* coeffs_mont, size_t k,
                        pcdhip_buf* out, size_t* out_len) {
  return guarded([&]() -> int {
  if (!ctx || !out || !out_len || (k && (!polys || !lens || !coeffs_mont)) || k >= (1ull << 31)) return PCDHIP_E_ARG;
  std::vector<PolyDesc> d;
  uint64_t max_len = 0;
  const int f = k ? poly_descs(polys, lens, k, &d, &max_len) : out->field_id;
  if (f < 0 || f != out->field_id || max_len > out->n) return PCDHIP_E_ARG;
  *out_len = max_len;
  if (max_len == 0) return PCDHIP_OK;
  BIND();
  const FieldEntry& fe = field_entry(f);
  const size_t db = (k * sizeof(PolyDesc) + 255) & ~(size_t)255;
  TRY(ctx->aux_ws.ensure(AUX_POLY, db + k * fe.abi_words * 4));
  char* base = (char*)ctx->aux_ws.buf[AUX_POLY];
  TRY(hipMemcpyAsync(base, d.data(), k * sizeof(PolyDesc), hipMemcpyHostToDevice, ctx->stream));
  TRY(hipMemcpyAsync(base + db, coeffs_mont, k * fe.abi_words * 4, hipMemcpyHostToDevice, ctx->stream));
  TRY(fe.poly_lincomb(ctx->stream, (const PolyDesc*)base, (const uint32_t*)(base + db), (uint32_t)k, max_len, out->dptr));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
  });
}

int pcdhip_poly_div_linear(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, const uint64_t* z_mont, pcdhip_buf* q, uint64_t* value_mont) {
  return guarded([&]() -> int {
  if (!ctx || !p || !z_mont || !value_mont || len > p->n || len >= (1ull << 31)) return PCDHIP_E_ARG;
  if (len > 1 && (!q || q->field_id != p->field_id || q->n < len - 1 || q->dptr == p->dptr)) return PCDHIP_E_ARG;
  BIND();
  const std::vector<PolyDesc> d = {{p->dptr, (uint64_t)len}};
  uint32_t* vals = nullptr;
  int rc = poly_eval_run(ctx, p->field_id, d, len, z_mont, &vals, &d[0], len > 1 ? q->dptr : nullptr, 0);
  if (rc) return rc;
  TRY(hipMemcpyAsync(value_mont, vals, kFieldLimbs[p->field_id] * 8, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
  });
}

int pcdhip_kzg_open(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g, const pcdhip_buf* p,
                    size_t len, const pcdhip_buf* blinding, size_t blinding_len, const uint64_t* z_mont, uint64_t* w_xyz_mont,
                    uint64_t* value_mont, uint64_t* random_v_mont) {
  return guarded([&]() -> int {
  if (!ctx || !powers_of_g || !p || !z_mont || !w_xyz_mont || !value_mont) return PCDHIP_E_ARG;
  if (!powers_of_g->shards.empty() || p->field_id != kCurveFr[powers_of_g->curve_id] || len > p->n || len >= (1ull << 31)) return PCDHIP_E_ARG;
  const size_t qn = len ? len - 1 : 0, bqn = blinding_len ? blinding_len - 1 : 0;
  if (qn > powers_of_g->n) return PCDHIP_E_ARG;  // upstream's TooManyCoefficients
  if (blinding && (!powers_of_gamma_g || !random_v_mont || !powers_of_gamma_g->shards.empty() ||
                   powers_of_gamma_g->curve_id != powers_of_g->curve_id || powers_of_gamma_g->group_id != powers_of_g->group_id ||
                   blinding->field_id != p->field_id || blinding_len > blinding->n || bqn > powers_of_gamma_g->n))
    return PCDHIP_E_ARG;
  BIND();
  uint32_t* q = nullptr;
  int rc = kzg_divide(ctx, p, len, z_mont, AUX_POLY_Q, &q, value_mont);
  rc = rc ? rc : kzg_witness(ctx, powers_of_g, q, qn, w_xyz_mont);
  if (rc || !blinding) return rc;
  // hiding: w += MSM(powers_of_gamma_g, blinding / (X - z)), random_v = blinding(z)
  const size_t jw = (size_t)pcdhip_point_limbs(powers_of_g->curve_id, powers_of_g->group_id) / 2 * 3;
  std::vector<uint64_t> both(2 * jw);
  memcpy(both.data(), w_xyz_mont, jw * 8);
  uint32_t* rq = nullptr;
  rc = kzg_divide(ctx, blinding, blinding_len, z_mont, AUX_POLY_R, &rq, random_v_mont);
  rc = rc ? rc : kzg_witness(ctx, powers_of_gamma_g, rq, bqn, &both[jw]);
  return rc ? rc : pcdhip_points_sum(ctx, powers_of_g->curve_id, powers_of_g->group_id, both.data(), 2, w_xyz_mont);
  });
}

// Both sides of the check are MSMs over one small uploaded vector (C_1..C_n, W_1..W_n, -g, -gamma_g): the left with the scalars
// (r_i, r_i z_i, sum r_i v_i, sum r_i rv_i), the right (sum r_i W_i) over its W range; the scalars are formed on the host with the
// field code of the RLC verification, the group and pairing work runs on the device.
int pcdhip_kzg_check(pcdhip_ctx* ctx, int curve_id, const uint64_t* g_xy, const uint64_t* gamma_g_xy, const uint64_t* h_xy,
                     const uint64_t* beta_h_xy, size_t n, const uint64_t* comms_xy, const uint8_t* comms_inf, const uint64_t* points_mont,
                     const uint64_t* values_mont, const uint64_t* w_xy, const uint8_t* w_inf, const uint64_t* random_v_mont,
                     const uint64_t* randomizers_canonical, int* ok) {
  return guarded([&]() -> int {
  if (!ctx || !valid_curve(curve_id) || !ok) return PCDHIP_E_ARG;
  *ok = 0;
  if (n == 0) { *ok = 1; return PCDHIP_OK; }
  if (!g_xy || !h_xy || !beta_h_xy || !comms_xy || !points_mont || !values_mont || !w_xy || (random_v_mont && !gamma_g_xy) ||
      (n > 1 && !randomizers_canonical) || n >= (1u << 20))
    return PCDHIP_E_ARG;
  BIND();
  const int fr = kCurveFr[curve_id];
  const size_t sl = (size_t)kFieldLimbs[fr], l1 = (size_t)pcdhip_point_limbs(curve_id, 1), l2 = (size_t)pcdhip_point_limbs(curve_id, 2);
  const size_t j1 = l1 / 2 * 3, nb = 2 * n + 2;
  std::vector<uint64_t> r(n * sl, 0), zc(n * sl), vc(n * sl), rvc(n * sl, 0);
  if (randomizers_canonical) memcpy(r.data(), randomizers_canonical, n * sl * 8);
  else r[0] = 1;
  for (size_t i = 0; i < n; i++) {
    mont_to_canonical(fr, points_mont + i * sl, &zc[i * sl]);
    mont_to_canonical(fr, values_mont + i * sl, &vc[i * sl]);
    if (random_v_mont) mont_to_canonical(fr, random_v_mont + i * sl, &rvc[i * sl]);
  }
  std::vector<uint64_t> sc(nb * sl, 0), pts(nb * l1, 0);
  std::vector<uint8_t> inf(nb, 0);
  std::vector<const uint64_t*> pr(n), pv(n), prv(n);
  for (size_t i = 0; i < n; i++) {
    pr[i] = &r[i * sl];
    pv[i] = &vc[i * sl];
    prv[i] = &rvc[i * sl];
    memcpy(&sc[i * sl], &r[i * sl], sl * 8);
    const uint64_t* zi = &zc[i * sl];
    scalar_lincomb(fr, &pr[i], &zi, 1, &sc[(n + i) * sl]);
    memcpy(&pts[i * l1], comms_xy + i * l1, l1 * 8);
    memcpy(&pts[(n + i) * l1], w_xy + i * l1, l1 * 8);
    inf[i] = comms_inf ? comms_inf[i] : 0;
    inf[n + i] = w_inf ? w_inf[i] : 0;
  }
  scalar_lincomb(fr, pr.data(), pv.data(), n, &sc[2 * n * sl]);
  memcpy(&pts[2 * n * l1], g_xy, l1 * 8);
  negate_point(curve_id, 1, &pts[2 * n * l1]);
  if (random_v_mont) {
    scalar_lincomb(fr, pr.data(), prv.data(), n, &sc[(2 * n + 1) * sl]);
    memcpy(&pts[(2 * n + 1) * l1], gamma_g_xy, l1 * 8);
    negate_point(curve_id, 1, &pts[(2 * n + 1) * l1]);
  } else {
    inf[2 * n + 1] = 1;
  }
  pcdhip_bases* b = nullptr;
  const int saved = ctx->precompute;
  ctx->precompute = 0;  // a handful of points used twice: no window copies
  int rc = pcdhip_bases_upload(ctx, curve_id, 1, pts.data(), inf.data(), nb, &b);
  ctx->precompute = saved;
  if (rc) return rc;
  std::vector<uint64_t> jac(2 * j1);
  // (pcdhip_msm_set_short: each of the two MSMs skips the buckets when it covers few enough pairs; a multi-device context's vector is
  //  sharded and keeps the bucket pipeline, which sums over the devices)
  const bool may_short = b->shards.empty();
  rc = may_short && nb <= ctx->msm_short_max ? msm_short_host(ctx, b, 0, sc.data(), nb, jac.data()) : pcdhip_msm(ctx, b, 0, sc.data(), nb, jac.data());
  if (!rc) rc = may_short && n <= ctx->msm_short_max ? msm_short_host(ctx, b, n, r.data(), n, &jac[j1]) : pcdhip_msm(ctx, b, n, r.data(), n, &jac[j1]);
  pcdhip_bases_free(ctx, b);
  if (rc) return rc;
  std::vector<uint64_t> aff(2 * l1);
  uint8_t aff_inf[2] = {0, 0};
  rc = pcdhip_to_affine(ctx, curve_id, 1, jac.data(), 2, aff.data(), aff_inf);
  if (rc) return rc;
  negate_point(curve_id, 1, aff.data());
  // e(-lhs, h) e(rhs, beta_h) == 1
  std::vector<uint64_t> g2s(2 * l2);
  memcpy(g2s.data(), h_xy, l2 * 8);
  memcpy(&g2s[l2], beta_h_xy, l2 * 8);
  const size_t gw = (size_t)pairing_entry(curve_id).gt_words / 2;
  std::vector<uint64_t> gt(gw), one(gw, 0);
  rc = pcdhip_multi_pairing(ctx, curve_id, aff.data(), aff_inf, g2s.data(), nullptr, 2, gt.data());
  if (rc) return rc;
  gt_one(curve_id, one.data());
  *ok = memcmp(gt.data(), one.data(), gw * 8) == 0 ? 1 : 0;
  return PCDHIP_OK;
  });
}

}  // extern "C"
