// CSR upload and the Groth16 witness map (h from the assignment) of libpcdhip.so.
#include "capi_internal.h"

using namespace pcd;

namespace {
// The small integers among the coefficients, recognised on the host by their C-ABI image (65 candidates, -32 .. 32, keyed by their
// first limb).  Real constraint systems are mostly such coefficients; the mat-vec kernels add instead of multiplying for them.
struct SmallCoeffTable {
  size_t limbs;
  std::vector<uint64_t> img;              // 65 x limbs
  std::vector<std::pair<uint64_t, int>> key;  // (first limb, c) sorted
  SmallCoeffTable(const FieldEntry& fe) : limbs((size_t)fe.abi_words / 2), img(65 * limbs) {
    for (int c = -32; c <= 32; c++) {
      fe.small_abi(c, (uint32_t*)&img[(size_t)(c + 32) * limbs]);
      key.push_back({img[(size_t)(c + 32) * limbs], c});
    }
    std::sort(key.begin(), key.end());
  }
  // the small integer equal to the coefficient at `w`, or 127
  int classify(const uint64_t* w) const {
    auto it = std::lower_bound(key.begin(), key.end(), std::make_pair(w[0], -64));
    for (; it != key.end() && it->first == w[0]; ++it)
      if (memcmp(w, &img[(size_t)(it->second + 32) * limbs], limbs * 8) == 0) return it->second;
    return 127;
  }
};
// ifft then coset_fft of v (tmp: ping-pong partner), result in v.  On a radix-2 domain the two transforms are chained without the copy back
// that an odd number of passes otherwise ends with (flag 4 of `inverse`: the first leaves its result in tmp, the second starts there and
// its last pass lands in v): six such copies of n elements per witness map gone (10 % of a 298-bit transform at 2^20).
int chain_transforms(pcdhip_ctx* ctx, int field_id, const Dom& d, uint32_t* v, uint32_t* tmp) {
  int rc;
  if (d.m != 1) {
    rc = domain_transform(ctx, field_id, d, v, tmp, 1, 0, nullptr, nullptr); if (rc) return rc;
    return domain_transform(ctx, field_id, d, v, tmp, 0, 1, nullptr, nullptr);
  }
  int P = 0;
  rc = domain_transform(ctx, field_id, d, v, tmp, 1 | 4, 0, nullptr, &P); if (rc) return rc;
  uint32_t *s2 = (P & 1) ? tmp : v, *t2 = (P & 1) ? v : tmp;
  return domain_transform(ctx, field_id, d, s2, t2, 0 | 4, 1, nullptr, &P);  // P odd: ends in v; P even: stays in v
}
}  // namespace

namespace pcd {
// device layout of one CSR matrix inside `d`: row_ptr | coeff (device image) | col | nl | long_rows | lc  (DevCsr, common.h)
size_t csr_bytes(const pcdhip_csr* m, const FieldEntry& fe, size_t off[6]) {
  const uint64_t nnz = m->row_ptr[m->num_rows];
  auto up8 = [](size_t x) { return (x + 7) / 8 * 8; };
  off[0] = 0;
  off[1] = (m->num_rows + 1) * 8;
  off[2] = off[1] + up8(nnz * fe.words * 4);
  off[3] = off[2] + up8(nnz * 4);
  off[4] = off[3] + up8((m->num_rows + 1) * 4);
  off[5] = off[4] + up8((m->num_rows + 1) * 4);   // (at most every row is long)
  return off[5] + up8(nnz + 8);
}
// host-side shape check of a caller's CSR matrix: row_ptr starts at 0 and never decreases, every column index is below
// `num_cols` (the kernels index the assignment with it) -- PCDHIP_E_ARG instead of an out-of-bounds device read
int validate_csr(const pcdhip_csr* m, size_t num_cols) {
  if (!m || !m->row_ptr || (m->num_rows >> 31) || m->row_ptr[0] != 0) return PCDHIP_E_ARG;
  for (uint64_t r = 0; r < m->num_rows; r++) if (m->row_ptr[r + 1] < m->row_ptr[r]) return PCDHIP_E_ARG;
  const uint64_t nnz = m->row_ptr[m->num_rows];
  if (nnz >> 31) return PCDHIP_E_ARG;
  if (nnz && (!m->col || !m->coeff)) return PCDHIP_E_ARG;
  uint32_t worst = 0;
  for (uint64_t k = 0; k < nnz; k++) worst = std::max(worst, m->col[k]);
  return (nnz && worst >= num_cols) ? PCDHIP_E_ARG : PCDHIP_OK;
}
int upload_csr_to(pcdhip_ctx* ctx, const pcdhip_csr* m, const FieldEntry& fe, size_t num_cols, char* d, DevCsr* out) try {
  int vrc = validate_csr(m, num_cols);
  if (vrc) return vrc;
  const uint64_t nnz = m->row_ptr[m->num_rows], rows = m->num_rows;
  size_t off[6];
  csr_bytes(m, fe, off);
  // classify, and reorder every row: light entries (small integer coefficients) first
  const size_t limbs = (size_t)fe.abi_words / 2;
  const SmallCoeffTable table(fe);
  std::vector<uint32_t> col(nnz), nl(rows + 1, 0), long_rows;
  std::vector<int8_t> lc(nnz + 8, 0);
  std::vector<uint64_t> heavy(nnz * limbs, 0);   // ABI coefficients in the new order (light slots stay zero)
  for (uint64_t r = 0; r < rows; r++) {
    const uint64_t lo = m->row_ptr[r], hi = m->row_ptr[r + 1];
    uint64_t front = lo, back = hi;
    for (uint64_t k = lo; k < hi; k++) {
      const int c = table.classify(m->coeff + k * limbs);
      if (c != 127) { col[front] = m->col[k]; lc[front] = (int8_t)c; front++; }
      else { back--; col[back] = m->col[k]; lc[back] = 127; memcpy(&heavy[back * limbs], m->coeff + k * limbs, limbs * 8); }
    }
    nl[r] = (uint32_t)(front - lo);
    if (hi - lo > SPMV_LONG_ROW) long_rows.push_back((uint32_t)r);
  }
  TRY(hipMemcpyAsync(d + off[0], m->row_ptr, (rows + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  TRY(hipMemcpyAsync(d + off[3], nl.data(), (rows + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!long_rows.empty()) TRY(hipMemcpyAsync(d + off[4], long_rows.data(), long_rows.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (nnz) {
    TRY(ctx->aux_ws.ensure(AUX_SCAL, nnz * fe.abi_words * 4));
    TRY(hipMemcpyAsync(ctx->aux_ws.buf[AUX_SCAL], heavy.data(), nnz * fe.abi_words * 4, hipMemcpyHostToDevice, ctx->stream));
    TRY(fe.convert(ctx->stream, (const uint32_t*)ctx->aux_ws.buf[AUX_SCAL], (uint32_t*)(d + off[1]), (uint32_t)nnz, 0));
    TRY(hipMemcpyAsync(d + off[2], col.data(), nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    TRY(hipMemcpyAsync(d + off[5], lc.data(), nnz, hipMemcpyHostToDevice, ctx->stream));
  }
  TRY(hipStreamSynchronize(ctx->stream));  // the host vectors above and the staging slot (reused by the next matrix) are done with
  out->rp = (const uint64_t*)(d + off[0]);
  out->coeff = (const uint32_t*)(d + off[1]);
  out->col = (const uint32_t*)(d + off[2]);
  out->nl = (const uint32_t*)(d + off[3]);
  out->long_rows = (const uint32_t*)(d + off[4]);
  out->lc = (const int8_t*)(d + off[5]);
  out->n_long = (uint32_t)long_rows.size();
  out->rows = (uint32_t)m->num_rows;
  return PCDHIP_OK;
} catch (const std::bad_alloc&) { return PCDHIP_E_OOM; }
int upload_csr(pcdhip_ctx* ctx, int slot, const pcdhip_csr* m, const FieldEntry& fe, size_t num_cols, DevCsr* out) {
  if (!m || !m->row_ptr) return PCDHIP_E_ARG;
  size_t off[6];
  TRY(ctx->aux_ws.ensure(slot, csr_bytes(m, fe, off) + 64));
  return upload_csr_to(ctx, m, fe, num_cols, (char*)ctx->aux_ws.buf[slot], out);
}

// One of the three independent chains of the witness map on `ctx`'s device and stream: v = M z (k == 0: plus the input-consistency
// rows), then ifft and coset_fft over the domain d, in ctx's own AUX_A / AUX_B / AUX_C buffer `slot` (tmp: AUX_FFT_TMP).
int witness_chain_dev(pcdhip_ctx* ctx, int field_id, const DevCsr& mat, int k, const uint32_t* z_dev, size_t num_inputs, const Dom& d, int slot,
                      bool transforms) {
  const FieldEntry& fe = field_entry(field_id);
  const size_t vb = (size_t)d.n * fe.words * 4;
  TRY(ctx->aux_ws.ensure(slot, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  uint32_t* v = (uint32_t*)ctx->aux_ws.buf[slot];
  uint32_t* tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
  TRY(fe.spmv(ctx->stream, mat, z_dev, (uint32_t)num_inputs, k == 0 ? 1 : 0, d.n, v));
  if (!transforms) return PCDHIP_OK;
  return chain_transforms(ctx, field_id, d, v, tmp);
}
// h = coset_ifft((a o b - c) / Z) from the three transformed chains in ctx's AUX_A, AUX_B, AUX_C; h ends up in AUX_A
int witness_finish_dev(pcdhip_ctx* ctx, int field_id, const Dom& d, const uint32_t* b_at, const uint32_t* c_at) {
  const FieldEntry& fe = field_entry(field_id);
  uint32_t* a = (uint32_t*)ctx->aux_ws.buf[AUX_A];
  const uint32_t* b = b_at ? b_at : (const uint32_t*)ctx->aux_ws.buf[AUX_B];
  const uint32_t* c = c_at ? c_at : (const uint32_t*)ctx->aux_ws.buf[AUX_C];
  uint32_t* tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
  int rc;
  const FftTables* t;
  if (d.m == 1) {
    rc = get_tables(ctx, field_id, d.a, &t); if (rc) return rc;
    TRY(fe.mul_sub_divz(ctx->stream, *t, a, b, c, d.a));
  } else {
    rc = get_mixed_tables(ctx, field_id, d, &t); if (rc) return rc;
    TRY(fe.mixed_mul_sub_divz(ctx->stream, *t, a, b, c, d.n));
  }
  return domain_transform(ctx, field_id, d, a, tmp, 1, 1, nullptr, nullptr);
}
// h (d.n elements, device image) left in aux slot AUX_A; z_dev: m elements on device; mats: A, B, C on device
int witness_map_dev(pcdhip_ctx* ctx, int field_id, const DevCsr mats[3], const uint32_t* z_dev, size_t num_inputs, Dom* dom_out,
                    hipEvent_t after_spmv) {
  const FieldEntry& fe = field_entry(field_id);
  if (mats[0].rows != mats[1].rows || mats[0].rows != mats[2].rows) return PCDHIP_E_ARG;
  Dom d;
  int rc = pick_domain(field_id, (size_t)mats[0].rows + num_inputs, &d);
  if (rc) return rc;
  const uint32_t n = d.n;
  const size_t vb = (size_t)n * fe.words * 4;
  hipStream_t st = ctx->stream;
  if (d.m == 1) {
    // radix-2 domain: the three chains live back to back in AUX_A (a | b | c) and every pass of their transforms is ONE launch for all
    // three (grid.y): 6 launches instead of 18 -- inside a proof every launch of the map queues behind the MSMs' resident accumulation
    // waves, so the map's length is its launch count as much as its work
    TRY(ctx->aux_ws.ensure(AUX_A, 3 * vb));
    TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, 3 * vb));
    uint32_t* a = (uint32_t*)ctx->aux_ws.buf[AUX_A];
    uint32_t* tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
    const size_t ew = (size_t)n * fe.words;
    TRY(fe.spmv3(st, mats, z_dev, (uint32_t)num_inputs, n, a, ew));
    if (after_spmv) TRY(hipEventRecord(after_spmv, st));
    const FftTables* t;
    rc = get_tables(ctx, field_id, d.a, &t);
    if (rc) return rc;
    int P = 0;
    TRY(fe.fft_run_batched(st, *t, a, tmp, d.a, 1 | 4, 0, &P, 3));                 // ifft, result left where the last pass wrote it
    uint32_t *s2 = (P & 1) ? tmp : a, *t2 = (P & 1) ? a : tmp;
    TRY(fe.fft_run_batched(st, *t, s2, t2, d.a, 0 | 4, 1, &P, 3));                 // coset fft from there: lands in a | b | c
    rc = witness_finish_dev(ctx, field_id, d, a + ew, a + 2 * ew);
    if (rc) return rc;
    *dom_out = d;
    return PCDHIP_OK;
  }
  TRY(ctx->aux_ws.ensure(AUX_A, vb));
  TRY(ctx->aux_ws.ensure(AUX_B, vb));
  TRY(ctx->aux_ws.ensure(AUX_C, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  uint32_t *a = (uint32_t*)ctx->aux_ws.buf[AUX_A], *b = (uint32_t*)ctx->aux_ws.buf[AUX_B], *c = (uint32_t*)ctx->aux_ws.buf[AUX_C];
  uint32_t* tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
  uint32_t* vecs[3] = {a, b, c};
  for (int k = 0; k < 3; k++)
    TRY(fe.spmv(st, mats[k], z_dev, (uint32_t)num_inputs, k == 0 ? 1 : 0, n, vecs[k]));
  if (after_spmv) TRY(hipEventRecord(after_spmv, st));
  // 3 x (ifft, coset_fft), pointwise, coset_ifft
  for (uint32_t* v : vecs) { rc = chain_transforms(ctx, field_id, d, v, tmp); if (rc) return rc; }
  rc = witness_finish_dev(ctx, field_id, d);
  if (rc) return rc;
  *dom_out = d;
  return PCDHIP_OK;
}

int upload_three(pcdhip_ctx* ctx, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, const FieldEntry& fe, size_t num_vars,
                 DevCsr out[3]) {
  const pcdhip_csr* ms[3] = {A, B, C};
  const int slots[3] = {AUX_CSR_RP, AUX_CSR_COL, AUX_CSR_COEF};  // one aux slot per matrix
  for (int k = 0; k < 3; k++) { int rc = upload_csr(ctx, slots[k], ms[k], fe, num_vars, &out[k]); if (rc) return rc; }
  return PCDHIP_OK;
}
}  // namespace pcd

extern "C" {

int pcdhip_groth16_witness_map(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C,
                               const uint64_t* z, size_t num_vars, size_t num_inputs, uint64_t* h_out) {
  if (!ctx || !valid_field(field_id) || !A || !B || !C || !z || !h_out || num_inputs == 0 || num_inputs > num_vars) return PCDHIP_E_ARG;
  if (num_vars >> 31) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(field_id);
  TRY(ctx->aux_ws.ensure(AUX_Z, num_vars * fe.words * 4));
  TRY(ctx->aux_ws.ensure(AUX_Z_CANON, num_vars * fe.abi_words * 4));
  TRY(hipMemcpyAsync(ctx->aux_ws.buf[AUX_Z_CANON], z, num_vars * fe.abi_words * 4, hipMemcpyHostToDevice, ctx->stream));
  TRY(fe.convert(ctx->stream, (const uint32_t*)ctx->aux_ws.buf[AUX_Z_CANON], (uint32_t*)ctx->aux_ws.buf[AUX_Z], (uint32_t)num_vars, 0));
  Dom dom;
  DevCsr mats[3];
  int rc = upload_three(ctx, A, B, C, fe, num_vars, mats);
  if (rc) return rc;
  rc = witness_map_dev(ctx, field_id, mats, (const uint32_t*)ctx->aux_ws.buf[AUX_Z], num_inputs, &dom);
  if (rc) return rc;
  const uint32_t n = dom.n;
  TRY(ctx->aux_ws.ensure(AUX_H_CANON, (size_t)n * fe.abi_words * 4));
  TRY(fe.convert(ctx->stream, (const uint32_t*)ctx->aux_ws.buf[AUX_A], (uint32_t*)ctx->aux_ws.buf[AUX_H_CANON], n, 1));
  TRY(hipMemcpyAsync(h_out, ctx->aux_ws.buf[AUX_H_CANON], (size_t)n * fe.abi_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}

// The witness map ALONE over the matrices resident with a key (pcdhip_g16_pk_set_r1cs), nothing else running: what
// pcdhip_groth16_prove queues on the context's stream while its MSMs run on the side streams.  out_ms = device time of
// [the three mat-vecs, the seven transforms + the pointwise step, both].  h_out may be null (timing only).
int pcdhip_g16_witness_map_resident(pcdhip_ctx* ctx, const pcdhip_g16_pk* pk, const uint64_t* z, uint64_t* h_out, float out_ms[3]) {
  if (!ctx || !pk || !z) return PCDHIP_E_ARG;
  if (!pk->shards.empty()) pk = pk->shards[0];
  if (!pk->r1cs_dev) return PCDHIP_E_ARG;
  BIND();
  const int fr = kCurveFr[pk->curve_id];
  const FieldEntry& fe = field_entry(fr);
  const size_t m = pk->num_vars;
  TRY(ctx->aux_ws.ensure(AUX_Z, m * fe.words * 4));
  TRY(ctx->aux_ws.ensure(AUX_Z_CANON, m * fe.abi_words * 4));
  TRY(hipMemcpyAsync(ctx->aux_ws.buf[AUX_Z_CANON], z, m * fe.abi_words * 4, hipMemcpyHostToDevice, ctx->stream));
  TRY(fe.convert(ctx->stream, (const uint32_t*)ctx->aux_ws.buf[AUX_Z_CANON], (uint32_t*)ctx->aux_ws.buf[AUX_Z], (uint32_t)m, 0));
  DevCsr mats[3];
  for (int k = 0; k < 3; k++) mats[k] = pk->mats[k];
  EventSet<3> ev;
  TRY(ev.create());
  TRY(hipEventRecord(ev[0], ctx->stream));
  Dom dom;
  int rc = witness_map_dev(ctx, fr, mats, (const uint32_t*)ctx->aux_ws.buf[AUX_Z], pk->num_inputs, &dom, ev[1]);
  if (rc) return rc;
  TRY(hipEventRecord(ev[2], ctx->stream));
  if (h_out) {
    TRY(ctx->aux_ws.ensure(AUX_H_CANON, (size_t)dom.n * fe.abi_words * 4));
    TRY(fe.convert(ctx->stream, (const uint32_t*)ctx->aux_ws.buf[AUX_A], (uint32_t*)ctx->aux_ws.buf[AUX_H_CANON], dom.n, 1));
    TRY(hipMemcpyAsync(h_out, ctx->aux_ws.buf[AUX_H_CANON], (size_t)dom.n * fe.abi_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  TRY(hipStreamSynchronize(ctx->stream));
  if (out_ms) {
    (void)hipEventElapsedTime(&out_ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&out_ms[1], ev[1], ev[2]);
    (void)hipEventElapsedTime(&out_ms[2], ev[0], ev[2]);
  }
  return PCDHIP_OK;
}

}  // extern "C"
