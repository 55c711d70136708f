// ------------------------------------------------------------------------------------------------ K9: Marlin's AHP rounds 2 and 3
// (marlin.hip.h and the t(X) kernels of inst_field.hip: r(alpha, .) on H, the transposed mat-vec behind t(X), the rational sumcheck).
// Every call queues its launches on the context's stream and returns: nothing here waits for the device except the upload of the matrices.
// K10, the index on device (the arithmetisation onto K, the coefficients, the evaluations on B, the twelve commitments), follows below;
// pcdhip_marlin_index_build waits for its own uploads and for the end of its work.  K11 at the end: round 1 (the assignment on H, z_A and
// z_B over the forward matrices, w) and the first sumcheck (q in one launch, h_1 and g_1).  K12 behind it: the second sumcheck (q = a - b f in
// one launch; f, g_2 and h_2 from an index in one call).
#include <stdlib.h>

#include "capi_internal.h"

using namespace pcd;

namespace {
// (AUX_MARLIN_WS: the vectors of a K11 driver in one block; AUX_MARLIN_BLIND: the blinding coefficients of a call, staged from the host)
// (AUX_MARLIN_MUL_B: route 2 of the K12 driver, the second operand of its polynomial product over the product's domain)
enum { AUX_MARLIN_PART = AUX_FB_OUT + 5, AUX_MARLIN_A, AUX_MARLIN_B, AUX_MARLIN_WS, AUX_MARLIN_BLIND, AUX_MARLIN_MUL_B };
const size_t kMaxLen = (size_t)1 << 31;

bool is_domain_size(int field_id, size_t n) { return n != 0 && n < kMaxLen && pcdhip_domain_size(field_id, n) == n; }

// ark-marlin `reindex_by_subdomain`: where variable c of the constraint system sits in H, the instance variables on the subdomain X
inline size_t reindex(size_t c, size_t x_n, size_t period) {
  if (c < x_n) return c * period;
  const size_t i = c - x_n;
  return i + i / (period - 1) + 1;
}

// the inputs of a sumcheck call: twelve vectors of one field, n elements each; row_col as a whole, or all of its entries, may be null
struct SumcheckArgs {
  int field_id;
  const uint32_t *row[3], *col[3], *rc[3], *val[3];
};
int sumcheck_args(const uint64_t* alpha, const uint64_t* beta, const uint64_t* coeff, const pcdhip_buf* const row[3], const pcdhip_buf* const col[3],
                  const pcdhip_buf* const row_col[3], const pcdhip_buf* const val[3], size_t n, SumcheckArgs* out) {
  if (!alpha || !beta || !coeff || !row || !col || !val || n >= kMaxLen) return PCDHIP_E_ARG;
  for (int m = 0; m < 3; m++) if (!row[m] || !col[m] || !val[m]) return PCDHIP_E_ARG;
  const int f = row[0]->field_id;
  int have_rc = 0;
  for (int m = 0; m < 3; m++) have_rc += (row_col && row_col[m]) ? 1 : 0;
  if (have_rc != 0 && have_rc != 3) return PCDHIP_E_ARG;
  for (int m = 0; m < 3; m++) {
    const pcdhip_buf* v[4] = {row[m], col[m], val[m], have_rc ? row_col[m] : row[m]};
    for (const pcdhip_buf* b : v) if (b->field_id != f || n > b->n) return PCDHIP_E_ARG;
    out->row[m] = row[m]->dptr; out->col[m] = col[m]->dptr; out->val[m] = val[m]->dptr;
    out->rc[m] = have_rc ? row_col[m]->dptr : nullptr;
  }
  out->field_id = f;
  return PCDHIP_OK;
}
bool is_input(const SumcheckArgs& a, const uint32_t* p) {
  for (int m = 0; m < 3; m++) if (p == a.row[m] || p == a.col[m] || p == a.val[m] || (a.rc[m] && p == a.rc[m])) return true;
  return false;
}
void mats_release(pcdhip_marlin_mats* h) {
  if (h->dev) (void)hipFree(h->dev);
  if (h->dev_fwd) (void)hipFree(h->dev_fwd);
  delete h;
}
// bit 0 of a handle's forms: the three matrices transposed, their rows at pi's places, and the segment tables of the long rows
int upload_transposed(pcdhip_ctx* ctx, const FieldEntry& fe, const pcdhip_csr* const ms[3], pcdhip_marlin_mats* h) {
  const size_t domain_h_n = h->domain_h_n, domain_x_n = h->domain_x_n, num_cols = h->num_cols, rows = h->num_rows;
  const size_t limbs = (size_t)fe.abi_words / 2, period = domain_h_n / domain_x_n;
  // segment length of the long rows: MARLIN_T_SEG, or the tuning knob PCDHIP_MARLIN_SEG (64 .. 2^20) read at upload
  uint32_t seg_len = MARLIN_T_SEG;
  if (const char* e = getenv("PCDHIP_MARLIN_SEG")) { const long v = atol(e); if (v >= 64 && v <= (1 << 20)) seg_len = (uint32_t)v; }
  std::vector<uint32_t> perm(num_cols);
  for (size_t c = 0; c < num_cols; c++) perm[c] = (uint32_t)reindex(c, domain_x_n, period);
  // (num_cols <= |H| keeps every image below |H|: pi maps [0, |H|) onto itself)
  HostCsrT tr[3];
  size_t total = 0, base[3], off[6];
  for (int k = 0; k < 3; k++) {
    int rc = transpose_csr(ms[k], num_cols, limbs, &tr[k], perm.data(), domain_h_n);
    if (rc) return rc;
    base[k] = total;
    total += csr_bytes(&tr[k].view, fe, off) + 64;
  }
  // the segments of the rows that a lane does not serve, by (row, matrix)
  std::vector<MarlinSeg> segs;
  std::vector<uint32_t> long_out, long_seg_lo;
  for (size_t j = 0; j < domain_h_n; j++) {
    bool any = false;
    for (uint32_t k = 0; k < 3; k++) {
      const uint64_t lo = tr[k].rp[j], hi = tr[k].rp[j + 1];
      if (hi - lo <= SPMV_LONG_ROW) continue;
      if (!any) { long_out.push_back((uint32_t)j); long_seg_lo.push_back((uint32_t)segs.size()); any = true; }
      for (uint64_t s = lo; s < hi; s += seg_len) segs.push_back({k, (uint32_t)j, s, std::min<uint64_t>(hi, s + seg_len)});
    }
  }
  if (segs.size() >> 31) return PCDHIP_E_ARG;
  long_seg_lo.push_back((uint32_t)segs.size());
  const size_t seg_off = total, lo_off = seg_off + segs.size() * sizeof(MarlinSeg), sl_off = lo_off + (long_out.size() + 2) / 2 * 8;
  total = sl_off + (long_seg_lo.size() + 2) / 2 * 8;
  h->seg_len = seg_len;
  hipError_t e = hipMalloc(&h->dev, total + 64);
  if (e != hipSuccess) { h->dev = nullptr; return fail(ctx, e); }
  char* d = (char*)h->dev;
  int rc = PCDHIP_OK;
  for (int k = 0; k < 3 && !rc; k++) rc = upload_csr_to(ctx, &tr[k].view, fe, std::max<size_t>(rows, 1), d + base[k], &h->view.m[k]);
  if (!rc && !segs.empty()) {
    e = hipMemcpyAsync(d + seg_off, segs.data(), segs.size() * sizeof(MarlinSeg), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + lo_off, long_out.data(), long_out.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + sl_off, long_seg_lo.data(), long_seg_lo.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the host vectors above are done with
    if (e != hipSuccess) rc = fail(ctx, e);
  }
  if (rc) return rc;
  h->view.rows = (uint32_t)domain_h_n;
  h->view.segs = (const MarlinSeg*)(d + seg_off); h->view.n_segs = (uint32_t)segs.size();
  h->view.long_out = (const uint32_t*)(d + lo_off); h->view.long_seg_lo = (const uint32_t*)(d + sl_off);
  h->view.n_long_out = (uint32_t)long_out.size();
  return PCDHIP_OK;
}
// bit 1: the forward A, B, C as the witness map's mat-vec takes them (upload_csr_to: small coefficients first in a row, long rows listed)
int upload_forward(pcdhip_ctx* ctx, const FieldEntry& fe, const pcdhip_csr* const ms[3], pcdhip_marlin_mats* h) {
  size_t base[3], total = 0, off[6];
  for (int k = 0; k < 3; k++) { base[k] = total; total += csr_bytes(ms[k], fe, off) + 64; }
  hipError_t e = hipMalloc(&h->dev_fwd, total + 64);
  if (e != hipSuccess) { h->dev_fwd = nullptr; return fail(ctx, e); }
  for (int k = 0; k < 3; k++) {
    int rc = upload_csr_to(ctx, ms[k], fe, h->num_cols, (char*)h->dev_fwd + base[k], &h->fwd[k]);
    if (rc) return rc;
  }
  return PCDHIP_OK;
}
// r(x, .) over the domain of n elements into out (n ABI elements on the device); the caller has bound the device and checked n
int lagrange_dev(pcdhip_ctx* ctx, int field_id, size_t n, const uint64_t* x_mont, uint32_t* out) {
  const FieldEntry& fe = field_entry(field_id);
  if (n == 1) {
    TRY(fe.marlin_lagrange(ctx->stream, nullptr, nullptr, 1, (const uint32_t*)x_mont, 1, out));
    return PCDHIP_OK;
  }
  Dom d;
  int rc = pick_domain(field_id, n, &d);
  if (rc) return rc;
  const FftTables* t;
  rc = d.m == 1 ? get_tables(ctx, field_id, d.a, &t) : get_mixed_tables(ctx, field_id, d, &t);
  if (rc) return rc;
  TRY(fe.marlin_lagrange(ctx->stream, t->consts, t->tw_fwd, d.n / d.m, (const uint32_t*)x_mont, d.n, out));
  return PCDHIP_OK;
}
// t on H from r_alpha (num_rows elements) into t_out (|H| elements), both ABI on the device and distinct
int t_evals_dev(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const uint64_t* eta_mont, const uint32_t* r_alpha, uint32_t* t_out) {
  const FieldEntry& fe = field_entry(mats->field_id);
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_PART, std::max<size_t>(mats->view.n_segs, 1) * fe.words * 4));
  TRY(fe.marlin_t_evals(ctx->stream, mats->view, (const uint32_t*)eta_mont, r_alpha, (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_PART], t_out, nullptr));
  return PCDHIP_OK;
}
}  // namespace

extern "C" {

int pcdhip_domain_bivariate_lagrange(pcdhip_ctx* ctx, int field_id, size_t domain_n, const uint64_t* x_mont, pcdhip_buf* out) {
  if (!ctx || !valid_field(field_id) || !x_mont || !out || out->field_id != field_id) return PCDHIP_E_ARG;
  if (!is_domain_size(field_id, domain_n)) return PCDHIP_E_SIZE_UNSUPPORTED;
  if (domain_n > out->n) return PCDHIP_E_ARG;
  BIND();
  return lagrange_dev(ctx, field_id, domain_n, x_mont, out->dptr);
}

int pcdhip_marlin_mats_upload(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                              size_t domain_h_n, size_t domain_x_n, pcdhip_marlin_mats** out) {
  return pcdhip_marlin_mats_upload_ex(ctx, field_id, A, B, C, num_cols, domain_h_n, domain_x_n, 1u, out);
}

int pcdhip_marlin_mats_upload_ex(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                                 size_t domain_h_n, size_t domain_x_n, uint32_t forms, pcdhip_marlin_mats** out) {
  if (!ctx || !valid_field(field_id) || !A || !B || !C || !out || forms == 0 || forms > 3) return PCDHIP_E_ARG;
  if (!is_domain_size(field_id, domain_h_n) || !is_domain_size(field_id, domain_x_n) || domain_h_n % domain_x_n != 0) return PCDHIP_E_ARG;
  if (A->num_rows != B->num_rows || A->num_rows != C->num_rows || A->num_rows > domain_h_n || num_cols > domain_h_n) return PCDHIP_E_ARG;
  const pcdhip_csr* ms[3] = {A, B, C};
  for (int k = 0; k < 3; k++) { int rc = validate_csr(ms[k], num_cols); if (rc) return rc; }
  BIND();
  return guarded([&]() -> int {
    const FieldEntry& fe = field_entry(field_id);
    const size_t rows = A->num_rows;
    pcdhip_marlin_mats* h = new pcdhip_marlin_mats();
    h->field_id = field_id; h->domain_h_n = domain_h_n; h->domain_x_n = domain_x_n; h->num_rows = rows; h->num_cols = num_cols;
    h->forms = forms;
    int rc = (forms & 1) ? upload_transposed(ctx, fe, ms, h) : PCDHIP_OK;
    if (!rc && (forms & 2)) rc = upload_forward(ctx, fe, ms, h);
    if (rc) { mats_release(h); return rc; }
    *out = h;
    return PCDHIP_OK;
  });
}

void pcdhip_marlin_mats_free(pcdhip_ctx* ctx, pcdhip_marlin_mats* mats) {
  if (!mats) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  mats_release(mats);
}

int pcdhip_marlin_mats_info(const pcdhip_marlin_mats* mats, uint64_t out[4]) {
  if (!mats || !out) return PCDHIP_E_ARG;
  out[0] = mats->seg_len; out[1] = mats->view.n_segs; out[2] = mats->view.n_long_out;
  out[3] = mats->view.n_segs ? 3 : 1;
  return PCDHIP_OK;
}

int pcdhip_marlin_t_evals(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const uint64_t* eta_mont, const pcdhip_buf* r_alpha, pcdhip_buf* t_out) {
  if (!ctx || !mats || !eta_mont || !r_alpha || !t_out) return PCDHIP_E_ARG;
  if (r_alpha->field_id != mats->field_id || t_out->field_id != mats->field_id || r_alpha->dptr == t_out->dptr) return PCDHIP_E_ARG;
  if (r_alpha->n < mats->num_rows || t_out->n < mats->domain_h_n || !(mats->forms & 1)) return PCDHIP_E_ARG;
  BIND();
  return t_evals_dev(ctx, mats, eta_mont, r_alpha->dptr, t_out->dptr);
}

int pcdhip_marlin_sumcheck_ab(pcdhip_ctx* ctx, const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* coeff_mont,
                              const pcdhip_buf* const row[3], const pcdhip_buf* const col[3], const pcdhip_buf* const row_col[3],
                              const pcdhip_buf* const val[3], size_t n, pcdhip_buf* a_out, pcdhip_buf* b_out) {
  if (!ctx || !a_out || !b_out) return PCDHIP_E_ARG;
  SumcheckArgs a;
  int rc = sumcheck_args(alpha_mont, beta_mont, coeff_mont, row, col, row_col, val, n, &a);
  if (rc) return rc;
  if (a_out->field_id != a.field_id || b_out->field_id != a.field_id || n > a_out->n || n > b_out->n) return PCDHIP_E_ARG;
  if (a_out->dptr == b_out->dptr || is_input(a, a_out->dptr) || is_input(a, b_out->dptr)) return PCDHIP_E_ARG;
  if (n == 0) return PCDHIP_OK;
  BIND();
  TRY(field_entry(a.field_id).marlin_sumcheck_ab(ctx->stream, (const uint32_t*)alpha_mont, (const uint32_t*)beta_mont, (const uint32_t*)coeff_mont,
                                                 a.row, a.col, a.rc, a.val, n, a_out->dptr, b_out->dptr));
  return PCDHIP_OK;
}

int pcdhip_marlin_sumcheck_f(pcdhip_ctx* ctx, const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* coeff_mont,
                             const pcdhip_buf* const row[3], const pcdhip_buf* const col[3], const pcdhip_buf* const row_col[3],
                             const pcdhip_buf* const val[3], size_t n, pcdhip_buf* f_out) {
  if (!ctx || !f_out) return PCDHIP_E_ARG;
  SumcheckArgs a;
  int rc = sumcheck_args(alpha_mont, beta_mont, coeff_mont, row, col, row_col, val, n, &a);
  if (rc) return rc;
  if (f_out->field_id != a.field_id || n > f_out->n || is_input(a, f_out->dptr)) return PCDHIP_E_ARG;
  if (n == 0) return PCDHIP_OK;
  BIND();
  const FieldEntry& fe = field_entry(a.field_id);
  const size_t vb = n * fe.abi_words * 4;
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_A, vb));
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_B, vb));
  uint32_t *av = (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_A], *bv = (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_B];
  TRY(fe.marlin_sumcheck_ab(ctx->stream, (const uint32_t*)alpha_mont, (const uint32_t*)beta_mont, (const uint32_t*)coeff_mont, a.row, a.col, a.rc,
                            a.val, n, av, bv));
  TRY(fe.vec_batch_inverse(ctx->stream, bv, n, nullptr, bv));
  TRY(fe.vec_mul(ctx->stream, av, bv, n, f_out->dptr, 1));
  return PCDHIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ K10: the index on device
// One matrix in the index's entry order: row by row, ascending column inside a row, equal columns as the CSR gives them.  A matrix whose
// rows are ascending already is uploaded from the caller's arrays as they stand; otherwise col and coeff are copied and the offending
// rows sorted stably (an index permutation per row).
namespace {
struct OrderedCsr {
  const uint32_t* col; const uint64_t* coeff;
  std::vector<uint32_t> col_own; std::vector<uint64_t> coeff_own;
};
void order_csr(const pcdhip_csr* m, size_t limbs, OrderedCsr* o) {
  o->col = m->col; o->coeff = m->coeff;
  std::vector<uint32_t> perm;
  for (uint64_t r = 0; r < m->num_rows; r++) {
    const uint64_t lo = m->row_ptr[r], hi = m->row_ptr[r + 1];
    bool ascending = true;
    for (uint64_t k = lo + 1; k < hi && ascending; k++) ascending = m->col[k - 1] <= m->col[k];
    if (ascending) continue;
    if (o->col_own.empty()) {
      const uint64_t nnz = m->row_ptr[m->num_rows];
      o->col_own.assign(m->col, m->col + nnz);
      o->coeff_own.assign(m->coeff, m->coeff + nnz * limbs);
      o->col = o->col_own.data(); o->coeff = o->coeff_own.data();
    }
    perm.resize(hi - lo);
    for (uint64_t k = lo; k < hi; k++) perm[k - lo] = (uint32_t)(k - lo);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return m->col[lo + a] < m->col[lo + b]; });
    for (uint64_t k = lo; k < hi; k++) {
      o->col_own[k] = m->col[lo + perm[k - lo]];
      memcpy(&o->coeff_own[k * limbs], m->coeff + (lo + perm[k - lo]) * limbs, limbs * 8);
    }
  }
}
void index_release(pcdhip_marlin_index* h) {
  for (int f = 0; f < 3; f++) if (h->block[f]) (void)hipFree(h->block[f]);
  delete h;
}
inline size_t up64(size_t x) { return (x + 63) & ~(size_t)63; }
// the events behind pcdhip_marlin_index_timings: [0], [1] around the arithmetisation, then per vector its start, its coefficients, its
// evaluations on B.  Recording one does not wait for the device; the times are read after the build's own final wait
struct BuildEvents {
  hipEvent_t ev[2 + 3 * 12] = {};
  hipError_t make() {
    for (hipEvent_t& e : ev) { hipError_t rc = hipEventCreate(&e); if (rc != hipSuccess) return rc; }
    return hipSuccess;
  }
  ~BuildEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};
}  // namespace

extern "C" {

int pcdhip_marlin_index_build(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                              size_t domain_h_n, size_t domain_x_n, size_t domain_k_n, size_t domain_b_n, int keep, pcdhip_marlin_index** out) {
  if (!ctx || !valid_field(field_id) || !A || !B || !C || !out || keep < 0 || keep > 7) return PCDHIP_E_ARG;
  if (!is_domain_size(field_id, domain_h_n) || !is_domain_size(field_id, domain_x_n) || domain_h_n % domain_x_n != 0) return PCDHIP_E_ARG;
  if (A->num_rows != B->num_rows || A->num_rows != C->num_rows || A->num_rows > domain_h_n || num_cols > domain_h_n) return PCDHIP_E_ARG;
  const pcdhip_csr* ms[3] = {A, B, C};
  size_t max_nnz = 0;
  for (int k = 0; k < 3; k++) {
    int rc = validate_csr(ms[k], num_cols);
    if (rc) return rc;
    max_nnz = std::max<size_t>(max_nnz, ms[k]->row_ptr[ms[k]->num_rows]);
  }
  if (keep == 0) keep = 7;
  // the two domains: the rules of the header, or the caller's sizes
  Dom dk, db, dh;
  if (domain_k_n) {
    if (split_domain(field_id, domain_k_n, &dk) != PCDHIP_OK || domain_k_n < max_nnz) return PCDHIP_E_ARG;
  } else if (pick_domain(field_id, std::max<size_t>(max_nnz, 1), &dk) != PCDHIP_OK) return PCDHIP_E_SIZE_UNSUPPORTED;
  if (domain_b_n) {
    if (split_domain(field_id, domain_b_n, &db) != PCDHIP_OK || domain_b_n < dk.n) return PCDHIP_E_ARG;
  } else if (3 * (size_t)dk.n >= kMaxLen || pick_domain(field_id, std::max<size_t>(3 * (size_t)dk.n - 3, 1), &db) != PCDHIP_OK) return PCDHIP_E_SIZE_UNSUPPORTED;
  if (pick_domain(field_id, domain_h_n, &dh) != PCDHIP_OK) return PCDHIP_E_ARG;
  BIND();
  return guarded([&]() -> int {
    const FieldEntry& fe = field_entry(field_id);
    const size_t limbs = (size_t)fe.abi_words / 2, eb = (size_t)fe.abi_words * 4, rows = A->num_rows;
    const bool want_b = (keep & 4) != 0;
    // the resident powers of H's generator (none for |H| = 1)
    const FftTables* th = nullptr;
    if (dh.n > 1) {
      int rc = dh.m == 1 ? get_tables(ctx, field_id, dh.a, &th) : get_mixed_tables(ctx, field_id, dh, &th);
      if (rc) return rc;
    }
    pcdhip_marlin_index* h = new pcdhip_marlin_index();
    h->field_id = field_id; h->domain_h_n = domain_h_n; h->domain_x_n = domain_x_n; h->domain_k_n = dk.n; h->domain_b_n = db.n;
    h->max_nnz = max_nnz;
    void* csr_dev = nullptr;
    auto bail = [&](int rc) { if (csr_dev) (void)hipFree(csr_dev); index_release(h); return rc; };
    // the evaluations on K are always made; coefficients and evaluations on B only where they are kept
    const size_t form_n[3] = {dk.n, dk.n, db.n};
    const bool form_on[3] = {(keep & 1) != 0, true, want_b};
    for (int f = 0; f < 3; f++) {
      if (!form_on[f]) continue;
      hipError_t e = hipMalloc(&h->block[f], 12 * form_n[f] * eb);
      if (e != hipSuccess) return bail(fail(ctx, e));
      for (int m = 0; m < 3; m++) for (int q = 0; q < 4; q++) {
        h->vec[f][m][q].field_id = field_id; h->vec[f][m][q].n = form_n[f];
        h->vec[f][m][q].dptr = (uint32_t*)((char*)h->block[f] + (size_t)(4 * m + q) * form_n[f] * eb);
      }
    }
    // the three CSRs in the index's order, one device block: per matrix rp, coeff, col
    OrderedCsr oc[3];
    size_t base[3], total = 0;
    for (int k = 0; k < 3; k++) {
      order_csr(ms[k], limbs, &oc[k]);
      const size_t nnz = ms[k]->row_ptr[rows];
      base[k] = total;
      total += up64((rows + 1) * 8) + up64(nnz * eb) + up64(nnz * 4);
    }
    hipError_t e = hipMalloc(&csr_dev, total + 64);
    if (e != hipSuccess) return bail(fail(ctx, e));
    MarlinIndexIn in;
    for (int k = 0; k < 3 && e == hipSuccess; k++) {
      const size_t nnz = ms[k]->row_ptr[rows];
      char* d = (char*)csr_dev + base[k];
      char* dco = d + up64((rows + 1) * 8);
      char* dcol = dco + up64(nnz * eb);
      e = hipMemcpyAsync(d, ms[k]->row_ptr, (rows + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess && nnz) e = hipMemcpyAsync(dco, oc[k].coeff, nnz * eb, hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess && nnz) e = hipMemcpyAsync(dcol, oc[k].col, nnz * 4, hipMemcpyHostToDevice, ctx->stream);
      in.rp[k] = (const uint64_t*)d; in.coeff[k] = (const uint32_t*)dco; in.col[k] = (const uint32_t*)dcol; in.nnz[k] = (uint32_t)nnz;
      for (int q = 0; q < 4; q++) in.out[k][q] = h->vec[1][k][q].dptr;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's arrays and the sorted copies are done with
    if (e != hipSuccess) return bail(fail(ctx, e));
    in.rows = (uint32_t)rows; in.k_n = dk.n; in.x_n = (uint32_t)domain_x_n; in.period = (uint32_t)(domain_h_n / domain_x_n);
    BuildEvents be;
    e = be.make();
    if (e == hipSuccess) e = hipEventRecord(be.ev[0], ctx->stream);
    if (e == hipSuccess) e = fe.marlin_index_arith(ctx->stream, th ? th->consts : nullptr, th ? th->tw_fwd : nullptr, dh.n / dh.m, in);
    if (e == hipSuccess) e = hipEventRecord(be.ev[1], ctx->stream);
    if (e != hipSuccess) return bail(fail(ctx, e));
    const bool transforms = (keep & 1) || want_b;
    // per vector: evaluations on K -> device image -> inverse transform on K (the coefficients) -> zero tail up to |B| -> forward
    // transform on B; the ABI images of the kept forms are written on the way
    if (transforms) {
      const size_t big = want_b ? db.n : dk.n, vb = big * fe.words * 4;
      e = ctx->aux_ws.ensure(AUX_FFT_X, vb);
      if (e == hipSuccess) e = ctx->aux_ws.ensure(AUX_FFT_TMP, vb);
      if (e != hipSuccess) return bail(fail(ctx, e));
      uint32_t *x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X], *tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
      for (int m = 0; m < 3; m++) for (int q = 0; q < 4; q++) {
        hipEvent_t* const ev = be.ev + 2 + 3 * (4 * m + q);
        e = hipEventRecord(ev[0], ctx->stream);
        if (e == hipSuccess) e = fe.convert(ctx->stream, h->vec[1][m][q].dptr, x, dk.n, 0);
        if (e != hipSuccess) return bail(fail(ctx, e));
        int rc = dk.n > 1 ? domain_transform(ctx, field_id, dk, x, tmp, 1, 0, nullptr, nullptr) : PCDHIP_OK;  // (|K| = 1: a constant)
        if (rc) return bail(rc);
        if (keep & 1) e = fe.convert(ctx->stream, x, h->vec[0][m][q].dptr, dk.n, 1);
        if (e == hipSuccess) e = hipEventRecord(ev[1], ctx->stream);
        if (e != hipSuccess) return bail(fail(ctx, e));
        if (!want_b) continue;
        if (db.n > dk.n) e = hipMemsetAsync(x + (size_t)dk.n * fe.words, 0, (size_t)(db.n - dk.n) * fe.words * 4, ctx->stream);
        if (e != hipSuccess) return bail(fail(ctx, e));
        rc = db.n > 1 ? domain_transform(ctx, field_id, db, x, tmp, 0, 0, nullptr, nullptr) : PCDHIP_OK;
        if (rc) return bail(rc);
        e = fe.convert(ctx->stream, x, h->vec[2][m][q].dptr, db.n, 1);
        if (e == hipSuccess) e = hipEventRecord(ev[2], ctx->stream);
        if (e != hipSuccess) return bail(fail(ctx, e));
      }
    }
    // the CSRs, and the evaluations on K when they were not asked for, go once the device is done with them
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(fail(ctx, e));
    (void)hipEventElapsedTime(&h->ms[0], be.ev[0], be.ev[1]);
    for (int i = 0; i < 12 && transforms; i++) {
      float t = 0;
      if (hipEventElapsedTime(&t, be.ev[2 + 3 * i], be.ev[3 + 3 * i]) == hipSuccess) h->ms[1] += t;
      if (want_b && hipEventElapsedTime(&t, be.ev[3 + 3 * i], be.ev[4 + 3 * i]) == hipSuccess) h->ms[2] += t;
    }
    (void)hipFree(csr_dev);
    if (!(keep & 2)) { (void)hipFree(h->block[1]); h->block[1] = nullptr; }
    *out = h;
    return PCDHIP_OK;
  });
}

void pcdhip_marlin_index_free(pcdhip_ctx* ctx, pcdhip_marlin_index* index) {
  if (!index) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  index_release(index);
}

int pcdhip_marlin_index_info(const pcdhip_marlin_index* index, uint64_t out[4]) {
  if (!index || !out) return PCDHIP_E_ARG;
  const size_t eb = (size_t)field_entry(index->field_id).abi_words * 4;
  out[0] = index->domain_k_n; out[1] = index->domain_b_n; out[2] = index->max_nnz;
  out[3] = 0;
  for (int f = 0; f < 3; f++) if (index->block[f]) out[3] += 12 * (f == 2 ? index->domain_b_n : index->domain_k_n) * eb;
  return PCDHIP_OK;
}

int pcdhip_marlin_index_timings(const pcdhip_marlin_index* index, float out_ms[3]) {
  if (!index || !out_ms) return PCDHIP_E_ARG;
  memcpy(out_ms, index->ms, sizeof index->ms);
  return PCDHIP_OK;
}

int pcdhip_marlin_index_vec(const pcdhip_marlin_index* index, int form, int matrix, int poly, const pcdhip_buf** out) {
  if (!index || !out || form < 0 || form > 2 || matrix < 0 || matrix > 2 || poly < 0 || poly > 3) return PCDHIP_E_ARG;
  if (!index->block[form]) return PCDHIP_E_ARG;
  *out = &index->vec[form][matrix][poly];
  return PCDHIP_OK;
}

int pcdhip_marlin_index_commit(pcdhip_ctx* ctx, const pcdhip_marlin_index* index, const pcdhip_bases* powers_of_g, uint64_t* comm_xy,
                               uint8_t* comm_inf) {
  if (!ctx || !index || !powers_of_g || !comm_xy || !comm_inf || !index->block[0]) return PCDHIP_E_ARG;
  pcdhip_kzg_commit_item items[12];
  memset(items, 0, sizeof items);
  for (int m = 0; m < 3; m++) for (int q = 0; q < 4; q++) {
    items[4 * m + q].poly = &index->vec[0][m][q];
    items[4 * m + q].len = index->domain_k_n;
  }
  return pcdhip_kzg_commit(ctx, powers_of_g, nullptr, nullptr, items, 12, comm_xy, comm_inf, nullptr, nullptr, nullptr);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ K11: round 1 and the first sumcheck
namespace {
// `len` ABI elements of src -> the device image over the domain d with a zero tail -> the forward or inverse transform -> the first
// out_n elements back as ABI words into dst (dst may be src: the vector sits in the workspace in between).  A domain of one element
// has the identity for both transforms.
int transform_abi(pcdhip_ctx* ctx, int field_id, const Dom& d, const uint32_t* src, size_t len, uint32_t* dst, size_t out_n, int inverse) {
  const FieldEntry& fe = field_entry(field_id);
  const size_t vb = (size_t)d.n * fe.words * 4;
  TRY(ctx->aux_ws.ensure(AUX_FFT_X, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  uint32_t* x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X];
  TRY(fe.convert(ctx->stream, src, x, (uint32_t)len, 0));
  if (len < d.n) TRY(hipMemsetAsync(x + len * fe.words, 0, (d.n - len) * fe.words * 4, ctx->stream));
  if (d.n > 1) {
    int rc = domain_transform(ctx, field_id, d, x, (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP], inverse, 0, nullptr, nullptr);
    if (rc) return rc;
  }
  TRY(fe.convert(ctx->stream, x, dst, (uint32_t)out_n, 1));
  return PCDHIP_OK;
}
// M z on H for the forward matrices of a handle: z (num_cols ABI elements) -> the device image, the witness map's mat-vecs without
// their input rows (spmv3 for all three, two spmv when C is not asked for: zero tails up to |H| included), -> out[M] as ABI words
int zm_evals_dev(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const uint32_t* z_abi, uint32_t* const out[3]) {
  const FieldEntry& fe = field_entry(mats->field_id);
  const size_t h_n = mats->domain_h_n, ew = h_n * fe.words;
  TRY(ctx->aux_ws.ensure(AUX_Z, std::max<size_t>(mats->num_cols, 1) * fe.words * 4));
  TRY(ctx->aux_ws.ensure(AUX_A, 3 * ew * 4));
  uint32_t *zd = (uint32_t*)ctx->aux_ws.buf[AUX_Z], *v = (uint32_t*)ctx->aux_ws.buf[AUX_A];
  TRY(fe.convert(ctx->stream, z_abi, zd, (uint32_t)mats->num_cols, 0));
  if (out[2]) TRY(fe.spmv3(ctx->stream, mats->fwd, zd, 0, (uint32_t)h_n, v, ew));
  else for (int k = 0; k < 2; k++) TRY(fe.spmv(ctx->stream, mats->fwd[k], zd, 0, 0, (uint32_t)h_n, v + k * ew));
  for (int k = 0; k < 3; k++) if (out[k]) TRY(fe.convert(ctx->stream, v + k * ew, out[k], (uint32_t)h_n, 1));
  return PCDHIP_OK;
}
// p (len coefficients, room for max(len, n + k)) += blind (X^n - 1); blind: k coefficients on the host, staged at element `at` of
// AUX_MARLIN_BLIND (which the caller has sized: several calls of one driver are queued before the stream is waited for)
int add_vanishing_dev(pcdhip_ctx* ctx, const FieldEntry& fe, uint32_t* p, size_t len, const uint64_t* blind, size_t k, size_t n, size_t at) {
  if (k == 0) return PCDHIP_OK;
  const size_t eb = (size_t)fe.abi_words * 4;
  uint32_t* bd = (uint32_t*)((char*)ctx->aux_ws.buf[AUX_MARLIN_BLIND] + at * eb);
  TRY(hipMemcpyAsync(bd, blind, k * eb, hipMemcpyHostToDevice, ctx->stream));
  if (len < n + k) TRY(hipMemsetAsync((char*)p + len * eb, 0, (n + k - len) * eb, ctx->stream));
  TRY(fe.poly_add_vanishing(ctx->stream, p, bd, k, n));
  return PCDHIP_OK;
}
// p = q (X^n - 1) + r for a SMALL n (round 1 divides |H| + k coefficients by v_X, and |X| is a handful of public inputs): the K8
// kernel gives every lane its whole stride-n column of p, len / n terms, which is a quadratic cost here (2^20 lanes of 2^18 terms).
// Instead the strided suffix sums S_m = sum_{i >= 0} p_(m + i n) by doubling -- S <- S + (S shifted down by n 2^t), log2(len / n)
// passes of one addition per element between two workspace vectors (a pass may not run in place: it reads what another lane
// writes) -- and then q_j = S_(j + n), r_j = S_j.  ws: two vectors of len elements.  Up to kDivDirect terms per lane the K8 kernel
// is the cheaper one and is used as it stands.
const size_t kDivDirect = 64;
int div_vanishing_small_n(pcdhip_ctx* ctx, const FieldEntry& fe, const uint32_t* p, size_t len, size_t n, uint32_t* q, uint32_t* r,
                          uint32_t* ws) {
  if (len <= n * kDivDirect) {
    TRY(fe.poly_div_vanishing(ctx->stream, p, len, n, q, r));
    return PCDHIP_OK;
  }
  const size_t aw = fe.abi_words, eb = aw * 4;
  const uint32_t* cur = p;
  uint32_t* next = ws;
  for (size_t off = n; off < len; off *= 2) {
    TRY(fe.vec_addsub(ctx->stream, cur, cur + off * aw, len - off, 0, next));
    TRY(hipMemcpyAsync(next + (len - off) * aw, cur + (len - off) * aw, off * eb, hipMemcpyDeviceToDevice, ctx->stream));
    cur = next;
    next = next == ws ? ws + len * aw : ws;
  }
  TRY(hipMemcpyAsync(q, cur + n * aw, (len - n) * eb, hipMemcpyDeviceToDevice, ctx->stream));
  TRY(hipMemcpyAsync(r, cur, n * eb, hipMemcpyDeviceToDevice, ctx->stream));
  return PCDHIP_OK;
}
bool same_field(int f, std::initializer_list<const pcdhip_buf*> bufs) {
  for (const pcdhip_buf* b : bufs) if (b && b->field_id != f) return false;
  return true;
}
// no two of the non-null buffers share their memory
bool all_distinct(std::initializer_list<const pcdhip_buf*> bufs) {
  for (auto a = bufs.begin(); a != bufs.end(); ++a)
    for (auto b = a + 1; b != bufs.end(); ++b) if (*a && *b && (*a)->dptr == (*b)->dptr) return false;
  return true;
}
}  // namespace

extern "C" {

int pcdhip_marlin_zm_evals(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const pcdhip_buf* z, pcdhip_buf* za_out, pcdhip_buf* zb_out,
                           pcdhip_buf* zc_out) {
  if (!ctx || !mats || !z || !za_out || !zb_out || !(mats->forms & 2)) return PCDHIP_E_ARG;
  if (!same_field(mats->field_id, {z, za_out, zb_out, zc_out}) || !all_distinct({z, za_out, zb_out, zc_out})) return PCDHIP_E_ARG;
  if (z->n < mats->num_cols || za_out->n < mats->domain_h_n || zb_out->n < mats->domain_h_n || (zc_out && zc_out->n < mats->domain_h_n))
    return PCDHIP_E_ARG;
  BIND();
  uint32_t* const out[3] = {za_out->dptr, zb_out->dptr, zc_out ? zc_out->dptr : nullptr};
  return zm_evals_dev(ctx, mats, z->dptr, out);
}

int pcdhip_marlin_place_assignment(pcdhip_ctx* ctx, int field_id, size_t domain_h_n, size_t domain_x_n, const pcdhip_buf* z, size_t num_cols,
                                   pcdhip_buf* out) {
  if (!ctx || !valid_field(field_id) || !z || !out || !same_field(field_id, {z, out}) || z->dptr == out->dptr) return PCDHIP_E_ARG;
  if (!is_domain_size(field_id, domain_h_n) || !is_domain_size(field_id, domain_x_n) || domain_h_n % domain_x_n != 0) return PCDHIP_E_ARG;
  if (num_cols > z->n || num_cols > domain_h_n || domain_h_n > out->n) return PCDHIP_E_ARG;
  BIND();
  TRY(field_entry(field_id).marlin_place(ctx->stream, z->dptr, num_cols, domain_x_n, domain_h_n, out->dptr));
  return PCDHIP_OK;
}

int pcdhip_poly_add_vanishing_multiple(pcdhip_ctx* ctx, pcdhip_buf* p, size_t len, const uint64_t* blind_mont, size_t k, size_t domain_n,
                                       size_t* out_len) {
  if (!ctx || !p || !out_len || (k && !blind_mont) || domain_n == 0 || domain_n >= kMaxLen || k >= kMaxLen || len > p->n) return PCDHIP_E_ARG;
  const size_t ol = k ? std::max(len, domain_n + k) : len;
  if (ol > p->n) return PCDHIP_E_ARG;
  *out_len = ol;
  if (k == 0) return PCDHIP_OK;
  BIND();
  const FieldEntry& fe = field_entry(p->field_id);
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_BLIND, k * fe.abi_words * 4));
  int rc = add_vanishing_dev(ctx, fe, p->dptr, len, blind_mont, k, domain_n, 0);
  if (rc) return rc;
  TRY(hipStreamSynchronize(ctx->stream));  // blind_mont is the caller's memory
  return PCDHIP_OK;
}

int pcdhip_marlin_sumcheck1_q(pcdhip_ctx* ctx, const uint64_t* eta_mont, const pcdhip_buf* za, const pcdhip_buf* zb, const pcdhip_buf* r_alpha,
                              const pcdhip_buf* t, const pcdhip_buf* z, size_t n, pcdhip_buf* q_out) {
  if (!ctx || !eta_mont || !za || !zb || !r_alpha || !t || !z || !q_out || n >= kMaxLen) return PCDHIP_E_ARG;
  if (!same_field(q_out->field_id, {za, zb, r_alpha, t, z})) return PCDHIP_E_ARG;
  for (const pcdhip_buf* b : {za, zb, r_alpha, t, z, (const pcdhip_buf*)q_out}) if (n > b->n) return PCDHIP_E_ARG;
  if (n == 0) return PCDHIP_OK;
  BIND();
  TRY(field_entry(q_out->field_id).marlin_sumcheck1_q(ctx->stream, (const uint32_t*)eta_mont, za->dptr, zb->dptr, r_alpha->dptr, t->dptr, z->dptr,
                                                       n, q_out->dptr));
  return PCDHIP_OK;
}

int pcdhip_marlin_round1(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const pcdhip_buf* z, const uint64_t* blind_w_mont, size_t k_w,
                         const uint64_t* blind_a_mont, size_t k_a, const uint64_t* blind_b_mont, size_t k_b, pcdhip_buf* x_hat,
                         pcdhip_buf* z_poly, pcdhip_buf* w, pcdhip_buf* w_rem, pcdhip_buf* za_poly, pcdhip_buf* zb_poly, pcdhip_buf* za_evals,
                         pcdhip_buf* zb_evals, size_t out_lens[5]) {
  if (!ctx || !mats || !z || !x_hat || !z_poly || !w_rem || !za_poly || !zb_poly || !out_lens || !(mats->forms & 2)) return PCDHIP_E_ARG;
  if ((k_w && !blind_w_mont) || (k_a && !blind_a_mont) || (k_b && !blind_b_mont) || k_w >= kMaxLen || k_a >= kMaxLen || k_b >= kMaxLen)
    return PCDHIP_E_ARG;
  const int f = mats->field_id;
  const size_t h_n = mats->domain_h_n, x_n = mats->domain_x_n, w_len = h_n + k_w - x_n;
  if (!same_field(f, {z, x_hat, z_poly, w, w_rem, za_poly, zb_poly, za_evals, zb_evals})) return PCDHIP_E_ARG;
  if (!all_distinct({z, x_hat, z_poly, w, w_rem, za_poly, zb_poly, za_evals, zb_evals})) return PCDHIP_E_ARG;
  if (z->n < mats->num_cols || x_hat->n < x_n || z_poly->n < h_n + k_w || w_rem->n < x_n || za_poly->n < h_n + k_a || zb_poly->n < h_n + k_b)
    return PCDHIP_E_ARG;
  if ((w_len && (!w || w->n < w_len)) || (za_evals && za_evals->n < h_n) || (zb_evals && zb_evals->n < h_n)) return PCDHIP_E_ARG;
  Dom dh, dx;
  if (pick_domain(f, h_n, &dh) != PCDHIP_OK || pick_domain(f, x_n, &dx) != PCDHIP_OK) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(f);
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_BLIND, std::max<size_t>(k_w + k_a + k_b, 1) * fe.abi_words * 4));
  // x^: the instance variables (those below num_cols) interpolated on X
  int rc = transform_abi(ctx, f, dx, z->dptr, std::min<size_t>(x_n, mats->num_cols), x_hat->dptr, x_n, 1);
  if (rc) return rc;
  // z_poly: the assignment at pi's places, interpolated on H, blinded
  TRY(fe.marlin_place(ctx->stream, z->dptr, mats->num_cols, x_n, h_n, z_poly->dptr));
  rc = transform_abi(ctx, f, dh, z_poly->dptr, h_n, z_poly->dptr, h_n, 1);
  rc = rc ? rc : add_vanishing_dev(ctx, fe, z_poly->dptr, h_n, blind_w_mont, k_w, h_n, 0);
  if (rc) return rc;
  // w = (z_poly - x^) / v_X: x^ is of degree below |X|, so the quotient is z_poly's and the remainder is z_poly's minus x^
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_WS, 2 * (h_n + k_w) * fe.abi_words * 4));
  rc = div_vanishing_small_n(ctx, fe, z_poly->dptr, h_n + k_w, x_n, w_len ? w->dptr : nullptr, w_rem->dptr, (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_WS]);
  if (rc) return rc;
  TRY(fe.vec_addsub(ctx->stream, w_rem->dptr, x_hat->dptr, x_n, 1, w_rem->dptr));
  // z_A, z_B on H (into the caller's vectors, or into the polynomials' own buffers), interpolated, blinded
  uint32_t* const ev[3] = {za_evals ? za_evals->dptr : za_poly->dptr, zb_evals ? zb_evals->dptr : zb_poly->dptr, nullptr};
  rc = zm_evals_dev(ctx, mats, z->dptr, ev);
  rc = rc ? rc : transform_abi(ctx, f, dh, ev[0], h_n, za_poly->dptr, h_n, 1);
  rc = rc ? rc : add_vanishing_dev(ctx, fe, za_poly->dptr, h_n, blind_a_mont, k_a, h_n, k_w);
  rc = rc ? rc : transform_abi(ctx, f, dh, ev[1], h_n, zb_poly->dptr, h_n, 1);
  rc = rc ? rc : add_vanishing_dev(ctx, fe, zb_poly->dptr, h_n, blind_b_mont, k_b, h_n, k_w + k_a);
  if (rc) return rc;
  out_lens[0] = x_n; out_lens[1] = h_n + k_w; out_lens[2] = w_len; out_lens[3] = h_n + k_a; out_lens[4] = h_n + k_b;
  TRY(hipStreamSynchronize(ctx->stream));  // the blinding coefficients are the caller's memory
  return PCDHIP_OK;
}

int pcdhip_marlin_sumcheck1(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const uint64_t* eta_mont, const uint64_t* alpha_mont,
                            const pcdhip_buf* za_poly, size_t len_za, const pcdhip_buf* zb_poly, size_t len_zb, const pcdhip_buf* z_poly,
                            size_t len_z, const pcdhip_buf* mask, size_t len_mask, size_t domain_d_n, pcdhip_buf* t_poly, pcdhip_buf* h1,
                            pcdhip_buf* g1, pcdhip_buf* sigma, size_t out_lens[3]) {
  if (!ctx || !mats || !eta_mont || !alpha_mont || !za_poly || !zb_poly || !z_poly || !t_poly || !sigma || !out_lens || !(mats->forms & 1))
    return PCDHIP_E_ARG;
  const int f = mats->field_id;
  const size_t h_n = mats->domain_h_n;
  if (!mask) len_mask = 0;
  if (!same_field(f, {za_poly, zb_poly, z_poly, mask, t_poly, h1, g1, sigma})) return PCDHIP_E_ARG;
  if (len_za == 0 || len_zb == 0 || len_z == 0 || len_za > za_poly->n || len_zb > zb_poly->n || len_z > z_poly->n || (mask && len_mask > mask->n))
    return PCDHIP_E_ARG;
  if (len_za >= kMaxLen || len_zb >= kMaxLen || len_z >= kMaxLen || len_mask >= kMaxLen) return PCDHIP_E_ARG;
  // outputs apart from each other and from the inputs (the inputs may coincide among themselves)
  for (const pcdhip_buf* in : {za_poly, zb_poly, z_poly, mask})
    if (!all_distinct({in, (const pcdhip_buf*)t_poly, (const pcdhip_buf*)h1, (const pcdhip_buf*)g1, (const pcdhip_buf*)sigma})) return PCDHIP_E_ARG;
  // the longest product r(alpha, .) z_A z_B decides D; q itself may be longer by t z or the mask
  const size_t prod_len = h_n + len_za + len_zb - 2, q_len = std::max({prod_len, h_n + len_z - 1, len_mask});
  Dom dh, dd;
  if (pick_domain(f, h_n, &dh) != PCDHIP_OK) return PCDHIP_E_ARG;
  if (domain_d_n) {
    int rc = split_domain(f, domain_d_n, &dd);
    if (rc) return rc == PCDHIP_E_ARG ? PCDHIP_E_SIZE_UNSUPPORTED : rc;
    if (domain_d_n < q_len) return PCDHIP_E_ARG;
  } else if (q_len >= kMaxLen || pick_domain(f, prod_len, &dd) != PCDHIP_OK) return PCDHIP_E_SIZE_UNSUPPORTED;
  else if (dd.n < q_len) return PCDHIP_E_ARG;
  const size_t h1_len = q_len - h_n, g1_len = h_n - 1, d_n = dd.n;
  if (t_poly->n < h_n || sigma->n < 1 || (h1_len && (!h1 || h1->n < h1_len)) || (g1_len && (!g1 || g1->n < g1_len))) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(f);
  const size_t eb = (size_t)fe.abi_words * 4;
  // one block: r(alpha, .) on H and then its coefficients | the five vectors on D (the first becomes q) | the remainder mod v_H
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_WS, (2 * h_n + 5 * d_n) * eb));
  uint32_t* const r_h = (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_WS];
  uint32_t* ev[5];
  for (int k = 0; k < 5; k++) ev[k] = r_h + (h_n + k * d_n) * fe.abi_words;
  uint32_t* const rem = ev[4] + d_n * fe.abi_words;
  int rc = lagrange_dev(ctx, f, h_n, alpha_mont, r_h);
  rc = rc ? rc : t_evals_dev(ctx, mats, eta_mont, r_h, t_poly->dptr);
  rc = rc ? rc : transform_abi(ctx, f, dh, r_h, h_n, r_h, h_n, 1);
  rc = rc ? rc : transform_abi(ctx, f, dh, t_poly->dptr, h_n, t_poly->dptr, h_n, 1);
  // za, zb, r(alpha, .), t, z on D
  const uint32_t* const src[5] = {za_poly->dptr, zb_poly->dptr, r_h, t_poly->dptr, z_poly->dptr};
  const size_t src_len[5] = {len_za, len_zb, h_n, h_n, len_z};
  for (int k = 0; k < 5 && !rc; k++) rc = transform_abi(ctx, f, dd, src[k], src_len[k], ev[k], d_n, 0);
  if (rc) return rc;
  TRY(fe.marlin_sumcheck1_q(ctx->stream, (const uint32_t*)eta_mont, ev[0], ev[1], ev[2], ev[3], ev[4], d_n, ev[0]));
  rc = transform_abi(ctx, f, dd, ev[0], d_n, ev[0], d_n, 1);
  if (rc) return rc;
  if (len_mask) TRY(fe.vec_addsub(ctx->stream, ev[0], mask->dptr, len_mask, 0, ev[0]));
  // q = h_1 v_H + (sigma_1 / |H| + X g_1)
  TRY(fe.poly_div_vanishing(ctx->stream, ev[0], q_len, h_n, h1_len ? h1->dptr : nullptr, rem));
  TRY(hipMemcpyAsync(sigma->dptr, rem, eb, hipMemcpyDeviceToDevice, ctx->stream));
  if (g1_len) TRY(hipMemcpyAsync(g1->dptr, rem + fe.abi_words, g1_len * eb, hipMemcpyDeviceToDevice, ctx->stream));
  out_lens[0] = h_n; out_lens[1] = h1_len; out_lens[2] = g1_len;
  return PCDHIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ K12: the second sumcheck
extern "C" {

int pcdhip_marlin_sumcheck2_q(pcdhip_ctx* ctx, const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* coeff_mont,
                              const pcdhip_buf* const row[3], const pcdhip_buf* const col[3], const pcdhip_buf* const row_col[3],
                              const pcdhip_buf* const val[3], const pcdhip_buf* f, size_t n, pcdhip_buf* q_out) {
  if (!ctx || !f || !q_out) return PCDHIP_E_ARG;
  SumcheckArgs a;
  int rc = sumcheck_args(alpha_mont, beta_mont, coeff_mont, row, col, row_col, val, n, &a);
  if (rc) return rc;
  if (f->field_id != a.field_id || q_out->field_id != a.field_id || n > f->n || n > q_out->n || is_input(a, q_out->dptr)) return PCDHIP_E_ARG;
  if (n == 0) return PCDHIP_OK;
  BIND();
  TRY(field_entry(a.field_id).marlin_sumcheck2_q(ctx->stream, (const uint32_t*)alpha_mont, (const uint32_t*)beta_mont, (const uint32_t*)coeff_mont,
                                                 a.row, a.col, a.rc, a.val, f->dptr, n, q_out->dptr));
  return PCDHIP_OK;
}

int pcdhip_marlin_sumcheck2(pcdhip_ctx* ctx, const pcdhip_marlin_index* index, const uint64_t* alpha_mont, const uint64_t* beta_mont,
                            const uint64_t* coeff_mont, int route, pcdhip_buf* f_poly, pcdhip_buf* g2, pcdhip_buf* sigma, pcdhip_buf* h2,
                            pcdhip_buf* h2_rem, size_t out_lens[3]) {
  if (!ctx || !index || !alpha_mont || !beta_mont || !coeff_mont || !sigma || !out_lens || route < 0 || route > 2) return PCDHIP_E_ARG;
  if (!index->block[1] || !index->block[2]) return PCDHIP_E_ARG;
  const int f = index->field_id;
  const size_t k_n = index->domain_k_n, b_n = index->domain_b_n;
  const size_t g2_len = k_n - 1, h2_len = 3 * k_n - 3, q_len = 4 * k_n - 3;
  if (q_len >= kMaxLen) return PCDHIP_E_SIZE_UNSUPPORTED;
  // route 1 multiplies b by f on B, where a - b f (4 |K| - 3 coefficients) must fit; route 2 only interpolates a and b there
  const bool fits1 = b_n >= q_len, fits2 = b_n >= 3 * k_n - 2;
  if (route == 0) route = fits1 ? 1 : 2;
  if ((route == 1 && !fits1) || (route == 2 && !fits2)) return PCDHIP_E_ARG;
  if (!same_field(f, {f_poly, g2, sigma, h2, h2_rem}) || !all_distinct({f_poly, g2, sigma, h2, h2_rem})) return PCDHIP_E_ARG;
  if (sigma->n < 1 || (f_poly && f_poly->n < k_n) || (h2_rem && h2_rem->n < k_n) || (g2_len && (!g2 || g2->n < g2_len)) ||
      (h2_len && (!h2 || h2->n < h2_len)))
    return PCDHIP_E_ARG;
  Dom dk, db, dm;
  if (split_domain(f, k_n, &dk) != PCDHIP_OK || split_domain(f, b_n, &db) != PCDHIP_OK) return PCDHIP_E_ARG;
  if (route == 2 && pick_domain(f, q_len, &dm) != PCDHIP_OK) return PCDHIP_E_SIZE_UNSUPPORTED;
  BIND();
  const FieldEntry& fe = field_entry(f);
  const size_t aw = fe.abi_words, eb = aw * 4;
  const pcdhip_buf *row[2][3], *col[2][3], *rcv[2][3], *val[2][3];  // [0]: on K, [1]: on B
  for (int m = 0; m < 3; m++) for (int on_b = 0; on_b < 2; on_b++) {
    const pcdhip_buf* v = index->vec[1 + on_b][m];
    row[on_b][m] = &v[0]; col[on_b][m] = &v[1]; rcv[on_b][m] = &v[2]; val[on_b][m] = &v[3];
  }
  // one block: f on K and then its coefficients | the remainder | route 1: q on B -- route 2: a on B, b on B; both become coefficients,
  // then a becomes q and b the product b f_poly, so each has room for the 4 |K| - 3 coefficients that a short B does not hold
  const size_t slot_n = std::max(b_n, q_len), big = route == 1 ? slot_n : 2 * slot_n;
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_WS, (2 * k_n + big) * eb));
  uint32_t* const fk = (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_WS];
  uint32_t* const rem_ws = fk + k_n * aw;
  uint32_t* const q = rem_ws + k_n * aw;
  pcdhip_buf fbuf;
  fbuf.field_id = f; fbuf.n = k_n; fbuf.dptr = f_poly ? f_poly->dptr : fk;
  uint32_t* const rem = h2_rem ? h2_rem->dptr : rem_ws;
  // f on K, interpolated; f_poly = sigma + X g_2
  int rc = pcdhip_marlin_sumcheck_f(ctx, alpha_mont, beta_mont, coeff_mont, row[0], col[0], rcv[0], val[0], k_n, &fbuf);
  rc = rc ? rc : transform_abi(ctx, f, dk, fbuf.dptr, k_n, fbuf.dptr, k_n, 1);
  if (rc) return rc;
  TRY(hipMemcpyAsync(sigma->dptr, fbuf.dptr, eb, hipMemcpyDeviceToDevice, ctx->stream));
  if (g2_len) TRY(hipMemcpyAsync(g2->dptr, fbuf.dptr + aw, g2_len * eb, hipMemcpyDeviceToDevice, ctx->stream));
  if (route == 1) {
    // f on B, q = a - b f there in place, back to coefficients
    rc = transform_abi(ctx, f, db, fbuf.dptr, k_n, q, b_n, 0);
    if (rc) return rc;
    const uint32_t* in[4][3];
    for (int m = 0; m < 3; m++) { in[0][m] = row[1][m]->dptr; in[1][m] = col[1][m]->dptr; in[2][m] = rcv[1][m]->dptr; in[3][m] = val[1][m]->dptr; }
    TRY(fe.marlin_sumcheck2_q(ctx->stream, (const uint32_t*)alpha_mont, (const uint32_t*)beta_mont, (const uint32_t*)coeff_mont, in[0], in[1], in[2],
                              in[3], q, b_n, q));
    rc = transform_abi(ctx, f, db, q, b_n, q, q_len, 1);
    if (rc) return rc;
  } else {
    // upstream's order: a and b on B to coefficients (3 |K| - 2 each), b f_poly as a polynomial product over the domain of
    // 4 |K| - 3 elements or more (pcdhip_poly_mul's steps, without its wait), a - b f_poly
    uint32_t* const bq = q + slot_n * aw;
    pcdhip_buf abuf, bbuf;
    abuf.field_id = bbuf.field_id = f; abuf.n = bbuf.n = b_n; abuf.dptr = q; bbuf.dptr = bq;
    rc = pcdhip_marlin_sumcheck_ab(ctx, alpha_mont, beta_mont, coeff_mont, row[1], col[1], rcv[1], val[1], b_n, &abuf, &bbuf);
    rc = rc ? rc : transform_abi(ctx, f, db, q, b_n, q, b_n, 1);
    rc = rc ? rc : transform_abi(ctx, f, db, bq, b_n, bq, b_n, 1);
    if (rc) return rc;
    const size_t ab_len = 3 * k_n - 2, vb = (size_t)dm.n * fe.words * 4;
    TRY(ctx->aux_ws.ensure(AUX_FFT_X, vb));
    TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
    TRY(ctx->aux_ws.ensure(AUX_MARLIN_MUL_B, vb));
    uint32_t *x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X], *y = (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_MUL_B], *tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
    const uint32_t* const src[2] = {bq, fbuf.dptr};
    const size_t src_len[2] = {ab_len, k_n};
    uint32_t* const dst[2] = {x, y};
    for (int k = 0; k < 2; k++) {
      TRY(fe.convert(ctx->stream, src[k], dst[k], (uint32_t)src_len[k], 0));
      TRY(hipMemsetAsync(dst[k] + src_len[k] * fe.words, 0, (dm.n - src_len[k]) * fe.words * 4, ctx->stream));
      rc = domain_transform(ctx, f, dm, dst[k], tmp, 0, 0, nullptr, nullptr);
      if (rc) return rc;
    }
    TRY(fe.vec_mul(ctx->stream, x, y, dm.n, x, 0));
    rc = domain_transform(ctx, f, dm, x, tmp, 1, 0, nullptr, nullptr);
    if (rc) return rc;
    TRY(fe.convert(ctx->stream, x, bq, (uint32_t)q_len, 1));
    // a has 3 |K| - 2 coefficients, the product 4 |K| - 3: q = -(b f) beyond a's length
    TRY(hipMemsetAsync(q + ab_len * aw, 0, (q_len - ab_len) * eb, ctx->stream));
    TRY(fe.vec_addsub(ctx->stream, q, bq, q_len, 1, q));
  }
  // q = h_2 v_K + remainder
  if (h2_len) TRY(fe.poly_div_vanishing(ctx->stream, q, q_len, k_n, h2->dptr, rem));
  else TRY(hipMemcpyAsync(rem, q, eb, hipMemcpyDeviceToDevice, ctx->stream));  // (|K| = 1: q is one coefficient, all of it remainder)
  out_lens[0] = g2_len; out_lens[1] = h2_len; out_lens[2] = (size_t)route;
  return PCDHIP_OK;
}

}  // extern "C"
