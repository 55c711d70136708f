// ------------------------------------------------------------------------------------------------ K9: Marlin's AHP rounds 2 and 3
// (marlin.hip.h and the t(X) kernels of inst_field.hip: r(alpha, .) on H, the transposed mat-vec behind t(X), the rational sumcheck).
// Every call queues its launches on the context's stream and returns: nothing here waits for the device except the upload of the matrices.
// K10, the index on device (the arithmetisation onto K, the coefficients, the evaluations on B, the twelve commitments), follows below;
// pcdhip_marlin_index_build waits for its own uploads and for the end of its work.
#include <stdlib.h>

#include "capi_internal.h"

using namespace pcd;

namespace {
enum { AUX_MARLIN_PART = AUX_FB_OUT + 5, AUX_MARLIN_A, AUX_MARLIN_B };
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
}  // namespace

extern "C" {

int pcdhip_domain_bivariate_lagrange(pcdhip_ctx* ctx, int field_id, size_t domain_n, const uint64_t* x_mont, pcdhip_buf* out) {
  if (!ctx || !valid_field(field_id) || !x_mont || !out || out->field_id != field_id) return PCDHIP_E_ARG;
  if (!is_domain_size(field_id, domain_n)) return PCDHIP_E_SIZE_UNSUPPORTED;
  if (domain_n > out->n) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(field_id);
  if (domain_n == 1) {
    TRY(fe.marlin_lagrange(ctx->stream, nullptr, nullptr, 1, (const uint32_t*)x_mont, 1, out->dptr));
    return PCDHIP_OK;
  }
  Dom d;
  int rc = pick_domain(field_id, domain_n, &d);
  if (rc) return rc;
  const FftTables* t;
  rc = d.m == 1 ? get_tables(ctx, field_id, d.a, &t) : get_mixed_tables(ctx, field_id, d, &t);
  if (rc) return rc;
  TRY(fe.marlin_lagrange(ctx->stream, t->consts, t->tw_fwd, d.n / d.m, (const uint32_t*)x_mont, d.n, out->dptr));
  return PCDHIP_OK;
}

int pcdhip_marlin_mats_upload(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                              size_t domain_h_n, size_t domain_x_n, pcdhip_marlin_mats** out) {
  if (!ctx || !valid_field(field_id) || !A || !B || !C || !out) return PCDHIP_E_ARG;
  if (!is_domain_size(field_id, domain_h_n) || !is_domain_size(field_id, domain_x_n) || domain_h_n % domain_x_n != 0) return PCDHIP_E_ARG;
  if (A->num_rows != B->num_rows || A->num_rows != C->num_rows || A->num_rows > domain_h_n || num_cols > domain_h_n) return PCDHIP_E_ARG;
  const pcdhip_csr* ms[3] = {A, B, C};
  for (int k = 0; k < 3; k++) { int rc = validate_csr(ms[k], num_cols); if (rc) return rc; }
  BIND();
  return guarded([&]() -> int {
    const FieldEntry& fe = field_entry(field_id);
    const size_t limbs = (size_t)fe.abi_words / 2, period = domain_h_n / domain_x_n, rows = A->num_rows;
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
    pcdhip_marlin_mats* h = new pcdhip_marlin_mats();
    h->field_id = field_id; h->domain_h_n = domain_h_n; h->domain_x_n = domain_x_n; h->num_rows = rows; h->num_cols = num_cols;
    h->seg_len = seg_len;
    hipError_t e = hipMalloc(&h->dev, total + 64);
    if (e != hipSuccess) { delete h; return fail(ctx, e); }
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
    if (rc) { (void)hipFree(h->dev); delete h; return rc; }
    h->view.rows = (uint32_t)domain_h_n;
    h->view.segs = (const MarlinSeg*)(d + seg_off); h->view.n_segs = (uint32_t)segs.size();
    h->view.long_out = (const uint32_t*)(d + lo_off); h->view.long_seg_lo = (const uint32_t*)(d + sl_off);
    h->view.n_long_out = (uint32_t)long_out.size();
    *out = h;
    return PCDHIP_OK;
  });
}

void pcdhip_marlin_mats_free(pcdhip_ctx* ctx, pcdhip_marlin_mats* mats) {
  if (!mats) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  if (mats->dev) (void)hipFree(mats->dev);
  delete mats;
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
  if (r_alpha->n < mats->num_rows || t_out->n < mats->domain_h_n) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(mats->field_id);
  TRY(ctx->aux_ws.ensure(AUX_MARLIN_PART, std::max<size_t>(mats->view.n_segs, 1) * fe.words * 4));
  TRY(fe.marlin_t_evals(ctx->stream, mats->view, (const uint32_t*)eta_mont, r_alpha->dptr, (uint32_t*)ctx->aux_ws.buf[AUX_MARLIN_PART],
                        t_out->dptr, nullptr));
  return PCDHIP_OK;
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
