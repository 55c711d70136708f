// ------------------------------------------------------------------------------------------------ K8: vector algebra for Marlin's AHP rounds
// (poly.hip.h: batch inversion, pointwise product, division by X^n - 1; the polynomial product over the transforms of capi_fft.hip)
#include "capi_internal.h"

using namespace pcd;

namespace {
// the polynomial product's second operand over the domain (device image); its first sits in AUX_FFT_X, the passes' partner in AUX_FFT_TMP
enum { AUX_POLY_MUL_B = AUX_FB_OUT + 4 };
const size_t kMaxLen = (size_t)1 << 31;

// `len` ABI coefficients of src into the device-image vector v of d.n elements, zeros behind them
int pad_in(pcdhip_ctx* ctx, const FieldEntry& fe, const uint32_t* src, size_t len, uint32_t* v, size_t n) {
  TRY(fe.convert(ctx->stream, src, v, (uint32_t)len, 0));
  TRY(hipMemsetAsync(v + len * fe.words, 0, (n - len) * fe.words * 4, ctx->stream));
  return PCDHIP_OK;
}
}  // namespace

extern "C" {

int pcdhip_vec_mul(pcdhip_ctx* ctx, const pcdhip_buf* a, const pcdhip_buf* b, size_t n, pcdhip_buf* out) {
  if (!ctx || !a || !b || !out) return PCDHIP_E_ARG;
  if (a->field_id != b->field_id || a->field_id != out->field_id || n > a->n || n > b->n || n > out->n || n >= kMaxLen) return PCDHIP_E_ARG;
  if (n == 0) return PCDHIP_OK;
  BIND();
  TRY(field_entry(a->field_id).vec_mul(ctx->stream, a->dptr, b->dptr, n, out->dptr, 1));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}

int pcdhip_vec_batch_inverse(pcdhip_ctx* ctx, const pcdhip_buf* in, size_t n, const uint64_t* scale_mont, pcdhip_buf* out) {
  if (!ctx || !in || !out) return PCDHIP_E_ARG;
  if (in->field_id != out->field_id || n > in->n || n > out->n || n >= kMaxLen) return PCDHIP_E_ARG;
  if (n == 0) return PCDHIP_OK;
  BIND();
  TRY(field_entry(in->field_id).vec_batch_inverse(ctx->stream, in->dptr, n, (const uint32_t*)scale_mont, out->dptr));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}

int pcdhip_poly_div_vanishing(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, size_t domain_n, pcdhip_buf* q, size_t* q_len, pcdhip_buf* r,
                              size_t* r_len) {
  if (!ctx || !p || !q_len || domain_n == 0 || len > p->n || len >= kMaxLen) return PCDHIP_E_ARG;
  const size_t ql = len > domain_n ? len - domain_n : 0, rl = std::min(len, domain_n);
  if (ql && !q) return PCDHIP_E_ARG;
  if (q && (q->field_id != p->field_id || q->n < ql || q->dptr == p->dptr)) return PCDHIP_E_ARG;
  if (r && (r->field_id != p->field_id || r->n < rl || r->dptr == p->dptr || (q && r->dptr == q->dptr))) return PCDHIP_E_ARG;
  *q_len = ql;
  if (r_len) *r_len = rl;
  if (len == 0) return PCDHIP_OK;
  BIND();
  TRY(field_entry(p->field_id).poly_div_vanishing(ctx->stream, p->dptr, len, domain_n, q ? q->dptr : nullptr, r ? r->dptr : nullptr));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}

int pcdhip_poly_mul(pcdhip_ctx* ctx, const pcdhip_buf* a, size_t la, const pcdhip_buf* b, size_t lb, pcdhip_buf* out, size_t* out_len) {
  if (!ctx || !a || !b || !out || !out_len) return PCDHIP_E_ARG;
  if (a->field_id != b->field_id || a->field_id != out->field_id || la > a->n || lb > b->n || la >= kMaxLen || lb >= kMaxLen) return PCDHIP_E_ARG;
  const size_t ol = la && lb ? la + lb - 1 : 0;
  if (ol > out->n) return PCDHIP_E_ARG;
  if (ol == 0) { *out_len = 0; return PCDHIP_OK; }
  Dom d;
  if (ol >= kMaxLen || pick_domain(a->field_id, ol, &d) != PCDHIP_OK) return PCDHIP_E_SIZE_UNSUPPORTED;
  *out_len = ol;
  BIND();
  const int f = a->field_id;
  const FieldEntry& fe = field_entry(f);
  const size_t vb = (size_t)d.n * fe.words * 4;
  TRY(ctx->aux_ws.ensure(AUX_FFT_X, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  TRY(ctx->aux_ws.ensure(AUX_POLY_MUL_B, vb));
  uint32_t *x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X], *y = (uint32_t*)ctx->aux_ws.buf[AUX_POLY_MUL_B], *tmp = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP];
  int rc = pad_in(ctx, fe, a->dptr, la, x, d.n);
  rc = rc ? rc : pad_in(ctx, fe, b->dptr, lb, y, d.n);  // (both operands are in the workspace from here on: out may be a or b)
  rc = rc ? rc : domain_transform(ctx, f, d, x, tmp, 0, 0, nullptr, nullptr);
  rc = rc ? rc : domain_transform(ctx, f, d, y, tmp, 0, 0, nullptr, nullptr);
  if (rc) return rc;
  TRY(fe.vec_mul(ctx->stream, x, y, d.n, x, 0));
  rc = domain_transform(ctx, f, d, x, tmp, 1, 0, nullptr, nullptr);
  if (rc) return rc;
  TRY(fe.convert(ctx->stream, x, out->dptr, (uint32_t)ol, 1));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}

}  // extern "C"
