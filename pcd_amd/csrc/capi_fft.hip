// Evaluation domains, the resident transform tables, and the FFT entry points of libpcdhip.so.
#include "capi_internal.h"

using namespace pcd;

namespace {
const uint32_t kSmallSubgroupBase[4] = {7, 0, 5, 0};  // ark-ff SMALL_SUBGROUP_BASE (adicity 2) of the two help fields

}  // namespace

namespace pcd {
int split_domain(int field_id, size_t n, Dom* d) {  // n = m * 2^a with m in {1, q, q^2}?
  if (n == 0 || n >= (1ull << 31)) return PCDHIP_E_ARG;
  const uint32_t q = kSmallSubgroupBase[field_id];
  uint32_t m = 1;
  size_t r = n;
  for (int b = 0; b < 2 && q && r % q == 0; b++) { r /= q; m *= q; }
  if (r & (r - 1)) return PCDHIP_E_SIZE_UNSUPPORTED;
  int a = 0;
  while (((size_t)1 << a) < r) a++;
  if (a > field_entry(field_id).two_adicity) return PCDHIP_E_SIZE_UNSUPPORTED;
  d->n = (uint32_t)n; d->m = m; d->a = a;
  return PCDHIP_OK;
}
int pick_domain(int field_id, size_t min_size, Dom* d) {
  const FieldEntry& fe = field_entry(field_id);
  int log_n = 0;
  while (((size_t)1 << log_n) < min_size) log_n++;
  if (log_n <= fe.two_adicity) { d->n = 1u << log_n; d->m = 1; d->a = log_n; return PCDHIP_OK; }
  const uint32_t q = kSmallSubgroupBase[field_id];
  if (!q) return PCDHIP_E_SIZE_UNSUPPORTED;
  size_t best = 0;
  for (int b = 0; b <= 2; b++) {
    size_t r = 1;
    for (int i = 0; i < b; i++) r *= q;
    const size_t mm = r;
    int aa = 0;
    while (r < min_size) { r *= 2; aa++; }
    if (aa <= fe.two_adicity && r < (1ull << 31) && (best == 0 || r < best)) { best = r; d->n = (uint32_t)r; d->m = (uint32_t)mm; d->a = aa; }
  }
  return best ? PCDHIP_OK : PCDHIP_E_SIZE_UNSUPPORTED;
}

int get_tables(pcdhip_ctx* ctx, int field_id, int log_n, const FftTables** out) {
  uint64_t key = ((uint64_t)field_id << 32) | (uint32_t)log_n;
  auto it = ctx->fft_tables.find(key);
  if (it == ctx->fft_tables.end()) {
    FftTables t;
    TRY(field_entry(field_id).fft_make_tables(ctx->stream, log_n, &t));
    try { it = ctx->fft_tables.emplace(key, t).first; } catch (...) { return PCDHIP_E_OOM; }
  }
  *out = &it->second;
  return PCDHIP_OK;
}
int get_mixed_tables(pcdhip_ctx* ctx, int field_id, const Dom& d, const FftTables** out) {
  uint64_t key = (1ull << 63) | ((uint64_t)field_id << 32) | d.n;
  auto it = ctx->fft_tables.find(key);
  if (it == ctx->fft_tables.end()) {
    FftTables t;
    TRY(field_entry(field_id).mixed_make_tables(ctx->stream, d.n, d.m, &t));
    try { it = ctx->fft_tables.emplace(key, t).first; } catch (...) { return PCDHIP_E_OOM; }
  }
  *out = &it->second;
  return PCDHIP_OK;
}
// v (d.n elements, device image) transformed in place
int domain_transform(pcdhip_ctx* ctx, int field_id, const Dom& d, uint32_t* v, uint32_t* tmp, int inverse, int coset, float* pass_ms,
                     int* npasses) {
  const FieldEntry& fe = field_entry(field_id);
  const FftTables* t2;
  int rc = get_tables(ctx, field_id, d.a, &t2);
  if (rc) return rc;
  if (d.m == 1) { TRY(fe.fft_run(ctx->stream, *t2, v, tmp, d.a, inverse, coset, pass_ms, npasses)); return PCDHIP_OK; }
  const FftTables* t;
  rc = get_mixed_tables(ctx, field_id, d, &t);
  if (rc) return rc;
  TRY(fe.mixed_run(ctx->stream, *t, *t2, v, tmp, d.m, d.a, inverse, coset));
  if (npasses) *npasses = 0;
  return PCDHIP_OK;
}
}  // namespace pcd

extern "C" {

static int fft_dev_general(pcdhip_ctx* ctx, pcdhip_buf* data, const Dom& d, int inverse, int coset) {
  inverse = inverse ? 1 : 0;  // (the higher bits of this argument are internal flags of the pass driver: never from the ABI)
  coset = coset ? 1 : 0;
  const FieldEntry& fe = field_entry(data->field_id);
  if (data->n < d.n) return PCDHIP_E_ARG;
  const size_t vb = (size_t)d.n * fe.words * 4;
  TRY(ctx->aux_ws.ensure(AUX_FFT_X, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  uint32_t* x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X];
  // C-ABI image -> device image, transform, and back (the witness-map pipeline keeps vectors in the device image
  // between its seven transforms and pays neither conversion)
  TRY(fe.convert(ctx->stream, data->dptr, x, d.n, 0));
  int rc = domain_transform(ctx, data->field_id, d, x, (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP], inverse, coset, ctx->fft_ms, &ctx->fft_passes);
  if (rc) return rc;
  TRY(fe.convert(ctx->stream, x, data->dptr, d.n, 1));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
int pcdhip_fft_dev(pcdhip_ctx* ctx, pcdhip_buf* data, uint32_t log_n, int inverse, int coset) {
  if (!ctx || !data || log_n > 30) return PCDHIP_E_ARG;
  if ((int)log_n > field_entry(data->field_id).two_adicity) return PCDHIP_E_SIZE_UNSUPPORTED;
  BIND();
  Dom d = {1u << log_n, 1, (int)log_n};
  return fft_dev_general(ctx, data, d, inverse, coset);
}
static int fft_host_general(pcdhip_ctx* ctx, int field_id, uint64_t* data, const Dom& d, int inverse, int coset) {
  const FieldEntry& fe = field_entry(field_id);
  const size_t bytes = (size_t)d.n * fe.abi_words * 4;
  TRY(ctx->aux_ws.ensure(AUX_SCAL, bytes));
  pcdhip_buf tmp;
  tmp.field_id = field_id; tmp.n = d.n; tmp.dptr = (uint32_t*)ctx->aux_ws.buf[AUX_SCAL];
  TRY(hipMemcpyAsync(tmp.dptr, data, bytes, hipMemcpyHostToDevice, ctx->stream));
  int rc = fft_dev_general(ctx, &tmp, d, inverse, coset);
  if (rc) return rc;
  TRY(hipMemcpyAsync(data, tmp.dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
int pcdhip_fft(pcdhip_ctx* ctx, int field_id, uint64_t* data, uint32_t log_n, int inverse, int coset) {
  if (!ctx || !data || !valid_field(field_id) || log_n > 30) return PCDHIP_E_ARG;
  if ((int)log_n > field_entry(field_id).two_adicity) return PCDHIP_E_SIZE_UNSUPPORTED;
  BIND();
  Dom d = {1u << log_n, 1, (int)log_n};
  return fft_host_general(ctx, field_id, data, d, inverse, coset);
}
int pcdhip_fft_general_dev(pcdhip_ctx* ctx, pcdhip_buf* data, size_t n, int inverse, int coset) {
  if (!ctx || !data) return PCDHIP_E_ARG;
  Dom d;
  int rc = split_domain(data->field_id, n, &d);
  if (rc) return rc;
  BIND();
  return fft_dev_general(ctx, data, d, inverse, coset);
}
// p (len coefficients, ABI words) -> its device image in AUX_FFT_X with a zero tail up to the domain, the forward transform, -> out
int pcdhip_poly_evals_on_domain(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, size_t domain_n, int coset, pcdhip_buf* out) {
  if (!ctx || !p || !out || p->field_id != out->field_id || len > p->n) return PCDHIP_E_ARG;
  Dom d;
  int rc = split_domain(p->field_id, domain_n, &d);
  if (rc) return rc == PCDHIP_E_ARG ? PCDHIP_E_SIZE_UNSUPPORTED : rc;
  if (len > domain_n || domain_n > out->n) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(p->field_id);
  const size_t vb = (size_t)d.n * fe.words * 4;
  TRY(ctx->aux_ws.ensure(AUX_FFT_X, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  uint32_t* x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X];
  TRY(fe.convert(ctx->stream, p->dptr, x, (uint32_t)len, 0));
  if (len < d.n) TRY(hipMemsetAsync(x + len * fe.words, 0, (d.n - len) * fe.words * 4, ctx->stream));  // (the device image of 0 is all zero words)
  // (the domain of one element: its only point is 1, or the coset's g, and the polynomial is the constant p_0)
  if (d.n > 1) rc = domain_transform(ctx, p->field_id, d, x, (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP], 0, coset ? 1 : 0, nullptr, nullptr);
  if (rc) return rc;
  TRY(fe.convert(ctx->stream, x, out->dptr, d.n, 1));
  return PCDHIP_OK;
}
int pcdhip_fft_general(pcdhip_ctx* ctx, int field_id, uint64_t* data, size_t n, int inverse, int coset) {
  if (!ctx || !data || !valid_field(field_id)) return PCDHIP_E_ARG;
  Dom d;
  int rc = split_domain(field_id, n, &d);
  if (rc) return rc;
  BIND();
  return fft_host_general(ctx, field_id, data, d, inverse, coset);
}
// Several transforms of ONE host vector with one trip over PCIe (round 5): pcdhip_fft moves the vector both ways per
// transform (2^20 elements over the 298-bit field: 42 MB each way for 0.3 ms of passes), and what ark-poly's callers do with a polynomial
// is usually a chain -- Marlin's `ifft` of evaluations followed by `coset_fft` on a larger domain, the witness map's `ifft; coset_fft` --
// that seam S2 (rust/src/s2.rs) can hand over whole.  ops[i]: bit 0 inverse, bit 1 coset; all on the domain of n = 2^a q^b elements.
int pcdhip_fft_seq(pcdhip_ctx* ctx, int field_id, uint64_t* data, size_t n, const int* ops, int n_ops) {
  if (!ctx || !data || !valid_field(field_id) || !ops || n_ops < 1 || n_ops > 64) return PCDHIP_E_ARG;
  for (int i = 0; i < n_ops; i++) if (ops[i] < 0 || ops[i] > 3) return PCDHIP_E_ARG;
  Dom d;
  int rc = split_domain(field_id, n, &d);
  if (rc) return rc;
  BIND();
  const FieldEntry& fe = field_entry(field_id);
  const size_t bytes = (size_t)d.n * fe.abi_words * 4, vb = (size_t)d.n * fe.words * 4;
  TRY(ctx->aux_ws.ensure(AUX_SCAL, bytes));
  TRY(ctx->aux_ws.ensure(AUX_FFT_X, vb));
  TRY(ctx->aux_ws.ensure(AUX_FFT_TMP, vb));
  uint32_t* abi = (uint32_t*)ctx->aux_ws.buf[AUX_SCAL];
  uint32_t* x = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X];
  TRY(hipMemcpyAsync(abi, data, bytes, hipMemcpyHostToDevice, ctx->stream));
  TRY(fe.convert(ctx->stream, abi, x, d.n, 0));
  for (int i = 0; i < n_ops; i++) {  // (the vector stays in the device image between the transforms: neither conversion in between)
    rc = domain_transform(ctx, field_id, d, x, (uint32_t*)ctx->aux_ws.buf[AUX_FFT_TMP], ops[i] & 1, (ops[i] >> 1) & 1, ctx->fft_ms, &ctx->fft_passes);
    if (rc) return rc;
  }
  TRY(fe.convert(ctx->stream, x, abi, d.n, 1));
  TRY(hipMemcpyAsync(data, abi, bytes, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
size_t pcdhip_domain_size(int field_id, size_t min_size) {
  if (!valid_field(field_id) || min_size == 0) return 0;
  Dom d;
  return pick_domain(field_id, min_size, &d) == PCDHIP_OK ? d.n : 0;
}
int pcdhip_fft_last_timings(pcdhip_ctx* ctx, float out_ms[8]) {
  if (!ctx || !out_ms) return PCDHIP_E_ARG;
  memcpy(out_ms, ctx->fft_ms, sizeof ctx->fft_ms);
  return ctx->fft_passes;
}

}  // extern "C"
