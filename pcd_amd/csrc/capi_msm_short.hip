// Short MSMs without buckets at the C ABI (msm_short.hip.h through GroupEntry::msm_short): host and device scalars, the batched form
// (k MSMs over one handle as one launch chain, GroupEntry::msm_short_batch), and the opt-in routing of the KZG open side's small MSMs.
#include "capi_internal.h"
#include "msm_short.hip.h"

using namespace pcd;

namespace {
enum { SHORT_SCAL = 0, SHORT_SCRATCH, SHORT_OUT, SHORT_BATCH };  // slots of pcdhip_ctx::short_ws (SHORT_BATCH: error words | table | rows)
constexpr size_t MSM_SHORT_BATCH_MAX_K = 1024;  // MSMs per public call (PCDHIP_E_SIZE_UNSUPPORTED beyond)

// what both public batch entry points share behind their argument checks: scal_dev holds the call's scalars, items[j].scalar_offset
// counts elements of it.  One chain, one conversion, one copy back, one wait.
int msm_short_batch_common(pcdhip_ctx* ctx, const pcdhip_bases* bases, const uint32_t* scal_dev, const pcdhip_msm_short_item* items, size_t k,
                           uint64_t* out_xyz) {
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const size_t jw = (size_t)ge.point_words / 2 * 3, jac_b = jw * 4, jac_abi_b = (size_t)ge.point_abi_words / 2 * 3 * 4;
  const size_t sw = (size_t)ge.scalar_words;
  std::vector<MsmShortBatchIn> in(k);
  bool live = false;
  for (size_t j = 0; j < k; j++) {
    in[j] = {scal_dev + (size_t)items[j].scalar_offset * sw, (uint32_t)items[j].base_offset, (uint32_t)items[j].n, (uint32_t)j};
    live |= items[j].n != 0;
  }
  if (!live) {  // identities only, as pcdhip_msm_short writes them (Z = 0): no launch
    for (size_t j = 0; j < k; j++) ge.identity_abi((uint32_t*)out_xyz + j * (jac_abi_b / 4));
    return PCDHIP_OK;
  }
  MsmWorkspace& ws = ctx->short_ws;
  const size_t abi_off = (k * jac_b + 255) & ~(size_t)255;
  TRY(ws.ensure(SHORT_OUT, abi_off + k * jac_abi_b));
  uint32_t* out_dev = (uint32_t*)ws.buf[SHORT_OUT];
  uint32_t* out_abi = out_dev + abi_off / 4;
  TRY(hipMemsetAsync(out_dev, 0, k * jac_b, ctx->stream));  // the slots of items with n == 0: the identity, which the chain does not write
  const uint32_t* err_dev = nullptr;
  int rc = msm_short_batch_async(ctx, bases, in.data(), k, out_dev, jw, &err_dev);
  if (rc) return rc;
  TRY(ge.jac_out(ctx->stream, out_dev, (uint32_t)k, out_abi));
  TRY(hipMemcpyAsync(out_xyz, out_abi, k * jac_abi_b, hipMemcpyDeviceToHost, ctx->stream));
  uint32_t too_wide = 0;  // a scalar of any item that is not a reduced canonical value
  TRY(hipMemcpyAsync(&too_wide, err_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return too_wide ? PCDHIP_E_ARG : PCDHIP_OK;
}
// the checks on the items that need no handle of scalars: sizes first, then ranges
int msm_short_batch_check(const pcdhip_bases* bases, size_t scalars_n, const pcdhip_msm_short_item* items, size_t k) {
  for (size_t j = 0; j < k; j++)
    if (items[j].n > MSM_SHORT_MAX_N) return PCDHIP_E_SIZE_UNSUPPORTED;
  for (size_t j = 0; j < k; j++) {
    const pcdhip_msm_short_item& it = items[j];
    if (it.base_offset > bases->n || it.n > bases->n - it.base_offset || it.scalar_offset > scalars_n || it.n > scalars_n - it.scalar_offset)
      return PCDHIP_E_ARG;
  }
  return PCDHIP_OK;
}
}

namespace pcd {
// scalars_dev: n canonical scalars on the device, ordered on the context's stream.  Sharded handles and ranges beyond the vector are
// refused here as well, whatever the caller has checked.
int msm_short_common(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint32_t* scalars_dev, size_t n, uint64_t* out_xyz) {
  if (!bases->shards.empty() || offset > bases->n || n > bases->n - offset) return PCDHIP_E_ARG;  // (a sharded parent holds no points itself)
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  if (n == 0) { ge.identity_abi((uint32_t*)out_xyz); return PCDHIP_OK; }
  if (n > MSM_SHORT_MAX_N) return PCDHIP_E_SIZE_UNSUPPORTED;
  const size_t jac_b = (size_t)ge.point_words / 2 * 3 * 4, jac_abi_b = (size_t)ge.point_abi_words / 2 * 3 * 4;
  const MsmBasesView bv = bases->view(offset);
  MsmWorkspace& ws = ctx->short_ws;
  TRY(ws.ensure(SHORT_SCRATCH, ge.msm_short_scratch_words(bv, (uint32_t)n) * 4));
  TRY(ws.ensure(SHORT_OUT, jac_b + jac_abi_b + 64));
  uint32_t* scratch = (uint32_t*)ws.buf[SHORT_SCRATCH];
  uint32_t* out_dev = (uint32_t*)ws.buf[SHORT_OUT];
  uint32_t* out_abi = out_dev + jac_b / 4;
  TRY(ge.msm_short(ctx->stream, bv, scalars_dev, (uint32_t)n, scratch, out_dev));
  TRY(ge.jac_out(ctx->stream, out_dev, 1, out_abi));
  TRY(hipMemcpyAsync(out_xyz, out_abi, jac_abi_b, hipMemcpyDeviceToHost, ctx->stream));
  uint32_t too_wide = 0;  // a scalar that is not a reduced canonical value (the rule of pcdhip_msm)
  TRY(hipMemcpyAsync(&too_wide, scratch, 4, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return too_wide ? PCDHIP_E_ARG : PCDHIP_OK;
}
int msm_short_async(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint32_t* scalars_dev, size_t n, uint32_t* out_dev) {
  if (!bases->shards.empty() || offset > bases->n || n > bases->n - offset || n == 0) return PCDHIP_E_ARG;
  if (n > MSM_SHORT_MAX_N) return PCDHIP_E_SIZE_UNSUPPORTED;
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const MsmBasesView bv = bases->view(offset);
  TRY(ctx->short_ws.ensure(SHORT_SCRATCH, ge.msm_short_scratch_words(bv, (uint32_t)n) * 4));
  TRY(ge.msm_short(ctx->stream, bv, scalars_dev, (uint32_t)n, (uint32_t*)ctx->short_ws.buf[SHORT_SCRATCH], out_dev));
  return PCDHIP_OK;
}
int msm_short_host(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars, size_t n, uint64_t* out_xyz) {
  if (!bases->shards.empty()) return PCDHIP_E_ARG;
  if (n > MSM_SHORT_MAX_N) return PCDHIP_E_SIZE_UNSUPPORTED;
  const size_t sbytes = n * kFieldLimbs[kCurveFr[bases->curve_id]] * 8;
  TRY(ctx->short_ws.ensure(SHORT_SCAL, std::max<size_t>(sbytes, 8)));
  if (n) TRY(hipMemcpyAsync(ctx->short_ws.buf[SHORT_SCAL], scalars, sbytes, hipMemcpyHostToDevice, ctx->stream));
  return msm_short_common(ctx, bases, offset, (const uint32_t*)ctx->short_ws.buf[SHORT_SCAL], n, out_xyz);
}
int msm_short_batch_async(pcdhip_ctx* ctx, const pcdhip_bases* bases, const MsmShortBatchIn* items, size_t k, uint32_t* out_dev,
                          size_t out_stride_words, const uint32_t** err_dev, uint32_t* launches) {
  if (!bases->shards.empty() || k >= (1ull << 31)) return PCDHIP_E_ARG;
  for (size_t j = 0; j < k; j++) {
    if (items[j].n > MSM_SHORT_MAX_N) return PCDHIP_E_SIZE_UNSUPPORTED;
    if (items[j].offset > bases->n || items[j].n > bases->n - items[j].offset) return PCDHIP_E_ARG;
  }
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const MsmBasesView bv = bases->view(0);
  TRY(ctx->short_ws.ensure(SHORT_BATCH, std::max<size_t>(ge.msm_short_batch_scratch_words(bv, items, (uint32_t)k), 4) * 4));
  uint32_t* scratch = (uint32_t*)ctx->short_ws.buf[SHORT_BATCH];
  uint32_t n_launch = 0;
  TRY(ge.msm_short_batch(ctx->stream, bv, items, (uint32_t)k, scratch, &ctx->short_batch_table, out_dev, out_stride_words, &n_launch));
  if (n_launch == 0) TRY(hipMemsetAsync(scratch, 0, 4, ctx->stream));  // (no MSM with n > 0: the error word is not written by a kernel)
  if (err_dev) *err_dev = scratch;
  if (launches) *launches = n_launch;
  return PCDHIP_OK;
}
}  // namespace pcd

extern "C" {

int pcdhip_msm_short_batch(pcdhip_ctx* ctx, const pcdhip_bases* bases, const uint64_t* scalars, size_t scalars_n, const pcdhip_msm_short_item* items,
                           size_t k, uint64_t* out_xyz) {
  return guarded([&]() -> int {
  if (!ctx || !bases || (k && (!items || !out_xyz)) || (!scalars && scalars_n) || !bases->shards.empty()) return PCDHIP_E_ARG;
  if (k == 0) return PCDHIP_OK;
  if (k > MSM_SHORT_BATCH_MAX_K) return PCDHIP_E_SIZE_UNSUPPORTED;
  int rc = msm_short_batch_check(bases, scalars_n, items, k);
  if (rc) return rc;
  BIND();
  const size_t sbytes = scalars_n * kFieldLimbs[kCurveFr[bases->curve_id]] * 8;
  TRY(ctx->short_ws.ensure(SHORT_SCAL, std::max<size_t>(sbytes, 8)));
  if (sbytes) TRY(hipMemcpyAsync(ctx->short_ws.buf[SHORT_SCAL], scalars, sbytes, hipMemcpyHostToDevice, ctx->stream));
  return msm_short_batch_common(ctx, bases, (const uint32_t*)ctx->short_ws.buf[SHORT_SCAL], items, k, out_xyz);
  });
}

int pcdhip_msm_short_batch_dev(pcdhip_ctx* ctx, const pcdhip_bases* bases, const pcdhip_buf* scalars, const pcdhip_msm_short_item* items, size_t k,
                               uint64_t* out_xyz) {
  return guarded([&]() -> int {
  if (!ctx || !bases || !scalars || (k && (!items || !out_xyz)) || !bases->shards.empty()) return PCDHIP_E_ARG;
  if (scalars->field_id != kCurveFr[bases->curve_id]) return PCDHIP_E_ARG;
  if (k == 0) return PCDHIP_OK;
  if (k > MSM_SHORT_BATCH_MAX_K) return PCDHIP_E_SIZE_UNSUPPORTED;
  int rc = msm_short_batch_check(bases, scalars->n, items, k);
  if (rc) return rc;
  BIND();
  return msm_short_batch_common(ctx, bases, scalars->dptr, items, k, out_xyz);
  });
}

int pcdhip_msm_short(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars, size_t n, uint64_t* out_xyz) {
  if (!ctx || !bases || (!scalars && n) || !out_xyz || !bases->shards.empty()) return PCDHIP_E_ARG;
  if (offset > bases->n || n > bases->n - offset) return PCDHIP_E_ARG;
  BIND();
  return msm_short_host(ctx, bases, offset, scalars, n, out_xyz);
}

int pcdhip_msm_short_dev(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset, size_t n,
                         uint64_t* out_xyz) {
  if (!ctx || !bases || !scalars || !out_xyz || !bases->shards.empty()) return PCDHIP_E_ARG;
  if (offset > bases->n || n > bases->n - offset || scalar_offset > scalars->n || n > scalars->n - scalar_offset) return PCDHIP_E_ARG;
  if (scalars->field_id != kCurveFr[bases->curve_id]) return PCDHIP_E_ARG;
  BIND();
  const size_t sw = (size_t)kFieldLimbs[scalars->field_id] * 2;
  return msm_short_common(ctx, bases, offset, scalars->dptr + scalar_offset * sw, n, out_xyz);
}

int pcdhip_msm_set_short(pcdhip_ctx* ctx, size_t max_n) {
  if (!ctx || max_n > MSM_SHORT_MAX_N) return PCDHIP_E_ARG;
  ctx->msm_short_max = max_n;
  return PCDHIP_OK;
}

}  // extern "C"
