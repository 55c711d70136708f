// Short MSMs without buckets at the C ABI (msm_short.hip.h through GroupEntry::msm_short): host and device scalars, and the opt-in
// routing of the KZG open side's small MSMs.
#include "capi_internal.h"
#include "msm_short.hip.h"

using namespace pcd;

namespace {
enum { SHORT_SCAL = 0, SHORT_SCRATCH, SHORT_OUT };  // slots of pcdhip_ctx::short_ws
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
}  // namespace pcd

extern "C" {

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
