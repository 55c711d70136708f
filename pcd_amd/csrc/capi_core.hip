// extern "C" surface of libpcdhip.so (include/pcdhip.h).  Host orchestration only: every arithmetic
// step is a HIP kernel from msm.hip.h / fft.hip.h / inst_*.hip.  There is no CPU fallback anywhere in this
// library -- if no GPU is usable, pcdhip_init fails with PCDHIP_E_NO_DEVICE and nothing else can be called.
// This unit: the entry tables, context lifetime, host memory, the timer, buffers.
#include "capi_internal.h"

namespace pcd {

#define PCD_DECL_G(k) const GroupEntry* pcd_group_entry_##k();
PCD_DECL_G(0) PCD_DECL_G(1) PCD_DECL_G(2) PCD_DECL_G(3) PCD_DECL_G(4) PCD_DECL_G(5) PCD_DECL_G(6) PCD_DECL_G(7)
#define PCD_DECL_F(k) const FieldEntry* pcd_field_entry_##k();
PCD_DECL_F(0) PCD_DECL_F(1) PCD_DECL_F(2) PCD_DECL_F(3)
#define PCD_DECL_C(k) const CurveEntry* pcd_curve_entry_##k();
PCD_DECL_C(0) PCD_DECL_C(1) PCD_DECL_C(2) PCD_DECL_C(3)
#define PCD_DECL_P(k) const PairingEntry* pcd_pairing_entry_##k();
PCD_DECL_P(0) PCD_DECL_P(1) PCD_DECL_P(2) PCD_DECL_P(3)

const GroupEntry& group_entry(int curve_id, int group_id) {
  typedef const GroupEntry* (*Fn)();
  static const Fn tab[8] = {pcd_group_entry_0, pcd_group_entry_1, pcd_group_entry_2, pcd_group_entry_3,
                            pcd_group_entry_4, pcd_group_entry_5, pcd_group_entry_6, pcd_group_entry_7};
  return *tab[curve_id * 2 + (group_id - 1)]();
}
const FieldEntry& field_entry(int field_id) {
  typedef const FieldEntry* (*Fn)();
  static const Fn tab[4] = {pcd_field_entry_0, pcd_field_entry_1, pcd_field_entry_2, pcd_field_entry_3};
  return *tab[field_id]();
}
const CurveEntry& curve_entry(int curve_id) {
  typedef const CurveEntry* (*Fn)();
  static const Fn tab[4] = {pcd_curve_entry_0, pcd_curve_entry_1, pcd_curve_entry_2, pcd_curve_entry_3};
  return *tab[curve_id]();
}

G1ScaleFn pcd_g1_scale_entry_0(); G1ScaleFn pcd_g1_scale_entry_1(); G1ScaleFn pcd_g1_scale_entry_2(); G1ScaleFn pcd_g1_scale_entry_3();
G1ScaleFn g1_scale_entry(int curve_id) {
  typedef G1ScaleFn (*Fn)();
  static const Fn tab[4] = {pcd_g1_scale_entry_0, pcd_g1_scale_entry_1, pcd_g1_scale_entry_2, pcd_g1_scale_entry_3};
  return tab[curve_id]();
}

const PairingEntry& pairing_entry(int curve_id) {
  typedef const PairingEntry* (*Fn)();
  static const Fn tab[4] = {pcd_pairing_entry_0, pcd_pairing_entry_1, pcd_pairing_entry_2, pcd_pairing_entry_3};
  return *tab[curve_id]();
}

}  // namespace pcd

using namespace pcd;

namespace {
// The roof the MSM, FFT and pairing kernels are priced against, measured on the device at hand: v_mad_u64_u32 issue rate with four waves
// per SIMD, eight independent accumulator chains per lane (tools/microbench/k0_int_rates.hip found 3.42e13 lane-mads/s that way in round 1;
// boxes of the pool differ by ~10 % in sustained clock, and a fraction against a constant moves with the box).
__global__ void __launch_bounds__(256) mad_rate_kernel(uint32_t* out, int iters, uint32_t seed) {
  uint32_t a = threadIdx.x * 2654435761u + seed, b = a ^ 0x9e3779b9u;
  uint64_t c0 = a, c1 = b, c2 = a + 1, c3 = b + 1, c4 = a + 2, c5 = b + 2, c6 = a + 3, c7 = b + 3;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int u = 0; u < 8; u++)
      asm volatile(
          "v_mad_u64_u32 %0, vcc, %8, %9, %0\n v_mad_u64_u32 %1, vcc, %8, %9, %1\n"
          "v_mad_u64_u32 %2, vcc, %8, %9, %2\n v_mad_u64_u32 %3, vcc, %8, %9, %3\n"
          "v_mad_u64_u32 %4, vcc, %8, %9, %4\n v_mad_u64_u32 %5, vcc, %8, %9, %5\n"
          "v_mad_u64_u32 %6, vcc, %8, %9, %6\n v_mad_u64_u32 %7, vcc, %8, %9, %7\n"
          : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7) : "v"(a), "v"(b) : "vcc");
  }
  const uint64_t x = c0 ^ c1 ^ c2 ^ c3 ^ c4 ^ c5 ^ c6 ^ c7;
  out[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)x ^ (uint32_t)(x >> 32);
}
}  // namespace

extern "C" {

const char* pcdhip_strerror(int code) {
  switch (code) {
    case PCDHIP_OK: return "ok";
    case PCDHIP_E_ARG: return "invalid argument";
    case PCDHIP_E_SIZE_UNSUPPORTED: return "size not supported by this build (e.g. log_n above the field's 2-adicity)";
    case PCDHIP_E_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case PCDHIP_E_OOM: return "out of device memory";
    case PCDHIP_E_HIP: return "HIP runtime error (see pcdhip_last_hip_error)";
    case PCDHIP_E_PREV_TICKET: return "the previous ticket of this slot had an unreduced scalar (this submission was enqueued)";
    default: return "unknown error";
  }
}

int pcdhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pcdhip_field_limbs(int field_id) { return valid_field(field_id) ? kFieldLimbs[field_id] : PCDHIP_E_ARG; }
int pcdhip_curve_base_field(int curve_id) { return valid_curve(curve_id) ? kCurveFq[curve_id] : PCDHIP_E_ARG; }
int pcdhip_curve_scalar_field(int curve_id) { return valid_curve(curve_id) ? kCurveFr[curve_id] : PCDHIP_E_ARG; }
int pcdhip_point_limbs(int curve_id, int group_id) {
  if (!valid_curve(curve_id) || !valid_group(group_id)) return PCDHIP_E_ARG;
  int deg = group_id == 1 ? 1 : kCurveG2Deg[curve_id];
  return 2 * deg * kFieldLimbs[kCurveFq[curve_id]];
}

int pcdhip_init(int device_id, pcdhip_ctx** out) {
  if (!out) return PCDHIP_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PCDHIP_E_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return PCDHIP_E_ARG;
  if (hipSetDevice(device_id) != hipSuccess) return PCDHIP_E_NO_DEVICE;
  pcdhip_ctx* ctx = new (std::nothrow) pcdhip_ctx();
  if (!ctx) return PCDHIP_E_OOM;
  ctx->device = device_id;
  // the context's own stream gets the highest priority: inside a proof it carries the witness map, whose small kernels
  // must not queue behind the MSMs of the other streams (the h MSM waits for it)
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest) != hipSuccess ||
      hipEventCreate(&ctx->t0) != hipSuccess || hipEventCreate(&ctx->t1) != hipSuccess) {
    delete ctx;
    return PCDHIP_E_HIP;
  }
  *out = ctx;
  return PCDHIP_OK;
}

int pcdhip_init_devices(const int* device_ids, int n_dev, pcdhip_ctx** out) {
  if (!device_ids || n_dev < 1 || n_dev > 64 || !out) return PCDHIP_E_ARG;
  int rc = pcdhip_init(device_ids[0], out);
  if (rc || n_dev == 1) return rc;
  pcdhip_ctx* ctx = *out;
  *out = nullptr;
  rc = guarded([&]() -> int {
    ctx->peers.push_back(ctx);
    for (int i = 1; i < n_dev; i++) {
      pcdhip_ctx* p = nullptr;
      int r = pcdhip_init(device_ids[i], &p);
      if (r) return r;
      ctx->peers.push_back(p);
    }
    // direct xGMI copies between the devices of the context where the platform allows them (the partial results and the
    // slices of h travel device to device; without peer access the runtime stages them through the host)
    for (pcdhip_ctx* a : ctx->peers)
      for (pcdhip_ctx* b : ctx->peers) {
        if (a->device == b->device) continue;
        int can = 0;
        if (hipSetDevice(a->device) != hipSuccess || hipDeviceCanAccessPeer(&can, a->device, b->device) != hipSuccess || !can) continue;
        if (hipDeviceEnablePeerAccess(b->device, 0) != hipSuccess) (void)hipGetLastError();  // (already enabled: fine)
      }
    return PCDHIP_OK;
  });
  if (rc) { pcdhip_destroy(ctx); return rc; }
  *out = ctx;
  return PCDHIP_OK;
}
int pcdhip_ctx_devices(const pcdhip_ctx* ctx) { return !ctx ? PCDHIP_E_ARG : ctx->peers.empty() ? 1 : (int)ctx->peers.size(); }

void pcdhip_destroy(pcdhip_ctx* ctx) {
  if (!ctx) return;
  for (size_t g = 1; g < ctx->peers.size(); g++) pcdhip_destroy(ctx->peers[g]);
  ctx->peers.clear();
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->msm_ws.release();
  ctx->aux_ws.release();
  ctx->short_ws.release();
  for (int k = 0; k < 6; k++) {
    ctx->g16_ws[k].release();
    if (ctx->g16_streams[k]) (void)hipStreamDestroy(ctx->g16_streams[k]);
    if (ctx->g16_begin[k]) (void)hipEventDestroy(ctx->g16_begin[k]);
    if (ctx->g16_end[k]) (void)hipEventDestroy(ctx->g16_end[k]);
  }
  if (ctx->lane_stream) (void)hipStreamDestroy(ctx->lane_stream);
  if (ctx->g16_ready) (void)hipEventDestroy(ctx->g16_ready);
  if (ctx->g16_share.ready) (void)hipEventDestroy(ctx->g16_share.ready);
  if (ctx->g16_share_b.ready) (void)hipEventDestroy(ctx->g16_share_b.ready);
  for (auto& kv : ctx->fft_tables) {
    (void)hipFree(kv.second.tw_fwd); (void)hipFree(kv.second.tw_inv);
    (void)hipFree(kv.second.coset); (void)hipFree(kv.second.coset_inv_scaled);
    (void)hipFree(kv.second.tw0_fwd); (void)hipFree(kv.second.tw0_inv);
  }
  if (ctx->xstream_ev) (void)hipEventDestroy(ctx->xstream_ev);
  if (ctx->wm_ev) (void)hipEventDestroy(ctx->wm_ev);
  for (int c = 0; c < 4; c++) if (ctx->vm_block[c]) (void)hipFree(ctx->vm_block[c]);
  for (int k = 0; k < pcdhip_ctx::PIPE_SLOTS; k++) if (ctx->pipe_done[k]) (void)hipEventDestroy(ctx->pipe_done[k]);
  if (ctx->pipe_host) (void)hipHostFree(ctx->pipe_host);
  if (ctx->count_host) (void)hipHostFree(ctx->count_host);
  if (ctx->count_ev) (void)hipEventDestroy(ctx->count_ev);
  if (ctx->t0) (void)hipEventDestroy(ctx->t0);
  if (ctx->t1) (void)hipEventDestroy(ctx->t1);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int pcdhip_host_alloc(size_t bytes, void** out) {
  if (!out) return PCDHIP_E_ARG;
  *out = nullptr;
  hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
  if (e == hipErrorOutOfMemory) return PCDHIP_E_OOM;
  return e == hipSuccess ? PCDHIP_OK : PCDHIP_E_HIP;
}
void pcdhip_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
int pcdhip_sync(pcdhip_ctx* ctx) {
  if (!ctx) return PCDHIP_E_ARG;
  BIND();
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
const char* pcdhip_last_hip_error(pcdhip_ctx* ctx) { return ctx ? ctx->last_hip_error.c_str() : ""; }

int pcdhip_timer_start(pcdhip_ctx* ctx) {
  if (!ctx) return PCDHIP_E_ARG;
  BIND();
  TRY(hipEventRecord(ctx->t0, ctx->stream));
  return PCDHIP_OK;
}
int pcdhip_timer_stop(pcdhip_ctx* ctx, float* out_ms) {
  if (!ctx || !out_ms) return PCDHIP_E_ARG;
  BIND();
  TRY(hipEventRecord(ctx->t1, ctx->stream));
  TRY(hipEventSynchronize(ctx->t1));
  TRY(hipEventElapsedTime(out_ms, ctx->t0, ctx->t1));
  return PCDHIP_OK;
}

// ------------------------------------------------------------------------------------------------ buffers
int pcdhip_buf_alloc(pcdhip_ctx* ctx, int field_id, size_t n, pcdhip_buf** out) {
  if (!ctx || !out || !valid_field(field_id)) return PCDHIP_E_ARG;
  BIND();
  pcdhip_buf* b = new (std::nothrow) pcdhip_buf();
  if (!b) return PCDHIP_E_OOM;
  b->field_id = field_id;
  b->n = n;
  b->dptr = nullptr;
  hipError_t e = hipMalloc(&b->dptr, std::max<size_t>(n, 1) * kFieldLimbs[field_id] * 8);
  if (e != hipSuccess) { delete b; return fail(ctx, e); }
  *out = b;
  return PCDHIP_OK;
}
int pcdhip_buf_upload(pcdhip_ctx* ctx, int field_id, const uint64_t* host, size_t n, pcdhip_buf** out) {
  if (!host && n) return PCDHIP_E_ARG;
  int rc = pcdhip_buf_alloc(ctx, field_id, n, out);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync((*out)->dptr, host, n * kFieldLimbs[field_id] * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { pcdhip_buf_free(ctx, *out); *out = nullptr; return fail(ctx, e); }
  return PCDHIP_OK;
}
int pcdhip_buf_download(pcdhip_ctx* ctx, const pcdhip_buf* buf, uint64_t* host, size_t n) {
  if (!ctx || !buf || !host || n > buf->n) return PCDHIP_E_ARG;
  BIND();
  TRY(hipMemcpyAsync(host, buf->dptr, n * kFieldLimbs[buf->field_id] * 8, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
void pcdhip_buf_free(pcdhip_ctx* ctx, pcdhip_buf* buf) {
  if (!buf) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  (void)hipFree(buf->dptr);
  delete buf;
}

int pcdhip_stream_wait(pcdhip_ctx* ctx, void* other_stream, int direction) {
  if (!ctx || direction < 0 || direction > 1) return PCDHIP_E_ARG;
  BIND();
  if (!ctx->xstream_ev) TRY(hipEventCreateWithFlags(&ctx->xstream_ev, hipEventDisableTiming));
  hipStream_t other = (hipStream_t)other_stream;
  TRY(hipEventRecord(ctx->xstream_ev, direction == 0 ? other : ctx->stream));
  TRY(hipStreamWaitEvent(direction == 0 ? ctx->stream : other, ctx->xstream_ev, 0));
  return PCDHIP_OK;
}
int pcdhip_mad_rate(pcdhip_ctx* ctx, double* out_lane_mads_per_s) {
  return guarded([&]() -> int {
  if (!ctx || !out_lane_mads_per_s) return PCDHIP_E_ARG;
  BIND();
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) cus = 256;
  const int blocks = cus * 4, iters = 1000;  // one workgroup of four waves per SIMD quartet, four of them per CU: four waves per SIMD
  TRY(ctx->aux_ws.ensure(AUX_SCAL, (size_t)blocks * 256 * 4));
  uint32_t* out = (uint32_t*)ctx->aux_ws.buf[AUX_SCAL];
  EventSet<2> ev;
  TRY(ev.create());
  float best = 0;
  for (int r = 0; r < 9; r++) {  // (the first pass warms up; the best of eight: the clock needs a few milliseconds of load to settle)
    TRY(hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL(mad_rate_kernel, dim3(blocks), dim3(256), 0, ctx->stream, out, r ? iters : 10, (uint32_t)r);
    TRY(hipEventRecord(ev[1], ctx->stream));
    TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (r && (best == 0 || ms < best)) best = ms;
  }
  TRY(hipGetLastError());
  *out_lane_mads_per_s = (double)blocks * 256.0 * iters * 64.0 / ((double)best * 1e-3);
  return PCDHIP_OK;
  });
}

}  // extern "C"
