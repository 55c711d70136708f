// The MSM front end of libpcdhip.so: resident bases and their precomputed copies, the MSM settings, the side streams and the accumulate
// lane, the submit / collect pipeline, multi-device sharding, and the small point utilities.
#include <mutex>

#include "capi_internal.h"

using namespace pcd;

namespace {
// affine points flagged as the point at infinity become literal zeros (0, 0) -- the device encoding of the identity
// (not on any of the eight curves: b != 0); `flags` = one byte per point, already on the device
__global__ void __launch_bounds__(256) zero_flagged_kernel(uint32_t* __restrict__ pts, const uint8_t* __restrict__ flags, size_t n_words,
                                                            uint32_t words_per_point) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words && flags[i / words_per_point]) pts[i] = 0;
}

// the context's side streams (created on first use): 0 and 1 with the highest priority, 2 with the default one, 3..5 with the lowest
// ... and the accumulate lane: a stream whose queue may use all but `lane_reserve` compute units.  The mask bits are dealt to the XCDs
// round-robin (bit i -> XCD i mod 8: tools/microbench/k3_cu_mask.hip, profiles/r05_k3_cu_mask.txt), so clearing the LAST 8 k bits leaves
// k CUs free in every XCD -- an unmasked kernel's workgroups are dealt to the XCDs round-robin as well, so each needs a free CU of its own.
int lane_reserve_of(const pcdhip_ctx* ctx) {
  int r = ctx->lane_reserve;
  if (r < 0) { const char* e = getenv("PCDHIP_LANE_RESERVE"); r = e ? atoi(e) : 8; }
  return r < 0 ? 0 : r;
}
// CU-masked streams are made once per (device, reserve) and NEVER destroyed: on this stack (ROCm 7.2) hipStreamDestroy of a stream created
// by hipExtStreamCreateWithCUMask stalls for good now and then once such streams have been created and destroyed before in the process
// (round 5: a soak that toggled the schedule per proof hung in the second round of destructions, profiles/r05_stress.log).  Contexts
// of one device share the lane: stream order only adds dependencies between their accumulations, and the mode is not the default.
hipStream_t masked_lane_of(int device, int cus, int reserve, hipError_t* err) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, hipStream_t> pool;
  std::lock_guard<std::mutex> lock(mu);
  auto it = pool.find({device, reserve});
  if (it != pool.end()) { *err = hipSuccess; return it->second; }
  std::vector<uint32_t> mask((cus + 31) / 32, 0u);
  for (int i = 0; i < cus - reserve; i++) mask[i / 32] |= 1u << (i % 32);
  hipStream_t s = nullptr;
  *err = hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data());
  if (*err == hipSuccess) pool[{device, reserve}] = s;
  return s;
}
int make_side_streams(pcdhip_ctx* ctx) {
  int least = 0, greatest = 0;
  TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  const bool lane_mode = ctx->g16_schedule == 2;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) cus = 256;
  const int normal = (least + greatest) / 2;
  for (int k = 0; k < 6; k++) {
    // The runtime multiplexes the streams of ONE priority over a few hardware queues (three for the high priority on this stack), and two
    // streams that share a queue run in submission order: with four high-priority streams the sort of l' sat in the queue of the B MSM, behind
    // that MSM's wait for its accumulation on the lane -- l' and h started 3 ms late (profiles/r05_pt_lane_aliased.txt: q5 carries s4 AND s5).
    // Lane mode therefore spreads its six side streams two per priority (with the context's own stream: three at the normal one); the other
    // schedules keep round 4's mix (2 high, 1 normal, 3 low).
    int prio = lane_mode ? (k < 2 ? greatest : k < 4 ? normal : least) : (k < 2 ? greatest : k == 2 ? normal : least);
    static const char* side_prio = getenv("PCDHIP_SIDE_PRIO");  // developer knob: "low" = every side stream at the lowest priority, "mid" = none above normal
    if (side_prio && !strcmp(side_prio, "low")) prio = least;
    if (side_prio && !strcmp(side_prio, "mid")) prio = k < 3 ? normal : least;
    TRY(hipStreamCreateWithPriority(&ctx->g16_streams[k], hipStreamNonBlocking, prio));
    TRY(hipEventCreate(&ctx->g16_begin[k]));
    TRY(hipEventCreate(&ctx->g16_end[k]));
  }
  if (lane_mode) {
    int reserve = lane_reserve_of(ctx);
    if (reserve >= cus) reserve = 0;
    if (reserve > 0) {
      hipError_t e = hipSuccess;
      ctx->lane.stream = masked_lane_of(ctx->device, cus, reserve, &e);
      TRY(e);
    } else {
      TRY(hipStreamCreateWithPriority(&ctx->lane_stream, hipStreamNonBlocking, least));   // (owned: an ordinary stream can be destroyed)
      ctx->lane.stream = ctx->lane_stream;
    }
    ctx->lane.cus = cus - reserve;
  }
  TRY(hipEventCreateWithFlags(&ctx->g16_ready, hipEventDisableTiming));
  return PCDHIP_OK;
}
}  // namespace

namespace pcd {
// developer knob (A/B of the partition sort's write pass, msm.hip.h): PCDHIP_COARSE_TILE = 0 selects the direct write pass, 256 .. 2048
// bounds the staged pass's tile from above; anything else, or unset, leaves the choice to msm_stage_tile
int msm_coarse_tile_knob() {
  static const int knob = [] {
    const char* e = getenv("PCDHIP_COARSE_TILE");
    if (!e || *e < '0' || *e > '9') return -1;
    const int v = atoi(e);
    return v == 0 || (v >= (int)MSM_STAGE_TILE_MIN && v <= (int)MSM_STAGE_TILE_MAX) ? v : -1;
  }();
  return knob;
}

// developer knob (A/B of the partition sort's per-bin sort, msm.hip.h): PCDHIP_BIN_STAGE = 0 selects msm_bin_sort_kernel for the whole process
int msm_bin_stage_knob() {
  static const int knob = [] {
    const char* e = getenv("PCDHIP_BIN_STAGE");
    return e && e[0] == '0' && e[1] == 0 ? 0 : -1;
  }();
  return knob;
}

hipError_t zero_flagged(hipStream_t st, uint32_t* pts_dev, uint8_t* flags_dev, const uint8_t* flags_host, size_t n, size_t point_bytes) {
  if (!flags_host || !n) return hipSuccess;
  hipError_t e = hipMemcpyAsync(flags_dev, flags_host, n, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  const size_t nw = n * (point_bytes / 4);
  hipLaunchKernelGGL(zero_flagged_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, pts_dev, flags_dev, nw, (uint32_t)(point_bytes / 4));
  return hipGetLastError();
}

// contiguous range [lo, hi) of part g out of `parts` (sizes differ by at most one) -- the point-range sharding of SURVEY.md 8e
void shard_range(size_t n, size_t g, size_t parts, size_t* lo, size_t* hi) {
  const size_t base = n / parts, rem = n % parts;
  *lo = g * base + std::min(g, rem);
  *hi = *lo + base + (g < rem ? 1 : 0);
}
int bases_upload_single(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xy, const uint8_t* inf, size_t n, pcdhip_bases** out) {
  BIND();
  const GroupEntry& ge = group_entry(curve_id, group_id);
  const size_t abi_b = (size_t)ge.point_abi_words * 4, int_b = (size_t)ge.base_stride_words * 4;
  pcdhip_bases* b = new (std::nothrow) pcdhip_bases();
  if (!b) return PCDHIP_E_OOM;
  b->curve_id = curve_id; b->group_id = group_id; b->n = n; b->dptr = nullptr; b->c = 0; b->groups = 1;
  // Precomputed window-shifted copies (HBM capacity traded for the serial window combine): group g
  // holds 2^(c Wg g) P_i.  Full precomputation (Wg = 1) needs W copies of the query vector.
  if (ctx->precompute != 0 && n >= 64) {
    const bool full = ctx->precompute < 0;
    const int c = ctx->msm_c ? ctx->msm_c : std::max(6, msm_pick_window(n, ge.scalar_bits, full ? 1 : 0) + ctx->msm_c_bias);
    const int W = msm_num_windows(ge.scalar_bits, c);
    b->c = c;
    b->groups = full ? W : std::min(W, ctx->precompute);
  }
  hipError_t e = hipErrorOutOfMemory;
  while (true) {
    const size_t want = std::max<size_t>(n, 1) * int_b * b->groups;
    // (the caller's budget for one vector counts like the device running out: a host that keeps several keys resident sets it)
    e = (ctx->precompute_budget && want > ctx->precompute_budget && b->groups > 1) ? hipErrorOutOfMemory : hipMalloc(&b->dptr, want);
    if (e == hipSuccess || b->groups == 1) break;
    (void)hipGetLastError();
    b->groups = (b->groups + 1) / 2;  // not enough HBM for this many copies: fewer groups, more bucket windows
  }
  if (e != hipSuccess) { (void)hipGetLastError(); delete b; return fail(ctx, e); }   // (the sticky error must not surface at a later launch's hipGetLastError)
  if (b->groups == 1) b->c = 0;
  // stage the C-ABI image, rewrite flagged points to (0, 0) (not on any of the curves: b != 0), convert
  e = ctx->aux_ws.ensure(AUX_MISC, std::max<size_t>(n, 1) * (abi_b + 1) + 64);
  char* stage = (char*)ctx->aux_ws.buf[AUX_MISC];
  if (e == hipSuccess) e = hipMemcpyAsync(stage, xy, n * abi_b, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = zero_flagged(ctx->stream, (uint32_t*)stage, (uint8_t*)stage + n * abi_b, inf, n, abi_b);
  if (e == hipSuccess) e = ge.points_in(ctx->stream, (const uint32_t*)stage, (uint32_t)n, b->dptr);
  if (e == hipSuccess && b->groups > 1) {
    const int W = msm_num_windows(ge.scalar_bits, b->c);
    const int Wg = (W + b->groups - 1) / b->groups;
    e = ge.precompute(ctx->stream, b->dptr, (uint32_t)n, b->groups, b->c * Wg);
  }
  // the points at infinity as a bitmap: their entries never enter an MSM's bucket lists (msm_base_is_inf)
  if (e == hipSuccess && inf) {
    std::vector<uint32_t> bits((n + 31) / 32 + 1, 0u);
    bool any = false;
    for (size_t i = 0; i < n; i++) if (inf[i]) { bits[i >> 5] |= 1u << (i & 31); any = true; }
    if (any) {
      e = hipMalloc((void**)&b->inf_bits, bits.size() * 4);
      if (e == hipSuccess) e = hipMemcpyAsync(b->inf_bits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (`bits` is a local)
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { (void)hipFree(b->dptr); (void)hipFree(b->inf_bits); delete b; return fail(ctx, e); }
  *out = b;
  return PCDHIP_OK;
}

int msm_common(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint32_t* scalars_dev, size_t n,
               uint64_t* out_xyz, bool out_on_device) {
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const size_t jac_b = (size_t)ge.point_words / 2 * 3 * 4, jac_abi_b = (size_t)ge.point_abi_words / 2 * 3 * 4;
  TRY(ctx->msm_ws.ensure(WS_OUT, jac_b + jac_abi_b + 64));
  uint32_t* out_dev = (uint32_t*)ctx->msm_ws.buf[WS_OUT];
  uint32_t* out_abi = out_dev + jac_b / 4;
  TRY(ge.msm(ctx->msm_ws, ctx->stream, bases->view(offset), scalars_dev, (uint32_t)n, out_dev, ctx->msm_c, ctx->msm_chunk,
             ctx->msm_sort, ctx->msm_profile ? &ctx->msm_tm : nullptr, nullptr, MSM_SHARE_NONE));
  if (out_on_device) { TRY(ge.jac_out(ctx->stream, out_dev, 1, (uint32_t*)out_xyz)); return PCDHIP_OK; }  // asynchronous
  TRY(ge.jac_out(ctx->stream, out_dev, 1, out_abi));
  TRY(hipMemcpyAsync(out_xyz, out_abi, jac_abi_b, hipMemcpyDeviceToHost, ctx->stream));
  uint32_t too_wide = 0;  // a scalar that is not a reduced canonical value (>= 2^bits): the digits would silently drop its top
  if (ctx->msm_ws.last_err_dev) TRY(hipMemcpyAsync(&too_wide, ctx->msm_ws.last_err_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return too_wide ? PCDHIP_E_ARG : PCDHIP_OK;
}

int ensure_side_streams(pcdhip_ctx* ctx) {
  if (ctx->g16_ready) return PCDHIP_OK;
  const int rc = make_side_streams(ctx);
  // (g16_ready is set last, so a failure partway -- a CU-masked stream the runtime refuses, the sixth stream -- used to leave
  //  the streams and events made so far in the context, to be overwritten and leaked by the next call: destroy them here instead)
  if (rc) (void)drop_side_streams(ctx, true);
  return rc;
}
// (a change of schedule or of the lane's reserve takes effect on streams made afresh)
int drop_side_streams(pcdhip_ctx* ctx, bool partial) {
  if (!ctx->g16_ready && !partial) return PCDHIP_OK;
  BIND();
  if (!partial) TRY(hipDeviceSynchronize());   // (partial: nothing has been enqueued on streams that were never handed out)
  for (int k = 0; k < 6; k++) {
    if (ctx->g16_streams[k]) { (void)hipStreamDestroy(ctx->g16_streams[k]); ctx->g16_streams[k] = nullptr; }
    if (ctx->g16_begin[k]) { (void)hipEventDestroy(ctx->g16_begin[k]); ctx->g16_begin[k] = nullptr; }
    if (ctx->g16_end[k]) { (void)hipEventDestroy(ctx->g16_end[k]); ctx->g16_end[k] = nullptr; }
  }
  if (ctx->lane_stream) { (void)hipStreamDestroy(ctx->lane_stream); ctx->lane_stream = nullptr; }   // (only the unmasked lane is owned)
  ctx->lane = MsmLane();
  if (ctx->g16_ready) (void)hipEventDestroy(ctx->g16_ready);
  ctx->g16_ready = nullptr;
  return PCDHIP_OK;
}
bool pipe_pending(const pcdhip_ctx* ctx) {
  for (int k = 0; k < pcdhip_ctx::PIPE_SLOTS; k++) if (ctx->pipe_busy[k]) return true;
  return false;
}

// (every error exit drains the peer streams before the frames that outstanding copies point into -- the error words, the caller's
//  scalars -- go away)
void drain_peers(pcdhip_ctx* ctx) {
  for (pcdhip_ctx* C : ctx->peers) { if (hipSetDevice(C->device) == hipSuccess) (void)hipStreamSynchronize(C->stream); }
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
}
}  // namespace pcd

namespace {
int msm_submit_common(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset, size_t n,
                      uint64_t* out_xyz_device, size_t out_slot_stride, int* ticket) {
  if (!ctx || !bases || !scalars || !ticket || !bases->shards.empty()) return PCDHIP_E_ARG;
  if (offset + n > bases->n || scalar_offset + n > scalars->n || n >= (1ull << 31)) return PCDHIP_E_ARG;
  if (scalars->field_id != kCurveFr[bases->curve_id]) return PCDHIP_E_ARG;
  BIND();
  int rc = ensure_side_streams(ctx);
  if (rc) return rc;
  int slot = -1;
  for (int t = 0; t < pcdhip_ctx::PIPE_SLOTS; t++) {
    const int k = (ctx->pipe_next + t) % pcdhip_ctx::PIPE_SLOTS;
    if (!ctx->pipe_busy[k]) { slot = k; break; }
  }
  if (slot < 0) return PCDHIP_E_ARG;  // PIPE_SLOTS submissions are in flight: collect one first
  ctx->pipe_next = (slot + 1) % pcdhip_ctx::PIPE_SLOTS;
  if (!ctx->pipe_host) TRY(hipHostMalloc((void**)&ctx->pipe_host, pcdhip_ctx::PIPE_SLOTS * pcdhip_ctx::PIPE_HOST_WORDS * 8, hipHostMallocDefault));
  if (!ctx->pipe_done[slot]) TRY(hipEventCreateWithFlags(&ctx->pipe_done[slot], hipEventDisableTiming));
  bool prev_bad = false;
  if (ctx->pipe_partial[slot]) {
    // the slot's previous ticket was handed to another stream (pcdhip_msm_ticket_wait), so nobody has looked at its error word and its
    // device-to-host copy may still be in flight: wait for that MSM (long finished in a pipelined loop: it was submitted PIPE_SLOTS
    // submissions ago and its gather has been consumed) before the word is reset, and report an unreduced scalar HERE
    TRY(hipEventSynchronize(ctx->pipe_done[slot]));
    ctx->pipe_partial[slot] = false;
    // (a code of its own, and the new submission goes ahead -- the caller learns that an EARLIER result was wrong without losing
    //  this one or mistaking the code for a refusal)
    prev_bad = (uint32_t)ctx->pipe_host[(size_t)slot * pcdhip_ctx::PIPE_HOST_WORDS + pcdhip_ctx::PIPE_HOST_WORDS - 1] != 0;
  }
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const size_t jac_b = (size_t)ge.point_words / 2 * 3 * 4, jac_abi_b = (size_t)ge.point_abi_words / 2 * 3 * 4;
  MsmWorkspace& ws = ctx->g16_ws[2 + slot];
  hipStream_t sk = ctx->g16_streams[2 + slot];
  TRY(ws.ensure(WS_OUT, jac_b + jac_abi_b + 64));
  uint32_t* out_dev = (uint32_t*)ws.buf[WS_OUT];
  uint32_t* out_abi = out_xyz_device ? (uint32_t*)((char*)out_xyz_device + (size_t)slot * out_slot_stride) : out_dev + jac_b / 4;
  // ordered behind whatever the context's own stream has queued so far (uploads of the operands; for the device-result form also
  // the previous reader of `out_xyz_device`, which pcdhip_stream_wait put in front of the context's stream)
  TRY(hipEventRecord(ctx->g16_ready, ctx->stream));
  TRY(hipStreamWaitEvent(sk, ctx->g16_ready, 0));
  const size_t sw = (size_t)kFieldLimbs[scalars->field_id] * 2;
  // (the accumulations of the MSMs in flight run one after the other on the lane; sorts and bucket reductions beside them)
  ws.lane = ctx->g16_schedule == 2 && ctx->pipe_lane && ctx->lane.stream ? &ctx->lane : nullptr;
  const hipError_t me = ge.msm(ws, sk, bases->view(offset), scalars->dptr + scalar_offset * sw, (uint32_t)n, out_dev, ctx->msm_c, ctx->msm_chunk, ctx->msm_sort,
                               nullptr, nullptr, MSM_SHARE_NONE);
  ws.lane = nullptr;
  TRY(me);
  TRY(ge.jac_out(sk, out_dev, 1, out_abi));
  uint64_t* host = ctx->pipe_host + (size_t)slot * pcdhip_ctx::PIPE_HOST_WORDS;
  host[pcdhip_ctx::PIPE_HOST_WORDS - 1] = 0;
  if (!out_xyz_device) TRY(hipMemcpyAsync(host, out_abi, jac_abi_b, hipMemcpyDeviceToHost, sk));
  if (ws.last_err_dev) TRY(hipMemcpyAsync(&host[pcdhip_ctx::PIPE_HOST_WORDS - 1], ws.last_err_dev, 4, hipMemcpyDeviceToHost, sk));
  TRY(hipEventRecord(ctx->pipe_done[slot], sk));
  ctx->pipe_busy[slot] = true;
  ctx->pipe_out_bytes[slot] = out_xyz_device ? 0 : jac_abi_b;
  *ticket = slot;
  return prev_bad ? PCDHIP_E_PREV_TICKET : PCDHIP_OK;
}

// MSM over bases sharded across the devices of the context: every device runs the whole pipeline on the part of [offset, offset + n)
// that falls into its point range (scalars: the matching slice of the host vector), the partial results travel device to device
// into device 0's gather buffer and one wave sums them there.  No host synchronisation before the result is read back.
int msm_sharded_impl(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars, size_t n, uint64_t* out_xyz,
                     uint32_t* too_wide) {
  const size_t G = bases->shards.size();
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const size_t jb = (size_t)ge.point_abi_words / 2 * 3 * 4, ji = (size_t)ge.point_words / 2 * 3 * 4;
  const size_t sl = (size_t)kFieldLimbs[kCurveFr[bases->curve_id]];
  BIND();
  TRY(ctx->aux_ws.ensure(AUX_MISC, (G + 1) * jb + 64 * ji + 64));
  uint32_t* d = (uint32_t*)ctx->aux_ws.buf[AUX_MISC];  // result | gathered partials | tree scratch
  uint32_t* gather = d + jb / 4;
  uint32_t* scratch = d + (G + 1) * jb / 4;
  for (size_t g = 0; g < G; g++) {
    const size_t lo = std::max(offset, bases->shard_lo[g]), hi = std::min(offset + n, bases->shard_lo[g + 1]);
    pcdhip_ctx* C = ctx->peers[g];
    if (hi <= lo) {  // nothing of this MSM on device g: its partial is the identity (Z = 0)
      TRY(hipSetDevice(ctx->device));
      TRY(hipMemsetAsync((char*)gather + g * jb, 0, jb, ctx->stream));
      continue;
    }
    const pcdhip_bases* sh = bases->shards[g];
    const size_t ng = hi - lo;
    C->msm_sort = ctx->msm_sort;
    {
      pcdhip_ctx* ctx = C;  // (TRY / BIND report into the device's own context)
      BIND();
      const size_t sbytes = ng * sl * 8;
      TRY(C->msm_ws.ensure(WS_SCAL, std::max<size_t>(sbytes, 8)));
      TRY(C->msm_ws.ensure(WS_OUT, ji + jb + 64));
      TRY(hipMemcpyAsync(C->msm_ws.buf[WS_SCAL], scalars + (lo - offset) * sl, sbytes, hipMemcpyHostToDevice, C->stream));
      uint32_t* out_dev = (uint32_t*)C->msm_ws.buf[WS_OUT];
      uint32_t* out_abi = out_dev + ji / 4;
      TRY(ge.msm(C->msm_ws, C->stream, sh->view(lo - bases->shard_lo[g]), (const uint32_t*)C->msm_ws.buf[WS_SCAL], (uint32_t)ng, out_dev, C->msm_c,
                 C->msm_chunk, C->msm_sort, nullptr, nullptr, MSM_SHARE_NONE));
      TRY(ge.jac_out(C->stream, out_dev, 1, out_abi));
      if (C->msm_ws.last_err_dev) TRY(hipMemcpyAsync(&too_wide[g], C->msm_ws.last_err_dev, 4, hipMemcpyDeviceToHost, C->stream));
    }
    const uint32_t* out_abi = (const uint32_t*)C->msm_ws.buf[WS_OUT] + ji / 4;
    TRY(hipSetDevice(C->device));
    TRY(hipMemcpyPeerAsync((char*)gather + g * jb, ctx->device, out_abi, C->device, jb, C->stream));
    if (C != ctx) {
      if (!C->xstream_ev) TRY(hipEventCreateWithFlags(&C->xstream_ev, hipEventDisableTiming));
      TRY(hipEventRecord(C->xstream_ev, C->stream));
      TRY(hipSetDevice(ctx->device));
      TRY(hipStreamWaitEvent(ctx->stream, C->xstream_ev, 0));
    }
  }
  BIND();
  TRY(ge.points_sum(ctx->stream, gather, (uint32_t)G, scratch, d));
  TRY(hipMemcpyAsync(out_xyz, d, jb, hipMemcpyDeviceToHost, ctx->stream));
  for (size_t g = 1; g < G; g++) { TRY(hipSetDevice(ctx->peers[g]->device)); TRY(hipStreamSynchronize(ctx->peers[g]->stream)); }
  BIND();
  TRY(hipStreamSynchronize(ctx->stream));
  for (size_t g = 0; g < G; g++) if (too_wide[g]) return PCDHIP_E_ARG;
  return PCDHIP_OK;
}
int msm_sharded(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars, size_t n, uint64_t* out_xyz) {
  if (ctx->peers.size() != bases->shards.size() || ctx->peers.size() > 64) return PCDHIP_E_ARG;
  uint32_t too_wide[64] = {0};
  const int rc = msm_sharded_impl(ctx, bases, offset, scalars, n, out_xyz, too_wide);
  if (rc) drain_peers(ctx);
  return rc;
}

int points_sum_common(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz, size_t n, uint64_t* out_xyz, bool in_on_device) {
  if (!ctx || !valid_curve(curve_id) || !valid_group(group_id) || (!xyz && n) || !out_xyz || (n >> 24)) return PCDHIP_E_ARG;
  BIND();
  const GroupEntry& ge = group_entry(curve_id, group_id);
  const size_t jb = (size_t)ge.point_abi_words / 2 * 3 * 4, ji = (size_t)ge.point_words / 2 * 3 * 4;
  TRY(ctx->aux_ws.ensure(AUX_MISC, (n + 1) * jb + 64 * ji + 64));
  uint32_t* d = (uint32_t*)ctx->aux_ws.buf[AUX_MISC];  // result | staged input | tree scratch
  uint32_t* scratch = d + (n + 1) * jb / 4;
  const uint32_t* in = (const uint32_t*)xyz;
  if (!in_on_device) {
    TRY(hipMemcpyAsync(d + jb / 4, xyz, n * jb, hipMemcpyHostToDevice, ctx->stream));
    in = d + jb / 4;
  }
  TRY(ge.points_sum(ctx->stream, in, (uint32_t)n, scratch, d));
  TRY(hipMemcpyAsync(out_xyz, d, jb, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
}  // namespace

extern "C" {

int pcdhip_bases_upload(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xy, const uint8_t* inf, size_t n,
                        pcdhip_bases** out) {
  if (!ctx || !out || !valid_curve(curve_id) || !valid_group(group_id) || (!xy && n) || n >= (1ull << 31)) return PCDHIP_E_ARG;
  if (ctx->peers.size() <= 1) return bases_upload_single(ctx, curve_id, group_id, xy, inf, n, out);
  // multi-device context: one ordinary handle per device, each over its point range
  *out = nullptr;
  return guarded([&]() -> int {
    pcdhip_bases* b = new pcdhip_bases();
    b->curve_id = curve_id; b->group_id = group_id; b->n = n; b->dptr = nullptr; b->c = 0; b->groups = 1;
    const size_t G = ctx->peers.size(), pl = (size_t)pcdhip_point_limbs(curve_id, group_id);
    b->shard_lo.resize(G + 1);
    for (size_t g = 0; g < G; g++) {
      size_t lo, hi;
      shard_range(n, g, G, &lo, &hi);
      b->shard_lo[g] = lo; b->shard_lo[g + 1] = hi;
      pcdhip_ctx* C = ctx->peers[g];
      C->precompute = ctx->precompute; C->precompute_budget = ctx->precompute_budget; C->msm_c = ctx->msm_c;
      pcdhip_bases* sh = nullptr;
      int rc = bases_upload_single(C, curve_id, group_id, xy + lo * pl, inf ? inf + lo : nullptr, hi - lo, &sh);
      if (rc) { pcdhip_bases_free(ctx, b); return rc; }
      b->shards.push_back(sh);
    }
    *out = b;
    return PCDHIP_OK;
  });
}
int pcdhip_set_precompute(pcdhip_ctx* ctx, int mode) {
  if (!ctx || mode < -1 || mode == 1) return PCDHIP_E_ARG;
  ctx->precompute = mode;
  return PCDHIP_OK;
}
int pcdhip_set_precompute_budget(pcdhip_ctx* ctx, size_t bytes_per_vector) {
  if (!ctx) return PCDHIP_E_ARG;
  ctx->precompute_budget = bytes_per_vector;
  return PCDHIP_OK;
}
int pcdhip_get_precompute_budget(pcdhip_ctx* ctx, size_t* bytes_per_vector) {
  if (!ctx || !bytes_per_vector) return PCDHIP_E_ARG;
  *bytes_per_vector = ctx->precompute_budget;
  return PCDHIP_OK;
}
void pcdhip_bases_free(pcdhip_ctx* ctx, pcdhip_bases* bases) {
  if (!bases) return;
  for (size_t g = 0; g < bases->shards.size(); g++)
    pcdhip_bases_free(ctx && g < ctx->peers.size() ? ctx->peers[g] : ctx, bases->shards[g]);
  bases->shards.clear();
  if (ctx) (void)hipSetDevice(ctx->device);
  (void)hipFree(bases->dptr);
  (void)hipFree(bases->inf_bits);
  delete bases;
}
int pcdhip_bases_info(const pcdhip_bases* bases, size_t n, int* window_bits, int* windows, int* copies) {
  if (!bases || !window_bits || !windows || !copies) return PCDHIP_E_ARG;
  if (!bases->shards.empty()) return pcdhip_bases_info(bases->shards[0], 0, window_bits, windows, copies);  // (the plan of device 0's shard)
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const int c = bases->groups > 1 ? bases->c : msm_pick_window(n ? n : bases->n, ge.scalar_bits, 0);
  *window_bits = c;
  *windows = msm_num_windows(ge.scalar_bits, c);
  *copies = bases->groups;
  return PCDHIP_OK;
}
int pcdhip_msm_config(pcdhip_ctx* ctx, int window_bits, int chunk) {
  if (!ctx || window_bits < 0 || window_bits > 24 || chunk < 0) return PCDHIP_E_ARG;
  ctx->msm_c = window_bits;
  ctx->msm_chunk = (uint32_t)chunk;
  return PCDHIP_OK;
}
int pcdhip_msm_set_sort(pcdhip_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 4) return PCDHIP_E_ARG;  // (3 / 4: the partition sort of mode 0 with the direct write pass / the two-read bin sort)
  ctx->msm_sort = (ctx->msm_sort & ~15) | mode;  // (the higher bits carry pcdhip_msm_set_accumulate's choice: msm.hip.h msm_run)
  return PCDHIP_OK;
}
int pcdhip_msm_set_bin_stage(pcdhip_ctx* ctx, int cap) {
  if (!ctx || cap < -1 || cap > (int)MSM_BIN_STAGE_CAP) return PCDHIP_E_ARG;
  // (every workspace an msm_run of this context may be given: its own, the proof's and the pipeline's, on every device)
  const std::vector<pcdhip_ctx*> one{ctx};
  for (pcdhip_ctx* c : ctx->peers.empty() ? one : ctx->peers) {
    c->msm_ws.bin_stage = cap;
    for (pcd::MsmWorkspace& w : c->g16_ws) w.bin_stage = cap;
  }
  return PCDHIP_OK;
}
int pcdhip_msm_set_accumulate(pcdhip_ctx* ctx, int mode, int chunk, int min_pairs) {
  if (!ctx || mode < 0 || mode > 2 || chunk < 0 || chunk > 1024 || (chunk && chunk < 2) || min_pairs < 0 || min_pairs > 255) return PCDHIP_E_ARG;
  ctx->msm_sort = (ctx->msm_sort & 15) | (mode << 4) | (chunk << 8) | (min_pairs << 20);
  return PCDHIP_OK;
}
int pcdhip_msm_profile(pcdhip_ctx* ctx, int on) {
  if (!ctx) return PCDHIP_E_ARG;
  ctx->msm_profile = on != 0;
  return PCDHIP_OK;
}
int pcdhip_msm_last_plan(pcdhip_ctx* ctx, uint32_t out[2]) {
  if (!ctx || !out) return PCDHIP_E_ARG;
  out[0] = ctx->msm_tm.entries; out[1] = ctx->msm_tm.chunk;
  return PCDHIP_OK;
}
int pcdhip_msm_last_timings(pcdhip_ctx* ctx, float out_ms[8]) {
  if (!ctx || !out_ms) return PCDHIP_E_ARG;
  const MsmTimings& t = ctx->msm_tm;
  float v[8] = {t.digits, t.scan, t.scatter, t.accumulate, t.fixup, t.tail, t.horner, t.total};
  memcpy(out_ms, v, sizeof v);
  return PCDHIP_OK;
}

int pcdhip_msm_ticket_status(pcdhip_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= pcdhip_ctx::PIPE_SLOTS || ctx->pipe_busy[slot] || !ctx->pipe_partial[slot]) return PCDHIP_E_ARG;
  BIND();
  TRY(hipEventSynchronize(ctx->pipe_done[slot]));
  ctx->pipe_partial[slot] = false;
  return (uint32_t)ctx->pipe_host[(size_t)slot * pcdhip_ctx::PIPE_HOST_WORDS + pcdhip_ctx::PIPE_HOST_WORDS - 1] ? PCDHIP_E_PREV_TICKET : PCDHIP_OK;
}
int pcdhip_msm_submit(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset, size_t n,
                      int* ticket) {
  // (PCDHIP_E_PREV_TICKET belongs to the released-ticket form alone.  A plain submission that lands on a slot whose last
  //  user was released by pcdhip_msm_ticket_wait clears that slot's deferred word without reporting it -- callers of this entry point
  //  treat any non-zero code as a refusal and would drop a ticket that IS in flight, leaving the slot busy for good.  A caller that
  //  mixes both forms polls pcdhip_msm_ticket_status before it switches.)
  const int rc = msm_submit_common(ctx, bases, offset, scalars, scalar_offset, n, nullptr, 0, ticket);
  return rc == PCDHIP_E_PREV_TICKET ? PCDHIP_OK : rc;
}
int pcdhip_msm_submit_partial(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset, size_t n,
                              uint64_t* out_xyz_device_slots, size_t slot_stride_bytes, int* ticket) {
  if (!out_xyz_device_slots || (slot_stride_bytes & 7)) return PCDHIP_E_ARG;
  return msm_submit_common(ctx, bases, offset, scalars, scalar_offset, n, out_xyz_device_slots, slot_stride_bytes, ticket);
}
int pcdhip_msm_ticket_wait(pcdhip_ctx* ctx, int ticket, void* other_stream) {
  if (!ctx || ticket < 0 || ticket >= pcdhip_ctx::PIPE_SLOTS || !ctx->pipe_busy[ticket]) return PCDHIP_E_ARG;
  BIND();
  TRY(hipStreamWaitEvent((hipStream_t)other_stream, ctx->pipe_done[ticket], 0));
  ctx->pipe_busy[ticket] = false;  // only once the other stream IS ordered behind the MSM: a failed wait keeps the ticket
  ctx->pipe_partial[ticket] = true;
  return PCDHIP_OK;
}
int pcdhip_msm_collect(pcdhip_ctx* ctx, int ticket, uint64_t* out_xyz) {
  if (!ctx || ticket < 0 || ticket >= pcdhip_ctx::PIPE_SLOTS || !ctx->pipe_busy[ticket] || !out_xyz) return PCDHIP_E_ARG;
  BIND();
  ctx->pipe_busy[ticket] = false;
  TRY(hipEventSynchronize(ctx->pipe_done[ticket]));
  const uint64_t* host = ctx->pipe_host + (size_t)ticket * pcdhip_ctx::PIPE_HOST_WORDS;
  memcpy(out_xyz, host, ctx->pipe_out_bytes[ticket]);
  return (uint32_t)host[pcdhip_ctx::PIPE_HOST_WORDS - 1] ? PCDHIP_E_ARG : PCDHIP_OK;
}

int pcdhip_msm_dev(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset,
                   size_t n, uint64_t* out_xyz) {
  if (!ctx || !bases || !scalars || !out_xyz) return PCDHIP_E_ARG;
  if (!bases->shards.empty()) return PCDHIP_E_ARG;  // sharded bases take host scalars (pcdhip_msm): a pcdhip_buf lives on one device
  if (offset + n > bases->n || scalar_offset + n > scalars->n || n >= (1ull << 31)) return PCDHIP_E_ARG;
  if (scalars->field_id != kCurveFr[bases->curve_id]) return PCDHIP_E_ARG;
  BIND();
  const size_t sw = (size_t)kFieldLimbs[scalars->field_id] * 2;
  return msm_common(ctx, bases, offset, scalars->dptr + scalar_offset * sw, n, out_xyz);
}

int pcdhip_msm_dev_partial(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset,
                           size_t n, uint64_t* out_xyz_device) {
  if (!ctx || !bases || !scalars || !out_xyz_device || !bases->shards.empty()) return PCDHIP_E_ARG;
  if (offset + n > bases->n || scalar_offset + n > scalars->n || n >= (1ull << 31)) return PCDHIP_E_ARG;
  if (scalars->field_id != kCurveFr[bases->curve_id]) return PCDHIP_E_ARG;
  BIND();
  const size_t sw = (size_t)kFieldLimbs[scalars->field_id] * 2;
  return msm_common(ctx, bases, offset, scalars->dptr + scalar_offset * sw, n, out_xyz_device, true);
}

int pcdhip_msm(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars, size_t n, uint64_t* out_xyz) {
  if (!ctx || !bases || (!scalars && n) || !out_xyz) return PCDHIP_E_ARG;
  if (offset + n > bases->n || n >= (1ull << 31)) return PCDHIP_E_ARG;
  if (!bases->shards.empty()) return msm_sharded(ctx, bases, offset, scalars, n, out_xyz);
  BIND();
  const size_t sbytes = n * kFieldLimbs[kCurveFr[bases->curve_id]] * 8;
  TRY(ctx->msm_ws.ensure(WS_SCAL, std::max<size_t>(sbytes, 8)));
  TRY(hipMemcpyAsync(ctx->msm_ws.buf[WS_SCAL], scalars, sbytes, hipMemcpyHostToDevice, ctx->stream));
  return msm_common(ctx, bases, offset, (const uint32_t*)ctx->msm_ws.buf[WS_SCAL], n, out_xyz);
}

int pcdhip_points_sum(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz, size_t n, uint64_t* out_xyz) {
  return points_sum_common(ctx, curve_id, group_id, xyz, n, out_xyz, false);
}
int pcdhip_points_sum_dev(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz_device, size_t n, uint64_t* out_xyz) {
  return points_sum_common(ctx, curve_id, group_id, xyz_device, n, out_xyz, true);
}

int pcdhip_to_affine(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
  if (!ctx || !valid_curve(curve_id) || !valid_group(group_id) || (!xyz && n) || !out_xy) return PCDHIP_E_ARG;
  BIND();
  const GroupEntry& ge = group_entry(curve_id, group_id);
  const size_t ab = (size_t)ge.point_abi_words * 4, jb = ab / 2 * 3;
  TRY(ctx->aux_ws.ensure(AUX_MISC, n * (jb + ab) + 64));
  uint32_t* dj = (uint32_t*)ctx->aux_ws.buf[AUX_MISC];
  uint32_t* da = dj + n * jb / 4;
  TRY(hipMemcpyAsync(dj, xyz, n * jb, hipMemcpyHostToDevice, ctx->stream));
  TRY(ge.to_affine(ctx->stream, dj, (uint32_t)n, da));
  TRY(hipMemcpyAsync(out_xy, da, n * ab, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  if (out_inf) {
    for (size_t i = 0; i < n; i++) {
      const uint64_t* p = out_xy + i * (ab / 8);
      uint64_t o = 0;
      for (size_t k = 0; k < ab / 8; k++) o |= p[k];
      out_inf[i] = (o == 0) ? 1 : 0;
    }
  }
  return PCDHIP_OK;
}

}  // extern "C"
