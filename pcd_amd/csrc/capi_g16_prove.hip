// The Groth16 prover of libpcdhip.so: one device's share of a proof (G16Run), the single-device and the sharded prover, their settings.
#include <chrono>

#include "capi_internal.h"

using namespace pcd;

namespace {
// scalars of `can` (n canonical values of sw words) that are neither 0 nor 1 (grid-stride, one atomic per workgroup: the count is read back by the
// host before the proof's MSMs are launched, so its latency is on the proof's path -- one atomic per wave on one address took 110 us at 2^20)
__global__ void __launch_bounds__(256) count_general_kernel(const uint32_t* __restrict__ can, uint32_t n, int sw, uint32_t* __restrict__ out) {
  __shared__ uint32_t block_count;
  if (threadIdx.x == 0) block_count = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t* p = can + (size_t)i * sw;
    uint32_t hi = 0;
    for (int k = 1; k < sw; k++) hi |= p[k];
    mine += (hi != 0 || p[0] > 1u) ? 1u : 0u;
  }
  if (mine) atomicAdd(&block_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && block_count) atomicAdd(out, block_count);
}
// One device's share of a Groth16 proof: the scalar vectors (assignment z followed by the tail [r, s, -rs, 1], canonical words,
// and their s / r multiples), the MSMs over an entry range of the device's queries, their results.  An ordinary context runs one
// of these over the whole key; a multi-device context one per device over that device's ranges.
struct G16Run {
  pcdhip_ctx* ctx;            // the device's context
  const pcdhip_g16_pk* pk;    // the device's key (whole queries, or this device's shard)
  int cid = 0;
  size_t m = 0, sw = 0, sb = 0, j1 = 0, j2 = 0;
  uint32_t *z_dev = nullptr, *z_can = nullptr, *sz_can = nullptr, *rz_can = nullptr, *rs_dev = nullptr, *t1 = nullptr, *h_can = nullptr;
  uint32_t *msm_g1 = nullptr, *msm_g2 = nullptr, *mul_scratch = nullptr, *proof_dev = nullptr;
  struct Job { const GroupEntry* ge; MsmBasesView bv; const uint32_t* sc; uint32_t n; uint32_t* out; int tslot; const uint32_t* k; uint32_t* kout; int share; };
  static constexpr int SHARE_B = 4;   // Job::share = role (MSM_SHARE_*) | SHARE_B: the sort shared by the two B MSMs (g16_share_b)
  Job jobs[6];
  int nj = 0;
  bool use_lane = false;      // the jobs' accumulate kernels run one after the other on the context's lane (pcdhip_groth16_set_schedule 2)
  bool sparse = false;        // the assignment MSMs take the key's sparse-window copies (decide_sparse)
  uint32_t* general_dev = nullptr;
  uint32_t* slot(int i) const { return (uint32_t*)((char*)msm_g1 + (size_t)i * j1); }
  size_t partial_bytes() const { return 6 * j1 + j2; }  // msm_g1 (six slots) and msm_g2 are contiguous

  // buffers, z -> device image and canonical words (plain, times s, times r), the scalar tails; ends with g16_ready recorded
  // (need_scaled: the folded assembly multiplies every scalar by s / r -- the chained form does not read those copies, 2 n products less)
  int prepare(const uint64_t* z, const uint64_t* r_mont, const uint64_t* s_mont, size_t n_dom, bool need_scaled = true) {
    BIND();
    cid = pk->curve_id;
    const FieldEntry& fe = field_entry(kCurveFr[cid]);
    m = pk->num_vars;
    sw = (size_t)fe.abi_words;  // words of a canonical scalar == words of an ABI element
    sb = sw * 4;
    hipStream_t st = ctx->stream;
    TRY(ctx->aux_ws.ensure(AUX_Z, m * fe.words * 4));
    TRY(ctx->aux_ws.ensure(AUX_SCAL, m * sb));
    TRY(ctx->aux_ws.ensure(AUX_Z_CANON, 3 * (m + 4) * sb + 2 * sb + 64));
    TRY(ctx->aux_ws.ensure(AUX_H_CANON, n_dom * sb));
    z_dev = (uint32_t*)ctx->aux_ws.buf[AUX_Z];
    uint32_t* z_abi = (uint32_t*)ctx->aux_ws.buf[AUX_SCAL];
    z_can = (uint32_t*)ctx->aux_ws.buf[AUX_Z_CANON];
    sz_can = z_can + (m + 4) * sw;
    rz_can = sz_can + (m + 4) * sw;
    rs_dev = rz_can + (m + 4) * sw;  // r, s (C-ABI Montgomery)
    general_dev = rs_dev + 2 * sw;   // one word: the count of general scalars (decide_sparse)
    h_can = (uint32_t*)ctx->aux_ws.buf[AUX_H_CANON];
    TRY(hipMemcpyAsync(z_abi, z, m * sb, hipMemcpyHostToDevice, st));
    TRY(hipMemcpyAsync(rs_dev, r_mont, sb, hipMemcpyHostToDevice, st));
    TRY(hipMemcpyAsync(rs_dev + sw, s_mont, sb, hipMemcpyHostToDevice, st));
    TRY(fe.convert(st, z_abi, z_dev, (uint32_t)m, 0));
    TRY(fe.scale_canon(st, z_dev, nullptr, z_can, (uint32_t)m, 1));
    if (need_scaled) {
      TRY(fe.scale_canon(st, z_dev, rs_dev + sw, sz_can, (uint32_t)m, 1));
      TRY(fe.scale_canon(st, z_dev, rs_dev, rz_can, (uint32_t)m, 1));
    }
    const GroupEntry& g1 = group_entry(cid, 1);
    const GroupEntry& g2 = group_entry(cid, 2);
    j1 = (size_t)g1.point_words / 2 * 3 * 4;
    j2 = (size_t)g2.point_words / 2 * 3 * 4;
    const CurveEntry& ce = curve_entry(cid);
    TRY(ctx->aux_ws.ensure(AUX_G16, 6 * j1 + j2 + 6 * 400 * j1 + ce.proof_abi_bytes + 256));  // (400 Jacobian slots per one-point product: inst_g16.hip)
    char* gbase = (char*)ctx->aux_ws.buf[AUX_G16];
    msm_g1 = (uint32_t*)gbase;  // h, l', A, s*A, r*B_1, B_1
    msm_g2 = (uint32_t*)(gbase + 6 * j1);
    mul_scratch = (uint32_t*)(gbase + 6 * j1 + j2);
    proof_dev = (uint32_t*)(gbase + 6 * j1 + j2 + 6 * 400 * j1);
    t1 = z_can + m * sw;  // [r, s, -rs, 1] canonical
    TRY(ce.prepare_scalars(st, rs_dev, t1, sz_can + m * sw, rz_can + m * sw));
    { int rc = ensure_side_streams(ctx); if (rc) return rc; }
    if (pipe_pending(ctx)) return PCDHIP_E_ARG;  // submitted MSMs still own side-stream workspaces: collect them first
    TRY(hipEventRecord(ctx->g16_ready, st));  // the scalars z || t (and their scaled copies) are ready
    if (!ctx->g16_share.ready) TRY(hipEventCreateWithFlags(&ctx->g16_share.ready, hipEventDisableTiming));
    if (!ctx->g16_share_b.ready) TRY(hipEventCreateWithFlags(&ctx->g16_share_b.ready, hipEventDisableTiming));
    ctx->g16_share.valid = false;
    ctx->g16_share_b.valid = false;
    nj = 0;
    use_lane = ctx->g16_schedule == 2 && ctx->lane.stream;
    return PCDHIP_OK;
  }
  // Which copies the four assignment MSMs run on: the sparse-window ones when at most an eighth of the assignment is general (neither 0 nor 1).
  // One small kernel over the canonical scalars and a 4-byte read-back: the only point where pcdhip_groth16_prove waits for the device before
  // its last launch (the upload is done by then; everything behind it is queued within 0.4 ms, profiles/r05_prove_host_enqueue.txt).
  int decide_sparse(bool folded) {
    sparse = false;
    ctx->g16_last_sparse = 0; ctx->g16_last_general = 0;
    if (folded || !pk->a_sparse) return PCDHIP_OK;   // (the folded form multiplies every scalar by s / r: nothing stays 0 / 1 but the zeros)
    BIND();
    hipStream_t st = ctx->stream;
    TRY(hipMemsetAsync(general_dev, 0, 4, st));
    hipLaunchKernelGGL(count_general_kernel, dim3((unsigned)std::min<size_t>((m + 255) / 256, 1024)), dim3(256), 0, st, z_can, (uint32_t)m, (int)sw, general_dev);
    // (a page-locked word and an event of its own instead of a pageable copy + a synchronisation of the whole stream -- the host
    //  waits for exactly the count kernel and its 4-byte copy, whatever else a caller has queued behind them on this stream)
    if (!ctx->count_host) TRY(hipHostMalloc((void**)&ctx->count_host, 64, hipHostMallocDefault));
    if (!ctx->count_ev) TRY(hipEventCreateWithFlags(&ctx->count_ev, hipEventDisableTiming));
    TRY(hipMemcpyAsync(ctx->count_host, general_dev, 4, hipMemcpyDeviceToHost, st));
    TRY(hipEventRecord(ctx->count_ev, st));
    TRY(hipEventSynchronize(ctx->count_ev));
    const uint32_t general = *(volatile uint32_t*)ctx->count_host;
    ctx->g16_last_general = general;
    sparse = (uint64_t)general * 8 <= m;
    ctx->g16_last_sparse = sparse ? 1 : 0;
    return PCDHIP_OK;
  }
  // the s z / r z copies of the folded form, when prepare() was told to leave them out (the form is chosen after the count)
  int scale_for_fold() {
    BIND();
    const FieldEntry& fe = field_entry(kCurveFr[cid]);
    hipStream_t st = ctx->stream;
    TRY(fe.scale_canon(st, z_dev, rs_dev + sw, sz_can, (uint32_t)m, 1));
    TRY(fe.scale_canon(st, z_dev, rs_dev, rz_can, (uint32_t)m, 1));
    TRY(hipEventRecord(ctx->g16_ready, st));
    return PCDHIP_OK;
  }
  int launch(int k, hipEvent_t after) {
    BIND();
    const CurveEntry& ce = curve_entry(cid);
    hipStream_t sk = ctx->g16_streams[k];
    TRY(hipStreamWaitEvent(sk, after, 0));
    TRY(hipEventRecord(ctx->g16_begin[k], sk));
    // (schedule 2: the accumulation goes to the lane, in the order the jobs are launched)
    ctx->g16_ws[k].lane = use_lane ? &ctx->lane : nullptr;
    const hipError_t me = jobs[k].ge->msm(ctx->g16_ws[k], sk, jobs[k].bv, jobs[k].sc, jobs[k].n, jobs[k].out, ctx->msm_c, ctx->msm_chunk, ctx->msm_sort, nullptr,
                        (jobs[k].share & 3) ? ((jobs[k].share & SHARE_B) ? &ctx->g16_share_b : &ctx->g16_share) : nullptr, jobs[k].share & 3);
    ctx->g16_ws[k].lane = nullptr;
    TRY(me);
    if (jobs[k].k) TRY(ce.scale_g1(sk, jobs[k].out, jobs[k].k, mul_scratch + (size_t)k * 400 * (j1 / 4), jobs[k].kout));
    TRY(hipEventRecord(ctx->g16_end[k], sk));
    static const bool serial = getenv("PCDHIP_G16_SERIAL") != nullptr;  // developer knob: every MSM of a proof with the device to itself (kernel traces)
    if (serial) TRY(hipDeviceSynchronize());
    return PCDHIP_OK;
  }
  // The MSMs that take the assignment (l', A, B_1 on G1; B on G2) over the entries [lo, lo + cnt) of z || t, which are the
  // entries [0, cnt) of this device's queries.  a', b1', b2', l' are indexed alike and take the same scalars: the first job sorts, the
  // others reuse its list.  The two variable-base products of the assembly, s*A and r*B_1, are either one-lane products queued right
  // behind the A / B_1 MSMs on their high-priority streams (whole-key runs only), or two more MSMs over the same bases with every
  // scalar scaled by s / r (`folded`; the form that also adds up across devices).
  int launch_assignment(size_t lo, size_t cnt, bool folded, hipEvent_t after = nullptr) {
    const GroupEntry& g1 = group_entry(cid, 1);
    const GroupEntry& g2 = group_entry(cid, 2);
    const int PRODUCE = MSM_SHARE_PRODUCE, CONSUME = MSM_SHARE_CONSUME, NONE = MSM_SHARE_NONE;
    const uint32_t n = (uint32_t)cnt;
    const uint32_t *zc = z_can + lo * sw, *szc = sz_can + lo * sw, *rzc = rz_can + lo * sw;
    // Which MSMs share a sort.  The a / b queries of a real key are full of points at infinity (a variable that no row of A / B mentions),
    // and an MSM that sorts for itself leaves their entries out of its bucket lists (MsmBasesView::inf_bits).  A sort that is SHARED must
    // keep every entry its consumers need: the list made for A and l' drops nothing (views without the bitmap); the two B MSMs, which flag
    // the same entries, get a sort of their own when enough of them are infinite to pay for it (a sort is ~15 % of a G1 MSM, ~5 % of a G2
    // one; the accumulations shrink by the infinite fraction).
    auto plain = [](MsmBasesView v) { v.inf_bits = nullptr; return v; };
    const MsmBasesView va = (sparse ? pk->a_sparse : pk->a_query)->view(0), vb1 = (sparse ? pk->b_g1_sparse : pk->b_g1_query)->view(0),
                       vb2 = (sparse ? pk->b_g2_sparse : pk->b_g2_query)->view(0), vl = (sparse ? pk->l_sparse : pk->l_query)->view(0);
    const bool sparse_b = pk->b_inf_count * 16 > cnt;
    if (folded) {
      // (A leaves the shared list for a sort of its own when enough of its entries are infinite AND the MSM is large: at 2^16 the sort costs
      //  what the shorter accumulation saves)
      const bool a_alone = pk->a_inf_count * 16 > cnt && cnt >= ((size_t)1 << 17);   // (measured, folded form: 298-bit 2^20 neutral, 753-bit 2^20 185 -> 180 ms)
      if (sparse_b) {
        jobs[nj++] = {&g2, vb2, zc, n, msm_g2, 5, nullptr, nullptr, NONE};                                   // B (heaviest: high priority), its own sort
        if (a_alone) jobs[nj++] = {&g1, va, zc, n, slot(2), 3, nullptr, nullptr, NONE};                      // A
        else jobs[nj++] = {&g1, plain(va), zc, n, slot(2), 3, nullptr, nullptr, PRODUCE};
      } else {
        jobs[nj++] = {&g2, plain(vb2), zc, n, msm_g2, 5, nullptr, nullptr, PRODUCE};                         // B
        if (a_alone) jobs[nj++] = {&g1, va, zc, n, slot(2), 3, nullptr, nullptr, NONE};                      // A
        else jobs[nj++] = {&g1, plain(va), zc, n, slot(2), 3, nullptr, nullptr, CONSUME};
      }
      jobs[nj++] = {&g1, va, szc, n, slot(3), 3, nullptr, nullptr, NONE};                                    // s * A
      jobs[nj++] = {&g1, vb1, rzc, n, slot(4), 4, nullptr, nullptr, NONE};                                   // r * B_1
      jobs[nj++] = {&g1, plain(vl), zc, n, slot(1), 2, nullptr, nullptr, (sparse_b && a_alone) ? NONE : CONSUME};   // l' (with -rs delta)
    } else {
      // (A sorts for itself when enough of its entries are infinite -- l' then does too: a sort is HBM and atomics and overlaps the other
      //  MSMs' multiply-adds, the accumulation it shortens does not; measured on the bench's 298-bit main proof: 17.2 -> 17.0 ms)
      const bool sparse_a = pk->a_inf_count * 16 > cnt;
      if (sparse_a) jobs[nj++] = {&g1, va, zc, n, slot(2), 3, t1 + sw, slot(3), NONE};                       // A, then s * A
      else jobs[nj++] = {&g1, plain(va), zc, n, slot(2), 3, t1 + sw, slot(3), PRODUCE};
      if (sparse_b && pk->b_inf_same) {
        jobs[nj++] = {&g1, vb1, zc, n, slot(5), 4, t1, slot(4), PRODUCE | SHARE_B};                          // B_1, then r * B_1
        // (b_g1 and b_g2 flag the same entries -- compared byte for byte at upload -- so B names B_1's bitmap: the shared list's identity,
        //  which msm_run checks before it consumes a filtered list)
        MsmBasesView vb2s = vb2;
        vb2s.inf_bits = vb1.inf_bits;
        jobs[nj++] = {&g2, vb2s, zc, n, msm_g2, 5, nullptr, nullptr, CONSUME | SHARE_B};                     // B
      } else if (sparse_b) {
        jobs[nj++] = {&g1, vb1, zc, n, slot(5), 4, t1, slot(4), NONE};
        jobs[nj++] = {&g2, vb2, zc, n, msm_g2, 5, nullptr, nullptr, NONE};
      } else {   // (the full list: made by A, or by B_1 when A sorts for itself)
        jobs[nj++] = {&g1, plain(vb1), zc, n, slot(5), 4, t1, slot(4), sparse_a ? PRODUCE : CONSUME};
        jobs[nj++] = {&g2, plain(vb2), zc, n, msm_g2, 5, nullptr, nullptr, CONSUME};
      }
      jobs[nj++] = {&g1, plain(vl), zc, n, slot(1), 2, nullptr, nullptr, (sparse_a && sparse_b) ? NONE : CONSUME};   // l'
    }
    // (round 5's diagnosis of what a proof waits for left jobs out here behind an environment variable -- profiles/r05_witness_like_critical_path.txt;
    //  a switch that makes proofs wrong does not stay in the library)
    for (int k = 0; k < nj; k++) { int rc = launch(k, after ? after : ctx->g16_ready); if (rc) return rc; }
    return PCDHIP_OK;
  }
  // ... behind `gate`: with the lane only the accumulations wait for it (the sorts start at once), otherwise the MSMs as a whole
  int launch_assignment_gated(size_t lo, size_t cnt, bool folded, hipEvent_t gate) {
    if (!use_lane) return launch_assignment(lo, cnt, folded, gate);
    BIND();
    TRY(hipStreamWaitEvent(ctx->lane.stream, gate, 0));
    return launch_assignment(lo, cnt, folded);
  }
  // the h MSM over the entries [hlo, hlo + cnt) of h (entries [0, cnt) of this device's h query), once `after` has fired
  int launch_h(size_t hlo, size_t cnt, hipEvent_t after) {
    const GroupEntry& g1 = group_entry(cid, 1);
    jobs[nj] = {&g1, pk->h_query->view(0), h_can + hlo * sw, (uint32_t)cnt, slot(0), 1, nullptr, nullptr, MSM_SHARE_NONE};
    return launch(nj++, after);
  }
  // the context's stream waits for every job
  int join() {
    BIND();
    for (int k = 0; k < nj; k++) TRY(hipStreamWaitEvent(ctx->stream, ctx->g16_end[k], 0));
    return PCDHIP_OK;
  }
};

int finish_proof(pcdhip_ctx* ctx, int cid, const uint32_t* proof_dev, uint64_t* proof_out, uint8_t* inf_out) {
  const GroupEntry& g1 = group_entry(cid, 1);
  const GroupEntry& g2 = group_entry(cid, 2);
  TRY(hipMemcpyAsync(proof_out, proof_dev, curve_entry(cid).proof_abi_bytes, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  if (inf_out) {
    const size_t a1 = (size_t)g1.point_abi_words * 4, a2 = (size_t)g2.point_abi_words * 4;
    const size_t offs[3] = {0, a1 / 8, (a1 + a2) / 8}, lens[3] = {a1 / 8, a2 / 8, a1 / 8};
    for (int i = 0; i < 3; i++) {
      uint64_t o = 0;
      for (size_t k = 0; k < lens[i]; k++) o |= proof_out[offs[i] + k];
      inf_out[i] = (o == 0) ? 1 : 0;
    }
  }
  return PCDHIP_OK;
}

// Where a proof's constraint matrices come from, as both provers use it: the caller's (A, B, C), or the ones resident with the key
// (`pk`: the whole key, or device 0's shard).  The rows and the domain are picked before anything is queued; the three device matrices
// when the witness map is about to be (a caller's matrices are uploaded through staging slots that prepare() has just used, so behind a
// synchronisation of the context's stream).
struct R1csSource {
  const pcdhip_g16_pk* pk;
  const pcdhip_csr *A, *B, *C;
  uint32_t rows = 0;
  Dom dom;
  int pick(int fr, size_t ni) {
    if (A && B && C) rows = (uint32_t)A->num_rows;
    else if (!A && !B && !C && pk->r1cs_dev) rows = pk->rows;
    else return PCDHIP_E_ARG;
    return pick_domain(fr, (size_t)rows + ni, &dom);
  }
  int matrices(pcdhip_ctx* ctx, const FieldEntry& fe, size_t m, DevCsr mats[3]) const {
    if (A && B && C) { TRY(hipStreamSynchronize(ctx->stream)); return upload_three(ctx, A, B, C, fe, m, mats); }  // (staging slot AUX_SCAL is reused)
    for (int k = 0; k < 3; k++) mats[k] = pk->mats[k];
    return PCDHIP_OK;
  }
};
// A proof over a key sharded across the devices of the context (BASELINE configs[4]: the merge node's MSMs on all GPUs).  Every
// device gets z and runs the five assignment MSMs over its entry range with the two assembly products folded in (partial sums add
// up across devices; one-lane products of partial results would not); device 0 computes h and hands each device its slice over
// xGMI; the partial results (six G1 points and one G2 point per device) travel to device 0, one lane per MSM sums them, and the
// ordinary assembly kernel finishes.  No host synchronisation until the proof is read back.
int prove_sharded_impl(pcdhip_ctx* ctx, const pcdhip_g16_pk* pk, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, const uint64_t* z,
                       const uint64_t* r_mont, const uint64_t* s_mont, uint64_t* proof_out, uint8_t* inf_out) {
  const size_t G = pk->shards.size();
  if (ctx->peers.size() != G) return PCDHIP_E_ARG;
  ctx->g16_last_sparse = 0; ctx->g16_last_general = 0;   // (a sharded proof folds the assembly products in: it never counts, never takes a second layout)
  const int cid = pk->curve_id, fr = kCurveFr[cid];
  const FieldEntry& fe = field_entry(fr);
  const size_t m = pk->num_vars, ni = pk->num_inputs;
  R1csSource r1cs{pk->shards[0], A, B, C};
  int rc = r1cs.pick(fr, ni);
  if (rc) return rc;
  const uint32_t rows = r1cs.rows;
  const Dom& dom = r1cs.dom;
  const size_t n = dom.n, hl = std::min<size_t>(pk->h_len, n);
  BIND();
  EventSet<3> ev;
  TRY(ev.create());
  TRY(hipEventRecord(ev[0], ctx->stream));
  const bool split3 = G >= 3 && !(A && B && C) && ctx->wm_split && pk->shards[1]->r1cs_dev && pk->shards[2]->r1cs_dev &&
                      pk->shards[1]->rows == rows && pk->shards[2]->rows == rows;
  // (pcdhip_groth16_set_schedule 1, off by default: measured slower) a device that carries a chain of the witness map starts its MSMs only
  // when that chain is through
  const bool map_first = ctx->g16_schedule == 1 || ctx->g16_schedule == 2;  // (2: only the accumulate lane of such a device waits for its chain)
  auto carries_chain = [&](size_t g) { return g == 0 || (split3 && g <= 2); };
  std::vector<G16Run> runs(G);
  for (size_t g = 0; g < G; g++) {
    runs[g].ctx = ctx->peers[g];
    runs[g].pk = pk->shards[g];
    ctx->peers[g]->msm_sort = ctx->msm_sort;
    rc = runs[g].prepare(z, r_mont, s_mont, n);
    if (rc) return rc;
    if (map_first && carries_chain(g)) continue;
    rc = runs[g].launch_assignment(pk->lo[g], pk->lo[g + 1] - pk->lo[g], true);
    if (rc) return rc;
  }
  // h on device 0 while the MSMs above run everywhere
  BIND();
  DevCsr mats[3];
  rc = r1cs.matrices(ctx, fe, m, mats);
  if (rc) return rc;
  if (split3) {
    // chains b and c on devices 1 and 2 (their z is resident since prepare()), each into its own AUX_A, then device to device into
    // device 0's AUX_B / AUX_C; chain a on device 0 meanwhile; the pointwise step and the last transform on device 0
    const size_t vb = (size_t)dom.n * fe.words * 4;
    TRY(ctx->aux_ws.ensure(AUX_B, vb));
    TRY(ctx->aux_ws.ensure(AUX_C, vb));
    for (size_t g = 1; g <= 2; g++) {
      pcdhip_ctx* Cg = ctx->peers[g];
      TRY(hipSetDevice(Cg->device));
      rc = witness_chain_dev(Cg, fr, pk->shards[g]->mats[g], (int)g, runs[g].z_dev, ni, dom, AUX_A);
      if (rc) return rc;
      TRY(hipMemcpyPeerAsync(ctx->aux_ws.buf[g == 1 ? AUX_B : AUX_C], ctx->device, Cg->aux_ws.buf[AUX_A], Cg->device, vb, Cg->stream));
      if (!Cg->wm_ev) TRY(hipEventCreateWithFlags(&Cg->wm_ev, hipEventDisableTiming));
      TRY(hipEventRecord(Cg->wm_ev, Cg->stream));
      if (map_first) { rc = runs[g].launch_assignment_gated(pk->lo[g], pk->lo[g + 1] - pk->lo[g], true, Cg->wm_ev); if (rc) return rc; }
    }
    BIND();
    rc = witness_chain_dev(ctx, fr, mats[0], 0, runs[0].z_dev, ni, dom, AUX_A);
    if (rc) return rc;
    for (size_t g = 1; g <= 2; g++) TRY(hipStreamWaitEvent(ctx->stream, ctx->peers[g]->wm_ev, 0));
    rc = witness_finish_dev(ctx, fr, dom);
    if (rc) return rc;
  } else {
    Dom dom_used;
    rc = witness_map_dev(ctx, fr, mats, runs[0].z_dev, ni, &dom_used);
    if (rc) return rc;
    if (dom_used.n != dom.n) return PCDHIP_E_ARG;
  }
  TRY(fe.convert(ctx->stream, (const uint32_t*)ctx->aux_ws.buf[AUX_A], runs[0].h_can, (uint32_t)n, 2));
  TRY(hipEventRecord(ev[1], ctx->stream));
  if (map_first) { rc = runs[0].launch_assignment_gated(pk->lo[0], pk->lo[1] - pk->lo[0], true, ev[1]); if (rc) return rc; BIND(); }
  const size_t sw = runs[0].sw, sb = runs[0].sb;
  for (size_t g = 0; g < G; g++) {
    const size_t hlo = std::min(pk->hlo[g], hl), hhi = std::min(pk->hlo[g + 1], hl);
    pcdhip_ctx* Cg = ctx->peers[g];
    hipEvent_t after = ev[1];
    if (g > 0) {  // this device's slice of h, device to device
      TRY(hipSetDevice(Cg->device));
      TRY(hipStreamWaitEvent(Cg->stream, ev[1], 0));
      if (hhi > hlo)
        TRY(hipMemcpyPeerAsync(runs[g].h_can + hlo * sw, Cg->device, runs[0].h_can + hlo * sw, ctx->device, (hhi - hlo) * sb, Cg->stream));
      if (!Cg->xstream_ev) TRY(hipEventCreateWithFlags(&Cg->xstream_ev, hipEventDisableTiming));
      TRY(hipEventRecord(Cg->xstream_ev, Cg->stream));
      after = Cg->xstream_ev;
    }
    rc = runs[g].launch_h(hlo, hhi - hlo, after);
    if (rc) return rc;
  }
  // partial results -> device 0
  const size_t pb = runs[0].partial_bytes(), j1 = runs[0].j1;
  BIND();
  TRY(ctx->aux_ws.ensure(AUX_FB_JAC, (G + 1) * pb + 64));
  char* gather = (char*)ctx->aux_ws.buf[AUX_FB_JAC];  // G partial blocks, then the summed block
  for (size_t g = 0; g < G; g++) {
    pcdhip_ctx* Cg = ctx->peers[g];
    rc = runs[g].join();
    if (rc) return rc;
    TRY(hipSetDevice(Cg->device));
    TRY(hipMemcpyPeerAsync(gather + g * pb, ctx->device, runs[g].msm_g1, Cg->device, pb, Cg->stream));
    if (g > 0) {
      TRY(hipEventRecord(Cg->xstream_ev, Cg->stream));
      TRY(hipSetDevice(ctx->device));
      TRY(hipStreamWaitEvent(ctx->stream, Cg->xstream_ev, 0));
    }
  }
  BIND();
  uint32_t* sum = (uint32_t*)(gather + G * pb);
  TRY(group_entry(cid, 1).jac_sum_parts(ctx->stream, (const uint32_t*)gather, pb / 4, (uint32_t)G, 5, sum));               // h, l', A, s*A, r*B_1
  TRY(group_entry(cid, 2).jac_sum_parts(ctx->stream, (const uint32_t*)(gather + 6 * j1), pb / 4, (uint32_t)G, 1, sum + 6 * j1 / 4));  // B
  TRY(curve_entry(cid).assemble(ctx->stream, sum, sum + 6 * j1 / 4, runs[0].proof_dev));
  TRY(hipEventRecord(ev[2], ctx->stream));
  rc = finish_proof(ctx, cid, runs[0].proof_dev, proof_out, inf_out);
  if (rc) return rc;
  for (size_t g = 1; g < G; g++) { TRY(hipSetDevice(ctx->peers[g]->device)); TRY(hipStreamSynchronize(ctx->peers[g]->stream)); }
  BIND();
  for (int k = 0; k < 7; k++) ctx->g16_ms[k] = 0;
  (void)hipEventElapsedTime(&ctx->g16_ms[0], ev[0], ev[1]);
  (void)hipEventElapsedTime(&ctx->g16_ms[7], ev[0], ev[2]);
  return PCDHIP_OK;
}
int prove_sharded(pcdhip_ctx* ctx, const pcdhip_g16_pk* pk, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, const uint64_t* z,
                  const uint64_t* r_mont, const uint64_t* s_mont, uint64_t* proof_out, uint8_t* inf_out) {
  const int rc = prove_sharded_impl(ctx, pk, A, B, C, z, r_mont, s_mont, proof_out, inf_out);
  if (rc) drain_peers(ctx);  // no device is left reading the caller's z / r / s, or writing into this call's buffers
  return rc;
}
}  // namespace

extern "C" {

int pcdhip_groth16_set_assembly(pcdhip_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return PCDHIP_E_ARG;
  ctx->g16_assembly = mode;
  return PCDHIP_OK;
}
int pcdhip_groth16_set_sparse_window(pcdhip_ctx* ctx, int bits) {
  if (!ctx || bits < -1 || (bits > 0 && (bits < 6 || bits > 22))) return PCDHIP_E_ARG;
  ctx->g16_sparse_window = bits;
  return PCDHIP_OK;
}
int pcdhip_groth16_last_plan(pcdhip_ctx* ctx, uint32_t out[2]) {
  if (!ctx || !out) return PCDHIP_E_ARG;
  out[0] = (uint32_t)ctx->g16_last_sparse; out[1] = ctx->g16_last_general;
  return PCDHIP_OK;
}
int pcdhip_groth16_set_schedule(pcdhip_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return PCDHIP_E_ARG;
  if (pipe_pending(ctx)) return PCDHIP_E_ARG;
  std::vector<pcdhip_ctx*> all = ctx->peers.empty() ? std::vector<pcdhip_ctx*>{ctx} : ctx->peers;
  int first = PCDHIP_OK;
  for (pcdhip_ctx* p : all) {
    if (p->g16_schedule == mode) continue;
    p->g16_schedule = mode;
    const int rc = drop_side_streams(p, false);  // (their priorities depend on the schedule)
    if (rc && !first) first = rc;                // (every peer gets the new schedule before the first failure is reported: ADVICE r05)
  }
  return first;
}
int pcdhip_set_lane_reserve(pcdhip_ctx* ctx, int cus) {
  if (!ctx || cus < -1 || cus > 128) return PCDHIP_E_ARG;
  if (pipe_pending(ctx)) return PCDHIP_E_ARG;
  std::vector<pcdhip_ctx*> all = ctx->peers.empty() ? std::vector<pcdhip_ctx*>{ctx} : ctx->peers;
  int first = PCDHIP_OK;
  for (pcdhip_ctx* p : all) {
    if (p->lane_reserve == cus) continue;
    p->lane_reserve = cus;
    const int rc = drop_side_streams(p, false);
    if (rc && !first) first = rc;
  }
  return first;
}
int pcdhip_groth16_set_witness_split(pcdhip_ctx* ctx, int on) {
  if (!ctx) return PCDHIP_E_ARG;
  ctx->wm_split = on != 0;
  return PCDHIP_OK;
}

int pcdhip_groth16_prove(pcdhip_ctx* ctx, const pcdhip_g16_pk* pk, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C,
                         const uint64_t* z, const uint64_t* r_mont, const uint64_t* s_mont, uint64_t* proof_out, uint8_t* inf_out) {
  return guarded([&]() -> int {
  if (!ctx || !pk || !z || !r_mont || !s_mont || !proof_out) return PCDHIP_E_ARG;
  // (r + q would prove as r does -- Fp::from_abi reduces what it is given: a second encoding of the blinding factors is refused, not served)
  if (!scalars_reduced(kCurveFr[pk->curve_id], r_mont, 1) || !scalars_reduced(kCurveFr[pk->curve_id], s_mont, 1)) return PCDHIP_E_ARG;
  if (A && B && C) { const pcdhip_csr* ms[3] = {A, B, C}; for (int k = 0; k < 3; k++) { int v = validate_csr(ms[k], pk->num_vars); if (v) return v; } }
  if (pipe_pending(ctx)) return PCDHIP_E_ARG;  // submitted MSMs still own side-stream workspaces: collect them first (before anything is queued)
  if (!pk->shards.empty()) return prove_sharded(ctx, pk, A, B, C, z, r_mont, s_mont, proof_out, inf_out);
  if (!ctx->peers.empty() && ctx->peers.size() > 1) return PCDHIP_E_ARG;  // a whole-key handle belongs to an ordinary context
  BIND();
  const int cid = pk->curve_id, fr = kCurveFr[cid];
  const FieldEntry& fe = field_entry(fr);
  const size_t m = pk->num_vars, ni = pk->num_inputs;
  hipStream_t st = ctx->stream;
  EventSet<8> ev;
  TRY(ev.create());
  TRY(hipEventRecord(ev[0], st));
  static const bool host_time = getenv("PCDHIP_G16_HOSTTIME") != nullptr;  // developer knob: where the HOST is while the proof's launches queue up
  const auto ht0 = std::chrono::steady_clock::now();
  double ht[6] = {0, 0, 0, 0, 0, 0};
  auto stamp = [&](int k) { if (host_time) ht[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ht0).count(); };
  R1csSource r1cs{pk, A, B, C};
  int rc = r1cs.pick(fr, ni);
  if (rc) return rc;
  const Dom& dom = r1cs.dom;
  const size_t n = dom.n;
  // ---- K3/K4/K5 first: the four MSMs that take the assignment (l', A, B_1 on G1; B on G2) do not need h, so they are
  // launched before the witness map and run concurrently with it; the h MSM follows the witness map.  Results stay on the
  // device (device image).
  G16Run run;
  run.ctx = ctx; run.pk = pk;
  // automatic choice of the assembly form: the one-point products cost ~2.5 ms (298-bit) / ~14 ms (753-bit; rounds 1-4: one lane, ~5 / ~75 ms) of
  // latency that hides under the other MSMs of a large proof; two more MSMs cost 2 x 3.5 ms (298-bit, 2^20) / 2 x 1 ms (298-bit, 2^16) / 2 x 8 ms
  // (753-bit, 2^16) of throughput.  Measured (folded vs chained, round 5): 17.6 vs 16.2 ms (298-bit, 2^20), 3.8 vs 5.0 ms (298-bit, 2^16),
  // 202 vs 180 ms (753-bit, 2^20), 29.7 vs 42.0 ms (753-bit, 5 * 2^14).
  const size_t fold_below = fe.abi_words > 12 ? (1u << 18) : (1u << 17);
  bool folded = ctx->g16_assembly == 1 || (ctx->g16_assembly == 0 && m + 4 <= fold_below);
  // (a SMALL proof over the 298-bit fields whose assignment turns out sparse takes the chained form after all: the shorter-window copies make its
  //  four MSMs cheap, and the folded form -- every scalar times s / r -- cannot use them: MNT6-298 at 2^16, witness-like: 3.36 ms folded,
  //  3.08 chained on 12-bit copies; over the 753-bit fields the one-point products (~9 ms) lose: 18.4 against 18.0)
  const bool may_unfold = ctx->g16_assembly == 0 && folded && pk->a_sparse && fe.abi_words <= 12;
  rc = run.prepare(z, r_mont, s_mont, n, folded && !may_unfold);
  if (rc) return rc;
  rc = run.decide_sparse(folded && !may_unfold);
  if (rc) return rc;
  if (may_unfold) {
    if (run.sparse) folded = false;
    else { rc = run.scale_for_fold(); if (rc) return rc; }
  }
  // Schedule (pcdhip_groth16_set_schedule).  Default 0: the four assignment MSMs are launched BEFORE the witness map and run concurrently
  // with it; the h MSM follows the map.  Inside a proof the map's ~30 short dependent kernels wait behind the MSMs' accumulate grids (the 8 ms
  // map of a 753-bit proof ends at 160 ms) and the h MSM runs last -- which LOOKS like a serialised tail, so round 4 built mode 1: the map
  // first with the device to itself, then all five MSMs at once.  Measured on one box (tools/ab_step.py, profiles/r04_ab_prove_schedule.txt):
  // mode 1 is SLOWER -- 23.4 against 20.3 ms (MNT4-298, 2^20), 5.9 against 4.9 ms (MNT6-298, 2^16), 202 against 196.5 ms (MNT4-753, 2^20): the
  // proof is bound by the sum of its MSMs' throughput either way, and mode 1 adds the map's time in front while mode 0 hides it.
  //   Round 5, mode 2: the accumulate LANE.  The map first while the MSMs sort beside it, then the accumulate kernels one after
  // the other on a stream whose CU mask leaves a CU per XCD to everything else, each MSM's fix-up / bucket reduction / one-point product on a
  // hardware queue of its own.  What the measurements say (profiles/r05_*): the accumulate kernels of this proof take 1.29 + 1.08 + 1.66 +
  // 1.67 ms (G1: A, B_1, l', h) + ~3.7 ms (G2) ALONE, the sorts 1.7, fix-ups 1.0, first reduction levels 1.1, the map 1.5, upload and
  // conversions 1.1 -- 15 .. 16 ms of work that all wants the same multiply-add issue slots, and mode 0 takes 15.7 .. 16.0 ms: the concurrency
  // round 4's timeline made look destructive is within a few per cent of the sum of the parts.  The lane cannot beat that sum, and pays for
  // the mask (a masked queue runs an accumulate kernel 15 .. 45 % slower: one CU less in ONE shader engine per XCD unbalances the dispatch) or,
  // unmasked, for its own serialisation (18.0 / 16.4 .. 18.4 ms).  Mode 0 stays the default; what round 5 gained came from doing less work.
  const bool map_first = ctx->g16_schedule >= 1;
  stamp(0);
  if (!map_first) { rc = run.launch_assignment(0, m + 4, folded); if (rc) return rc; }
  stamp(1);
  // ---- K1: h, on the context's stream
  DevCsr mats[3];
  rc = r1cs.matrices(ctx, fe, m, mats);
  if (rc) return rc;
  Dom dom_used;
  rc = witness_map_dev(ctx, fr, mats, run.z_dev, ni, &dom_used);
  if (rc) return rc;
  if (dom_used.n != dom.n) return PCDHIP_E_ARG;
  TRY(fe.convert(st, (const uint32_t*)ctx->aux_ws.buf[AUX_A], run.h_can, (uint32_t)n, 2));
  TRY(hipEventRecord(ev[1], st));
  stamp(2);
  // (round 5 also tried the map's launches merely ENQUEUED first with the h MSM right behind it and the assignment MSMs after, nothing
  //  gated -- the critical path of a proof over a witness-like assignment is upload -> map -> h MSM: slower everywhere, 11.2 against 8.0 ms
  //  there, 19.0 against 15.8 ms on a uniform assignment, because the G2 MSM and the one-point products then start last; and mode 0 with only
  //  the map's launches moved ahead of the MSMs' in host order: no difference beyond noise on either assignment, as in round 4:
  //  profiles/r05_ab_prove_schedule3.txt)
  if (map_first) { rc = run.launch_assignment_gated(0, m + 4, folded, ev[1]); if (rc) return rc; }  // (lane: no accumulation under the map; the sorts start at once)
  rc = run.launch_h(0, std::min<size_t>(pk->h_query->n, n), ev[1]);
  if (rc) return rc;
  stamp(3);
  rc = run.join();
  if (rc) return rc;
  TRY(hipEventRecord(ev[6], st));
  // assembly: three additions and three affine conversions (writes the proof in the C-ABI image)
  TRY(curve_entry(cid).assemble(st, run.msm_g1, run.msm_g2, run.proof_dev));
  TRY(hipEventRecord(ev[7], st));
  stamp(4);
  rc = finish_proof(ctx, cid, run.proof_dev, proof_out, inf_out);
  if (rc) return rc;
  stamp(5);
  if (host_time)
    fprintf(stderr, "pcdhip prove host ms: prepared %.3f, assignment MSMs enqueued %.3f, map enqueued %.3f, h enqueued %.3f, all enqueued %.3f, done %.3f\n",
            ht[0], ht[1], ht[2], ht[3], ht[4], ht[5]);
  // [witness_map, msm_h, msm_l, msm_a (A and s*A), msm_b_g1 (B_1 and r*B_1), msm_b_g2 (each on its own stream: they
  //  overlap), assembly, total]
  (void)hipEventElapsedTime(&ctx->g16_ms[0], ev[0], ev[1]);
  for (int k = 1; k <= 5; k++) ctx->g16_ms[k] = 0;
  for (int k = 0; k < run.nj; k++) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->g16_begin[k], ctx->g16_end[k]);
    ctx->g16_ms[run.jobs[k].tslot] = std::max(ctx->g16_ms[run.jobs[k].tslot], ms);
  }
  (void)hipEventElapsedTime(&ctx->g16_ms[6], ev[6], ev[7]);
  (void)hipEventElapsedTime(&ctx->g16_ms[7], ev[0], ev[7]);
  return PCDHIP_OK;
  });
}

int pcdhip_groth16_last_timings(pcdhip_ctx* ctx, float out_ms[8]) {
  if (!ctx || !out_ms) return PCDHIP_E_ARG;
  memcpy(out_ms, ctx->g16_ms, sizeof ctx->g16_ms);
  return PCDHIP_OK;
}

}  // extern "C"
