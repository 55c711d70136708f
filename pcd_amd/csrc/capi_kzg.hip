// ------------------------------------------------------------------------------------------------ K7: KZG10 commit and open side
// (poly.hip.h: canonical scalars and trimmed lengths for the commitments' MSMs; division by (X - z), evaluation, linear combination;
//  then the witness MSMs and the pairing check)
#include "capi_internal.h"
#include "msm_short.hip.h"

using namespace pcd;

namespace {
// descriptors | values | tile scratch;  the two quotients of an opening;  everything of one pcdhip_kzg_commit call
// (K13's calls take the slot of pcdhip_kzg_commit: neither runs while the other does, and a slot only ever grows)
enum { AUX_POLY = AUX_FB_OUT + 1, AUX_POLY_Q, AUX_POLY_R, AUX_COMMIT, AUX_OPEN = AUX_COMMIT };

// descriptors of k polynomials of one field (lens[j] <= their buffers' n, below 2^31) -> the field, or -1 when they do not qualify
int poly_descs(const pcdhip_buf* const* polys, const size_t* lens, size_t k, std::vector<PolyDesc>* d, uint64_t* max_len) {
  int f = -1;
  *max_len = 0;
  d->resize(k);
  for (size_t j = 0; j < k; j++) {
    const pcdhip_buf* b = polys[j];
    if (!b || lens[j] > b->n || lens[j] >= (1ull << 31) || (j && b->field_id != f)) return -1;
    f = b->field_id;
    (*d)[j] = {b->dptr, (uint64_t)lens[j]};
    *max_len = std::max<uint64_t>(*max_len, lens[j]);
  }
  return f;
}
// the k values land on the device at *values_dev (ABI Montgomery); with div (k == 1) the quotient goes to q_out as well
int poly_eval_run(pcdhip_ctx* ctx, int f, const std::vector<PolyDesc>& d, uint64_t max_len, const uint64_t* z_mont, uint32_t** values_dev,
                  const PolyDesc* div = nullptr, uint32_t* q_out = nullptr, int q_canonical = 0) {
  const FieldEntry& fe = field_entry(f);
  const size_t k = d.size();
  const size_t db = (k * sizeof(PolyDesc) + 255) & ~(size_t)255, vb = (k * fe.abi_words * 4 + 255) & ~(size_t)255;
  TRY(ctx->aux_ws.ensure(AUX_POLY, db + vb + fe.poly_scratch_words((uint32_t)k, max_len) * 4));
  char* base = (char*)ctx->aux_ws.buf[AUX_POLY];
  TRY(hipMemcpyAsync(base, d.data(), k * sizeof(PolyDesc), hipMemcpyHostToDevice, ctx->stream));
  *values_dev = (uint32_t*)(base + db);
  TRY(fe.poly_eval(ctx->stream, (const PolyDesc*)base, (uint32_t)k, max_len, (const uint32_t*)z_mont, (uint32_t*)(base + db + vb), *values_dev,
                   div, q_out, q_canonical));
  return PCDHIP_OK;
}
// p / (X - z) as canonical scalars in the workspace slot (len - 1 of them), p(z) to the host
int kzg_divide(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, const uint64_t* z_mont, int slot, uint32_t** q_dev, uint64_t* value_mont) {
  const FieldEntry& fe = field_entry(p->field_id);
  TRY(ctx->aux_ws.ensure(slot, std::max<size_t>(len, 1) * fe.abi_words * 4));
  *q_dev = (uint32_t*)ctx->aux_ws.buf[slot];
  const std::vector<PolyDesc> d = {{p->dptr, (uint64_t)len}};
  uint32_t* vals = nullptr;
  int rc = poly_eval_run(ctx, p->field_id, d, len, z_mont, &vals, &d[0], *q_dev, 1);
  if (rc) return rc;
  TRY(hipMemcpyAsync(value_mont, vals, (size_t)fe.abi_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
// the witness MSM over the bases' prefix; an empty quotient gives the point at infinity (Z = 0).  Upstream skips the quotient's
// leading zeros before its MSM: not needed here, a zero scalar drops out of the buckets.
int kzg_witness(pcdhip_ctx* ctx, const pcdhip_bases* bases, const uint32_t* q_dev, size_t n, uint64_t* out_xyz) {
  if (n == 0) {
    memset(out_xyz, 0, (size_t)pcdhip_point_limbs(bases->curve_id, bases->group_id) / 2 * 3 * 8);
    return PCDHIP_OK;
  }
  if (n <= ctx->msm_short_max) return msm_short_common(ctx, bases, 0, q_dev, n, out_xyz);  // pcdhip_msm_set_short: no buckets for a few pairs
  return msm_common(ctx, bases, 0, q_dev, n, out_xyz);
}
// One MSM of a commitment's hiding part, on the context's own stream, its Jacobian result (device image) left at `out`: without buckets
// for a few pairs when pcdhip_msm_set_short allows it (the rule of kzg_witness), through the bucket pipeline otherwise.  Asynchronous;
// the scalars come from poly_commit_scalars and are reduced, so no error word is read.
int commit_hiding_msm(pcdhip_ctx* ctx, const pcdhip_bases* bases, const uint32_t* scalars_dev, size_t n, uint32_t* out) {
  if (n <= ctx->msm_short_max) return msm_short_async(ctx, bases, 0, scalars_dev, n, out);
  const GroupEntry& ge = group_entry(bases->curve_id, bases->group_id);
  const size_t jac_b = (size_t)ge.point_words / 2 * 3 * 4;
  TRY(ctx->msm_ws.ensure(WS_OUT, jac_b + 64));
  uint32_t* out_dev = (uint32_t*)ctx->msm_ws.buf[WS_OUT];
  TRY(ge.msm(ctx->msm_ws, ctx->stream, bases->view(0), scalars_dev, (uint32_t)n, out_dev, ctx->msm_c, ctx->msm_chunk, ctx->msm_sort, nullptr, nullptr,
             MSM_SHARE_NONE));
  TRY(hipMemcpyAsync(out, out_dev, jac_b, hipMemcpyDeviceToDevice, ctx->stream));
  return PCDHIP_OK;
}

struct CommitPlan {            // what pcdhip_kzg_commit has validated, per item
  uint64_t n = 0;              // pairs of the item's MSMs: min(len, cap)
  size_t scal = 0;             // first element of its canonical scalars in the call's scalar area
  int blind = -1, sblind = -1; // descriptor index of the blinding polynomials (-1: none)
  size_t bscal = 0, sbscal = 0;
};
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Everything of the call behind its argument checks.  One scalar area holds the canonical coefficients of all k polynomials and of their
// blinding polynomials, written by ONE launch of poly_commit_scalars on the context's stream; item j's MSMs then run on side stream
// j mod 4 over their slice while the hiding MSMs, a few coefficients each, run on the context's stream.  No host wait before the end: the
// MSMs cover min(len, cap) pairs and the size rule is applied to the trimmed lengths that come back with the results.
// Under pcdhip_msm_set_short the hiding MSMs of at most that many pairs do not queue one behind the other: they are collected into ONE
// msm_short_batch_async (one chain of two or three launches, a wave per MSM) that writes straight into their slots of `res`; only the
// first HIDING_BATCH_MAX of a call, the rest and the longer ones go one at a time through commit_hiding_msm.  ctx->kzg_commit_plan says
// which path ran (pcdhip_kzg_commit_last_plan).
constexpr size_t HIDING_BATCH_MAX = 1024;
int kzg_commit_run(pcdhip_ctx* ctx, const pcdhip_bases* pg, const pcdhip_bases* pgg, const pcdhip_bases* sp, const pcdhip_kzg_commit_item* items,
                   size_t k, const std::vector<CommitPlan>& plan, std::vector<PolyCommitDesc>& descs, size_t scal_elems, uint64_t max_len,
                   uint64_t* comm_xy, uint8_t* comm_inf, uint64_t* shifted_xy, uint8_t* shifted_inf, uint64_t* trimmed_len) {
  const GroupEntry& ge = group_entry(pg->curve_id, 1);
  const FieldEntry& fe = field_entry(kCurveFr[pg->curve_id]);
  const size_t jw = (size_t)ge.point_words / 2 * 3, jac_b = jw * 4, jac_abi_b = (size_t)ge.point_abi_words / 2 * 3 * 4;
  const size_t ab = (size_t)ge.point_abi_words * 4, sw = (size_t)fe.abi_words, nd = descs.size(), slots = 2 * k;
  // descriptors | results: part 0 the large MSMs, part 1 the hiding MSMs, slot 2j item j's plain and 2j + 1 its shifted commitment |
  // their sums | the sums in the C-ABI image | what goes back to the host: affine points, trimmed lengths | scalars
  const size_t o_res = up256(nd * sizeof(PolyCommitDesc)), o_sum = o_res + up256(2 * slots * jac_b), o_abi = o_sum + up256(slots * jac_b);
  const size_t o_back = o_abi + up256(slots * jac_abi_b), back_b = slots * ab + nd * 4, o_scal = o_back + up256(back_b);
  TRY(ctx->aux_ws.ensure(AUX_COMMIT, o_scal + std::max<size_t>(scal_elems, 1) * sw * 4));
  char* base = (char*)ctx->aux_ws.buf[AUX_COMMIT];
  uint32_t* res = (uint32_t*)(base + o_res);
  uint32_t* scal = (uint32_t*)(base + o_scal);
  uint32_t* trimmed_dev = (uint32_t*)(base + o_back + slots * ab);
  for (size_t j = 0; j < k; j++) {
    descs[j].out = scal + plan[j].scal * sw;
    if (plan[j].blind >= 0) descs[plan[j].blind].out = scal + plan[j].bscal * sw;
    if (plan[j].sblind >= 0) descs[plan[j].sblind].out = scal + plan[j].sbscal * sw;
  }
  hipStream_t st = ctx->stream;
  TRY(hipMemcpyAsync(base, descs.data(), nd * sizeof(PolyCommitDesc), hipMemcpyHostToDevice, st));
  TRY(hipMemsetAsync(res, 0, 2 * slots * jac_b, st));  // (all zeros: Z = 0, the identity -- what an item without that part contributes)
  TRY(hipMemsetAsync(trimmed_dev, 0, nd * 4, st));
  TRY(fe.poly_commit_scalars(st, (const PolyCommitDesc*)base, (uint32_t)nd, max_len, trimmed_dev));
  TRY(hipEventRecord(ctx->g16_ready, st));
  bool used[pcdhip_ctx::PIPE_SLOTS] = {};
  uint64_t large = 0;
  for (size_t j = 0; j < k; j++) {
    if (plan[j].n == 0) continue;
    const int s = (int)(j % pcdhip_ctx::PIPE_SLOTS);
    MsmWorkspace& ws = ctx->g16_ws[2 + s];
    hipStream_t sk = ctx->g16_streams[2 + s];
    if (!used[s]) TRY(hipStreamWaitEvent(sk, ctx->g16_ready, 0));
    used[s] = true;
    TRY(ws.ensure(WS_OUT, jac_b + 64));
    uint32_t* out_dev = (uint32_t*)ws.buf[WS_OUT];
    for (int sh = 0; sh < (items[j].shifted ? 2 : 1); sh++) {
      const MsmBasesView bv = sh ? sp->view((size_t)items[j].shifted_offset) : pg->view(0);
      ws.lane = ctx->g16_schedule == 2 && ctx->pipe_lane && ctx->lane.stream ? &ctx->lane : nullptr;
      const hipError_t me = ge.msm(ws, sk, bv, scal + plan[j].scal * sw, (uint32_t)plan[j].n, out_dev, ctx->msm_c, ctx->msm_chunk, ctx->msm_sort,
                                   nullptr, nullptr, MSM_SHARE_NONE);
      ws.lane = nullptr;
      TRY(me);
      large++;
      TRY(hipMemcpyAsync(res + (2 * j + sh) * jw, out_dev, jac_b, hipMemcpyDeviceToDevice, sk));  // (before the workspace is used again)
    }
    TRY(hipEventRecord(ctx->g16_end[2 + s], sk));
  }
  std::vector<MsmShortBatchIn> batch;  // (stays empty under the default pcdhip_msm_set_short(ctx, 0): every length is at least 1)
  uint64_t one_by_one = 0;
  auto hiding = [&](const uint32_t* scalars_dev, uint64_t n, size_t slot) -> int {
    if (n <= ctx->msm_short_max && batch.size() < HIDING_BATCH_MAX) {
      batch.push_back({scalars_dev, 0u, (uint32_t)n, (uint32_t)slot});
      return PCDHIP_OK;
    }
    one_by_one++;
    return commit_hiding_msm(ctx, pgg, scalars_dev, (size_t)n, res + slot * jw);
  };
  for (size_t j = 0; j < k; j++) {
    int rc = PCDHIP_OK;
    if (plan[j].blind >= 0 && items[j].blinding_len) rc = hiding(scal + plan[j].bscal * sw, items[j].blinding_len, slots + 2 * j);
    if (!rc && plan[j].sblind >= 0 && items[j].shifted_blinding_len)
      rc = hiding(scal + plan[j].sbscal * sw, items[j].shifted_blinding_len, slots + 2 * j + 1);
    if (rc) return rc;
  }
  uint32_t chain = 0;
  if (!batch.empty()) {  // (the scalars come from poly_commit_scalars and are reduced: no error word is read)
    int rc = msm_short_batch_async(ctx, pgg, batch.data(), batch.size(), res, jw, nullptr, &chain);
    if (rc) return rc;
  }
  ctx->kzg_commit_plan[0] = large;
  ctx->kzg_commit_plan[1] = batch.size();
  ctx->kzg_commit_plan[2] = one_by_one;
  ctx->kzg_commit_plan[3] = chain;
  for (int s = 0; s < pcdhip_ctx::PIPE_SLOTS; s++) if (used[s]) TRY(hipStreamWaitEvent(st, ctx->g16_end[2 + s], 0));
  TRY(ge.jac_sum_parts(st, res, slots * jw, 2, (uint32_t)slots, (uint32_t*)(base + o_sum)));
  TRY(ge.jac_out(st, (const uint32_t*)(base + o_sum), (uint32_t)slots, (uint32_t*)(base + o_abi)));
  TRY(ge.to_affine(st, (const uint32_t*)(base + o_abi), (uint32_t)slots, (uint32_t*)(base + o_back)));
  std::vector<uint64_t> back((back_b + 7) / 8);
  TRY(hipMemcpyAsync(back.data(), base + o_back, back_b, hipMemcpyDeviceToHost, st));
  TRY(hipStreamSynchronize(st));
  const uint32_t* t = (const uint32_t*)((const char*)back.data() + slots * ab);
  // upstream's TooManyCoefficients / IncorrectDegreeBound, on the trimmed lengths
  for (size_t j = 0; j < k; j++)
    if (t[j] > pg->n || (items[j].shifted && items[j].shifted_offset + t[j] > sp->n)) return PCDHIP_E_ARG;
  const size_t pl = ab / 8;
  auto is_identity = [&](const uint64_t* p) { uint64_t o = 0; for (size_t i = 0; i < pl; i++) o |= p[i]; return o == 0 ? 1 : 0; };
  for (size_t j = 0; j < k; j++) {
    memcpy(comm_xy + j * pl, &back[2 * j * pl], ab);
    comm_inf[j] = (uint8_t)is_identity(&back[2 * j * pl]);
    if (shifted_xy) memcpy(shifted_xy + j * pl, &back[(2 * j + 1) * pl], ab);  // (zeros for an item without a degree bound)
    if (shifted_inf) shifted_inf[j] = items[j].shifted ? (uint8_t)is_identity(&back[(2 * j + 1) * pl]) : 1;
    if (trimmed_len) trimmed_len[j] = t[j];
  }
  return PCDHIP_OK;
}

// ---- K13: a round's openings.  What pcdhip_poly_open_quotients and pcdhip_kzg_batch_open have validated: the parts of the call
// (common.h PolyOpenPart; src / work / q are filled in once the workspace is known), their terms, and where each part of opening o sits
// in the P x (2 + m) table the C ABI speaks of -- [o][0] the combined polynomial, [o][1] R_o, [o][2 + i] the degree-bound term of item i.
struct OpenPlan {
  int field = -1;
  size_t m = 0, P = 0;
  std::vector<PolyOpenPart> parts;
  std::vector<PolyOpenTerm> terms;
  std::vector<int> part_of;        // P x (2 + m): the part's index, -1 when there is none
  std::vector<size_t> slot_of;     // per part: its place in part_of
  std::vector<size_t> work_off;    // per part: first element of its workspace vector ((size_t)-1: none)
  std::vector<size_t> q_off;       // per part: first element of its quotient in one scalar area
  size_t work_elems = 0, q_elems = 0;
  uint64_t max_len = 0;
  bool takes_blinding = false;     // some opening's R_o names a blinding buffer
};
constexpr size_t OPEN_MAX_ITEMS = 1024, OPEN_MAX_OPENINGS = 64, OPEN_MAX_DB = 8;

bool abi_is_zero(const uint64_t* x, size_t limbs) { uint64_t o = 0; for (size_t i = 0; i < limbs; i++) o |= x[i]; return o == 0; }

// -> PCDHIP_OK or PCDHIP_E_ARG; every buffer must be of `field`
int open_plan(const pcdhip_kzg_commit_item* items, size_t m, size_t P, const uint64_t* coeffs, const uint64_t* scoeffs, int field, OpenPlan* pl) {
  if (m > OPEN_MAX_ITEMS || P > OPEN_MAX_OPENINGS) return PCDHIP_E_ARG;
  pl->m = m;
  pl->P = P;
  auto buf_ok = [&](const pcdhip_buf* b, uint64_t len) { return b->field_id == field && len <= b->n && len < (1ull << 31); };
  for (size_t i = 0; i < m; i++) {
    const pcdhip_kzg_commit_item& it = items[i];
    if ((!it.poly && it.len) || (it.poly && !buf_ok(it.poly, it.len))) return PCDHIP_E_ARG;
    if (it.blinding && !buf_ok(it.blinding, it.blinding_len)) return PCDHIP_E_ARG;
    if (it.shifted_blinding && (!it.shifted || !buf_ok(it.shifted_blinding, it.shifted_blinding_len))) return PCDHIP_E_ARG;
  }
  pl->field = field;
  pl->part_of.assign(P * (2 + m), -1);
  const size_t L = (size_t)kFieldLimbs[field];
  std::vector<uint64_t> one(L, 0);
  with_host_field(field, [&](auto f) { decltype(f)::type::one().to_abi((uint32_t*)one.data()); });
  auto coeff_idx = [&](const uint64_t* c, size_t idx) { return memcmp(c, one.data(), L * 8) == 0 ? POLY_OPEN_ONE : (uint32_t)idx; };
  for (size_t o = 0; o < P; o++) {
    bool first = true;
    // a part from the terms [t0, end): dropped when it has none
    auto close_part = [&](size_t t0, size_t slot, uint32_t scale) {
      const size_t nt = pl->terms.size() - t0;
      if (nt == 0) return;
      PolyOpenPart pt = {};
      for (size_t t = t0; t < pl->terms.size(); t++) pt.len = std::max<uint64_t>(pt.len, pl->terms[t].len);
      pt.term_lo = (uint32_t)t0; pt.n_terms = (uint32_t)nt; pt.point = (uint32_t)o; pt.scale = scale;
      pt.first_of_point = first ? 1 : 0;
      first = false;
      const bool own = nt == 1 && pl->terms[t0].coeff == POLY_OPEN_ONE;  // read from its item again: no workspace vector
      pl->work_off.push_back(own ? (size_t)-1 : pl->work_elems);
      if (!own) pl->work_elems += pt.len;
      pl->q_off.push_back(pl->q_elems);
      pl->q_elems += pt.len - 1;
      pl->max_len = std::max(pl->max_len, pt.len);
      pl->part_of[o * (2 + m) + slot] = (int)pl->parts.size();
      pl->slot_of.push_back(o * (2 + m) + slot);
      pl->parts.push_back(pt);
    };
    size_t t0 = pl->terms.size();
    for (size_t i = 0; i < m; i++) {  // the combined polynomial
      const uint64_t* a = coeffs + (o * m + i) * L;
      if (!abi_is_zero(a, L) && items[i].len) pl->terms.push_back({items[i].poly->dptr, items[i].len, coeff_idx(a, o * m + i), 0});
    }
    close_part(t0, 0, POLY_OPEN_ONE);
    t0 = pl->terms.size();
    size_t db = 0;
    for (size_t i = 0; i < m; i++) {  // R_o: both kinds of blinding over the same bases, one polynomial
      const uint64_t* a = coeffs + (o * m + i) * L;
      const uint64_t* s = scoeffs ? scoeffs + (o * m + i) * L : nullptr;
      if (s && !abi_is_zero(s, L) && !items[i].shifted) return PCDHIP_E_ARG;
      if (!abi_is_zero(a, L) && items[i].blinding) {
        pl->takes_blinding = true;
        if (items[i].blinding_len) pl->terms.push_back({items[i].blinding->dptr, items[i].blinding_len, coeff_idx(a, o * m + i), 0});
      }
      if (s && !abi_is_zero(s, L) && items[i].shifted_blinding) {
        pl->takes_blinding = true;
        if (items[i].shifted_blinding_len)
          pl->terms.push_back({items[i].shifted_blinding->dptr, items[i].shifted_blinding_len, coeff_idx(s, (P + o) * m + i), 0});
      }
    }
    close_part(t0, 1, POLY_OPEN_ONE);
    for (size_t i = 0; scoeffs && i < m; i++) {  // the degree-bound terms: the item itself, its quotient scaled in the store
      const uint64_t* s = scoeffs + (o * m + i) * L;
      if (abi_is_zero(s, L)) continue;
      if (++db > OPEN_MAX_DB) return PCDHIP_E_ARG;
      if (!items[i].len) continue;
      t0 = pl->terms.size();
      pl->terms.push_back({items[i].poly->dptr, items[i].len, POLY_OPEN_ONE, 0});
      close_part(t0, 2 + i, coeff_idx(s, (P + o) * m + i));
    }
  }
  return PCDHIP_OK;
}

// The three launches of a plan on the context's stream.  The tables, the values and the scratch of the kernels sit at `base` (device,
// open_tables_bytes(...) bytes); part y's workspace vector at work + work_off[y] elements; q[y] = where its quotient goes.  *values_dev:
// one ABI element per part.  Asynchronous: the host vectors of `pl` are read by the staging copies, which return once they are staged.
size_t open_tables_bytes(const OpenPlan& pl, const FieldEntry& fe, size_t off[6]) {
  const size_t np = pl.parts.size(), eb = (size_t)fe.abi_words * 4;
  off[0] = 0;                                                   // parts
  off[1] = off[0] + up256(np * sizeof(PolyOpenPart));           // terms
  off[2] = off[1] + up256(pl.terms.size() * sizeof(PolyOpenTerm));  // coefficients, then shifted coefficients
  off[3] = off[2] + up256(2 * pl.P * pl.m * eb);                // points
  off[4] = off[3] + up256(pl.P * eb);                           // values
  off[5] = off[4] + up256(np * eb);                             // kernel scratch
  return off[5] + up256(fe.poly_open_scratch_words((uint32_t)np, (uint32_t)pl.P, pl.max_len) * 4);
}
int open_run(pcdhip_ctx* ctx, OpenPlan& pl, char* base, uint32_t* work, uint32_t* const* q, const uint64_t* points, const uint64_t* coeffs,
             const uint64_t* scoeffs, uint32_t** values_dev, uint32_t* launches) {
  const FieldEntry& fe = field_entry(pl.field);
  const size_t np = pl.parts.size(), eb = (size_t)fe.abi_words * 4, sw = (size_t)fe.abi_words;
  size_t off[6];
  open_tables_bytes(pl, fe, off);
  for (size_t y = 0; y < np; y++) {
    PolyOpenPart& pt = pl.parts[y];
    pt.work = pl.work_off[y] == (size_t)-1 ? nullptr : work + pl.work_off[y] * sw;
    pt.src = pt.work ? pt.work : pl.terms[pt.term_lo].p;
    pt.q = q[y];
  }
  hipStream_t st = ctx->stream;
  *values_dev = (uint32_t*)(base + off[4]);
  if (np == 0) { if (launches) *launches = 0; return PCDHIP_OK; }  // (no coefficient anywhere: nothing to divide)
  TRY(hipMemcpyAsync(base + off[0], pl.parts.data(), np * sizeof(PolyOpenPart), hipMemcpyHostToDevice, st));
  TRY(hipMemcpyAsync(base + off[1], pl.terms.data(), pl.terms.size() * sizeof(PolyOpenTerm), hipMemcpyHostToDevice, st));
  TRY(hipMemcpyAsync(base + off[2], coeffs, pl.P * pl.m * eb, hipMemcpyHostToDevice, st));
  if (scoeffs) TRY(hipMemcpyAsync(base + off[2] + pl.P * pl.m * eb, scoeffs, pl.P * pl.m * eb, hipMemcpyHostToDevice, st));
  TRY(hipMemcpyAsync(base + off[3], points, pl.P * eb, hipMemcpyHostToDevice, st));
  TRY(fe.poly_open(st, (const PolyOpenPart*)(base + off[0]), (const PolyOpenTerm*)(base + off[1]), (const uint32_t*)(base + off[2]),
                   (const uint32_t*)(base + off[3]), (uint32_t)np, (uint32_t)pl.P, pl.max_len, (uint32_t*)(base + off[5]), *values_dev, launches));
  return PCDHIP_OK;
}

// Everything of pcdhip_kzg_batch_open behind its argument checks, in the shape of kzg_commit_run: the three launches of the divisions on
// the context's stream, every opening's large MSMs (its combined quotient over powers_of_g, one per degree-bound term over
// shifted_powers_of_g from the term's offset) on the side streams, slot = running index mod 4, the hiding MSMs batched or one at a time
// on the context's stream, one epilogue over OPEN_SLOTS slots per opening, one copy back, ONE wait.
constexpr size_t OPEN_SLOTS = 2 + OPEN_MAX_DB;  // combined, hiding, degree-bound terms; an absent part stays zero: Z = 0, the identity
int kzg_batch_open_run(pcdhip_ctx* ctx, const pcdhip_bases* pg, const pcdhip_bases* pgg, const pcdhip_bases* sp, const pcdhip_kzg_commit_item* items,
                       OpenPlan& pl, const uint64_t* points, const uint64_t* coeffs, const uint64_t* scoeffs, uint64_t* w_xy, uint8_t* w_inf,
                       uint64_t* values_mont, uint64_t* random_v_mont) {
  const GroupEntry& ge = group_entry(pg->curve_id, 1);
  const FieldEntry& fe = field_entry(pl.field);
  const size_t P = pl.P, m = pl.m, np = pl.parts.size(), sw = (size_t)fe.abi_words, eb = sw * 4;
  const size_t jw = (size_t)ge.point_words / 2 * 3, jac_b = jw * 4, jac_abi_b = (size_t)ge.point_abi_words / 2 * 3 * 4, ab = (size_t)ge.point_abi_words * 4;
  size_t off[6];
  // tables and scratch | results, slot-major | their sums | the sums in the C-ABI image | what goes back: P affine points, then the
  // parts' values | workspace vectors | quotient scalars
  const size_t o_res = open_tables_bytes(pl, fe, off), o_sum = o_res + up256(OPEN_SLOTS * P * jac_b), o_abi = o_sum + up256(P * jac_b);
  const size_t o_back = o_abi + up256(P * jac_abi_b), back_b = P * ab + np * eb, o_work = o_back + up256(back_b);
  const size_t o_scal = o_work + up256(std::max<size_t>(pl.work_elems, 1) * eb);
  TRY(ctx->aux_ws.ensure(AUX_OPEN, o_scal + std::max<size_t>(pl.q_elems, 1) * eb));
  char* base = (char*)ctx->aux_ws.buf[AUX_OPEN];
  uint32_t* res = (uint32_t*)(base + o_res);
  uint32_t* scal = (uint32_t*)(base + o_scal);
  std::vector<uint32_t*> q(np);
  for (size_t y = 0; y < np; y++) q[y] = scal + pl.q_off[y] * sw;
  hipStream_t st = ctx->stream;
  TRY(hipMemsetAsync(res, 0, OPEN_SLOTS * P * jac_b, st));
  uint32_t* values_dev = nullptr;
  uint32_t launches = 0;
  int rc = open_run(ctx, pl, base, (uint32_t*)(base + o_work), q.data(), points, coeffs, scoeffs, &values_dev, &launches);
  if (rc) return rc;
  TRY(hipEventRecord(ctx->g16_ready, st));
  bool used[pcdhip_ctx::PIPE_SLOTS] = {};
  uint64_t large = 0, running = 0, one_by_one = 0;
  std::vector<MsmShortBatchIn> batch;
  for (size_t o = 0; o < P; o++) {
    size_t db_slot = 2;
    for (size_t k = 0; k < 2 + m; k++) {
      const int y = pl.part_of[o * (2 + m) + k];
      if (y < 0) continue;
      const uint64_t n = pl.parts[y].len - 1;
      const size_t slot = (k < 2 ? k : db_slot++) * P + o;
      if (n == 0) continue;  // (a constant: no quotient, the identity)
      if (k == 1) {          // the hiding MSM, on the context's stream
        if (n <= ctx->msm_short_max && batch.size() < HIDING_BATCH_MAX) { batch.push_back({q[y], 0u, (uint32_t)n, (uint32_t)slot}); continue; }
        one_by_one++;
        rc = commit_hiding_msm(ctx, pgg, q[y], (size_t)n, res + slot * jw);
        if (rc) return rc;
        continue;
      }
      const int s = (int)(running++ % pcdhip_ctx::PIPE_SLOTS);
      MsmWorkspace& ws = ctx->g16_ws[2 + s];
      hipStream_t sk = ctx->g16_streams[2 + s];
      if (!used[s]) TRY(hipStreamWaitEvent(sk, ctx->g16_ready, 0));
      used[s] = true;
      TRY(ws.ensure(WS_OUT, jac_b + 64));
      uint32_t* out_dev = (uint32_t*)ws.buf[WS_OUT];
      const MsmBasesView bv = k == 0 ? pg->view(0) : sp->view((size_t)items[k - 2].shifted_offset);
      ws.lane = ctx->g16_schedule == 2 && ctx->pipe_lane && ctx->lane.stream ? &ctx->lane : nullptr;
      const hipError_t me = ge.msm(ws, sk, bv, q[y], (uint32_t)n, out_dev, ctx->msm_c, ctx->msm_chunk, ctx->msm_sort, nullptr, nullptr, MSM_SHARE_NONE);
      ws.lane = nullptr;
      TRY(me);
      large++;
      TRY(hipMemcpyAsync(res + slot * jw, out_dev, jac_b, hipMemcpyDeviceToDevice, sk));  // (before the workspace is used again)
    }
  }
  for (int s = 0; s < pcdhip_ctx::PIPE_SLOTS; s++) if (used[s]) TRY(hipEventRecord(ctx->g16_end[2 + s], ctx->g16_streams[2 + s]));
  uint32_t chain = 0;
  if (!batch.empty()) {  // (the quotients are canonical by construction: no error word is read)
    rc = msm_short_batch_async(ctx, pgg, batch.data(), batch.size(), res, jw, nullptr, &chain);
    if (rc) return rc;
  }
  ctx->kzg_batch_open_plan[0] = large;
  ctx->kzg_batch_open_plan[1] = batch.size();
  ctx->kzg_batch_open_plan[2] = one_by_one;
  ctx->kzg_batch_open_plan[3] = launches;
  for (int s = 0; s < pcdhip_ctx::PIPE_SLOTS; s++) if (used[s]) TRY(hipStreamWaitEvent(st, ctx->g16_end[2 + s], 0));
  TRY(ge.jac_sum_parts(st, res, P * jw, (uint32_t)OPEN_SLOTS, (uint32_t)P, (uint32_t*)(base + o_sum)));
  TRY(ge.jac_out(st, (const uint32_t*)(base + o_sum), (uint32_t)P, (uint32_t*)(base + o_abi)));
  TRY(ge.to_affine(st, (const uint32_t*)(base + o_abi), (uint32_t)P, (uint32_t*)(base + o_back)));
  if (np) TRY(hipMemcpyAsync(base + o_back + P * ab, values_dev, np * eb, hipMemcpyDeviceToDevice, st));
  std::vector<uint64_t> back((back_b + 7) / 8);
  TRY(hipMemcpyAsync(back.data(), base + o_back, back_b, hipMemcpyDeviceToHost, st));
  TRY(hipStreamSynchronize(st));
  const size_t pl1 = ab / 8, L = sw / 2;
  memcpy(w_xy, back.data(), P * ab);
  memset(values_mont, 0, P * L * 8);
  memset(random_v_mont, 0, P * L * 8);
  for (size_t o = 0; o < P; o++) {
    w_inf[o] = abi_is_zero(&back[o * pl1], pl1) ? 1 : 0;
    const int yc = pl.part_of[o * (2 + m)], yr = pl.part_of[o * (2 + m) + 1];
    if (yc >= 0) memcpy(values_mont + o * L, &back[P * pl1 + (size_t)yc * L], L * 8);
    if (yr >= 0) memcpy(random_v_mont + o * L, &back[P * pl1 + (size_t)yr * L], L * 8);
  }
  return PCDHIP_OK;
}
void mont_to_canonical(int fr, const uint64_t* in, uint64_t* out) {
  with_host_field(fr, [&](auto f) { decltype(f)::type::from_abi((const uint32_t*)in).to_canonical_words((uint32_t*)out); });
}
// the one of GT in the C-ABI image (tower order: its first base-field coefficient is 1, the others 0), as the pairing writes it
void gt_one(int curve_id, uint64_t* out /* zeroed */) {
  with_host_field(kCurveFq[curve_id], [&](auto fq) { decltype(fq)::type::one().to_abi((uint32_t*)out); });
}
}  // namespace

extern "C" {

int pcdhip_poly_eval(pcdhip_ctx* ctx, const pcdhip_buf* const* polys, const size_t* lens, size_t k, const uint64_t* z_mont,
                     uint64_t* out_mont) {
  return guarded([&]() -> int {
  if (!ctx || !z_mont || (k && (!polys || !lens || !out_mont)) || k > 65535) return PCDHIP_E_ARG;
  if (k == 0) return PCDHIP_OK;
  std::vector<PolyDesc> d;
  uint64_t max_len = 0;
  const int f = poly_descs(polys, lens, k, &d, &max_len);
  if (f < 0) return PCDHIP_E_ARG;
  BIND();
  uint32_t* vals = nullptr;
  int rc = poly_eval_run(ctx, f, d, max_len, z_mont, &vals);
  if (rc) return rc;
  TRY(hipMemcpyAsync(out_mont, vals, k * kFieldLimbs[f] * 8, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
  });
}

int pcdhip_poly_lincomb(pcdhip_ctx* ctx, const pcdhip_buf* const* polys, const size_t* lens, const uint64_t* coeffs_mont, size_t k,
                        pcdhip_buf* out, size_t* out_len) {
  return guarded([&]() -> int {
  if (!ctx || !out || !out_len || (k && (!polys || !lens || !coeffs_mont)) || k >= (1ull << 31)) return PCDHIP_E_ARG;
  std::vector<PolyDesc> d;
  uint64_t max_len = 0;
  const int f = k ? poly_descs(polys, lens, k, &d, &max_len) : out->field_id;
  if (f < 0 || f != out->field_id || max_len > out->n) return PCDHIP_E_ARG;
  *out_len = max_len;
  if (max_len == 0) return PCDHIP_OK;
  BIND();
  const FieldEntry& fe = field_entry(f);
  const size_t db = (k * sizeof(PolyDesc) + 255) & ~(size_t)255;
  TRY(ctx->aux_ws.ensure(AUX_POLY, db + k * fe.abi_words * 4));
  char* base = (char*)ctx->aux_ws.buf[AUX_POLY];
  TRY(hipMemcpyAsync(base, d.data(), k * sizeof(PolyDesc), hipMemcpyHostToDevice, ctx->stream));
  TRY(hipMemcpyAsync(base + db, coeffs_mont, k * fe.abi_words * 4, hipMemcpyHostToDevice, ctx->stream));
  TRY(fe.poly_lincomb(ctx->stream, (const PolyDesc*)base, (const uint32_t*)(base + db), (uint32_t)k, max_len, out->dptr));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
  });
}

int pcdhip_poly_div_linear(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, const uint64_t* z_mont, pcdhip_buf* q, uint64_t* value_mont) {
  return guarded([&]() -> int {
  if (!ctx || !p || !z_mont || !value_mont || len > p->n || len >= (1ull << 31)) return PCDHIP_E_ARG;
  if (len > 1 && (!q || q->field_id != p->field_id || q->n < len - 1 || q->dptr == p->dptr)) return PCDHIP_E_ARG;
  BIND();
  const std::vector<PolyDesc> d = {{p->dptr, (uint64_t)len}};
  uint32_t* vals = nullptr;
  int rc = poly_eval_run(ctx, p->field_id, d, len, z_mont, &vals, &d[0], len > 1 ? q->dptr : nullptr, 0);
  if (rc) return rc;
  TRY(hipMemcpyAsync(value_mont, vals, kFieldLimbs[p->field_id] * 8, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
  });
}

int pcdhip_kzg_open(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g, const pcdhip_buf* p,
                    size_t len, const pcdhip_buf* blinding, size_t blinding_len, const uint64_t* z_mont, uint64_t* w_xyz_mont,
                    uint64_t* value_mont, uint64_t* random_v_mont) {
  return guarded([&]() -> int {
  if (!ctx || !powers_of_g || !p || !z_mont || !w_xyz_mont || !value_mont) return PCDHIP_E_ARG;
  if (!powers_of_g->shards.empty() || p->field_id != kCurveFr[powers_of_g->curve_id] || len > p->n || len >= (1ull << 31)) return PCDHIP_E_ARG;
  const size_t qn = len ? len - 1 : 0, bqn = blinding_len ? blinding_len - 1 : 0;
  if (qn > powers_of_g->n) return PCDHIP_E_ARG;  // upstream's TooManyCoefficients
  if (blinding && (!powers_of_gamma_g || !random_v_mont || !powers_of_gamma_g->shards.empty() ||
                   powers_of_gamma_g->curve_id != powers_of_g->curve_id || powers_of_gamma_g->group_id != powers_of_g->group_id ||
                   blinding->field_id != p->field_id || blinding_len > blinding->n || bqn > powers_of_gamma_g->n))
    return PCDHIP_E_ARG;
  BIND();
  uint32_t* q = nullptr;
  int rc = kzg_divide(ctx, p, len, z_mont, AUX_POLY_Q, &q, value_mont);
  rc = rc ? rc : kzg_witness(ctx, powers_of_g, q, qn, w_xyz_mont);
  if (rc || !blinding) return rc;
  // hiding: w += MSM(powers_of_gamma_g, blinding / (X - z)), random_v = blinding(z)
  const size_t jw = (size_t)pcdhip_point_limbs(powers_of_g->curve_id, powers_of_g->group_id) / 2 * 3;
  std::vector<uint64_t> both(2 * jw);
  memcpy(both.data(), w_xyz_mont, jw * 8);
  uint32_t* rq = nullptr;
  rc = kzg_divide(ctx, blinding, blinding_len, z_mont, AUX_POLY_R, &rq, random_v_mont);
  rc = rc ? rc : kzg_witness(ctx, powers_of_gamma_g, rq, bqn, &both[jw]);
  return rc ? rc : pcdhip_points_sum(ctx, powers_of_g->curve_id, powers_of_g->group_id, both.data(), 2, w_xyz_mont);
  });
}

int pcdhip_kzg_commit(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g,
                      const pcdhip_bases* shifted_powers_of_g, const pcdhip_kzg_commit_item* items, size_t k, uint64_t* comm_xy, uint8_t* comm_inf,
                      uint64_t* shifted_xy, uint8_t* shifted_inf, uint64_t* trimmed_len) {
  return guarded([&]() -> int {
  if (!ctx || !powers_of_g || (k && (!items || !comm_xy || !comm_inf))) return PCDHIP_E_ARG;  // (before any handle is looked into)
  const pcdhip_bases *pg = powers_of_g, *pgg = powers_of_gamma_g, *sp = shifted_powers_of_g;
  auto g1_of_pg = [&](const pcdhip_bases* b) { return b->shards.empty() && b->group_id == 1 && b->curve_id == pg->curve_id; };
  if (!valid_curve(pg->curve_id) || !g1_of_pg(pg) || (pgg && !g1_of_pg(pgg)) || (sp && !g1_of_pg(sp)) || k > 21845) return PCDHIP_E_ARG;
  if (pipe_pending(ctx)) return PCDHIP_E_ARG;  // submitted MSMs still own side-stream workspaces: collect them first
  if (k == 0) return PCDHIP_OK;
  const int fr = kCurveFr[pg->curve_id];
  std::vector<CommitPlan> plan(k);
  std::vector<PolyCommitDesc> descs(k);
  size_t scal_elems = 0;
  uint64_t max_len = 0;
  auto blinding_ok = [&](const pcdhip_buf* b, uint64_t len) { return pgg && b->field_id == fr && len <= b->n && len <= pgg->n; };
  for (size_t j = 0; j < k; j++) {
    const pcdhip_kzg_commit_item& it = items[j];
    if ((!it.poly && it.len) || (it.poly && (it.poly->field_id != fr || it.len > it.poly->n)) || it.len >= (1ull << 31)) return PCDHIP_E_ARG;
    if (it.blinding && !blinding_ok(it.blinding, it.blinding_len)) return PCDHIP_E_ARG;
    if (it.shifted_blinding && (!it.shifted || !blinding_ok(it.shifted_blinding, it.shifted_blinding_len))) return PCDHIP_E_ARG;
    if (it.shifted && (!sp || !shifted_xy || !shifted_inf || it.shifted_offset > sp->n)) return PCDHIP_E_ARG;
    const uint64_t cap = it.shifted ? std::min<uint64_t>(pg->n, sp->n - it.shifted_offset) : pg->n;  // bases the item may use
    plan[j].n = std::min<uint64_t>(it.len, cap);
    plan[j].scal = scal_elems;
    scal_elems += plan[j].n;
    descs[j] = {it.poly ? it.poly->dptr : nullptr, it.len, cap, nullptr};
    max_len = std::max(max_len, it.len);
  }
  for (size_t j = 0; j < k; j++) {  // the blinding polynomials: further descriptors of the same launch
    const pcdhip_kzg_commit_item& it = items[j];
    if (it.blinding && it.blinding_len) {
      plan[j].blind = (int)descs.size(); plan[j].bscal = scal_elems; scal_elems += it.blinding_len;
      descs.push_back({it.blinding->dptr, it.blinding_len, it.blinding_len, nullptr});
      max_len = std::max(max_len, it.blinding_len);
    }
    if (it.shifted_blinding && it.shifted_blinding_len) {
      plan[j].sblind = (int)descs.size(); plan[j].sbscal = scal_elems; scal_elems += it.shifted_blinding_len;
      descs.push_back({it.shifted_blinding->dptr, it.shifted_blinding_len, it.shifted_blinding_len, nullptr});
      max_len = std::max(max_len, it.shifted_blinding_len);
    }
  }
  BIND();
  int rc = ensure_side_streams(ctx);
  if (rc) return rc;
  rc = kzg_commit_run(ctx, pg, pgg, sp, items, k, plan, descs, scal_elems, max_len, comm_xy, comm_inf, shifted_xy, shifted_inf, trimmed_len);
  if (rc) (void)hipDeviceSynchronize();  // (an error partway: nothing of this call stays in flight on the side streams, or reads the frames above)
  return rc;
  });
}

int pcdhip_kzg_commit_last_plan(pcdhip_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return PCDHIP_E_ARG;
  for (int i = 0; i < 4; i++) out[i] = ctx->kzg_commit_plan[i];
  return PCDHIP_OK;
}

int pcdhip_poly_open_quotients(pcdhip_ctx* ctx, int field_id, const pcdhip_kzg_commit_item* items, size_t m, size_t n_openings, const uint64_t* points_mont,
                               const uint64_t* coeffs_mont, const uint64_t* shifted_coeffs_mont, pcdhip_buf* const* q_bufs, size_t* q_lens,
                               uint64_t* values_mont) {
  return guarded([&]() -> int {
  const size_t P = n_openings;
  if (!ctx || !valid_field(field_id) || (m && !items) || (P && (!points_mont || !q_lens || !values_mont || (m && !coeffs_mont))))
    return PCDHIP_E_ARG;
  if (P == 0) return PCDHIP_OK;
  OpenPlan pl;
  int rc = open_plan(items, m, P, coeffs_mont, shifted_coeffs_mont, field_id, &pl);
  if (rc) return rc;
  const size_t np = pl.parts.size(), tab = P * (2 + m);
  std::vector<uint32_t*> q(np, nullptr);
  for (size_t y = 0; y < np; y++) {
    if (pl.parts[y].len <= 1) continue;
    const pcdhip_buf* b = q_bufs ? q_bufs[pl.slot_of[y]] : nullptr;
    if (!b || b->field_id != pl.field || b->n < pl.parts[y].len - 1) return PCDHIP_E_ARG;
    q[y] = b->dptr;
  }
  const size_t L = (size_t)kFieldLimbs[pl.field];
  if (np == 0) {  // (no coefficient: every part is absent)
    for (size_t s = 0; s < tab; s++) q_lens[s] = 0;
    memset(values_mont, 0, tab * L * 8);
    return PCDHIP_OK;
  }
  BIND();
  const FieldEntry& fe = field_entry(pl.field);
  const size_t eb = (size_t)fe.abi_words * 4;
  size_t off[6];
  const size_t o_work = open_tables_bytes(pl, fe, off);
  TRY(ctx->aux_ws.ensure(AUX_OPEN, o_work + std::max<size_t>(pl.work_elems, 1) * eb));
  char* base = (char*)ctx->aux_ws.buf[AUX_OPEN];
  uint32_t* values_dev = nullptr;
  rc = open_run(ctx, pl, base, (uint32_t*)(base + o_work), q.data(), points_mont, coeffs_mont, shifted_coeffs_mont, &values_dev, nullptr);
  if (rc) return rc;
  std::vector<uint64_t> vals(np * L);
  TRY(hipMemcpyAsync(vals.data(), values_dev, np * eb, hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  memset(values_mont, 0, tab * L * 8);
  for (size_t s = 0; s < tab; s++) q_lens[s] = 0;
  for (size_t y = 0; y < np; y++) {
    q_lens[pl.slot_of[y]] = (size_t)(pl.parts[y].len - 1);
    memcpy(values_mont + pl.slot_of[y] * L, &vals[y * L], L * 8);
  }
  return PCDHIP_OK;
  });
}

int pcdhip_kzg_batch_open(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g,
                          const pcdhip_bases* shifted_powers_of_g, const pcdhip_kzg_commit_item* items, size_t m, size_t n_openings,
                          const uint64_t* points_mont, const uint64_t* coeffs_mont, const uint64_t* shifted_coeffs_mont, uint64_t* w_xy,
                          uint8_t* w_inf, uint64_t* values_mont, uint64_t* random_v_mont) {
  return guarded([&]() -> int {
  const size_t P = n_openings;
  if (!ctx || !powers_of_g || (m && !items) || (P && (!points_mont || !w_xy || !w_inf || !values_mont || !random_v_mont || (m && !coeffs_mont))))
    return PCDHIP_E_ARG;  // (before any handle is looked into)
  const pcdhip_bases *pg = powers_of_g, *pgg = powers_of_gamma_g, *sp = shifted_powers_of_g;
  auto g1_of_pg = [&](const pcdhip_bases* b) { return b->shards.empty() && b->group_id == 1 && b->curve_id == pg->curve_id; };
  if (!valid_curve(pg->curve_id) || !g1_of_pg(pg) || (pgg && !g1_of_pg(pgg)) || (sp && !g1_of_pg(sp))) return PCDHIP_E_ARG;
  if (pipe_pending(ctx)) return PCDHIP_E_ARG;  // submitted MSMs still own side-stream workspaces: collect them first
  if (P == 0) return PCDHIP_OK;
  const int fr = kCurveFr[pg->curve_id];
  OpenPlan pl;
  int rc = open_plan(items, m, P, coeffs_mont, shifted_coeffs_mont, fr, &pl);
  if (rc) return rc;
  if (pl.takes_blinding && !pgg) return PCDHIP_E_ARG;
  for (size_t y = 0; y < pl.parts.size(); y++) {  // upstream's TooManyCoefficients, and the degree bound's room in the shifted powers
    const size_t k = pl.slot_of[y] % (2 + m);
    const uint64_t qn = pl.parts[y].len - 1;
    if (k == 0 && qn > pg->n) return PCDHIP_E_ARG;
    if (k == 1 && qn > pgg->n) return PCDHIP_E_ARG;
    if (k >= 2 && (!sp || items[k - 2].shifted_offset > sp->n || qn > sp->n - items[k - 2].shifted_offset)) return PCDHIP_E_ARG;
  }
  if (shifted_coeffs_mont && !sp) {  // a degree-bound term of an empty item has no part, and still needs its handle
    const size_t L = (size_t)kFieldLimbs[fr];
    for (size_t s = 0; s < P * m; s++) if (!abi_is_zero(shifted_coeffs_mont + s * L, L)) return PCDHIP_E_ARG;
  }
  BIND();
  rc = ensure_side_streams(ctx);
  if (rc) return rc;
  rc = kzg_batch_open_run(ctx, pg, pgg, sp, items, pl, points_mont, coeffs_mont, shifted_coeffs_mont, w_xy, w_inf, values_mont, random_v_mont);
  if (rc) (void)hipDeviceSynchronize();  // (an error partway: nothing of this call stays in flight on the side streams, or reads the frames above)
  return rc;
  });
}

int pcdhip_kzg_batch_open_last_plan(pcdhip_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return PCDHIP_E_ARG;
  for (int i = 0; i < 4; i++) out[i] = ctx->kzg_batch_open_plan[i];
  return PCDHIP_OK;
}

// Both sides of the check are MSMs over one small uploaded vector (C_1..C_n, W_1..W_n, -g, -gamma_g): the left with the scalars
// (r_i, r_i z_i, sum r_i v_i, sum r_i rv_i), the right (sum r_i W_i) over its W range; the scalars are formed on the host with the
// field code of the RLC verification, the group and pairing work runs on the device.
int pcdhip_kzg_check(pcdhip_ctx* ctx, int curve_id, const uint64_t* g_xy, const uint64_t* gamma_g_xy, const uint64_t* h_xy,
                     const uint64_t* beta_h_xy, size_t n, const uint64_t* comms_xy, const uint8_t* comms_inf, const uint64_t* points_mont,
                     const uint64_t* values_mont, const uint64_t* w_xy, const uint8_t* w_inf, const uint64_t* random_v_mont,
                     const uint64_t* randomizers_canonical, int* ok) {
  return guarded([&]() -> int {
  if (!ctx || !valid_curve(curve_id) || !ok) return PCDHIP_E_ARG;
  *ok = 0;
  if (n == 0) { *ok = 1; return PCDHIP_OK; }
  if (!g_xy || !h_xy || !beta_h_xy || !comms_xy || !points_mont || !values_mont || !w_xy || (random_v_mont && !gamma_g_xy) ||
      (n > 1 && !randomizers_canonical) || n >= (1u << 20))
    return PCDHIP_E_ARG;
  BIND();
  const int fr = kCurveFr[curve_id];
  const size_t sl = (size_t)kFieldLimbs[fr], l1 = (size_t)pcdhip_point_limbs(curve_id, 1), l2 = (size_t)pcdhip_point_limbs(curve_id, 2);
  const size_t j1 = l1 / 2 * 3, nb = 2 * n + 2;
  std::vector<uint64_t> r(n * sl, 0), zc(n * sl), vc(n * sl), rvc(n * sl, 0);
  if (randomizers_canonical) memcpy(r.data(), randomizers_canonical, n * sl * 8);
  else r[0] = 1;
  for (size_t i = 0; i < n; i++) {
    mont_to_canonical(fr, points_mont + i * sl, &zc[i * sl]);
    mont_to_canonical(fr, values_mont + i * sl, &vc[i * sl]);
    if (random_v_mont) mont_to_canonical(fr, random_v_mont + i * sl, &rvc[i * sl]);
  }
  std::vector<uint64_t> sc(nb * sl, 0), pts(nb * l1, 0);
  std::vector<uint8_t> inf(nb, 0);
  std::vector<const uint64_t*> pr(n), pv(n), prv(n);
  for (size_t i = 0; i < n; i++) {
    pr[i] = &r[i * sl];
    pv[i] = &vc[i * sl];
    prv[i] = &rvc[i * sl];
    memcpy(&sc[i * sl], &r[i * sl], sl * 8);
    const uint64_t* zi = &zc[i * sl];
    scalar_lincomb(fr, &pr[i], &zi, 1, &sc[(n + i) * sl]);
    memcpy(&pts[i * l1], comms_xy + i * l1, l1 * 8);
    memcpy(&pts[(n + i) * l1], w_xy + i * l1, l1 * 8);
    inf[i] = comms_inf ? comms_inf[i] : 0;
    inf[n + i] = w_inf ? w_inf[i] : 0;
  }
  scalar_lincomb(fr, pr.data(), pv.data(), n, &sc[2 * n * sl]);
  memcpy(&pts[2 * n * l1], g_xy, l1 * 8);
  negate_point(curve_id, 1, &pts[2 * n * l1]);
  if (random_v_mont) {
    scalar_lincomb(fr, pr.data(), prv.data(), n, &sc[(2 * n + 1) * sl]);
    memcpy(&pts[(2 * n + 1) * l1], gamma_g_xy, l1 * 8);
    negate_point(curve_id, 1, &pts[(2 * n + 1) * l1]);
  } else {
    inf[2 * n + 1] = 1;
  }
  pcdhip_bases* b = nullptr;
  const int saved = ctx->precompute;
  ctx->precompute = 0;  // a handful of points used twice: no window copies
  int rc = pcdhip_bases_upload(ctx, curve_id, 1, pts.data(), inf.data(), nb, &b);
  ctx->precompute = saved;
  if (rc) return rc;
  std::vector<uint64_t> jac(2 * j1);
  // (pcdhip_msm_set_short: each of the two MSMs skips the buckets when it covers few enough pairs; a multi-device context's vector is
  //  sharded and keeps the bucket pipeline, which sums over the devices)
  const bool may_short = b->shards.empty();
  rc = may_short && nb <= ctx->msm_short_max ? msm_short_host(ctx, b, 0, sc.data(), nb, jac.data()) : pcdhip_msm(ctx, b, 0, sc.data(), nb, jac.data());
  if (!rc) rc = may_short && n <= ctx->msm_short_max ? msm_short_host(ctx, b, n, r.data(), n, &jac[j1]) : pcdhip_msm(ctx, b, n, r.data(), n, &jac[j1]);
  pcdhip_bases_free(ctx, b);
  if (rc) return rc;
  std::vector<uint64_t> aff(2 * l1);
  uint8_t aff_inf[2] = {0, 0};
  rc = pcdhip_to_affine(ctx, curve_id, 1, jac.data(), 2, aff.data(), aff_inf);
  if (rc) return rc;
  negate_point(curve_id, 1, aff.data());
  // e(-lhs, h) e(rhs, beta_h) == 1
  std::vector<uint64_t> g2s(2 * l2);
  memcpy(g2s.data(), h_xy, l2 * 8);
  memcpy(&g2s[l2], beta_h_xy, l2 * 8);
  const size_t gw = (size_t)pairing_entry(curve_id).gt_words / 2;
  std::vector<uint64_t> gt(gw), one(gw, 0);
  rc = pcdhip_multi_pairing(ctx, curve_id, aff.data(), aff_inf, g2s.data(), nullptr, 2, gt.data());
  if (rc) return rc;
  gt_one(curve_id, one.data());
  *ok = memcmp(gt.data(), one.data(), gw * 8) == 0 ? 1 : 0;
  return PCDHIP_OK;
  });
}

}  // extern "C"
