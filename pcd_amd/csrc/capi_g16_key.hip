// The resident Groth16 proving key of libpcdhip.so: upload (whole or sharded across devices), resident R1CS, its plan and memory.
#include "capi_internal.h"

using namespace pcd;

extern "C" {

int pcdhip_g16_pk_upload(pcdhip_ctx* ctx, const pcdhip_g16_pk_host* h, pcdhip_g16_pk** out) {
  return guarded([&]() -> int {
  if (!ctx || !h || !out || !valid_curve((int)h->curve_id)) return PCDHIP_E_ARG;
  if (!h->alpha_g1 || !h->beta_g1 || !h->delta_g1 || !h->beta_g2 || !h->delta_g2 || !h->a_query || !h->b_g1_query ||
      !h->b_g2_query || (!h->h_query && h->h_len) || (!h->l_query && h->l_len))
    return PCDHIP_E_ARG;
  if (h->num_vars < 1 || h->num_inputs < 1 || h->num_inputs > h->num_vars || h->l_len != h->num_vars - h->num_inputs) return PCDHIP_E_ARG;
  BIND();
  const int cid = (int)h->curve_id;
  const size_t m = h->num_vars, ni = h->num_inputs;
  // delta is appended to the a / b / l queries: r*delta, s*delta and -rs*delta then ride inside the MSMs as
  // one more (base, scalar) pair instead of being serial scalar multiplications in the assembly.
  // Every a / b / l query gets four trailing slots matching the scalar tail [r, s, -rs, 1] that follows the
  // assignment: delta sits in the slot whose scalar the query needs, the vk point (alpha / beta) in the last one,
  // the remaining slots hold the point at infinity.  See inst_g16.hip.
  struct HostQuery { std::vector<uint64_t> pts; std::vector<uint8_t> inf; size_t n = 0; int group = 1; };
  auto with_tail = [&](int group, const uint64_t* q, const uint8_t* inf, size_t n, const uint64_t* delta, int delta_slot, const uint64_t* vk_point) {
    HostQuery hq;
    const size_t pl = (size_t)pcdhip_point_limbs(cid, group);
    hq.group = group; hq.n = n + 4;
    hq.pts.assign((n + 4) * pl, 0);
    hq.inf.assign(n + 4, 1);
    if (n) memcpy(hq.pts.data(), q, n * pl * 8);
    for (size_t i = 0; i < n; i++) hq.inf[i] = inf ? inf[i] : 0;
    memcpy(hq.pts.data() + (n + delta_slot) * pl, delta, pl * 8);
    hq.inf[n + delta_slot] = 0;
    if (vk_point) { memcpy(hq.pts.data() + (n + 3) * pl, vk_point, pl * 8); hq.inf[n + 3] = 0; }
    return hq;
  };
  HostQuery qa = with_tail(1, h->a_query, h->a_inf, m, h->delta_g1, 0, h->alpha_g1);          // r * delta + alpha
  HostQuery qb1 = with_tail(1, h->b_g1_query, h->b_g1_inf, m, h->delta_g1, 1, h->beta_g1);     // s * delta + beta
  HostQuery qb2 = with_tail(2, h->b_g2_query, h->b_g2_inf, m, h->delta_g2, 1, h->beta_g2);
  HostQuery ql;
  {  // l: padded in front with num_inputs points at infinity, so that it is indexed by the variable like a / b (one
     // sort of the assignment's digits then serves all four MSMs);  -rs * delta in slot 2
    const size_t pl = (size_t)pcdhip_point_limbs(cid, 1);
    std::vector<uint64_t> tmp(m * pl, 0);
    std::vector<uint8_t> tinf(m, 1);
    if (h->l_len) memcpy(tmp.data() + ni * pl, h->l_query, h->l_len * pl * 8);
    for (size_t i = 0; i < h->l_len; i++) tinf[ni + i] = h->l_inf ? h->l_inf[i] : 0;
    ql = with_tail(1, tmp.data(), tinf.data(), m, h->delta_g1, 2, nullptr);
  }
  // one key per device: the whole queries on an ordinary context, the entry range [lo, hi) of the a' / b' / l' queries and the
  // range [hlo, hhi) of the h query on device g of a multi-device context
  auto upload_range = [&](pcdhip_ctx* C, size_t lo, size_t hi, size_t hlo, size_t hhi, pcdhip_g16_pk** res) -> int {
    pcdhip_g16_pk* pk = new pcdhip_g16_pk();
    pk->curve_id = cid; pk->num_vars = m; pk->num_inputs = ni; pk->domain_size = h->domain_size; pk->h_len = h->h_len;
    C->precompute = ctx->precompute; C->precompute_budget = ctx->precompute_budget; C->msm_c = ctx->msm_c;
    auto up = [&](const HostQuery& q, pcdhip_bases** dst) -> int {
      const size_t pl = (size_t)pcdhip_point_limbs(cid, q.group);
      return bases_upload_single(C, cid, q.group, q.pts.data() + lo * pl, q.inf.data() + lo, hi - lo, dst);
    };
    for (size_t i = lo; i < hi && i < m; i++) { pk->a_inf_count += qa.inf[i] != 0; pk->b_inf_count += qb2.inf[i] != 0; }
    // Window bits of a key's queries: one less than the lone MSM's choice for large queries.  A proof runs six MSMs at once and is bound by
    // the sum of their kernels' work; the bucket reductions and fix-ups (proportional to 2^c, a third of that sum at the lone optimum) count
    // in full there, while the lone MSM hides part of them behind its own latency.  Same box, tools/ab_window_step.py: MNT4-298 main proof
    // 17.5 -> 16.8 ms (c = 20 -> 19; 18: 18.2), MNT4-753 160.3 -> 153.0 ms (21 -> 20; 19: 155.8); flat at the help proofs' 2^16 (left alone).
    struct BiasGuard { pcdhip_ctx* c; ~BiasGuard() { c->msm_c_bias = 0; } } bias_guard{C};
    C->msm_c_bias = (hi - lo >= ((size_t)1 << 18)) ? -1 : 0;
    pk->b_inf_same = memcmp(qb1.inf.data() + lo, qb2.inf.data() + lo, hi - lo) == 0;
    int rc = up(qa, &pk->a_query);
    rc = rc ? rc : up(qb1, &pk->b_g1_query);
    rc = rc ? rc : up(qb2, &pk->b_g2_query);
    rc = rc ? rc : up(ql, &pk->l_query);
    const size_t pl1 = (size_t)pcdhip_point_limbs(cid, 1);
    rc = rc ? rc : bases_upload_single(C, cid, 1, h->h_query ? h->h_query + hlo * pl1 : nullptr, h->h_inf ? h->h_inf + hlo : nullptr, hhi - hlo, &pk->h_query);
    if (rc) { pcdhip_g16_pk_free(C, pk); return rc; }
    // A second layout of the four queries over the assignment, for a smaller window (round 5).  The window of a key is fixed by its window-shifted
    // copies, and it is chosen for a DENSE scalar vector: c = 19 / 20 at 2^20 entries, one bucket window of 2^18 / 2^19.  A witness-like
    // assignment leaves a few per cent general scalars, but the fix-up, the first reduction level (two additions per bucket) and the 19 levels
    // over that bucket window cost every one of its four MSMs the same as a dense list: ~1.7 ms of device-filling work per G1 MSM of a proof
    // that takes 8.3 (profiles/r05_witness_like_critical_path.txt).  With copies for a window four bits shorter as well -- what the picker
    // chooses for a sixteenth of the entries -- pcdhip_groth16_prove counts the general scalars and takes the copies that fit the list.
    // Whole keys on an ordinary context only; automatic mode builds them for large keys whose extra copies take at most a quarter of the memory that
    // is free at upload (9.2 GB for a 298-bit key of 2^20 entries, 54 GB for a 753-bit one; pcdhip_set_precompute_budget applies to them as to any vector).
    if (C == ctx && ctx->peers.size() <= 1 && ctx->g16_sparse_window != 0 && pk->a_query && pk->a_query->groups > 1 &&
        (ctx->g16_sparse_window > 0 || hi - lo >= ((size_t)1 << 18) || (field_entry(kCurveFr[cid]).abi_words <= 12 && hi - lo >= ((size_t)1 << 14)))) {
      const int cs = ctx->g16_sparse_window > 0 ? ctx->g16_sparse_window : std::max(8, pk->a_query->c - 4);
      const int Ws = (group_entry(cid, 1).scalar_bits + 1 + cs - 1) / cs;
      const size_t extra = (size_t)Ws * (hi - lo) * (3 * (size_t)group_entry(cid, 1).point_words + (size_t)group_entry(cid, 2).point_words) * 4;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
      if (cs != pk->a_query->c && (ctx->g16_sparse_window > 0 || extra <= free_b / 4)) {
        const int saved_c = C->msm_c, saved_pre = C->precompute;
        auto drop_sparse = [&]() {
          pcdhip_bases_free(C, pk->a_sparse); pcdhip_bases_free(C, pk->b_g1_sparse); pcdhip_bases_free(C, pk->b_g2_sparse); pcdhip_bases_free(C, pk->l_sparse);
          pk->a_sparse = pk->b_g1_sparse = pk->b_g2_sparse = pk->l_sparse = nullptr;
        };
        // The four layouts must agree in window AND in the number of copies (they share one sorted entry list: MsmSharedSort), while memory (the
        // device's, or pcdhip_set_precompute_budget's bound per vector) grants the wide G2 vector fewer copies than the G1 ones: upload with all
        // copies, then bring everyone down to the smallest count granted (`precompute` = k copies).
        auto up_sparse = [&](int copies) -> int {
          C->msm_c = cs; C->msm_c_bias = 0; C->precompute = copies;
          // (the G2 vector first: it is the widest, so the count it is granted is the one the G1 vectors are then asked for)
          int rs = up(qb2, &pk->b_g2_sparse);
          if (!rs && pk->b_g2_sparse->groups >= 2 && pk->b_g2_sparse->groups < Ws) C->precompute = pk->b_g2_sparse->groups;
          rs = rs ? rs : up(qa, &pk->a_sparse);
          rs = rs ? rs : up(qb1, &pk->b_g1_sparse);
          rs = rs ? rs : up(ql, &pk->l_sparse);
          C->msm_c = saved_c; C->precompute = saved_pre;
          return rs;
        };
        auto sparse_whole = [&]() {
          return pk->a_sparse && pk->b_g1_sparse && pk->b_g2_sparse && pk->l_sparse && pk->a_sparse->groups >= 2 &&
                 pk->a_sparse->c == cs && pk->b_g1_sparse->c == cs && pk->b_g2_sparse->c == cs && pk->l_sparse->c == cs &&
                 pk->a_sparse->groups == pk->b_g1_sparse->groups && pk->a_sparse->groups == pk->b_g2_sparse->groups && pk->a_sparse->groups == pk->l_sparse->groups;
        };
        auto try_sparse = [&]() -> bool {
          int rs = up_sparse(-1);
          if (!rs && !sparse_whole() && pk->a_sparse && pk->b_g1_sparse && pk->b_g2_sparse && pk->l_sparse) {
            const int k = std::min(std::min(pk->a_sparse->groups, pk->b_g1_sparse->groups), std::min(pk->b_g2_sparse->groups, pk->l_sparse->groups));
            drop_sparse();
            if (k >= 2) rs = up_sparse(k);
          }
          if (rs || !sparse_whole()) { drop_sparse(); (void)hipGetLastError(); return false; }   // (the key works without them)
          return true;
        };
        bool have = try_sparse();
        // A window asked for OUTRIGHT (bits > 0) when the ordinary copies have already taken the memory: fewer ordinary copies + the second layout
        // instead of all ordinary copies and none -- the ordinary queries are uploaded again with half the copies (a Horner combine over the
        // windows that share a copy comes back for dense assignments) until the second layout fits beside them.
        for (int round = 0; !have && ctx->g16_sparse_window > 0 && round < 4; round++) {
          const int k = std::min(std::min(pk->a_query->groups, pk->b_g1_query->groups), std::min(pk->b_g2_query->groups, pk->l_query->groups)) / 2;
          if (k < 2) break;
          pcdhip_bases_free(C, pk->a_query); pcdhip_bases_free(C, pk->b_g1_query); pcdhip_bases_free(C, pk->b_g2_query); pcdhip_bases_free(C, pk->l_query);
          pk->a_query = pk->b_g1_query = pk->b_g2_query = pk->l_query = nullptr;
          C->precompute = k; C->msm_c_bias = (hi - lo >= ((size_t)1 << 18)) ? -1 : 0;
          int ro = up(qa, &pk->a_query);
          ro = ro ? ro : up(qb1, &pk->b_g1_query);
          ro = ro ? ro : up(qb2, &pk->b_g2_query);
          ro = ro ? ro : up(ql, &pk->l_query);
          C->precompute = saved_pre;
          if (ro) { pcdhip_g16_pk_free(C, pk); return ro; }
          have = try_sparse();
        }
      }
    }
    *res = pk;
    return PCDHIP_OK;
  };
  *out = nullptr;
  if (ctx->peers.size() <= 1) return upload_range(ctx, 0, m + 4, 0, h->h_len, out);
  pcdhip_g16_pk* parent = new pcdhip_g16_pk();
  parent->curve_id = cid; parent->num_vars = m; parent->num_inputs = ni; parent->domain_size = h->domain_size; parent->h_len = h->h_len;
  const size_t G = ctx->peers.size();
  parent->lo.resize(G + 1); parent->hlo.resize(G + 1);
  for (size_t g = 0; g < G; g++) {
    size_t lo, hi, hlo, hhi;
    shard_range(m + 4, g, G, &lo, &hi);
    shard_range(h->h_len, g, G, &hlo, &hhi);
    parent->lo[g] = lo; parent->lo[g + 1] = hi; parent->hlo[g] = hlo; parent->hlo[g + 1] = hhi;
    pcdhip_g16_pk* sh = nullptr;
    int rc = upload_range(ctx->peers[g], lo, hi, hlo, hhi, &sh);
    if (rc) { pcdhip_g16_pk_free(ctx, parent); return rc; }
    parent->shards.push_back(sh);
  }
  *out = parent;
  return PCDHIP_OK;
  });
}
int pcdhip_g16_pk_set_r1cs(pcdhip_ctx* ctx, pcdhip_g16_pk* pk, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C) {
  if (!ctx || !pk || !A || !B || !C) return PCDHIP_E_ARG;
  if (!pk->shards.empty()) {
    // the witness map's three chains (a, b, c: mat-vec, ifft, coset fft each) run on the first three devices of a sharded key
    // (SURVEY.md 8e), the pointwise step and the last transform on device 0: the matrices are resident wherever a chain runs
    int rc = pcdhip_g16_pk_set_r1cs(ctx->peers.empty() ? ctx : ctx->peers[0], pk->shards[0], A, B, C);
    for (size_t g = 1; !rc && g < 3 && g < pk->shards.size() && g < ctx->peers.size(); g++)
      rc = pcdhip_g16_pk_set_r1cs(ctx->peers[g], pk->shards[g], A, B, C);
    return rc;
  }
  if (A->num_rows != B->num_rows || A->num_rows != C->num_rows || (A->num_rows >> 31)) return PCDHIP_E_ARG;
  if (!A->row_ptr || !B->row_ptr || !C->row_ptr) return PCDHIP_E_ARG;
  BIND();
  const FieldEntry& fe = field_entry(kCurveFr[pk->curve_id]);
  const pcdhip_csr* ms[3] = {A, B, C};
  for (int k = 0; k < 3; k++) { int rc = validate_csr(ms[k], pk->num_vars); if (rc) return rc; }
  size_t total = 0, base[3], off[6];
  for (int k = 0; k < 3; k++) { base[k] = total; total += csr_bytes(ms[k], fe, off) + 64; }
  if (pk->r1cs_dev) { (void)hipFree(pk->r1cs_dev); pk->r1cs_dev = nullptr; }
  TRY(hipMalloc(&pk->r1cs_dev, total + 64));
  for (int k = 0; k < 3; k++) {
    DevCsr dc;
    int rc = upload_csr_to(ctx, ms[k], fe, pk->num_vars, (char*)pk->r1cs_dev + base[k], &dc);
    if (rc) return rc;
    pk->mats[k] = dc;
  }
  pk->rows = (uint32_t)A->num_rows;
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}
void pcdhip_g16_pk_free(pcdhip_ctx* ctx, pcdhip_g16_pk* pk) {
  if (!pk) return;
  for (size_t g = 0; g < pk->shards.size(); g++) pcdhip_g16_pk_free(ctx && g < ctx->peers.size() ? ctx->peers[g] : ctx, pk->shards[g]);
  pk->shards.clear();
  if (ctx) (void)hipSetDevice(ctx->device);
  if (pk->r1cs_dev) (void)hipFree(pk->r1cs_dev);
  pcdhip_bases_free(ctx, pk->a_query); pcdhip_bases_free(ctx, pk->b_g1_query); pcdhip_bases_free(ctx, pk->b_g2_query);
  pcdhip_bases_free(ctx, pk->h_query); pcdhip_bases_free(ctx, pk->l_query);
  pcdhip_bases_free(ctx, pk->a_sparse); pcdhip_bases_free(ctx, pk->b_g1_sparse); pcdhip_bases_free(ctx, pk->b_g2_sparse); pcdhip_bases_free(ctx, pk->l_sparse);
  delete pk;
}

int pcdhip_g16_pk_info(const pcdhip_g16_pk* pk, int window_bits[5], int windows[5]) {
  if (!pk || !window_bits || !windows) return PCDHIP_E_ARG;
  if (!pk->shards.empty()) return pcdhip_g16_pk_info(pk->shards[0], window_bits, windows);  // (the plan of device 0's shard)
  const pcdhip_bases* q[5] = {pk->a_query, pk->b_g1_query, pk->b_g2_query, pk->l_query, pk->h_query};
  for (int i = 0; i < 5; i++) {
    int copies = 0;
    int rc = q[i] ? pcdhip_bases_info(q[i], 0, &window_bits[i], &windows[i], &copies) : PCDHIP_E_ARG;
    if (rc) return rc;
  }
  return PCDHIP_OK;
}
// bytes of device memory a key's base vectors hold: out[0] the five queries with their window-shifted copies (every shard of a multi-device
// key), out[1] the second layout of the assignment queries for a shorter window (0 when not built), out[2] / out[3] the copies per point of the
// a query in the two layouts (device 0's shard)
int pcdhip_g16_pk_memory(const pcdhip_g16_pk* pk, uint64_t out[4]) {
  if (!pk || !out) return PCDHIP_E_ARG;
  out[0] = out[1] = out[2] = out[3] = 0;
  auto bytes = [](const pcdhip_bases* b) -> uint64_t {
    if (!b || !b->dptr) return 0;
    return (uint64_t)std::max<size_t>(b->n, 1) * group_entry(b->curve_id, b->group_id).base_stride_words * 4 * (uint64_t)b->groups + (b->inf_bits ? (b->n + 7) / 8 : 0);
  };
  std::vector<const pcdhip_g16_pk*> parts;
  if (pk->shards.empty()) parts.push_back(pk); else for (const pcdhip_g16_pk* s : pk->shards) parts.push_back(s);
  for (const pcdhip_g16_pk* s : parts) {
    out[0] += bytes(s->a_query) + bytes(s->b_g1_query) + bytes(s->b_g2_query) + bytes(s->l_query) + bytes(s->h_query);
    out[1] += bytes(s->a_sparse) + bytes(s->b_g1_sparse) + bytes(s->b_g2_sparse) + bytes(s->l_sparse);
  }
  out[2] = parts[0]->a_query ? (uint64_t)parts[0]->a_query->groups : 0;
  out[3] = parts[0]->a_sparse ? (uint64_t)parts[0]->a_sparse->groups : 0;
  return PCDHIP_OK;
}

}  // extern "C"
