// Fixed-base multiplication batches and the Groth16 setup of libpcdhip.so.
#include "capi_internal.h"

using namespace pcd;

namespace {
// out (device, AUX_FB_OUT): n affine points in the C-ABI image followed by n flag bytes; scalars canonical words on the device
int fixed_base_dev(pcdhip_ctx* ctx, const GroupEntry& ge, const uint32_t* base_abi_dev, const uint32_t* scalars_dev, size_t n,
                   uint32_t** out_pts, uint8_t** out_inf) {
  const size_t ab = (size_t)ge.point_abi_words * 4, jb = (size_t)ge.point_words / 2 * 3 * 4;
  TRY(ctx->aux_ws.ensure(AUX_FB_TABLE, ge.fb_table_words * 4));
  TRY(ctx->aux_ws.ensure(AUX_FB_JAC, std::max<size_t>(n, 1) * jb));
  TRY(ctx->aux_ws.ensure(AUX_FB_OUT, std::max<size_t>(n, 1) * (ab + 1) + 64));
  *out_pts = (uint32_t*)ctx->aux_ws.buf[AUX_FB_OUT];
  *out_inf = (uint8_t*)ctx->aux_ws.buf[AUX_FB_OUT] + n * ab;
  TRY(ge.fixed_base(ctx->stream, base_abi_dev, scalars_dev, (uint32_t)n, (uint32_t*)ctx->aux_ws.buf[AUX_FB_TABLE],
                    (uint32_t*)ctx->aux_ws.buf[AUX_FB_JAC], *out_pts, *out_inf));
  return PCDHIP_OK;
}

}  // namespace

namespace pcd {
// transpose of a CSR matrix with `cols` columns, as CSR (host side: an index permutation, no field arithmetic).  With `perm`, column c
// becomes row perm[c] of a result with `rows_out` rows (every perm[c] < rows_out; the rows that no column maps to stay empty)
int transpose_csr(const pcdhip_csr* m, size_t cols, size_t limbs, HostCsrT* t, const uint32_t* perm, size_t rows_out) {
  if (!m || !m->row_ptr) return PCDHIP_E_ARG;
  const uint64_t nnz = m->row_ptr[m->num_rows];
  if (nnz && (!m->col || !m->coeff)) return PCDHIP_E_ARG;
  const size_t rows = perm ? rows_out : cols;
  auto at = [&](uint32_t c) -> size_t { return perm ? perm[c] : c; };
  t->rp.assign(rows + 1, 0);
  for (uint64_t k = 0; k < nnz; k++) {
    if (m->col[k] >= cols || at(m->col[k]) >= rows) return PCDHIP_E_ARG;
    t->rp[at(m->col[k]) + 1]++;
  }
  for (size_t c = 0; c < rows; c++) t->rp[c + 1] += t->rp[c];
  t->col.resize(nnz);
  t->coeff.resize(nnz * limbs);
  std::vector<uint64_t> fill(t->rp.begin(), t->rp.end() - 1);
  for (uint64_t r = 0; r < m->num_rows; r++)
    for (uint64_t k = m->row_ptr[r]; k < m->row_ptr[r + 1]; k++) {
      const uint64_t d = fill[at(m->col[k])]++;
      t->col[d] = (uint32_t)r;
      memcpy(&t->coeff[d * limbs], m->coeff + k * limbs, limbs * 8);
    }
  t->view = {rows, t->rp.data(), t->col.data(), t->coeff.data()};
  return PCDHIP_OK;
}
}  // namespace pcd

extern "C" {

int pcdhip_fixed_base_mul(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* base_xy, const uint64_t* scalars, size_t n,
                          uint64_t* out_xy, uint8_t* out_inf) {
  if (!ctx || !valid_curve(curve_id) || !valid_group(group_id) || !base_xy || (n && (!scalars || !out_xy || !out_inf)) || (n >> 31))
    return PCDHIP_E_ARG;
  BIND();
  const GroupEntry& ge = group_entry(curve_id, group_id);
  const size_t ab = (size_t)ge.point_abi_words * 4, sb = (size_t)ge.scalar_words * 4;
  const size_t base_off = (n * sb + 63) / 64 * 64;  // the base point sits behind the scalars
  TRY(ctx->aux_ws.ensure(AUX_SCAL, base_off + ab));
  uint32_t* sc = (uint32_t*)ctx->aux_ws.buf[AUX_SCAL];
  uint32_t* base_dev = (uint32_t*)((char*)sc + base_off);
  if (n) TRY(hipMemcpyAsync(sc, scalars, n * sb, hipMemcpyHostToDevice, ctx->stream));
  TRY(hipMemcpyAsync(base_dev, base_xy, ab, hipMemcpyHostToDevice, ctx->stream));
  uint32_t* pts;
  uint8_t* inf;
  int rc = fixed_base_dev(ctx, ge, base_dev, sc, n, &pts, &inf);
  if (rc) return rc;
  if (n) {
    TRY(hipMemcpyAsync(out_xy, pts, n * ab, hipMemcpyDeviceToHost, ctx->stream));
    TRY(hipMemcpyAsync(out_inf, inf, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  TRY(hipStreamSynchronize(ctx->stream));
  return PCDHIP_OK;
}

int pcdhip_groth16_setup(pcdhip_ctx* ctx, int curve_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_vars,
                         size_t num_inputs, const uint64_t* g1_xy, const uint64_t* g2_xy, const uint64_t* toxic, pcdhip_g16_setup_out* out) {
  return guarded([&]() -> int {
  if (!ctx || !valid_curve(curve_id) || !A || !B || !C || !g1_xy || !g2_xy || !toxic || !out) return PCDHIP_E_ARG;
  if (num_inputs < 1 || num_inputs > num_vars || (num_vars >> 31) || A->num_rows != B->num_rows || A->num_rows != C->num_rows) return PCDHIP_E_ARG;
  if (!out->alpha_g1 || !out->beta_g1 || !out->delta_g1 || !out->beta_g2 || !out->gamma_g2 || !out->delta_g2 || !out->a_query ||
      !out->a_inf || !out->b_g1_query || !out->b_g1_inf || !out->b_g2_query || !out->b_g2_inf || !out->gamma_abc_g1 || !out->gamma_abc_inf)
    return PCDHIP_E_ARG;
  const int fr = kCurveFr[curve_id];
  // toxic waste, before anything is queued: all five reduced; alpha, beta, gamma, delta non-zero (upstream unwraps 1/gamma and 1/delta,
  // and the six single points have no flag to say "identity").  The Montgomery image of zero is zero.
  if (!scalars_reduced(fr, toxic, 5)) return PCDHIP_E_ARG;
  for (size_t k = 0; k < 4; k++) {
    const uint64_t* e = toxic + k * (size_t)kFieldLimbs[fr];
    if (std::all_of(e, e + kFieldLimbs[fr], [](uint64_t w) { return w == 0; })) return PCDHIP_E_ARG;
  }
  BIND();
  const FieldEntry& fe = field_entry(fr);
  const size_t m = num_vars, ni = num_inputs, nc = A->num_rows, limbs = (size_t)kFieldLimbs[fr];
  if (m > ni && (!out->l_query || !out->l_inf)) return PCDHIP_E_ARG;
  Dom d;
  int rc = pick_domain(fr, nc + ni, &d);
  if (rc) return rc;
  const size_t n = d.n;
  if (n > 1 && (!out->h_query || !out->h_inf)) return PCDHIP_E_ARG;
  hipStream_t st = ctx->stream;
  const size_t sb = (size_t)fe.abi_words * 4, eb = (size_t)fe.words * 4;
  // domain constants (generator, 1/n): the tables of the transforms over the same domain
  const FftTables* t;
  rc = d.m == 1 ? get_tables(ctx, fr, d.a, &t) : get_mixed_tables(ctx, fr, d, &t);
  if (rc) return rc;
  // scalars:  G1 [a (m) | b (m) | gamma_abc, l (m) | h (n - 1) | alpha, beta, delta]   G2 [b (m) | beta, gamma, delta]
  const size_t n1 = 3 * m + (n - 1) + 3, n2 = m + 3;
  TRY(ctx->aux_ws.ensure(AUX_FFT_X, n * eb));
  TRY(ctx->aux_ws.ensure(AUX_A, m * eb));
  TRY(ctx->aux_ws.ensure(AUX_B, m * eb));
  TRY(ctx->aux_ws.ensure(AUX_C, m * eb));
  TRY(ctx->aux_ws.ensure(AUX_Z_CANON, n1 * sb));
  TRY(ctx->aux_ws.ensure(AUX_H_CANON, n2 * sb));
  const GroupEntry& g1 = group_entry(curve_id, 1);
  const GroupEntry& g2 = group_entry(curve_id, 2);
  const size_t a1 = (size_t)g1.point_abi_words * 4, a2 = (size_t)g2.point_abi_words * 4;
  TRY(ctx->aux_ws.ensure(AUX_Z, 5 * sb + (size_t)fe.setup_consts * eb + a1 + a2 + 256));
  uint32_t* toxic_dev = (uint32_t*)ctx->aux_ws.buf[AUX_Z];
  uint32_t* consts_dev = toxic_dev + 5 * fe.abi_words;
  uint32_t* err_dev = consts_dev + (size_t)fe.setup_consts * fe.words;
  uint32_t* g1_dev = err_dev + 16;
  uint32_t* g2_dev = g1_dev + g1.point_abi_words;
  uint32_t* u = (uint32_t*)ctx->aux_ws.buf[AUX_FFT_X];
  uint32_t *at = (uint32_t*)ctx->aux_ws.buf[AUX_A], *bt = (uint32_t*)ctx->aux_ws.buf[AUX_B], *ct = (uint32_t*)ctx->aux_ws.buf[AUX_C];
  uint32_t* s1 = (uint32_t*)ctx->aux_ws.buf[AUX_Z_CANON];
  uint32_t* s2 = (uint32_t*)ctx->aux_ws.buf[AUX_H_CANON];
  TRY(hipMemcpyAsync(toxic_dev, toxic, 5 * sb, hipMemcpyHostToDevice, st));
  TRY(hipMemcpyAsync(g1_dev, g1_xy, a1, hipMemcpyHostToDevice, st));
  TRY(hipMemcpyAsync(g2_dev, g2_xy, a2, hipMemcpyHostToDevice, st));
  TRY(hipMemsetAsync(err_dev, 0, 4, st));
  TRY(fe.setup_scalars(st, t->consts, toxic_dev, (uint32_t)n, (uint32_t)nc, (uint32_t)m, (uint32_t)ni, nullptr, nullptr, nullptr, u, consts_dev,
                       err_dev, nullptr, nullptr, nullptr, nullptr, nullptr, 0));
  // At, Bt, Ct: a_i(tau) = sum_j A[j][i] u_j  -- the transposed matrices times u
  const pcdhip_csr* ms[3] = {A, B, C};
  uint32_t* vecs[3] = {at, bt, ct};
  for (int k = 0; k < 3; k++) {
    HostCsrT tr;
    rc = transpose_csr(ms[k], m, limbs, &tr);
    if (rc) return rc;
    DevCsr dm;
    rc = upload_csr(ctx, AUX_CSR_RP, &tr.view, fe, nc, &dm);
    if (rc) return rc;
    TRY(fe.spmv(st, dm, u, 0, 0, (uint32_t)m, vecs[k]));
    TRY(hipStreamSynchronize(st));  // `tr` and the staging slot are reused by the next matrix
  }
  uint32_t err = 0;
  TRY(hipMemcpyAsync(&err, err_dev, 4, hipMemcpyDeviceToHost, st));
  TRY(hipStreamSynchronize(st));
  if (err) return PCDHIP_E_ARG;  // tau lies in the evaluation domain
  TRY(fe.setup_scalars(st, t->consts, toxic_dev, (uint32_t)n, (uint32_t)nc, (uint32_t)m, (uint32_t)ni, at, bt, ct, u, consts_dev, err_dev, s1,
                       s1 + m * fe.abi_words, s1 + 2 * m * fe.abi_words, s1 + 3 * m * fe.abi_words, s2, 1));
  // alpha, beta, delta | beta, gamma, delta: C-ABI Montgomery -> canonical
  uint32_t* tail1 = s1 + (3 * m + (n - 1)) * fe.abi_words;
  uint32_t* tail2 = s2 + m * fe.abi_words;
  const int idx1[3] = {0, 1, 3}, idx2[3] = {1, 2, 3};
  for (int k = 0; k < 3; k++) {
    TRY(fe.convert(st, toxic_dev + idx1[k] * fe.abi_words, tail1 + k * fe.abi_words, 1, 3));
    TRY(fe.convert(st, toxic_dev + idx2[k] * fe.abi_words, tail2 + k * fe.abi_words, 1, 3));
  }
  // the fixed-base batches, then scatter into the caller's arrays
  uint32_t* pts;
  uint8_t* inf;
  rc = fixed_base_dev(ctx, g1, g1_dev, s1, n1, &pts, &inf);
  if (rc) return rc;
  auto fetch = [&](uint64_t* dst, uint8_t* dst_inf, size_t first, size_t cnt, size_t ab) -> hipError_t {
    if (!cnt) return hipSuccess;
    hipError_t e = hipMemcpyAsync(dst, (char*)pts + first * ab, cnt * ab, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dst_inf) e = hipMemcpyAsync(dst_inf, inf + first, cnt, hipMemcpyDeviceToHost, st);
    return e;
  };
  TRY(fetch(out->a_query, out->a_inf, 0, m, a1));
  TRY(fetch(out->b_g1_query, out->b_g1_inf, m, m, a1));
  TRY(fetch(out->gamma_abc_g1, out->gamma_abc_inf, 2 * m, ni, a1));
  TRY(fetch(out->l_query, out->l_inf, 2 * m + ni, m - ni, a1));
  TRY(fetch(out->h_query, out->h_inf, 3 * m, n - 1, a1));
  TRY(fetch(out->alpha_g1, nullptr, 3 * m + n - 1, 1, a1));
  TRY(fetch(out->beta_g1, nullptr, 3 * m + n, 1, a1));
  TRY(fetch(out->delta_g1, nullptr, 3 * m + n + 1, 1, a1));
  TRY(hipStreamSynchronize(st));
  rc = fixed_base_dev(ctx, g2, g2_dev, s2, n2, &pts, &inf);
  if (rc) return rc;
  TRY(fetch(out->b_g2_query, out->b_g2_inf, 0, m, a2));
  TRY(fetch(out->beta_g2, nullptr, m, 1, a2));
  TRY(fetch(out->gamma_g2, nullptr, m + 1, 1, a2));
  TRY(fetch(out->delta_g2, nullptr, m + 2, 1, a2));
  TRY(hipStreamSynchronize(st));
  out->domain_size = n;
  return PCDHIP_OK;
  });
}

}  // extern "C"
