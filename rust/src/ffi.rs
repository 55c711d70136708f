//! `extern "C"` binding of include/pcdhip.h (one declaration per entry point the shim uses; the header cites, for each, the
//! upstream function it replaces).  Source only; see INTEGRATION.md.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct pcdhip_ctx { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_bases { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_buf { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_g16_pk { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_pvk { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_marlin_index { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_marlin_mats { _p: [u8; 0] }
#[repr(C)] pub struct pcdhip_csr { pub num_rows: u64, pub row_ptr: *const u64, pub col: *const u32, pub coeff: *const u64 }
#[repr(C)]
pub struct pcdhip_g16_pk_host {
    pub curve_id: u32, pub _pad: u32, pub num_vars: u64, pub num_inputs: u64, pub domain_size: u64,
    pub alpha_g1: *const u64, pub beta_g1: *const u64, pub delta_g1: *const u64, pub beta_g2: *const u64, pub delta_g2: *const u64,
    pub a_query: *const u64, pub a_inf: *const u8, pub b_g1_query: *const u64, pub b_g1_inf: *const u8,
    pub b_g2_query: *const u64, pub b_g2_inf: *const u8, pub h_query: *const u64, pub h_inf: *const u8, pub h_len: u64,
    pub l_query: *const u64, pub l_inf: *const u8, pub l_len: u64,
}
#[repr(C)]
pub struct pcdhip_g16_setup_out {
    pub alpha_g1: *mut u64, pub beta_g1: *mut u64, pub delta_g1: *mut u64, pub beta_g2: *mut u64, pub gamma_g2: *mut u64, pub delta_g2: *mut u64,
    pub a_query: *mut u64, pub a_inf: *mut u8, pub b_g1_query: *mut u64, pub b_g1_inf: *mut u8, pub b_g2_query: *mut u64, pub b_g2_inf: *mut u8,
    pub h_query: *mut u64, pub h_inf: *mut u8, pub l_query: *mut u64, pub l_inf: *mut u8, pub gamma_abc_g1: *mut u64, pub gamma_abc_inf: *mut u8,
    pub domain_size: u64,
}
/// one labeled polynomial of `pcdhip_kzg_commit` (KZG10::commit / MarlinKZG10::commit over device-resident coefficients)
#[repr(C)]
pub struct pcdhip_kzg_commit_item {
    pub poly: *const pcdhip_buf, pub len: u64, pub blinding: *const pcdhip_buf, pub blinding_len: u64,
    pub shifted_blinding: *const pcdhip_buf, pub shifted_blinding_len: u64, pub shifted_offset: u64, pub shifted: u32, pub _pad: u32,
}
/// one MSM of `pcdhip_msm_short_batch` / `_dev`: `n` pairs from point `base_offset` and scalar `scalar_offset` on
#[repr(C)]
pub struct pcdhip_msm_short_item { pub base_offset: u64, pub scalar_offset: u64, pub n: u64 }

extern "C" {
    pub fn pcdhip_strerror(code: c_int) -> *const c_char;
    pub fn pcdhip_device_count() -> c_int;
    pub fn pcdhip_init(device_id: c_int, out: *mut *mut pcdhip_ctx) -> c_int;
    pub fn pcdhip_init_devices(device_ids: *const c_int, n_dev: c_int, out: *mut *mut pcdhip_ctx) -> c_int;
    pub fn pcdhip_destroy(ctx: *mut pcdhip_ctx);
    pub fn pcdhip_domain_size(field_id: c_int, min_size: usize) -> usize;
    pub fn pcdhip_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn pcdhip_host_free(p: *mut c_void);
    // K3 / K4 / K7: VariableBaseMSM::multi_scalar_mul over resident bases
    pub fn pcdhip_bases_upload(ctx: *mut pcdhip_ctx, curve: c_int, group: c_int, xy: *const u64, inf: *const u8, n: usize, out: *mut *mut pcdhip_bases) -> c_int;
    pub fn pcdhip_bases_free(ctx: *mut pcdhip_ctx, b: *mut pcdhip_bases);
    pub fn pcdhip_set_precompute_budget(ctx: *mut pcdhip_ctx, bytes: usize) -> c_int;
    pub fn pcdhip_get_precompute_budget(ctx: *mut pcdhip_ctx, bytes: *mut usize) -> c_int;
    pub fn pcdhip_msm(ctx: *mut pcdhip_ctx, bases: *const pcdhip_bases, offset: usize, scalars: *const u64, n: usize, out_xyz: *mut u64) -> c_int;
    // the same over short slices (at most 1024 pairs): no buckets, bit-plane sums over the handle's resident copies
    pub fn pcdhip_msm_short(ctx: *mut pcdhip_ctx, bases: *const pcdhip_bases, offset: usize, scalars: *const u64, n: usize, out_xyz: *mut u64) -> c_int;
    pub fn pcdhip_msm_short_dev(ctx: *mut pcdhip_ctx, bases: *const pcdhip_bases, offset: usize, scalars: *const pcdhip_buf, scalar_offset: usize, n: usize,
                                out_xyz: *mut u64) -> c_int;
    pub fn pcdhip_msm_short_batch(ctx: *mut pcdhip_ctx, bases: *const pcdhip_bases, scalars: *const u64, scalars_n: usize,
                                  items: *const pcdhip_msm_short_item, k: usize, out_xyz: *mut u64) -> c_int;
    pub fn pcdhip_msm_short_batch_dev(ctx: *mut pcdhip_ctx, bases: *const pcdhip_bases, scalars: *const pcdhip_buf,
                                      items: *const pcdhip_msm_short_item, k: usize, out_xyz: *mut u64) -> c_int;
    pub fn pcdhip_msm_set_short(ctx: *mut pcdhip_ctx, max_n: usize) -> c_int;
    pub fn pcdhip_to_affine(ctx: *mut pcdhip_ctx, curve: c_int, group: c_int, xyz: *const u64, n: usize, out_xy: *mut u64, out_inf: *mut u8) -> c_int;
    // K2: Radix2EvaluationDomain / GeneralEvaluationDomain transforms
    pub fn pcdhip_fft(ctx: *mut pcdhip_ctx, field: c_int, data: *mut u64, log_n: u32, inverse: c_int, coset: c_int) -> c_int;
    pub fn pcdhip_fft_general(ctx: *mut pcdhip_ctx, field: c_int, data: *mut u64, n: usize, inverse: c_int, coset: c_int) -> c_int;
    pub fn pcdhip_fft_seq(ctx: *mut pcdhip_ctx, field: c_int, data: *mut u64, n: usize, ops: *const c_int, n_ops: c_int) -> c_int;
    // K1 + K3 + K4 + K5: create_proof after synthesis
    pub fn pcdhip_g16_pk_upload(ctx: *mut pcdhip_ctx, host: *const pcdhip_g16_pk_host, out: *mut *mut pcdhip_g16_pk) -> c_int;
    pub fn pcdhip_g16_pk_set_r1cs(ctx: *mut pcdhip_ctx, pk: *mut pcdhip_g16_pk, a: *const pcdhip_csr, b: *const pcdhip_csr, c: *const pcdhip_csr) -> c_int;
    pub fn pcdhip_g16_pk_free(ctx: *mut pcdhip_ctx, pk: *mut pcdhip_g16_pk);
    /// device bytes a resident key holds: out[0] ordinary copies, out[1] the second layout, out[2] / out[3] copies per point (what a host
    /// that caches several keys budgets with: `prover::MAX_CACHED_KEYS`)
    pub fn pcdhip_g16_pk_memory(pk: *const pcdhip_g16_pk, out: *mut u64) -> c_int;
    pub fn pcdhip_groth16_prove(ctx: *mut pcdhip_ctx, pk: *const pcdhip_g16_pk, a: *const pcdhip_csr, b: *const pcdhip_csr, c: *const pcdhip_csr,
                                z: *const u64, r: *const u64, s: *const u64, proof: *mut u64, inf: *mut u8) -> c_int;
    // key memory: the second layout of a key's assignment queries (a window per proof; INTEGRATION.md "Key memory"): -1 automatic, 0 never, 6..22 bits
    pub fn pcdhip_groth16_set_sparse_window(ctx: *mut pcdhip_ctx, bits: c_int) -> c_int;
    // 8f rank 2: generate_parameters after synthesis
    pub fn pcdhip_groth16_setup(ctx: *mut pcdhip_ctx, curve: c_int, a: *const pcdhip_csr, b: *const pcdhip_csr, c: *const pcdhip_csr,
                                num_vars: usize, num_inputs: usize, g1_xy: *const u64, g2_xy: *const u64, toxic: *const u64,
                                out: *mut pcdhip_g16_setup_out) -> c_int;
    // K6 + 8f rank 3: process_vk, verify_with_processed_vk (n proofs), random-linear-combination batch
    pub fn pcdhip_process_vk(ctx: *mut pcdhip_ctx, curve: c_int, alpha_g1: *const u64, beta_g2: *const u64, gamma_g2: *const u64, delta_g2: *const u64,
                             gamma_abc_g1: *const u64, gamma_abc_inf: *const u8, num_inputs: usize, out: *mut *mut pcdhip_pvk) -> c_int;
    pub fn pcdhip_pvk_free(ctx: *mut pcdhip_ctx, pvk: *mut pcdhip_pvk);
    pub fn pcdhip_groth16_verify_prepared(ctx: *mut pcdhip_ctx, pvk: *const pcdhip_pvk, n_proofs: usize, public_inputs: *const u64,
                                          proofs: *const u64, proofs_inf: *const u8, ok: *mut c_int) -> c_int;
    pub fn pcdhip_groth16_verify_batch_rlc(ctx: *mut pcdhip_ctx, pvk: *const pcdhip_pvk, n_proofs: usize, public_inputs: *const u64,
                                           proofs: *const u64, proofs_inf: *const u8, rho: *const u64, all_ok: *mut c_int) -> c_int;
    // K8: vector algebra for Marlin's AHP rounds (batch_inversion[_and_mul], pointwise product, divide_by_vanishing_poly, &p * &q)
    pub fn pcdhip_vec_mul(ctx: *mut pcdhip_ctx, a: *const pcdhip_buf, b: *const pcdhip_buf, n: usize, out: *mut pcdhip_buf) -> c_int;
    pub fn pcdhip_vec_batch_inverse(ctx: *mut pcdhip_ctx, input: *const pcdhip_buf, n: usize, scale_mont: *const u64, out: *mut pcdhip_buf) -> c_int;
    pub fn pcdhip_poly_div_vanishing(ctx: *mut pcdhip_ctx, p: *const pcdhip_buf, len: usize, domain_n: usize, q: *mut pcdhip_buf, q_len: *mut usize,
                                     r: *mut pcdhip_buf, r_len: *mut usize) -> c_int;
    pub fn pcdhip_poly_mul(ctx: *mut pcdhip_ctx, a: *const pcdhip_buf, la: usize, b: *const pcdhip_buf, lb: usize, out: *mut pcdhip_buf,
                           out_len: *mut usize) -> c_int;
    // K7 commit side: KZG10::commit / the loop of MarlinKZG10::commit, polynomials and blinding polynomials resident on the device
    pub fn pcdhip_kzg_commit(ctx: *mut pcdhip_ctx, powers_of_g: *const pcdhip_bases, powers_of_gamma_g: *const pcdhip_bases,
                             shifted_powers_of_g: *const pcdhip_bases, items: *const pcdhip_kzg_commit_item, k: usize, comm_xy: *mut u64,
                             comm_inf: *mut u8, shifted_xy: *mut u64, shifted_inf: *mut u8, trimmed_len: *mut u64) -> c_int;
    pub fn pcdhip_kzg_commit_last_plan(ctx: *mut pcdhip_ctx, out: *mut u64) -> c_int;
    // K10: the Marlin index on device (row / col / row_col / val of A, B, C on K and B, the twelve commitments) and the two device
    // transforms it is made of
    pub fn pcdhip_marlin_index_build(ctx: *mut pcdhip_ctx, field: c_int, a: *const pcdhip_csr, b: *const pcdhip_csr, c: *const pcdhip_csr,
                                     num_cols: usize, domain_h_n: usize, domain_x_n: usize, domain_k_n: usize, domain_b_n: usize, keep: c_int,
                                     out: *mut *mut pcdhip_marlin_index) -> c_int;
    pub fn pcdhip_marlin_index_free(ctx: *mut pcdhip_ctx, index: *mut pcdhip_marlin_index);
    pub fn pcdhip_marlin_index_info(index: *const pcdhip_marlin_index, out: *mut u64) -> c_int;
    pub fn pcdhip_marlin_index_timings(index: *const pcdhip_marlin_index, out_ms: *mut f32) -> c_int;
    pub fn pcdhip_marlin_index_vec(index: *const pcdhip_marlin_index, form: c_int, matrix: c_int, poly: c_int, out: *mut *const pcdhip_buf) -> c_int;
    pub fn pcdhip_marlin_index_commit(ctx: *mut pcdhip_ctx, index: *const pcdhip_marlin_index, powers_of_g: *const pcdhip_bases, comm_xy: *mut u64,
                                      comm_inf: *mut u8) -> c_int;
    pub fn pcdhip_fft_general_dev(ctx: *mut pcdhip_ctx, data: *mut pcdhip_buf, n: usize, inverse: c_int, coset: c_int) -> c_int;
    pub fn pcdhip_poly_evals_on_domain(ctx: *mut pcdhip_ctx, p: *const pcdhip_buf, len: usize, domain_n: usize, coset: c_int,
                                       out: *mut pcdhip_buf) -> c_int;
    // K11: Marlin's round 1 (the assignment on H, z_A / z_B over the forward matrices, w, hiding) and the first sumcheck (q in one
    // launch, h_1, g_1); forms: bit 0 the transposed matrices of t(X), bit 1 the forward ones
    pub fn pcdhip_marlin_mats_upload_ex(ctx: *mut pcdhip_ctx, field: c_int, a: *const pcdhip_csr, b: *const pcdhip_csr, c: *const pcdhip_csr,
                                        num_cols: usize, domain_h_n: usize, domain_x_n: usize, forms: u32,
                                        out: *mut *mut pcdhip_marlin_mats) -> c_int;
    pub fn pcdhip_marlin_mats_free(ctx: *mut pcdhip_ctx, mats: *mut pcdhip_marlin_mats);
    pub fn pcdhip_marlin_zm_evals(ctx: *mut pcdhip_ctx, mats: *const pcdhip_marlin_mats, z: *const pcdhip_buf, za_out: *mut pcdhip_buf,
                                  zb_out: *mut pcdhip_buf, zc_out: *mut pcdhip_buf) -> c_int;
    pub fn pcdhip_marlin_place_assignment(ctx: *mut pcdhip_ctx, field: c_int, domain_h_n: usize, domain_x_n: usize, z: *const pcdhip_buf,
                                          num_cols: usize, out: *mut pcdhip_buf) -> c_int;
    pub fn pcdhip_poly_add_vanishing_multiple(ctx: *mut pcdhip_ctx, p: *mut pcdhip_buf, len: usize, blind_mont: *const u64, k: usize,
                                              domain_n: usize, out_len: *mut usize) -> c_int;
    pub fn pcdhip_marlin_sumcheck1_q(ctx: *mut pcdhip_ctx, eta_mont: *const u64, za: *const pcdhip_buf, zb: *const pcdhip_buf,
                                     r_alpha: *const pcdhip_buf, t: *const pcdhip_buf, z: *const pcdhip_buf, n: usize,
                                     q_out: *mut pcdhip_buf) -> c_int;
    pub fn pcdhip_marlin_round1(ctx: *mut pcdhip_ctx, mats: *const pcdhip_marlin_mats, z: *const pcdhip_buf, blind_w_mont: *const u64, k_w: usize,
                                blind_a_mont: *const u64, k_a: usize, blind_b_mont: *const u64, k_b: usize, x_hat: *mut pcdhip_buf,
                                z_poly: *mut pcdhip_buf, w: *mut pcdhip_buf, w_rem: *mut pcdhip_buf, za_poly: *mut pcdhip_buf,
                                zb_poly: *mut pcdhip_buf, za_evals: *mut pcdhip_buf, zb_evals: *mut pcdhip_buf, out_lens: *mut usize) -> c_int;
    pub fn pcdhip_marlin_sumcheck1(ctx: *mut pcdhip_ctx, mats: *const pcdhip_marlin_mats, eta_mont: *const u64, alpha_mont: *const u64,
                                   za_poly: *const pcdhip_buf, len_za: usize, zb_poly: *const pcdhip_buf, len_zb: usize,
                                   z_poly: *const pcdhip_buf, len_z: usize, mask: *const pcdhip_buf, len_mask: usize, domain_d_n: usize,
                                   t_poly: *mut pcdhip_buf, h1: *mut pcdhip_buf, g1: *mut pcdhip_buf, sigma: *mut pcdhip_buf,
                                   out_lens: *mut usize) -> c_int;
    // K12: Marlin's second sumcheck (q = a - b f in one launch; f, g_2 and h_2 from an index); row / col / row_col / val: arrays of
    // three buffers each, row_col or its entries nullable; route: 0 auto, 1 pointwise on B, 2 by the polynomial product
    pub fn pcdhip_marlin_sumcheck2_q(ctx: *mut pcdhip_ctx, alpha_mont: *const u64, beta_mont: *const u64, coeff_mont: *const u64,
                                     row: *const *const pcdhip_buf, col: *const *const pcdhip_buf, row_col: *const *const pcdhip_buf,
                                     val: *const *const pcdhip_buf, f: *const pcdhip_buf, n: usize, q_out: *mut pcdhip_buf) -> c_int;
    pub fn pcdhip_marlin_sumcheck2(ctx: *mut pcdhip_ctx, index: *const pcdhip_marlin_index, alpha_mont: *const u64, beta_mont: *const u64,
                                   coeff_mont: *const u64, route: c_int, f_poly: *mut pcdhip_buf, g2: *mut pcdhip_buf,
                                   sigma: *mut pcdhip_buf, h2: *mut pcdhip_buf, h2_rem: *mut pcdhip_buf, out_lens: *mut usize) -> c_int;
}

/// `PCDHIP_E_*` (include/pcdhip.h)
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Error { Arg, SizeUnsupported, NoDevice, Oom, Hip }
pub fn check(rc: c_int) -> Result<(), Error> {
    match rc { 0 => Ok(()), -1 => Err(Error::Arg), -2 => Err(Error::SizeUnsupported), -3 => Err(Error::NoDevice), -4 => Err(Error::Oom), _ => Err(Error::Hip) }
}
impl core::fmt::Display for Error {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result { write!(f, "pcdhip: {:?}", self) }
}
impl std::error::Error for Error {}
