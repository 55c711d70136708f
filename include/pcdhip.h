/* pcdhip.h -- C ABI of libpcdhip.so: MI355X (gfx950) prover arithmetic for arkworks-style PCD.
 *
 * Drop-in boundary for the hot path behind `ECCyclePCD::prove`
 * (/root/reference src/ec_cycle_pcd/mod.rs:92-181): the two calls `IC::MainSNARK::prove`
 * (mod.rs:171) and `IC::HelpSNARK::prove` (mod.rs:179) spend their time in upstream
 * ark-ec `VariableBaseMSM::multi_scalar_mul`, ark-poly `Radix2EvaluationDomain::{fft,ifft,
 * coset_fft,coset_ifft}_in_place` and ark-groth16 `R1CSToQAP::witness_map` / `create_proof`
 * (Cargo.toml:17-19,39: git dependencies, not vendored).  Each entry point below names the
 * upstream function it replaces; INTEGRATION.md shows the Rust `extern "C"` binding and the
 * `SNARK` impl (the plug-in seam `ECCyclePCDConfig`, mod.rs:24-33) that calls them.
 *
 * Encodings (exactly the in-memory image of the upstream types, so the Rust side is a memcpy):
 *   field element   L little-endian uint64_t limbs (L = 5 for the 298-bit fields, 12 for the
 *                   753-bit fields), Montgomery form with R = 2^(64 L)       [ark-ff Fp320/Fp768]
 *   scalar (MSM)    L limbs, canonical (non-Montgomery, reduced: < r)        [`into_repr()`]
 *   Fq2 / Fq3       consecutive base-field elements c0, c1 (, c2)
 *   affine point    x || y, infinity in a separate byte array (nullable = no point at infinity)
 *   Jacobian point  X || Y || Z, Z = 0 means infinity                        [GroupProjective]
 * Ownership: the caller owns every host buffer for the duration of the call only; device
 * objects are opaque handles with explicit free functions.  No RNG inside the library: the
 * Groth16 blinding factors r, s are inputs.  Thread-safety: one pcdhip_ctx per host thread;
 * handles may be shared by contexts on the same device once created.
 * Every function returns 0 on success or a negative PCDHIP_E_* code; nothing aborts or throws.
 * There is NO CPU fallback: without a usable GPU every call fails with PCDHIP_E_NO_DEVICE.
 */
#ifndef PCDHIP_H
#define PCDHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PCDHIP_MNT4_298 = 0, PCDHIP_MNT6_298 = 1, PCDHIP_MNT4_753 = 2, PCDHIP_MNT6_753 = 3 };  /* curve_id */
/* field_id: 0 = MNT4-298 Fq (= MNT6-298 Fr), 1 = MNT4-298 Fr (= MNT6-298 Fq),
 *           2 = MNT4-753 Fq (= MNT6-753 Fr), 3 = MNT4-753 Fr (= MNT6-753 Fq) */
enum { PCDHIP_F298A = 0, PCDHIP_F298B = 1, PCDHIP_F753A = 2, PCDHIP_F753B = 3 };
enum { PCDHIP_G1 = 1, PCDHIP_G2 = 2 };  /* group_id */

enum {
  PCDHIP_OK = 0,
  PCDHIP_E_ARG = -1,              /* null pointer / bad id / inconsistent sizes */
  PCDHIP_E_SIZE_UNSUPPORTED = -2, /* e.g. log_n above the field's 2-adicity (mixed-radix domain needed) */
  PCDHIP_E_NO_DEVICE = -3,
  PCDHIP_E_OOM = -4,
  PCDHIP_E_HIP = -5,              /* any other HIP runtime failure; see pcdhip_last_hip_error */
  PCDHIP_E_PREV_TICKET = -6       /* pcdhip_msm_submit_partial only: the PREVIOUS ticket of the slot had an unreduced scalar (its result is
                                     wrong); THIS submission was enqueued all the same and *ticket is valid */
};

typedef struct pcdhip_ctx pcdhip_ctx;
typedef struct pcdhip_bases pcdhip_bases;     /* device-resident affine base points (one query vector) */
typedef struct pcdhip_buf pcdhip_buf;         /* device-resident vector of field elements / scalars */
typedef struct pcdhip_g16_pk pcdhip_g16_pk;   /* device-resident Groth16 proving key */

const char* pcdhip_strerror(int code);
int pcdhip_device_count(void);
/* One context = one device + one HIP stream + reusable workspaces. */
int pcdhip_init(int device_id, pcdhip_ctx** out);
/* a context over a device LIST (one host thread drives all of them).  n_dev = 1 is pcdhip_init.  With more devices
 * the context shards by contiguous point range: pcdhip_bases_upload places range g of the vector on device g and
 * pcdhip_msm (host scalars) runs one MSM per device, gathers the partial results on device 0 over xGMI (peer copies) and sums them
 * there; pcdhip_g16_pk_upload shards every query the same way and pcdhip_groth16_prove runs the five MSMs of the proof on every
 * device over its range (the witness map on device 0, slices of h handed device to device) -- BASELINE configs[4]'s merge node,
 * "its MSMs use all GPUs".  Results are bit-identical to the single-device ones.  Independent PCD DAG branches need no such
 * context: one ordinary context per (host thread, device), N threads x N contexts (pcd_amd/dag.py).  The same id may appear more
 * than once (two logical shards on one device; the 1-GPU tests do that).  Device-resident scalars (pcdhip_msm_dev*) and the
 * FFT / pairing / setup entry points address device 0 only; handles created through a multi-device context belong to it. */
int pcdhip_init_devices(const int* device_ids, int n_dev, pcdhip_ctx** out);
int pcdhip_ctx_devices(const pcdhip_ctx* ctx);  /* number of devices of the context */
void pcdhip_destroy(pcdhip_ctx* ctx);
int pcdhip_sync(pcdhip_ctx* ctx);
/* Page-locked host memory for the buffers that cross PCIe on every proof (the assignment z: 42 MB at 2^20 x 298 bits):
 * host-to-device copies from it run at full PCIe rate and without a staging copy.  Optional -- every entry point
 * accepts ordinary host pointers. */
int pcdhip_host_alloc(size_t bytes, void** out);
void pcdhip_host_free(void* p);
const char* pcdhip_last_hip_error(pcdhip_ctx* ctx);
/* Static facts (no GPU needed). */
int pcdhip_field_limbs(int field_id);                 /* L */
int pcdhip_curve_base_field(int curve_id);            /* field_id of Fq */
int pcdhip_curve_scalar_field(int curve_id);          /* field_id of Fr */
int pcdhip_point_limbs(int curve_id, int group_id);   /* uint64 limbs per affine point (x||y) */

/* ---- device vectors ------------------------------------------------------------------------- */
int pcdhip_buf_upload(pcdhip_ctx* ctx, int field_id, const uint64_t* host, size_t n, pcdhip_buf** out);
int pcdhip_buf_alloc(pcdhip_ctx* ctx, int field_id, size_t n, pcdhip_buf** out);
int pcdhip_buf_download(pcdhip_ctx* ctx, const pcdhip_buf* buf, uint64_t* host, size_t n);
void pcdhip_buf_free(pcdhip_ctx* ctx, pcdhip_buf* buf);

/* ---- K3/K4: variable-base MSM ----------------------------------------------------------------
 * Replaces ark-ec `VariableBaseMSM::multi_scalar_mul(&bases[offset..offset+n], &scalars)`.
 * Bases are uploaded once (proving-key residency) and addressed by handle. */
int pcdhip_bases_upload(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xy_mont,
                        const uint8_t* inf_flags, size_t n, pcdhip_bases** out);
void pcdhip_bases_free(pcdhip_ctx* ctx, pcdhip_bases* bases);
int pcdhip_msm(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars_canonical,
               size_t n, uint64_t* out_xyz_mont);
/* Same with scalars already resident on the device (element `scalar_offset` onwards). */
int pcdhip_msm_dev(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars,
                   size_t scalar_offset, size_t n, uint64_t* out_xyz_mont);
/* Short MSMs without buckets (msm_short.hip.h): the same arguments, encodings and result as pcdhip_msm / pcdhip_msm_dev -- a Jacobian
 * point X || Y || Z with Z = 0 for the identity, the same affine image (the Jacobian representative may differ) -- at a cost that scales
 * with n: one mixed addition per set scalar bit over the handle's resident copies, then a chain of c * (windows per copy) doublings
 * (the scalar's bits on a handle without copies).  n == 0 gives the identity without a launch; n > 1024 PCDHIP_E_SIZE_UNSUPPORTED;
 * PCDHIP_E_ARG for offset + n beyond the vector, a wrong field, null pointers, an unreduced scalar and sharded bases.  Runs on the
 * context's own stream with a workspace of its own: outstanding MSM tickets are unaffected. */
int pcdhip_msm_short(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const uint64_t* scalars_canonical,
                     size_t n, uint64_t* out_xyz_mont);
int pcdhip_msm_short_dev(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars,
                         size_t scalar_offset, size_t n, uint64_t* out_xyz_mont);
/* k independent short MSMs over ONE handle as one launch chain: the hiding MSMs of a commit round, the vectors of a batch check, a
 * verifier's linear combinations of commitments.  One after the other, k short MSMs cost k serial chains of doublings on one wave
 * each; here every MSM gets its own wave of the same two or three launches, so the call costs about one chain.  Item j is
 *   out[j] = MSM(bases[base_offset .. base_offset + n), scalars[scalar_offset .. scalar_offset + n))
 * with the encodings and the result of pcdhip_msm_short: k Jacobian points X || Y || Z one behind the other, Z = 0 for the identity
 * (n == 0 gives it), the same affine image as pcdhip_msm.  Items may overlap and repeat; everything is read only.  The host form
 * uploads its scalars_n scalars once; the _dev form reads a resident buffer.  k == 0 succeeds without a launch; k > 1024 or an item
 * with n > 1024 gives PCDHIP_E_SIZE_UNSUPPORTED; PCDHIP_E_ARG for null pointers, an item's range beyond the handle or the scalars, a
 * buffer that is not of the curve's scalar field, sharded bases, and an unreduced scalar in ANY item -- the call then fails as a whole
 * (no result is valid) and the next call is clean.  One wait at the end, one copy back for all k. */
typedef struct {
  uint64_t base_offset;    /* first point of `bases` this MSM uses */
  uint64_t scalar_offset;  /* first element of the scalar array / buffer */
  uint64_t n;              /* pairs, 0 .. 1024; 0 gives the identity */
} pcdhip_msm_short_item;
int pcdhip_msm_short_batch(pcdhip_ctx* ctx, const pcdhip_bases* bases, const uint64_t* scalars_canonical, size_t scalars_n,
                           const pcdhip_msm_short_item* items, size_t k, uint64_t* out_xyz_mont /* k Jacobian points */);
int pcdhip_msm_short_batch_dev(pcdhip_ctx* ctx, const pcdhip_bases* bases, const pcdhip_buf* scalars,
                               const pcdhip_msm_short_item* items, size_t k, uint64_t* out_xyz_mont);
/* Opt-in routing: with max_n > 0 the witness MSMs of pcdhip_kzg_open and the two MSMs of pcdhip_kzg_check take the short path when
 * they cover at most max_n pairs (at most 1024), and the hiding MSMs of pcdhip_kzg_commit of at most max_n coefficients run as ONE
 * batched chain (pcdhip_msm_short_batch's kernels) instead of one bucket pipeline each.  Default 0: never -- those functions then run
 * exactly the code they ran before.  Vectors uploaded through a multi-device context are sharded and keep the bucket pipeline. */
int pcdhip_msm_set_short(pcdhip_ctx* ctx, size_t max_n);
/* Throughput form of pcdhip_msm_dev for a caller with several INDEPENDENT MSMs to make (the commitments of a Marlin round over one
 * resident committer key, BASELINE configs[3]; consecutive steps of a benchmark): submit enqueues the MSM on one of the context's four
 * side streams (own stream and workspace, round robin) and returns at once with a ticket; collect waits for that submission and
 * returns its result (PCDHIP_E_ARG as from pcdhip_msm_dev for an unreduced scalar).  The latency-bound bucket reduction of one MSM
 * then overlaps the sort and accumulation of the next.  At most four tickets may be outstanding (a fifth submit fails with
 * PCDHIP_E_ARG); pcdhip_groth16_prove refuses to run while any is (it uses the same side streams).  Not for sharded bases. */
int pcdhip_msm_submit(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset, size_t n,
                      int* ticket);
int pcdhip_msm_collect(pcdhip_ctx* ctx, int ticket, uint64_t* out_xyz_mont);
/* The same for the shard of a process-per-GPU run: the Jacobian partial is left in device memory of the caller
 * -- slot `*ticket` (0..3) of `out_xyz_device_slots`, four slots `slot_stride_bytes` apart: the send buffers of the RCCL
 * all-gather -- instead of coming back to the host, and pcdhip_msm_ticket_wait makes `other_stream` (a hipStream_t: the stream the
 * collective is enqueued on) wait for that MSM -- no host wait -- and frees the ticket.  Before a slot is written again its reader
 * must have been ordered in front of the context's stream (pcdhip_stream_wait direction 0), which every submission follows.
 * Several shard MSMs then overlap each other and the exchange of earlier ones, like pcdhip_msm_submit / collect on one GPU.
 * An unreduced scalar (PCDHIP_E_ARG from pcdhip_msm_dev) is reported on this path by the NEXT submission that reuses the ticket's slot, as
 * PCDHIP_E_PREV_TICKET: a code of its own, so that a pipelined caller can tell "an earlier MSM of this slot was wrong" from "this submission
 * was refused" -- the new submission IS enqueued and *ticket valid in that case.  pcdhip_msm_ticket_status polls a released ticket's word
 * without submitting (e.g. after the last step of a loop).  pcdhip_msm_submit never returns PCDHIP_E_PREV_TICKET: when it reuses a slot
 * whose last user was released by pcdhip_msm_ticket_wait it clears that slot's deferred word unreported (poll pcdhip_msm_ticket_status
 * first when mixing the two forms). */
int pcdhip_msm_submit_partial(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars, size_t scalar_offset,
                              size_t n, uint64_t* out_xyz_device_slots, size_t slot_stride_bytes, int* ticket);
int pcdhip_msm_ticket_wait(pcdhip_ctx* ctx, int ticket, void* other_stream);
/* The error word of the last MSM that used `slot` (0 .. 3) and was released by pcdhip_msm_ticket_wait: waits for that MSM, then
 * PCDHIP_OK, or PCDHIP_E_PREV_TICKET when one of its scalars was not reduced.  PCDHIP_E_ARG for a slot that is busy or was never released. */
int pcdhip_msm_ticket_status(pcdhip_ctx* ctx, int slot);
/* Precomputed window-shifted copies of bases uploaded AFTER this call through this context
 * (HBM capacity traded against the serial window combine; the proving key of a PCD is fixed for the whole
 * computation, so the one-time cost amortises over every step):
 *   -1 (default) one copy per scalar window: a single bucket window, no doubling chain at all;
 *    0           none (W bucket windows + Horner combine, as upstream);   k >= 2  k copies.
 * Falls back to fewer copies when device memory does not suffice (the Horner combine comes back for the windows that share a
 * copy); pcdhip_bases_info reports the number of copies a handle actually holds, so the fallback is never silent. */
int pcdhip_set_precompute(pcdhip_ctx* ctx, int mode);
/* Upper bound, in bytes, on what ONE base vector uploaded afterwards through this context may occupy with its copies (0, the
 * default: no bound other than the device's free memory).  A vector whose copies would exceed it gets fewer copies exactly as if
 * hipMalloc had failed (halving until it fits; at worst the plain vector, which is always accepted).  For hosts that keep several
 * proving keys resident: the full set of copies of ONE MNT4-753 key at 2^22 constraints is ~195 GB (BASELINE configs[4]). */
int pcdhip_set_precompute_budget(pcdhip_ctx* ctx, size_t bytes_per_vector);
/* The bound currently set (a layer that changes it for one upload puts the host's own setting back afterwards: rust/src/s2.rs). */
int pcdhip_get_precompute_budget(pcdhip_ctx* ctx, size_t* bytes_per_vector);
/* The plan an MSM of n pairs over these bases runs with (n = 0: the whole vector): signed-digit window bits c, scalar
 * windows W = ceil((bits + 1) / c), and how many window-shifted copies of the vector are resident (1 = none).  bench.py
 * prices the accumulate kernel's executed multiply-adds from it. */
int pcdhip_bases_info(const pcdhip_bases* bases, size_t n, int* window_bits, int* windows, int* copies);
/* Order the context's stream against a caller-owned HIP stream without a host wait (the RCCL stream of the exchange step,
 * SURVEY.md 8e): direction 0 -- work queued on the context's stream from now on waits for everything already queued on
 * `other_stream`; direction 1 -- `other_stream` waits for the context's stream.  `other_stream` is a hipStream_t (NULL =
 * the legacy default stream) of the same device and HIP runtime. */
int pcdhip_stream_wait(pcdhip_ctx* ctx, void* other_stream, int direction);
/* Tuning / introspection: window bits (0 = automatic), sorted entries per lane (0 = default). */
int pcdhip_msm_config(pcdhip_ctx* ctx, int window_bits, int chunk);
/* Sorting strategy of the (bucket, base) entries: 0 (default) MSD partition through LDS (per-workgroup bin
 * histograms, one global atomic per workgroup and bin, per-bin LDS counting sort); 1 single-pass binning into
 * per-bucket slots with an on-device fallback when a bucket overflows; 2 two-pass counting sort with one global
 * atomic per entry (also what small inputs use); 3 the partition of mode 0 with its direct write pass (entries stored
 * one by one into their bins) where mode 0 stages a tile's entries in LDS and writes whole bin runs: the A/B partner of
 * mode 0 and what it uses itself when no tile fits the LDS; 4 mode 0 with the two-read per-bin sort (every entry of a bin read twice,
 * every sorted index stored on its own) where modes 0 and 3 order a bin that fits the LDS there from one read and write it out in whole
 * lines: the A/B partner of mode 0 for that kernel (PCDHIP_BIN_STAGE=0 in the environment selects it for a whole process). */
int pcdhip_msm_set_sort(pcdhip_ctx* ctx, int mode);
/* Developer and test knob of the per-bin sort of modes 0 and 3: a bin of at most `cap` entries is ordered in LDS from one read, a larger
 * one takes the two-read form inside the same launch.  -1 (default): 18 432, what the LDS holds; 0: the two-read kernel of mode 4;
 * 1 .. 18 432: that threshold.  Results are identical for every value. */
int pcdhip_msm_set_bin_stage(pcdhip_ctx* ctx, int cap);
/* Form of the bucket accumulation.  mode 0 (default) and 1: running sums (Jacobian / XYZZ mixed additions); 2: for the 753-bit G1
 * groups a PAIR TREE of affine additions whose inversions are shared (5M + 1S per addition instead of 7M + 4S, one divstep inversion per
 * lane and level; msm.hip.h msm_pair_tree_kernel) -- measured -9 % on the accumulation and -5 % on an MSM of 2^20 uniform scalars,
 * +5 % on witness-like ones, hence opt-in; other groups ignore the setting.  chunk (0 = by size, else 2 .. 1024 entries
 * per lane; the per-wave scratch grows with it: ~12 GB for the whole chip at the default cap of 640) and min_pairs (0 = default 12: the
 * smallest batch an inversion is spent on) are tuning and test knobs.  Results are identical in every mode. */
int pcdhip_msm_set_accumulate(pcdhip_ctx* ctx, int mode, int chunk, int min_pairs);
/* Per-stage device time of the last MSM (HIP events on the context's stream), milliseconds:
 * [digits, scan, scatter, accumulate, fixup, tail, horner, total]; enable with on != 0. */
int pcdhip_msm_profile(pcdhip_ctx* ctx, int on);
int pcdhip_msm_last_timings(pcdhip_ctx* ctx, float out_ms[8]);
/* ... and what the device planned for that MSM: out[0] = entries of the sorted (bucket, base) list -- n x windows less the zero digits, the
 * scalars equal to zero or one and the bases at infinity --, out[1] = entries per lane of the accumulate kernel chosen for it. */
int pcdhip_msm_last_plan(pcdhip_ctx* ctx, uint32_t out[2]);
/* Measurement aid: the v_mad_u64_u32 issue rate of the context's device in lane-operations per second (four waves per SIMD, eight independent
 * chains per lane, ~1 ms) -- the roof bench.py prices the integer kernels against (`roofline_int.peak_live`), measured on the box at hand. */
int pcdhip_mad_rate(pcdhip_ctx* ctx, double* out_lane_mads_per_s);
/* Sum of n Jacobian points (the multi-GPU combine step after the all-gather of partial results). */
int pcdhip_points_sum(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz_mont, size_t n,
                      uint64_t* out_xyz_mont);
/* The same exchange without host round trips (bench.py / pcd_amd.dist at N > 1): pcdhip_msm_dev_partial leaves the Jacobian
 * result (X||Y||Z Montgomery limbs) in DEVICE memory owned by the caller -- the send buffer of the RCCL all-gather --
 * asynchronously on the context's stream (pcdhip_sync before another stream reads it); pcdhip_points_sum_dev sums n
 * Jacobian points that already sit in device memory (the receive buffer) and returns the sum to the host. */
int pcdhip_msm_dev_partial(pcdhip_ctx* ctx, const pcdhip_bases* bases, size_t offset, const pcdhip_buf* scalars,
                           size_t scalar_offset, size_t n, uint64_t* out_xyz_device);
int pcdhip_points_sum_dev(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz_device, size_t n,
                          uint64_t* out_xyz_mont);
/* Jacobian -> affine (x||y, flag) for n points, as `into_affine()`. */
int pcdhip_to_affine(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* xyz_mont, size_t n,
                     uint64_t* out_xy_mont, uint8_t* out_inf);

/* ---- K2: radix-2 FFT --------------------------------------------------------------------------
 * Replaces ark-poly Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}_in_place on a
 * domain of size 2^log_n: (inverse, coset) = (0,0) fft, (1,0) ifft, (0,1) coset_fft, (1,1) coset_ifft.
 * In place, natural order in and out, Montgomery form. */
int pcdhip_fft(pcdhip_ctx* ctx, int field_id, uint64_t* data_mont, uint32_t log_n, int inverse, int coset);
int pcdhip_fft_dev(pcdhip_ctx* ctx, pcdhip_buf* data, uint32_t log_n, int inverse, int coset);
/* K2m: ark-poly `GeneralEvaluationDomain` transforms on a domain of n = 2^a q^b elements (b <= 2; q = 7 for field
 * F298A, 5 for F753A: `MixedRadixEvaluationDomain`, what upstream selects for the HELP proof of a PCD step once its
 * circuit exceeds 2^17 / 2^15 rows); b = 0 is the radix-2 domain.  group_gen = GENERATOR^((p-1)/n). */
int pcdhip_fft_general(pcdhip_ctx* ctx, int field_id, uint64_t* data_mont, size_t n, int inverse, int coset);
/* n_ops transforms of ONE host vector, one after the other, with a single trip over PCIe (seam S2: ark-poly callers chain transforms on a
 * polynomial -- `ifft` then `coset_fft` in R1CSToQAP::witness_map and in Marlin's AHP rounds, reference path tests/mnt4_marlin.rs:141-204 --
 * and pcdhip_fft pays the 2 x n x 40 / 96 bytes per call).  ops[i]: bit 0 = inverse, bit 1 = coset; every transform over the domain of
 * n = 2^a q^b elements (GeneralEvaluationDomain).  Same results as n_ops calls of pcdhip_fft_general. */
int pcdhip_fft_seq(pcdhip_ctx* ctx, int field_id, uint64_t* data_mont, size_t n, const int* ops, int n_ops);
/* Size `GeneralEvaluationDomain::new(min_size)` would pick (0 if none exists): the witness map uses it. */
size_t pcdhip_domain_size(int field_id, size_t min_size);
/* Per-pass device time of the last transform; returns the number of passes written (<= 8). */
int pcdhip_fft_last_timings(pcdhip_ctx* ctx, float out_ms[8]);

/* ---- K1: Groth16 witness map -------------------------------------------------------------------
 * Replaces ark-groth16 `R1CSToQAP::witness_map` (libsnark reduction): h = (A z o B z - C z) / Z on
 * the domain `GeneralEvaluationDomain::new(num_constraints + num_inputs)` (radix-2, or mixed-radix for the help
 * fields beyond their 2-adicity; n = pcdhip_domain_size(...)); writes n elements of h. */
typedef struct {
  uint64_t num_rows;        /* = num_constraints */
  const uint64_t* row_ptr;  /* num_rows + 1 */
  const uint32_t* col;      /* nnz column (variable) indices */
  const uint64_t* coeff;    /* nnz coefficients, Montgomery limbs */
} pcdhip_csr;
int pcdhip_groth16_witness_map(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B,
                               const pcdhip_csr* C, const uint64_t* z_mont, size_t num_vars, size_t num_inputs,
                               uint64_t* h_out_mont);

/* ---- K1+K3+K4+K5: Groth16 prover arithmetic ----------------------------------------------------
 * Replaces the body of ark-groth16 `create_proof` after constraint synthesis (which stays in the
 * Rust host): witness map + 4 G1 MSMs + 1 G2 MSM + assembly with the caller's r, s. */
typedef struct {
  uint32_t curve_id, _pad;
  uint64_t num_vars;     /* m, including the leading 1 */
  uint64_t num_inputs;   /* including the leading 1 */
  uint64_t domain_size;  /* n */
  const uint64_t *alpha_g1, *beta_g1, *delta_g1;  /* vk.alpha_g1, pk.beta_g1, pk.delta_g1 */
  const uint64_t *beta_g2, *delta_g2;             /* vk.beta_g2, vk.delta_g2 */
  const uint64_t* a_query;    const uint8_t* a_inf;      /* m points */
  const uint64_t* b_g1_query; const uint8_t* b_g1_inf;   /* m */
  const uint64_t* b_g2_query; const uint8_t* b_g2_inf;   /* m */
  const uint64_t* h_query;    const uint8_t* h_inf;  uint64_t h_len;   /* n - 1 */
  const uint64_t* l_query;    const uint8_t* l_inf;  uint64_t l_len;   /* m - num_inputs */
} pcdhip_g16_pk_host;
int pcdhip_g16_pk_upload(pcdhip_ctx* ctx, const pcdhip_g16_pk_host* host, pcdhip_g16_pk** out);
void pcdhip_g16_pk_free(pcdhip_ctx* ctx, pcdhip_g16_pk* pk);
/* The MSM plan of a resident key's queries, in the order a, b_g1, b_g2, l, h: window bits and scalar windows (what a bench needs to count
 * the multiply-adds a proof executes; a key's large queries run one bit under the lone MSM's window, pcdhip_g16_pk_upload). */
int pcdhip_g16_pk_info(const pcdhip_g16_pk* pk, int window_bits[5], int windows[5]);
/* Device memory of a resident key's base vectors, in bytes: out[0] the five queries with their window-shifted copies (summed over the shards of a
 * multi-device key), out[1] the second layout for a shorter window (pcdhip_groth16_set_sparse_window; 0 when not built), out[2] / out[3] the
 * copies per point of the a query in the two layouts.  What a host that keeps several keys resident budgets with (T1). */
int pcdhip_g16_pk_memory(const pcdhip_g16_pk* pk, uint64_t out[4]);
/* Keep the circuit's constraint matrices (`ConstraintMatrices` from `cs.to_matrices()`, fixed per circuit like
 * the key) resident on the device; pcdhip_groth16_prove then accepts A = B = C = NULL and only the assignment
 * z crosses PCIe per proof. */
int pcdhip_g16_pk_set_r1cs(pcdhip_ctx* ctx, pcdhip_g16_pk* pk, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C);
/* `R1CSToQAP::witness_map` alone over the matrices resident with `pk`, with nothing else on the device: h_out (nullable) =
 * the n coefficients of h as from pcdhip_groth16_witness_map; out_ms (nullable) = device milliseconds of [the three mat-vecs,
 * the seven transforms + the pointwise step, both].  pcdhip_groth16_prove overlaps the same work with four of its MSMs. */
int pcdhip_g16_witness_map_resident(pcdhip_ctx* ctx, const pcdhip_g16_pk* pk, const uint64_t* z_mont, uint64_t* h_out_mont,
                                    float out_ms[3]);
/* proof_out = A (G1 x||y) || B (G2 x||y) || C (G1 x||y), affine Montgomery; inf_out[3].  A point at infinity has flag 1 and zero
 * coordinates; any of the three may be one (r = s = 0 is ark-groth16's create_proof_no_zk; A, B or C vanish for one value of r or s).
 * r_mont and s_mont are ABI Montgomery elements of the scalar field and must be reduced: limbs that, read as an integer, are not below
 * the modulus give PCDHIP_E_ARG before anything is queued (two elements compared on the host).  The entries of z_mont are NOT checked --
 * that would be a host pass over num_vars elements on the hot path; the caller hands over reduced elements. */
int pcdhip_groth16_prove(pcdhip_ctx* ctx, const pcdhip_g16_pk* pk, const pcdhip_csr* A, const pcdhip_csr* B,
                         const pcdhip_csr* C, const uint64_t* z_mont, const uint64_t* r_mont, const uint64_t* s_mont,
                         uint64_t* proof_out, uint8_t* inf_out);
/* Device time of the stages of the last prove, milliseconds:
 * [witness_map, msm_h, msm_l, msm_a, msm_b_g1, msm_b_g2, assembly, total]. */
int pcdhip_groth16_last_timings(pcdhip_ctx* ctx, float out_ms[8]);
/* How pcdhip_groth16_prove obtains the two variable-base products s*A and r*B_1 of upstream's assembly
 * (ark-groth16 create_proof, reached from src/ec_cycle_pcd/mod.rs:171,179); the proof is the same either way:
 *   2  one-lane windowed products queued behind the A / B_1 MSMs on high-priority streams, hidden under the longer
 *      MSMs (B in G2, h, l) of the same proof;
 *   1  folded into two more MSMs over the a / b_g1 bases with every scalar multiplied by s / r;
 *   0  (default) automatic: 2 for large proofs, 1 for small ones (<= 2^17 variables, 2^18 over the 753-bit fields). */
int pcdhip_groth16_set_assembly(pcdhip_ctx* ctx, int mode);
/* A window per PROOF for the four MSMs over the assignment (round 5).  The window of an MSM over a resident key is fixed by the key's
 * window-shifted copies and chosen for a dense scalar vector; the assignment of a verifier circuit (reference src/ec_cycle_pcd/data_structures.rs:269-304:
 * bit decompositions) is zeros and ones with a few per cent general scalars, and the bucket reduction of the dense window then costs more than the
 * additions.  OPT-IN (the second layout more than doubles a key's memory, upload and precompute time, and a host may keep several keys resident):
 * bits: 0 (default) never; -1 automatic: pcdhip_g16_pk_upload also lays the a / b_g1 / b_g2 / l queries out for a window four bits shorter when the key is a
 * whole key of at least 2^18 entries (2^14 over the 298-bit fields) on an ordinary context and the extra copies take at most a quarter of the device memory free at that moment
 * (9.2 GB for a 298-bit key of 2^20 entries, 54 GB for a 753-bit one); 6 .. 22: always, with that window.  Takes effect
 * at the next key upload.  pcdhip_groth16_prove counts the general scalars (neither 0 nor 1) of the assignment on the device and runs the four MSMs
 * on the shorter-window copies when they are at most an eighth of it (chained assembly only -- which a small 298-bit proof with such an assignment
 * then takes instead of the folded form its size would choose); the proof is the same either way.
 * pcdhip_groth16_last_plan: out[0] = 1 when the last proof took them, out[1] = its count of general scalars (0 when not counted). */
int pcdhip_groth16_set_sparse_window(pcdhip_ctx* ctx, int bits);
int pcdhip_groth16_last_plan(pcdhip_ctx* ctx, uint32_t out[2]);
/* Multi-device contexts with at least three devices: where the three independent chains of the witness map (a = A z, b = B z, c = C z:
 * mat-vec, ifft, coset fft each -- ark-groth16 `R1CSToQAP::witness_map`, SURVEY.md 8e "a || b || c on 3 GPUs") run.  1 (default): chain a on
 * device 0, b on device 1, c on device 2 (the matrices are resident on all three, pcdhip_g16_pk_set_r1cs), the two vectors come back
 * device to device, the pointwise step and the last transform run on device 0 -- about 45 % of the map's time leaves the critical path of
 * device 0, which also carries its share of the MSMs.  0: everything on device 0.  The proof is the same either way. */
int pcdhip_groth16_set_witness_split(pcdhip_ctx* ctx, int on);
/* Order of the stages of pcdhip_groth16_prove (what ark-groth16 `create_proof_with_reduction` does one after the other on rayon:
 * witness_map, then the five `VariableBaseMSM::multi_scalar_mul`; reference call sites src/ec_cycle_pcd/mod.rs:171,179).
 *   0 (default)  the four MSMs over the assignment first, each on its own stream, the witness map concurrently with them, the h MSM behind
 *      the map.  Measured in round 5 (profiles/r05_acc_probe_mnt4_298_2p20.txt, r05_pt_serial_lane8.txt): the proof takes the SUM of its kernels' standalone
 *      times to within a few per cent -- every kernel is bound by the same multiply-add issue slots, so no order can beat that sum;
 *   1  the witness map first with the device to itself, then all five MSMs at once (round 4's A/B knob; slower);
 *   2  the accumulate LANE (round 5): the map first while the MSMs sort beside it, then the MSMs' accumulate kernels one
 *      after the other on a stream confined by a CU mask to all but a few compute units (pcdhip_set_lane_reserve), each MSM's fix-up,
 *      bucket reduction and assembly products on a hardware queue of its own under the next accumulation.  A chain of one-wave launches
 *      no longer waits for accumulate workgroups to retire (0.98 ms instead of 20 .. 38 ms behind a device-filling grid,
 *      profiles/r05_k3_cu_mask.txt), but a masked queue runs the accumulate kernels 15 .. 45 % slower than an unmasked one (one CU less
 *      in one shader engine of every XCD unbalances the workgroup dispatch), and unmasked the lane is as fast as mode 0 at best:
 *      main proof MNT4-298 2^20: 15.7 (mode 0) / 18.0 (lane, 8 CUs reserved) / 16.4 .. 18.4 ms (lane, no mask); MNT4-753: 152 / 164 / 156.
 * The proof is the same in every mode.  Not while submitted MSMs are pending (PCDHIP_E_ARG). */
int pcdhip_groth16_set_schedule(pcdhip_ctx* ctx, int mode);
/* Compute units the accumulate lane leaves to the context's other streams (schedule 2; also pcdhip_msm_submit): a multiple of the number
 * of XCDs (8) keeps the same count free in every XCD.  -1 (default): the environment's PCDHIP_LANE_RESERVE, else 8; 0: no mask. */
int pcdhip_set_lane_reserve(pcdhip_ctx* ctx, int cus);

/* ---- the caller side of the path -- key generation -------------------------------------
 * Replaces ark-ec `FixedBaseMSM::{get_window_table, multi_scalar_mul}` + `batch_normalization_into_affine`:
 * out[i] = scalars[i] * base as affine points (x||y Montgomery, flag).  This is the primitive every query of
 * ark-groth16 `generate_parameters` is made of (reference call sites: circuit_specific_setup,
 * src/ec_cycle_pcd/mod.rs:69,78) and the KZG powers of `universal_setup` (mod.rs:346-354). */
int pcdhip_fixed_base_mul(pcdhip_ctx* ctx, int curve_id, int group_id, const uint64_t* base_xy_mont,
                          const uint64_t* scalars_canonical, size_t n, uint64_t* out_xy_mont, uint8_t* out_inf);
/* Replaces ark-groth16 `generate_parameters` (the body of `Groth16::circuit_specific_setup`, mod.rs:69,78) after
 * constraint synthesis, with the caller's randomness: toxic = [alpha, beta, gamma, delta, tau] (5 scalar-field
 * elements, Montgomery; tau must lie outside the evaluation domain, as upstream's
 * `sample_element_outside_domain` guarantees -- PCDHIP_E_ARG otherwise) and the two group generators.
 * All five elements must be reduced and alpha, beta, gamma, delta non-zero (tau = 0 is legal), checked on the host
 * before anything is queued -- PCDHIP_E_ARG otherwise: upstream unwraps the inverses of gamma and delta (a zero
 * would panic there, and give a key of identities here), and the six single points alpha_g1 .. delta_g2 carry no
 * infinity flag, so the identity cannot be returned in them.  A refused call leaves the context usable.
 * num_constraints = 0 is accepted (n = 1, no h); l_query / l_inf may be NULL when num_inputs == num_vars, h_query /
 * h_inf when n == 1.
 * QAP evaluation at tau (`instance_map_with_evaluation`: Lagrange coefficients, transposed mat-vecs) and every
 * fixed-base batch run on the device.  All output arrays are caller-allocated:
 * a / b_g1 / b_g2: num_vars points; gamma_abc_g1: num_inputs; l: num_vars - num_inputs;
 * h: n - 1 with n = pcdhip_domain_size(scalar field, num_constraints + num_inputs) (also returned in domain_size). */
typedef struct {
  uint64_t *alpha_g1, *beta_g1, *delta_g1;   /* one G1 point each */
  uint64_t *beta_g2, *gamma_g2, *delta_g2;   /* one G2 point each */
  uint64_t* a_query;      uint8_t* a_inf;
  uint64_t* b_g1_query;   uint8_t* b_g1_inf;
  uint64_t* b_g2_query;   uint8_t* b_g2_inf;
  uint64_t* h_query;      uint8_t* h_inf;
  uint64_t* l_query;      uint8_t* l_inf;
  uint64_t* gamma_abc_g1; uint8_t* gamma_abc_inf;
  uint64_t domain_size;   /* out */
} pcdhip_g16_setup_out;
int pcdhip_groth16_setup(pcdhip_ctx* ctx, int curve_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C,
                         size_t num_vars, size_t num_inputs, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont,
                         const uint64_t* toxic_mont, pcdhip_g16_setup_out* out);

/* ---- K6: pairing ---------------------------------------------------------------------------------
 * Replaces ark-ec `PairingEngine::product_of_pairings`: gt_out = final_exponentiation(prod_i miller_loop(P_i, Q_i)),
 * an element of Fq4 (MNT4) / Fq6 (MNT6) in tower order c0, c1 over Fq2 / Fq3, Montgomery limbs.  Up to 4096 pairs per call run ONE
 * WAVE PER PAIRING (the independent field products of every curve / tower step on sibling lanes, values in LDS: the latency of a
 * verification is what a merge node waits for); larger batches one lane per pair (64 pairings per wave: throughput). */
int pcdhip_multi_pairing(pcdhip_ctx* ctx, int curve_id, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                         const uint8_t* g2_inf, size_t n_pairs, uint64_t* gt_out);
/* 0 (default): as described above; 1: always the lane-per-pair kernels (A/B measurements, parity tests of both forms).  Applies to
 * every entry point that computes pairings (multi_pairing, the Groth16 verifications, process_vk). */
int pcdhip_pairing_set_mode(pcdhip_ctx* ctx, int mode);
/* Replaces ark-groth16 `Groth16::verify` (reference call site mod.rs:239):
 * e(A,B) == e(alpha,beta) e(gamma_abc[0] + sum_i x_i gamma_abc[i], gamma) e(C,delta); public inputs canonical, without the leading 1.
 * Canonical means reduced: every public input is an integer < r.  All four verifications (this one, _batch, _prepared, _batch_rlc)
 * compare each input with r on the host before anything is enqueued and return PCDHIP_E_ARG when one is >= r -- an error, not a
 * verdict of 0: x + r would otherwise verify wherever x does, and a caller must be able to tell a bad encoding from a bad proof. */
int pcdhip_groth16_verify(pcdhip_ctx* ctx, int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                          const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t num_inputs,
                          const uint64_t* public_inputs_canonical, const uint64_t* proof, const uint8_t* proof_inf, int* ok);

/* ---- `process_vk` and the verifications that use it --------------------------------------------------
 * pcdhip_process_vk replaces ark-groth16 `prepare_verifying_key` (`SNARK::process_vk`, reference call sites
 * src/ec_cycle_pcd/mod.rs:71,371,445,495,553): e(alpha, beta) is computed ONCE and kept, gamma and delta are negated, gamma_abc_g1
 * becomes a resident base vector with one 8-bit window table per point (0.86 / 5.2 MB each at 298 / 753 bits, keys of up to 256 public
 * inputs; larger keys keep the plain vector): the input accumulation of a verification is then a few dozen table additions per proof
 * on one workgroup, not a chain of hundreds of doublings.  (The G2 line coefficients upstream also precomputes are not stored: the
 * Miller-loop kernels fuse the G2 steps with the line evaluations, and a coefficient stream would be three times their state.) */
typedef struct pcdhip_pvk pcdhip_pvk;
int pcdhip_process_vk(pcdhip_ctx* ctx, int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                      const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t num_inputs, pcdhip_pvk** out);
void pcdhip_pvk_free(pcdhip_ctx* ctx, pcdhip_pvk* pvk);
/* `Groth16::verify_with_processed_vk` for n_proofs proofs under one key (`ECCyclePCD::verify`, mod.rs:239, once per prior message
 * of a merge node):  e(A, B) e(acc, -gamma) e(C, -delta) == e(alpha, beta)  -- three Miller loops and ONE final exponentiation per
 * proof (upstream's form; four and two without the prepared key), every Miller loop of the batch in one launch (3 n_proofs lanes),
 * the products and final exponentiations in another (one lane per proof); the input combinations acc_i = gamma_abc[0] + sum_j
 * x_ij gamma_abc[j] are n_proofs small MSMs over the resident gamma_abc vector.  Deterministic: ok[i] = 1 / 0 per proof.
 * public inputs: n_proofs x (num_inputs - 1) canonical scalars; proofs: n_proofs x (A || B || C); proofs_inf: n_proofs x 3 or NULL. */
int pcdhip_groth16_verify_prepared(pcdhip_ctx* ctx, const pcdhip_pvk* pvk, size_t n_proofs, const uint64_t* public_inputs_canonical,
                                   const uint64_t* proofs, const uint8_t* proofs_inf, int* ok);
/* The same n_proofs checks folded into ONE product with a SHARED final exponentiation, by a random linear combination with the
 * caller's challenges rho (n_proofs x 2 u64 limbs = 128 bits each, non-zero; the library draws no randomness):
 *   prod_i e(rho_i A_i, B_i) e(sum rho_i acc_i, -gamma) e(sum rho_i C_i, -delta) e(-(sum rho_i) alpha, beta) == 1
 * -- n_proofs + 3 Miller loops in one launch, one final exponentiation.  *all_ok = 1 iff the product is one: every proof valid,
 * or an invalid batch that slipped through with probability 2^-128 over rho.  On 0, pcdhip_groth16_verify_prepared finds the culprit.
 * A batch whose 3 n_proofs pairings all find a SIMD at once (wave-per-pairing mode, n_proofs <= 341) is answered by the n_proofs
 * deterministic checks side by side instead -- they take the time of one, less than the combination's scalings -- with the same
 * meaning of *all_ok (and no slip probability); rho is validated either way. */
int pcdhip_groth16_verify_batch_rlc(pcdhip_ctx* ctx, const pcdhip_pvk* pvk, size_t n_proofs, const uint64_t* public_inputs_canonical,
                                    const uint64_t* proofs, const uint8_t* proofs_inf, const uint64_t* rho, int* all_ok);

/* The native verifications of a merge node (`ECCyclePCD::verify`, mod.rs:239, once per prior
 * message) in one call = pcdhip_process_vk + pcdhip_groth16_verify_prepared + pcdhip_pvk_free.  Same verification key for all; public inputs:
 * n_proofs x (num_inputs - 1) canonical scalars; proofs: n_proofs x (A || B || C); proofs_inf: n_proofs x 3 flags or NULL.
 * ok[i] = 1 / 0 per proof -- deterministic, the same answers as n_proofs calls of pcdhip_groth16_verify. */
int pcdhip_groth16_verify_batch(pcdhip_ctx* ctx, int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2,
                                const uint64_t* gamma_g2, const uint64_t* delta_g2, const uint64_t* gamma_abc_g1,
                                const uint8_t* gamma_abc_inf, size_t num_inputs, size_t n_proofs,
                                const uint64_t* public_inputs_canonical, const uint64_t* proofs, const uint8_t* proofs_inf, int* ok);

/* ---- wire format ---------------------------------------------------------------------------
 * Replaces ark-serialize `CanonicalSerialize::{serialize, serialize_uncompressed}` / `CanonicalDeserialize` for
 * `GroupAffine` (G1 and G2 of the four curves), ark-groth16 `Proof` (A || B || C) and `VerifyingKey` (alpha_g1, beta_g2, gamma_g2,
 * delta_g2, u64 length + gamma_abc_g1): what a proof or key looks like when it leaves the process that made it.  Host-side
 * (no GPU, no context).  Field elements: canonical little-endian integers in ceil(bits / 8) bytes (38 / 95), Fq2 / Fq3 as c0, c1
 * (, c2); flags in the top bits of the last byte: 0x80 = y is the larger of (y, -y), 0x40 = infinity; compressed = x with flags,
 * uncompressed = x, y with flags.  Points at this ABI are x || y Montgomery limbs + a flag byte, as everywhere in this header.
 * Reading checks that coordinates are reduced, that the point lies on the curve (compressed: rebuilds y by a square root) and --
 * like upstream's checked `deserialize` -- that a G2 point lies in the prime-order subgroup ([r]Q = O; G1 has cofactor 1):
 * PCDHIP_E_ARG otherwise.  The subgroup test is one scalar multiplication on the host per G2 point (~10 ms at 298 bits, ~0.1 s at
 * 753 bits); pcdhip_deserialize_points_unchecked (= `deserialize_unchecked`: curve check only) is for bulk data a trusted party
 * wrote, e.g. a proving key.  Proofs and verifying keys are always checked.  Sizes are 0 for invalid ids. */
size_t pcdhip_serialized_size(int curve_id, int group_id, int compressed);  /* bytes of one point */
int pcdhip_serialize_points(int curve_id, int group_id, const uint64_t* xy_mont, const uint8_t* inf, size_t n, int compressed, uint8_t* out);
int pcdhip_deserialize_points(int curve_id, int group_id, const uint8_t* in, size_t n, int compressed, uint64_t* xy_mont, uint8_t* inf);
int pcdhip_deserialize_points_unchecked(int curve_id, int group_id, const uint8_t* in, size_t n, int compressed, uint64_t* xy_mont,
                                        uint8_t* inf);
size_t pcdhip_proof_serialized_size(int curve_id, int compressed);
int pcdhip_proof_serialize(int curve_id, const uint64_t* proof, const uint8_t* proof_inf, int compressed, uint8_t* out);
int pcdhip_proof_deserialize(int curve_id, const uint8_t* in, int compressed, uint64_t* proof, uint8_t* proof_inf);
size_t pcdhip_vk_serialized_size(int curve_id, size_t num_inputs, int compressed);
int pcdhip_vk_serialize(int curve_id, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2,
                        const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t num_inputs, int compressed, uint8_t* out);
/* gamma_abc arrays hold up to max_inputs points; the count found is returned in num_inputs */
int pcdhip_vk_deserialize(int curve_id, const uint8_t* in, size_t in_len, int compressed, uint64_t* alpha_g1, uint64_t* beta_g2, uint64_t* gamma_g2,
                          uint64_t* delta_g2, uint64_t* gamma_abc_g1, uint8_t* gamma_abc_inf, size_t max_inputs, size_t* num_inputs);

/* ---- K7 open side: KZG10 / MarlinKZG10 openings ------------------------------------------------------------------------
 * The open half of ark-poly-commit's KZG10 (the commit half is pcdhip_kzg_commit below).  Polynomials are
 * device vectors of ABI Montgomery coefficients, low degree first (lens[j] of them, at most the buffer's n); field elements are in
 * ABI Montgomery form, MSM scalars stay canonical.  Every division / evaluation runs on the device in three stream-ordered launches
 * (tile values, one carry scan, the tiles again from their carries); only the pairing check's scalar bookkeeping is on the host. */
/* ark-poly `evaluate`: out_mont[j] = polys[j](z), the k polynomials in one launch per phase (all of one field; len 0 gives 0) */
int pcdhip_poly_eval(pcdhip_ctx* ctx, const pcdhip_buf* const* polys, const size_t* lens, size_t k, const uint64_t* z_mont,
                     uint64_t* out_mont);
/* MarlinKZG10's combined polynomial: out_i = sum_j coeffs_j p_(j,i) for i < *out_len = max lens (out may be one of the inputs) */
int pcdhip_poly_lincomb(pcdhip_ctx* ctx, const pcdhip_buf* const* polys, const size_t* lens, const uint64_t* coeffs_mont, size_t k,
                        pcdhip_buf* out, size_t* out_len);
/* ark-poly `&p / &DensePolynomial([-z, 1])`: len-1 quotient coefficients (none for len <= 1), remainder = p(z).  q may be null when
 * len <= 1 and must not be p's buffer. */
int pcdhip_poly_div_linear(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, const uint64_t* z_mont, pcdhip_buf* q,
                           uint64_t* value_mont);
/* ark-poly-commit KZG10::open (+ p(z)): w = MSM(powers_of_g, p/(X-z)) + MSM(powers_of_gamma_g, blinding/(X-z)),
   random_v = blinding(z); blinding == NULL: no hiding part, random_v untouched.  w is Jacobian (X || Y || Z).  PCDHIP_E_ARG when
   a quotient has more coefficients than its bases (upstream's TooManyCoefficients), for a field that is not the curve's scalar
   field, and for sharded bases.  It runs on the context's own stream and workspaces, which MSM tickets do not use. */
int pcdhip_kzg_open(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g, const pcdhip_buf* p,
                    size_t len, const pcdhip_buf* blinding, size_t blinding_len, const uint64_t* z_mont, uint64_t* w_xyz_mont,
                    uint64_t* value_mont, uint64_t* random_v_mont);
/* KZG10::check (n == 1, randomizers may be NULL) and KZG10::batch_check (caller's randomizers, canonical, the first
   1 as upstream): ok = [ e(sum r_i (C_i + z_i W_i) - (sum r_i v_i) g - (sum r_i rv_i) gamma_g, h) == e(sum r_i W_i, beta_h) ].
   Affine G1 / G2 points (x || y, flags nullable); n == 0 is true. */
int pcdhip_kzg_check(pcdhip_ctx* ctx, int curve_id, const uint64_t* g_xy, const uint64_t* gamma_g_xy, const uint64_t* h_xy,
                     const uint64_t* beta_h_xy, size_t n, const uint64_t* comms_xy, const uint8_t* comms_inf, const uint64_t* points_mont,
                     const uint64_t* values_mont, const uint64_t* w_xy, const uint8_t* w_inf, const uint64_t* random_v_mont,
                     const uint64_t* randomizers_canonical, int* ok);

/* ---- K7 commit side: KZG10 / MarlinKZG10 commitments of device-resident polynomials ------------------------------------
 * Replaces ark-poly-commit `KZG10::commit` and the loop of `MarlinKZG10::commit` over the labeled polynomials of one AHP round
 * (SURVEY.md A.7), for polynomials that already live on the device as ABI Montgomery coefficients (what pcdhip_fft_dev, pcdhip_poly_mul,
 * pcdhip_poly_div_vanishing, pcdhip_poly_lincomb and pcdhip_vec_* leave): one launch turns all of them into the canonical scalars the MSMs
 * take and finds their trimmed lengths, up to four items' MSMs run side by side on the streams of pcdhip_msm_submit, the hiding MSMs
 * beside them, and one epilogue adds, normalises and copies back.  No coefficient crosses PCIe.  The library draws no randomness: the
 * blinding polynomials (`Randomness::blinding_polynomial`, and `shifted_rand` of a degree-bound commitment) are inputs.
 *   comm[j]    = MSM(powers_of_g[0 .. t_j), p_j) + MSM(powers_of_gamma_g[0 .. blinding_len), blinding_j)
 *   shifted[j] = MSM(shifted_powers_of_g[shifted_offset .. shifted_offset + t_j), p_j)
 *                + MSM(powers_of_gamma_g[0 .. shifted_blinding_len), shifted_blinding_j)                      (items with `shifted`)
 * with t_j the TRIMMED length of p_j: the index of its highest non-zero coefficient below len, plus one (0 for a zero or empty
 * polynomial) -- a device buffer is not trimmed as upstream's DensePolynomial is, so zeros at the top of len do not count against the
 * size checks.  trimmed_len[j] = t_j (nullable), which the caller needs as the length for pcdhip_kzg_open. */
typedef struct {
  const pcdhip_buf* poly;              /* ABI Montgomery coefficients, low degree first; may be NULL when len == 0 */
  uint64_t len;
  const pcdhip_buf* blinding;          /* NULL: the commitment is not hiding */
  uint64_t blinding_len;
  const pcdhip_buf* shifted_blinding;  /* NULL: the shifted commitment is not hiding (non-NULL only with `shifted`) */
  uint64_t shifted_blinding_len;
  uint64_t shifted_offset;             /* first element of shifted_powers_of_g this item uses (upstream: max_degree - degree_bound) */
  uint32_t shifted, _pad;              /* != 0: also produce the degree-bound ("shifted") commitment */
} pcdhip_kzg_commit_item;
/* Outputs: one affine point (x || y, ABI Montgomery) and one flag byte per item; the identity is flag 1 with zero coordinates, as
 * pcdhip_to_affine writes it; items without `shifted` get flag 1 in shifted_inf.  shifted_xy / shifted_inf may be NULL when no item is
 * shifted.  k == 0 succeeds without a launch.  PCDHIP_E_ARG (upstream's TooManyCoefficients / IncorrectDegreeBound) when t_j >
 * powers_of_g->n, shifted_offset + t_j > shifted_powers_of_g->n, or a blinding length exceeds powers_of_gamma_g->n; the first two are
 * found from the trimmed lengths that come back with the results, so the call then fails after the fact with no partial output
 * guaranteed.  Also PCDHIP_E_ARG: null required pointers, len beyond the buffer's n, a buffer that is not of the curve's scalar field,
 * handles of different curves or not G1, sharded handles, `shifted` or a blinding set while its handle (or shifted_xy / shifted_inf) is
 * NULL, and outstanding MSM tickets (the rule of pcdhip_groth16_prove: the call uses the same side streams and workspaces). */
int pcdhip_kzg_commit(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g /* nullable */,
                      const pcdhip_bases* shifted_powers_of_g /* nullable */, const pcdhip_kzg_commit_item* items, size_t k,
                      uint64_t* comm_xy, uint8_t* comm_inf, uint64_t* shifted_xy /* nullable */, uint8_t* shifted_inf /* nullable */,
                      uint64_t* trimmed_len /* nullable, k entries */);
/* Which path the last pcdhip_kzg_commit of this context took: out[0] = large MSMs run (one per non-empty polynomial, two with a
 * degree bound), out[1] = hiding MSMs that ran in the batched short chain (pcdhip_msm_set_short; at most 1024 of a call), out[2] = hiding
 * MSMs that ran one at a time (the bucket pipeline -- all of them under the default), out[3] = kernel launches of the batched chain
 * (2, or 3 when an MSM's planes take several workgroups; 0 without a batch). */
int pcdhip_kzg_commit_last_plan(pcdhip_ctx* ctx, uint64_t out[4]);

/* ---- K13: a round's openings as one queued call ---------------------------------------------------------------------------
 * The last prover step of a MarlinKZG10 proof, ark-poly-commit's `open_combinations` / `batch_open`, for polynomials that live on the
 * device.  ark-poly-commit is not vendored here: the formula below is the contract, and what is said about upstream's order (its
 * per-query accumulation over the labeled polynomials, the challenge xi_(j+1) on a degree-bound term) is restated from memory.
 *
 * Inputs: m items -- the records of pcdhip_kzg_commit: poly, len, blinding, shifted flag, shifted_offset, shifted_blinding -- and P
 * openings.  Opening o has a point z_o (points_mont[o]) and two vectors of m ABI Montgomery elements, row o of coeffs_mont and of
 * shifted_coeffs_mont (nullable: no degree-bound term anywhere):
 *   a_(o,i)  the caller's collapse of its linear combinations and opening challenges onto the items; zero: item i is not in opening o;
 *   s_(o,i)  non-zero only for items with `shifted`: the challenge that multiplies the item's degree-bound witness (upstream's xi_(j+1)).
 * A constant term of a linear combination never changes a quotient ((c - c) / (X - z) = 0), so the interface has none: the caller adds
 * it to the value.  For each opening
 *   p_o = sum_i a_(o,i) p_i                          (its length the longest len_i with a_(o,i) != 0)
 *   R_o = sum_i a_(o,i) blinding_i + sum_i s_(o,i) shifted_blinding_i
 *   W_o = MSM(powers_of_g,                              (p_o - p_o(z_o)) / (X - z_o))
 *       + sum_{i : s_(o,i) != 0} MSM(shifted_powers_of_g[shifted_offset_i ..], s_(o,i) (p_i - p_i(z_o)) / (X - z_o))
 *       + MSM(powers_of_gamma_g,                        (R_o - R_o(z_o)) / (X - z_o))
 *   value_o = p_o(z_o),   random_v_o = R_o(z_o).
 * Both hiding parts are over the same bases, powers_of_gamma_g, so they are ONE polynomial R_o and ONE hiding MSM per opening: the same
 * group element as upstream's two.  Lengths are taken as given (a device buffer is not trimmed): zeros at the top of len count.
 *
 * Every division of the call is a PART: the combined polynomial of each opening, R_o of each opening, and one single-term part per
 * (o, i) with s_(o,i) != 0.  All parts run in three launches (combine + tile values, one carry scan, the tiles again from their carries,
 * the canonical scalars scaled by s in the store); nothing waits for the host in between.
 * Limits (PCDHIP_E_ARG beyond): m <= 1024, P <= 64, at most 8 non-zero s_(o,i) per opening, every len below 2^31. */
/* The three launches alone, the testable core.  Tables of P x (2 + m) entries, entry [o][0] the combined polynomial, [o][1] R_o,
 * [o][2 + i] the degree-bound term of item i: q_bufs (device buffers of field_id for the quotients' CANONICAL scalars, times s for a
 * degree-bound term; an entry may be NULL when its part is absent or has a quotient of no coefficient, and q_bufs itself when all are),
 * q_lens (out: the quotients' lengths, len - 1; 0 for an absent part) and values_mont (out: the part at z_o -- p_i(z_o), unscaled, for a
 * degree-bound term; zero for an absent part).  A part is absent when no item with a buffer and len > 0 has a non-zero coefficient in
 * it.  It waits once, to return the values.  PCDHIP_E_ARG: null required pointers, a buffer of another field or shorter than its
 * length, s != 0 on an item without `shifted`, a quotient buffer that is missing, of another field or too short, the limits above;
 * nothing is written then.  P == 0 succeeds without a launch. */
int pcdhip_poly_open_quotients(pcdhip_ctx* ctx, int field_id, const pcdhip_kzg_commit_item* items, size_t m, size_t n_openings,
                               const uint64_t* points_mont, const uint64_t* coeffs_mont, const uint64_t* shifted_coeffs_mont /* nullable */,
                               pcdhip_buf* const* q_bufs, size_t* q_lens, uint64_t* values_mont);
/* The whole round: the three launches, every opening's large MSMs (the combined quotient, and one per degree-bound term over
 * shifted_powers_of_g from the item's shifted_offset) side by side on the streams of pcdhip_msm_submit, the hiding MSMs as ONE batched
 * short chain under pcdhip_msm_set_short (one at a time otherwise), one epilogue that adds, normalises and copies back, ONE wait at the
 * end.  Per opening: the affine W_o (x || y, ABI Montgomery) with its flag (the identity is flag 1 with zero coordinates), value_o and
 * random_v_o (zero without a blinding).  An opening whose coefficients are all zero gives the identity and zero values.  P == 0
 * succeeds without a launch.
 * PCDHIP_E_ARG, with no output written: a combined quotient (len - 1 coefficients) longer than powers_of_g->n (upstream's
 * TooManyCoefficients); shifted_offset + len - 1 above shifted_powers_of_g->n; R_o's quotient longer than powers_of_gamma_g->n;
 * s != 0 on an item without `shifted`, or while shifted_powers_of_g is NULL; a blinding with a non-zero coefficient while
 * powers_of_gamma_g is NULL; buffers that are not of the curve's scalar field; handles of different curves or not G1; sharded handles;
 * outstanding MSM tickets (the rule of pcdhip_kzg_commit: the same side streams and workspaces); the limits above. */
int pcdhip_kzg_batch_open(pcdhip_ctx* ctx, const pcdhip_bases* powers_of_g, const pcdhip_bases* powers_of_gamma_g /* nullable */,
                          const pcdhip_bases* shifted_powers_of_g /* nullable */, const pcdhip_kzg_commit_item* items, size_t m,
                          size_t n_openings, const uint64_t* points_mont, const uint64_t* coeffs_mont,
                          const uint64_t* shifted_coeffs_mont /* nullable */, uint64_t* w_xy, uint8_t* w_inf, uint64_t* values_mont,
                          uint64_t* random_v_mont);
/* Which path the last pcdhip_kzg_batch_open of this context took: out[0] = large MSMs run, out[1] = hiding MSMs in the batched short
 * chain, out[2] = hiding MSMs that ran one at a time, out[3] = launches of the division chain (3; 2 when every part is a constant; 0
 * without a part). */
int pcdhip_kzg_batch_open_last_plan(pcdhip_ctx* ctx, uint64_t out[4]);

/* ---- K14: the MarlinKZG10 check, a round's openings verified in one call -------------------------------------------------
 * The verifier's half of K13: ark-poly-commit's `MarlinKZG10::check_combinations` -> `batch_check`, the group and pairing work on the
 * device (the verifier's scalar checks stay with the caller).  ark-poly-commit is not vendored here: the equation below is the
 * contract.
 *
 * Inputs: m commitments comm_i; for the items with a degree bound a shifted commitment shifted_i and the index k(i) of the key's shift
 * power S_k(i) = shifted_powers_of_g[shifted_offset_i] (upstream's `get_shift_power(bound)`), shift_index[i] = -1 for an item without a
 * bound; and P openings.  Opening o has a point z_o, row o of the SAME two P x m tables that pcdhip_kzg_batch_open takes -- a_(o,i), and
 * s_(o,i), non-zero only on degree-bound items: a prover's tables serve the verifier unchanged -- the claimed value_o and random_v_o, the
 * claimed individual values v_(o,i) = p_i(z_o) wherever s_(o,i) != 0 (item_values_mont, P x m, read nowhere else), and the witness W_o.
 *   C_o   = sum_i a_(o,i) comm_i + sum_i s_(o,i) (shifted_i - v_(o,i) S_k(i))
 *   L_o   = C_o - value_o g - random_v_o gamma_g + z_o W_o
 *   check : e(L_o, h) == e(W_o, beta_h)
 * Equation e of E combines the openings with row e of an E x P matrix of randomizers rho: e(sum_o rho_o L_o, h) == e(sum_o rho_o W_o, beta_h).
 * Each side is ONE MSM over the N = 2 + n_shift + 2 m + P points
 *   [0] g   [1] gamma_g   [2 + k] S_k   [2 + n_shift + i] comm_i   [2 + n_shift + m + i] shifted_i   [2 + n_shift + 2 m + o] W_o
 * with the left scalars
 *   g: -sum_o rho_o value_o    gamma_g: -sum_o rho_o random_v_o    S_k: -sum_o sum_{i : k(i) = k} rho_o s_(o,i) v_(o,i)
 *   comm_i: sum_o rho_o a_(o,i)    shifted_i: sum_o rho_o s_(o,i)    W_o: rho_o z_o
 * and the right scalars rho_o over the W range.  Two modes:
 *   combined     (randomizers_canonical given: P canonical scalars, the first one 1 as upstream draws them; the library draws none):
 *                E = 1, one verdict in ok[0] -- upstream's batch_check;
 *   per-opening  (randomizers_canonical == NULL): E = P, rho the identity matrix, ok[o] per opening, deterministic -- what finds the
 *                culprit after a combined 0.
 * Encodings are those of pcdhip_kzg_batch_open and pcdhip_kzg_check: affine points x || y in ABI Montgomery form with nullable flag
 * bytes (a flagged point, and one with all-zero coordinates, is the identity), field elements in ABI Montgomery form, randomizers
 * canonical.
 *
 * Refusals -- a bad encoding is an argument error, never a verdict; `ok` is left untouched on any error:
 *   PCDHIP_E_SIZE_UNSUPPORTED  P > 64, or N > 1024 (the short MSM's limit);
 *   PCDHIP_E_ARG, found on the host before anything is queued: null required pointers; any field input not reduced (>= r), Montgomery
 *                tables and randomizers alike (item values where s != 0); s != 0 on an item whose shift_index is -1 or >= n_shift, or
 *                while shift_index, shifted_xy or item_values_mont is NULL; random_v_mont given while the key has no gamma_g.
 * A multi-device context addresses its device 0.  Everything runs on the context's own stream and its short-MSM workspace, which MSM
 * tickets do not use. */
typedef struct pcdhip_kzg_vk pcdhip_kzg_vk;
/* The prepared verifier key: g, gamma_g (nullable: a key without hiding) and the n_shift shift powers resident in the device image in
 * front of the range for a call's fresh points; h, beta_h and GT's one.  After it no call allocates or frees device memory, except to
 * grow the key's scratch to the largest call seen (a Marlin-sized round fits from the start).  PCDHIP_E_SIZE_UNSUPPORTED for n_shift >
 * 1022. */
int pcdhip_kzg_vk_prepare(pcdhip_ctx* ctx, int curve_id, const uint64_t* g_xy, const uint64_t* gamma_g_xy /* nullable */, const uint64_t* h_xy,
                          const uint64_t* beta_h_xy, const uint64_t* shift_powers_xy /* n_shift points; nullable with n_shift == 0 */,
                          size_t n_shift, pcdhip_kzg_vk** out);
void pcdhip_kzg_vk_free(pcdhip_ctx* ctx, pcdhip_kzg_vk* vk);
/* The check.  One staged upload, one chain of launches (the fresh points into the device image, the scalar collapse, 2 E short MSMs
 * over the key's vector as one batch, the hand-over of their Jacobian results to the pairing -- no inversion --, E two-pair pairings),
 * one download, ONE wait.  ok: E verdicts (1 in combined mode, P per opening).  n_openings == 0 is true (ok[0] = 1) without a launch.
 * Under pcdhip_pairing_set_mode(ctx, 1) the sums are normalised by one more launch; the verdicts are the same. */
int pcdhip_kzg_check_combinations(pcdhip_ctx* ctx, pcdhip_kzg_vk* vk, size_t m, const uint64_t* comm_xy, const uint8_t* comm_inf /* nullable */,
                                  const uint64_t* shifted_xy /* nullable */, const uint8_t* shifted_inf /* nullable */,
                                  const int32_t* shift_index /* m entries, -1: no bound; nullable */, size_t n_openings,
                                  const uint64_t* points_mont, const uint64_t* coeffs_mont, const uint64_t* shifted_coeffs_mont /* nullable */,
                                  const uint64_t* values_mont, const uint64_t* random_v_mont /* nullable */,
                                  const uint64_t* item_values_mont /* P x m, nullable; read only where s != 0 */, const uint64_t* w_xy,
                                  const uint8_t* w_inf /* nullable */, const uint64_t* randomizers_canonical /* nullable: per-opening mode */,
                                  int* ok);
/* The scalar collapse alone, the testable core: the same tables of a field (no key: n_shift is an argument) -> the E x N left and the
 * E x P right canonical scalars, in the order of the vector above.  It waits once, to return them.  The refusals of the check that need
 * no points; n_openings == 0 succeeds without a launch. */
int pcdhip_kzg_check_scalars(pcdhip_ctx* ctx, int field_id, size_t n_shift, size_t m, const int32_t* shift_index /* nullable */,
                             size_t n_openings, const uint64_t* points_mont, const uint64_t* coeffs_mont,
                             const uint64_t* shifted_coeffs_mont /* nullable */, const uint64_t* values_mont,
                             const uint64_t* random_v_mont /* nullable */, const uint64_t* item_values_mont /* nullable */,
                             const uint64_t* randomizers_canonical /* nullable */, uint64_t* left_canonical, uint64_t* right_canonical);
/* What the last pcdhip_kzg_check_combinations of this context ran: out[0] = equations, out[1] = pairs of the left MSM (N), out[2] =
 * kernel launches of the chain (7; 8 when the left MSM's planes take several workgroups, one more in pairing mode 1), out[3] = host
 * waits (1). */
int pcdhip_kzg_check_combinations_last_plan(pcdhip_ctx* ctx, uint64_t out[4]);

/* ---- K8 vector algebra for Marlin's AHP rounds ---------------------------------------------------------------------------
 * What the prover does with a polynomial between its transforms and its commitments, on device vectors of ABI Montgomery elements.
 * All buffers of one call are of the same field and a count may not exceed a buffer's n (PCDHIP_E_ARG otherwise, as for null
 * pointers).  Everything runs on the context's own stream and workspaces, which MSM tickets do not use; a multi-device context
 * addresses its device 0. */
/* the pointwise product: out_i = a_i b_i for i < n (out may be a or b, and a may be b) */
int pcdhip_vec_mul(pcdhip_ctx* ctx, const pcdhip_buf* a, const pcdhip_buf* b, size_t n, pcdhip_buf* out);
/* ark-ff `batch_inversion` (scale_mont == NULL) / `batch_inversion_and_mul`: out_i = scale / in_i for in_i != 0 and out_i = 0 for
 * in_i == 0 (upstream leaves zeros in place).  Montgomery's trick per tile of the vector, one kernel; out may be in; n == 0 is fine. */
int pcdhip_vec_batch_inverse(pcdhip_ctx* ctx, const pcdhip_buf* in, size_t n, const uint64_t* scale_mont, pcdhip_buf* out);
/* ark-poly `DensePolynomial::divide_by_vanishing_poly`: the unique q, r with p = q (X^domain_n - 1) + r and deg r < domain_n, for any
 * domain_n >= 1 (not only domain sizes).  *q_len = len > domain_n ? len - domain_n : 0 coefficients of q, *r_len = min(len, domain_n)
 * of r; r and r_len may be NULL, q may be NULL when *q_len == 0.  q and r must not be p's buffer nor each other.  One lane per
 * coefficient sums its stride-domain_n column of p: a single streaming pass for len up to a few domain_n, and a cost that grows with
 * len / domain_n beyond that. */
int pcdhip_poly_div_vanishing(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, size_t domain_n, pcdhip_buf* q, size_t* q_len,
                              pcdhip_buf* r, size_t* r_len);
/* ark-poly `&DensePolynomial * &DensePolynomial`: *out_len = la + lb - 1 coefficients (0 when la == 0 or lb == 0), NOT trimmed of
 * leading zeros as upstream's result is.  Two forward transforms, a pointwise product and an inverse transform over the domain
 * pcdhip_domain_size(field, la + lb - 1); PCDHIP_E_SIZE_UNSUPPORTED when that is 0.  out may be a or b. */
int pcdhip_poly_mul(pcdhip_ctx* ctx, const pcdhip_buf* a, size_t la, const pcdhip_buf* b, size_t lb, pcdhip_buf* out, size_t* out_len);

/* ---- K9 Marlin's AHP rounds 2 and 3: r(alpha, .), t(X) and the rational sumcheck -----------------------------------------------
 * What ark-marlin's prover computes between its first commitments and its openings, besides the transforms, K8 and the commitments:
 * on device vectors of ABI Montgomery elements of ONE field, on the context's own stream and workspaces (a multi-device context
 * addresses its device 0).  Null pointers, a count beyond a buffer's n and mixed fields give PCDHIP_E_ARG.  These calls only QUEUE
 * their launches: none waits for the device (pcdhip_buf_download, pcdhip_sync and every K7 / K8 call do), and nothing of size n or nnz
 * is computed on the host per call.  Field elements of the host (x, eta, alpha, beta, the coefficients) are ABI Montgomery limbs. */
/* ark-marlin `batch_eval_unnormalized_bivariate_lagrange_poly_with_diff_inputs`: out_i = (x^domain_n - 1) / (x - w^i) for i < domain_n,
 * w the generator the resident transform of that size uses (radix-2 or mixed-radix).  domain_n must be a domain size
 * (pcdhip_domain_size(field_id, domain_n) == domain_n), PCDHIP_E_SIZE_UNSUPPORTED otherwise.  When x lies in the domain EVERY output is
 * 0, as upstream's formula gives it: the batch inversion leaves the zero difference in place, and the scale x^domain_n - 1 is 0.
 * Two launches: the differences, then the batch inversion of pcdhip_vec_batch_inverse with that scale. */
int pcdhip_domain_bivariate_lagrange(pcdhip_ctx* ctx, int field_id, size_t domain_n, const uint64_t* x_mont, pcdhip_buf* out);
/* The three constraint matrices of an index, resident for t(X): transposed on the host (an index permutation) with the variables at
 * their places in H, pi = ark-marlin's `reindex_by_subdomain`: period = domain_h_n / domain_x_n, pi(c) = c period for c < domain_x_n,
 * else i = c - domain_x_n and pi(c) = i + i / (period - 1) + 1.  PCDHIP_E_ARG unless domain_x_n divides domain_h_n, both are domain
 * sizes, the matrices have the same number of rows, num_rows <= domain_h_n, num_cols <= domain_h_n and every column index is below
 * num_cols.  Duplicate (row, column) entries accumulate; explicit zeros are allowed.  A transposed row of more than 16 entries is cut
 * into segments of at most S = 4096 entries (the environment's PCDHIP_MARLIN_SEG at upload, 64 .. 2^20: a tuning knob), one wave each. */
typedef struct pcdhip_marlin_mats pcdhip_marlin_mats;
int pcdhip_marlin_mats_upload(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                              size_t domain_h_n, size_t domain_x_n, pcdhip_marlin_mats** out);
void pcdhip_marlin_mats_free(pcdhip_ctx* ctx, pcdhip_marlin_mats* mats);
/* out[0] = the segment length S of this handle, out[1] = segments (= waves of the second launch), out[2] = outputs that own segments,
 * out[3] = launches of one pcdhip_marlin_t_evals (1, or 3 with segments) */
int pcdhip_marlin_mats_info(const pcdhip_marlin_mats* mats, uint64_t out[4]);
/* ark-marlin `calculate_t` on H: t_out[j] = sum_M eta_M sum_{(r, c, v) in M, pi(c) = j} v r_alpha[r] for j < domain_h_n, M = A, B, C
 * (eta_mont: 3 elements; r_alpha: at least num_rows elements, e.g. from pcdhip_domain_bivariate_lagrange; t_out: at least domain_h_n,
 * not r_alpha).  One lane per output walks its short rows in the three matrices and applies eta_M once per row sum; the segments of
 * the long rows get a wave each and a small third launch adds them in: no atomics, at most three launches. */
int pcdhip_marlin_t_evals(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const uint64_t* eta_mont /* 3 elements */,
                          const pcdhip_buf* r_alpha, pcdhip_buf* t_out);
/* The rational sumcheck of round 3 over the index's row / col / row_col / val evaluations (on K, and again on the larger domain B),
 * for i < n and M = A, B, C:
 *   d_M = alpha beta - alpha row_M[i] - beta col_M[i] + row_col_M[i]   -- row_col taken as given (on B it is NOT the pointwise product);
 *   d_M = (beta - row_M[i]) (alpha - col_M[i])                         -- when row_col, or each of its entries, is NULL;
 *   b_i = d_A d_B d_C      a_i = c_A val_A[i] d_B d_C + c_B val_B[i] d_A d_C + c_C val_C[i] d_A d_B       (coeff_mont = c_A, c_B, c_C)
 * in ONE launch, one lane per element.  a_out and b_out must not be each other nor any input (PCDHIP_E_ARG); n == 0 succeeds without a
 * launch. */
int pcdhip_marlin_sumcheck_ab(pcdhip_ctx* ctx, const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* coeff_mont /* 3 */,
                              const pcdhip_buf* const row[3], const pcdhip_buf* const col[3],
                              const pcdhip_buf* const row_col[3] /* array or entries nullable */, const pcdhip_buf* const val[3], size_t n,
                              pcdhip_buf* a_out, pcdhip_buf* b_out);
/* f_i = a_i / b_i, and f_i = 0 where b_i = 0: that kernel into workspace, the batch inversion of b, the pointwise product (three
 * launches); f_out must not be an input.  Upstream inverts per matrix (f = sum_M c_M val_M / d_M), so where one d_M is zero it drops
 * that matrix's term only, while this call gives 0; the two agree whenever alpha and beta lie outside H, which is how the verifier
 * samples them. */
int pcdhip_marlin_sumcheck_f(pcdhip_ctx* ctx, const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* coeff_mont /* 3 */,
                             const pcdhip_buf* const row[3], const pcdhip_buf* const col[3],
                             const pcdhip_buf* const row_col[3] /* array or entries nullable */, const pcdhip_buf* const val[3], size_t n,
                             pcdhip_buf* f_out);

/* ---- K10 Marlin's index on device: arithmetise A, B, C onto K and B, commit ----------------------------------------------------
 * The producer of what K9 consumes: ark-marlin's `index` turns each constraint matrix into the polynomials row, col, row_col and val
 * -- by their evaluations on a domain K of at least nnz elements, their coefficients, and their evaluations on the larger domain B
 * that round 3 divides on -- and commits to the twelve.  Same conventions as K8 / K9: device vectors of ABI Montgomery elements of ONE
 * scalar field, the context's own stream and workspaces, device 0 of a multi-device context, PCDHIP_E_ARG for bad arguments, no
 * randomness, no CPU fallback.
 *
 * The arithmetisation of one matrix M with entries (r, c, v), w the generator of the resident transform of domain_h_n elements and pi
 * the `reindex_by_subdomain` of pcdhip_marlin_mats_upload.  Entry k runs over M row by row; inside a row by ascending column index,
 * equal columns in the order the CSR gives them (upstream sorts a row stably when it is not ascending); duplicate (r, c) entries stay
 * separate entries and explicit zeros stay entries.  This order is part of the contract: the commitments depend on it.
 *   k < nnz_M:          row_k = w^pi(c)    col_k = w^r    val_k = v w^pi(c) / |H|    row_col_k = row_k col_k
 *   nnz_M <= k < |K|:   row_k = col_k = row_col_k = 1,   val_k = 0
 * (val_k is v / u_H(w^pi(c), w^pi(c)) in closed form: u_H(x, x) = |H| x^(|H| - 1) = |H| / x on H.)
 * Domains: |K| = pcdhip_domain_size(field, max(nnz_A, nnz_B, nnz_C, 1)) and |B| = pcdhip_domain_size(field, max(3 |K| - 3, 1)).  The
 * rule for |B| is upstream's RESTATED FROM MEMORY (ark-marlin is not vendored here: the domain on which the prover divides a - b f by
 * v_K, whose degree is below 3 |K| - 3); a caller that knows better passes its own sizes.
 *
 * pcdhip_marlin_index_build: validates as pcdhip_marlin_mats_upload does (domain sizes, domain_x_n divides domain_h_n, equal row
 * counts, rows and num_cols <= domain_h_n, column indices below num_cols), lays every row out in ascending column order on the host
 * (O(nnz), once per index), uploads the three CSRs, and then works on the device alone: ONE launch writes the twelve vectors on K (one
 * lane per k and matrix: its row from the row pointers, pi(c) in the lane, w^j from the transform's resident powers), twelve inverse
 * transforms on K give the coefficients, and each coefficient vector, zero-padded on the device to |B| elements, goes through a forward
 * transform on B -- so on B row_col is the interpolated polynomial's evaluation, NOT row col.  Transforms are the library's general
 * ones: K and B may be mixed-radix.  domain_k_n / domain_b_n: 0 for the rules above, or the caller's own sizes -- each n = 2^a q^b that
 * pcdhip_fft_general takes, domain_k_n >= the largest nnz, domain_b_n >= domain_k_n; PCDHIP_E_ARG otherwise, and
 * PCDHIP_E_SIZE_UNSUPPORTED when a rule finds no domain of the size it needs.  keep: bit 0 the coefficients on K, bit 1 the evaluations
 * on K, bit 2 the evaluations on B; 0 means all three.  Forms that keep leaves out are computed where a kept one needs them and hold
 * no memory once the call returns.  The call waits for its own uploads: it never returns while reading caller memory. */
typedef struct pcdhip_marlin_index pcdhip_marlin_index;
int pcdhip_marlin_index_build(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                              size_t domain_h_n, size_t domain_x_n, size_t domain_k_n /* 0: rule */, size_t domain_b_n /* 0: rule */,
                              int keep, pcdhip_marlin_index** out);
void pcdhip_marlin_index_free(pcdhip_ctx* ctx, pcdhip_marlin_index* index);
/* out[0] = |K|, out[1] = |B|, out[2] = the largest nnz of the three matrices, out[3] = device bytes the handle holds */
int pcdhip_marlin_index_info(const pcdhip_marlin_index* index, uint64_t out[4]);
/* Device time of the build that made this handle, from events on the context's stream, in milliseconds: out_ms[0] the arithmetisation
 * launch, out_ms[1] the twelve inverse transforms on K with their conversions, out_ms[2] the twelve extensions to B (zero tail, forward
 * transform, conversion); a part that keep left out is 0 */
int pcdhip_marlin_index_timings(const pcdhip_marlin_index* index, float out_ms[3]);
/* One vector of the index as a BORROWED pcdhip_buf: valid until the index is freed, not to be freed or written by the caller.  form 0
 * coefficients (|K| of them) / 1 evaluations on K / 2 evaluations on B; matrix 0..2 = A, B, C; poly 0..3 = row, col, row_col, val.
 * PCDHIP_E_ARG for an index out of range and for a form that was not kept.  The buffers are ordinary device vectors: pcdhip_marlin_sumcheck_ab
 * / _f take them as row[3], col[3], row_col[3], val[3]; pcdhip_kzg_commit items, pcdhip_poly_eval and pcdhip_buf_download take them too. */
int pcdhip_marlin_index_vec(const pcdhip_marlin_index* index, int form, int matrix, int poly, const pcdhip_buf** out);
/* The twelve index commitments, matrix-major (A.row, A.col, A.row_col, A.val, B.row, ...): pcdhip_kzg_commit over the coefficient form,
 * non-hiding and without degree bounds, as upstream commits the index.  comm_xy: 12 affine points, comm_inf: 12 flags.  Argument rules
 * of pcdhip_kzg_commit (powers_of_g of the curve whose scalar field the index is over, at least as many as the longest trimmed
 * polynomial, not sharded, no outstanding MSM tickets); PCDHIP_E_ARG also when the coefficient form was not kept. */
int pcdhip_marlin_index_commit(pcdhip_ctx* ctx, const pcdhip_marlin_index* index, const pcdhip_bases* powers_of_g, uint64_t* comm_xy,
                               uint8_t* comm_inf);
/* Two device entry points the builder is made of, which the rounds need as well (f on K -> coefficients -> f on B is the same step).
 * pcdhip_fft_general_dev: pcdhip_fft_general on a device vector, in place -- any n = 2^a q^b (b = 0: pcdhip_fft_dev), n <= data's
 * elements; PCDHIP_E_SIZE_UNSUPPORTED for another n.
 * pcdhip_poly_evals_on_domain: out = the transform (coset != 0: on the coset) of the polynomial p of `len` coefficients over the domain
 * of domain_n elements, p padded with zeros: ark-poly `evaluate_over_domain`.  len <= domain_n <= out's elements and len <= p's
 * (PCDHIP_E_ARG otherwise, as for buffers of different fields); domain_n = 2^a q^b, else PCDHIP_E_SIZE_UNSUPPORTED.  out may be p when
 * p's buffer is large enough.  The call queues its launches and returns. */
int pcdhip_fft_general_dev(pcdhip_ctx* ctx, pcdhip_buf* data, size_t n, int inverse, int coset);
int pcdhip_poly_evals_on_domain(pcdhip_ctx* ctx, const pcdhip_buf* p, size_t len, size_t domain_n, int coset, pcdhip_buf* out);

/* ---- K11 Marlin's round 1 and the first sumcheck: w, z_A, z_B, h_1, g_1 ----------------------------------------------------------
 * The first half of ark-marlin's prover, on the conventions of K9 / K10: device vectors of ABI Montgomery elements of ONE scalar field,
 * the context's own stream and workspaces, device 0 of a multi-device context, host field elements as ABI Montgomery limbs, no
 * randomness inside (blinding coefficients and the mask polynomial are inputs), no host work of size n or nnz per call.  PCDHIP_E_ARG
 * for null pointers, mixed fields, counts beyond a buffer and the aliases each call forbids.  ark-marlin is not vendored: every call is
 * specified by the formula written here.  Notation: H the domain of domain_h_n elements with the generator w of the resident
 * transform, X its subdomain of domain_x_n elements, period = |H| / |X|, pi the `reindex_by_subdomain` of pcdhip_marlin_mats_upload,
 * z the full assignment of num_cols elements in variable order (the first |X| the formatted public input; z[c] = 0 for c >= num_cols),
 * v_S = X^|S| - 1.  Unless said otherwise a call only QUEUES its launches, as K9's do.
 *
 * pcdhip_marlin_mats_upload_ex: pcdhip_marlin_mats_upload with a choice of forms.  bit 0: the transposed matrices that
 * pcdhip_marlin_t_evals needs (all that pcdhip_marlin_mats_upload makes: it is this call with forms = 1, and its handle holds the same
 * memory and gives the same pcdhip_marlin_mats_info and results as before); bit 1: the forward A, B, C for pcdhip_marlin_zm_evals, laid
 * out as the witness map's mat-vec takes them.  forms == 0 or any higher bit: PCDHIP_E_ARG.  pcdhip_marlin_t_evals on a handle without
 * bit 0 and pcdhip_marlin_zm_evals on one without bit 1 return PCDHIP_E_ARG; pcdhip_marlin_mats_info speaks of the transposed form
 * alone (no segments for a handle without it). */
int pcdhip_marlin_mats_upload_ex(pcdhip_ctx* ctx, int field_id, const pcdhip_csr* A, const pcdhip_csr* B, const pcdhip_csr* C, size_t num_cols,
                                 size_t domain_h_n, size_t domain_x_n, uint32_t forms, pcdhip_marlin_mats** out);
/* z_M on H: out_M[r] = sum_{(r, c, v) in M} v z[c] for r < num_rows and out_M[r] = 0 for num_rows <= r < domain_h_n, M = A, B and
 * (zc_out non-NULL) C; duplicate entries accumulate.  z: at least num_cols elements; outputs: at least domain_h_n each, distinct from z
 * and from each other.  The witness map's mat-vec (one lane per short row, a wave per row of more than 16 entries, additions instead of
 * products for the coefficients -32 .. 32) between two conversions of image; C is not computed when zc_out is NULL. */
int pcdhip_marlin_zm_evals(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const pcdhip_buf* z, pcdhip_buf* za_out, pcdhip_buf* zb_out,
                           pcdhip_buf* zc_out /* nullable */);
/* z on H at pi's places, out[pi(c)] = z[c]: for k < domain_h_n, out[k] = z[k / period] when k % period == 0, else
 * out[k] = z[domain_x_n + (k - k / period - 1)]; an index >= num_cols reads as 0.  period == 1 (X = H) is legal: out[k] = z[k].  A gather,
 * one lane per k, no field arithmetic.  Both sizes must be domain sizes and domain_x_n divide domain_h_n; num_cols <= domain_h_n and
 * <= z's elements; out at least domain_h_n elements and not z (PCDHIP_E_ARG otherwise). */
int pcdhip_marlin_place_assignment(pcdhip_ctx* ctx, int field_id, size_t domain_h_n, size_t domain_x_n, const pcdhip_buf* z, size_t num_cols,
                                   pcdhip_buf* out);
/* Hiding: p <- p + b(X) (X^domain_n - 1) in place, b of k host coefficients (low degree first).  *out_len = max(len, domain_n + k); the
 * coefficients from len up to that are taken as 0 first, and the buffer must hold *out_len elements.  k == 0 is a no-op: nothing is
 * read or written and *out_len = len.  Only the two windows of k coefficients (and the zero tail) are touched, whatever len is; any
 * domain_n >= 1 and any k (the windows may overlap).  Upstream's hiding uses k = 1.  WAITS for the device: b is the caller's memory. */
int pcdhip_poly_add_vanishing_multiple(pcdhip_ctx* ctx, pcdhip_buf* p, size_t len, const uint64_t* blind_mont, size_t k, size_t domain_n,
                                       size_t* out_len);
/* The pointwise core of the first sumcheck, for i < n and eta_mont = eta_A, eta_B, eta_C:
 *   q_i = r_alpha_i (eta_A za_i + eta_B zb_i + eta_C za_i zb_i) - t_i z_i
 * computed as r (za (eta_A + eta_C zb) + eta_B zb) - t z in ONE launch, one lane per element: the five inputs are read once as ABI
 * words, one store.  Aliasing: element i depends on element i of the inputs alone and is stored after they are read, so q_out may be
 * any input's buffer.  Buffers never overlap in part, so a q_out that is two inputs' buffer means that those two inputs are the same
 * vector, which is legal like any other repeated input; there is no alias this call refuses.  n == 0 succeeds without a launch. */
int pcdhip_marlin_sumcheck1_q(pcdhip_ctx* ctx, const uint64_t* eta_mont /* 3 elements */, const pcdhip_buf* za, const pcdhip_buf* zb,
                              const pcdhip_buf* r_alpha, const pcdhip_buf* t, const pcdhip_buf* z, size_t n, pcdhip_buf* q_out);
/* Round 1 whole.  mats: a handle with the forward form; z: at least num_cols elements; blind_*_mont: k_w, k_a, k_b >= 0 host
 * coefficients (0: not hiding; the pointer may then be NULL).  Coefficient vectors written, low degree first:
 *   x_hat   = the inverse transform on X of z[0 .. |X|)                                      |X| coefficients
 *   z_poly  = interp_H(place(z)) + b_w v_H      (place = pcdhip_marlin_place_assignment)     |H| + k_w
 *   w       = (z_poly - x_hat) / v_X                                                         |H| + k_w - |X|   (0 for X = H, k_w = 0)
 *   w_rem   = the remainder of that division, |X| coefficients: ZERO by construction (z_poly - x_hat vanishes on X); it is written so
 *             that the caller can see it.  Since deg x_hat < |X|, w is the quotient of z_poly itself and w_rem its remainder less x_hat.
 *   za_poly = interp_H(A z) + b_a v_H           zb_poly = interp_H(B z) + b_b v_H            |H| + k_a, |H| + k_b
 * and, when za_evals / zb_evals are not NULL, z_A and z_B on H (|H| elements each, pcdhip_marlin_zm_evals).  out_lens = the lengths of
 * x_hat, z_poly, w, za_poly, zb_poly; every buffer must hold its length (w may be NULL when its length is 0) and all buffers of the
 * call are distinct.  The transforms are the library's general ones (H and X may be mixed-radix); workspace is the context's.  The
 * call WAITS for the device before it returns: the blinding coefficients are the caller's memory. */
int pcdhip_marlin_round1(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const pcdhip_buf* z, const uint64_t* blind_w_mont, size_t k_w,
                         const uint64_t* blind_a_mont, size_t k_a, const uint64_t* blind_b_mont, size_t k_b, pcdhip_buf* x_hat,
                         pcdhip_buf* z_poly, pcdhip_buf* w, pcdhip_buf* w_rem, pcdhip_buf* za_poly, pcdhip_buf* zb_poly,
                         pcdhip_buf* za_evals /* nullable */, pcdhip_buf* zb_evals /* nullable */, size_t out_lens[5]);
/* The first sumcheck whole: with r = r(alpha, X) (|H| coefficients, the interpolation of pcdhip_domain_bivariate_lagrange on H), t the
 * interpolation of pcdhip_marlin_t_evals(eta, r on H), and s the mask polynomial (NULL: none),
 *   q_1 = s + r (eta_A z_A + eta_B z_B + eta_C z_A z_B) - t z = h_1 v_H + X g_1 + sigma_1 / |H|
 * mats: a handle with the transposed form; za_poly, zb_poly, z_poly with their lengths (each >= 1) as round 1 leaves them.  Steps: r
 * and t on H, both to coefficients, the five polynomials z_A, z_B, r, t, z evaluated on D, pcdhip_marlin_sumcheck1_q there, the inverse
 * transform on D, + s, the division by v_H.  Outputs: t_poly (|H| coefficients), h_1 (len_q - |H| coefficients, len_q = max(|H| + len_za
 * + len_zb - 2, |H| + len_z - 1, len_mask): the quotient, its top coefficients zero when q_1 is shorter than that bound), g_1 (|H| - 1
 * coefficients: the remainder shifted down by one), and sigma = the remainder's constant term in a one-element buffer -- sigma_1 / |H|,
 * which is 0 for a satisfied system and a mask that sums to zero on H.  out_lens = the lengths of t_poly, h_1, g_1.  Outputs are
 * distinct from each other and from the inputs; h_1 / g_1 may be NULL when their length is 0.
 * D: domain_d_n == 0 means pcdhip_domain_size(field, |H| + len_za + len_zb - 2), the length of the longest product -- 3 |H| + k_a + k_b - 2
 * after round 1.  This is upstream's `mul_domain` RESTATED FROM MEMORY, as K10's rule for |B| is; a caller that knows better passes its
 * own n = 2^a q^b.  PCDHIP_E_SIZE_UNSUPPORTED for a size that is no such domain (or when the rule finds none), PCDHIP_E_ARG for one
 * below len_q.  H and D may be mixed-radix.  The call only queues its work: nothing of the caller's host memory is read after it
 * returns, and the results are there after pcdhip_sync or any call that waits. */
int pcdhip_marlin_sumcheck1(pcdhip_ctx* ctx, const pcdhip_marlin_mats* mats, const uint64_t* eta_mont /* 3 elements */,
                            const uint64_t* alpha_mont, const pcdhip_buf* za_poly, size_t len_za, const pcdhip_buf* zb_poly, size_t len_zb,
                            const pcdhip_buf* z_poly, size_t len_z, const pcdhip_buf* mask /* nullable */, size_t len_mask,
                            size_t domain_d_n /* 0: rule */, pcdhip_buf* t_poly, pcdhip_buf* h1, pcdhip_buf* g1, pcdhip_buf* sigma,
                            size_t out_lens[3]);

/* ---- K12 Marlin's second sumcheck: f, g_2 and h_2 -----------------------------------------------------------------------------------
 * The last prover step of ark-marlin's round 3, on the conventions of K9 - K11: device vectors of ABI Montgomery elements of ONE scalar
 * field, the context's own stream and workspaces, device 0 of a multi-device context, host field elements as ABI Montgomery limbs,
 * PCDHIP_E_ARG for bad arguments, no CPU fallback.  Both calls only QUEUE their launches.  ark-marlin is not vendored: the calls are
 * specified by the formulas written here, and what is said about upstream -- the order of its steps, the rule for |B| -- is RESTATED
 * FROM MEMORY.
 *
 * pcdhip_marlin_sumcheck2_q, the pointwise core: q_i = a_i - b_i f_i for i < n, with a and b EXACTLY those of
 * pcdhip_marlin_sumcheck_ab (both forms of d_M, the same rule for a NULL row_col), in ONE launch, one lane per element: the thirteen
 * vectors are read once as ABI words, there is one store, and a and b never reach memory.  Argument rules of
 * pcdhip_marlin_sumcheck_ab; f and q_out hold at least n elements of the same field.  Aliasing: every load of element i precedes its
 * store, so q_out may be f (in place); q_out on any of the twelve index vectors is PCDHIP_E_ARG.  n == 0 succeeds without a launch. */
int pcdhip_marlin_sumcheck2_q(pcdhip_ctx* ctx, const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* coeff_mont /* 3 */,
                              const pcdhip_buf* const row[3], const pcdhip_buf* const col[3],
                              const pcdhip_buf* const row_col[3] /* array or entries nullable */, const pcdhip_buf* const val[3],
                              const pcdhip_buf* f, size_t n, pcdhip_buf* q_out);
/* The second sumcheck whole, from an index that kept its evaluations on K and on B (keep bits 1 and 2; PCDHIP_E_ARG otherwise).
 * coeff_mont = c_A, c_B, c_C is the caller's: eta_M v_H(alpha) v_H(beta) in the prover.  With v_K = X^|K| - 1:
 *   f on K   = pcdhip_marlin_sumcheck_f over the index's evaluations on K (row_col as the index holds it)
 *   f_poly   = the interpolation of f on K                                                     |K| coefficients   (nullable)
 *   f_poly   = sigma + X g_2:   sigma = f_poly's constant term = sigma_2 / |K| = (sum_K f) / |K|   1 element
 *                               g_2   = f_poly shifted down by one                                 |K| - 1 coefficients
 *   a, b     = the polynomials of degree <= 3 |K| - 3 whose evaluations on B pcdhip_marlin_sumcheck_ab gives over the index's vectors on
 *              B: there row_col is the interpolated polynomial, so a and b are the formulas of pcdhip_marlin_sumcheck_ab over the
 *              POLYNOMIALS row, col, row_col, val
 *   a - b f_poly = h_2 v_K + remainder:   h_2 3 |K| - 3 coefficients, NOT trimmed;   remainder |K| coefficients
 * The remainder is ZERO by construction whenever no d_M vanishes on K (a = b f there); it is written to h2_rem when that is given, so
 * that the caller can see it.  out_lens[0] = |K| - 1, out_lens[1] = 3 |K| - 3, out_lens[2] = the route taken; all three are known on
 * the host before anything runs.  The outputs are distinct buffers that hold their lengths (g2 and h2 may be NULL for |K| = 1); nothing
 * is written when the call refuses.
 * Routes.  deg(a - b f_poly) = 4 |K| - 4, and upstream forms b f_poly as a polynomial product rather than pointwise on B:
 *   route 1  pointwise on B, needs |B| >= 4 |K| - 3: f_poly zero-padded onto B, pcdhip_marlin_sumcheck2_q there in place over the
 *            index's vectors, the inverse transform on B, the division by v_K.  Workspace: ONE vector of |B| elements (and 2 |K|)
 *            beyond the transform's own.
 *   route 2  upstream's order, needs |B| >= 3 |K| - 2: pcdhip_marlin_sumcheck_ab on B, two inverse transforms on B, b_poly f_poly by
 *            the steps of pcdhip_poly_mul over pcdhip_domain_size(field, 4 |K| - 3) elements (PCDHIP_E_SIZE_UNSUPPORTED when there is
 *            none), the subtraction, the division.  Workspace: two vectors of max(|B|, 4 |K| - 3) and a third transform vector.
 *   route 0  picks 1 when |B| allows it, else 2.  A forced route whose condition fails is PCDHIP_E_ARG.
 * K10's rule |B| = pcdhip_domain_size(field, 3 |K| - 3) gives 4 |K| for a radix-2 B and about 3.06 |K| for a mixed-radix one, hence
 * both.  K and B may be mixed-radix: every transform is the library's general one.  Both routes give the same h_2, bit for bit. */
int pcdhip_marlin_sumcheck2(pcdhip_ctx* ctx, const pcdhip_marlin_index* index, const uint64_t* alpha_mont, const uint64_t* beta_mont,
                            const uint64_t* coeff_mont /* 3 */, int route /* 0 auto, 1, 2 */, pcdhip_buf* f_poly /* nullable */,
                            pcdhip_buf* g2, pcdhip_buf* sigma, pcdhip_buf* h2, pcdhip_buf* h2_rem /* nullable */, size_t out_lens[3]);

/* ---- timing helpers (HIP events on the context's stream, for bench.py) ------------------------- */
int pcdhip_timer_start(pcdhip_ctx* ctx);
int pcdhip_timer_stop(pcdhip_ctx* ctx, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* PCDHIP_H */
