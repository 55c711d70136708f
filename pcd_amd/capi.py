"""ctypes binding of libpcdhip.so (include/pcdhip.h).  numpy uint64 arrays in, numpy arrays out.

Mirrors the C-ABI one to one; the class/method names follow the upstream functions they stand in
for (`multi_scalar_mul`, `fft`/`ifft`/`coset_fft`/`coset_ifft`, `witness_map`, `create_proof`).
No fallback: a missing library or a missing GPU raises PcdHipError."""
import ctypes as C
import os

import numpy as np

from .build import library_path

MNT4_298, MNT6_298, MNT4_753, MNT6_753 = 0, 1, 2, 3
G1, G2 = 1, 2
FIELD_LIMBS = [5, 5, 12, 12]
CURVE_FQ = [0, 1, 2, 3]
CURVE_FR = [1, 0, 3, 2]
CURVE_G2_DEG = [2, 3, 2, 3]


class PcdHipError(RuntimeError):
    pass


class PrevTicketError(PcdHipError):
    """PCDHIP_E_PREV_TICKET: an EARLIER MSM of the slot had an unreduced scalar; `ticket` (when not None) is the NEW submission, which was
    enqueued all the same and must be waited for / released like any other"""

    def __init__(self, msg, ticket=None):
        super().__init__(msg)
        self.ticket = ticket


class Csr(C.Structure):
    _fields_ = [("num_rows", C.c_uint64), ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("coeff", C.c_void_p)]


class G16PkHost(C.Structure):
    _fields_ = [("curve_id", C.c_uint32), ("_pad", C.c_uint32), ("num_vars", C.c_uint64), ("num_inputs", C.c_uint64),
                ("domain_size", C.c_uint64),
                ("alpha_g1", C.c_void_p), ("beta_g1", C.c_void_p), ("delta_g1", C.c_void_p),
                ("beta_g2", C.c_void_p), ("delta_g2", C.c_void_p),
                ("a_query", C.c_void_p), ("a_inf", C.c_void_p),
                ("b_g1_query", C.c_void_p), ("b_g1_inf", C.c_void_p),
                ("b_g2_query", C.c_void_p), ("b_g2_inf", C.c_void_p),
                ("h_query", C.c_void_p), ("h_inf", C.c_void_p), ("h_len", C.c_uint64),
                ("l_query", C.c_void_p), ("l_inf", C.c_void_p), ("l_len", C.c_uint64)]


class KzgCommitItem(C.Structure):
    """Mirror of `pcdhip_kzg_commit_item` (include/pcdhip.h)."""
    _fields_ = [("poly", C.c_void_p), ("len", C.c_uint64), ("blinding", C.c_void_p), ("blinding_len", C.c_uint64),
                ("shifted_blinding", C.c_void_p), ("shifted_blinding_len", C.c_uint64), ("shifted_offset", C.c_uint64),
                ("shifted", C.c_uint32), ("_pad", C.c_uint32)]


class MsmShortItem(C.Structure):
    """Mirror of `pcdhip_msm_short_item` (include/pcdhip.h)."""
    _fields_ = [("base_offset", C.c_uint64), ("scalar_offset", C.c_uint64), ("n", C.c_uint64)]


_LIB = None

EXPORTS = [
    "pcdhip_strerror", "pcdhip_device_count", "pcdhip_init", "pcdhip_init_devices", "pcdhip_ctx_devices", "pcdhip_destroy", "pcdhip_sync", "pcdhip_host_alloc", "pcdhip_host_free", "pcdhip_last_hip_error",
    "pcdhip_field_limbs", "pcdhip_curve_base_field", "pcdhip_curve_scalar_field", "pcdhip_point_limbs",
    "pcdhip_buf_upload", "pcdhip_buf_alloc", "pcdhip_buf_download", "pcdhip_buf_free",
    "pcdhip_bases_upload", "pcdhip_bases_free", "pcdhip_msm", "pcdhip_msm_dev", "pcdhip_msm_config", "pcdhip_msm_submit", "pcdhip_msm_collect", "pcdhip_msm_submit_partial", "pcdhip_msm_ticket_wait", "pcdhip_msm_ticket_status", "pcdhip_bases_info", "pcdhip_stream_wait",
    "pcdhip_set_precompute", "pcdhip_set_precompute_budget", "pcdhip_get_precompute_budget", "pcdhip_msm_set_sort", "pcdhip_msm_set_bin_stage", "pcdhip_msm_set_accumulate", "pcdhip_msm_profile", "pcdhip_msm_last_timings", "pcdhip_msm_last_plan", "pcdhip_mad_rate", "pcdhip_points_sum", "pcdhip_msm_dev_partial", "pcdhip_points_sum_dev", "pcdhip_to_affine",
    "pcdhip_fft", "pcdhip_fft_dev", "pcdhip_fft_general", "pcdhip_fft_seq", "pcdhip_domain_size", "pcdhip_fft_last_timings", "pcdhip_groth16_witness_map",
    "pcdhip_g16_pk_upload", "pcdhip_g16_pk_free", "pcdhip_g16_pk_set_r1cs", "pcdhip_g16_pk_info", "pcdhip_g16_pk_memory", "pcdhip_g16_witness_map_resident", "pcdhip_groth16_prove", "pcdhip_groth16_last_timings", "pcdhip_groth16_set_assembly", "pcdhip_groth16_set_sparse_window", "pcdhip_groth16_last_plan", "pcdhip_groth16_set_witness_split", "pcdhip_groth16_set_schedule", "pcdhip_set_lane_reserve", "pcdhip_fixed_base_mul", "pcdhip_groth16_setup",
    "pcdhip_serialized_size", "pcdhip_serialize_points", "pcdhip_deserialize_points", "pcdhip_deserialize_points_unchecked", "pcdhip_proof_serialized_size", "pcdhip_proof_serialize",
    "pcdhip_proof_deserialize", "pcdhip_vk_serialized_size", "pcdhip_vk_serialize", "pcdhip_vk_deserialize",
    "pcdhip_process_vk", "pcdhip_pvk_free", "pcdhip_groth16_verify_prepared", "pcdhip_groth16_verify_batch_rlc",
    "pcdhip_multi_pairing", "pcdhip_pairing_set_mode", "pcdhip_groth16_verify", "pcdhip_groth16_verify_batch", "pcdhip_timer_start", "pcdhip_timer_stop",
    "pcdhip_poly_eval", "pcdhip_poly_lincomb", "pcdhip_poly_div_linear", "pcdhip_kzg_open", "pcdhip_kzg_check", "pcdhip_kzg_commit",
    "pcdhip_vec_mul", "pcdhip_vec_batch_inverse", "pcdhip_poly_div_vanishing", "pcdhip_poly_mul",
    "pcdhip_msm_short", "pcdhip_msm_short_dev", "pcdhip_msm_set_short",
    "pcdhip_msm_short_batch", "pcdhip_msm_short_batch_dev", "pcdhip_kzg_commit_last_plan",
    "pcdhip_domain_bivariate_lagrange", "pcdhip_marlin_mats_upload", "pcdhip_marlin_mats_free", "pcdhip_marlin_mats_info", "pcdhip_marlin_t_evals",
    "pcdhip_marlin_sumcheck_ab", "pcdhip_marlin_sumcheck_f",
    "pcdhip_marlin_index_build", "pcdhip_marlin_index_free", "pcdhip_marlin_index_info", "pcdhip_marlin_index_timings", "pcdhip_marlin_index_vec", "pcdhip_marlin_index_commit",
    "pcdhip_fft_general_dev", "pcdhip_poly_evals_on_domain",
    "pcdhip_marlin_mats_upload_ex", "pcdhip_marlin_zm_evals", "pcdhip_marlin_place_assignment", "pcdhip_poly_add_vanishing_multiple",
    "pcdhip_marlin_sumcheck1_q", "pcdhip_marlin_round1", "pcdhip_marlin_sumcheck1",
    "pcdhip_marlin_sumcheck2_q", "pcdhip_marlin_sumcheck2",
    "pcdhip_poly_open_quotients", "pcdhip_kzg_batch_open", "pcdhip_kzg_batch_open_last_plan",
    "pcdhip_kzg_vk_prepare", "pcdhip_kzg_vk_free", "pcdhip_kzg_check_combinations", "pcdhip_kzg_check_scalars", "pcdhip_kzg_check_combinations_last_plan",
]


def lib():
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise PcdHipError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        _LIB = C.CDLL(path)
        _LIB.pcdhip_strerror.restype = C.c_char_p
        _LIB.pcdhip_last_hip_error.restype = C.c_char_p
        _LIB.pcdhip_destroy.restype = None
        _LIB.pcdhip_domain_size.restype = C.c_size_t
        for name in ("pcdhip_serialized_size", "pcdhip_proof_serialized_size", "pcdhip_vk_serialized_size"):
            getattr(_LIB, name).restype = C.c_size_t
        for name in ("pcdhip_buf_free", "pcdhip_bases_free", "pcdhip_g16_pk_free", "pcdhip_host_free", "pcdhip_pvk_free", "pcdhip_marlin_mats_free"):
            getattr(_LIB, name).restype = None
        vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
        _LIB.pcdhip_vec_mul.argtypes = [vp, vp, vp, sz, vp]
        _LIB.pcdhip_vec_batch_inverse.argtypes = [vp, vp, sz, vp, vp]
        _LIB.pcdhip_poly_div_vanishing.argtypes = [vp, vp, sz, sz, vp, szp, vp, szp]
        _LIB.pcdhip_poly_mul.argtypes = [vp, vp, sz, vp, sz, vp, szp]
        _LIB.pcdhip_kzg_commit.argtypes = [vp, vp, vp, vp, C.POINTER(KzgCommitItem), sz, vp, vp, vp, vp, vp]
        _LIB.pcdhip_msm_short_batch.argtypes = [vp, vp, vp, sz, C.POINTER(MsmShortItem), sz, vp]
        _LIB.pcdhip_msm_short_batch_dev.argtypes = [vp, vp, vp, C.POINTER(MsmShortItem), sz, vp]
        _LIB.pcdhip_domain_bivariate_lagrange.argtypes = [vp, C.c_int, sz, vp, vp]
        _LIB.pcdhip_marlin_mats_upload.argtypes = [vp, C.c_int, vp, vp, vp, sz, sz, sz, vp]
        _LIB.pcdhip_marlin_mats_free.argtypes = [vp, vp]
        _LIB.pcdhip_marlin_mats_info.argtypes = [vp, vp]
        _LIB.pcdhip_marlin_t_evals.argtypes = [vp, vp, vp, vp, vp]
        _LIB.pcdhip_marlin_sumcheck_ab.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]
        _LIB.pcdhip_marlin_sumcheck_f.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        _LIB.pcdhip_marlin_index_build.argtypes = [vp, C.c_int, vp, vp, vp, sz, sz, sz, sz, sz, C.c_int, vp]
        _LIB.pcdhip_marlin_index_free.argtypes = [vp, vp]
        _LIB.pcdhip_marlin_index_free.restype = None
        _LIB.pcdhip_marlin_index_info.argtypes = [vp, vp]
        _LIB.pcdhip_marlin_index_timings.argtypes = [vp, vp]
        _LIB.pcdhip_marlin_index_vec.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        _LIB.pcdhip_marlin_index_commit.argtypes = [vp, vp, vp, vp, vp]
        _LIB.pcdhip_fft_general_dev.argtypes = [vp, vp, sz, C.c_int, C.c_int]
        _LIB.pcdhip_poly_evals_on_domain.argtypes = [vp, vp, sz, sz, C.c_int, vp]
        _LIB.pcdhip_marlin_mats_upload_ex.argtypes = [vp, C.c_int, vp, vp, vp, sz, sz, sz, C.c_uint32, vp]
        _LIB.pcdhip_marlin_zm_evals.argtypes = [vp, vp, vp, vp, vp, vp]
        _LIB.pcdhip_marlin_place_assignment.argtypes = [vp, C.c_int, sz, sz, vp, sz, vp]
        _LIB.pcdhip_poly_add_vanishing_multiple.argtypes = [vp, vp, sz, vp, sz, sz, szp]
        _LIB.pcdhip_marlin_sumcheck1_q.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp]
        _LIB.pcdhip_marlin_round1.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, szp]
        _LIB.pcdhip_marlin_sumcheck1.argtypes = [vp, vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, sz, vp, vp, vp, vp, szp]
        _LIB.pcdhip_marlin_sumcheck2_q.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        _LIB.pcdhip_marlin_sumcheck2.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, szp]
        _LIB.pcdhip_poly_open_quotients.argtypes = [vp, C.c_int, C.POINTER(KzgCommitItem), sz, sz, vp, vp, vp, vp, szp, vp]
        _LIB.pcdhip_kzg_batch_open.argtypes = [vp, vp, vp, vp, C.POINTER(KzgCommitItem), sz, sz, vp, vp, vp, vp, vp, vp, vp]
        _LIB.pcdhip_kzg_batch_open_last_plan.argtypes = [vp, vp]
        _LIB.pcdhip_kzg_vk_prepare.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, sz, vp]
        _LIB.pcdhip_kzg_vk_free.argtypes = [vp, vp]
        _LIB.pcdhip_kzg_vk_free.restype = None
        _LIB.pcdhip_kzg_check_combinations.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, sz] + [vp] * 10
        _LIB.pcdhip_kzg_check_scalars.argtypes = [vp, C.c_int, sz, sz, vp, sz] + [vp] * 9
        _LIB.pcdhip_kzg_check_combinations_last_plan.argtypes = [vp, vp]
    return _LIB


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def point_limbs(curve, group):
    return 2 * (1 if group == G1 else CURVE_G2_DEG[curve]) * FIELD_LIMBS[CURVE_FQ[curve]]


class Context:
    """One device + one HIP stream (pcdhip_ctx); with `devices=[...]` a multi-device context (pcdhip_init_devices) that shards
    bases, keys, MSMs and proofs by point range over the listed devices."""

    def __init__(self, device=0, devices=None):
        self._ctx = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = lib().pcdhip_init_devices(ids, len(devices), C.byref(self._ctx))
            device = devices[0]
        else:
            rc = lib().pcdhip_init(int(device), C.byref(self._ctx))
        if rc != 0:
            raise PcdHipError(f"pcdhip_init(device={device}, devices={devices}) failed: {lib().pcdhip_strerror(rc).decode()}")
        self.device = device
        self.devices = list(devices) if devices is not None else [device]

    def close(self):
        if self._ctx:
            lib().pcdhip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            detail = lib().pcdhip_last_hip_error(self._ctx).decode()
            raise PcdHipError(f"{lib().pcdhip_strerror(rc).decode()} (rc={rc}) {detail}")

    def sync(self):
        self._check(lib().pcdhip_sync(self._ctx))

    # ---- device vectors
    def buf_upload(self, field, arr):
        arr = _u64(arr)
        n = arr.shape[0]
        h = C.c_void_p()
        self._check(lib().pcdhip_buf_upload(self._ctx, field, _p(arr), C.c_size_t(n), C.byref(h)))
        return DeviceBuf(self, h, field, n)

    # ---- MSM
    def bases_upload(self, curve, group, xy, inf=None):
        xy = _u64(xy)
        n = xy.shape[0]
        infp = np.ascontiguousarray(inf, dtype=np.uint8) if inf is not None else None
        h = C.c_void_p()
        self._check(lib().pcdhip_bases_upload(self._ctx, curve, group, _p(xy), _p(infp), C.c_size_t(n), C.byref(h)))
        return Bases(self, h, curve, group, n)

    def msm(self, bases, scalars, offset=0, n=None):
        """multi_scalar_mul(bases[offset:offset+n], scalars) -> Jacobian X||Y||Z (uint64 limbs)."""
        out = np.zeros(3 * point_limbs(bases.curve, bases.group) // 2, dtype=np.uint64)
        if isinstance(scalars, DeviceBuf):
            n = scalars.n if n is None else n
            self._check(lib().pcdhip_msm_dev(self._ctx, bases._h, C.c_size_t(offset), scalars._h, C.c_size_t(0), C.c_size_t(n), _p(out)))
        else:
            scalars = _u64(scalars)
            n = scalars.shape[0] if n is None else n
            self._check(lib().pcdhip_msm(self._ctx, bases._h, C.c_size_t(offset), _p(scalars), C.c_size_t(n), _p(out)))
        return out

    def msm_short(self, bases, scalars, offset=0, n=None, scalar_offset=0):
        """msm() for a few pairs (at most 1024) without buckets: bit-plane sums over the handle's resident copies.  `scalars`: canonical
        limbs (numpy) or a DeviceBuf, then from element `scalar_offset` on.  Same result up to the Jacobian representative."""
        out = np.zeros(3 * point_limbs(bases.curve, bases.group) // 2, dtype=np.uint64)
        if isinstance(scalars, DeviceBuf):
            n = scalars.n - scalar_offset if n is None else n
            self._check(lib().pcdhip_msm_short_dev(self._ctx, bases._h, C.c_size_t(offset), scalars._h, C.c_size_t(scalar_offset), C.c_size_t(n), _p(out)))
        else:
            scalars = _u64(scalars)
            n = scalars.shape[0] if n is None else n
            self._check(lib().pcdhip_msm_short(self._ctx, bases._h, C.c_size_t(offset), _p(scalars), C.c_size_t(n), _p(out)))
        return out

    def msm_short_batch(self, bases, scalars, items):
        """k independent short MSMs over one handle as one launch chain (pcdhip_msm_short_batch / _dev).  `items`: (base_offset,
        scalar_offset, n) tuples, n pairs each from those positions on; `scalars`: canonical limbs (numpy, uploaded once) or a DeviceBuf
        -> a (k, limbs) array of Jacobian points X||Y||Z, Z = 0 for the identity (which n == 0 gives)."""
        k = len(items)
        arr = (MsmShortItem * max(k, 1))()
        for a, (bo, so, n) in zip(arr, items):
            a.base_offset, a.scalar_offset, a.n = int(bo), int(so), int(n)
        out = np.zeros((k, 3 * point_limbs(bases.curve, bases.group) // 2), dtype=np.uint64)
        if isinstance(scalars, DeviceBuf):
            self._check(lib().pcdhip_msm_short_batch_dev(self._ctx, bases._h, scalars._h, arr if k else None, k, _p(out)))
        else:
            scalars = _u64(scalars)
            self._check(lib().pcdhip_msm_short_batch(self._ctx, bases._h, _p(scalars), scalars.shape[0], arr if k else None, k, _p(out)))
        return out

    def msm_set_short(self, max_n):
        """kzg_open / kzg_check run their MSMs over at most `max_n` pairs through msm_short, and kzg_commit its hiding MSMs of at most
        `max_n` coefficients as one msm_short_batch chain (0, the default: never)."""
        self._check(lib().pcdhip_msm_set_short(self._ctx, C.c_size_t(int(max_n))))

    def msm_submit(self, bases, scalars, offset=0, n=None, scalar_offset=0):
        """enqueue an MSM over resident scalars on a side stream -> ticket (at most four outstanding); see msm_collect"""
        n = scalars.n - scalar_offset if n is None else n
        t = C.c_int(-1)
        self._check(lib().pcdhip_msm_submit(self._ctx, bases._h, C.c_size_t(offset), scalars._h, C.c_size_t(scalar_offset), C.c_size_t(n), C.byref(t)))
        return (t.value, bases.curve, bases.group)

    def msm_collect(self, ticket):
        t, curve, group = ticket
        out = np.zeros(3 * point_limbs(curve, group) // 2, dtype=np.uint64)
        self._check(lib().pcdhip_msm_collect(self._ctx, t, _p(out)))
        return out

    def msm_submit_partial(self, bases, scalars, out_slots_device_ptr, slot_stride_bytes, offset=0, n=None):
        """msm_submit with the Jacobian partial left in slot `ticket` of the caller's device buffer (four slots, `slot_stride_bytes`
        apart) -> ticket number; release it with msm_ticket_wait(ticket, stream), which makes `stream` wait for the MSM."""
        n = scalars.n if n is None else n
        t = C.c_int(-1)
        rc = lib().pcdhip_msm_submit_partial(self._ctx, bases._h, C.c_size_t(offset), scalars._h, C.c_size_t(0), C.c_size_t(n),
                                             C.c_void_p(out_slots_device_ptr), C.c_size_t(slot_stride_bytes), C.byref(t))
        if rc == -6:   # PCDHIP_E_PREV_TICKET: this submission is in flight; an earlier one of the slot was wrong
            raise PrevTicketError(lib().pcdhip_strerror(rc).decode(), t.value)
        self._check(rc)
        return t.value

    def msm_ticket_wait(self, ticket, other_stream):
        self._check(lib().pcdhip_msm_ticket_wait(self._ctx, int(ticket), C.c_void_p(other_stream)))

    def msm_ticket_status(self, slot):
        """waits for the last released MSM of `slot`; raises PrevTicketError when one of its scalars was not reduced"""
        rc = lib().pcdhip_msm_ticket_status(self._ctx, int(slot))
        if rc == -6:
            raise PrevTicketError(lib().pcdhip_strerror(rc).decode())
        self._check(rc)

    def msm_partial_to_device(self, bases, scalars, out_device_ptr, offset=0, n=None):
        """The MSM of a shard with its Jacobian result left at `out_device_ptr` (device memory of the caller, e.g. a torch
        tensor's data_ptr(): the send buffer of the all-gather).  Asynchronous: call sync() before another stream reads it."""
        n = scalars.n if n is None else n
        self._check(lib().pcdhip_msm_dev_partial(self._ctx, bases._h, C.c_size_t(offset), scalars._h, C.c_size_t(0), C.c_size_t(n),
                                                 C.c_void_p(out_device_ptr)))

    def points_sum_device(self, curve, group, xyz_device_ptr, n):
        """Sum of n Jacobian points that sit in device memory (the receive buffer of the all-gather) -> host limbs."""
        out = np.zeros(3 * point_limbs(curve, group) // 2, dtype=np.uint64)
        self._check(lib().pcdhip_points_sum_dev(self._ctx, curve, group, C.c_void_p(xyz_device_ptr), C.c_size_t(n), _p(out)))
        return out

    def bases_info(self, bases, n=0):
        """(window bits c, scalar windows W, resident window-shifted copies) of an MSM of n pairs over `bases`."""
        c, w, k = C.c_int(), C.c_int(), C.c_int()
        self._check(lib().pcdhip_bases_info(bases._h, C.c_size_t(n), C.byref(c), C.byref(w), C.byref(k)))
        return c.value, w.value, k.value

    def stream_wait(self, other_stream, direction):
        """direction 0: this context's stream waits for `other_stream` (a raw hipStream_t); 1: the other way round."""
        self._check(lib().pcdhip_stream_wait(self._ctx, C.c_void_p(other_stream), int(direction)))

    def msm_config(self, window_bits=0, chunk=0):
        self._check(lib().pcdhip_msm_config(self._ctx, window_bits, chunk))

    def set_precompute(self, mode):
        """-1 full (default), 0 none, k >= 2 copies; applies to bases uploaded afterwards."""
        self._check(lib().pcdhip_set_precompute(self._ctx, int(mode)))

    def set_precompute_budget(self, bytes_per_vector):
        """bytes one base vector uploaded afterwards may occupy with its window-shifted copies (0: no bound); fewer copies otherwise."""
        self._check(lib().pcdhip_set_precompute_budget(self._ctx, C.c_size_t(int(bytes_per_vector))))

    def get_precompute_budget(self):
        v = C.c_size_t(0)
        self._check(lib().pcdhip_get_precompute_budget(self._ctx, C.byref(v)))
        return v.value

    def msm_set_sort(self, mode):
        """0: LDS partition sort (default); 1: single-pass binning with on-device fallback; 2: two-pass counting sort;
        3: the partition sort with its direct (unstaged) write pass; 4: the partition sort with the two-read per-bin sort."""
        self._check(lib().pcdhip_msm_set_sort(self._ctx, int(mode)))

    def msm_set_bin_stage(self, cap=-1):
        """per-bin sort of modes 0 and 3: bins of at most `cap` entries are ordered in LDS from one read (-1: the default, 18 432; 0: the
        two-read kernel of mode 4); a developer and test knob, results do not depend on it"""
        self._check(lib().pcdhip_msm_set_bin_stage(self._ctx, int(cap)))

    def msm_set_accumulate(self, mode, chunk=0, min_pairs=0):
        """0 by size, 1 running sums, 2 pair tree of affine additions (753-bit G1); chunk / min_pairs: tuning and test knobs"""
        self._check(lib().pcdhip_msm_set_accumulate(self._ctx, int(mode), int(chunk), int(min_pairs)))

    def msm_profile(self, on=True):
        self._check(lib().pcdhip_msm_profile(self._ctx, int(on)))

    def msm_last_timings(self):
        out = (C.c_float * 8)()
        self._check(lib().pcdhip_msm_last_timings(self._ctx, out))
        return dict(zip(["digits", "scan", "scatter", "accumulate", "fixup", "tail", "horner", "total"], list(out)))

    def msm_last_plan(self):
        """(entries of the sorted list, entries per lane the device chose) of the last profiled MSM"""
        out = (C.c_uint32 * 2)()
        self._check(lib().pcdhip_msm_last_plan(self._ctx, out))
        return int(out[0]), int(out[1])

    def mad_rate(self):
        """v_mad_u64_u32 lane-operations per second of this device, measured now (pcdhip_mad_rate)"""
        out = C.c_double(0.0)
        self._check(lib().pcdhip_mad_rate(self._ctx, C.byref(out)))
        return float(out.value)

    def points_sum(self, curve, group, xyz):
        xyz = _u64(xyz).reshape(-1, 3 * point_limbs(curve, group) // 2)
        out = np.zeros(xyz.shape[1], dtype=np.uint64)
        self._check(lib().pcdhip_points_sum(self._ctx, curve, group, _p(xyz), C.c_size_t(xyz.shape[0]), _p(out)))
        return out

    def to_affine(self, curve, group, xyz):
        xyz = _u64(xyz).reshape(-1, 3 * point_limbs(curve, group) // 2)
        n = xyz.shape[0]
        xy = np.zeros((n, point_limbs(curve, group)), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        self._check(lib().pcdhip_to_affine(self._ctx, curve, group, _p(xyz), C.c_size_t(n), _p(xy), _p(inf)))
        return xy, inf

    # ---- FFT
    def fft(self, field, data, inverse=False, coset=False):
        if isinstance(data, DeviceBuf):
            log_n = data.n.bit_length() - 1
            self._check(lib().pcdhip_fft_dev(self._ctx, data._h, log_n, int(inverse), int(coset)))
            return data
        data = _u64(data).copy()
        n = data.shape[0]
        log_n = n.bit_length() - 1
        assert 1 << log_n == n
        self._check(lib().pcdhip_fft(self._ctx, field, _p(data), log_n, int(inverse), int(coset)))
        return data

    def fft_general(self, field, data, inverse=False, coset=False):
        """GeneralEvaluationDomain transform on n = 2^a q^b elements (mixed radix for the help fields)."""
        data = _u64(data).copy()
        self._check(lib().pcdhip_fft_general(self._ctx, field, _p(data), C.c_size_t(data.shape[0]), int(inverse), int(coset)))
        return data

    def fft_seq(self, field, data, ops):
        """the transforms `ops` = [(inverse, coset), ..] applied one after the other to one host vector, one trip over PCIe"""
        data = _u64(data).copy()
        codes = (C.c_int * len(ops))(*[int(bool(i)) | (int(bool(c)) << 1) for i, c in ops])
        self._check(lib().pcdhip_fft_seq(self._ctx, field, _p(data), C.c_size_t(data.shape[0]), codes, len(ops)))
        return data

    def fft_last_timings(self):
        out = (C.c_float * 8)()
        k = lib().pcdhip_fft_last_timings(self._ctx, out)
        return list(out)[:max(k, 0)]

    # ---- Groth16
    @staticmethod
    def _csr(rp, col, coeff):
        s = Csr()
        s.num_rows = len(rp) - 1
        s.row_ptr, s.col, s.coeff = rp.ctypes.data, col.ctypes.data, coeff.ctypes.data
        return s

    def witness_map(self, field, r1cs):
        """R1CSToQAP::witness_map: r1cs has rp_/col_/coeff_{a,b,c}, z, num_inputs (any object with those numpy arrays)."""
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        n = lib().pcdhip_domain_size(field, C.c_size_t(r1cs.num_constraints + r1cs.num_inputs))
        h = np.zeros((n, FIELD_LIMBS[field]), dtype=np.uint64)
        self._check(lib().pcdhip_groth16_witness_map(self._ctx, field, C.byref(A), C.byref(B), C.byref(Cm), _p(r1cs.z),
                                                     C.c_size_t(r1cs.num_vars), C.c_size_t(r1cs.num_inputs), _p(h)))
        return h

    def g16_pk_upload(self, host_struct, curve):
        h = C.c_void_p()
        self._check(lib().pcdhip_g16_pk_upload(self._ctx, C.byref(host_struct), C.byref(h)))
        return G16Pk(self, h, curve)

    def g16_pk_set_r1cs(self, pk, r1cs):
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        self._check(lib().pcdhip_g16_pk_set_r1cs(self._ctx, pk._h, C.byref(A), C.byref(B), C.byref(Cm)))

    def witness_map_resident(self, pk, r1cs, want_h=True):
        """witness map alone over the matrices resident with pk -> (h or None, {"spmv", "transforms", "total"} device ms)."""
        n = lib().pcdhip_domain_size(CURVE_FR[pk.curve], C.c_size_t(r1cs.num_constraints + r1cs.num_inputs))
        h = np.zeros((n, FIELD_LIMBS[CURVE_FR[pk.curve]]), dtype=np.uint64) if want_h else None
        ms = (C.c_float * 3)()
        self._check(lib().pcdhip_g16_witness_map_resident(self._ctx, pk._h, _p(r1cs.z), _p(h), ms))
        return h, dict(zip(["spmv", "transforms", "total"], list(ms)))

    def groth16_prove(self, pk, r1cs, r_mont, s_mont, resident_r1cs=False):
        """create_proof after synthesis -> (proof A||B||C affine limbs, inf flags[3]).  With resident_r1cs the
        matrices set by g16_pk_set_r1cs are used and only z is uploaded."""
        w1, w2 = point_limbs(pk.curve, G1), point_limbs(pk.curve, G2)
        proof = np.zeros(2 * w1 + w2, dtype=np.uint64)
        inf = np.zeros(3, dtype=np.uint8)
        if resident_r1cs:
            self._check(lib().pcdhip_groth16_prove(self._ctx, pk._h, None, None, None, _p(r1cs.z),
                                                   _p(_u64(r_mont)), _p(_u64(s_mont)), _p(proof), _p(inf)))
            return proof, inf
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        self._check(lib().pcdhip_groth16_prove(self._ctx, pk._h, C.byref(A), C.byref(B), C.byref(Cm), _p(r1cs.z),
                                               _p(_u64(r_mont)), _p(_u64(s_mont)), _p(proof), _p(inf)))
        return proof, inf

    def g16_pk_info(self, pk):
        """{query: (window bits, windows)} of a resident key's a / b_g1 / b_g2 / l / h queries"""
        c, w = (C.c_int * 5)(), (C.c_int * 5)()
        self._check(lib().pcdhip_g16_pk_info(pk._h, c, w))
        return {k: (int(c[i]), int(w[i])) for i, k in enumerate(("a", "b_g1", "b_g2", "l", "h"))}

    def g16_pk_memory(self, pk):
        """device bytes of a resident key's base vectors: {"ordinary", "sparse_window", "copies", "sparse_copies"}"""
        out = (C.c_uint64 * 4)()
        self._check(lib().pcdhip_g16_pk_memory(pk._h, out))
        return {"ordinary": int(out[0]), "sparse_window": int(out[1]), "copies": int(out[2]), "sparse_copies": int(out[3])}

    def groth16_set_sparse_window(self, bits):
        """0 off (default), -1 automatic, 6..22 forced window bits of the sparse-assignment copies (takes effect at the next key upload)"""
        self._check(lib().pcdhip_groth16_set_sparse_window(self._ctx, int(bits)))

    def groth16_last_plan(self):
        """(the last proof ran its assignment MSMs on the sparse-window copies, its count of general scalars)"""
        out = (C.c_uint32 * 2)()
        self._check(lib().pcdhip_groth16_last_plan(self._ctx, out))
        return bool(out[0]), int(out[1])

    def groth16_set_assembly(self, mode):
        """0: automatic (default); 1: s*A, r*B_1 folded into two extra MSMs; 2: chained one-lane products overlapping the other MSMs."""
        self._check(lib().pcdhip_groth16_set_assembly(self._ctx, int(mode)))

    def groth16_set_schedule(self, mode):
        """0 (default): the assignment MSMs first, the witness map under them; 1: the witness map first, then all five MSMs at once;
        2: the witness map first, then the accumulate lane (round 5; measured slower, see include/pcdhip.h)"""
        self._check(lib().pcdhip_groth16_set_schedule(self._ctx, int(mode)))

    def set_lane_reserve(self, cus):
        """compute units the accumulate lane leaves to the other streams (-1: default 8 / PCDHIP_LANE_RESERVE; 0: no CU mask)"""
        self._check(lib().pcdhip_set_lane_reserve(self._ctx, int(cus)))

    def groth16_set_witness_split(self, on):
        """multi-device contexts of >= 3 devices: the witness map's a / b / c chains on devices 0 / 1 / 2 (default) or all on device 0"""
        self._check(lib().pcdhip_groth16_set_witness_split(self._ctx, int(bool(on))))

    def groth16_last_timings(self):
        out = (C.c_float * 8)()
        self._check(lib().pcdhip_groth16_last_timings(self._ctx, out))
        return dict(zip(["witness_map", "msm_h", "msm_l", "msm_a", "msm_b_g1", "msm_b_g2", "assembly", "total"], list(out)))

    # ---- key generation
    def fixed_base_mul(self, curve, group, base_xy, scalars_canonical):
        """FixedBaseMSM::multi_scalar_mul + batch normalisation: (n affine points, n flags) = scalars[i] * base."""
        sc = _u64(scalars_canonical).reshape(-1, FIELD_LIMBS[CURVE_FR[curve]])
        n = sc.shape[0]
        out = np.zeros((n, point_limbs(curve, group)), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        self._check(lib().pcdhip_fixed_base_mul(self._ctx, curve, group, _p(_u64(base_xy)), _p(sc), C.c_size_t(n), _p(out), _p(inf)))
        return out, inf

    def groth16_setup(self, curve, r1cs, g1_xy, g2_xy, toxic_mont):
        """ark-groth16 generate_parameters after synthesis (circuit_specific_setup, src/ec_cycle_pcd/mod.rs:69,78);
        toxic_mont = (alpha, beta, gamma, delta, tau).  Returns a dict of arrays named like the key's fields."""
        w1, w2 = point_limbs(curve, G1), point_limbs(curve, G2)
        m, ni = r1cs.num_vars, r1cs.num_inputs
        n = lib().pcdhip_domain_size(CURVE_FR[curve], C.c_size_t(r1cs.num_constraints + ni))
        z64 = lambda *sh: np.zeros(sh, dtype=np.uint64)
        z8 = lambda k: np.zeros(k, dtype=np.uint8)
        K = dict(alpha_g1=z64(w1), beta_g1=z64(w1), delta_g1=z64(w1), beta_g2=z64(w2), gamma_g2=z64(w2), delta_g2=z64(w2),
                 a_query=z64(m, w1), a_inf=z8(m), b_g1_query=z64(m, w1), b_g1_inf=z8(m), b_g2_query=z64(m, w2), b_g2_inf=z8(m),
                 h_query=z64(max(n - 1, 0), w1), h_inf=z8(max(n - 1, 0)), l_query=z64(m - ni, w1), l_inf=z8(m - ni),
                 gamma_abc_g1=z64(ni, w1), gamma_abc_inf=z8(ni))
        out = G16SetupOut()
        for name, _ in G16SetupOut._fields_:
            if name != "domain_size":
                setattr(out, name, K[name].ctypes.data if K[name].size else None)
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        self._check(lib().pcdhip_groth16_setup(self._ctx, curve, C.byref(A), C.byref(B), C.byref(Cm), C.c_size_t(m), C.c_size_t(ni),
                                               _p(_u64(g1_xy)), _p(_u64(g2_xy)), _p(_u64(toxic_mont)), C.byref(out)))
        assert out.domain_size == n
        K["domain_size"] = n
        return K

    # ---- pairing
    def multi_pairing(self, curve, g1_xy, g2_xy, g1_inf=None, g2_inf=None):
        """product_of_pairings: final_exponentiation(prod miller_loop(P_i, Q_i)) -> GT limbs (tower order)."""
        g1 = _u64(g1_xy).reshape(-1, point_limbs(curve, G1))
        g2 = _u64(g2_xy).reshape(-1, point_limbs(curve, G2))
        n = g1.shape[0]
        out = np.zeros(2 * CURVE_G2_DEG[curve] * FIELD_LIMBS[CURVE_FQ[curve]], dtype=np.uint64)
        i1 = np.ascontiguousarray(g1_inf, dtype=np.uint8) if g1_inf is not None else None
        i2 = np.ascontiguousarray(g2_inf, dtype=np.uint8) if g2_inf is not None else None
        self._check(lib().pcdhip_multi_pairing(self._ctx, curve, _p(g1), _p(i1), _p(g2), _p(i2), C.c_size_t(n), _p(out)))
        return out

    def pairing_set_mode(self, mode):
        """0: one wave per pairing for batches up to 4096 pairs (default); 1: always one lane per pairing."""
        self._check(lib().pcdhip_pairing_set_mode(self._ctx, int(mode)))

    def groth16_verify(self, curve, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, public_inputs_canonical, proof,
                       gamma_abc_inf=None, proof_inf=None):
        """Groth16::verify (reference call site src/ec_cycle_pcd/mod.rs:239)."""
        abc = _u64(gamma_abc_g1).reshape(-1, point_limbs(curve, G1))
        ok = C.c_int(0)
        pi = _u64(public_inputs_canonical)
        gi = np.ascontiguousarray(gamma_abc_inf, dtype=np.uint8) if gamma_abc_inf is not None else None
        pinf = np.ascontiguousarray(proof_inf, dtype=np.uint8) if proof_inf is not None else None
        self._check(lib().pcdhip_groth16_verify(self._ctx, curve, _p(_u64(alpha_g1)), _p(_u64(beta_g2)), _p(_u64(gamma_g2)),
                                                _p(_u64(delta_g2)), _p(abc), _p(gi), C.c_size_t(abc.shape[0]), _p(pi),
                                                _p(_u64(proof)), _p(pinf), C.byref(ok)))
        return ok.value == 1

    def groth16_verify_batch(self, curve, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, public_inputs_canonical, proofs,
                             gamma_abc_inf=None, proofs_inf=None):
        """n Groth16 verifications under one key (the inputs of a merge node) with all Miller loops in one launch -> bool array."""
        abc = _u64(gamma_abc_g1).reshape(-1, point_limbs(curve, G1))
        ni = abc.shape[0]
        pr = _u64(proofs).reshape(-1, 2 * point_limbs(curve, G1) + point_limbs(curve, G2))
        k = pr.shape[0]
        pi = _u64(public_inputs_canonical).reshape(k, (ni - 1) * FIELD_LIMBS[CURVE_FR[curve]]) if ni > 1 else None
        ok = (C.c_int * max(k, 1))()
        gi = np.ascontiguousarray(gamma_abc_inf, dtype=np.uint8) if gamma_abc_inf is not None else None
        pinf = np.ascontiguousarray(proofs_inf, dtype=np.uint8) if proofs_inf is not None else None
        self._check(lib().pcdhip_groth16_verify_batch(self._ctx, curve, _p(_u64(alpha_g1)), _p(_u64(beta_g2)), _p(_u64(gamma_g2)),
                                                      _p(_u64(delta_g2)), _p(abc), _p(gi), C.c_size_t(ni), C.c_size_t(k), _p(pi), _p(pr),
                                                      _p(pinf), ok))
        return np.array([ok[i] == 1 for i in range(k)])

    def process_vk(self, curve, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, gamma_abc_inf=None):
        """SNARK::process_vk: e(alpha, beta) cached, gamma / delta negated, gamma_abc resident."""
        abc = _u64(gamma_abc_g1).reshape(-1, point_limbs(curve, G1))
        gi = np.ascontiguousarray(gamma_abc_inf, dtype=np.uint8) if gamma_abc_inf is not None else None
        h = C.c_void_p()
        self._check(lib().pcdhip_process_vk(self._ctx, curve, _p(_u64(alpha_g1)), _p(_u64(beta_g2)), _p(_u64(gamma_g2)), _p(_u64(delta_g2)),
                                            _p(abc), _p(gi), C.c_size_t(abc.shape[0]), C.byref(h)))
        return Pvk(self, h, curve, abc.shape[0])

    def _proof_batch(self, pvk, public_inputs_canonical, proofs, proofs_inf):
        pr = _u64(proofs).reshape(-1, 2 * point_limbs(pvk.curve, G1) + point_limbs(pvk.curve, G2))
        k = pr.shape[0]
        pi = _u64(public_inputs_canonical).reshape(k, (pvk.num_inputs - 1) * FIELD_LIMBS[CURVE_FR[pvk.curve]]) if pvk.num_inputs > 1 else None
        pinf = np.ascontiguousarray(proofs_inf, dtype=np.uint8) if proofs_inf is not None else None
        return pr, k, pi, pinf

    def groth16_verify_prepared(self, pvk, public_inputs_canonical, proofs, proofs_inf=None):
        """verify_with_processed_vk for n proofs -> bool array (3 Miller loops + 1 final exponentiation per proof)."""
        pr, k, pi, pinf = self._proof_batch(pvk, public_inputs_canonical, proofs, proofs_inf)
        ok = (C.c_int * max(k, 1))()
        self._check(lib().pcdhip_groth16_verify_prepared(self._ctx, pvk._h, C.c_size_t(k), _p(pi), _p(pr), _p(pinf), ok))
        return np.array([ok[i] == 1 for i in range(k)])

    def groth16_verify_batch_rlc(self, pvk, public_inputs_canonical, proofs, rho, proofs_inf=None):
        """all n proofs with ONE shared final exponentiation; rho: (n, 2) uint64 non-zero 128-bit challenges -> bool."""
        pr, k, pi, pinf = self._proof_batch(pvk, public_inputs_canonical, proofs, proofs_inf)
        rho = _u64(rho).reshape(k, 2)
        ok = C.c_int(0)
        self._check(lib().pcdhip_groth16_verify_batch_rlc(self._ctx, pvk._h, C.c_size_t(k), _p(pi), _p(pr), _p(pinf), _p(rho), C.byref(ok)))
        return ok.value == 1

    # ---- K7: the open side of KZG10 / MarlinKZG10
    @staticmethod
    def _polys(polys, lens):
        lens = [p.n for p in polys] if lens is None else [int(x) for x in lens]
        k = len(polys)
        arr = (C.c_void_p * max(k, 1))(*[p._h.value for p in polys])
        ln = (C.c_size_t * max(k, 1))(*lens)
        return arr, ln, k

    def poly_eval(self, polys, z_mont, lens=None):
        """ark-poly `evaluate` of k polynomials (DeviceBufs of one field, lens[j] coefficients) at z -> (k, L) ABI Montgomery values"""
        arr, ln, k = self._polys(polys, lens)
        out = np.zeros((k, FIELD_LIMBS[polys[0].field] if k else 1), dtype=np.uint64)
        self._check(lib().pcdhip_poly_eval(self._ctx, arr, ln, C.c_size_t(k), _p(_u64(z_mont)), _p(out)))
        return out

    def poly_lincomb(self, polys, coeffs_mont, out, lens=None):
        """out_i = sum_j coeffs_j p_(j,i) into the DeviceBuf `out` -> the length written (the longest input)"""
        arr, ln, k = self._polys(polys, lens)
        cf = _u64(coeffs_mont) if k else np.zeros(1, dtype=np.uint64)
        n = C.c_size_t(0)
        self._check(lib().pcdhip_poly_lincomb(self._ctx, arr, ln, _p(cf), C.c_size_t(k), out._h, C.byref(n)))
        return n.value

    def poly_div_linear(self, p, z_mont, length=None, q=None):
        """p / (X - z) -> (quotient DeviceBuf of length - 1 coefficients, or None for length <= 1; p(z))"""
        length = p.n if length is None else int(length)
        own = q is None and length > 1
        if own:
            h = C.c_void_p()
            self._check(lib().pcdhip_buf_alloc(self._ctx, p.field, C.c_size_t(length - 1), C.byref(h)))
            q = DeviceBuf(self, h, p.field, length - 1)
        v = np.zeros(FIELD_LIMBS[p.field], dtype=np.uint64)
        rc = lib().pcdhip_poly_div_linear(self._ctx, p._h, C.c_size_t(length), _p(_u64(z_mont)), q._h if q is not None else None, _p(v))
        if rc and own:
            q.free()
        self._check(rc)
        return q, v

    # ---- K8: vector algebra for Marlin's AHP rounds
    def buf_alloc(self, field, n):
        h = C.c_void_p()
        self._check(lib().pcdhip_buf_alloc(self._ctx, field, C.c_size_t(n), C.byref(h)))
        return DeviceBuf(self, h, field, n)

    def _call_into(self, own, fn):
        """fn() -> rc; the buffers of `own` (allocated for this call) are freed when it fails"""
        rc = fn()
        if rc:
            for b in own:
                b.free()
        self._check(rc)

    def vec_mul(self, a, b, n=None, out=None):
        """out_i = a_i b_i for i < n (default: the shorter vector) -> out (allocated when not passed; may be a or b)"""
        n = min(a.n, b.n) if n is None else int(n)
        own = [] if out is not None else [self.buf_alloc(a.field, n)]
        out = out if out is not None else own[0]
        self._call_into(own, lambda: lib().pcdhip_vec_mul(self._ctx, a._h, b._h, n, out._h))
        return out

    def vec_batch_inverse(self, x, n=None, scale_mont=None, out=None):
        """ark-ff batch_inversion / batch_inversion_and_mul: out_i = scale / x_i, zeros stay zero -> out (may be x)"""
        n = x.n if n is None else int(n)
        own = [] if out is not None else [self.buf_alloc(x.field, n)]
        out = out if out is not None else own[0]
        sc = _p(_u64(scale_mont)) if scale_mont is not None else None
        self._call_into(own, lambda: lib().pcdhip_vec_batch_inverse(self._ctx, x._h, n, sc, out._h))
        return out

    def poly_div_vanishing(self, p, domain_n, length=None, q=None, r=None, want_r=True):
        """p = q (X^domain_n - 1) + r -> (q, q_len, r, r_len); q is None when there is no quotient, r is None with want_r=False"""
        length = p.n if length is None else int(length)
        domain_n = int(domain_n)
        ql, rl = max(length - domain_n, 0), min(length, domain_n)
        own = []
        if q is None and ql:
            q = self.buf_alloc(p.field, ql)
            own.append(q)
        if r is None and want_r:
            r = self.buf_alloc(p.field, rl)
            own.append(r)
        qn, rn = C.c_size_t(0), C.c_size_t(0)
        self._call_into(own, lambda: lib().pcdhip_poly_div_vanishing(self._ctx, p._h, length, domain_n, q._h if q is not None else None,
                                                                     C.byref(qn), r._h if r is not None else None,
                                                                     C.byref(rn) if r is not None else None))
        return q, qn.value, r, (rn.value if r is not None else None)

    def poly_mul(self, a, b, la=None, lb=None, out=None):
        """ark-poly &a * &b -> (out, la + lb - 1 coefficients, not trimmed; 0 when an operand is empty); out may be a or b"""
        la = a.n if la is None else int(la)
        lb = b.n if lb is None else int(lb)
        own = [] if out is not None else [self.buf_alloc(a.field, la + lb - 1 if la and lb else 0)]
        out = out if out is not None else own[0]
        n = C.c_size_t(0)
        self._call_into(own, lambda: lib().pcdhip_poly_mul(self._ctx, a._h, la, b._h, lb, out._h, C.byref(n)))
        return out, n.value

    # ---- K9: Marlin's AHP rounds 2 and 3
    def domain_bivariate_lagrange(self, field, domain_n, x_mont, out=None):
        """out_i = (x^domain_n - 1) / (x - w^i) over the domain of domain_n elements (all zero when x lies in it) -> out"""
        domain_n = int(domain_n)
        own = [] if out is not None else [self.buf_alloc(field, domain_n)]
        out = out if out is not None else own[0]
        self._call_into(own, lambda: lib().pcdhip_domain_bivariate_lagrange(self._ctx, field, domain_n, _p(_u64(x_mont)), out._h))
        return out

    def marlin_mats_upload(self, field, r1cs, domain_h_n, domain_x_n, num_cols=None):
        """the constraint matrices of `r1cs` (rp_/col_/coeff_{a,b,c}, num_vars) resident for marlin_t_evals: transposed, the variables at
        reindex_by_subdomain's places in H"""
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        num_cols = r1cs.num_vars if num_cols is None else int(num_cols)
        h = C.c_void_p()
        self._check(lib().pcdhip_marlin_mats_upload(self._ctx, field, C.byref(A), C.byref(B), C.byref(Cm), num_cols, int(domain_h_n),
                                                    int(domain_x_n), C.byref(h)))
        return MarlinMats(self, h, field, int(domain_h_n), int(domain_x_n), int(num_cols))

    def marlin_t_evals(self, mats, eta_mont, r_alpha, out=None):
        """t_out[j] = sum_M eta_M sum_{(r, c, v) in M, pi(c) = j} v r_alpha[r] for j < |H| -> out"""
        own = [] if out is not None else [self.buf_alloc(mats.field, mats.domain_h_n)]
        out = out if out is not None else own[0]
        eta = _u64(eta_mont).reshape(3, FIELD_LIMBS[mats.field])
        self._call_into(own, lambda: lib().pcdhip_marlin_t_evals(self._ctx, mats._h, _p(eta), r_alpha._h, out._h))
        return out

    @staticmethod
    def _three(bufs):
        if bufs is None:
            return None
        return (C.c_void_p * 3)(*[b._h.value if b is not None else None for b in bufs])

    def marlin_sumcheck_ab(self, alpha_mont, beta_mont, coeff_mont, row, col, row_col, val, n=None, a_out=None, b_out=None):
        """the rational sumcheck's a and b over the three matrices' row / col / row_col (None: the product form) / val vectors -> (a, b)"""
        n = min(x.n for x in list(row) + list(col) + list(val)) if n is None else int(n)
        f = row[0].field
        own = []
        for o in (a_out, b_out):
            if o is None:
                own.append(self.buf_alloc(f, n))
        a_out = a_out if a_out is not None else own[0]
        b_out = b_out if b_out is not None else own[-1]
        cf = _u64(coeff_mont).reshape(3, FIELD_LIMBS[f])
        self._call_into(own, lambda: lib().pcdhip_marlin_sumcheck_ab(self._ctx, _p(_u64(alpha_mont)), _p(_u64(beta_mont)), _p(cf), self._three(row),
                                                                     self._three(col), self._three(row_col), self._three(val), n, a_out._h,
                                                                     b_out._h))
        return a_out, b_out

    def marlin_sumcheck_f(self, alpha_mont, beta_mont, coeff_mont, row, col, row_col, val, n=None, out=None):
        """f_i = a_i / b_i of marlin_sumcheck_ab, 0 where b_i = 0 -> out"""
        n = min(x.n for x in list(row) + list(col) + list(val)) if n is None else int(n)
        f = row[0].field
        own = [] if out is not None else [self.buf_alloc(f, n)]
        out = out if out is not None else own[0]
        cf = _u64(coeff_mont).reshape(3, FIELD_LIMBS[f])
        self._call_into(own, lambda: lib().pcdhip_marlin_sumcheck_f(self._ctx, _p(_u64(alpha_mont)), _p(_u64(beta_mont)), _p(cf), self._three(row),
                                                                    self._three(col), self._three(row_col), self._three(val), n, out._h))
        return out

    # ---- K10: the index on device
    def marlin_index_build(self, field, r1cs, domain_h_n, domain_x_n, num_cols=None, domain_k_n=0, domain_b_n=0, keep=0):
        """the index of `r1cs` (rp_/col_/coeff_{a,b,c}, num_vars): row / col / row_col / val of A, B, C as coefficients, on K and on B
        (keep: bit 0 / 1 / 2, 0 = all; domain_k_n / domain_b_n 0 = the library's rules) -> MarlinIndex"""
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        num_cols = r1cs.num_vars if num_cols is None else int(num_cols)
        h = C.c_void_p()
        self._check(lib().pcdhip_marlin_index_build(self._ctx, field, C.byref(A), C.byref(B), C.byref(Cm), num_cols, int(domain_h_n),
                                                    int(domain_x_n), int(domain_k_n), int(domain_b_n), int(keep), C.byref(h)))
        return MarlinIndex(self, h, field)

    # ---- K11: round 1 and the first sumcheck
    def marlin_mats_upload_ex(self, field, r1cs, domain_h_n, domain_x_n, forms, num_cols=None):
        """marlin_mats_upload with a choice of forms: bit 0 the transposed matrices of marlin_t_evals, bit 1 the forward A, B, C of
        marlin_zm_evals"""
        A = self._csr(r1cs.rp_a, r1cs.col_a, r1cs.coeff_a)
        B = self._csr(r1cs.rp_b, r1cs.col_b, r1cs.coeff_b)
        Cm = self._csr(r1cs.rp_c, r1cs.col_c, r1cs.coeff_c)
        num_cols = r1cs.num_vars if num_cols is None else int(num_cols)
        h = C.c_void_p()
        self._check(lib().pcdhip_marlin_mats_upload_ex(self._ctx, field, C.byref(A), C.byref(B), C.byref(Cm), num_cols, int(domain_h_n),
                                                       int(domain_x_n), int(forms), C.byref(h)))
        return MarlinMats(self, h, field, int(domain_h_n), int(domain_x_n), int(num_cols), int(forms))

    def marlin_zm_evals(self, mats, z, za=None, zb=None, zc=None, want_c=True):
        """z_M[r] = sum_{(r, c, v) in M} v z[c] on H, zeros from num_rows up -> (za, zb, zc); zc is None with want_c=False"""
        own = []
        outs = []
        for o, want in ((za, True), (zb, True), (zc, want_c)):
            if o is None and want:
                o = self.buf_alloc(mats.field, mats.domain_h_n)
                own.append(o)
            outs.append(o)
        self._call_into(own, lambda: lib().pcdhip_marlin_zm_evals(self._ctx, mats._h, z._h, outs[0]._h, outs[1]._h,
                                                                  outs[2]._h if outs[2] is not None else None))
        return tuple(outs)

    def marlin_place_assignment(self, field, domain_h_n, domain_x_n, z, num_cols=None, out=None):
        """out[pi(c)] = z[c] over the domain_h_n places of H, zeros where no variable sits -> out"""
        num_cols = z.n if num_cols is None else int(num_cols)
        own = [] if out is not None else [self.buf_alloc(field, int(domain_h_n))]
        out = out if out is not None else own[0]
        self._call_into(own, lambda: lib().pcdhip_marlin_place_assignment(self._ctx, field, int(domain_h_n), int(domain_x_n), z._h, num_cols,
                                                                          out._h))
        return out

    def poly_add_vanishing_multiple(self, p, blind_mont, domain_n, length=None):
        """p += b(X) (X^domain_n - 1) in place for the host coefficients b (k rows; None or empty: a no-op) -> the new length"""
        length = p.n if length is None else int(length)
        b = None if blind_mont is None else _u64(blind_mont).reshape(-1, FIELD_LIMBS[p.field])
        k = 0 if b is None else b.shape[0]
        n = C.c_size_t(0)
        self._check(lib().pcdhip_poly_add_vanishing_multiple(self._ctx, p._h, length, _p(b) if k else None, k, int(domain_n), C.byref(n)))
        return n.value

    def marlin_sumcheck1_q(self, eta_mont, za, zb, r_alpha, t, z, n=None, out=None):
        """q_i = r_i (eta_A za_i + eta_B zb_i + eta_C za_i zb_i) - t_i z_i for i < n -> out (allocated when not passed; may be an input)"""
        n = min(x.n for x in (za, zb, r_alpha, t, z)) if n is None else int(n)
        own = [] if out is not None else [self.buf_alloc(za.field, n)]
        out = out if out is not None else own[0]
        eta = _u64(eta_mont).reshape(3, FIELD_LIMBS[za.field])
        self._call_into(own, lambda: lib().pcdhip_marlin_sumcheck1_q(self._ctx, _p(eta), za._h, zb._h, r_alpha._h, t._h, z._h, n, out._h))
        return out

    def marlin_round1(self, mats, z, blind_w=None, blind_a=None, blind_b=None, want_evals=False):
        """round 1 over a handle with the forward form: z (DeviceBuf of num_cols elements) and the host blinding coefficients of w, z_A,
        z_B (rows of ABI limbs; None: not hiding) -> dict of DeviceBufs x_hat, z_poly, w (None when empty), w_rem, za_poly, zb_poly, (with
        want_evals) za_evals, zb_evals, and "lens": the lengths of x_hat, z_poly, w, za_poly, zb_poly"""
        f, h_n, x_n = mats.field, mats.domain_h_n, mats.domain_x_n
        bl = [None if b is None else _u64(b).reshape(-1, FIELD_LIMBS[f]) for b in (blind_w, blind_a, blind_b)]
        k = [0 if b is None else b.shape[0] for b in bl]
        sizes = {"x_hat": x_n, "z_poly": h_n + k[0], "w": h_n + k[0] - x_n, "w_rem": x_n, "za_poly": h_n + k[1], "zb_poly": h_n + k[2]}
        if want_evals:
            sizes.update(za_evals=h_n, zb_evals=h_n)
        out = {name: (self.buf_alloc(f, n) if n else None) for name, n in sizes.items()}
        hd = lambda name: out[name]._h if out.get(name) is not None else None
        lens = (C.c_size_t * 5)()
        self._call_into([b for b in out.values() if b is not None], lambda: lib().pcdhip_marlin_round1(
            self._ctx, mats._h, z._h, _p(bl[0]) if k[0] else None, k[0], _p(bl[1]) if k[1] else None, k[1], _p(bl[2]) if k[2] else None, k[2],
            hd("x_hat"), hd("z_poly"), hd("w"), hd("w_rem"), hd("za_poly"), hd("zb_poly"), hd("za_evals"), hd("zb_evals"), lens))
        out["lens"] = [int(v) for v in lens]
        return out

    def marlin_sumcheck1(self, mats, eta_mont, alpha_mont, za_poly, zb_poly, z_poly, len_za=None, len_zb=None, len_z=None, mask=None,
                         len_mask=None, domain_d_n=0):
        """the first sumcheck over a handle with the transposed form -> dict of DeviceBufs t_poly, h1 (None when empty), g1 (None when
        empty), sigma (one element: the remainder's constant term) and "lens": the lengths of t_poly, h1, g1"""
        f, h_n = mats.field, mats.domain_h_n
        len_za = za_poly.n if len_za is None else int(len_za)
        len_zb = zb_poly.n if len_zb is None else int(len_zb)
        len_z = z_poly.n if len_z is None else int(len_z)
        len_mask = 0 if mask is None else (mask.n if len_mask is None else int(len_mask))
        q_len = max(h_n + len_za + len_zb - 2, h_n + len_z - 1, len_mask)
        sizes = {"t_poly": h_n, "h1": max(q_len - h_n, 0), "g1": h_n - 1, "sigma": 1}
        out = {name: (self.buf_alloc(f, n) if n else None) for name, n in sizes.items()}
        hd = lambda name: out[name]._h if out[name] is not None else None
        lens = (C.c_size_t * 3)()
        eta = _u64(eta_mont).reshape(3, FIELD_LIMBS[f])
        self._call_into([b for b in out.values() if b is not None], lambda: lib().pcdhip_marlin_sumcheck1(
            self._ctx, mats._h, _p(eta), _p(_u64(alpha_mont)), za_poly._h, len_za, zb_poly._h, len_zb, z_poly._h, len_z,
            mask._h if mask is not None else None, len_mask, int(domain_d_n), hd("t_poly"), hd("h1"), hd("g1"), hd("sigma"), lens))
        out["lens"] = [int(v) for v in lens]
        return out

    # ---- K12: the second sumcheck
    def marlin_sumcheck2_q(self, alpha_mont, beta_mont, coeff_mont, row, col, row_col, val, f, n=None, out=None):
        """q_i = a_i - b_i f_i for i < n, a and b those of marlin_sumcheck_ab (never stored) -> out (allocated when not passed; may be f)"""
        n = min(x.n for x in list(row) + list(col) + list(val) + [f]) if n is None else int(n)
        fld = row[0].field
        own = [] if out is not None else [self.buf_alloc(fld, n)]
        out = out if out is not None else own[0]
        cf = _u64(coeff_mont).reshape(3, FIELD_LIMBS[fld])
        self._call_into(own, lambda: lib().pcdhip_marlin_sumcheck2_q(self._ctx, _p(_u64(alpha_mont)), _p(_u64(beta_mont)), _p(cf), self._three(row),
                                                                     self._three(col), self._three(row_col), self._three(val), f._h, n, out._h))
        return out

    def marlin_sumcheck2(self, index, alpha_mont, beta_mont, coeff_mont, route=0, want_f_poly=True, want_rem=True):
        """the second sumcheck over an index that kept its evaluations on K and on B -> dict of DeviceBufs f_poly (None without
        want_f_poly), g2 and h2 (None when empty), sigma (one element), h2_rem (None without want_rem), "lens": the lengths of g2 and
        h2, and "route": the route taken (1 pointwise on B, 2 by the polynomial product)"""
        fld = index.field
        k_n = index.info()["domain_k_n"]
        sizes = {"f_poly": k_n if want_f_poly else 0, "g2": k_n - 1, "sigma": 1, "h2": 3 * k_n - 3, "h2_rem": k_n if want_rem else 0}
        out = {name: (self.buf_alloc(fld, n) if n else None) for name, n in sizes.items()}
        hd = lambda name: out[name]._h if out[name] is not None else None
        lens = (C.c_size_t * 3)()
        cf = _u64(coeff_mont).reshape(3, FIELD_LIMBS[fld])
        self._call_into([b for b in out.values() if b is not None], lambda: lib().pcdhip_marlin_sumcheck2(
            self._ctx, index._h, _p(_u64(alpha_mont)), _p(_u64(beta_mont)), _p(cf), int(route), hd("f_poly"), hd("g2"), hd("sigma"), hd("h2"),
            hd("h2_rem"), lens))
        out["lens"] = [int(lens[0]), int(lens[1])]
        out["route"] = int(lens[2])
        return out

    def fft_general_dev(self, data, n=None, inverse=False, coset=False):
        """pcdhip_fft_general on the first n (default: all) elements of a DeviceBuf, in place; n = 2^a q^b"""
        n = data.n if n is None else int(n)
        self._check(lib().pcdhip_fft_general_dev(self._ctx, data._h, n, int(inverse), int(coset)))
        return data

    def poly_evals_on_domain(self, p, domain_n, length=None, coset=False, out=None):
        """the evaluations over the domain of domain_n elements of the polynomial p (`length` coefficients, zero-padded) -> out"""
        length = p.n if length is None else int(length)
        domain_n = int(domain_n)
        own = [] if out is not None else [self.buf_alloc(p.field, domain_n)]
        out = out if out is not None else own[0]
        self._call_into(own, lambda: lib().pcdhip_poly_evals_on_domain(self._ctx, p._h, length, domain_n, int(coset), out._h))
        return out

    def kzg_open(self, powers_of_g, p, z_mont, length=None, powers_of_gamma_g=None, blinding=None, blinding_len=None):
        """KZG10::open -> (w Jacobian X||Y||Z, p(z), blinding(z) or None when there is no blinding polynomial)"""
        length = p.n if length is None else int(length)
        bl = 0 if blinding is None else (blinding.n if blinding_len is None else int(blinding_len))
        w = np.zeros(3 * point_limbs(powers_of_g.curve, powers_of_g.group) // 2, dtype=np.uint64)
        v = np.zeros(FIELD_LIMBS[p.field], dtype=np.uint64)
        rv = np.zeros_like(v)
        self._check(lib().pcdhip_kzg_open(self._ctx, powers_of_g._h, powers_of_gamma_g._h if powers_of_gamma_g is not None else None, p._h,
                                          C.c_size_t(length), blinding._h if blinding is not None else None, C.c_size_t(bl),
                                          _p(_u64(z_mont)), _p(w), _p(v), _p(rv)))
        return w, v, (rv if blinding is not None else None)

    def kzg_commit(self, powers, items, powers_of_gamma_g=None, shifted_powers=None):
        """KZG10::commit / the loop of MarlinKZG10::commit over the polynomials of one round, all on device data.  `items`: dicts with
        `poly` (DeviceBuf of ABI Montgomery coefficients, or None for the empty polynomial) and optionally `len`, `blinding`, `blinding_len`,
        `shifted` (bool), `shifted_offset`, `shifted_blinding`, `shifted_blinding_len` (lengths default to the buffers' n)
        -> (comm_xy, comm_inf, shifted_xy, shifted_inf, trimmed_len), one row per item"""
        k = len(items)
        arr = (KzgCommitItem * max(k, 1))()
        h = lambda b: b._h if b is not None else None
        ln = lambda it, key, b: 0 if b is None else int(it.get(key, b.n) if it.get(key) is not None else b.n)
        for a, it in zip(arr, items):
            p, bl, sbl = it.get("poly"), it.get("blinding"), it.get("shifted_blinding")
            a.poly, a.len = h(p), ln(it, "len", p)
            a.blinding, a.blinding_len = h(bl), ln(it, "blinding_len", bl)
            a.shifted_blinding, a.shifted_blinding_len = h(sbl), ln(it, "shifted_blinding_len", sbl)
            a.shifted_offset, a.shifted = int(it.get("shifted_offset", 0)), 1 if it.get("shifted") else 0
        l1 = point_limbs(powers.curve, G1)
        comm, sh = np.zeros((k, l1), dtype=np.uint64), np.zeros((k, l1), dtype=np.uint64)
        cinf, sinf = np.zeros(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8)
        tl = np.zeros(k, dtype=np.uint64)
        self._check(lib().pcdhip_kzg_commit(self._ctx, powers._h, h(powers_of_gamma_g), h(shifted_powers), arr if k else None, k,
                                            _p(comm), _p(cinf), _p(sh), _p(sinf), _p(tl)))
        return comm, cinf, sh, sinf, tl

    def kzg_commit_last_plan(self):
        """(large MSMs run, hiding MSMs in the batched short chain, hiding MSMs one at a time, launches of that chain) of the last
        kzg_commit"""
        out = (C.c_uint64 * 4)()
        self._check(lib().pcdhip_kzg_commit_last_plan(self._ctx, out))
        return tuple(int(v) for v in out)

    # ---- K13: a round's openings as one call
    @staticmethod
    def _kzg_items(items):
        """dicts as for kzg_commit -> the C array of pcdhip_kzg_commit_item"""
        arr = (KzgCommitItem * max(len(items), 1))()
        h = lambda b: b._h if b is not None else None
        ln = lambda it, key, b: 0 if b is None else int(it.get(key, b.n) if it.get(key) is not None else b.n)
        for a, it in zip(arr, items):
            p, bl, sbl = it.get("poly"), it.get("blinding"), it.get("shifted_blinding")
            a.poly, a.len = h(p), ln(it, "len", p)
            a.blinding, a.blinding_len = h(bl), ln(it, "blinding_len", bl)
            a.shifted_blinding, a.shifted_blinding_len = h(sbl), ln(it, "shifted_blinding_len", sbl)
            a.shifted_offset, a.shifted = int(it.get("shifted_offset", 0)), 1 if it.get("shifted") else 0
        return arr

    @staticmethod
    def _open_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont):
        L = FIELD_LIMBS[field]
        pts = _u64(points_mont).reshape(-1, L)
        P = pts.shape[0]
        a = _u64(coeffs_mont).reshape(P, m, L) if m else np.zeros((P, 1, L), dtype=np.uint64)
        s = None if shifted_coeffs_mont is None else (_u64(shifted_coeffs_mont).reshape(P, m, L) if m else np.zeros((P, 1, L), dtype=np.uint64))
        return pts, P, a, s

    def poly_open_quotients(self, field, items, points_mont, coeffs_mont, shifted_coeffs_mont=None, q_bufs=None):
        """The three launches of a round's openings (pcdhip_poly_open_quotients).  `items` as for kzg_commit; points (P, L); coefficient
        tables (P, m, L), ABI Montgomery.  -> (q_bufs, q_lens (P, 2 + m), values (P, 2 + m, L)): entry [o][0] the combined polynomial,
        [o][1] the combined blinding polynomial, [o][2 + i] the degree-bound term of item i.  q_bufs: dict (o, k) -> DeviceBuf of canonical
        scalars; allocated here from the items' lengths when not passed (the caller frees them)."""
        m = len(items)
        arr = self._kzg_items(items)
        pts, P, a, s = self._open_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont)
        own = []
        if q_bufs is None:
            q_bufs = {}
            for o in range(P):
                nza = [bool(a[o, i].any()) for i in range(m)]
                nzs = [s is not None and bool(s[o, i].any()) for i in range(m)]
                lens = {0: max([arr[i].len for i in range(m) if nza[i]], default=0),
                        1: max([arr[i].blinding_len for i in range(m) if nza[i] and arr[i].blinding] +
                               [arr[i].shifted_blinding_len for i in range(m) if nzs[i] and arr[i].shifted_blinding], default=0)}
                lens.update({2 + i: arr[i].len for i in range(m) if nzs[i]})
                for k, n in lens.items():
                    if n > 1:
                        q_bufs[(o, k)] = self.buf_alloc(field, n - 1)
                        own.append(q_bufs[(o, k)])
        tab = (C.c_void_p * max(P * (2 + m), 1))()
        for (o, k), b in q_bufs.items():
            tab[o * (2 + m) + k] = b._h.value
        q_lens = (C.c_size_t * max(P * (2 + m), 1))()
        vals = np.zeros((P, 2 + m, FIELD_LIMBS[field]), dtype=np.uint64)
        self._call_into(own, lambda: lib().pcdhip_poly_open_quotients(self._ctx, int(field), arr if m else None, m, P, _p(pts), _p(a), _p(s), tab, q_lens,
                                                                      _p(vals)))
        return q_bufs, np.array([int(x) for x in q_lens][:P * (2 + m)], dtype=np.uint64).reshape(P, 2 + m), vals

    def kzg_batch_open(self, powers, items, points_mont, coeffs_mont, shifted_coeffs_mont=None, powers_of_gamma_g=None, shifted_powers=None):
        """MarlinKZG10's open_combinations / batch_open over device-resident polynomials, one call that only queues
        (pcdhip_kzg_batch_open) -> (w_xy (P, l1), w_inf (P,), values (P, L), random_v (P, L))"""
        m = len(items)
        field = CURVE_FR[powers.curve]
        arr = self._kzg_items(items)
        pts, P, a, s = self._open_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont)
        h = lambda b: b._h if b is not None else None
        w = np.zeros((P, point_limbs(powers.curve, G1)), dtype=np.uint64)
        winf = np.zeros(P, dtype=np.uint8)
        v = np.zeros((P, FIELD_LIMBS[field]), dtype=np.uint64)
        rv = np.zeros_like(v)
        self._check(lib().pcdhip_kzg_batch_open(self._ctx, powers._h, h(powers_of_gamma_g), h(shifted_powers), arr if m else None, m, P, _p(pts),
                                                _p(a), _p(s), _p(w), _p(winf), _p(v), _p(rv)))
        return w, winf, v, rv

    def kzg_batch_open_last_plan(self):
        """(large MSMs run, hiding MSMs in the batched short chain, hiding MSMs one at a time, launches of the division chain) of the last
        kzg_batch_open"""
        out = (C.c_uint64 * 4)()
        self._check(lib().pcdhip_kzg_batch_open_last_plan(self._ctx, out))
        return tuple(int(v) for v in out)

    def kzg_check(self, curve, g_xy, h_xy, beta_h_xy, comms_xy, points_mont, values_mont, w_xy, gamma_g_xy=None, random_v_mont=None,
                  randomizers_canonical=None, comms_inf=None, w_inf=None):
        """KZG10::check (one opening) / batch_check (n openings, randomizers canonical, the first 1) -> bool"""
        l1, fl = point_limbs(curve, G1), FIELD_LIMBS[CURVE_FR[curve]]
        cm = _u64(comms_xy).reshape(-1, l1)
        n = cm.shape[0]
        arr = lambda a, w: None if a is None else _u64(a).reshape(n, w)
        flags = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
        ok = C.c_int(0)
        self._check(lib().pcdhip_kzg_check(self._ctx, curve, _p(_u64(g_xy)), _p(None if gamma_g_xy is None else _u64(gamma_g_xy)),
                                           _p(_u64(h_xy)), _p(_u64(beta_h_xy)), C.c_size_t(n), _p(cm), _p(flags(comms_inf)),
                                           _p(arr(points_mont, fl)), _p(arr(values_mont, fl)), _p(arr(w_xy, l1)), _p(flags(w_inf)),
                                           _p(arr(random_v_mont, fl)), _p(arr(randomizers_canonical, fl)), C.byref(ok)))
        return ok.value == 1

    # ---- K14: the MarlinKZG10 check
    def kzg_vk_prepare(self, curve, g_xy, h_xy, beta_h_xy, gamma_g_xy=None, shift_powers_xy=None):
        """The prepared verifier key of kzg_check_combinations (pcdhip_kzg_vk_prepare): g, gamma_g and the shift powers resident -> KzgVk"""
        l1 = point_limbs(curve, G1)
        sp = None if shift_powers_xy is None else _u64(shift_powers_xy).reshape(-1, l1)
        h = C.c_void_p()
        self._check(lib().pcdhip_kzg_vk_prepare(self._ctx, int(curve), _p(_u64(g_xy)), _p(None if gamma_g_xy is None else _u64(gamma_g_xy)),
                                                _p(_u64(h_xy)), _p(_u64(beta_h_xy)), _p(sp), 0 if sp is None else sp.shape[0], C.byref(h)))
        return KzgVk(self, h, curve, 0 if sp is None else sp.shape[0])

    @staticmethod
    def _check_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont, values_mont, random_v_mont, item_values_mont, randomizers_canonical,
                      shift_index):
        L = FIELD_LIMBS[field]
        pts, P, a, s = Context._open_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont)
        row = lambda x: None if x is None else _u64(x).reshape(P, L)
        iv = None if item_values_mont is None else (_u64(item_values_mont).reshape(P, m, L) if m else np.zeros((P, 1, L), dtype=np.uint64))
        idx = None if shift_index is None else np.ascontiguousarray(shift_index, dtype=np.int32).reshape(m)
        return pts, P, a, s, row(values_mont), row(random_v_mont), iv, row(randomizers_canonical), idx

    def kzg_check_scalars(self, field, n_shift, points_mont, coeffs_mont, values_mont, shifted_coeffs_mont=None, random_v_mont=None,
                          item_values_mont=None, randomizers_canonical=None, shift_index=None):
        """The scalar collapse of the check alone (pcdhip_kzg_check_scalars) -> (left (E, N, L), right (E, P, L)) canonical, N = 2 + n_shift +
        2 m + P in the order g, gamma_g, shift powers, commitments, shifted commitments, witnesses; E = 1 with randomizers, P without"""
        L = FIELD_LIMBS[field]
        n_pts = np.size(points_mont) // L
        m = np.size(coeffs_mont) // (n_pts * L) if n_pts else 0
        pts, P, a, s, v, rv, iv, rnd, idx = self._check_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont, values_mont, random_v_mont,
                                                               item_values_mont, randomizers_canonical, shift_index)
        E, N = (1 if rnd is not None else P), 2 + n_shift + 2 * m + P
        left, right = np.zeros((E, N, L), dtype=np.uint64), np.zeros((E, P, L), dtype=np.uint64)
        self._check(lib().pcdhip_kzg_check_scalars(self._ctx, int(field), n_shift, m, _p(idx), P, _p(pts), _p(a), _p(s), _p(v), _p(rv), _p(iv), _p(rnd),
                                                   _p(left), _p(right)))
        return left, right

    def kzg_check_combinations(self, vk, comm_xy, points_mont, coeffs_mont, values_mont, w_xy, shifted_coeffs_mont=None, random_v_mont=None,
                               item_values_mont=None, randomizers_canonical=None, shift_index=None, shifted_xy=None, comm_inf=None,
                               shifted_inf=None, w_inf=None):
        """MarlinKZG10's check_combinations / batch_check as one queued call (pcdhip_kzg_check_combinations).  The tables are those of
        kzg_batch_open.  With randomizers (P canonical scalars, the first 1) -> one bool; without -> a list of P bools, one per opening."""
        curve = vk.curve
        field, l1 = CURVE_FR[curve], point_limbs(curve, G1)
        cm = _u64(comm_xy).reshape(-1, l1)
        m = cm.shape[0]
        pts, P, a, s, v, rv, iv, rnd, idx = self._check_tables(field, m, points_mont, coeffs_mont, shifted_coeffs_mont, values_mont, random_v_mont,
                                                               item_values_mont, randomizers_canonical, shift_index)
        flags = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint8)
        sh = None if shifted_xy is None else _u64(shifted_xy).reshape(m, l1)
        ok = (C.c_int * max(P, 1))()
        self._check(lib().pcdhip_kzg_check_combinations(self._ctx, vk._h, m, _p(cm) if m else None, _p(flags(comm_inf)), _p(sh), _p(flags(shifted_inf)),
                                                        _p(idx), P, _p(pts), _p(a), _p(s), _p(v), _p(rv), _p(iv), _p(_u64(w_xy).reshape(P, l1)),
                                                        _p(flags(w_inf)), _p(rnd), ok))
        return ok[0] == 1 if (rnd is not None or P == 0) else [x == 1 for x in ok[:P]]

    def kzg_check_combinations_last_plan(self):
        """(equations run, pairs of the left MSM, kernel launches of the chain, host waits) of the last kzg_check_combinations"""
        out = (C.c_uint64 * 4)()
        self._check(lib().pcdhip_kzg_check_combinations_last_plan(self._ctx, out))
        return tuple(int(v) for v in out)

    # ---- timing
    def timer_start(self):
        self._check(lib().pcdhip_timer_start(self._ctx))

    def timer_stop(self):
        ms = C.c_float()
        self._check(lib().pcdhip_timer_stop(self._ctx, C.byref(ms)))
        return ms.value


# ---- wire format (host-side: no context, no GPU)
def _wire_check(rc):
    if rc != 0:
        raise PcdHipError(f"{lib().pcdhip_strerror(rc).decode()} (rc={rc})")


def serialize_points(curve, group, xy, inf=None, compressed=True):
    """CanonicalSerialize of n affine points -> bytes."""
    xy = _u64(xy).reshape(-1, point_limbs(curve, group))
    n = xy.shape[0]
    infp = np.ascontiguousarray(inf, dtype=np.uint8) if inf is not None else None
    out = np.zeros(n * lib().pcdhip_serialized_size(curve, group, int(compressed)), dtype=np.uint8)
    _wire_check(lib().pcdhip_serialize_points(curve, group, _p(xy), _p(infp), C.c_size_t(n), int(compressed), _p(out)))
    return out.tobytes()


def deserialize_points(curve, group, data, n, compressed=True, unchecked=False):
    """CanonicalDeserialize of n affine points; unchecked=True skips the G2 subgroup test (`deserialize_unchecked`)."""
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    xy = np.zeros((n, point_limbs(curve, group)), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    fn = lib().pcdhip_deserialize_points_unchecked if unchecked else lib().pcdhip_deserialize_points
    _wire_check(fn(curve, group, _p(buf), C.c_size_t(n), int(compressed), _p(xy), _p(inf)))
    return xy, inf


def proof_serialize(curve, proof, proof_inf=None, compressed=True):
    out = np.zeros(lib().pcdhip_proof_serialized_size(curve, int(compressed)), dtype=np.uint8)
    pinf = np.ascontiguousarray(proof_inf, dtype=np.uint8) if proof_inf is not None else None
    _wire_check(lib().pcdhip_proof_serialize(curve, _p(_u64(proof)), _p(pinf), int(compressed), _p(out)))
    return out.tobytes()


def proof_deserialize(curve, data, compressed=True):
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    proof = np.zeros(2 * point_limbs(curve, G1) + point_limbs(curve, G2), dtype=np.uint64)
    inf = np.zeros(3, dtype=np.uint8)
    _wire_check(lib().pcdhip_proof_deserialize(curve, _p(buf), int(compressed), _p(proof), _p(inf)))
    return proof, inf


def vk_serialize(curve, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, gamma_abc_inf=None, compressed=True):
    abc = _u64(gamma_abc_g1).reshape(-1, point_limbs(curve, G1))
    ni = abc.shape[0]
    gi = np.ascontiguousarray(gamma_abc_inf, dtype=np.uint8) if gamma_abc_inf is not None else None
    out = np.zeros(lib().pcdhip_vk_serialized_size(curve, C.c_size_t(ni), int(compressed)), dtype=np.uint8)
    _wire_check(lib().pcdhip_vk_serialize(curve, _p(_u64(alpha_g1)), _p(_u64(beta_g2)), _p(_u64(gamma_g2)), _p(_u64(delta_g2)), _p(abc), _p(gi),
                                          C.c_size_t(ni), int(compressed), _p(out)))
    return out.tobytes()


def vk_deserialize(curve, data, compressed=True, max_inputs=1 << 16):
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    l1, l2 = point_limbs(curve, G1), point_limbs(curve, G2)
    a, b, g, d = (np.zeros(k, dtype=np.uint64) for k in (l1, l2, l2, l2))
    abc = np.zeros((max_inputs, l1), dtype=np.uint64)
    inf = np.zeros(max_inputs, dtype=np.uint8)
    cnt = C.c_size_t(0)
    _wire_check(lib().pcdhip_vk_deserialize(curve, _p(buf), C.c_size_t(len(buf)), int(compressed), _p(a), _p(b), _p(g), _p(d), _p(abc), _p(inf),
                                            C.c_size_t(max_inputs), C.byref(cnt)))
    return dict(alpha_g1=a, beta_g2=b, gamma_g2=g, delta_g2=d, gamma_abc_g1=abc[:cnt.value].copy(), gamma_abc_inf=inf[:cnt.value].copy())


def pinned_like(a):
    """Copy of `a` in page-locked host memory (pcdhip_host_alloc); the array keeps the allocation alive."""
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    rc = lib().pcdhip_host_alloc(C.c_size_t(max(a.nbytes, 1)), C.byref(p))
    if rc:
        raise PcdHipError(f"pcdhip_host_alloc: {lib().pcdhip_strerror(rc).decode()}")
    buf = (C.c_char * max(a.nbytes, 1)).from_address(p.value)
    out = np.frombuffer(buf, dtype=a.dtype, count=a.size).reshape(a.shape)
    out[...] = a
    _PINNED.append((out, p))   # freed at interpreter exit with the process
    return out


_PINNED = []


class G16SetupOut(C.Structure):
    """Mirror of `pcdhip_g16_setup_out` (include/pcdhip.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2", "a_query", "a_inf",
                                          "b_g1_query", "b_g1_inf", "b_g2_query", "b_g2_inf", "h_query", "h_inf", "l_query", "l_inf",
                                          "gamma_abc_g1", "gamma_abc_inf")] + [("domain_size", C.c_uint64)]


class DeviceBuf:
    def __init__(self, ctx, h, field, n):
        self.ctx, self._h, self.field, self.n = ctx, h, field, n

    def download(self):
        out = np.zeros((self.n, FIELD_LIMBS[self.field]), dtype=np.uint64)
        self.ctx._check(lib().pcdhip_buf_download(self.ctx._ctx, self._h, _p(out), C.c_size_t(self.n)))
        return out

    def free(self):
        if self._h:
            lib().pcdhip_buf_free(self.ctx._ctx, self._h)
            self._h = None


class MarlinMats:
    def __init__(self, ctx, h, field, domain_h_n, domain_x_n=None, num_cols=None, forms=1):
        self.ctx, self._h, self.field, self.domain_h_n = ctx, h, field, domain_h_n
        self.domain_x_n, self.num_cols, self.forms = domain_x_n, num_cols, forms

    def info(self):
        """{"seg_len", "segments", "long_outputs", "launches"} of this handle (pcdhip_marlin_mats_info)"""
        out = (C.c_uint64 * 4)()
        self.ctx._check(lib().pcdhip_marlin_mats_info(self._h, out))
        return dict(zip(["seg_len", "segments", "long_outputs", "launches"], [int(v) for v in out]))

    def free(self):
        if self._h:
            lib().pcdhip_marlin_mats_free(self.ctx._ctx, self._h)
            self._h = None


class BorrowedBuf(DeviceBuf):
    """a DeviceBuf that another handle owns (MarlinIndex.vec): free() leaves the device memory alone"""

    def free(self):
        self._h = None


class MarlinIndex:
    """pcdhip_marlin_index: form 0 coefficients / 1 evaluations on K / 2 evaluations on B; matrix 0..2 = A, B, C; poly 0..3 = row,
    col, row_col, val"""

    def __init__(self, ctx, h, field):
        self.ctx, self._h, self.field = ctx, h, field

    def info(self):
        """{"domain_k_n", "domain_b_n", "max_nnz", "device_bytes"} (pcdhip_marlin_index_info)"""
        out = (C.c_uint64 * 4)()
        self.ctx._check(lib().pcdhip_marlin_index_info(self._h, out))
        return dict(zip(["domain_k_n", "domain_b_n", "max_nnz", "device_bytes"], [int(v) for v in out]))

    def timings(self):
        """{"arith_ms", "inverse_ms", "extend_ms"}: device time of the build's parts (pcdhip_marlin_index_timings)"""
        out = (C.c_float * 3)()
        self.ctx._check(lib().pcdhip_marlin_index_timings(self._h, out))
        return dict(zip(["arith_ms", "inverse_ms", "extend_ms"], [float(v) for v in out]))

    def vec(self, form, matrix, poly):
        """one vector as a borrowed DeviceBuf, valid until the index is freed"""
        b = C.c_void_p()
        self.ctx._check(lib().pcdhip_marlin_index_vec(self._h, int(form), int(matrix), int(poly), C.byref(b)))
        i = self.info()
        return BorrowedBuf(self.ctx, b, self.field, i["domain_b_n"] if form == 2 else i["domain_k_n"])

    def vecs(self, form):
        """(row, col, row_col, val), each a list of the three matrices' vectors: the arguments of marlin_sumcheck_ab / _f"""
        return tuple([self.vec(form, m, q) for m in range(3)] for q in range(4))

    def commit(self, powers):
        """the twelve index commitments, matrix-major -> (comm_xy (12, L), comm_inf (12,))"""
        comm = np.zeros((12, point_limbs(powers.curve, G1)), dtype=np.uint64)
        cinf = np.zeros(12, dtype=np.uint8)
        self.ctx._check(lib().pcdhip_marlin_index_commit(self.ctx._ctx, self._h, powers._h, _p(comm), _p(cinf)))
        return comm, cinf

    def free(self):
        if self._h:
            lib().pcdhip_marlin_index_free(self.ctx._ctx, self._h)
            self._h = None


class Bases:
    def __init__(self, ctx, h, curve, group, n):
        self.ctx, self._h, self.curve, self.group, self.n = ctx, h, curve, group, n

    def free(self):
        if self._h:
            lib().pcdhip_bases_free(self.ctx._ctx, self._h)
            self._h = None


class Pvk:
    def __init__(self, ctx, h, curve, num_inputs):
        self.ctx, self._h, self.curve, self.num_inputs = ctx, h, curve, num_inputs

    def free(self):
        if self._h:
            lib().pcdhip_pvk_free(self.ctx._ctx, self._h)
            self._h = None


class KzgVk:
    def __init__(self, ctx, h, curve, n_shift):
        self.ctx, self._h, self.curve, self.n_shift = ctx, h, curve, n_shift

    def free(self):
        if self._h:
            lib().pcdhip_kzg_vk_free(self.ctx._ctx, self._h)
            self._h = None


class G16Pk:
    def __init__(self, ctx, h, curve):
        self.ctx, self._h, self.curve = ctx, h, curve

    def free(self):
        if self._h:
            lib().pcdhip_g16_pk_free(self.ctx._ctx, self._h)
            self._h = None
