"""Exact-integer reference for the K7 tests (tests/test_kzg_open_host.py, tests/test_gpu_kzg_open.py): polynomial division by
(X - z), Horner evaluation and linear combinations over the scalar fields, with the moduli of oracle/params.json.  Field elements
cross to the library's ABI image (Montgomery limbs) through the oracle's own conversions (co.fp_op)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "oracle", "params.json")) as _f:
    _FIELDS = json.load(_f)["fields"]
assert [f["name"] for f in _FIELDS][:4] == ["F298A", "F298B", "F753A", "F753B"]
MODULI = [int(f["p"]) for f in _FIELDS[:4]]
LIMBS = [5, 5, 12, 12]


def ints_of_limbs(a):
    """rows of little-endian u64 limbs -> Python integers"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return []
    a = a.reshape(a.shape[0], -1)
    raw = a.tobytes()
    w = a.shape[1] * 8
    return [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(a.shape[0])]


def limbs_of_ints(xs, limbs):
    raw = b"".join(int(x).to_bytes(8 * limbs, "little") for x in xs)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(xs), limbs).copy()


def to_ints(co, field, mont):
    """ABI Montgomery rows -> canonical integers"""
    mont = np.ascontiguousarray(mont, dtype=np.uint64).reshape(-1, LIMBS[field])
    return ints_of_limbs(co.fp_op(field, "to_canonical", mont)) if mont.shape[0] else []


def to_mont(co, field, xs):
    """integers -> ABI Montgomery rows"""
    if len(xs) == 0:
        return np.zeros((0, LIMBS[field]), dtype=np.uint64)
    return co.fp_op(field, "from_canonical", limbs_of_ints([x % MODULI[field] for x in xs], LIMBS[field]))


def div_linear(coeffs, z, p):
    """p(X) = q(X)(X - z) + v: (q, v) by the recurrence q_(d-1) = p_d, q_(i-1) = p_i + z q_i, v = p_0 + z q_0"""
    n = len(coeffs)
    if n == 0:
        return [], 0
    q = [0] * (n - 1)
    h = 0
    for i in range(n - 1, 0, -1):
        h = (coeffs[i] + z * h) % p
        q[i - 1] = h
    return q, (coeffs[0] + z * h) % p


def horner(coeffs, z, p):
    h = 0
    for c in reversed(coeffs):
        h = (c + z * h) % p
    return h


def lincomb(polys, cs, p):
    n = max((len(a) for a in polys), default=0)
    out = [0] * n
    for a, c in zip(polys, cs):
        for i, x in enumerate(a):
            out[i] = (out[i] + c * x) % p
    return out
