"""TEST INFRASTRUCTURE: Groth16 verification cases with a known verdict, without a circuit -- "trapdoor keys".

With the discrete logarithms of a verifying key known, a valid proof exists for ANY public inputs and ANY gamma_abc.  All scalar arithmetic
is Python integers mod r (r = the curve's scalar modulus, oracle/params.json through oracle/pyoracle.py):

  key     a, b, c, d in [1, r), s_0 .. s_{ni-1} in [0, r):  alpha = a G1, beta = b G2, gamma = c G2, delta = d G2, gamma_abc[j] = s_j G1
          (s_j = 0: the point is flagged infinity and its coordinates are zero)
  proof   for the inputs x_1 .. x_{ni-1} (x_0 = 1) let S = sum_j x_j s_j; with u, v in [1, r):  A = u G1, B = v G2,
          w = (u v - a b - S c) / d, C = w G1
  why     e(A, B) = e(alpha, beta) e(acc, gamma) e(C, delta) with acc = S G1  <=>  u v = a b + S c + w d

so the verdict of every case below is known by construction; the C++ oracle's own pairing check (oracle/coracle.py groth16_verify) is the
second witness (tests/test_verify_inputs_host.py), and the points themselves come from its fixed_base_mul.  `cases(cid)` is the one case
list, used unchanged by the host test and by tests/test_gpu_verify_inputs.py.  No GPU, no library."""
import collections
import hashlib
import random

import numpy as np

from oracle import pyoracle as O

Case = collections.namedtuple("Case", "name s members")
# xs: the public inputs SUBMITTED (Python ints, without the leading 1); expect_accept: the verdict.  The proof is the one made for the
# inputs proof_xs (force_c_infinite: with u solved so that w = 0), then, for c_is_alpha, with C replaced by the key's alpha.
Member = collections.namedtuple("Member", "xs expect_accept proof_xs force_c_infinite c_is_alpha")
Built = collections.namedtuple("Built", "key pubs proofs proofs_inf expect")


def scalar_modulus(cid):
    return O.CURVES[cid].fr.p


def num_windows(cid):
    """8-bit windows of the verifier's input tables: ceil(bits(r) / 8)"""
    return (scalar_modulus(cid).bit_length() + 7) // 8


def _rng(*tag):
    return random.Random(int.from_bytes(hashlib.sha256(repr(tag).encode()).digest()[:8], "little"))


def scalar_words(cid, xs):
    """Python ints (< 2^(64 L), reduced or not) -> (n, L) little-endian u64 limbs, the C-ABI image of canonical scalars"""
    L = O.CURVES[cid].fr.n64
    out = np.zeros((len(xs), L), dtype=np.uint64)
    for i, x in enumerate(xs):
        assert 0 <= x < 1 << (64 * L)
        for k in range(L):
            out[i, k] = (x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def mont(co, cid, xs):
    """reduced Python ints -> Montgomery limbs (what co.groth16_verify takes)"""
    assert all(0 <= x < scalar_modulus(cid) for x in xs)
    w = scalar_words(cid, xs)
    return co.fp_op(co.CURVE_FR[cid], "from_canonical", w) if len(xs) else w


def _multiples(co, cid, group, ks):
    """k G for the group's generator -> (affine points, flags); a flagged point has zero coordinates"""
    xy, inf = co.fixed_base_mul(cid, group, co.generator(cid, group), scalar_words(cid, ks))
    xy[inf != 0] = 0
    assert [bool(f) for f in inf] == [k == 0 for k in ks]
    return xy, inf


class TrapdoorKey:
    """the attributes co.groth16_verify reads, and the trapdoor"""

    def __init__(self, co, cid, s, seed):
        r = scalar_modulus(cid)
        rng = _rng("key", cid, seed)
        self.curve, self.num_inputs, self.r = cid, len(s), r
        self.a, self.b, self.c, self.d = (rng.randrange(1, r) for _ in range(4))
        self.s = [int(v) % r for v in s]
        g1, inf1 = _multiples(co, cid, 1, [self.a] + self.s)
        g2, _ = _multiples(co, cid, 2, [self.b, self.c, self.d])
        self.alpha_g1 = np.ascontiguousarray(g1[0])
        self.beta_g2, self.gamma_g2, self.delta_g2 = (np.ascontiguousarray(g2[i]) for i in range(3))
        self.gamma_abc_g1 = np.ascontiguousarray(g1[1:])
        self.gamma_abc_inf = np.ascontiguousarray(inf1[1:])

    def S(self, xs):
        """the discrete logarithm of the input accumulation"""
        assert len(xs) == self.num_inputs - 1
        return (self.s[0] + sum(x * sj for x, sj in zip(xs, self.s[1:]))) % self.r

    def args(self):
        return (self.curve, self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2, self.gamma_abc_g1)


def trapdoor_key(co, cid, s, seed):
    return TrapdoorKey(co, cid, s, seed)


def proof_scalars(key, xs, seed, force_c_infinite=False):
    """(u, v, w): the discrete logarithms of A, B, C of the proof trapdoor_proof makes"""
    r = key.r
    rng = _rng("proof", key.curve, seed)
    u, v = rng.randrange(1, r), rng.randrange(1, r)
    ab_sc = (key.a * key.b + key.S(xs) * key.c) % r
    if force_c_infinite:
        u = ab_sc * pow(v, -1, r) % r
    w = (u * v - ab_sc) * pow(key.d, -1, r) % r
    return u, v, w


def trapdoor_proofs(co, key, xs_list, seed, force_c_infinite=False):
    """one proof per input vector (proof i is seeded (seed, i)): (n x (A || B || C), n x 3 flags), the points of all of them from two
    fixed-base batches"""
    n = len(xs_list)
    uvw = [proof_scalars(key, xs, (seed, i), force_c_infinite) for i, xs in enumerate(xs_list)]
    g1, inf1 = _multiples(co, key.curve, 1, [t[0] for t in uvw] + [t[2] for t in uvw])
    g2, inf2 = _multiples(co, key.curve, 2, [t[1] for t in uvw])
    return np.concatenate([g1[:n], g2, g1[n:]], axis=1), np.stack([inf1[:n], inf2, inf1[n:]], axis=1)


def trapdoor_proof(co, key, xs, seed, force_c_infinite=False):
    """(proof = A || B || C, proof_inf = the three flags) valid under `key` for the inputs xs"""
    u, v, w = proof_scalars(key, xs, seed, force_c_infinite)
    g1, inf1 = _multiples(co, key.curve, 1, [u, w])
    g2, inf2 = _multiples(co, key.curve, 2, [v])
    return np.concatenate([g1[0], g2[0], g1[1]]), np.array([inf1[0], inf2[0], inf1[1]], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the case list
def _dot(s, xs, r):
    return (s[0] + sum(x * sj for x, sj in zip(xs, s[1:]))) % r


def _members(s, r, accepts, neighbours=True):
    """accepts: (xs, force_c_infinite) of the valid proofs.  Each gets its reject neighbours: the same proof with one USED input + 1
    (kept below r), with the inputs rotated by one where that changes S, and with C replaced by alpha"""
    out = []
    for xs, force in accepts:
        xs = list(xs)
        out.append(Member(xs, True, xs, force, False))
        if not neighbours:
            continue
        j = next((j for j, x in enumerate(xs) if s[j + 1] and x + 1 < r), None)
        if j is not None:
            out.append(Member(xs[:j] + [xs[j] + 1] + xs[j + 1:], False, xs, force, False))
        rot = xs[1:] + xs[:1]
        if _dot(s, rot, r) != _dot(s, xs, r):
            out.append(Member(rot, False, xs, force, False))
        out.append(Member(xs, False, xs, force, True))
    return out


def edge_values(cid):
    """0, 1, r - 1, 2^8 - 1, 2^8, a single top digit, r - 2, the largest all-0xFF-bytes value below r"""
    r, nwin = scalar_modulus(cid), num_windows(cid)
    ff = max(m for m in range(1, nwin + 1) if (1 << (8 * m)) - 1 < r)
    vals = [0, 1, r - 1, (1 << 8) - 1, 1 << 8, 1 << (8 * (nwin - 1)), r - 2, (1 << (8 * ff)) - 1]
    assert all(0 <= v < r for v in vals)
    return vals


def equal_digit_value(cid):
    """nwin equal non-zero byte digits, below r"""
    r, nwin = scalar_modulus(cid), num_windows(cid)
    x = int.from_bytes(b"\x01" * nwin, "little")
    assert x < r
    return x


def non_canonical(cid):
    """(name, value) of unreduced encodings that fit the scalar's words: r + 1 and 1 + 2^(8 nwin) are 1 to a verifier that reduces mod r
    or reads nwin digits only, r is 0, and the last one fills the top word"""
    r, nwin, L = scalar_modulus(cid), num_windows(cid), O.CURVES[cid].fr.n64
    out = [("r+1", r + 1), ("r", r)]
    if 8 * nwin < 64 * L:
        out.append(("1+2^(8 nwin)", 1 + (1 << (8 * nwin))))
    out.append(("top word ones", 1 | ((1 << 64) - 1) << (64 * (L - 1))))
    return out


EQUAL_BASES = 64  # the inputs of equal_lanes / opposite_lanes: one table addition per lane and window
TABLE_LIMIT = 256  # PVK_TABLE_INPUTS of pcd_amd/csrc/capi_internal.h: keys with more inputs have no window tables


def cases(cid):
    """the named cases: Case(name, s, members), members = Member(xs, expect_accept, ...)"""
    r, nwin = scalar_modulus(cid), num_windows(cid)
    out = []

    def rnd(name, n, lo=1):
        g = _rng("case", cid, name)
        return [g.randrange(lo, r) for _ in range(n)]

    s = rnd("no_inputs/s", 1)
    out.append(Case("no_inputs", s, _members(s, r, [([], False)])))
    s = rnd("zeros/s", 4)
    out.append(Case("zeros", s, _members(s, r, [([0, 0, 0], False)])))
    s = rnd("edges/s", 9)
    out.append(Case("edges", s, _members(s, r, [(edge_values(cid), False)])))
    ni = 1 + -(-130 // nwin)
    s = rnd("lanes_twice/s", ni)
    out.append(Case("lanes_twice", s, _members(s, r, [(rnd("lanes_twice/x", ni - 1, 0), False)])))
    s = [0] + rnd("abc0_infinite/s", 2)
    out.append(Case("abc0_infinite", s, _members(s, r, [(rnd("abc0_infinite/x", 2, 0), False)])))
    s = rnd("unused_input/s", 4)
    s[2] = 0
    xs = rnd("unused_input/x", 3)
    other = xs[:1] + [(xs[1] + 12345) % r] + xs[2:]
    out.append(Case("unused_input", s, _members(s, r, [(xs, False)], neighbours=False) + [Member(other, True, xs, False, False)]))
    s = rnd("acc_infinite/s", 4)
    xs = rnd("acc_infinite/x", 2)
    xs.append(-_dot(s[:3], xs, r) * pow(s[3], -1, r) % r)
    # (two entries, same key data: each proof brings its three reject neighbours, and one lane-per-pairing verification takes 0.3 s on a
    # 753-bit curve)
    out.append(Case("acc_infinite", s, _members(s, r, [(xs, False)])))
    out.append(Case("acc_infinite_c_infinite", s, _members(s, r, [(xs, True)])))
    s0, se = rnd("equal_lanes/s", 2)
    s = [s0] + [se] * EQUAL_BASES
    out.append(Case("equal_lanes", s, _members(s, r, [([equal_digit_value(cid)] * EQUAL_BASES, False)])))
    s0, se = rnd("opposite_lanes/s", 2)
    s = [s0] + [se] * (EQUAL_BASES // 2) + [r - se] * (EQUAL_BASES // 2)
    out.append(Case("opposite_lanes", s, _members(s, r, [([equal_digit_value(cid)] * EQUAL_BASES, False)])))
    if cid == 0:   # the two sides of the table limit on the same prefix of s and x (about 220 MB of tables: the smallest curve only)
        s = rnd("table_limit/s", TABLE_LIMIT + 1)
        xs = rnd("table_limit/x", TABLE_LIMIT, 0)
        for ni in (TABLE_LIMIT, TABLE_LIMIT + 1):
            out.append(Case(f"table_limit_{ni}", s[:ni], _members(s[:ni], r, [(xs[:ni - 1], False)])))
    return out


def case_named(cid, name):
    return next(c for c in cases(cid) if c.name == name)


_BUILT = {}


def build(co, cid, case):
    """the case as arrays: Built(key, pubs: per member (ni - 1, L) canonical limbs, proofs, proofs_inf: (n, 3), expect: bool (n,)).
    Made once per process and shared; callers leave it unchanged."""
    tag = (cid, case.name)
    if tag in _BUILT:
        return _BUILT[tag]
    key = trapdoor_key(co, cid, case.s, seed=case.name)
    made = {}
    w1 = co.point_words(cid, 1)
    pubs, proofs, infs = [], [], []
    for m in case.members:
        pt = (tuple(m.proof_xs), m.force_c_infinite)
        if pt not in made:
            made[pt] = trapdoor_proof(co, key, m.proof_xs, seed=(case.name, m.force_c_infinite), force_c_infinite=m.force_c_infinite)
        proof, inf = made[pt][0].copy(), made[pt][1].copy()
        if m.c_is_alpha:
            proof[len(proof) - w1:] = key.alpha_g1
            inf[2] = 0
            assert proof_scalars(key, m.proof_xs, (case.name, m.force_c_infinite), m.force_c_infinite)[2] != key.a
        pubs.append(scalar_words(cid, m.xs))
        proofs.append(proof)
        infs.append(inf)
    b = Built(key, pubs, np.stack(proofs), np.stack(infs), np.array([m.expect_accept for m in case.members]))
    for a in [b.proofs, b.proofs_inf, b.expect] + pubs:
        a.setflags(write=False)
    _BUILT[tag] = b
    return b
