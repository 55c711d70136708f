"""TEST INFRASTRUCTURE: prover and MSM inputs whose discrete logarithms are known, so that PARTIAL SUMS coincide on purpose.

Every group element is k G for a known k, and every expected value is arithmetic in Python integers mod the scalar modulus q plus one
fixed-base multiple (verify_reference._multiples) -- independent of the C++ oracle's MSM and proof assembly.  No GPU, no library.

Prover side.  A small satisfied R1CS on a radix-2 domain, toxic waste (alpha, beta, gamma, delta, tau), the key's exponents At_i, Bt_i,
Ct_i as oracle/pyoracle.py groth16_setup computes them, h as integers, and then, mod q:

  u0  = alpha + sum_i z_i At_i                 v0 = beta + sum_i z_i Bt_i
  K_l = sum_{i>=ni} z_i (beta At_i + alpha Bt_i + Ct_i) / delta          K_h = sum_{i<n-1} h_i tau^i (tau^n - 1) / delta
  S   = sum_{i<ni} z_i (beta At_i + alpha Bt_i + Ct_i)
  u = u0 + r delta      v = v0 + s delta      w = s u + r v - r s delta + K_l + K_h
  proof = (u G1, v G2, w G1), flag and zero coordinates where the logarithm is 0;   it verifies  <=>  u v = alpha beta + S + w delta

`prover_cases` solves r or s so that an operand of the assembly (pcd_amd/csrc/inst_g16.hip g16_finish: t1 = s A + r B_1, t2 = t1 + M_l',
C = t2 + M_h, with M_l' of logarithm K_l - r s delta) is the identity, or equals or is opposite to the other operand.

MSM side.  `msm_cases` builds bases k_i G with small or solved k_i under scalars whose c-bit windows all lie in [2, 2^(c-1) - 1] (the
signed digits are the windows themselves), so every bucket sum S_{w,d} = sum of the k_i with digit d in window w is a known integer."""
import collections

import numpy as np

from oracle import pyoracle as O
from verify_reference import _multiples, _rng, mont, scalar_words  # noqa: F401  (mont, scalar_words: re-exported for the tests)

# ------------------------------------------------------------------------------------------------------------------------ prover
Circuit = collections.namedtuple("Circuit", "name cid kind nc seed")
CONSTRAINTS = (200, 120, 60, 40)
CIRCUITS = [Circuit(f"synthetic{cid}", cid, "synthetic", CONSTRAINTS[cid], 7100 + cid) for cid in range(4)] + \
           [Circuit("skewed0", 0, "skewed", 150, 7110)]
# assignments of zeros and ones with at most an eighth general scalars (co.witness_r1cs: bit decompositions): what the prover's
# sparse-window copies are taken for (pcdhip_groth16_set_sparse_window)
WITNESS_CIRCUITS = {0: Circuit("witness0", 0, "witness", 200, 7131), 2: Circuit("witness2", 2, "witness", 100, 7130)}
CIRCUITS += list(WITNESS_CIRCUITS.values())
TINY = Circuit("tiny0", 0, "synthetic", 6, 7120)   # small enough for the pure-Python prover


def circuit_of(cid):
    return CIRCUITS[cid]


PCase = collections.namedtuple("PCase", "name r s u v w")
_STATEMENTS = {}


class Statement:
    """a circuit, its satisfying assignment and toxic waste as integers; the exponents of the key and of the proof's parts"""

    def __init__(self, co, circ):
        cid = circ.cid
        self.circuit, self.cid = circ, cid
        fld = O.CURVES[cid].fr
        self.fld, self.q = fld, fld.p
        q = self.q
        gen = {"synthetic": co.synthetic_r1cs, "skewed": co.skewed_r1cs, "witness": co.witness_r1cs}[circ.kind]
        r = gen(co.CURVE_FR[cid], circ.nc, 2, seed=circ.seed)
        self.r1cs = r

        def rows(rp, col, cf):
            cf = O.unpack_fp(fld, cf)
            rp = [int(x) for x in rp]
            return [[(cf[k], int(col[k])) for k in range(rp[j], rp[j + 1])] for j in range(len(rp) - 1)]
        A, B, C = rows(r.rp_a, r.col_a, r.coeff_a), rows(r.rp_b, r.col_b, r.coeff_b), rows(r.rp_c, r.col_c, r.coeff_c)
        z = O.unpack_fp(fld, r.z)
        py = O.R1CS(fld, r.num_inputs, A, B, C, z)
        assert z[0] == 1 and py.is_satisfied() and py.num_constraints == circ.nc
        self.general = sum(1 for v in z if v > 1)   # scalars that are neither 0 nor 1
        assert circ.kind != "witness" or 0 < self.general * 8 <= len(z)
        log_n = py.domain_log()
        assert log_n == r.domain_log and log_n <= fld.two_adicity, "radix-2 domains only"
        n = 1 << log_n
        self.py, self.z, self.n, self.log_n = py, z, n, log_n
        self.ni, self.m = r.num_inputs, r.num_vars
        h = O.witness_map_naive(py) if n <= 256 else O.unpack_fp(fld, co.witness_map(r))
        assert len(h) == n and h[n - 1] == 0
        self.h = h
        rng = _rng("dlog/toxic", circ.name)
        self.toxic = tuple(rng.randrange(1, q) for _ in range(5))
        alpha, beta, gamma, delta, tau = self.toxic
        L = O.lagrange_at(fld, log_n, tau)   # asserts tau^n != 1
        m, ni = self.m, self.ni
        At, Bt, Ct = [0] * m, [0] * m, [0] * m
        for j, (ra, rb, rc) in enumerate(zip(A, B, C)):
            for c, col in ra:
                At[col] = (At[col] + c * L[j]) % q
            for c, col in rb:
                Bt[col] = (Bt[col] + c * L[j]) % q
            for c, col in rc:
                Ct[col] = (Ct[col] + c * L[j]) % q
        for i in range(ni):
            At[i] = (At[i] + L[circ.nc + i]) % q
        zt = (pow(tau, n, q) - 1) % q
        assert zt and delta % q and gamma % q
        dinv, ginv = pow(delta, -1, q), pow(gamma, -1, q)
        mix = [(beta * At[i] + alpha * Bt[i] + Ct[i]) % q for i in range(m)]
        self.exponents = dict(
            alpha_g1=alpha, beta_g1=beta, delta_g1=delta, beta_g2=beta, delta_g2=delta, gamma_g2=gamma,
            a_query=At, b_g1_query=Bt, b_g2_query=Bt,
            h_query=[pow(tau, i, q) * zt % q * dinv % q for i in range(n - 1)],
            l_query=[mix[i] * dinv % q for i in range(ni, m)],
            gamma_abc_g1=[mix[i] * ginv % q for i in range(ni)])
        self.u0 = (alpha + sum(zi * a for zi, a in zip(z, At))) % q
        self.v0 = (beta + sum(zi * b for zi, b in zip(z, Bt))) % q
        self.K_l = sum(z[i] * mix[i] for i in range(ni, m)) % q * dinv % q
        self.K_h = sum(hi * e for hi, e in zip(h, self.exponents["h_query"])) % q
        self.S = sum(z[i] * mix[i] for i in range(ni)) % q
        self.alpha, self.beta, self.delta = alpha, beta, delta

    def toxic_mont(self):
        return O.pack_fp(self.fld, list(self.toxic))

    def uvw(self, r, s):
        q, d = self.q, self.delta
        u = (self.u0 + r * d) % q
        v = (self.v0 + s * d) % q
        w = (s * u + r * v - r * s * d + self.K_l + self.K_h) % q
        return u, v, w

    def verifies(self, u, v, w):
        """the verification equation in the exponent"""
        return (u * v - self.alpha * self.beta - self.S - w * self.delta) % self.q == 0


def statement(co, circ):
    """made once per process and shared; callers leave it unchanged"""
    if circ.name not in _STATEMENTS:
        _STATEMENTS[circ.name] = Statement(co, circ)
    return _STATEMENTS[circ.name]


def nibble_values(q):
    """15, 16, 2^(4j) for a low, a middle and the top 4-bit window, the largest value below q whose hex digits are all F"""
    top = (q.bit_length() - 1) // 4
    ff = max(m for m in range(1, top + 2) if 16 ** m - 1 < q)
    vals = [15, 16, 1 << 8, 1 << (4 * (top // 2)), 1 << (4 * top), 16 ** ff - 1]
    assert all(0 < v < q for v in vals) and (1 << (4 * (top + 1))) >= q
    return vals


def prover_cases(cid, circuit=None):
    """THE case list of a curve's circuit (default: CIRCUITS[cid]): PCase(name, r, s, u, v, w).  Every case asserts the property that
    defines it, in integers, and that what it divides by is not zero."""
    from oracle import coracle as co
    st = statement(co, circuit or circuit_of(cid))
    assert st.cid == cid
    q, d, u0, v0, K_l, K_h = st.q, st.delta, st.u0, st.v0, st.K_l, st.K_h
    rng = _rng("dlog/cases", st.circuit.name)
    out = []

    def inv(x):
        assert x % q != 0, "a case divides by zero: take another seed"
        return pow(x % q, -1, q)

    def add(name, r, s, prop):
        r, s = r % q, s % q
        u, v, w = st.uvw(r, s)
        # the operands of g16_finish: t1 = s A + r B_1, then + M_l', then + M_h
        sA, rB, l, hh = s * u % q, r * v % q, (K_l - r * s * d) % q, K_h
        t1 = (sA + rB) % q
        t2 = (t1 + l) % q
        assert (t2 + hh) % q == w
        assert prop(dict(r=r, s=s, u=u, v=v, w=w, sA=sA, rB=rB, l=l, h=hh, t1=t1, t2=t2)), name
        out.append(PCase(name, r, s, u, v, w))

    rr = lambda: rng.randrange(2, q)
    add("random", rr(), rr(), lambda e: e["u"] and e["v"] and e["w"] and e["sA"] not in (e["rB"], q - e["rB"]))
    add("no_zk", 0, 0, lambda e: e["u"] == u0 and e["v"] == v0 and e["w"] == (K_l + K_h) % q and e["t1"] == 0)
    add("r0", 0, rr(), lambda e: e["r"] == 0 and e["rB"] == 0 and e["sA"] != 0)
    add("s0", rr(), 0, lambda e: e["s"] == 0 and e["sA"] == 0 and e["rB"] != 0)
    add("ones", 1, 1, lambda e: e["sA"] == e["u"] and e["rB"] == e["v"])
    add("top", q - 1, q - 1, lambda e: e["sA"] == q - e["u"] and e["rB"] == q - e["v"])
    nib = nibble_values(q)
    for i, x in enumerate(nib):
        add(f"nibbles{i}", x, nib[(i + 1) % len(nib)], lambda e: e["u"] and e["v"])
    add("A_inf", -u0 * inv(d), rr(), lambda e: e["u"] == 0 and e["r"] != 0 and e["v"] != 0)
    add("B_inf", rr(), -v0 * inv(d), lambda e: e["v"] == 0 and e["s"] != 0 and e["u"] != 0)
    add("AB_inf", -u0 * inv(d), -v0 * inv(d), lambda e: e["u"] == 0 and e["v"] == 0 and e["w"] == (K_l + K_h - e["r"] * e["s"] * d) % q)
    r = rr()
    add("C_inf", r, -(K_l + K_h + r * v0) * inv(u0 + r * d), lambda e: e["w"] == 0 and e["u"] and e["v"])
    r = rr()
    add("sA_eq_rB1", r, r * v0 * inv(u0), lambda e: e["sA"] == e["rB"] != 0)
    r = rr()
    add("sA_opp_rB1", r, -r * v0 * inv(u0 + 2 * r * d), lambda e: e["t1"] == 0 and e["sA"] != 0)
    r = rr()
    add("t1_eq_l", r, (K_l - r * v0) * inv(u0 + 3 * r * d), lambda e: e["t1"] == e["l"] != 0)
    r = rr()
    add("t1_opp_l", r, -(K_l + r * v0) * inv(u0 + r * d), lambda e: e["t2"] == 0 and e["t1"] != 0)
    r = rr()
    add("t2_eq_h", r, (K_h - K_l - r * v0) * inv(u0 + r * d), lambda e: e["t2"] == e["h"] != 0)
    r = rr()
    add("l_inf", r, K_l * inv(r * d), lambda e: e["l"] == 0 and K_l != 0 and e["t1"] != 0)
    assert all(st.verifies(c.u, c.v, c.w) for c in out)
    assert len({c.name for c in out}) == len(out)
    return out


_PROOFS = {}


def reference_proofs(co, circ):
    """{case name: (proof = A || B || C affine C-ABI image, flags[3])} of prover_cases, from two fixed-base batches; shared, read-only"""
    if circ.name not in _PROOFS:
        cs = prover_cases(circ.cid, circ)
        k = len(cs)
        g1, i1 = _multiples(co, circ.cid, 1, [c.u for c in cs] + [c.w for c in cs])
        g2, i2 = _multiples(co, circ.cid, 2, [c.v for c in cs])
        made = {}
        for j, c in enumerate(cs):
            proof = np.concatenate([g1[j], g2[j], g1[k + j]])
            inf = np.array([i1[j], i2[j], i1[k + j]], dtype=np.uint8)
            proof.setflags(write=False)
            inf.setflags(write=False)
            made[c.name] = (proof, inf)
        _PROOFS[circ.name] = made
    return _PROOFS[circ.name]


# --------------------------------------------------------------------------------------------------------------------------- MSM
MsmInput = collections.namedtuple("MsmInput", "name ks scalars")   # ks: the bases' logarithms (any integers); scalars: ints in [0, q)
SmallDlog = collections.namedtuple("SmallDlog", "input seed counts")
BIG_LIMIT, SEG_LEN = 8, 128   # msm_run's big_limit and seg_len (pcd_amd/csrc/msm.hip.h): a run over more than 8 chunks is a big bucket,
#                               cut into segments of 128 chunk pieces
RUN_CHUNK = 33                # the forced chunk the run lengths below are derived for
# A run of N sorted entries lies in at least ceil(N / chunk) chunks wherever it starts.  N = 8 * 33 + 1 = 265 is the shortest run that is a
# big bucket at chunk 33 for every alignment (>= 9 pieces); N = 128 * 33 + 1 = 4225 the shortest with more than 128 pieces, i.e. with a
# second segment in msm_big_segments_kernel (at chunk 128: >= 34 pieces, a big bucket of one segment).
RUN_N_BIG = BIG_LIMIT * RUN_CHUNK + 1
RUN_N_TWO_SEGMENTS = SEG_LEN * RUN_CHUNK + 1
assert -(-RUN_N_BIG // RUN_CHUNK) > BIG_LIMIT and -(-RUN_N_TWO_SEGMENTS // RUN_CHUNK) > SEG_LEN and -(-RUN_N_TWO_SEGMENTS // 128) > BIG_LIMIT


def scalar_modulus(cid):
    return O.CURVES[cid].fr.p


def dlog_bases(co, cid, grp, ks):
    """k_i G -> (affine points, flags); k = 0 mod q is a flagged identity with zero coordinates"""
    q = scalar_modulus(cid)
    red = [k % q for k in ks]
    uniq = sorted(set(red))
    xy, inf = _multiples(co, cid, grp, uniq)
    at = {k: i for i, k in enumerate(uniq)}
    idx = np.array([at[k] for k in red], dtype=np.int64)
    return np.ascontiguousarray(xy[idx]), np.ascontiguousarray(inf[idx])


def expected_msm(co, cid, grp, ks, scalars):
    """(sum_i s_i k_i mod q) G -> (affine point, flag)"""
    q = scalar_modulus(cid)
    assert len(ks) == len(scalars)
    xy, inf = _multiples(co, cid, grp, [sum(s * k for s, k in zip(scalars, ks)) % q])
    return xy[0], inf[0]


def num_windows(cid, c):
    w = (scalar_modulus(cid).bit_length() - 2) // c   # a value of w windows is < 2^(bits - 2) < q
    assert w >= 2
    return w


def digits_of(value, c):
    out = []
    while value:
        out.append(value & ((1 << c) - 1))
        value >>= c
    return out


def _from_digits(ds, c):
    return sum(d << (c * w) for w, d in enumerate(ds))


def paired_values(cid, c, pairs=20):
    """2 * pairs scalar values of num_windows(cid, c) windows each: in every window, value 2a has digit 2j + 1 and value 2a + 1 digit
    2j + 2 for a random j -- the two buckets are one item of msm_tail_pair_item.  Digits lie in [3, 2^(c-1) - 1]."""
    rng = _rng("dlog/values", cid, c)
    W, jmax = num_windows(cid, c), ((1 << (c - 1)) - 3) // 2
    assert jmax >= 1
    vals = []
    for _ in range(pairs):
        js = [rng.randrange(1, jmax + 1) for _ in range(W)]
        vals.append(_from_digits([2 * j + 1 for j in js], c))
        vals.append(_from_digits([2 * j + 2 for j in js], c))
    assert len(set(vals)) == 2 * pairs
    assert all(2 <= d <= (1 << (c - 1)) - 1 for v in vals for d in digits_of(v, c))
    return vals


def bucket_sums(ks, scalars, c):
    """{(window, digit): (entries, sum of their k)} over the scalars that are neither 0 nor 1, digit != 0"""
    by_value = {}
    for k, s in zip(ks, scalars):
        if s > 1:
            cnt, tot = by_value.get(s, (0, 0))
            by_value[s] = (cnt + 1, tot + k)
    out = {}
    for s, (cnt, tot) in by_value.items():
        for w, d in enumerate(digits_of(s, c)):
            if d:
                a, b = out.get((w, d), (0, 0))
                out[(w, d)] = (a + cnt, b + tot)
    return out


def coincidence_counts(ks, scalars, c):
    """the four conditions of the small-dlog family on the integers: non-empty buckets with S = 0, and aligned adjacent bucket pairs
    (digits 2j + 1, 2j + 2 of one window, both non-empty, S != 0) with equal sums, opposite sums, S_{2j+1} = 2 S_{2j+2}"""
    S = bucket_sums(ks, scalars, c)
    zero = sum(1 for cnt, tot in S.values() if cnt and tot == 0)
    eq = opp = dbl = 0
    for (w, d), (cnt, tot) in S.items():
        if d % 2 == 1 and (w, d + 1) in S and tot != 0:
            t2 = S[(w, d + 1)][1]
            eq += tot == t2
            opp += tot == -t2
            dbl += tot == 2 * t2
    return dict(zero=zero, equal=eq, opposite=opp, double=dbl)


_SMALL = {}


def small_dlog(cid, c, n, need=5, max_seeds=20000):
    """Family 1: n bases k_i G with k_i uniform in {-4 .. 4} \\ {0} under scalars over the 40 paired_values (value 0 about a third of the
    vector: runs that cross many chunk edges), 100 ones and 100 zeros.  All partial sums are small multiples of G, so equal, opposite and
    cancelling operands recur at every stage of the MSM.  The seed of the k_i is the first for which the input holds at least `need`
    non-empty buckets with S = 0 and at least `need` aligned adjacent bucket pairs each with equal sums, opposite sums and S_{2j+1} =
    2 S_{2j+2} (coincidence_counts: a condition on the input, checked here on the integers).  The counts are per bucket WINDOW, which is
    what an MSM without resident copies sums; with window-shifted copies the device's bucket d holds sum_w 2^(c w) S_{w,d}, where whole
    rows coincide less often.  Coincidences at the deeper levels of the reduction and inside the accumulation are frequent by
    construction but not counted.  -> SmallDlog(input, seed, counts)"""
    tag = (cid, c, n)
    if tag in _SMALL:
        return _SMALL[tag]
    assert n >= 240
    q = scalar_modulus(cid)
    vals = paired_values(cid, c)
    g0 = np.random.Generator(np.random.PCG64([11, cid, c, n]))
    weights = np.ones(40)
    weights[0] = 20.0
    pick = g0.choice(40, size=n, p=weights / weights.sum())
    where = g0.permutation(n)
    ones, zeros = where[:100], where[100:200]
    general = np.ones(n, dtype=bool)
    general[where[:200]] = False
    scalars = [vals[int(k)] for k in pick]
    for i in ones:
        scalars[int(i)] = 1
    for i in zeros:
        scalars[int(i)] = 0
    assert all(0 <= s < q for s in scalars)
    pg = pick[general]
    for seed in range(max_seeds):
        g = np.random.Generator(np.random.PCG64([12, cid, c, n, seed]))
        ks = g.integers(1, 5, size=n) * (2 * g.integers(0, 2, size=n) - 1)
        K = np.bincount(pg, weights=ks[general], minlength=40).astype(np.int64)
        a, b = K[0::2], K[1::2]
        live = (a != 0) & (b != 0)
        if not ((K == 0).any() and (live & (a == b)).any() and (live & (a == -b)).any() and (live & (a == 2 * b)).any()):
            continue   # (no pair of values can give the pairs of buckets: skip the exact count)
        ksl = [int(k) for k in ks]
        counts = coincidence_counts(ksl, scalars, c)
        if min(counts.values()) >= need:
            _SMALL[tag] = SmallDlog(MsmInput(f"small_dlog_{n}", ksl, scalars), seed, counts)
            return _SMALL[tag]
    raise AssertionError(f"no seed below {max_seeds} gives the small-dlog conditions for {tag}")


def _background(cid, c, n, tag):
    """n entries over the paired values with small k: something for the other buckets to hold"""
    rng = _rng("dlog/background", cid, c, tag)
    vals = paired_values(cid, c)
    ks = [rng.choice((-4, -3, -2, -1, 1, 2, 3, 4)) for _ in range(n)]
    return ks, [rng.choice(vals) for _ in range(n)]


def total_cancels(cid, c):
    """Family 2: small_dlog(600) with the last scalar solved so that sum s_i k_i = 0 mod q: the result is the identity although the
    scalars are not zero"""
    q = scalar_modulus(cid)
    base = small_dlog(cid, c, 600).input
    ks, sc = list(base.ks), list(base.scalars)
    rest = sum(s * k for s, k in zip(sc[:-1], ks[:-1])) % q
    assert ks[-1] % q and rest
    sc[-1] = -rest * pow(ks[-1], -1, q) % q
    assert sum(s * k for s, k in zip(sc, ks)) % q == 0 and sc[-1] > 1
    return MsmInput("total_cancels", ks, sc)


def giant_equal_run(cid, c, N, variant):
    """Family 3: one bucket (per window) of N entries with one scalar between 300 background entries.  equal: N copies of 3 G (every full
    chunk's partial is the same point: the tree nodes double); alternating: 3 G, -3 G, .. (partials O or +-3 G); halves_cancel: N / 2
    copies of 3 G, then N / 2 of -3 G (equal partials, then their opposites; the bucket is O while non-empty)"""
    rng = _rng("dlog/run_value", cid, c)
    lim = 1 << (c - 1)
    value = _from_digits([rng.randrange(2, lim) for _ in range(num_windows(cid, c))], c)
    assert value not in paired_values(cid, c)
    if variant == "equal":
        run = [3] * N
    elif variant == "alternating":
        run = [3 if i % 2 == 0 else -3 for i in range(N)]
    else:
        assert variant == "halves_cancel" and N % 2 == 0
        run = [3] * (N // 2) + [-3] * (N // 2)
    want = {"equal": 3 * N, "alternating": 3 * (N % 2), "halves_cancel": 0}[variant]
    assert sum(run) == want
    bk, bs = _background(cid, c, 300, "run")
    return MsmInput(f"giant_{variant}_{N}", bk[:150] + run + bk[150:], bs[:150] + [value] * N + bs[150:])


GIANT_VARIANTS = [("equal", RUN_N_BIG), ("equal", RUN_N_TWO_SEGMENTS), ("alternating", RUN_N_BIG), ("alternating", RUN_N_BIG + 1),
                  ("halves_cancel", RUN_N_BIG + 1), ("halves_cancel", RUN_N_TWO_SEGMENTS + 1)]


def ones_meet_bucket1(cid, c, variant):
    """Family 4: the pseudo bucket of the scalars equal to one and bucket (window 0, digit 1), which msm_merge_ones_kernel adds: equal
    sums, opposite sums, and each O while non-empty.  The bucket-1 entries have the scalar 1 + 2 * 2^c (digits 1, 2)."""
    one_ks, b1_ks = {"equal": ([1, 2], [3]), "opposite": ([1, 2], [-3]), "ones_inf": ([1, 1, -2], [5]), "bucket1_inf": ([5], [1, 1, -2]),
                     "both_inf": ([2, -1, -1], [1, 1, -2])}[variant]
    bk, bs = _background(cid, c, 300, "ones")
    ks = bk[:100] + one_ks + bk[100:200] + b1_ks + bk[200:]
    sc = bs[:100] + [1] * len(one_ks) + bs[100:200] + [1 + (2 << c)] * len(b1_ks) + bs[200:]
    S = bucket_sums(ks, sc, c)
    assert S[(0, 1)] == (len(b1_ks), sum(b1_ks))   # nothing else has digit 1 in window 0
    so, sb = sum(one_ks), sum(b1_ks)
    assert {"equal": so == sb != 0, "opposite": so == -sb != 0, "ones_inf": so == 0 != sb, "bucket1_inf": sb == 0 != so,
            "both_inf": so == 0 == sb}[variant]
    return MsmInput(f"ones_{variant}", ks, sc)


ONES_VARIANTS = ["equal", "opposite", "ones_inf", "bucket1_inf", "both_inf"]


def horner(cid, c, variant):
    """Family 5 (for MSMs without resident copies, where msm_horner_kernel combines the windows): every scalar has two windows, and one
    base is solved so that the window sums V_w = sum_d d S_{w,d} satisfy V_0 = 2^c V_1 (the last addition doubles), V_0 = -2^c V_1 (it
    gives O), or V_1 = O while window 1 is not empty"""
    q = scalar_modulus(cid)
    rng = _rng("dlog/horner", cid, c, variant)
    lim = 1 << (c - 1)
    ks = [rng.choice((-4, -3, -2, -1, 1, 2, 3, 4)) for _ in range(300)]
    sc = [_from_digits([rng.randrange(2, lim), rng.randrange(2, lim)], c) for _ in range(300)]

    def V(w):
        return sum(k * ((s >> (c * w)) & ((1 << c) - 1)) for k, s in zip(ks, sc)) % q
    half = pow(2, -1, q)
    if variant == "v1_inf":
        ks.append(-V(1) * half % q)
        sc.append(2 << c)           # digits (0, 2)
        assert V(1) == 0 and V(0) != 0
    else:
        sign = {"equal": 1, "opposite": -1}[variant]
        assert V(1) != 0
        ks.append((sign * (V(1) << c) - V(0)) * half % q)
        sc.append(2)                # digits (2, 0)
        assert V(0) == sign * (V(1) << c) % q and V(0) != 0
    return MsmInput(f"horner_{variant}", ks, sc)


HORNER_VARIANTS = ["equal", "opposite", "v1_inf"]


def msm_cases(cid, grp, c):
    """every MSM input family for the forced window c -> list of MsmInput (grp does not enter: the inputs are logarithms)"""
    out = [small_dlog(cid, c, 600).input, small_dlog(cid, c, 5000).input, total_cancels(cid, c)]
    out += [giant_equal_run(cid, c, N, v) for v, N in GIANT_VARIANTS]
    out += [ones_meet_bucket1(cid, c, v) for v in ONES_VARIANTS]
    out += [horner(cid, c, v) for v in HORNER_VARIANTS]
    q = scalar_modulus(cid)
    assert all(len(i.ks) == len(i.scalars) and all(0 <= s < q for s in i.scalars) for i in out)
    return out


def jacobian(co, cid, grp, xy, inf):
    """affine points + flags -> Jacobian C-ABI images X || Y || Z with Z = 1, or all zero for a flagged point"""
    fq = co.CURVE_FQ[cid]
    L = co.FIELD_N64[fq]
    deg = 1 if grp == 1 else co.CURVE_G2_DEG[cid]
    assert L == co.FIELD_N64[co.CURVE_FR[cid]]   # (base and scalar field of a curve have the same limb count: scalar_words serves both)
    one = co.fp_op(fq, "from_canonical", scalar_words(cid, [1]))[0]
    n = xy.shape[0]
    out = np.zeros((n, 3 * deg * L), dtype=np.uint64)
    out[:, :2 * deg * L] = xy
    out[:, 2 * deg * L:2 * deg * L + L] = one
    out[np.asarray(inf) != 0] = 0
    return out

