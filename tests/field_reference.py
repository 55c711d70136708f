"""TEST INFRASTRUCTURE ONLY: exact-integer references and the seeded case lists for the device field arithmetic (pcd_amd/csrc/fp.hip.h)
and the lazily reduced addition steps (ec.hip.h), shared by tests/test_field_ops_host.py (host build of the templates, 128-bit column
check on) and tests/test_gpu_field_ops.py (gfx950 build); and for the lane-split towers and the group law in them, which exist in the
gfx950 build only (tests/test_gpu_lanesplit_ops.py; the lists themselves are checked by tests/test_lanesplit_reference_host.py).  Plain
Python integers throughout: no numpy arithmetic, and nothing here is another build of the code under test.

The raw device image of a field element is N 28-bit limbs in 32-bit words (N = 11 for the 298-bit fields, 27 for the 753-bit ones);
limbs 0 .. N-2 are below 2^28 and the top limb takes the rest of the value.  A residue x is held as x R' mod p (+ p), R' = 2^(28 N).
An `Lz` image has SIGNED limbs and need not be carried."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyoracle as O  # noqa: E402

B = 1 << 28
MASK = B - 1

# operation numbers of tests/gpucheck/fieldops_ops.h
(F_MUL, F_SQR, F_ADD, F_SUB, F_NEG, F_DBL, F_MUL_SMALL, F_MUL_SMALL_VAR, F_INV_GCD, F_INV_FERMAT, F_MUL_INV, F_CANONICAL, F_IS_ZERO, F_EQ,
 F_TO_ABI, F_ABI_ROUNDTRIP, F_TO_WORDS, F_WORDS_ROUNDTRIP, F_SIGNED_SUM) = range(19)
L_MUL, L_DOT2, L_DOT4, L_SQR, L_SCALE_CARRY, L_CARRY, L_SUB0, L_SUB2, L_SHL = range(9)
T_MUL, T_SQR, T_INV = range(3)
S_MADD_LZ, S_MADD_X, S_MADD_X_PLAIN, S_MADD_JAC = range(4)


class Fld:
    def __init__(self, fid):
        f = O.FIELDS[fid]
        self.fid, self.p, self.N = fid, f.p, (11 if fid < 2 else 27)
        self.R = 1 << (28 * self.N)                 # the device's Montgomery radix R'
        self.Rinv = pow(self.R, -1, self.p)
        self.n32 = 2 * f.n64
        self.R_abi = 1 << (32 * self.n32)           # the C-ABI's (upstream) Montgomery radix
        self.top_w = B ** (self.N - 1)              # weight of the top limb

    def mont(self, x):
        return x * self.R % self.p

    def unmont(self, a):
        return a * self.Rinv % self.p


FLD = [Fld(i) for i in range(4)]


# ----------------------------------------------------------------------------- limb images
def limbs(x, N):
    """carried form: limbs 0 .. N-2 in [0, 2^28), the top limb takes the rest (it may be negative or wider than 28 bits)"""
    return [(x >> (28 * i)) & MASK for i in range(N - 1)] + [x >> (28 * (N - 1))]


def unlimbs(ws):
    return sum(int(w) << (28 * i) for i, w in enumerate(ws))


def signed(ws):
    """uint32 words read back as the int32 limbs of an Lz image"""
    return [int(w) - (1 << 32) if int(w) >= (1 << 31) else int(w) for w in ws]


def is_normal(ws):
    return all(0 <= int(w) < B for w in ws[:-1]) and int(ws[-1]) >= 0


def check_reduced(fld, ws, want_residue, what):
    """the contract of every reducing operation: limbs 0 .. N-2 below 2^28, value in [0, 2p), and the right residue"""
    assert is_normal(ws), ("limb not normalised", what)
    r = unlimbs(ws)
    assert 0 <= r < 2 * fld.p, ("result not in [0, 2p)", what, r)
    assert (r - want_residue) % fld.p == 0, ("wrong residue", what, r)
    return r


# ----------------------------------------------------------------------------- operand classes in [0, 2p)
def operand_classes(fid, seed=1, n_random=200):
    """[(label, value)], values in [0, 2p): the representatives and limb patterns the arithmetic could trip on"""
    fld = FLD[fid]
    p, N, R = fld.p, fld.N, fld.R
    rnd = random.Random(1000 * seed + fid)
    out = []

    def add(label, v):
        if 0 <= v < 2 * p and all(v != w for _, w in out):
            out.append((label, v))
    for label, v in (("0", 0), ("1", 1), ("2", 2), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("2p-2", 2 * p - 2), ("2p-1", 2 * p - 1),
                     ("(p-1)/2", (p - 1) // 2), ("(p+1)/2", (p + 1) // 2), ("R", R % p), ("R+p", R % p + p), ("R^2", R * R % p),
                     ("R^2+p", R * R % p + p)):
        add(label, v)
    for j in range(0, N + 1):
        for d in (-1, 0, 1):
            if 28 * j + d >= 0:
                add(f"2^{28 * j + d}", 1 << (28 * j + d))
    add("low limbs all ones", ((2 * p - fld.top_w) // fld.top_w) * fld.top_w + fld.top_w - 1)
    top_max = (2 * p - 1) >> (28 * (N - 1))
    for i in range(N):
        add(f"limb {i} all ones", (MASK if i < N - 1 else min(MASK, top_max)) << (28 * i))
    for ph in (0, 1):
        v = sum(MASK << (28 * i) for i in range(N - 1) if i % 2 == ph)
        t = top_max if (N - 1) % 2 == ph else 0
        while t * fld.top_w + v >= 2 * p:
            t -= 1
        add(f"alternating phase {ph}", t * fld.top_w + v)
    n_special = len(out)
    for k in range(n_random):
        out.append((f"random {k}", rnd.randrange(2 * p)))
    return out, n_special


CORE = ("0", "1", "p-1", "p", "p+1", "2p-2", "2p-1", "(p+1)/2", "R", "R^2+p", "low limbs all ones", "alternating phase 0",
        "alternating phase 1", "2^27", "2^28", "2^57")


def unary_cases(fid, seed=1):
    return [v for _, v in operand_classes(fid, seed)[0]]


def binary_cases(fid, seed=2):
    """every special value against itself and against the CORE ones in both orders, random against random and against the CORE ones"""
    cls, ns = operand_classes(fid, seed)
    core = [v for lbl, v in cls[:ns] if lbl in CORE]
    rnd = random.Random(77 * seed + fid)
    pairs = []
    for _, v in cls[:ns]:
        pairs.append((v, v))
        for c in core:
            pairs.append((v, c)); pairs.append((c, v))
    rand = [v for _, v in cls[ns:]]
    for v in rand:
        pairs.append((v, rnd.choice(rand)))
        pairs.append((v, rnd.choice(core)))
    return pairs


def addsub_band_pairs(fid, seed=None):
    """operand pairs aimed at the band the two-top-limb estimate of Fp::operator+ / operator- cannot decide (sums around 2p, differences
    around 0, differences whose two top limbs cancel) next to random ones; any representative in [0, 2p)"""
    fld = FLD[fid]
    p, N = fld.p, fld.N
    rnd = random.Random(77 + fid if seed is None else seed)
    lo = B ** (N - 2)                      # weight of the second limb from the top
    pairs = []

    def both(a, b):
        if 0 <= a < 2 * p and 0 <= b < 2 * p:
            pairs.append((a, b))
    for _ in range(2000):
        both(rnd.randrange(2 * p), rnd.randrange(2 * p))
    for a in [0, 1, p - 1, p, p + 1, 2 * p - 1] + [rnd.randrange(2 * p) for _ in range(40)]:
        for d in (-2 * lo, -lo - 1, -lo, -lo + 1, -3, -2, -1, 0, 1, 2, 3, lo - 1, lo, lo + 1, 2 * lo):
            both(a, 2 * p - a + d)         # sums around 2p: the band the estimate leaves open
            both(a, a + d)                 # differences around 0
            both(a + d, a)
        both(a, a); both(a, 0); both(0, a); both(a, 2 * p - 1); both(2 * p - 1, a)
    for _ in range(300):                   # differences whose two top limbs cancel
        a = rnd.randrange(2 * p)
        both(a, a - (a % lo) + rnd.randrange(lo))
        both(a, (2 * p - a) - ((2 * p - a) % lo) + rnd.randrange(lo))
    return pairs


def add_exact(fld, a, b):
    return a + b - 2 * fld.p if a + b >= 2 * fld.p else a + b


def sub_exact(fld, a, b):
    return a - b + 2 * fld.p if a < b else a - b


def small_constants(fid):
    """every k the product passes to mul_small / mul_small_var on this field (curve coefficient a, non-residue nr, a nr, 2 nr, and the
    1 / 2 of the lane-split forms), the shortcuts 0 .. 4, and the top of the documented range k < 2^8"""
    ks = {0, 1, 2, 3, 4, 17, 121, 255}
    for c in O.CURVES:
        if c.fq is O.FIELDS[fid]:
            ks |= {c.a, c.nr, c.a * c.nr, 2 * c.nr}
    return sorted(ks)


def signed_sum_cases(fid, seed=40):
    """[(terms, coefficients)]: the term shapes of test_signed_sum_reduction on raw operands in [0, 2p), sum |c| <= 2000"""
    fld = FLD[fid]
    p = fld.p
    rnd = random.Random(seed + fid)
    cases = {}
    for T in (1, 2, 8, 16):
        lst = []
        w = 2000 // T
        for mode in ("pos", "neg", "alt", "rand"):
            for vals in ("max", "p", "p-1", "rand", "small"):
                a = [{"max": 2 * p - 1, "p": p, "p-1": p - 1}.get(vals, None) for _ in range(T)]
                a = [rnd.randrange(2 * p) if vals == "rand" else rnd.randrange(3) if vals == "small" else x for x in a]
                c = [w if mode == "pos" else -w if mode == "neg" else (w if i % 2 else -w) if mode == "alt" else rnd.randrange(-w, w + 1)
                     for i in range(T)]
                lst.append((a, c))
        cases[T] = lst
    return cases


# ----------------------------------------------------------------------------- Lz operands, taken from the call sites
def lz_sub_limbs(fld, a, b, S):
    """the uncarried difference the call sites form: a - b + (4 << S) p, limb-wise"""
    m4 = limbs(4 * fld.p, fld.N)
    return [x - y + (m << S) for x, y, m in zip(a, b, m4)]


def _all_ones_below(fld, bound):
    """the largest value below `bound` whose limbs 0 .. N-2 are all 0xFFFFFFF"""
    return ((bound - fld.top_w) // fld.top_w) * fld.top_w + fld.top_w - 1


def _top_only_above(fld, lo):
    """the smallest multiple of the top limb's weight above `lo` (limbs 0 .. N-2 zero)"""
    return (lo // fld.top_w + 1) * fld.top_w


def lz_roles(fid, nr=17):
    """{role: [limb lists]}: for every operand role the comments of ec.hip.h name (madd_lz: 'P < 18p carried' ... ; madd_x_lz2: 'P = U2 - X1
    + 4 in (2, 6)' ...), the largest and the smallest value of its interval and the most extreme limbs, in the limb form the call site produces"""
    fld = FLD[fid]
    p, N = fld.p, fld.N
    L = lambda x: limbs(x, N)
    ones2 = _all_ones_below(fld, 2 * p)
    roles = {}
    # normalised operands in [0, 2p): affine coordinates, ZZ, ZZZ, PP, PPP, Q, U2, S2 ...
    roles["normal"] = [L(v) for v in (0, 1, p - 1, p, 2 * p - 1, ones2, fld.top_w * ((2 * p - 1) // fld.top_w))]
    # madd_lz: the accumulator's X, carried, value < 16p
    roles["X<16p"] = [L(v) for v in (0, 1, 16 * p - 1, _all_ones_below(fld, 16 * p), 15 * p)]
    # madd_lz: P = lz_carry(lz_sub<2>(U2, X1)) = U2 - X1 + 16p in (0, 18p)
    roles["P<18p"] = [L(v) for v in (1, 16 * p, 18 * p - 1, _all_ones_below(fld, 18 * p), 2 * p - 1 + 16 * p - _top_only_above(fld, 0))]
    # madd_lz R, madd_x_lz2 P0 P1 R0 R1 t0 t1: lz_carry(lz_sub<0>(a, b)) = a - b + 4p in (2p, 6p)
    roles["(2p,6p)"] = [L(v) for v in (2 * p + 1, 4 * p, 6 * p - 1, _all_ones_below(fld, 6 * p), _top_only_above(fld, 2 * p))]
    # madd_lz: X3 = lz_carry(RR - PPP - 2Q + 8p) in (2p, 10p): the b of t below
    x3 = [2 * p + 1, 10 * p - 1, _all_ones_below(fld, 10 * p), _top_only_above(fld, 2 * p)]
    # madd_lz: t = lz_sub<2>(Q, X3) = Q - X3 + 16p in (6p, 18p), NOT carried: limbs in (-2^28, 1.25 2^30)
    roles["t uncarried"] = [lz_sub_limbs(fld, L(a), L(b), 2) for a, b in
                            ((2 * p - 1, 1),                                         # the largest value the stated interval allows (18p)
                             (2 * p - 1, 2 * p + 1),                                 # the largest one madd_lz reaches: X3 > 2p, so t < 16p
                             (0, 10 * p - 1),                                       # the smallest value
                             (0, _all_ones_below(fld, 10 * p)),                     # a limbs 0, b limbs all ones: the most negative limbs
                             (ones2, _top_only_above(fld, 2 * p)),                  # the reverse: the largest limbs
                             (ones2, _all_ones_below(fld, 10 * p)))]
    # Y1' = lz_sub<0>(0, Y1) = 4p - Y1 in (2p, 4p], NOT carried
    roles["4p-Y uncarried"] = [lz_sub_limbs(fld, L(0), L(b), 0) for b in (0, 1, 2 * p - 1, ones2, p)]
    # madd_x_lz2: lz_scale_carry(x, nr) of a normal x < 2p and of a carried P1 / R1 < 6p
    roles["nr*normal"] = [L(nr * v) for v in (0, 1, 2 * p - 1, ones2)]
    roles["nr*(2p,6p)"] = [L(nr * v) for v in (2 * p + 1, 6 * p - 1, _all_ones_below(fld, 6 * p))]
    # madd_x_lz2: lz_shl(P0, 1), limbs doubled without a carry
    roles["2*(2p,6p)"] = [[2 * w for w in ws] for ws in roles["(2p,6p)"]]
    roles["x3"] = [L(v) for v in x3]
    return roles


def lz_product_cases(fid, nr=17):
    """{op: [operand tuples (a0, b0[, a1, b1[, a2, b2, a3, b3]])]} for lz_mul, lz_sqr, lz_dot2, lz_dot4: every combination of role extremes that a
    call site of madd_lz / madd_x_lz2 / lz_to_jac can produce, the pairs at the global limit ca cb = 1024, and the term combinations whose
    weights reach the stated sums 116 (madd_lz Y3), 648 (madd_x_lz2 PP.c0) and 792 (madd_x_lz2 Y3.c0)"""
    fld = FLD[fid]
    p, N = fld.p, fld.N
    r = lz_roles(fid, nr)
    L = lambda x: limbs(x, N)
    prod = lambda A, Bs: [(a, b) for a in A for b in Bs]
    mul = []
    mul += prod(r["normal"], r["normal"])                      # U2, S2, ZZ3, ZZZ3 (4)
    mul += prod(r["P<18p"], r["normal"])                       # PPP = P PP (36)
    mul += prod(r["X<16p"], r["normal"])                       # Q = X1 PP, lz_to_jac (32)
    mul += prod(r["2*(2p,6p)"], r["(2p,6p)"])                  # PP.c1 = (2 P0) P1 (72)
    # the global limit ca cb = 1024, carried operands (limb products per column: N 2^28 2^29 < 2^63)
    for ca in (32, 1024, 512, 64, 2):
        cb = 1024 // ca
        for a in (ca * p - 1, _all_ones_below(fld, ca * p)):
            for b in (cb * p - 1, cb * p, _all_ones_below(fld, cb * p) if cb > 1 else p):
                if a * b <= 1024 * p * p:
                    mul.append((L(a), L(b)))
    sqr = [(a,) for a in r["P<18p"] + r["(2p,6p)"] + r["normal"]] + [(L(32 * p - 1),), (L(_all_ones_below(fld, 32 * p)),)]
    dot2 = []
    # madd_lz Y3 = R t + Y1' PPP: 6 * 18 + 4 * 2 = 116 (the stated sum; the call site itself stays below 6 * 16 + 8 = 104, see lz_roles)
    for R in r["(2p,6p)"]:
        for t in r["t uncarried"]:
            for y in (r["4p-Y uncarried"][0], r["4p-Y uncarried"][2], r["4p-Y uncarried"][3]):
                for ppp in (r["normal"][4], r["normal"][5], r["normal"][0]):
                    dot2.append((R, t, y, ppp))
    # madd_x_lz2 PP.c0 = P0 P0 + P1 (nr P1): 36 (nr + 1) = 648; nr P1 is the carried scale of the SAME P1
    for P0 in r["(2p,6p)"]:
        for P1 in r["(2p,6p)"]:
            dot2.append((P0, P0, P1, L(nr * unlimbs(P1))))
    # madd_x_lz2 mulr: c0 = a0 b0 + a1 (nr b1), c1 = a0 b1 + a1 b0 with a in {normal, (2p,6p)} and b normal: <= 12 (nr + 1) = 216
    for a0 in (r["normal"][4], r["normal"][5], r["(2p,6p)"][2], r["(2p,6p)"][3]):
        for b in (r["normal"][4], r["normal"][5]):
            dot2.append((a0, b, a0, L(nr * unlimbs(b))))
            dot2.append((a0, b, a0, b))
    dot4 = []
    # madd_x_lz2 Y3.c0 = R0 t0 + (nr R1) t1 + Y0' PPP0 + Y1' (nr PPP1): (36 + 8) (nr + 1) = 792;  Y3.c1 = R0 t1 + R1 t0 + Y0' PPP1 + Y1' PPP0: 88
    band = r["(2p,6p)"]
    for R0, R1 in ((band[2], band[2]), (band[3], band[3]), (band[0], band[2]), (band[4], band[3])):
        for t0, t1 in ((band[2], band[2]), (band[3], band[2]), (band[0], band[0])):
            for y in (r["4p-Y uncarried"][0], r["4p-Y uncarried"][2], r["4p-Y uncarried"][3]):
                for ppp in (r["normal"][4], r["normal"][5]):
                    nR1, nppp = L(nr * unlimbs(R1)), L(nr * unlimbs(ppp))
                    dot4.append((R0, t0, nR1, t1, y, ppp, y, nppp))
                    dot4.append((R0, t1, R1, t0, y, ppp, y, ppp))
    return {L_MUL: mul, L_SQR: sqr, L_DOT2: dot2, L_DOT4: dot4}


def lz_terms(ops):
    return [(ops[i], ops[i + 1]) for i in range(0, len(ops), 2)] if len(ops) > 1 else [(ops[0], ops[0])]


def lz_exact(ops):
    """the exact integer sum a_i b_i of the signed-limb operands"""
    return sum(unlimbs(a) * unlimbs(b) for a, b in lz_terms(ops))


def lz_value_weight(fld, ops):
    """sum of the products of the operand values, in units of p^2 (what the comments bound by 1024)"""
    return lz_exact(ops) / (fld.p * fld.p)


def lz_columns_fit(fld, ops):
    """The limb-magnitude condition, from the operands alone: the Montgomery column sums of lz_dot / lz_sqr / lz_dot4 (operand products of
    column k, the m_i p_(k-i) terms with m_i < 2^28, and the carry from the column below) stay inside a signed 64-bit accumulator"""
    N = fld.N
    worst, carry = 0, 0
    for k in range(2 * N - 1):
        col = sum(abs(a[i]) * abs(b[k - i]) for a, b in lz_terms(ops) for i in range(max(0, k - N + 1), min(k, N - 1) + 1))
        col += min(k + 1, N, 2 * N - 1 - k) * MASK * MASK + carry
        worst = max(worst, col)
        carry = col >> 28
    return worst < (1 << 63)


# ----------------------------------------------------------------------------- towers
def tower_of(fid):
    """(degree, non-residue) of the plain tower the product computes G2 coordinates in over this base field"""
    for c in O.CURVES:
        if c.fq is O.FIELDS[fid]:
            return c.k // 2, c.nr
    raise KeyError(fid)


def tower_cases(fid, seed=5, n=96):
    """[(a, b)]: elements as tuples of raw coefficients, drawn from the operand classes (specials twice as likely as random ones)"""
    cls, ns = operand_classes(fid, seed)
    d, _ = tower_of(fid)
    rnd = random.Random(31 * seed + fid)
    sp, rd = [v for _, v in cls[:ns]], [v for _, v in cls[ns:]]
    pick = lambda: rnd.choice(sp) if rnd.random() < 0.66 else rnd.choice(rd)
    cases = [(tuple(pick() for _ in range(d)), tuple(pick() for _ in range(d))) for _ in range(n)]
    z = (0,) * d
    pz = (FLD[fid].p,) * d
    cases += [(z, z), (pz, z), (z, pz), ((1,) + (0,) * (d - 1), pz)]
    return cases


# ----------------------------------------------------------------------------- accumulator steps
def ext_to_raw(fld, e):
    return tuple(fld.mont(c) for c in e)


def raw_to_ext(fld, r):
    return tuple(fld.unmont(c) for c in r)


def small_points(cid, grp, n, seed):
    """n affine points k_i G (ext-tuples) with small seeded k_i"""
    c = O.CURVES[cid]
    F, a = c.group(grp)
    g = c.g1 if grp == 1 else c.g2
    rnd = random.Random(900 + 10 * cid + grp + seed)
    return [O.ec_mul(F, a, rnd.randrange(2, 1 << 20), g) for _ in range(n)]


def accumulator_of(cid, grp, pt, z):
    """(X, Y, ZZ, ZZZ) = (x z^2, y z^3, z^2, z^3) as ext-tuples of residues"""
    F, _ = O.CURVES[cid].group(grp)
    z2 = F.mul(z, z)
    z3 = F.mul(z2, z)
    return (F.mul(pt[0], z2), F.mul(pt[1], z3), z2, z3)


def affine_of(cid, grp, coords, inf):
    """the affine point of a raw accumulator record, by Python integers: x = X / ZZ, y = Y / ZZZ (four coordinates), or of a raw Jacobian
    record: x = X / Z^2, y = Y / Z^3 (three)"""
    if inf:
        return None
    c = O.CURVES[cid]
    F, _ = c.group(grp)
    fld = FLD[O.FIELDS.index(c.fq)]
    if len(coords) == 3:
        X, Y, Z = (raw_to_ext(fld, v) for v in coords)
        ZZ = F.mul(Z, Z)
        ZZZ = F.mul(ZZ, Z)
    else:
        X, Y, ZZ, ZZZ = (raw_to_ext(fld, v) for v in coords)
    return (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))


def jacobian_of(cid, grp, pt, z):
    """(X, Y, Z) = (x z^2, y z^3, z) as ext-tuples of residues"""
    return accumulator_of(cid, grp, pt, z)[:2] + (z,)


def lifted_record(fld, coords, lift, top=None):
    """the raw record of coordinates (tuples of raw coefficients below p): coordinate j on its upper representative c + p where bit j of `lift`
    is set (top[j] p where `top` names another band), every coefficient of it; then the identity flag 0"""
    rec = []
    for j, co in enumerate(coords):
        k = ((top[j] if top else 1) if (lift >> j) & 1 else 0)
        for cf in co:
            rec += limbs(cf + k * fld.p, fld.N)
    return rec + [0]


def step_cases(cid, grp, lz, seed=3, n_base=2, chain=8, jac=False):
    """[(raw accumulator record, [q_0 .. q_chain] raw affine images, expected affine point after step 1, ... after the whole chain, (kind, lift),
    (the accumulator's affine point, its z, the affine q_0 .. q_chain))]:
    valid accumulators (x z^2, y z^3, z^2, z^3) -- jac: Jacobian ones (x z^2, y z^3, z) -- with every coordinate lifted to the bottom and to
    the top representative of its band -- madd_lz's X: carried, below p or in [15p, 16p); every other coordinate c and c + p -- in all 16 (8)
    combinations, against q = a generic point, the accumulator's own point (doubling branch), its negative (infinity) and the infinity
    image; then `chain` generic steps.  Last, the identity record (flag set) against a generic point and against the infinity image."""
    c = O.CURVES[cid]
    F, a = c.group(grp)
    fld = FLD[O.FIELDS.index(c.fq)]
    p, N, d = fld.p, fld.N, F.d
    rnd = random.Random(4000 + 100 * seed + 10 * cid + grp)
    pts = small_points(cid, grp, n_base + chain + 1, seed)
    base, generic = pts[:n_base], pts[n_base:]
    aff_raw = lambda P: [0] * (2 * d * N) if P is None else [w for co in P for cf in co for w in limbs(fld.mont(cf), N)]
    ncoord = 3 if jac else 4
    cases = []

    def emit(rec, pt, z, q, tag):
        qs = [q] + generic[1:1 + chain]
        want1 = O.ec_add(F, a, pt, q)
        want = want1
        for g in qs[1:]:
            want = O.ec_add(F, a, want, g)
        cases.append((rec, [aff_raw(x) for x in qs], want1, want, tag, (pt, z, qs)))
    for pt in base:
        z = tuple(rnd.randrange(1, p) for _ in range(d))
        coords = [ext_to_raw(fld, e) for e in (jacobian_of if jac else accumulator_of)(cid, grp, pt, z)]
        for lift in range(1 << ncoord):
            rec = lifted_record(fld, coords, lift, top=(15, 1, 1, 1) if lz else None)
            for kind, q in (("generic", generic[0]), ("same", pt), ("negative", O.ec_neg(F, pt)), ("infinity", None)):
                emit(rec, pt, z, q, (kind, lift))
    for kind, q in (("identity+generic", generic[0]), ("identity+infinity", None)):
        emit([0] * (ncoord * d * N) + [1], None, None, q, (kind, 0))
    return cases


def jadd_cases(cid, grp, seed=6, n_base=2):
    """[(raw Jacobian record of P, raw Jacobian record of Q, expected affine P + Q, (kind, lift), (P, zP, Q, zQ))] for EC::add: P and Q with
    Z lifted independently (bits 0, 1 of `lift`) and X, Y of either lifted together (bits 2, 3), Q = a generic point, P itself and -P under
    a DIFFERENT Z (the H = 0 branch through unequal coordinates); then the identity on the left, on the right and on both sides, as
    the flagged record, as literal Z = 0 and as Z = p in every coefficient under arbitrary X, Y"""
    c = O.CURVES[cid]
    F, a = c.group(grp)
    fld = FLD[O.FIELDS.index(c.fq)]
    p, N, d = fld.p, fld.N, F.d
    rnd = random.Random(6000 + 100 * seed + 10 * cid + grp)
    pts = small_points(cid, grp, n_base + 1, seed + 1)
    base, generic = pts[:n_base], pts[n_base]
    rz = lambda: tuple(rnd.randrange(1, p) for _ in range(d))

    def record(pt, z, lz_, lxy):
        coords = [ext_to_raw(fld, e) for e in jacobian_of(cid, grp, pt, z)]
        return lifted_record(fld, coords, (4 if lz_ else 0) | (3 if lxy else 0))

    def identity(form):
        if form == "flag":
            return [0] * (3 * d * N) + [1]
        xy = [w for _ in range(2 * d) for w in limbs(rnd.randrange(2 * p), N)]
        return xy + [w for _ in range(d) for w in limbs(p if form == "Z=p" else 0, N)] + [0]
    cases = []
    for pt in base:
        zp = rz()
        for kind, q in (("generic", generic), ("same", pt), ("negative", O.ec_neg(F, pt))):
            zq = rz()
            assert zq != zp
            for lift in range(16):
                cases.append((record(pt, zp, lift & 1, lift & 4), record(q, zq, lift & 2, lift & 8), O.ec_add(F, a, pt, q), (kind, lift), (pt, zp, q, zq)))
        for form in ("flag", "Z=0", "Z=p"):
            for lift in range(2):
                cases.append((identity(form), record(pt, zp, lift, lift), pt, ("identity left " + form, lift), (None, None, pt, zp)))
                cases.append((record(pt, zp, lift, lift), identity(form), pt, ("identity right " + form, lift), (pt, zp, None, None)))
            cases.append((identity(form), identity("flag" if form == "Z=p" else "Z=p"), None, ("identity both " + form, 0), (None, None, None, None)))
    return cases


def jac_unary_cases(cid, grp, seed=8, n_base=2):
    """[(raw Jacobian record of P, P, (kind, lift), z)] for EC::dbl and x_to_jac(x_from(.)): every coordinate lifted, in all 8 combinations,
    and the identity in its three forms"""
    c = O.CURVES[cid]
    F, _ = c.group(grp)
    fld = FLD[O.FIELDS.index(c.fq)]
    p, N, d = fld.p, fld.N, F.d
    rnd = random.Random(8000 + 100 * seed + 10 * cid + grp)
    cases = []
    for pt in small_points(cid, grp, n_base, seed + 2):
        z = tuple(rnd.randrange(1, p) for _ in range(d))
        coords = [ext_to_raw(fld, e) for e in jacobian_of(cid, grp, pt, z)]
        for lift in range(8):
            cases.append((lifted_record(fld, coords, lift), pt, ("finite", lift), z))
    xy = lambda: [w for _ in range(2 * d) for w in limbs(rnd.randrange(2 * p), N)]
    cases.append(([0] * (3 * d * N) + [1], None, ("identity flag", 0), None))
    cases.append((xy() + [0] * (d * N) + [0], None, ("identity Z=0", 0), None))
    cases.append((xy() + [w for _ in range(d) for w in limbs(p, N)] + [0], None, ("identity Z=p", 0), None))
    return cases


# ----------------------------------------------------------------------------- drivers: one launch per case list, checked against the integers
class Backend:
    """ctypes entry points of one build of the per-element code: prefix 'hc' (host, tests/hostcheck) or 'gc' (gfx950, tests/gpucheck)"""

    def __init__(self, lib, prefix):
        import ctypes as C
        self.C = C
        self.f_field = getattr(lib, "hc_field_case_ops" if prefix == "hc" else "gc_field_ops")
        self.f_lz = getattr(lib, prefix + "_lz_ops")
        self.f_tower = getattr(lib, prefix + "_tower_ops")
        self.f_step = getattr(lib, prefix + "_madd_step")
        vp, i, u = C.c_void_p, C.c_int, C.c_uint32
        self.f_field.argtypes = [i, i, i, vp, vp, u, i, vp, vp]
        self.f_lz.argtypes = [i, i, vp, C.c_int32, i, vp, vp]
        self.f_tower.argtypes = [i, i, vp, vp, i, vp, vp]
        self.f_step.argtypes = [i, i, i, vp, vp, i, i, vp, vp]

    def _call(self, fn, head, arrays, mid, n, out_words):
        import numpy as np
        arrs = [np.ascontiguousarray(np.array(a, dtype=np.int64).astype(np.uint32).reshape(-1)) for a in arrays]
        out = np.zeros(n * out_words + 1, dtype=np.uint32)
        ran = np.zeros(1, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(self.C.c_void_p)
        rc = fn(*head, *[ptr(a) for a in arrs], *mid, n, ptr(out), ptr(ran))
        assert rc == 0, ("harness error", rc)
        assert int(ran[0]) == n, ("elements run", int(ran[0]), "of", n)
        return [[int(w) for w in out[i * out_words:(i + 1) * out_words]] for i in range(n)]

    def field(self, fid, variant, op, a_rows, b_rows, k=0):
        return self._call(self.f_field, (fid, variant, op), (a_rows, b_rows), (k,), len(a_rows), FLD[fid].N)

    def lz(self, fid, op, rows, k=0):
        return self._call(self.f_lz, (fid, op), (rows,), (k,), len(rows), FLD[fid].N)

    def tower(self, fid, op, a_rows, b_rows):
        return self._call(self.f_tower, (fid, op), (a_rows, b_rows), (), len(a_rows), FLD[fid].N * tower_of(fid)[0])

    def step(self, cid, grp, op, acc_rows, q_rows, steps):
        return self._call(self.f_step, (cid, grp, op), (acc_rows, q_rows), (steps,), len(acc_rows), len(acc_rows[0]))


FIELD_OPS = {"mul": F_MUL, "sqr": F_SQR, "add": F_ADD, "sub": F_SUB, "neg": F_NEG, "dbl": F_DBL, "mul_small": F_MUL_SMALL,
             "mul_small_var": F_MUL_SMALL_VAR, "inv_gcd": F_INV_GCD, "inv_fermat": F_INV_FERMAT, "mul_inv": F_MUL_INV, "canonical": F_CANONICAL,
             "is_zero": F_IS_ZERO, "eq": F_EQ, "to_abi": F_TO_ABI, "abi_roundtrip": F_ABI_ROUNDTRIP, "to_words": F_TO_WORDS,
             "words_roundtrip": F_WORDS_ROUNDTRIP, "signed_sum": F_SIGNED_SUM}


def _ragged(cases):
    """at least one partly filled 64-lane wave per launch"""
    return cases + cases[:1] if len(cases) % 64 == 0 else cases


def check_field_op(be, fid, variant, name):
    """runs every case of operation `name` through backend `be` and checks each result against Python integers; returns the case count"""
    fld = FLD[fid]
    p, N, op = fld.p, fld.N, FIELD_OPS[name]
    L = lambda x: limbs(x, N)
    total = 0
    if name == "signed_sum":
        for T, lst in signed_sum_cases(fid).items():
            lst = _ragged(lst)
            out = be.field(fid, variant, op, [[w for x in a for w in L(x)] for a, _ in lst], [c for _, c in lst], T)
            for (a, c), ws in zip(lst, out):
                check_reduced(fld, ws, sum(x * y for x, y in zip(a, c)), (name, a, c))
            total += len(lst)
        return total
    if name in ("mul_small", "mul_small_var"):
        vals = _ragged(unary_cases(fid))
        for k in small_constants(fid):
            out = be.field(fid, variant, op, [L(a) for a in vals], [L(0)] * len(vals), k)
            for a, ws in zip(vals, out):
                r = check_reduced(fld, ws, k * a, (name, k, a))
                if name == "mul_small" and k < 2:
                    assert r == k * a, (name, k, a)
            total += len(vals)
        return total
    if name in ("mul", "add", "sub", "eq"):
        pairs = binary_cases(fid)
        if name in ("add", "sub"):
            pairs = pairs + addsub_band_pairs(fid)
        if name == "eq":
            pairs = pairs + [(a, b) for a in unary_cases(fid) for b in (a, a + p, a - p, a + 1, 2 * p - 1 - a) if 0 <= b < 2 * p]
        pairs = _ragged(pairs)
        out = be.field(fid, variant, op, [L(a) for a, _ in pairs], [L(b) for _, b in pairs])
        for (a, b), ws in zip(pairs, out):
            if name == "mul":
                check_reduced(fld, ws, a * b * fld.Rinv, (name, a, b))
            elif name == "eq":
                same = (a - b) % p == 0
                assert ws[0] == int(same) and ws[1] == int(not same), (name, a, b)
            else:
                assert is_normal(ws) and unlimbs(ws) == (add_exact if name == "add" else sub_exact)(fld, a, b), (name, a, b)
        return len(pairs)
    vals = _ragged(unary_cases(fid))
    out = be.field(fid, variant, op, [L(a) for a in vals], [L(0)] * len(vals))
    for a, ws in zip(vals, out):
        what = (name, a)
        if name == "sqr":
            check_reduced(fld, ws, a * a * fld.Rinv, what)
        elif name in ("neg", "dbl"):
            assert is_normal(ws) and unlimbs(ws) == (sub_exact(fld, 0, a) if name == "neg" else add_exact(fld, a, a)), what
        elif name in ("inv_gcd", "inv_fermat"):
            if a % p == 0:
                r = check_reduced(fld, ws, 0, what)
                assert name == "inv_fermat" or r == 0, what   # inv(0) == 0 on both representatives of zero (a^(p-2), the cross-check, may return p)
            else:
                r = check_reduced(fld, ws, fld.R * fld.R * pow(a, -1, p), what)        # (x R')^-1 R'^2 = x^-1 R'
                assert fld.unmont(r) == pow(fld.unmont(a), -1, p), what
        elif name == "mul_inv":
            assert is_normal(ws) and unlimbs(ws) == (0 if a % p == 0 else fld.R % p), what   # a inv(a) = 1, canonical
        elif name == "canonical":
            assert is_normal(ws) and unlimbs(ws) == a % p, what
        elif name == "is_zero":
            assert ws[0] == int(a in (0, p)), what
        elif name in ("to_abi", "to_words"):
            got = sum(w << (32 * i) for i, w in enumerate(ws[:fld.n32]))
            assert got == fld.unmont(a) * (fld.R_abi if name == "to_abi" else 1) % p, what
        elif name in ("abi_roundtrip", "words_roundtrip"):
            check_reduced(fld, ws, a, what)
        else:
            raise KeyError(name)
    return len(vals)


def check_lz_products(be, fid, nr=17):
    """lz_mul / lz_sqr / lz_dot2 / lz_dot4 on the role extremes: the exact integer sum a_i b_i of the signed-limb operands is the reference"""
    fld = FLD[fid]
    N = fld.N
    counts = {}
    for op, cases in lz_product_cases(fid, nr).items():
        cases = _ragged(cases)
        for ops in cases:   # the declared bounds, from the operands alone (the harness would stop the process where they break)
            assert 0 <= lz_exact(ops) <= 1024 * fld.p * fld.p, ("value bound ca cb <= 1024", op, ops)
            assert lz_columns_fit(fld, ops), ("column sums below 2^63", op, ops)
            assert all(-(1 << 31) <= w < (1 << 31) for o in ops for w in o), ("limb does not fit 32 bits", op, ops)
        rows = [[w for o in ops for w in o] + [0] * (N * (8 - len(ops))) for ops in cases]
        out = be.lz(fid, op, rows)
        for ops, ws in zip(cases, out):
            check_reduced(fld, ws, lz_exact(ops) * fld.Rinv, (op, ops))
        counts[op] = len(cases)
    return counts


def check_lz_forms(be, fid, nr=17):
    """lz_scale_carry, lz_carry, lz_sub<0>, lz_sub<2>, lz_shl: exact limb images"""
    fld = FLD[fid]
    N = fld.N
    r = lz_roles(fid, nr)
    pad = lambda *ops: [w for o in ops for w in o] + [0] * (N * (8 - len(ops)))
    n = 0
    for k in (nr, 13, 5, 11):
        ins = _ragged(r["normal"] + r["(2p,6p)"])
        out = be.lz(fid, L_SCALE_CARRY, [pad(a) for a in ins], k)
        for a, ws in zip(ins, out):
            assert signed(ws) == limbs(k * unlimbs(a), N), ("lz_scale_carry", k, a)
        n += len(ins)
    ins = _ragged(r["t uncarried"] + r["4p-Y uncarried"] + r["normal"] + r["2*(2p,6p)"])
    for a, ws in zip(ins, be.lz(fid, L_CARRY, [pad(a) for a in ins])):
        assert signed(ws) == limbs(unlimbs(a), N), ("lz_carry", a)
    n += len(ins)
    pairs = _ragged([(a, b) for a in r["normal"] for b in r["normal"] + r["X<16p"] + r["x3"]])
    for S, op in ((0, L_SUB0), (2, L_SUB2)):
        for (a, b), ws in zip(pairs, be.lz(fid, op, [pad(a, b) for a, b in pairs])):
            assert signed(ws) == lz_sub_limbs(fld, a, b, S), ("lz_sub", S, a, b)
        n += len(pairs)
    ins = _ragged(r["(2p,6p)"])
    for a, ws in zip(ins, be.lz(fid, L_SHL, [pad(a) for a in ins], 1)):
        assert signed(ws) == [2 * w for w in a], ("lz_shl", a)
    return n + len(ins)


def check_tower_op(be, fid, name):
    fld = FLD[fid]
    N = fld.N
    d, nr = tower_of(fid)
    E = O.Ext(fld.p, d, nr)
    cases = _ragged(tower_cases(fid))
    flat = lambda e: [w for c in e for w in limbs(c, N)]
    out = be.tower(fid, {"mul": T_MUL, "sqr": T_SQR, "inv": T_INV}[name], [flat(a) for a, _ in cases], [flat(b) for _, b in cases])
    for (a, b), ws in zip(cases, out):
        x, y = raw_to_ext(fld, a), raw_to_ext(fld, b)
        want = E.mul(x, y) if name == "mul" else E.mul(x, x) if name == "sqr" else (E.zero() if x == E.zero() else E.inv(x))
        for j in range(d):
            check_reduced(fld, ws[j * N:(j + 1) * N], fld.mont(want[j]), (name, a, b, j))
    return len(cases)


def record_point(cid, grp, fld, ws, W, ncoord, flags, want, tag, lz_x=False):
    """one returned record -- ncoord coordinate images of W words at ws[0:], identity flags `flags` (one, or one per lane of the item: all
    must agree) -- against the expected affine point: the flag exact, limbs normalised, every coefficient below 2p (madd_lz's X: carried,
    below 16p), and the affine point equal by Python integers"""
    N = fld.N
    assert all(f in (0, 1) for f in flags) and len(set(flags)) == 1, ("identity flags", tag, flags)
    assert flags[0] == int(want is None), ("identity flag", tag, flags[0])
    if want is None:
        return
    coords = []
    for j in range(ncoord):
        co = []
        for i in range(0, W, N):
            words = ws[j * W + i:j * W + i + N]
            if lz_x and j == 0:
                words = signed(words)
            assert is_normal(words), ("limb not normalised", tag, j)
            v = unlimbs(words)
            assert 0 <= v < (16 if (lz_x and j == 0) else 2) * fld.p, ("coordinate outside its band", tag, j)
            co.append(v)
        coords.append(tuple(co))
    assert affine_of(cid, grp, coords, False) == want, ("wrong point", tag)


def check_steps(be, cid, grp, op):
    """one addition step and the chain behind it from every lifted accumulator, against the affine group law in Python integers"""
    c = O.CURVES[cid]
    fld = FLD[O.FIELDS.index(c.fq)]
    ncoord = 3 if op == S_MADD_JAC else 4
    cases = step_cases(cid, grp, lz=(op == S_MADD_LZ), jac=(op == S_MADD_JAC))
    W = (len(cases[0][0]) - 1) // ncoord
    for steps, idx in ((1, 2), (len(cases[0][1]), 3)):
        out = be.step(cid, grp, op, [rec for rec, *_ in cases], [[w for q in qs[:steps] for w in q] for _, qs, *_ in cases], steps)
        for case, ws in zip(cases, out):
            record_point(cid, grp, fld, ws, W, ncoord, ws[ncoord * W:], case[idx], (cid, grp, op, steps, case[4]), lz_x=(op == S_MADD_LZ))
    return len(cases)


# ----------------------------------------------------------------------------- lane-split towers and the group law in them (gfx950 only)
# type / group numbers and operation numbers of tests/gpucheck/lanesplit_check.hip; the coordinate field of split group g is split type g
SPLIT_NAMES = ["Fp2S-298A", "Fp3S-298B", "Fp2S-753A", "Fp3S-753B", "Fp2S-753A-mailbox", "Fp3S-753B-mailbox"]
SPLIT_TOWER_OPS = ["mul", "sqr", "add", "sub", "neg", "dbl", "mul_small", "mul_by_a", "is_zero", "is_raw_zero", "eq", "one", "from_abi",
                   "abi_roundtrip"]
SPLIT_GROUP_OPS = ["S_MADD_X", "S_MADD_JAC", "J_ADD", "J_DBL", "X_ROUNDTRIP"]


def split_curve(sid):
    """the curve (= base field) number of a split type / group: 0 .. 3 plain, 4 / 5 the mailbox forms over fields 2 / 3"""
    return sid if sid < 4 else sid - 2


def split_zero_cases(fid, seed=9):
    """[(a, b)] for is_zero / is_raw_zero / ==: exactly ONE coefficient 0 or p and the others not; the same element on the other
    representative of every coefficient; pairs that differ in one coefficient only and pairs that agree in one only; every coefficient
    but one zero; and every mix of the representatives 0 and p (the zero element)"""
    p = FLD[fid].p
    d, _ = tower_of(fid)
    rnd = random.Random(9000 + 10 * seed + fid)
    nz = lambda: rnd.choice([1, p - 1, p + 1, 2 * p - 1, rnd.randrange(2, p - 1), rnd.randrange(p + 2, 2 * p - 1)])
    other = lambda c: c + p if c < p else c - p
    cases = []
    for j in range(d):
        for z in (0, p):
            a = tuple(z if i == j else nz() for i in range(d))
            cases.append((a, a))
            cases.append((a, tuple(other(c) for c in a)))
            b = list(a)
            while (b[j] - a[j]) % p == 0:
                b[j] = nz()
            cases.append((a, tuple(b)))                                                     # differ in coefficient j only
            cases.append((a, tuple(a[i] if i == j else (a[i] + 1) % (2 * p) for i in range(d))))   # agree in coefficient j only
            cases.append((tuple(nz() if i == j else rnd.choice((0, p)) for i in range(d)), a))     # every coefficient but j zero
    for m in range(1 << d):
        zero = tuple(p if (m >> i) & 1 else 0 for i in range(d))
        cases.append((zero, tuple(p - c for c in zero)))
    return cases


def split_tower_cases(fid):
    """tower_cases (100 pairs, every coefficient drawn independently from the operand classes) and split_zero_cases"""
    return tower_cases(fid) + split_zero_cases(fid)


def split_masks(n, seed=11):
    """the three active-item masks every case list runs under: all items, every third item inactive, a seeded random half inactive"""
    rnd = random.Random(seed + n)
    half = [1] * n
    for i in rnd.sample(range(n), n // 2):
        half[i] = 0
    return [("all", [1] * n), ("every third off", [0 if i % 3 == 2 else 1 for i in range(n)]), ("random half off", half)]


class SplitBackend:
    """ctypes entry points of tests/gpucheck/libgpucheck_ls.so"""

    def __init__(self, lib):
        import ctypes as C
        self.C, self.lib = C, lib
        vp, i, u = C.c_void_p, C.c_int, C.c_uint32
        lib.gc_split_tower_ops.argtypes = [i, i, vp, vp, u, i, vp, vp, vp]
        lib.gc_split_group_ops.argtypes = [i, i, vp, vp, i, i, vp, vp, vp]
        lib.gc_split_words.argtypes = [i, i, i, i, vp]
        lib.gc_split_sentinel.restype = u
        self.sentinel = int(lib.gc_split_sentinel())

    def _call(self, what, sid, op, a_rows, b_rows, mid, active):
        """one launch: rows of the ACTIVE items as lists of words, None for the inactive ones.  Checked here: the harness's own word counts
        against the rows passed, `ran` = lanes per item times active items, every word of an inactive item still the sentinel"""
        import numpy as np
        n = len(a_rows)
        assert n == len(b_rows) == len(active) and n > 0
        w3 = np.zeros(3, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(self.C.c_void_p)
        assert self.lib.gc_split_words(what, sid, op, mid if what == 1 else 0, ptr(w3)) == 0
        wa, wb, wo = (int(x) for x in w3)
        arrs = []
        for rows, w in ((a_rows, wa), (b_rows, wb)):
            assert all(len(r) == w for r in rows), ("operand words", w, [len(r) for r in rows][:3])
            arrs.append(np.ascontiguousarray(np.array(rows, dtype=np.int64).astype(np.uint32).reshape(-1)))
            assert arrs[-1].size == n * w
        act = np.ascontiguousarray(np.array(active, dtype=np.uint8))
        out = np.zeros(n * wo + 1, dtype=np.uint32)
        ran = np.zeros(1, dtype=np.uint32)
        fn = self.lib.gc_split_tower_ops if what == 0 else self.lib.gc_split_group_ops
        rc = fn(sid, op, ptr(arrs[0]), ptr(arrs[1]), mid, n, ptr(act), ptr(out), ptr(ran))
        assert rc == 0, ("harness error", rc)
        L = 2 + split_curve(sid) % 2
        assert int(ran[0]) == L * sum(active), ("lanes run", int(ran[0]), "of", L * sum(active))
        rows = []
        for i in range(n):
            ws = [int(w) for w in out[i * wo:(i + 1) * wo]]
            if active[i]:
                rows.append(ws)
            else:
                assert all(w == self.sentinel for w in ws), ("inactive item written", i)
                rows.append(None)
        return rows

    def tower(self, sid, op, a_rows, b_rows, k, active):
        return self._call(0, sid, op, a_rows, b_rows, k, active)

    def group(self, sid, op, p_rows, q_rows, steps, active):
        return self._call(1, sid, op, p_rows, q_rows, steps, active)


def _mask_runs(cases):
    """(label, case list, active flags): the whole list under the three masks, then its first item alone (one item, L active lanes in a
    partly filled wave: the shape of the single-item kernels)"""
    return [(lbl, cases, act) for lbl, act in split_masks(len(cases))] + [("one item", cases[:1], [1])]


def abi_words(fld, x):
    """the C-ABI image of the residue x: x R mod p (R = 2^(32 n32)), n32 little-endian 32-bit words"""
    v = x * fld.R_abi % fld.p
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(fld.n32)]


def check_split_tower_op(sb, sid, name):
    """every case of one operation of one lane-split type, under every mask, against Python integers; returns the number of items checked"""
    fid = split_curve(sid)
    fld = FLD[fid]
    p, N = fld.p, fld.N
    d, nr = tower_of(fid)
    curve = O.CURVES[fid]
    assert curve.fq is O.FIELDS[fid]
    E = O.Ext(p, d, nr)
    op = SPLIT_TOWER_OPS.index(name)
    flat = lambda e: [w for c in e for w in limbs(c, N)]
    pad = lambda ws: ws + [0] * (d * N - len(ws))
    checked = 0
    for k in (small_constants(fid) if name == "mul_small" else [0]):
        for lbl, cases, active in _mask_runs(split_tower_cases(fid)):
            if name in ("from_abi", "abi_roundtrip"):
                a_rows = [pad([w for c in a for w in abi_words(fld, c % p)]) for a, _ in cases]
            else:
                a_rows = [flat(a) for a, _ in cases]
            out = sb.tower(sid, op, a_rows, [flat(b) for _, b in cases], k, active)
            for (a, b), row, ws in zip(cases, a_rows, out):
                if ws is None:
                    continue
                what = (SPLIT_NAMES[sid], name, k, lbl, a, b)
                co = [ws[j * N:(j + 1) * N] for j in range(d)]
                if name in ("is_zero", "is_raw_zero", "eq"):
                    want = {"is_zero": all(c % p == 0 for c in a), "is_raw_zero": all(c == 0 for c in a),
                            "eq": all((x - y) % p == 0 for x, y in zip(a, b))}[name]
                    for j in range(d):   # every lane of the item reports, and all agree
                        assert co[j][0] == int(want), (what, "lane", j)
                        if name == "eq":
                            assert co[j][1] == int(not want), (what, "lane", j, "!=")
                elif name == "abi_roundtrip":
                    assert ws[:d * fld.n32] == row[:d * fld.n32], what
                    assert all(w == sb.sentinel for w in ws[d * fld.n32:]), what
                else:
                    x, y = raw_to_ext(fld, a), raw_to_ext(fld, b)
                    if name == "mul":
                        want = [fld.mont(c) for c in E.mul(x, y)]
                    elif name == "sqr":
                        want = [fld.mont(c) for c in E.mul(x, x)]
                    elif name == "mul_by_a":   # the twist coefficient of the curve itself: (a nr, 0) in Fq2, (0, 0, a) = a u^2 in Fq3
                        want = list(E.mul(tuple(c % p for c in a), curve.a2))
                    elif name == "one":
                        want = [fld.R] + [0] * (d - 1)
                    elif name == "from_abi":
                        want = [fld.mont(c % p) for c in a]   # the C-ABI image was that of the residue a_j mod p
                    else:
                        want = {"add": [x_ + y_ for x_, y_ in zip(a, b)], "sub": [x_ - y_ for x_, y_ in zip(a, b)], "neg": [-x_ for x_ in a],
                                "dbl": [2 * x_ for x_ in a], "mul_small": [k * x_ for x_ in a]}[name]
                    for j in range(d):
                        check_reduced(fld, co[j], want[j], (what, "coefficient", j))
                checked += 1
    return checked


def split_group_cases(sid, name):
    """the case list of one group operation in one lane-split group: rows p, q of the harness, expected affine points, tags"""
    cid = split_curve(sid)
    if name in ("S_MADD_X", "S_MADD_JAC"):
        return step_cases(cid, 2, lz=False, jac=(name == "S_MADD_JAC"))
    if name == "J_ADD":
        return jadd_cases(cid, 2)
    return jac_unary_cases(cid, 2)


def check_split_group_op(sb, sid, name):
    """every case of one group operation in one lane-split group, under every mask, against the affine group law in Python integers;
    returns the number of items checked"""
    cid = split_curve(sid)
    c = O.CURVES[cid]
    F, a = c.group(2)
    fld = FLD[O.FIELDS.index(c.fq)]
    W = F.d * fld.N
    L = F.d
    op = SPLIT_GROUP_OPS.index(name)
    all_cases = split_group_cases(sid, name)
    chain = name in ("S_MADD_X", "S_MADD_JAC")
    ncoord = 4 if name == "S_MADD_X" else 3
    checked = 0
    for steps, idx in (((1, 2), (len(all_cases[0][1]), 3)) if chain else ((0, None),)):
        for lbl, cases, active in _mask_runs(all_cases):
            if chain:
                q_rows = [[w for q in case[1][:steps] for w in q] for case in cases]
            elif name == "J_ADD":
                q_rows = [case[1] for case in cases]
            else:
                q_rows = [[] for _ in cases]
            out = sb.group(sid, op, [case[0] for case in cases], q_rows, steps, active)
            for case, ws in zip(cases, out):
                if ws is None:
                    continue
                if chain:
                    want, tag = case[idx], case[4]
                elif name == "J_ADD":
                    want, tag = case[2], case[3]
                else:
                    want, tag = (O.ec_add(F, a, case[1], case[1]) if name == "J_DBL" else case[1]), case[2]
                record_point(cid, 2, fld, ws, W, ncoord, ws[4 * W:4 * W + L], want, (SPLIT_NAMES[sid], name, steps, lbl, tag))
                if ncoord == 3:
                    assert all(w == sb.sentinel for w in ws[3 * W:4 * W]), ("fourth slot written", SPLIT_NAMES[sid], name, tag)
                checked += 1
    return checked
