"""Integer reference for the K7 commit tests (tests/test_kzg_commit_host.py, tests/test_gpu_kzg_commit.py): the trimmed length of a
coefficient list, then the oracle's MSM over the canonical integers, its Jacobian addition and its normalisation -- what
ark-poly-commit `KZG10::commit` computes for a polynomial and its blinding polynomial.  The host test pins it against Horner
evaluation on a setup with known beta and gamma, independently of the library."""
import random

import numpy as np

import kzg_reference as kr


def trimmed_len(a, p):
    """index of the highest non-zero coefficient, plus one (0 for a zero or empty polynomial)"""
    n = len(a)
    while n and a[n - 1] % p == 0:
        n -= 1
    return n


def commit(co, curve, powers, a, gpowers=None, bl=None, offset=0, nthreads=8):
    """-> (affine x || y, flag, trimmed length) of MSM(powers[offset : offset + t], a) + MSM(gpowers[: len(bl)], bl)"""
    fr = co.CURVE_FR[curve]
    p, L = kr.MODULI[fr], kr.LIMBS[fr]
    t = trimmed_len(a, p)
    acc = None
    if t:
        assert offset + t <= len(powers)
        acc = co.msm(curve, 1, powers[offset:offset + t], kr.limbs_of_ints(a[:t], L), nthreads=nthreads)
    if bl:
        assert len(bl) <= len(gpowers)
        h = co.msm(curve, 1, gpowers[:len(bl)], kr.limbs_of_ints(bl, L), nthreads=nthreads)
        acc = h if acc is None else co.jac_add(curve, 1, acc, h)
    if acc is None:
        return np.zeros(co.point_words(curve, 1), dtype=np.uint64), 1, t
    xy, inf = co.to_affine(curve, 1, acc)
    return (np.zeros_like(xy[0]) if inf[0] else xy[0]), int(inf[0]), t


class Srs:
    """KZG10 setup that keeps its trapdoor: powers_of_g = [beta^i] g, powers_of_gamma_g = [gamma beta^i] g, h, beta h"""

    def __init__(self, co, curve, degree, seed):
        rnd = random.Random(seed)
        fr = co.CURVE_FR[curve]
        p = kr.MODULI[fr]
        self.curve, self.fr, self.p = curve, fr, p
        self.beta, self.gamma = rnd.randrange(1, p), rnd.randrange(1, p)
        g, h = co.generator(curve, 1), co.generator(curve, 2)
        L = kr.LIMBS[fr]
        pw = [pow(self.beta, i, p) for i in range(degree + 1)]
        self.powers, _ = co.fixed_base_mul(curve, 1, g, kr.limbs_of_ints(pw, L), nthreads=8)
        self.gpowers, _ = co.fixed_base_mul(curve, 1, g, kr.limbs_of_ints([self.gamma * x % p for x in pw], L), nthreads=8)
        bh, _ = co.fixed_base_mul(curve, 2, h, kr.limbs_of_ints([self.beta], L))
        self.g, self.gamma_g, self.h, self.beta_h = g, self.gpowers[0], h, bh[0]

    def exponent_times_g(self, co, e):
        """(e g) as (affine, flag), by the oracle's double-and-add"""
        xy, inf = co.to_affine(self.curve, 1, co.scalar_mul(self.curve, 1, self.g, kr.limbs_of_ints([e % self.p], kr.LIMBS[self.fr])[0]))
        return (np.zeros_like(xy[0]) if inf[0] else xy[0]), int(inf[0])
