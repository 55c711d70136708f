"""Integer reference for the K13 tests (tests/test_kzg_batch_open_host.py, tests/test_gpu_kzg_batch_open.py): the parts of a round's
openings -- combined polynomial, combined blinding polynomial R, one degree-bound term per non-zero s -- by the exact arithmetic of
tests/kzg_reference.py, their witness through the oracle's MSM, and the collapse of linear combinations and per-query challenges onto
the two coefficient vectors of pcdhip_kzg_batch_open.  An item is a dict of integer lists: `poly`, optionally `blinding`, `shifted`
(bool), `shifted_offset`, `shifted_blinding`."""
import numpy as np

import kzg_reference as kr


def parts_of_opening(items, z, a_row, s_row, p):
    """-> dict: "comb" / "rand": (coefficients, quotient, value) or None when no term has a coefficient; "db": {i: (scaled quotient,
    p_i(z))} for the items with s != 0 and at least one coefficient"""
    s_row = s_row if s_row is not None else [0] * len(items)
    comb = [(it["poly"], a % p) for it, a in zip(items, a_row) if a % p and len(it["poly"])]
    rand = [(it["blinding"], a % p) for it, a in zip(items, a_row) if a % p and it.get("blinding")]
    rand += [(it["shifted_blinding"], s % p) for it, s in zip(items, s_row) if s % p and it.get("shifted_blinding")]
    out = {"db": {}}
    for name, terms in (("comb", comb), ("rand", rand)):
        if not terms:
            out[name] = None
            continue
        c = kr.lincomb([t[0] for t in terms], [t[1] for t in terms], p)
        q, v = kr.div_linear(c, z, p)
        out[name] = (c, q, v)
    for i, (it, s) in enumerate(zip(items, s_row)):
        if s % p:
            assert it.get("shifted"), "s != 0 on an item without a degree bound"
            if len(it["poly"]):
                q, v = kr.div_linear(it["poly"], z, p)
                out["db"][i] = ([s * x % p for x in q], v)
    return out


def witness_exponent(srs, items, z, a_row, s_row):
    """the exponent of W on a setup whose trapdoor is kept: the quotients of parts_of_opening at beta -> (w, value, random_v)"""
    p = srs.p
    pt = parts_of_opening(items, z, a_row, s_row, p)
    w = 0
    if pt["comb"]:
        w += kr.horner(pt["comb"][1], srs.beta, p)
    if pt["rand"]:
        w += srs.gamma * kr.horner(pt["rand"][1], srs.beta, p)
    for i, (q, _) in pt["db"].items():
        w += pow(srs.beta, items[i].get("shifted_offset", 0), p) * kr.horner(q, srs.beta, p)
    return w % p, (pt["comb"][2] if pt["comb"] else 0), (pt["rand"][2] if pt["rand"] else 0)


def identity_sides(srs, items, z, a_row, s_row, w):
    """(w (beta - z),  p_o(beta) - p_o(z) + gamma (R_o(beta) - R_o(z)) + sum_i s_i beta^offset_i (p_i(beta) - p_i(z)))"""
    p, b = srs.p, srs.beta
    s_row = s_row if s_row is not None else [0] * len(items)
    ev = lambda c, x: kr.horner(c, x, p)
    rhs = 0
    for it, a, s in zip(items, a_row, s_row):
        rhs += a * (ev(it["poly"], b) - ev(it["poly"], z))
        if it.get("blinding"):
            rhs += srs.gamma * a * (ev(it["blinding"], b) - ev(it["blinding"], z))
        if s % p:
            rhs += s * pow(b, it.get("shifted_offset", 0), p) * (ev(it["poly"], b) - ev(it["poly"], z))
            if it.get("shifted_blinding"):
                rhs += srs.gamma * s * (ev(it["shifted_blinding"], b) - ev(it["shifted_blinding"], z))
    return w * (b - z) % p, rhs % p


def batch_open(co, curve, powers, gpowers, spowers, items, points, a, s, nthreads=8):
    """-> per opening (affine x || y, flag, value, random_v): the oracle's MSMs over the parts' quotients, jac_add, to_affine"""
    fr = co.CURVE_FR[curve]
    p, L = kr.MODULI[fr], kr.LIMBS[fr]
    out = []
    for o, z in enumerate(points):
        pt = parts_of_opening(items, z, a[o], s[o] if s is not None else None, p)
        msms = []
        if pt["comb"] and pt["comb"][1]:
            assert len(pt["comb"][1]) <= len(powers)
            msms.append((powers[:len(pt["comb"][1])], pt["comb"][1]))
        if pt["rand"] and pt["rand"][1]:
            assert len(pt["rand"][1]) <= len(gpowers)
            msms.append((gpowers[:len(pt["rand"][1])], pt["rand"][1]))
        for i, (q, _) in pt["db"].items():
            off = items[i].get("shifted_offset", 0)
            assert off + len(q) <= len(spowers)
            if q:
                msms.append((spowers[off:off + len(q)], q))
        acc = None
        for bases, q in msms:
            r = co.msm(curve, 1, bases, kr.limbs_of_ints(q, L), nthreads=nthreads)
            acc = r if acc is None else co.jac_add(curve, 1, acc, r)
        value = pt["comb"][2] if pt["comb"] else 0
        rv = pt["rand"][2] if pt["rand"] else 0
        if acc is None:
            out.append((np.zeros(co.point_words(curve, 1), dtype=np.uint64), 1, value, rv))
            continue
        xy, inf = co.to_affine(curve, 1, acc)
        out.append(((np.zeros_like(xy[0]) if inf[0] else xy[0]), int(inf[0]), value, rv))
    return out


def collapse(lcs, queries, challenges, m, n_points, p):
    """Linear combinations and per-query challenges -> the two P x m coefficient tables.  lcs[j] = dict(terms=[(c, item)], bound=bool):
    `bound` says that the degree bound of the combination is enforced, and the combination is then one item with coefficient 1 (as
    upstream requires).  queries[q] = (j, point index), challenges[q] = (xi, xi_s): the combination enters its point's opening times xi,
    its degree-bound witness times xi_s (ignored without `bound`)."""
    a = [[0] * m for _ in range(n_points)]
    s = [[0] * m for _ in range(n_points)]
    for (j, o), (xi, xi_s) in zip(queries, challenges):
        lc = lcs[j]
        for c, i in lc["terms"]:
            a[o][i] = (a[o][i] + xi * c) % p
        if lc.get("bound"):
            assert len(lc["terms"]) == 1 and lc["terms"][0][0] % p == 1
            i = lc["terms"][0][1]
            s[o][i] = (s[o][i] + xi_s) % p
    return a, s
