"""CPU: the K12 entry points (the second sumcheck's q and its driver) as the header declares them, their argument checks without a
device, the exact-integer reference the GPU tests compare against (tests/marlin_sumcheck2_reference.py) checked against itself -- the
h_2 identity at a random point with a(z) and b(z) from the definition, a zero remainder, |K| sigma = sum_K f -- and the kernel's
element function marlin_sumcheck2_element compiled for the host (tests/hostcheck/marlin_sumcheck2_check.hip) against that reference,
word for word, for all four fields."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import marlin_index_reference as mir  # noqa: E402
import marlin_reference as mr  # noqa: E402
import marlin_sumcheck2_reference as m2  # noqa: E402

K12 = {
    "pcdhip_marlin_sumcheck2_q": ("i32", ["ptr"] * 9 + ["usize", "ptr"]),
    "pcdhip_marlin_sumcheck2": ("i32", ["ptr"] * 5 + ["i32"] + ["ptr"] * 6),
}


def test_prototypes_exports_and_rust_declarations():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    rust, _ = crb.rust_externs()
    lib = capi.lib()
    for name, sig in K12.items():
        assert protos.get(name) == sig, name
        assert rust.get(name) == sig, name
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name
    assert not crb.check_ffi()[0]
    assert hasattr(capi.Context, "marlin_sumcheck2_q") and hasattr(capi.Context, "marlin_sumcheck2")


def test_null_arguments_are_argument_errors():
    from pcd_amd import capi
    lib = capi.lib()
    E_ARG = -1
    lens = (C.c_size_t * 3)(7, 7, 7)
    assert lib.pcdhip_marlin_sumcheck2_q(None, None, None, None, None, None, None, None, None, 0, None) == E_ARG
    assert lib.pcdhip_marlin_sumcheck2(None, None, None, None, None, 0, None, None, None, None, None, lens) == E_ARG
    assert list(lens) == [7, 7, 7]


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_reference_second_sumcheck(field):
    from oracle import coracle as co
    rnd = random.Random(1200 + field)
    p = mr.MODULI[field]
    h_n, x_n, k_n, b_n = 16, 4, 64, 256
    rows, cols = 14, 16
    dom_h, dom_k, dom_b = (mr.domain_elements(co, field, n) for n in (h_n, k_n, b_n))
    mats = [[(rnd.randrange(rows), rnd.randrange(cols), rnd.choice([1, p - 1, 2, 0, rnd.randrange(p)])) for _ in range(n)] for n in (64, 41, 57)]
    mats[1].append(mats[1][0])  # a duplicated (r, c)
    alpha, beta = rnd.randrange(p), rnd.randrange(p)
    assert pow(alpha, h_n, p) != 1 and pow(beta, h_n, p) != 1  # outside H: no d_M vanishes on K
    coeff = [rnd.randrange(1, p) for _ in range(3)]
    per_matrix = [mir.arithmetize(m, dom_h, h_n, x_n, k_n, p) for m in mats]
    on_k = tuple([per_matrix[m][q] for m in range(3)] for q in range(4))
    sc = m2.sumcheck2(alpha, beta, coeff, on_k, dom_k, dom_b, p)
    assert [len(sc[k]) for k in ("f_poly", "g2", "a_poly", "b_poly", "q", "h2", "rem")] == [k_n, k_n - 1, 3 * k_n - 2, 3 * k_n - 2, 4 * k_n - 3,
                                                                                           3 * k_n - 3, k_n]
    assert sc["rem"] == [0] * k_n and any(sc["h2"]) and any(sc["g2"])
    assert k_n * sc["sigma"] % p == sum(sc["f_evals"]) % p
    assert [sc["sigma"]] + sc["g2"] == sc["f_poly"]
    z = rnd.randrange(p)
    a_z, b_z = m2.ab_at(alpha, beta, coeff, sc["polys"], z, p)
    assert (a_z, b_z) == (mr.horner(sc["a_poly"], z, p), mr.horner(sc["b_poly"], z, p))
    assert mr.horner(sc["h2"], z, p) * (pow(z, k_n, p) - 1) % p == (a_z - b_z * mr.horner(sc["f_poly"], z, p)) % p
    # q on B is the pointwise formula over the B-evaluations
    on_b = [[m2.evaluate(c, dom_b, p) for c in vecs] for vecs in sc["polys"]]
    assert on_b[2][0] != [r * c % p for r, c in zip(on_b[0][0], on_b[1][0])]  # on B row_col is not the pointwise product
    q_b = m2.sumcheck2_q(alpha, beta, coeff, *on_b, m2.evaluate(sc["f_poly"], dom_b, p), p)
    assert q_b == m2.evaluate(sc["q"], dom_b, p)
    # alpha in H: a d_M vanishes on K, f drops to 0 there and the remainder shows it
    bad = m2.sumcheck2(dom_h[3], beta, coeff, on_k, dom_k, dom_b, p)
    assert any(bad["rem"])


# ---------------------------------------------------------------------------------------------- the element function on the host
def planted_cases(rnd, p):
    """(name, alpha, beta, coeff, row, col, row_col, val, f): row_col is NOT row col, so that the four-term form is what gets checked"""
    n = 6
    vec3 = lambda: [[rnd.randrange(p) for _ in range(n)] for _ in range(3)]
    const3 = lambda x: [[x] * n for _ in range(3)]
    out = []
    alpha, beta, coeff = rnd.randrange(p), rnd.randrange(p), [rnd.randrange(p) for _ in range(3)]
    out.append(("random", alpha, beta, coeff, vec3(), vec3(), vec3(), vec3(), [rnd.randrange(p) for _ in range(n)]))
    out.append(("zeros", 0, 0, [0, 0, 0], const3(0), const3(0), const3(0), const3(0), [0] * n))
    out.append(("p-1", p - 1, p - 1, [p - 1] * 3, const3(p - 1), const3(p - 1), const3(p - 1), const3(p - 1), [p - 1] * n))
    # d_A = 0 in both forms: row_A = beta for the product form, row_col_A = -(alpha beta - alpha row_A - beta col_A) for the other
    row, col, rc = vec3(), vec3(), vec3()
    row[0] = [beta] * n
    rc[0] = [(-(alpha * beta - alpha * r - beta * c)) % p for r, c in zip(row[0], col[0])]
    out.append(("d_A=0", alpha, beta, coeff, row, col, rc, vec3(), [rnd.randrange(p) for _ in range(n)]))
    out.append(("f=0", alpha, beta, coeff, vec3(), vec3(), vec3(), vec3(), [0] * n))
    return out


@pytest.fixture(scope="module")
def sumcheck2_check(tmp_path_factory):
    out = tmp_path_factory.mktemp("marlin_sumcheck2")
    exe = str(out / "marlin_sumcheck2_check")
    src = os.path.join(ROOT, "tests", "hostcheck", "marlin_sumcheck2_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", src, "-o", exe])
    return exe, out


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_element_function_on_host(sumcheck2_check, field):
    from oracle import coracle as co
    exe, out = sumcheck2_check
    rnd = random.Random(1210 + field)
    p, L = mr.MODULI[field], mr.LIMBS[field]
    mont = lambda ints: mr.to_mont(co, field, ints).reshape(len(ints), L)
    want, blobs = [], []
    for name, alpha, beta, coeff, row, col, rc, val, f in planted_cases(rnd, p):
        for have_rc in (1, 0):
            q = m2.sumcheck2_q(alpha, beta, coeff, row, col, rc if have_rc else None, val, f, p)
            if name == "d_A=0":
                assert m2.sumcheck_ab(alpha, beta, coeff, row, col, rc if have_rc else None, val, p)[1] == [0] * len(f)
            want.append((name, have_rc, mont(q)))
            blobs.append(np.array([len(f), have_rc], dtype=np.uint64).tobytes())
            blobs.append(mont([alpha, beta] + coeff).tobytes())
            blobs += [mont(v).tobytes() for v in row + col + rc + val + [f]]
    cases, result = str(out / f"cases{field}.bin"), str(out / f"q{field}.bin")
    with open(cases, "wb") as fh:
        fh.write(b"".join(blobs))
    r = subprocess.run([exe, str(field), cases, result], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.split() == ["ok", str(len(want)), str(sum(w.shape[0] for _, _, w in want))]
    got = np.fromfile(result, dtype=np.uint64).reshape(-1, L)
    at = 0
    for name, have_rc, w in want:
        assert np.array_equal(got[at:at + w.shape[0]], w), (field, name, have_rc)
        at += w.shape[0]
    assert at == got.shape[0]
