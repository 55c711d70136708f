"""CPU: the field arithmetic of pcd_amd/csrc/fp.hip.h and the lazily reduced addition steps of ec.hip.h, operation by operation on raw
limb images, compiled for the HOST (tests/hostcheck/hostcheck.hip, 128-bit column check on) and checked against Python integers only
(tests/field_reference.py): operands at the representatives and limb patterns the code's own comments declare -- 0, p, 2p - 1, the
undecidable band of the two-top-limb add / sub estimate, every Lz operand role of madd_lz / madd_x_lz2 at the top and bottom of its
interval, accumulators lifted to upper representatives.  tests/test_gpu_field_ops.py runs the same case lists on the gfx950 build.
madd_x_lz2 exists for Fq2 of the 298-bit curves only, i.e. G2 of curve 0; the LDS-resident madd_lz_st (PCD_ACC_LDS, off) is not covered.

What inv_gcd's cases do NOT pin: the NUMBER of divstep batches.  BATCHES comes from the Bernstein-Yang worst-case bound
(49 bits + 57) / 17; with one batch fewer every case here still passes (tried; no operand is known that needs the last batch, and
none was searched for beyond these lists), so a change of that count is not caught by this file.  The steps per batch (28), the
transition-matrix arithmetic and the final R'^3 product are: 27 steps per batch fails inv_gcd on the first field."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_reference as fr  # noqa: E402
from test_hostcheck import hc  # noqa: E402,F401  (the fixture that builds and loads the host harness)

VARIANTS = [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (3, 1)]   # (field, variant): 0 inlined products, 1 mul_call / sqr_call bodies (753 bits)


@pytest.fixture(scope="module")
def be(hc):  # noqa: F811
    return fr.Backend(hc, "hc")


@pytest.mark.parametrize("name", sorted(fr.FIELD_OPS))
@pytest.mark.parametrize("fid,variant", VARIANTS)
def test_field_op(be, fid, variant, name):
    assert fr.check_field_op(be, fid, variant, name) > 0


@pytest.mark.parametrize("fid", [0, 1])
def test_lz_products_at_their_bounds(be, fid):
    counts = fr.check_lz_products(be, fid)
    assert all(counts[op] > 0 for op in (fr.L_MUL, fr.L_SQR, fr.L_DOT2, fr.L_DOT4))


def test_lz_cases_reach_the_stated_weights():
    """the case lists really contain operands at the sums the comments state: 116 (madd_lz Y3), 648 (PP.c0), 792 (Y3.c0), 1024 (global)"""
    fld = fr.FLD[0]
    cases = fr.lz_product_cases(0)
    top = lambda op, lo, hi: max(w for w in (fr.lz_value_weight(fld, ops) for ops in cases[op]) if lo < w <= hi)
    assert 115.9 < top(fr.L_DOT2, 0, 116)
    assert 647.9 < top(fr.L_DOT2, 116, 648)
    assert 791.9 < top(fr.L_DOT4, 0, 792)
    assert 1023.9 < top(fr.L_MUL, 0, 1024)
    # t = Q - X3 + 16p limb-wise, "limbs in (-2^28, 1.25 2^30)": both ends are attained for the limbs of 16p this field has
    m16 = [4 * w for w in fr.limbs(4 * fld.p, fld.N)[:-1]]
    low = [w for ops in cases[fr.L_DOT2][:200] for w in ops[1][:-1]]
    assert min(low) == min(m16) - fr.MASK and max(low) == max(m16) + fr.MASK
    assert -(1 << 28) < min(low) < 0 and (1 << 30) < max(low) < (5 << 28)


@pytest.mark.parametrize("fid", [0, 1])
def test_lz_limb_forms(be, fid):
    assert fr.check_lz_forms(be, fid) > 0


@pytest.mark.parametrize("name", ["mul", "sqr", "inv"])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_tower_op(be, fid, name):
    assert fr.check_tower_op(be, fid, name) > 0


# madd_lz: G1 of curves 0 and 1.  madd_x (what the accumulation calls): on curve 0 G2 is Fq2 and madd_x IS madd_x_lz2 -- the only place the
# product has it (LazyFq2 exists for Fp2 alone); on curve 1 G2 is Fq3 and madd_x is madd_x_plain.  madd_x_plain on G1 and on curve 0's G2
# for comparison.  Not covered: EC::madd_lz_st, the LDS-resident form of madd_lz behind PCD_ACC_LDS (an experiment, off by default).
STEP_CASES = [pytest.param(0, 1, fr.S_MADD_LZ, id="madd_lz-c0-G1"), pytest.param(1, 1, fr.S_MADD_LZ, id="madd_lz-c1-G1"),
              pytest.param(0, 2, fr.S_MADD_X, id="madd_x_lz2-c0-G2"), pytest.param(1, 2, fr.S_MADD_X, id="madd_x(plain)-c1-G2-Fq3"),
              pytest.param(0, 1, fr.S_MADD_X_PLAIN, id="madd_x_plain-c0-G1"), pytest.param(1, 1, fr.S_MADD_X_PLAIN, id="madd_x_plain-c1-G1"),
              pytest.param(0, 2, fr.S_MADD_X_PLAIN, id="madd_x_plain-c0-G2")]


@pytest.mark.parametrize("cid,grp,op", STEP_CASES)
def test_accumulator_step_from_lifted_coordinates(be, cid, grp, op):
    assert fr.check_steps(be, cid, grp, op) > 0
