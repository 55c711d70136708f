"""GPU: the gfx950 build of the field arithmetic of pcd_amd/csrc/fp.hip.h -- with the device-only parts the host build does not have:
the always-true assumes that keep the column sums one multiply-add chain, the LDS mailbox of mb_mul / mb_sqr, the non-inlined mul_call /
sqr_call bodies of the 753-bit fields -- and of the lazily reduced addition steps of ec.hip.h, operation by operation on raw limb images
(tests/gpucheck/fieldops_check.hip, one element per lane, partly filled waves included) against Python integers only.  The case lists
are those of tests/test_field_ops_host.py (tests/field_reference.py): the representatives and limb patterns the code's comments declare."""
import ctypes as C
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GC = os.path.join(ROOT, "tests", "gpucheck")
# (field, variant): 0 inlined products, 1 mul_call / sqr_call bodies, 2 LDS mailbox (the last two: what the 753-bit kernels run)
VARIANTS = [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2)]


def _lib():
    so = os.path.join(GC, "libgpucheck_fp.so")
    # built by __graft_entry__.build(); only a missing library is built here (see tests/test_gpu_mailbox.py)
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", GC, "libgpucheck_fp.so"], stdout=subprocess.DEVNULL)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def be():
    return fr.Backend(_lib(), "gc")


@pytest.mark.parametrize("name", sorted(fr.FIELD_OPS))
@pytest.mark.parametrize("fid,variant", VARIANTS)
def test_field_op(be, fid, variant, name):
    assert fr.check_field_op(be, fid, variant, name) > 0


@pytest.mark.parametrize("fid", [0, 1])
def test_lz_products_at_their_bounds(be, fid):
    counts = fr.check_lz_products(be, fid)
    assert all(counts[op] > 0 for op in (fr.L_MUL, fr.L_SQR, fr.L_DOT2, fr.L_DOT4))


@pytest.mark.parametrize("fid", [0, 1])
def test_lz_limb_forms(be, fid):
    assert fr.check_lz_forms(be, fid) > 0


@pytest.mark.parametrize("name", ["mul", "sqr", "inv"])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_tower_op(be, fid, name):
    assert fr.check_tower_op(be, fid, name) > 0


# Which types the kernels instantiate (ec.hip.h AccOf / SplitOfTail, msm.hip.h MsmUseXyzz), and where each is compared with integers:
#   madd_lz: the accumulation of G1 on curves 0 and 1.                                             here
#   madd_x = madd_x_lz2 on the unsplit Fq2 of curve 0 (LazyFq2 exists for Fp2 alone): its G2 accumulation.   here
#   curve 1's G2 (Fq3) accumulates with madd_x_plain in the LANE-SPLIT G2Cfg3S<F298B, .., true>, three lanes per point: the kernels never
#   instantiate the unsplit G2_MNT6_298 that "madd_x(plain)-c1-G2-Fq3" runs.  That case stays as a check of the formula on the unsplit
#   tower; its split counterpart is test_split_fq3_accumulation_step below (tests/gpucheck/lanesplit_check.hip), and all the lane-split
#   groups, plain and mailbox, are in tests/test_gpu_lanesplit_ops.py.
#   G1 of curves 2 and 3 accumulates with EC<G1CfgMB>::madd on a Jacobian record (mailbox field): madd-c2-G1-mailbox, madd-c3-G1-mailbox;
#   madd_x_plain in the same type is the PCD_XYZZ_753 form.
#   madd_x_plain on G1 of curves 0 / 1 and on curve 0's unsplit G2: for comparison.
# Not covered: EC::madd_lz_st, the LDS-resident form of madd_lz behind PCD_ACC_LDS (an experiment, off by default).
STEP_CASES = [pytest.param(0, 1, fr.S_MADD_LZ, id="madd_lz-c0-G1"), pytest.param(1, 1, fr.S_MADD_LZ, id="madd_lz-c1-G1"),
              pytest.param(0, 2, fr.S_MADD_X, id="madd_x_lz2-c0-G2"), pytest.param(1, 2, fr.S_MADD_X, id="madd_x(plain)-c1-G2-Fq3"),
              pytest.param(0, 1, fr.S_MADD_X_PLAIN, id="madd_x_plain-c0-G1"), pytest.param(1, 1, fr.S_MADD_X_PLAIN, id="madd_x_plain-c1-G1"),
              pytest.param(0, 2, fr.S_MADD_X_PLAIN, id="madd_x_plain-c0-G2"),
              pytest.param(2, 1, fr.S_MADD_JAC, id="madd-c2-G1-mailbox"), pytest.param(3, 1, fr.S_MADD_JAC, id="madd-c3-G1-mailbox"),
              pytest.param(2, 1, fr.S_MADD_X_PLAIN, id="madd_x_plain-c2-G1-mailbox"),
              pytest.param(3, 1, fr.S_MADD_X_PLAIN, id="madd_x_plain-c3-G1-mailbox")]


@pytest.mark.parametrize("cid,grp,op", STEP_CASES)
def test_accumulator_step_from_lifted_coordinates(be, cid, grp, op):
    assert fr.check_steps(be, cid, grp, op) > 0


def test_split_fq3_accumulation_step():
    """the split counterpart of madd_x(plain)-c1-G2-Fq3: the same case list in G2Cfg3S<F298B, .., true>, the type the kernels run"""
    import test_gpu_lanesplit_ops as ls
    assert fr.check_split_group_op(fr.SplitBackend(ls._lib()), 1, "S_MADD_X") > 0
