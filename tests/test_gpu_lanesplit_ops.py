"""GPU: the lane-split extension fields of pcd_amd/csrc/fp.hip.h (Fp2S: two lanes per element, Fp3S: three; plain and LDS-mailbox) and
the group law of ec.hip.h in them -- the forms the bucket accumulation, the tail kernels and the single-item kernels of five of the
eight groups compute in, and which exist in the gfx950 build only -- one operation per item on raw limb images
(tests/gpucheck/lanesplit_check.hip) against Python integers only (tests/field_reference.py).  Every case list runs under three
active-item masks (all items, every third item off, a seeded random half off: the collective operations then run under a ragged exec
mask) and once more as one item alone; the lanes that ran are counted, and an inactive item's output must keep the sentinel.
Operands: the representatives and limb patterns of tower_cases drawn per coefficient, exactly one coefficient 0 or p for the zero tests,
accumulators and Jacobian operands with every coordinate on c and on c + p, against a generic point, the same point, its negative and
the identity (tests/test_lanesplit_reference_host.py pins these lists against the C++ oracle without a GPU)."""
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
SPLIT = list(range(len(fr.SPLIT_NAMES)))


def _lib():
    so = os.path.join(GC, "libgpucheck_ls.so")
    # built by __graft_entry__.build(); only a missing library is built here (see tests/test_gpu_mailbox.py)
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", GC, "libgpucheck_ls.so"], stdout=subprocess.DEVNULL)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def sb():
    return fr.SplitBackend(_lib())


@pytest.mark.parametrize("name", fr.SPLIT_TOWER_OPS)
@pytest.mark.parametrize("sid", SPLIT, ids=fr.SPLIT_NAMES)
def test_split_tower_op(sb, sid, name):
    assert fr.check_split_tower_op(sb, sid, name) > 0


# S_MADD_X is EC::madd_x = madd_x_plain in these types (what the accumulation of the MNT6-298 and MNT4-753 G2 runs), S_MADD_JAC EC::madd (the
# accumulation of the MNT6-753 G2); J_ADD / J_DBL are what the tail and the single-item kernels run in all of them
@pytest.mark.parametrize("name", fr.SPLIT_GROUP_OPS)
@pytest.mark.parametrize("sid", SPLIT, ids=fr.SPLIT_NAMES)
def test_split_group_op(sb, sid, name):
    assert fr.check_split_group_op(sb, sid, name) > 0
