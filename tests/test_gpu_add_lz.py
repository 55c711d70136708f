"""GPU: EC::add_lz (pcd_amd/csrc/ec.hip.h), the full addition of two lazily reduced XYZZ accumulators, against the device's plain Jacobian
EC::add for both 298-bit G1 groups under random lane masks (tests/gpucheck/add_lz_check.hip): random pairs, operands as madd_lz steps
leave them and at the upper end of the format, equal points (the doubling branch), opposite points, identities on either side and on
both, chains of 32 with the output fed back as the left and as the right operand -- each lane its own case each round, so the rare
branches run beside ordinary additions in one wave.  The harness is compiled here, into a temporary directory."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["pair", "pair'", "after madd_lz", "at the edge", "P + P", "P + (-P)", "identities", "idle", "chain left", "chain right"]


@pytest.fixture(scope="module")
def add_lz_lib(tmp_path_factory, gpu_ctx):
    # (gpu_ctx first: torch's own HIP runtime has to own the device before this library brings in the system's -- tests/conftest.py)
    so = str(tmp_path_factory.mktemp("add_lz_gpu") / "libgpucheck_add_lz.so")
    src = os.path.join(ROOT, "tests", "gpucheck", "add_lz_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", so])
    lib = C.CDLL(so)
    lib.gc_add_lz_check.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_add_lz_equals_plain_add_under_masks(add_lz_lib, which):
    for seed in (2026, 31337):
        out = np.zeros(21, dtype=np.uint32)
        rc = add_lz_lib.gc_add_lz_check(which, 48, seed, out.ctypes.data_as(C.c_void_p))
        assert rc == 0
        assert out[20] == 8 * 64, "the check kernel did not run to the end in every lane"
        ran = {n: int(v) for n, v in zip(CASES, out[10:20])}
        assert all(v > 0 for n, v in ran.items() if n != "idle"), ran
        assert not out[:10].any(), {n: int(v) for n, v in zip(CASES, out[:10]) if v}
