"""EC::add_lz (pcd_amd/csrc/ec.hip.h) -- the full addition of two lazily reduced XYZZ accumulators, what the MSM's edge pass and first
reduction level sum flushed records with -- compiled for the HOST by tests/hostcheck/add_lz_check.hip with the 128-bit column check on, on
curve points from the oracle, for both 298-bit G1 groups: 4 032 random pairs against the Jacobian EC::add on the affine image, the
identity on either side and on both, P + P, P + (-P), operands as a chain of madd_lz steps leaves them and pushed to the upper end of the
format (X just below 16p, Y / ZZ / ZZZ in [p, 2p)), chains of 32 additions with the output fed back as the left and as the right operand,
and the running sums of the first reduction level with empty buckets in between.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 64


@pytest.fixture(scope="module")
def add_lz_check(tmp_path_factory):
    out = tmp_path_factory.mktemp("add_lz")
    exe = str(out / "add_lz_check")
    src = os.path.join(ROOT, "tests", "hostcheck", "add_lz_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-DPCD_LZ_CHECK", src, "-o", exe])
    return exe, out


@pytest.mark.parametrize("cid", [0, 1])
def test_add_lz_equals_jacobian_add_on_host(co, add_lz_check, cid):
    exe, out = add_lz_check
    pts = co.gen_points(cid, 1, N_POINTS, seed=7300 + cid)
    path = str(out / f"points{cid}.bin")
    pts.tofile(path)
    r = subprocess.run([exe, str(cid), path, str(N_POINTS)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)   # (an abort here is a column sum that left 64 bits)
    word, checks, bad = r.stdout.split()
    assert word == "ok" and int(bad) == 0
    assert int(checks) >= N_POINTS * (N_POINTS - 1) + 7 * N_POINTS + 400, checks
