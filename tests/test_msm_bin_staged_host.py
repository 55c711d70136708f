"""The sizing of the staged per-bin sort of the MSM partition sort (pcd_amd/csrc/msm.hip.h: msm_bin_sort_staged_kernel -- a bin of at most
MSM_BIN_STAGE_CAP entries is read once, ordered in LDS and written out in whole lines), from the constants that
tests/hostcheck/msm_bin_stage_check.hip prints -- no GPU.

Two workgroups must fit a compute unit's LDS, a lane holds a whole number of entries, and every bin of the headline MSM (bench.py: MNT4-298
G1, n = 2^20, a copy per window, c = 20, 15 windows) must fit the cap: the bin loads are recomputed here in numpy from the bench's own
scalars with the signed recoding of msm_signed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024   # MI355X
CONST = ["cap", "block", "per", "lds_bytes", "bin_shift"]
BENCH_SEED = 0x5043443031  # bench.py SEED; the headline's scalars are gen_scalars(fr, n, seed=SEED + 1000)


def bin_stage_constants(tmpdir):
    exe = os.path.join(str(tmpdir), "msm_bin_stage_check")
    src = os.path.join(ROOT, "tests", "hostcheck", "msm_bin_stage_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", src, "-o", exe])
    head = subprocess.check_output([exe], text=True).split()
    assert head[0] == "const"
    return dict(zip(CONST, (int(x) for x in head[1:])))


def bin_loads(sc, bits, c, Wg, live=None, bin_shift=9):
    """entries per bin of the partition sort for canonical scalars sc (n x N64 uint64): window w of a scalar has the signed digit of
    msm_signed (raw + carry > 2^(c-1) -> 2^c - that, carry 1), a non-zero digit d makes one entry with key ((w mod Wg) << c) | d, and the
    bin is key >> bin_shift.  Scalars equal to zero or one and bases at infinity (live[i] false) make none.  W = (bits + c) // c."""
    sc = np.ascontiguousarray(sc, dtype=np.uint64)
    n, n64 = sc.shape
    W = (bits + c) // c
    keep = (sc[:, 1:] != 0).any(axis=1) | (sc[:, 0] > 1)
    if live is not None:
        keep &= np.asarray(live, dtype=bool)
    s = sc[keep]
    carry = np.zeros(len(s), dtype=np.uint64)
    nbins = (Wg << c) >> bin_shift
    loads = np.zeros(nbins, dtype=np.int64)
    half, full, mask = np.uint64(1 << (c - 1)), np.uint64(1 << c), np.uint64((1 << c) - 1)
    for w in range(W):
        word, off = (w * c) >> 6, (w * c) & 63
        raw = s[:, word] >> np.uint64(off) if word < n64 else np.zeros(len(s), dtype=np.uint64)
        if off + c > 64 and word + 1 < n64:
            raw = raw | (s[:, word + 1] << np.uint64(64 - off))
        d = (raw & mask) + carry
        neg = d > half
        carry = neg.astype(np.uint64)
        d = np.where(neg, full - d, d)
        key = (np.uint64((w % Wg) << c) | d[d != 0]) >> np.uint64(bin_shift)
        loads += np.bincount(key.astype(np.int64), minlength=nbins)
    assert not carry.any(), "a scalar wider than the field"
    return loads


@pytest.fixture(scope="module")
def const(tmp_path_factory):
    return bin_stage_constants(tmp_path_factory.mktemp("binstage"))


def test_two_workgroups_fit_a_compute_unit(const):
    assert const["bin_shift"] == 9
    # the word buffer, the 2^bin_shift counters and a total per wave, with room for the alignment shift of up to three words
    need = 4 * (const["cap"] + 3 + (1 << const["bin_shift"]) + const["block"] // 64)
    assert need <= const["lds_bytes"] <= 78 * 1024
    assert const["lds_bytes"] % 16 == 0
    assert 2 * const["lds_bytes"] <= LDS_PER_CU


def test_cap_is_a_whole_number_of_entries_per_lane(const):
    assert const["cap"] == 18432
    assert const["cap"] % const["block"] == 0 and const["cap"] == const["block"] * const["per"]
    assert const["block"] % 64 == 0 and const["block"] <= 1024
    assert const["cap"] % 4 == 0                           # the buffer is written out in 16-byte lines
    assert const["cap"] < 1 << (32 - const["bin_shift"])   # the rank of an entry sits beside its low key bits in one word


def test_every_bin_of_the_headline_fits(co, const):
    fr = co.CURVE_FR[0]
    sc = co.gen_scalars(fr, 1 << 20, seed=BENCH_SEED + 1000)
    loads = bin_loads(sc, 298, 20, 1, bin_shift=const["bin_shift"])  # a copy per window: one bucket window
    assert len(loads) == 2048 and int((loads > 0).sum()) == 1025 and not loads[1025:].any()  # signed digits reach 2^19: bin 1024 holds that digit alone
    assert int(loads.sum()) == 15728626
    assert int(loads.max()) == 16911
    assert loads.max() <= const["cap"]
