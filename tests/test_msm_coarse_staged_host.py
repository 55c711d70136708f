"""The tile rule of the staged write pass of the MSM partition sort (pcd_amd/csrc/msm.hip.h: msm_stage_tile), compiled for the host by
tests/hostcheck/msm_stage_tile_check.hip and evaluated for every W = 1 .. 64 and nbins = 1, 2, 4 .. 8192 -- no GPU.

What the rule promises, restated here from the constants the program prints and not from its answers: the tile is the largest power of two
in [tile_min, tile_max] whose LDS footprint (4 B x tile x W for the word buffer plus three arrays over the bins and the total) fits the
budget, provided a (tile, bin) run then holds min_run entries on average; otherwise 0, and msm_run launches the direct write pass."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024   # MI355X
CONST = ["budget", "tile_min", "tile_max", "w_max", "min_run", "bin_shift", "sign_at", "g_at", "g_bits", "idx_at", "idx_bits"]


def build_tile_check(tmpdir):
    exe = os.path.join(str(tmpdir), "msm_stage_tile_check")
    src = os.path.join(ROOT, "tests", "hostcheck", "msm_stage_tile_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", src, "-o", exe])
    return exe


def run_tile_check(exe, pairs=()):
    """(constants, {(W, nbins): (tile, lds_bytes)})"""
    out = subprocess.check_output([exe] + [str(v) for p in pairs for v in p], text=True).strip().splitlines()
    head = out[0].split()
    assert head[0] == "const"
    const = dict(zip(CONST, (int(x) for x in head[1:])))
    table = {}
    for ln in out[1:]:
        W, nbins, tile, lds = (int(x) for x in ln.split())
        table[(W, nbins)] = (tile, lds)
    return const, table


def footprint(tile, W, nbins):
    return 4 * (tile * W + 3 * nbins + 4)


def expected_tile(const, W, nbins):
    if not (1 <= W <= const["w_max"]) or nbins < 1:
        return 0
    t = const["tile_max"]
    while t >= const["tile_min"]:
        if footprint(t, W, nbins) <= const["budget"]:
            return t if t * W >= const["min_run"] * nbins else 0
        t //= 2
    return 0


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = build_tile_check(tmp_path_factory.mktemp("stage"))
    const, table = run_tile_check(exe)
    return exe, const, table


def test_constants_and_staged_word(rule):
    _, c, _ = rule
    assert c["tile_min"] == 256 and c["tile_max"] == 2048 and c["bin_shift"] == 9
    # the budget leaves room on the CU for the kernel's static arrays; at least the headline shape (2 048 x 15 words, 2 048 bins) fits it
    assert footprint(2048, 15, 2048) <= c["budget"] <= LDS_PER_CU - 4096
    # fields of the staged word: low key bits | sign | group | index inside the tile -- disjoint, in order, inside 32 bits, and wide enough
    assert c["sign_at"] == c["bin_shift"] and c["g_at"] == c["sign_at"] + 1 and c["idx_at"] == c["g_at"] + c["g_bits"]
    assert c["idx_at"] + c["idx_bits"] <= 32
    assert (1 << c["idx_bits"]) >= c["tile_max"]      # the largest local scalar index is tile_max - 1
    assert (1 << c["g_bits"]) >= c["w_max"]           # the largest group is W - 1


def test_rule_over_every_shape(rule):
    _, c, table = rule
    shapes = [(W, 1 << k) for W in range(1, 65) for k in range(0, 14)]
    assert sorted(table) == sorted(shapes)
    none_fits = 0
    for (W, nbins) in shapes:
        tile, lds = table[(W, nbins)]
        want = expected_tile(c, W, nbins)
        assert tile == want, (W, nbins, tile, want)
        if tile:
            assert tile in (256, 512, 1024, 2048)
            assert lds == footprint(tile, W, nbins) <= c["budget"], (W, nbins)
            assert (tile << c["idx_at"]) <= 1 << 32 and W - 1 < (1 << c["g_bits"])
            # the largest: the next power of two does not fit (or is beyond tile_max)
            assert tile == c["tile_max"] or footprint(2 * tile, W, nbins) > c["budget"], (W, nbins)
            assert tile * W >= c["min_run"] * nbins
        else:
            none_fits += 1
            # exactly when the smallest tile is over the budget, or the largest one that fits leaves runs shorter than min_run
            fits = [t for t in (2048, 1024, 512, 256) if footprint(t, W, nbins) <= c["budget"]]
            assert not fits or fits[0] * W < c["min_run"] * nbins, (W, nbins)
    assert 0 < none_fits < len(shapes)
    # the shapes the design names: the headline takes the largest tile, 8 192 bins and a 753-bit field's 42 windows at 1 024 bins do as stated
    assert table[(15, 1024)][0] == 2048 and table[(15, 2048)][0] == 2048
    assert table[(42, 1024)][0] == 512
    assert table[(15, 8192)][0] == 0


def test_rule_outside_its_domain(rule):
    exe, c, _ = rule
    _, t = run_tile_check(exe, [(0, 16), (65, 16), (15, 0), (64, 1), (15, 960), (19, 2432), (18, 4608)])
    assert t[(0, 16)][0] == 0 and t[(65, 16)][0] == 0 and t[(15, 0)][0] == 0
    assert t[(64, 1)][0] == 512            # 4 x 512 x 64 = 128 KiB fits, 256 KiB does not
    assert t[(15, 960)][0] == 2048
    assert t[(19, 2432)][0] == 1024        # runs of exactly min_run entries: still staged
    assert t[(18, 4608)][0] == 0           # runs of four entries: direct
