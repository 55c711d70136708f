"""The batched short MSM (pcdhip_msm_short_batch / _dev, pcdhip_kzg_commit_last_plan) through the layers that need no GPU: the header, the
library's exports, the Python and Rust bindings, and the host-side planner of the launch chain (msm_short_batch_plan, compiled for the host
by tests/hostcheck/msm_short_batch_plan_check.hip) over every list of up to three sizes around its thresholds."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_rust_boundary as crb  # noqa: E402

NAMES = ["pcdhip_msm_short_batch", "pcdhip_msm_short_batch_dev", "pcdhip_kzg_commit_last_plan"]
E_PER_ITEM = 4   # MSM_SHORT_E: candidates per item of a plane's workgroup


def test_header_declares_the_three_functions_and_the_struct():
    text = open(os.path.join(ROOT, "include", "pcdhip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*pcdhip_ctx\s*\*", text), name
    protos, structs = crb.c_prototypes()
    assert structs.get("pcdhip_msm_short_item") == ["u64", "u64", "u64"]
    assert protos.get("pcdhip_msm_short_batch") == ("i32", ["ptr", "ptr", "ptr", "usize", "ptr", "usize", "ptr"])
    assert protos.get("pcdhip_msm_short_batch_dev") == ("i32", ["ptr", "ptr", "ptr", "ptr", "usize", "ptr"])
    assert protos.get("pcdhip_kzg_commit_last_plan") == ("i32", ["ptr", "ptr"])


def test_library_exports_and_binding_list():
    from pcd_amd import capi
    lib = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
    assert C.sizeof(capi.MsmShortItem) == 24


def test_null_context_is_an_argument_error():
    from pcd_amd import capi
    lib = capi.lib()
    out = (C.c_uint64 * 64)()
    item = (capi.MsmShortItem * 1)()
    z = C.c_size_t(0)
    assert lib.pcdhip_msm_short_batch(None, None, None, z, item, C.c_size_t(1), out) == -1
    assert lib.pcdhip_msm_short_batch(None, None, None, z, None, z, None) == -1
    assert lib.pcdhip_msm_short_batch_dev(None, None, None, item, C.c_size_t(1), out) == -1
    assert lib.pcdhip_kzg_commit_last_plan(None, out) == -1


def test_context_has_both_methods():
    from pcd_amd import capi
    assert callable(getattr(capi.Context, "msm_short_batch", None))
    assert callable(getattr(capi.Context, "kzg_commit_last_plan", None))


def test_rust_boundary_matches_the_header():
    fns, rstructs = crb.rust_externs()
    protos, structs = crb.c_prototypes()
    for name in NAMES:
        assert fns.get(name) == protos[name], name
    assert rstructs.get("pcdhip_msm_short_item") == structs["pcdhip_msm_short_item"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_boundary.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "msm_short_batch_plan_check")
    src = os.path.join(ROOT, "tests", "hostcheck", "msm_short_batch_plan_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", src, "-o", exe])

    def run(per_wave, groups, ns):
        out = subprocess.check_output([exe, str(per_wave), str(groups)] + [str(n) for n in ns], text=True)
        plan, items, entries, part_item, fold_item = None, [], [], None, None
        for line in out.strip().splitlines():
            tag, *rest = line.split()
            vals = [int(x) for x in rest]
            if tag == "plan":
                plan = dict(zip(["span", "entries", "parts", "folds", "err_words", "table_words", "scratch_words", "jac_words"], vals))
            elif tag == "item":
                items.append(vals)
            elif tag == "entry":
                entries.append(dict(zip(["e", "offset", "n", "part0", "parts", "row0", "out_slot", "scalars"], vals)))
            elif tag == "part_item":
                part_item = vals
            elif tag == "fold_item":
                fold_item = vals
        return plan, items, entries, part_item, fold_item
    return run


SIZES = (0, 1, 84, 85, 256, 257, 1024)


@pytest.mark.parametrize("groups", (1, 50))
@pytest.mark.parametrize("per_wave", (64, 32, 21))
def test_plan_of_every_short_list(plan_check, per_wave, groups):
    """every (item, part) exactly once in the part list, the sum of parts equal to msm_short_plan's per item, scratch ranges disjoint and
    inside scratch_words, nothing owned by an item with n == 0 -- for every list of up to three sizes around the thresholds (84 / 85: one
    and two parts of a 21-item wave without copies; 256 / 257: of a 64-item one)"""
    per_wg = per_wave * E_PER_ITEM
    lists = [ns for L in range(0, 4) for ns in itertools.product(SIZES, repeat=L)]
    assert len(lists) == 1 + 7 + 49 + 343
    for ns in lists:
        plan, items, entries, part_item, fold_item = plan_check(per_wave, groups, ns)
        tag = (per_wave, groups, ns)
        assert [it[1] for it in items] == list(ns), tag
        # msm_short_plan's own value per item, and the rule it states: ceil(n * groups / (items of a wave * E)), at least one
        for (j, n, single) in items:
            assert single == (max(1, -(-n * groups // per_wg)) if n else 0), tag
        live = [(j, n, single) for (j, n, single) in items if n]
        assert plan["entries"] == len(live) == len(entries), tag
        assert plan["parts"] == sum(s for _, _, s in live) == len(part_item), tag
        assert plan["span"] == (8 if groups > 1 else 298), tag
        # entries in item order, each carrying its item's fields (offset j, slot 100 + j, pointer 4096 (j + 1)); n == 0 items own none
        for ent, (j, n, single) in zip(entries, live):
            assert (ent["offset"], ent["n"], ent["out_slot"], ent["scalars"], ent["parts"]) == (j, n, 100 + j, 4096 * (j + 1), single), tag
        # every (entry, part) exactly once: entry e owns the contiguous range part0 .. part0 + parts of the part list
        seen = set()
        for x, e in enumerate(part_item):
            ent = entries[e]
            assert ent["part0"] <= x < ent["part0"] + ent["parts"], tag
            seen.add((e, x - ent["part0"]))
        assert len(seen) == len(part_item) == sum(ent["parts"] for ent in entries), tag
        assert seen == {(ent["e"], p) for ent in entries for p in range(ent["parts"])}, tag
        assert fold_item == [ent["e"] for ent in entries if ent["parts"] > 1] and plan["folds"] == len(fold_item), tag
        # scratch: error words (the call's, one per entry, one per part) | table | rows; row ranges disjoint, in order, inside the rows
        assert plan["err_words"] >= 1 + plan["entries"] + plan["parts"], tag
        assert plan["table_words"] >= 8 * plan["entries"] + plan["parts"] + plan["folds"], tag
        rows_total = plan["span"] * plan["parts"]
        assert plan["scratch_words"] == plan["err_words"] + plan["table_words"] + rows_total * plan["jac_words"], tag
        end = 0
        for ent in entries:
            assert ent["row0"] == end, tag
            end = ent["row0"] + plan["span"] * ent["parts"]
        assert end == rows_total, tag
