"""CPU: the size decisions of the flank stage (hipstr_amd/csrc/flank_layout.h) through hipstr_debug_flank_plan: which task the device
assembles and which one leaves it for the host twin, at each cap and one past it.  The caps of a call are the compiled limits or smaller
ones from HIPSTR_DEBUG_FLANK_CAPS ("edges,nodes,recs,reads,len,path_len"), read per call."""
import os
import re

import pytest

from hipstr_amd import capi
import flank_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("edges", "nodes", "recs", "reads", "len", "path_len")
LIMIT = dict(edges="HS_FLK_MAX_EDGES", nodes="HS_FLK_MAX_NODES", recs="HS_FLK_MAX_RECS", reads="HS_FLK_MAX_READS", len="HS_FLK_MAX_LEN", path_len="HS_FLK_MAX_PATH_LEN")
FLAG = dict(edges="edges", nodes="nodes", recs="recs", reads="reads", len="len", path_len="len")


@pytest.fixture(scope="module")
def lib():
    return capi.load_hmm()


@pytest.fixture(scope="module")
def unit():
    return fc.build(fc.unit_loci())


def plan(lib, c, caps=None, **kw):
    old = os.environ.pop("HIPSTR_DEBUG_FLANK_CAPS", None)
    try:
        if caps is not None:
            os.environ["HIPSTR_DEBUG_FLANK_CAPS"] = ",".join(str(int(caps.get(k, 0))) for k in ORDER)
        return capi.flank_plan(lib, trace=c.trace, **fc.args(c, **kw))
    finally:
        os.environ.pop("HIPSTR_DEBUG_FLANK_CAPS", None)
        if old is not None:
            os.environ["HIPSTR_DEBUG_FLANK_CAPS"] = old


def rows(p):
    return [dict(zip(p["fields"], r)) for r in p["tasks"]]


def test_thresholds_are_the_headers(lib, unit):
    p = plan(lib, unit)
    with open(os.path.join(ROOT, "hipstr_amd", "csrc", "flank_layout.h")) as f:
        text = f.read()
    for name, value in p["thresholds"].items():
        if name == "lds_bytes":
            assert value <= 65536
            continue
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == value, name
    assert p["caps"] == {k: p["thresholds"][LIMIT[k]] for k in ORDER}
    assert p["thresholds"]["HS_FLK_MAX_EDGES"] * 2 <= p["thresholds"]["HS_FLK_EDGE_SLOTS"] and p["thresholds"]["HS_FLK_MAX_NODES"] * 2 <= p["thresholds"]["HS_FLK_NODE_SLOTS"]
    assert p["peel_rounds"] == p["caps"]["nodes"] + 2 and p["workgroups"] == len(p["tasks"]) == 2 * int(unit.samp_off[-1])
    # a cap above the compiled limit, or below 1, is clamped
    q = plan(lib, unit, caps=dict(edges=10 ** 9, nodes=-5, recs=7))
    assert q["caps"] == dict(p["caps"], recs=7)


def test_default_caps_keep_every_unit_task_on_the_device(lib, unit):
    p = plan(lib, unit)
    r = rows(p)
    skipped = sum(1 for x in r if x["route"] == 2)
    assert p["routes_hit"] == [len(r) - skipped, 0, skipped] and skipped >= 4          # the masked sample and the flanks without k
    assert all(x["flags"] == 0 for x in r)
    # the sizes are the graphs': the reference flank alone has len - k edges and one node more
    l = [i for i, L in enumerate(unit.loci) if L["name"] == "no_reads_and_short_strings"][0]
    t = r[2 * int(unit.samp_off[l])]
    assert (t["k"], t["edges"], t["nodes"], t["recs"], t["reads"], t["len"], t["path_len"], t["strings"]) == (10, 22, 23, 23, 0, 32, 32, 0)


@pytest.mark.parametrize("kind", ORDER)
def test_each_cap_and_one_past_it(lib, unit, kind):
    """With the cap at the largest size of the batch nothing leaves the device for it; one below, exactly the tasks of that size do."""
    base = rows(plan(lib, unit))
    top = max(x[kind] for x in base)
    assert top > 1
    at = rows(plan(lib, unit, caps={kind: top}))
    assert all(x["flags"] == 0 for x in at)
    past = rows(plan(lib, unit, caps={kind: top - 1}))
    bit = capi.FLANK_FLAGS[FLAG[kind]]
    hit = [i for i, x in enumerate(past) if x["flags"]]
    assert hit == [i for i, x in enumerate(base) if x[kind] == top] and all(past[i]["flags"] == bit and past[i]["route"] == 1 for i in hit)
    # the sizes themselves do not depend on the caps
    assert [[x[k] for k in ORDER] for x in past] == [[x[k] for k in ORDER] for x in base]


def test_k_range_and_max_paths_the_device_does_not_serve(lib, unit):
    """The decision is per flank: its max_k = min(max_kmer, len - 1) and the k calc_kmer_length starts it at."""
    ref_len = [len(L["ref"][f]) for L in unit.loci for f in range(2) for _ in L["samples"]]
    K = capi.FLANK_FLAGS["k"]
    r = rows(plan(lib, unit, max_kmer=16))
    assert [x["flags"] for x in r if x["route"] != 2] == [K if n - 1 >= 16 else 0 for x, n in zip(r, ref_len) if x["route"] != 2]
    r = rows(plan(lib, unit, min_kmer=9))                      # seven values of k where the flank is long enough for k = 15
    assert [x["flags"] for x in r if x["route"] != 2] == [K if n - 1 >= 15 else 0 for x, n in zip(r, ref_len) if x["route"] != 2]
    assert K in [x["flags"] for x in r] and 0 in [x["flags"] for x in r if x["route"] != 2]
    r = rows(plan(lib, unit, max_paths=17))
    assert all(x["flags"] & capi.FLANK_FLAGS["param"] for x in r if x["route"] != 2)
    r = rows(plan(lib, unit, max_paths=16, min_kmer=11, max_kmer=12))
    assert all(x["flags"] == 0 for x in r)


def test_bytes_the_device_does_not_pack(lib):
    L = fc.unit_loci()[1]
    L["samples"][0]["reads"][0] = fc.rd(L["samples"][0]["reads"][0]["l"], L["samples"][0]["reads"][0]["r"].lower())
    c = fc.build([L])
    r = rows(plan(lib, c))
    assert [x["flags"] for x in r] == [0, capi.FLANK_FLAGS["byte"]]
