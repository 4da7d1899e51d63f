"""CPU: the host-only parts of the allele census (hipstr_post_census, include/hipstr_hmm.h): the launch decisions of
hipstr_amd/csrc/census_layout.h as hipstr_debug_census_plan reports them, on either side of every threshold and against the header's own
constants; the exported symbols; the refusal of NULL arguments on a library that never opened a device."""
import ctypes as C
import os
import re

import pytest

from hipstr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    txt = open(os.path.join(ROOT, "hipstr_amd", "csrc", "census_layout.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (HS_CENSUS_[A-Z_]+) (\d+)\b", txt, flags=re.M)}


def test_thresholds_are_the_headers(hmm_host):
    h = header_constants()
    t = capi.census_plan(hmm_host, 0, 0)["thresholds"]
    assert t == {k: h[k] for k in t} and len(t) == 5
    assert h["HS_CENSUS_ROUTE_WAVE"] == 0 and h["HS_CENSUS_ROUTE_LDS"] == 1 and h["HS_CENSUS_ROUTE_GLOBAL"] == 2
    assert capi.CENSUS_ROUTES == ("wave", "lds", "global")
    # the workgroup route's workspace and three of it fit a CU's 160 KiB of LDS; the wavefront route's four slices fit easily
    assert 3 * 4 * t["HS_CENSUS_LDS_INTS"] <= 160 * 1024
    assert 4 * 4 * (t["HS_CENSUS_REQ_INTS"] * t["HS_CENSUS_WAVE_REQS"] + t["HS_CENSUS_WAVE_READS"] + 1) <= 16 * 1024


def test_routes_on_either_side_of_every_threshold(hmm_host):
    p = lambda q, r: capi.census_plan(hmm_host, q, r)
    t = p(0, 0)["thresholds"]
    wq, wr, lds, ri, wg = t["HS_CENSUS_WAVE_REQS"], t["HS_CENSUS_WAVE_READS"], t["HS_CENSUS_LDS_INTS"], t["HS_CENSUS_REQ_INTS"], t["HS_CENSUS_THREADS"]
    assert p(0, 0) == dict(route="wave", ws_ints=1, lanes=64, loci_per_workgroup=wg // 64, global_ints=0, thresholds=t)
    assert p(wq, wr)["route"] == "wave" and p(wq + 1, wr)["route"] == "lds" and p(wq, wr + 1)["route"] == "lds"
    assert p(wq + 1, 0)["lanes"] == wg and p(wq + 1, 0)["loci_per_workgroup"] == 1
    # the workspace: REQ_INTS dwords per request, one per read, the key counter
    assert p(7, 11)["ws_ints"] == ri * 7 + 11 + 1
    q = (lds - 1) // ri; r = lds - 1 - ri * q
    assert p(q, r)["ws_ints"] == lds and p(q, r)["route"] == "lds" and p(q, r)["global_ints"] == 0
    assert p(q, r + 1)["route"] == "global" and p(q + 1, 0)["route"] == "global"
    assert p(1, lds - 1 - ri)["route"] == "lds" and p(1, lds - ri)["route"] == "global"
    g = p(q, r + 1)
    assert g["global_ints"] >= g["ws_ints"] and g["global_ints"] % 32 == 0 and g["global_ints"] - g["ws_ints"] < 32      # a 128-byte line of its own


def test_routes_are_monotone(hmm_host):
    """More requests or more reads never send a locus back to a cheaper route."""
    order = {r: i for i, r in enumerate(capi.CENSUS_ROUTES)}
    t = capi.census_plan(hmm_host, 0, 0)["thresholds"]
    qs = [0, 1, 63, 64, 65, 1000, 4095, 4096, 4097, 100000]; rs = [0, 1, 255, 256, 257, 5000, t["HS_CENSUS_LDS_INTS"], 10 ** 6]
    grid = [[order[capi.census_plan(hmm_host, q, r)["route"]] for r in rs] for q in qs]
    for i in range(len(qs)):
        for j in range(len(rs)):
            assert i == 0 or grid[i][j] >= grid[i - 1][j]
            assert j == 0 or grid[i][j] >= grid[i][j - 1]
    assert {v for row in grid for v in row} == {0, 1, 2}
    with pytest.raises(RuntimeError, match="bad argument"):
        capi.census_plan(hmm_host, -1, 0)


def test_symbols_are_exported_and_declared(hmm_host):
    assert hasattr(hmm_host, "hipstr_post_census") and hasattr(hmm_host, "hipstr_debug_census_plan")
    pub = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read(); dbg = open(os.path.join(ROOT, "include", "hipstr_hmm_debug.h")).read()
    assert "int hipstr_post_census(" in pub and "hipstr_debug_census_plan" not in pub and "int hipstr_debug_census_plan(" in dbg
    # the Python structs have the header's fields, in its order
    for name, cls in (("hipstr_census_request", capi.HipstrCensusRequest), ("hipstr_census_out", capi.HipstrCensusOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), pub, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                parts = decl.split(",")
                names.append(parts[0].split()[-1].lstrip("*").split("[")[0])
                names += [x.strip().lstrip("*").split("[")[0] for x in parts[1:]]
        assert names == [f for f, _ in cls._fields_], name


def test_null_arguments_fail_without_a_device(hmm_host):
    capi._sig(hmm_host.hipstr_post_census, C.c_int, [C.c_void_p, C.POINTER(capi.HipstrCensusRequest), C.POINTER(capi.HipstrCensusOut)])
    rq = capi.HipstrCensusRequest(); o = capi.HipstrCensusOut()
    for a in ((None, None, None), (None, C.byref(rq), C.byref(o))):
        assert hmm_host.hipstr_post_census(*a) != 0
        assert b"null" in hmm_host.hipstr_last_error()
