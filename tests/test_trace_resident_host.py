"""CPU: the host-only side of the resident traceback result (hipstr_hmm_trace_resident, hipstr_trace_dev_*, hipstr_post_census_dev,
hipstr_assign_trace_stats_dev) — the entry points are exported and declared where they belong, capi's field constants are the header's, and
everything that can be refused without a device is refused by a library that never opened one."""
import ctypes as C
import re

import numpy as np

from hipstr_amd import capi

PUBLIC = ("hipstr_hmm_trace_resident", "hipstr_trace_dev_sizes", "hipstr_trace_dev_fetch", "hipstr_trace_dev_free", "hipstr_post_census_dev",
          "hipstr_assign_trace_stats_dev")
DEBUG = ("hipstr_debug_trace_dev_from_host",)


def _headers():
    return open(capi.ROOT + "/include/hipstr_hmm.h").read(), open(capi.ROOT + "/include/hipstr_hmm_debug.h").read()


def test_entry_points_are_exported_and_declared(hmm_host):
    public, debug = _headers()
    assert len(PUBLIC + DEBUG) == 7
    for name in PUBLIC + DEBUG:
        assert hasattr(hmm_host, name), name
    for name in PUBLIC:
        assert re.search(r"\b%s\(" % name, public), name
        assert not re.search(r"\b%s\(" % name, debug), name
    for name in DEBUG:
        assert re.search(r"\bint %s\(" % name, debug) and not re.search(r"\b%s\(" % name, public), name
    assert "typedef struct hipstr_trace_dev hipstr_trace_dev_t;" in public
    # the census request is part of the drop-in ABI: the resident form is an entry point, not a field
    body = public[public.index("typedef struct hipstr_census_request {"):public.index("} hipstr_census_request_t;")]
    assert "hipstr_trace_dev" not in body
    assert C.sizeof(capi.HipstrCensusRequest) == 96             # as before the resident form


def test_field_constants_are_the_headers():
    public, _ = _headers()
    names = ("SCALARS", "HAP_ALN", "STR_SEQ", "FLANKS", "INDELS", "SNPS", "STITCH", "ALL")
    got = {}
    for nm in names:
        m = re.search(r"#define HIPSTR_TRACE_F_%s\s+(0x[0-9a-fA-F]+)u" % nm, public)
        assert m, nm
        got[nm] = int(m.group(1), 16)
        assert getattr(capi, "TRACE_F_" + nm) == got[nm], nm
    assert got["ALL"] == sum(got[nm] for nm in names[:-1]) == 0x7f
    assert sorted(capi.TRACE_GROUPS) == sorted(got[nm] for nm in names[:-1])
    # every array of hipstr_trace_out_t belongs to exactly one group
    fields = [f for f, _ in capi.HipstrTraceOut._fields_ if f != "cap_chars"]
    assert sorted(nm for arrays in capi.TRACE_GROUPS.values() for nm, _, _ in arrays) == sorted(fields)


def _null_words(lib):
    return lib.hipstr_last_error().decode()


def test_refusals_without_a_device(hmm_host):
    lib = hmm_host
    capi._trace_dev_sigs(lib)
    z = np.zeros(8, np.int32); p = z.ctypes.data_as(capi._i32p)
    b = capi.HipstrBatch()
    h = C.c_void_p(0xdead)
    # ---- hipstr_hmm_trace_resident
    assert lib.hipstr_hmm_trace_resident(None, 1, p, p, None, None, 0, C.byref(h)) != 0 and "null" in _null_words(lib) and not h.value
    assert lib.hipstr_hmm_trace_resident(C.byref(b), 1, p, p, None, None, 0, None) != 0 and "null" in _null_words(lib)
    for args in ((1, None, p), (1, p, None), (-1, p, p)):
        h = C.c_void_p(0xdead)
        assert lib.hipstr_hmm_trace_resident(C.byref(b), args[0], args[1], args[2], None, None, 0, C.byref(h)) != 0
        assert "null" in _null_words(lib) and not h.value
    for flags in (1, 2, 1 << 31):
        h = C.c_void_p(0xdead)
        assert lib.hipstr_hmm_trace_resident(C.byref(b), 1, p, p, None, None, flags, C.byref(h)) != 0
        assert "unknown flag" in _null_words(lib) and not h.value
    # ---- sizes / fetch / free
    n = np.zeros(1, np.int32); tot = np.zeros(7, np.int64)
    assert lib.hipstr_trace_dev_sizes(None, n.ctypes.data_as(capi._i32p), tot.ctypes.data_as(C.POINTER(C.c_int64))) != 0 and "null" in _null_words(lib)
    o = capi.HipstrTraceOut()
    assert lib.hipstr_trace_dev_fetch(None, capi.TRACE_F_ALL, C.byref(o)) != 0 and "null" in _null_words(lib)
    lib.hipstr_trace_dev_free(None)
    for bits in (0x80, 0x100, 1 << 31, 0xff):
        assert lib.hipstr_trace_dev_fetch(None, bits, C.byref(o)) != 0 and "unknown field" in _null_words(lib)
    # ---- hipstr_debug_trace_dev_from_host
    h = C.c_void_p(0xdead)
    assert lib.hipstr_debug_trace_dev_from_host(None, 0, C.byref(h)) != 0 and "null" in _null_words(lib) and not h.value
    assert lib.hipstr_debug_trace_dev_from_host(C.byref(o), 0, None) != 0 and "null" in _null_words(lib)
    # ---- hipstr_post_census_dev
    rq = capi.HipstrCensusRequest(); out = capi.HipstrCensusOut()
    fn = lib.hipstr_post_census_dev
    assert fn(None, None, None, None) != 0 and "null" in _null_words(lib)
    assert fn(None, C.byref(rq), None, C.byref(out)) != 0 and "null" in _null_words(lib)
    rq.pooled = C.pointer(b); rq.seed = p; rq.read_req = p
    t = capi.HipstrTraceOut(); rq.trace = C.pointer(t)
    assert fn(None, C.byref(rq), None, C.byref(out)) != 0 and "rq->trace must be NULL" in _null_words(lib)
    # ---- hipstr_assign_trace_stats_dev
    pb = capi.PostBatch([2], [1], [0, 2], [0, 0], np.zeros(2), np.zeros(2), np.ones(2, np.int32), None)
    args = [pb.ptr, p, None] + [p] * 9            # (no handle exists without a device: the handle's place stays NULL throughout)
    for i in range(len(args)):
        bad = list(args); bad[i] = None
        assert lib.hipstr_assign_trace_stats_dev(*bad) != 0 and "null" in _null_words(lib)
