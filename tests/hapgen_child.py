"""Child process of tests/test_hapgen_gpu.py: the device call on the `random` golden batch under whatever HIPSTR_DEBUG_HAPGEN_HASH_BITS the
parent set in its environment, against the host twin.  Prints one JSON line: hipstr_debug_hapgen_last and whether every output was
identical.  A fresh process: the library opens its device here and nowhere else."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
from hipstr_amd import capi  # noqa: E402
import hapgen_cases as hc  # noqa: E402


def main():
    lib = capi.load_hmm()
    assert lib.hipstr_hmm_init(0) == 0, lib.hipstr_last_error().decode()
    loci, _ = hc.load_golden("random")
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    host = capi.run_hapgen(lib, b.ptr, rq, host=True)
    got = capi.run_hapgen(lib, b.ptr, rq)
    last = capi.hapgen_last(lib)
    try:
        hc.assert_same(got, host, "child")
        hc.assert_result(got, hc.expectation(loci), "child")
        same = True
    except AssertionError as e:
        same = False
        last["why"] = str(e)[:200]
    print(json.dumps(dict(last, same=same, loci=len(loci), bits=os.environ.get("HIPSTR_DEBUG_HAPGEN_HASH_BITS", ""))))
    lib.hipstr_hmm_shutdown()


if __name__ == "__main__":
    main()
