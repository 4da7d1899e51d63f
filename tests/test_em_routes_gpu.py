"""GPU: hipstr_em_train on the cases of tests/em_route_cases.py — both sides of every size edge of em.hip, the degenerate but legal inputs
(no reads, samples without reads, one allele, an unseen non-zero reference size, periods 1 and 7 to 9), batches around the block and
chunk sizes of the device-resident loop — against the oracle under the contract of tests/test_em_gpu.py (bit for bit; else device == the
oracle with correctly rounded exp / log bit for bit and that within 1e-9 of the host-libm oracle with identical iteration counts).
Every batch runs twice (identical bits) and its named loci alone (identical to their results in the batch).  The refusals are decided on
the host before any launch: tests/test_em_routes.py checks them without a device; here the call itself raises and the device goes on."""
import numpy as np
import pytest

from hipstr_amd import capi
import em_route_cases as ec
from test_em_gpu import _exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lim(hmm):
    return ec.limits(hmm)


@pytest.fixture(scope="module")
def cases(lim):
    return ec.cases(lim)


@pytest.fixture(scope="module")
def wanted(oracle, cases):
    """The oracle's result of a case, computed once."""
    memo = {}
    def get(name):
        if name not in memo:
            memo[name] = capi.run_em(oracle, "oracle_", **cases[name].kw)
            for a in memo[name]:
                a.setflags(write=False)
        return memo[name]
    return get


def _bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_case_against_the_oracle(hmm, oracle, cases, wanted, name):
    c = cases[name]
    got = capi.run_em(hmm, "hipstr_", **c.kw)
    again = capi.run_em(hmm, "hipstr_", **c.kw)
    assert _bits(got, again), "two runs of the same batch differ"
    want = wanted(name)
    assert len(got[0]) == len(c.kw["period"]) and np.all(np.isfinite(want[1])) and np.all(np.isfinite(want[3]))
    _exact(got, want, oracle, c.kw, "EM route case " + name)
    assert np.all(got[2] <= c.kw["max_iter"]) and np.all(got[0] | (got[2] == c.kw["max_iter"]))
    for l in c.alone:
        one = capi.run_em(hmm, "hipstr_", **ec.sub_batch(c.kw, [l]))
        assert _bits(one, tuple(x[l:l + 1] for x in got)), "locus %d alone differs from its result in the batch" % l
    if name.startswith("batch_of_") and len(got[2]) > 1 and c.kw["max_iter"] == 100:
        slow = ec.slow_indices(len(got[2]))
        rest = [i for i in range(len(got[2])) if i not in slow]
        assert want[2][slow].min() >= 3 * want[2][rest].max()


@pytest.mark.parametrize("name", ec.REFUSAL_NAMES)
def test_refused_inputs_raise_and_leave_the_device_usable(hmm, oracle, lim, cases, wanted, name):
    r = {x.name: x for x in ec.refusals(lim)}[name]
    with pytest.raises(RuntimeError, match=r.message):        # (the plan refuses the same input without a device: test_em_routes.py)
        capi.em_plan(hmm, **r.kw)
    with pytest.raises(RuntimeError, match=r.message):
        capi.run_em(hmm, "hipstr_", **r.kw)
    c = cases[ec.ORDINARY]
    _exact(capi.run_em(hmm, "hipstr_", **c.kw), wanted(ec.ORDINARY), oracle, c.kw, "after the refusal " + name)
