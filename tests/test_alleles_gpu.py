"""GPU: hipstr_alleles_apply and hipstr_alleles_step on the device (hipstr_amd/csrc/alleles.hip) against the reference's records
(tests/golden/alleles_*.npz) and, bit for bit in every output array — the rebuilt seq and opt_off included — against the host form.  The
`edges` batch holds the sizes at which the kernel's loops and its table turn over, and one locus just beyond each limit of
hipstr_amd/csrc/alleles_layout.h, which must take the host code inside the device call."""
import numpy as np
import pytest

from hipstr_amd import capi
import alleles_cases as ac
import alleles_checks as chk

pytestmark = pytest.mark.gpu
OVER = ("old_opts_over", "new_opts_over", "old_haps_over", "new_haps_over")


@pytest.fixture
def lib(hmm):
    capi._alleles_sigs(hmm)
    assert hmm.hipstr_debug_alleles_hash_bits(0) == 0
    yield hmm
    hmm.hipstr_debug_alleles_hash_bits(0)


@pytest.mark.parametrize("batch", sorted(ac.BATCHES))
def test_golden_batches_and_the_host_form(lib, batch):
    a, cases = chk.run_golden(lib, batch, host=False)
    last = capi.alleles_last(lib)
    over = [c["name"] for c in cases if c["name"] in OVER]
    assert (sorted(over) == sorted(OVER)) == (batch == "edges")
    assert last["host_loci"] == len(over) and last["identity_loci"] == sum(not c["on"] for c in cases), last
    assert last["device_loci"] == len(cases) - last["host_loci"] - last["identity_loci"] and last["chunks"] == 1, last
    chk.same(a, chk.apply_cases(lib, cases, host=True), "device against host form")


def test_each_limit_alone_sends_its_locus_to_the_host_code(lib):
    assert capi.alleles_limits(lib) == dict(threads=ac.THREADS, max_haps=ac.MAX_HAPS, max_opts=ac.MAX_OPTS, slots=2 * ac.MAX_HAPS)
    cases, recs = chk.golden("edges")
    by = {c["name"]: c for c in cases}
    for name in OVER:
        a = chk.apply_cases(lib, [by["wide_1000"], by[name]], host=False)
        last = capi.alleles_last(lib)
        assert last["device_loci"] == 1 and last["host_loci"] == 1, (name, last)
        chk.check_golden(a, [by["wide_1000"], by[name]], recs)


@pytest.mark.parametrize("batch", ["unit", "random"])
def test_bytes_decide_when_hashes_collide(lib, batch):
    full, cases = chk.run_golden(lib, batch, host=False)
    n64 = capi.alleles_last(lib)["compares"]
    assert lib.hipstr_debug_alleles_hash_bits(4) == 0
    cut, _ = chk.run_golden(lib, batch, host=False)
    last = capi.alleles_last(lib)
    chk.same(cut, full, "4-bit hash against 64-bit hash")
    assert last["compares"] > n64 and last["host_loci"] == 0, (last, n64)


@pytest.mark.parametrize("batch", ["unit", "edges"])
def test_alleles_on_poisoned_cache_blocks(lib, batch):
    """tests/test_poison_gpu.py's protocol (its docstring has this kernel's entry): the chunk's device block and its two pinned blocks are
    recycled cache blocks filled with 0xFF, 0x7F, 0x80 and 0x00 — every output array identical under the four bytes, the first result
    the reference's records, no block fresh from the driver.  `edges` has the loci the host code does inside the device call: their
    pieces of the result never pass through a block."""
    import test_poison_gpu as tp
    lib.hipstr_hmm_trim()                                           # what the tests before left: a fill then costs milliseconds
    cases, recs = chk.golden(batch)
    held = []
    def run():
        held.append(chk.apply_cases(lib, cases, host=False))
        return held[-1].arrays()
    try:
        tp.poisoned(lib, run, "alleles " + batch)
        chk.check_golden(held[1], cases, recs)                      # (held[0] is the warm-up)
        last = capi.alleles_last(lib)
        assert last["chunks"] == 1 and last["host_loci"] == sum(c["name"] in OVER for c in cases), last
    finally:
        for a in held:
            a.free()


def test_refusals(lib):
    chk.refusals(lib, host=False)


def test_policy_against_flow_chain_state(lib, oracle):
    chk.policy(lib, oracle, host=False)
