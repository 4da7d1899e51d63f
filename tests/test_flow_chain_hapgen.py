"""CPU: the cross-check of the haplotype generator on the existing fixtures.  All 18 loci of tests/golden/flowin_*.txt.gz as ONE ragged
batch: from the reads, the region and a window made of the fixture's own blocks (tests/flow_chain_hapgen.py), read_stop = NULL,
hipstr_hapgen_host must return exactly the three `block` lines the reference's build_haplotype left in the fixture, and the haplotype
arrays of hipstr_hapgen_batch(HIPSTR_HAPGEN_ON_HOST) must equal those flow_chain.build_batch makes from the fixture — so the rest of the
chain (tests/test_flow_chain*.py) is unchanged by construction when it starts from reads alone."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain_hapgen as fh
import hapgen_cases as hc

HAP_KEYS = ("blk_start", "blk_end", "blk_nopts", "period", "stutter", "opt_off", "hap_off")
READ_KEYS = ("read_off", "base_off", "read_start", "cigar_off", "cigar_len")


@pytest.fixture(scope="module")
def eighteen():
    inps = [fh.inputs(n) for n in fh.NAMES]
    loci = [fh.locus_of(i) for i in inps]
    return inps, loci, hc.ReadsBatch(loci), hc.request_of(loci, give_stop=False)


def test_the_fixtures_are_the_eighteen(eighteen):
    inps, loci = eighteen[:2]
    assert len(loci) == 18 and len({lc["name"] for lc in loci}) == 18
    assert {lc["period"] for lc in loci} == {1, 2, 3, 4, 5, 6} and max(len(i.blocks[1][2]) for i in inps) >= 4
    assert len({len(lc["reads"]) for lc in loci}) > 6                   # ragged


def check_blocks(got, inps):
    assert got["status"].tolist() == [0] * len(inps)
    for l, inp in enumerate(inps):
        assert hc.blocks_of(got, l) == [(s, e, list(o)) for s, e, o in inp.blocks], inp.name


def check_batch(hb, inps):
    want = fh.fixture_batch(inps).arrays
    got = hb.arrays()
    assert hb.locus.tolist() == list(range(len(inps))) and hb.status.tolist() == [0] * len(inps)
    for k in HAP_KEYS + READ_KEYS:
        assert np.array_equal(got[k], want[k]), k
    for k in ("seq", "bases", "quals", "cigar_op"):
        assert bytes(got[k]) == want[k][:-1], k
    assert got["realign_hap"].size == 0 and got["realign_read"].size == 0 and want["realign_hap"] is None


def test_host_twin_returns_the_fixtures_blocks(hmm_host, eighteen):
    inps, loci, b, rq = eighteen
    got = capi.run_hapgen(hmm_host, b.ptr, rq, host=True)
    check_blocks(got, inps)
    hc.assert_result(got, restated(loci), "the eighteen")


def restated(loci):
    """hapgen_cases.expectation on loci that bring a window instead of a chromosome: the window placed in a chromosome of N."""
    full = []
    for lc in loci:
        a = lc["region_start"]
        chrom = "N" * (a - 40) + lc["window"] + "N" * (lc["chrom_len"] - (lc["region_stop"] + 40))
        reads = []
        for r in lc["reads"]:
            reads.append(dict(r, stop=r["start"] + sum(n for op, n in r["cigar"] if op != "I")))
        full.append(dict(lc, chrom=chrom, reads=reads))
    return hc.expectation(full)


def test_hapgen_batch_equals_the_fixture_built_batch(hmm_host, eighteen):
    inps, loci, b, rq = eighteen
    hb = capi.HapgenBatch(hmm_host, b.ptr, rq, capi.HAPGEN_ON_HOST)
    try:
        check_batch(hb, inps)
    finally:
        hb.close()
