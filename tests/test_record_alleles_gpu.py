"""GPU: hipstr_record_alleles (hipstr_amd/csrc/record_alleles.hip) against its host form, which tests/test_record_alleles_host.py holds to
the compiled reference: every output byte equal on every case of tests/record_alleles_cases.py — the goldens' batches, the cases the
reference cannot be given, loci one at a time, one batch that mixes loci below and above the device's option cap, poisoned cache blocks —
and the chained run: the twelve loci of tests/flow_chain.py through genotype() on the device backend, hipstr_record_alleles on the final
blocks, then hipstr_post_extract_vcf on the posteriors the chain left launched with the maps the library returned, against
hipstr_post_extract gathered in numpy."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain as fc
import post_extract_vcf_cases as pc
import record_alleles_cases as ac
from test_poison_gpu import poisoned, same_bits
from test_record_alleles_host import check_against

pytestmark = pytest.mark.gpu


def both(hmm, cases, **kw):
    loci = [ac.locus_of(c) for c in cases]
    dev = capi.run_record_alleles(hmm, loci, **kw)
    last = capi.record_alleles_last(hmm)
    same_bits(dev, capi.run_record_alleles(hmm, loci, host=True, **kw), "hipstr_record_alleles against its host form")
    return dev, last


@pytest.mark.parametrize("batch", sorted(ac.BATCHES))
def test_goldens_batches(hmm, batch):
    cases = ac.BATCHES[batch]()
    dev, last = both(hmm, cases)
    check_against(dev, cases, ac.golden(batch), batch)
    assert last["loci"] == len(cases) and last["host_loci"] == 0 and last["bytes_up"] > 0 and last["bytes_down"] > 0
    both(hmm, cases, flanks=False)


def test_one_locus_at_a_time_and_nothing(hmm):
    gold = ac.golden("unit")
    for c in ac.unit_cases():
        dev, _ = both(hmm, [c])
        check_against(dev, [c], gold, "alone")
    dev, last = both(hmm, [])
    assert dev == [] and last["loci"] == 0


def test_loci_below_and_above_the_cap_in_one_batch(hmm):
    """Block 1 of 300 options between loci of a few: the host twin inside the call, the offsets behind it unmoved."""
    unit = ac.unit_cases()
    cases = unit[:5] + [ac.beyond_cap_case()] + ac.no_reference_cases() + unit[5:] + [ac.beyond_cap_case()] + ac.random_cases(9, 12)
    at_cap = ac.case("v256", 150, 170, 146, 174, ac.beyond_cap_case()["blocks"][1][2][:ac.DEVICE_OPTIONS])
    dev, last = both(hmm, cases + [at_cap])
    assert last["loci"] == len(cases) + 1 and last["host_loci"] == 2
    check_against([d for d, c in zip(dev, cases) if c["name"] in ac.golden("unit")], unit, ac.golden("unit"), "mixed")
    assert dev[5]["status"] == 0 and len(dev[5]["alleles"]) == 300 and dev[-1]["status"] == 0 and len(dev[-1]["alleles"]) == ac.DEVICE_OPTIONS
    _, last = both(hmm, [ac.beyond_cap_case()])
    assert last["host_loci"] == 1 and last["bytes_up"] == 0                       # nothing left for the device: nothing is sent


def test_refusals_launch_nothing(hmm):
    L = ac.locus_of(ac.unit_cases()[3])
    with pytest.raises(RuntimeError, match="cap_alleles is too small") as e:
        capi.run_record_alleles(hmm, [L], caps=(10, 1000, 1000))
    assert all(np.all(v == (0xEE if v.dtype == np.uint8 else capi.UNTOUCHED)) for v in e.value.raw.values())
    L["region_stop"] = L["region_start"] - 1
    with pytest.raises(RuntimeError, match="region_stop < region_start"):
        capi.run_record_alleles(hmm, [L])


def test_on_poisoned_cache_blocks(hmm):
    loci = [ac.locus_of(c) for c in ac.unit_cases() + ac.random_cases()]
    out = poisoned(hmm, lambda: capi.run_record_alleles(hmm, loci), "record alleles")
    same_bits(out[0], capi.run_record_alleles(hmm, loci, host=True), "poisoned against the host form")


def chain_locus(s):
    """A state's final blocks as a locus of hipstr_record_alleles: the region of its fixture, and a window whose bases are the reference
    options of the three blocks where they lie (lower case, to be folded) and N around them."""
    _, rs, re_, _, _ = s.inp.region
    ref = {}
    for st, en, opts in s.blocks:
        for i, ch in enumerate(opts[0][:en - st]):
            ref[st + i] = ch.lower()
    window = "".join(ref.get(p, "N") for p in range(rs - ac.WIN_PAD, re_ + ac.WIN_PAD)).encode()
    return dict(region_start=rs, region_stop=re_, window=window, blocks=[(st, en, [o.encode() for o in opts]) for st, en, opts in s.blocks])


def test_alleles_and_vcf_order_after_the_chain(hmm, oracle):
    names = list(fc.CASES)
    assert len(names) == 12
    states = [fc.State(fc.Inputs(n), oracle) for n in names]
    be = fc.DeviceBackend(hmm)
    try:
        k, pooled, seeds = fc.genotype_pass(states, be, oracle, None)          # genotype(): the final posteriors are launched on be.pd
        loci = [chain_locus(s) for s in states]
        al = capi.run_record_alleles(hmm, loci)
        same_bits(al, capi.run_record_alleles(hmm, loci, host=True), "alleles of the chain's blocks against the host form")
        assert all(a["status"] & ~ac.FLANK_ASSERT == 0 for a in al)
        for a, s in zip(al, states):                                           # the maps sort the strings the call returned
            srt = [a["alleles"][i] for i in a["new_to_old"]]
            assert a["new_to_old"][0] == 0 and srt[1:] == sorted(srt[1:], key=lambda x: (len(x), x)) and len(a["alleles"]) == len(s.blocks[1][2])
        assert sum(a["new_to_old"] != sorted(a["new_to_old"]) for a in al) >= 2, "the chain's final blocks are all in the record's order"
        n2o = np.concatenate([a["new_to_old"] for a in al]).astype(np.int32); o2n = np.concatenate([a["old_to_new"] for a in al]).astype(np.int32)
        bp = np.concatenate([a["bp_diff"] for a in al]).astype(np.int32)
        h2a = np.concatenate([s.options()[:, 1] for s in states]).astype(np.int32)
        nv = np.array([len(s.blocks[1][2]) for s in states], np.int32)
        plain = capi.run_post_extract_flat(hmm, be.pb, nv, h2a, pd=be.pd)
        got = capi.run_post_extract_flat(hmm, be.pb, nv, h2a, order=(n2o, o2n), pd=be.pd, allele_bp_diff=bp)
        want = pc.permute_gt_outputs(plain, be.pb, nv, n2o, o2n)
        keys = ("best_hap", "best_gt", "log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff", "gls", "pls", "phased_gls")
        same_bits({x: got[x] for x in keys}, {x: want[x] for x in keys}, "hipstr_post_extract_vcf after the chain")
        at = np.repeat(np.concatenate([[0], np.cumsum(nv)])[:-1], nv)
        assert np.array_equal(got["bp_diffs"], bp[at + n2o])
        # BPDIFFS ascend by length within a locus: the order is the record's
        for l in range(len(states)):
            d = got["bp_diffs"][int(np.sum(nv[:l])) + 1:int(np.sum(nv[:l + 1]))]
            assert np.all(np.diff(d) >= 0), names[l]
    finally:
        be.close()
