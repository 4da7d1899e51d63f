"""The 18 loci of tests/golden/flowin_*.txt.gz as inputs of the haplotype generator: what a caller of the C-ABI has BEFORE the blocks exist
— the un-pooled reads, the region and a reference window — so that hipstr_hapgen_* can be held to the three `block` lines
SeqStutterGenotyper::init -> build_haplotype left in the same files.

The fixtures hold no chromosome.  The window is put together from the fixture's own blocks: block 0 + option 0 of block 1 + block 2 is the
reference over [block 0's start, block 2's end), padded with N out to region_start - 40 and region_stop + 40.  The reference never reads
the padded positions: the fused flanks start at min_start >= blk1_start - 35 >= region_start - 40 and the padded region lies inside the
blocks.  read_stop is not in the fixtures either: the request leaves it NULL (start + the =, X and D runs, the flow driver's exclusive end)."""
import flow_chain as fc
import flow_chain_flanks as ff

NAMES = list(fc.CASES) + list(ff.CASES)
CHROM_LEN = 1400                       # integration/genotype_flow.cpp's chromosome


def inputs(name):
    return fc.Inputs(name) if name in fc.CASES else ff.Inputs(name)


def locus_of(inp):
    """tests/hapgen_cases.py's locus dict from a fixture."""
    _, start, stop, period, _ = inp.region
    (s0, e0, o0), (s1, e1, o1), (s2, e2, o2) = inp.blocks
    assert e0 == s1 and e1 == s2 and len(o0) == len(o2) == 1 and period == inp.period
    left, right = s0 - (start - 40), (stop + 40) - e2
    assert left >= 0 and right >= 0 and s1 >= start - 5 and e1 <= stop + 5
    window = "N" * left + o0[0] + o1[0] + o2[0] + "N" * right
    assert len(window) == stop - start + 80
    reads = [dict(start=r["start"], cigar=r["cigar"], seq=r["seq"], qual=r["qual"], sample=s, use=True, stop=0) for r, s in zip(inp.reads, inp.sample)]
    return dict(name=inp.name, window=window, chrom_len=CHROM_LEN, region_start=start, region_stop=stop, period=period, n_samples=inp.n_samples, reads=reads,
                stutter=list(inp.stutter))


def fixture_batch(inps):
    """The un-pooled batch flow_chain.build_batch makes from the fixtures' own blocks."""
    return fc.build_batch([fc.State(i, None) for i in inps], [i.reads for i in inps])
