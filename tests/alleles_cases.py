"""Cases of the allele-set update (hipstr_alleles_apply): the makers of the three batches, the text format integration/genotype_flow.cpp's
--allele-cases mode reads and writes, and the rule that turns the reference's two haplotype lists into the expected mapping and mask.

A case is one locus: dict(name, period, blocks = 3 x (start, end, [option strings]), remove = 3 lists of option indices, add = 3 lists of
strings, on, n_reads).  `remove` / `add` are what the reference is given; a locus that is off keeps them empty and carries in `ignored_remove`
what the request says all the same (the call must not read it).
"""
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

# the limits of hipstr_amd/csrc/alleles_layout.h the `edges` batch is built around (the tests check them against hipstr_debug_alleles_limits)
THREADS, MAX_HAPS, MAX_OPTS = 256, 1024, 1024


def case(name, blocks, remove=None, add=None, period=2, on=True, n_reads=1, ignored_remove=None):
    nopts = [len(b) for b in blocks]
    start = 1000
    bl = []
    for b in blocks:
        bl.append((start, start + len(b[0]), list(b))); start += len(b[0])
    c = dict(name=name, period=period, blocks=bl, remove=[list(x) for x in (remove or [[], [], []])], add=[list(x) for x in (add or [[], [], []])],
             on=on, n_reads=n_reads, ignored_remove=[list(x) for x in (ignored_remove or [[], [], []])])
    for k in range(3):
        assert all(1 <= i < nopts[k] for i in c["remove"][k] + c["ignored_remove"][k])
    return c


def word(i, n=6):
    """the i-th string of length n over ACGT: distinct for i < 4**n"""
    return "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(n))


L, R = "GATTACAG", "CTTGCATA"


def unit():
    return [
        case("one_add", [[L], ["ACAC", "ACACAC"], [R]], add=[[], ["AC"], []]),
        # all three Gray digits reflected, the mapping not monotone
        case("remove_and_add", [["GG", "GA"], ["ACAC", "AC", "ACACAC"], ["TT", "TC"]], remove=[[], [1], []], add=[["GT"], [], []]),
        # "AC"+"GT" == "A"+"CGT": two option triples, one haplotype string; the later old haplotype wins
        case("equal_concat", [["AC", "A"], ["GT", "CGT"], [R]], add=[[], ["GTGT"], []]),
        case("readd_removed", [[L], ["ACAC", "AC", "ACACAC"], [R]], remove=[[], [1], []], add=[[], ["AC"], []]),
        case("add_present", [[L], ["ACAC", "AC"], [R]], add=[[], ["AC"], []]),
        case("empty_string", [[L], ["ACAC", "", "AC"], [R]], remove=[[], [2], []], add=[[], ["", "ACACAC"], []]),
        case("all_single", [[L], ["ACAC"], [R]], add=[["GATTACAT"], ["AC", "ACACAC"], ["CTTGCATT"]]),
        case("off_between", [[L, "GATTACAT"], ["ACAC", "AC", "ACACAC"], [R]], on=False, ignored_remove=[[1], [1], []]),
        case("no_reads", [[L], ["ACAC", "AC", "ACACAC"], [R]], remove=[[], [2], []], add=[[], ["ACACACAC"], []], n_reads=0),
    ]


def edges():
    out = []
    for a in (THREADS - 1, THREADS, THREADS + 1):                      # the new A around the workgroup's lane count
        out.append(case("new_A_%d" % a, [[L], [word(i) for i in range(a - 1)], [R]], add=[[], [word(5000, 7)], []]))
    out.append(case("wide_1000", [[L], [word(i) for i in range(1000)], [R]], remove=[[], [3, 500, 999], []], add=[[], [word(3), word(2000), word(7, 5)], []]))
    out.append(case("cube_4_62_4", [[word(i, 4) for i in range(4)], [word(i) for i in range(62)], [word(9 + i, 4) for i in range(4)]],
                    remove=[[2], [1, 60], [3]], add=[[word(77, 4)], [word(100)], [word(78, 4)]]))      # 992 -> 4 * 61 * 4 = 976
    long = ("ACG" * 683)[:2047]
    out.append(case("str_2047", [[L], ["ACGACG", long, "ACG"], [R]], remove=[[], [2], []], add=[[], [long[:-1] + "T", long[:2046]], []], period=3))
    # just beyond each limit: the host code inside the device call
    out.append(case("old_opts_over", [[L], [word(i) for i in range(MAX_OPTS - 1)], [R]], remove=[[], [1, 2], []]))                    # 1025 old options, 1023 haplotypes
    out.append(case("new_opts_over", [[L], [word(i) for i in range(MAX_OPTS - 4)], [R]], add=[[], [word(4000), word(4001), word(4002)], []]))    # 1025 new options
    out.append(case("old_haps_over", [[word(i, 4) for i in range(5)], [word(i) for i in range(205)], [R]], remove=[[4], [], []]))     # 1025 old haplotypes, 820 new
    out.append(case("new_haps_over", [[word(i, 4) for i in range(4)], [word(i) for i in range(205)], [R]], add=[[word(99, 4)], [], []]))  # 820 old, 1025 new
    return out


def random_batch(seed=20240607, n=64):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        period = rng.randint(1, 6)
        motif = "".join(rng.choice("ACGT") for _ in range(period))
        blocks = [[L], [], [R]]
        for k in (0, 2):
            for _ in range(rng.choice([0, 0, 1, 2])):
                s = list(blocks[k][0]); s[rng.randrange(len(s))] = rng.choice("ACGT"); blocks[k].append("".join(s))
        blocks[1] = [motif * rng.randint(2, 8)]
        for _ in range(rng.randint(0, 11)):
            blocks[1].append(motif * rng.randint(0, 12) + rng.choice(["", "", motif[:rng.randint(0, period)]]))
        remove = [[o for o in range(1, len(b)) if rng.random() < 0.3] for b in blocks]
        add = [[], [], []]
        for k in range(3):
            for _ in range(rng.choice([0, 0, 1, 2]) if k == 1 else rng.choice([0, 0, 0, 1])):
                s = list(rng.choice(blocks[k]))                         # a mutated existing option: sometimes unchanged, sometimes a removed one
                r = rng.random()
                if s and r < 0.4:
                    s[rng.randrange(len(s))] = rng.choice("ACGT")
                elif r < 0.6:
                    s += list(motif)
                elif s and r < 0.7:
                    s = s[:-1]
                add[k].append("".join(s))
        out.append(case("rnd_%02d" % i, blocks, remove=remove, add=add, period=period, n_reads=rng.randint(0, 2)))
    return out


BATCHES = dict(unit=unit, edges=edges, random=random_batch)


# ------------------------------------------------------------------------------------------------------------------ the text format
_show = lambda s: s if s else "-"
_seq = lambda s: "" if s == "-" else s


def case_text(cases):
    out = []
    for c in cases:
        out.append("case %s %d" % (c["name"], c["period"]))
        for b, (s, e, opts) in enumerate(c["blocks"]):
            out.append("block %d %d %d %d %s" % (b, s, e, len(opts), " ".join(_show(o) for o in opts)))
        for b in range(3):
            out.append(("remove %d %d %s" % (b, len(c["remove"][b]), " ".join(str(i) for i in c["remove"][b]))).rstrip())
        for b in range(3):
            out.append(("add %d %d %s" % (b, len(c["add"][b]), " ".join(_show(o) for o in c["add"][b]))).rstrip())
    return "\n".join(out) + "\n"


def parse_cases(text):
    """case_text's inverse, but for on / n_reads / ignored_remove, which the reference does not see: the caller takes those from the makers"""
    out = []; lines = text.splitlines(); i = 0
    while i < len(lines):
        w = lines[i].split(" ")
        assert w[0] == "case"
        c = dict(name=w[1], period=int(w[2]), blocks=[], remove=[], add=[])
        for b in range(3):
            x = lines[i + 1 + b].split(" "); assert x[0] == "block" and int(x[1]) == b and int(x[4]) == len(x) - 5
            c["blocks"].append((int(x[2]), int(x[3]), [_seq(o) for o in x[5:]]))
        for b in range(3):
            x = lines[i + 4 + b].split(" "); assert x[0] == "remove" and int(x[2]) == len(x) - 3
            c["remove"].append([int(o) for o in x[3:]])
        for b in range(3):
            x = lines[i + 7 + b].split(" "); assert x[0] == "add" and int(x[2]) == len(x) - 3
            c["add"].append([_seq(o) for o in x[3:]])
        out.append(c); i += 10
    return out


def parse_records(text):
    """{name: dict(old = haplotype strings, blocks = 3 x (start, end, options), new = haplotype strings)} in the reference's order"""
    out = {}; cur = None; into = None
    for line in text.splitlines():
        w = line.split(" ")
        if w[0] == "case":
            cur = out[w[1]] = dict(old=[], blocks=[], new=[])
        elif w[0] in ("old", "new"):
            into = cur[w[0]]; cur["n_" + w[0]] = int(w[1])
        elif w[0] == "hap":
            into.append(_seq(w[1]))
        elif w[0] == "block":
            assert int(w[1]) == len(cur["blocks"]) and int(w[4]) == len(w) - 5
            cur["blocks"].append((int(w[2]), int(w[3]), [_seq(o) for o in w[5:]]))
    for r in out.values():
        assert len(r["old"]) == r["n_old"] and len(r["new"]) == r["n_new"] and len(r["blocks"]) == 3
    return out


def golden(batch):
    """(cases with the makers' on / n_reads / ignored_remove, records) of tests/golden/alleles_<batch>.npz"""
    z = np.load(os.path.join(GOLD, "alleles_%s.npz" % batch))
    cases = parse_cases(bytes(z["cases"]).decode()); made = BATCHES[batch]()
    assert [c["name"] for c in cases] == [m["name"] for m in made]
    for c, m in zip(cases, made):
        assert c["blocks"] == m["blocks"] and c["remove"] == m["remove"] and c["add"] == m["add"], c["name"]      # the fixture is of these makers
        c.update(on=m["on"], n_reads=m["n_reads"], ignored_remove=m["ignored_remove"])
    return cases, parse_records(bytes(z["records"]).decode())


# ------------------------------------------------------------------------------------------------------------------ what is expected
def expected_of(rec):
    """seq_stutter_genotyper.cpp:331-336 / :358-367 on the reference's own two lists -> (allele_mapping, realign_to_haplotype)"""
    index = {}
    for i, s in enumerate(rec["old"]):
        index[s] = i                                                   # a later haplotype with the same string wins
    mapping = [-1] * len(rec["old"]); realign = []
    for j, s in enumerate(rec["new"]):
        if s in index:
            realign.append(0); mapping[index[s]] = j
        else:
            realign.append(1)
    return np.array(mapping, np.int32), np.array(realign, np.uint8)


def gray_options(nopts):
    """[A, 3]: Haplotype::next's visit order (Haplotype.cpp:157-196) by stepping it: block 0 fastest, each block bouncing between its ends"""
    counts = [0, 0, 0]; dirs = [1, 1, 1]; A = nopts[0] * nopts[1] * nopts[2]
    factors = [1, nopts[0], nopts[0] * nopts[1]]
    out = [tuple(counts)]
    for counter in range(A - 1):
        t = counter + 1; index = -1
        for j in (2, 1, 0):
            t %= factors[j]
            if t == 0:
                index = j; break
        counts[index] += dirs[index]
        if counts[index] == 0 or counts[index] == nopts[index] - 1:
            dirs[index] *= -1
        out.append(tuple(counts))
    return np.array(out, np.int32).reshape(A, 3)


def request_of(cases):
    """(capi.Batch arguments per locus, locus_on, keep, add) for capi.run_alleles_apply"""
    loci = []; on = []; keep = []; add = []
    for c in cases:
        reads = [dict(seq="ACGT", qual="FFFF", start=c["blocks"][0][0], cigar=[("=", 4)]) for _ in range(c["n_reads"])]
        loci.append((c["blocks"], c["period"], [0.9, 0.05, 0.05, 0.7, 0.005, 0.005], reads))
        on.append(1 if c["on"] else 0)
        rem = c["remove"] if c["on"] else c["ignored_remove"]
        for b in range(3):
            keep += [0 if o in rem[b] else 1 for o in range(len(c["blocks"][b][2]))]
        add.append([[s.encode() for s in c["add"][b]] for b in range(3)])
    return loci, np.array(on, np.uint8), np.array(keep, np.uint8), add
