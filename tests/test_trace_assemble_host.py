"""CPU: the host-only side of hipstr_hmm_trace_ex's device assembly — the entry points exist, the slots hipstr_debug_trace_assemble_plan
reports hold every piece the oracle's records have (a slot that is too small is how the assemble kernel could go wrong: it would refuse the
request), and the LDS-or-HBM route follows the plan's threshold."""
import ctypes as C

import numpy as np

from hipstr_amd import capi
import util

FIELDS = ["hap_aln", "seq", "indel", "snp", "stitched", "lds_bytes", "in_lds"]


def test_entry_points_exist(hmm_host):
    for name in ("hipstr_hmm_trace_ex", "hipstr_debug_trace_assemble_plan"):
        assert hasattr(hmm_host, name), name
    assert capi.TRACE_ASSEMBLE_DEVICE == 1
    header = open(capi.ROOT + "/include/hipstr_hmm.h").read()
    assert "#define HIPSTR_TRACE_ASSEMBLE_DEVICE 1u" in header and "hipstr_hmm_trace_ex" in header


def _requests(oracle, sb, per_read, seed):
    _, seeds = capi.run_align(oracle, "oracle_", sb.ptr)
    A = sb.n_out // sb.n_reads
    rng = np.random.default_rng(seed)
    rr, aa = [], []
    for r in range(sb.n_reads):
        if seeds[r] >= 0:
            for k in rng.choice(A, size=min(A, per_read), replace=False):
                rr.append(r); aa.append(int(k))
    return rr, aa


def test_every_piece_of_the_oracle_fits_its_slot(hmm_host, oracle, monkeypatch):
    """About 200 fuzzed requests (fixed seed; interrupted repeats, 2-3 flank options): each piece of the oracle's record against the
    capacity the plan reports for that request."""
    rng = np.random.default_rng(4711)
    total = 0
    while total < 200:
        monkeypatch.setenv("HIPSTR_SYNTH_IMPERFECT", str(float(rng.choice([0.5, 1.0]))))
        kw = dict(n_loci=1, reads_per_locus=int(rng.integers(4, 16)), n_str_alleles=int(rng.integers(2, 12)), read_len=int(rng.integers(24, 251)),
                  flank_len=int(rng.integers(8, 161)), str_bp=int(rng.integers(4, 121)), n_flank_opts=int(rng.integers(2, 4)), seed=int(rng.integers(1, 1 << 30)))
        sb = capi.SynthBatch(**kw)
        rr, aa = _requests(oracle, sb, 2, 5)
        if not rr:
            continue
        h2r = capi.hap_aln_info(oracle, "oracle_", sb.ptr)
        rec = capi.run_trace(oracle, "oracle_", sb.ptr, rr, aa, h2r, cap=1 << 21)
        plan = capi.trace_assemble_plan(hmm_host, sb.ptr, rr, aa, None, h2r)
        assert plan["fields"] == FIELDS and len(plan["requests"]) == len(rr)
        for w, row in zip(rec, plan["requests"]):
            c = dict(zip(FIELDS, row))
            n_cigar = sum(ch in "MIDS" for ch in w["cigar"])
            stitched = sum(int(x) for x in "".join(ch if ch.isdigit() else " " for ch in w["cigar"]).split())
            assert len(w["hap_aln"]) <= c["hap_aln"], (kw, w, c)
            assert max(len(w["str_seq"]), len(w["flank_left"]), len(w["flank_right"])) <= c["seq"], (kw, w, c)
            assert len(w["indels"]) <= c["indel"] and len(w["snps"]) <= c["snp"], (kw, w, c)
            assert max(stitched, n_cigar, len(w["aln_str"])) <= c["stitched"], (kw, w, c)
            assert c["in_lds"] == (1 if c["lds_bytes"] <= plan["thresholds"]["HS_ASM_LDS"] else 0)
        total += len(rr)
    # without hap_to_ref nothing is stitched: no slot
    assert all(row[4] == 0 for row in capi.trace_assemble_plan(hmm_host, sb.ptr, rr, aa)["requests"])


def test_a_request_on_each_side_of_the_lds_threshold(hmm_host):
    """One read against one allele; hap_to_ref strings one character apart put the staging at the threshold and one byte past it."""
    rng = np.random.default_rng(7)
    seq = lambda n: "".join(rng.choice(list("ACGT"), n))
    lf, rf, st = seq(60), seq(60), "CAG" * 10
    b, A = util.simple_locus(lf, [st], rf, 3, [((lf + st + rf)[5:145], None, 5, True)])
    b.finalize()
    base = capi.trace_assemble_plan(hmm_host, b.ptr, [0], [0], [70], [b"M"])
    lim = base["thresholds"]["HS_ASM_LDS"]
    assert base["routes"] == ["assemble_lds", "assemble_hbm"]
    need = base["requests"][0][5]                       # grows by 2 per hap_to_ref character: the string and the stitched string's slot
    assert need < lim
    n_at = 1 + (lim - need) // 2
    at = capi.trace_assemble_plan(hmm_host, b.ptr, [0], [0], [70], [b"M" * n_at])
    past = capi.trace_assemble_plan(hmm_host, b.ptr, [0], [0], [70], [b"M" * (n_at + 1)])
    assert at["requests"][0][5] in (lim, lim - 1) and at["requests"][0][6] == 1 and at["routes_hit"] == ["assemble_lds"]
    assert past["requests"][0][5] > lim and past["requests"][0][6] == 0 and past["routes_hit"] == ["assemble_hbm"]
