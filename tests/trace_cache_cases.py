"""Helper (not a test module): the batch, the sources and the numpy bookkeeping shared by tests/test_trace_gather_gpu.py,
tests/test_trace_cache_gpu.py and tests/test_trace_cache_threads_gpu.py.

The batch is a capi.SynthBatch of 2 loci x 40 reads x 4 alleles whose sizes (reads of 200 bases, flanks of 70, STR blocks of 72) and
generator seed were picked on the CPU with the oracle's trace (oracle_trace over every seeded read and every allele) so that the records
hold pieces on both sides of a wavefront's 64 elements where a traceback can: seed 8 has a read that misses the STR block
(stutter_size == HIPSTR_NO_STR_DATA, an empty str_seq and an empty flank), str_seq pieces of up to 76 bases, flank pieces of up to 74, an
indel record, hap_aln and alignment strings of 200 and more.  test_trace_gather_gpu.py asserts all of that from the fetched sources."""
import numpy as np

from hipstr_amd import capi

NO_STR = -100000                     # HIPSTR_NO_STR_DATA
AUTO = -2                            # HIPSTR_SEED_AUTO
MAX_SEGMENTS, COMPACT_MIN_DEAD = 16, 4096      # HS_TC_MAX_SEGMENTS, HS_TC_COMPACT_MIN_DEAD (tests/test_trace_cache_host.py pins them)
BATCH = dict(n_loci=2, reads_per_locus=40, n_str_alleles=4, read_len=200, flank_len=70, str_bp=72, seed=8)
SCALARS = ("ll", "max_index", "stutter_size", "flank_ins", "flank_del", "aln_start", "aln_stop")
# (offset array, pieces per record, arrays that share the offsets) in hipstr_trace_dev_sizes' order
POOLS = [("hap_aln_off", 1, ("hap_aln",)), ("str_seq_off", 1, ("str_seq",)), ("flank_seq_off", 2, ("flank_seq",)), ("indel_off", 1, ("indel_pos", "indel_size")),
         ("snp_off", 1, ("snp_pos", "snp_base")), ("cigar_off", 1, ("cigar_op", "cigar_len")), ("aln_str_off", 1, ("aln_str",))]


class Setup:
    """The batch, its seeds (the oracle's: host only), the hap_to_ref strings (hipstr_hap_aln_info) and every (read, allele) pair that can be traced."""

    def __init__(self, hmm, oracle):
        self.sb = capi.SynthBatch(**BATCH)
        self.ptr = self.sb.ptr
        _, self.seeds = capi.run_align(oracle, "oracle_", self.ptr)
        self.A = self.sb.n_out // self.sb.n_reads
        self.pool_off = capi.batch_arrays(self.ptr)["read_off"].astype(np.int32)
        self.n_alleles = np.full(self.sb.n_loci, self.A, np.int32)
        self.h2r = capi.hap_aln_info(hmm, "hipstr_", self.ptr)
        self.reads = [r for r in range(self.sb.n_reads) if self.seeds[r] >= 0]
        assert len(self.reads) >= 70 and self.A == 4

    def requests(self, alleles, reads=None):
        """(req_read, req_allele): read-major, grouped by locus in locus order."""
        rs = self.reads if reads is None else reads
        return np.array([r for r in rs for _ in alleles], np.int32), np.array([k for _ in rs for k in alleles], np.int32)

    def close(self):
        self.sb.close()


def raw(a):
    return a.tobytes() if isinstance(a, np.ndarray) else a.raw


def fetch(hmm, td):
    """(n, totals, dict of hipstr_trace_dev_fetch(ALL))."""
    n, tot = td.sizes()
    return n, tot, capi.trace_dev_fetch(hmm, td, capi.TRACE_F_ALL)


def content(n, keep):
    """What a fetched handle holds, as bytes per array: scalars [n], offsets with their leading 0, pools up to their totals."""
    out = {}
    for nm in SCALARS:
        out[nm] = keep[nm][:n].tobytes()
    for off, per, arrays in POOLS:
        m = per * n + 1
        out[off] = keep[off][:m].tobytes()
        total = int(keep[off][m - 1])
        for nm in arrays:
            a = keep[nm]
            out[nm] = a[:total].tobytes() if isinstance(a, np.ndarray) else a.raw[:total]
    return out


def reorder(sources, out_src, out_idx):
    """The gather in numpy.  sources: list of (n, keep) of fetched handles -> (totals[7], content dict) of the handle whose record q is record
    out_idx[q] of source out_src[q]."""
    n_out = len(out_src); out = {}; totals = []
    for nm in SCALARS:
        dt = np.float64 if nm == "ll" else np.int32
        out[nm] = np.array([sources[s][1][nm][i] for s, i in zip(out_src, out_idx)], dt).tobytes()
    for off, per, arrays in POOLS:
        offs = [0]; chunks = {nm: [] for nm in arrays}
        for s, i in zip(out_src, out_idx):
            k = sources[s][1]
            for f in range(per):
                a, b = int(k[off][per * i + f]), int(k[off][per * i + f + 1])
                offs.append(offs[-1] + b - a)
                for nm in arrays:
                    arr = k[nm]
                    chunks[nm].append(arr[a:b].tobytes() if isinstance(arr, np.ndarray) else arr.raw[a:b])
        assert len(offs) == per * n_out + 1
        out[off] = np.array(offs, np.int32).tobytes(); totals.append(offs[-1])
        for nm in arrays:
            out[nm] = b"".join(chunks[nm])
    return np.array(totals, np.int64), out


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], "%s: %s differs" % (what, k)


def handle_content(hmm, td):
    n, tot, keep = fetch(hmm, td)
    return n, tot, content(n, keep)


class Book:
    """The cache in numpy: keys (locus, pool, haplotype) -> the record's content as it was first traced, plus the counts hipstr_trace_cache_stats_t reports."""

    def __init__(self, pool_off, n_alleles):
        self.pool_off = np.asarray(pool_off); self.A = list(n_alleles)
        self.keys = {}; self.n_records = 0; self.n_segments = 0

    def locus(self, r):
        return int(np.searchsorted(self.pool_off, r, side="right")) - 1

    def key(self, r, a):
        l = self.locus(r)
        return (l, int(r - self.pool_off[l]), int(a))

    def round(self, rr, aa, takes=None):
        """-> (missed requests' indices, n_inserted): what a round must trace, in order of first occurrence."""
        seen = set(); miss = []
        for q, (r, a) in enumerate(zip(rr, aa)):
            k = self.key(r, a)
            if k not in self.keys and k not in seen:
                seen.add(k); miss.append(q)
        ins = [q for q in miss if takes is None or takes[self.locus(rr[q])]]
        for q in ins:
            self.keys[self.key(rr[q], aa[q])] = None
        if ins:
            self.n_records += len(miss); self.n_segments += 1
        dead = self.n_records - len(self.keys)                         # trace_cache_layout.h: hs_tc_should_compact, restated
        if self.n_segments > MAX_SEGMENTS or (dead >= COMPACT_MIN_DEAD and dead > len(self.keys)):
            self.compact()
        return miss, len(ins)

    def remap(self, new_A, mapping):
        base = np.concatenate([[0], np.cumsum(self.A)])
        nxt = {}
        for (l, p, h), v in self.keys.items():
            m = int(mapping[base[l] + h])
            if m != -1:
                nxt[(l, p, m)] = v
        self.keys = nxt; self.A = list(new_A)

    def clear(self, locus=None):
        self.keys = {k: v for k, v in self.keys.items() if locus is not None and not locus[k[0]]}
        if not self.keys:
            self.n_records = 0; self.n_segments = 0

    def compact(self):
        self.n_records = len(self.keys); self.n_segments = 1 if self.keys else 0

    def entries(self):
        ks = sorted(self.keys)
        return (np.array([self.pool_off[l] + p for l, p, _ in ks], np.int32), np.array([h for _, _, h in ks], np.int32))

    def state(self):
        return dict(n_segments=self.n_segments, n_live=len(self.keys), n_dead=self.n_records - len(self.keys))
