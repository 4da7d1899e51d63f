"""The forward pass's launch routes and the size thresholds between them ("Routes and the cases that pin them").

Every case builds deterministic batches on the two or three sides of one threshold the library reports (hipstr_debug_launch_plan:
thresholds are read from the library, not copied, so the cases follow a retuned constant) and names the route it expects on each
side.  tests/test_routes.py checks the plan on the host, tests/test_routes_gpu.py runs the same batches on the device against the oracle.
"""
import collections
import contextlib
import os

import numpy as np

from hipstr_amd import capi
import util

Case = collections.namedtuple("Case", "name threshold deltas build observe expect env")
# build(lim, d) -> capi.Batch (finalized); observe(plan) -> (measured quantity, route); expect(lim, d) -> (quantity, route)
# env: environment the launches run under (the plan reads it too)


def lim_of(lib):
    """The library's thresholds and shapes (hipstr_debug_launch_plan of an empty batch)."""
    b = capi.Batch().finalize()
    return capi.launch_plan(lib, b.ptr)["thresholds"]


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n)) if n > 0 else ""


def add_locus(b, rng, lf=16, rf=16, strs=("CAG" * 10, "CAG" * 12), period=3, n_reads=1, read_len=None, lf_opts=(), rf_opts=()):
    """One locus: random flanks of lf / rf bases (the seed lands in the left flank when it is 16 bases long), STR options `strs`,
    n_reads reads of the reference haplotype's first read_len bases (all of it by default), qualities varying along the read.
    A flank of F bases is a rowset of F rows: F - 1 rows after the block's first row."""
    L, R = _seq(rng, lf), _seq(rng, rf)
    ref = L + strs[0] + R
    n = len(ref) if read_len is None else min(read_len, len(ref))
    reads = []
    for i in range(n_reads):
        q = "".join(chr(ord("5") + (7 * j + 3 * i) % 40) for j in range(n))
        reads.append((ref[:n], q, 0, True))
    util.simple_locus(L, list(strs), R, period, reads, batch=b, lf_opts=[_seq(rng, o) if isinstance(o, int) else o for o in lf_opts],
                      rf_opts=[_seq(rng, o) if isinstance(o, int) else o for o in rf_opts])
    return b


def _rng(tag):
    return np.random.default_rng(sum(map(ord, tag)) * 7919)


# ------------------------------------------------------------------ builders
def lead_items(n):
    """n leading-flank items (and as many trailing): single-read loci of two items each, plus one locus with two left-flank options
    (three of each) when n is odd."""
    rng, b = _rng("lead_items"), capi.Batch()
    for _ in range(n // 2 - (n & 1)):
        add_locus(b, rng, strs=("CAG" * 6,))
    if n & 1:
        add_locus(b, rng, strs=("CAG" * 6,), rf_opts=[16])
    return b.finalize()


def trail_items(n, long_read=False):
    """About n trailing-flank items and 2 leading: one locus of n / 2 reads and 40 alleles (a group of 40 takes a wavefront of its own
    per read and side: two items per read, so odd counts are not reachable and the nearest even ones stand in).  long_read: read
    sides above HS_SYS_MAXCOLS (the systolic form is out)."""
    rng, b = _rng("trail_items"), capi.Batch()
    add_locus(b, rng, strs=tuple("CAG" * k for k in range(4, 44)), n_reads=max(1, n // 2), rf=300 if long_read else 16)
    return b.finalize()


def lead_items_long(n):
    """n leading-flank items, read sides above HS_SYS_MAXCOLS (one locus with a 300-base right flank, read through)."""
    rng, b = _rng("lead_items_long"), capi.Batch()
    add_locus(b, rng, rf=300, strs=("CAG" * 6,))
    n -= 2
    for _ in range(n // 2 - (n & 1)):
        add_locus(b, rng, strs=("CAG" * 6,))
    if n & 1:
        add_locus(b, rng, strs=("CAG" * 6,), rf_opts=[16])
    return b.finalize()


def side_cols(cols, **kw):
    """One locus whose longest read side is `cols` columns: the read length that gives it is searched (the seed is the host's)."""
    lib = capi.load_hmm()
    for n, lf in ((n, lf) for n in range(int(cols * 1.5), int(cols * 2)) for lf in (16, 17, 18)):     # (the seed lands near the read's middle)
        rng, b = _rng("side_cols"), capi.Batch()
        add_locus(b, rng, lf=lf, rf=420, read_len=n, **kw)
        b.finalize()
        if capi.launch_plan(lib, b.ptr)["max_cols"] == cols:
            return b
    raise AssertionError("no read length gives a side of %d columns" % cols)


def deep_trail(rows, n_reads=65, elsewhere=False):
    """130 trailing-flank items (beyond the systolic and the latency shapes) whose longest flank rowset has `rows` rows: in the same
    locus, or (elsewhere) in a second one-read locus while the 130 items stay 17 rows deep — the limit is batch-wide."""
    rng, b = _rng("deep_trail"), capi.Batch()
    strs = tuple("CAG" * k for k in range(4, 44))
    add_locus(b, rng, strs=strs, n_reads=n_reads, lf=16 if elsewhere else max(rows, 16), rf=17 if elsewhere else rows)
    if elsewhere:
        add_locus(b, rng, strs=("CAG" * 6,), lf=16, rf=rows)
    return b.finalize()


def depths_for(R, W):
    """Flank rows (after the first) that reach every band height 1..R, every last-round band count 1..W and rounds 1..3: 0 (the single
    row), 1..W, k W for k = 1..R, R W +- 1, 2 R W +- 1, 3 R W — shallow -> deep -> shallow in launch order."""
    d = sorted(set([1, 2] + list(range(1, W + 1)) + [k * W for k in range(1, R + 1)] + [R * W - 1, R * W + 1, 2 * R * W - 1, 2 * R * W + 1, 3 * R * W]))
    deep = [x for x in d if x > W]
    return [0] + list(range(1, W + 1)) + deep + [W, 1, 0]


def bands_batch(R, W, tag, pad_items=0, max_rows=None):
    """One locus per depth of depths_for(R, W): left flank 16 bases (the seed), right flank depth + 1 bases (the trailing flank of the
    left side and the leading flank of the right side); pad_items extra single-read loci push the item count past a limit; max_rows:
    the depths the shape takes at most (the short trailing shape: one round)."""
    rng, b = _rng(tag), capi.Batch()
    for dpt in depths_for(R, W):
        if max_rows is not None and dpt > max_rows:
            continue
        add_locus(b, rng, strs=("CAG" * 6, "CAG" * 7), rf=dpt + 1)
    for _ in range(pad_items):
        add_locus(b, rng, strs=("CAG" * 6,))
    return b.finalize()


def str_block(period, length, breaks=0, n_loci=1):
    """Loci whose one STR allele is a block of `length` bases of a period-`period` motif with `breaks` interruptions spread over it."""
    rng, b = _rng("str_block%d" % period), capi.Batch()
    motif = "ACGTTGCAT"[:period] if period > 1 else "A"
    blk = list((motif * (length // period + 1))[:length])
    for i in range(breaks):
        at = (i + 1) * length // (breaks + 1)
        at -= at % period
        blk[at] = "T" if blk[at] != "T" else "G"
    blk = "".join(blk)
    for _ in range(n_loci):
        add_locus(b, rng, strs=(blk,), period=period, read_len=120)
    return b.finalize()


def str_items(n):
    """About n STR items with interrupted alleles: single-read loci of two items each (odd counts unreachable: the nearest even ones)."""
    rng, b = _rng("str_items"), capi.Batch()
    blk = "CAG" * 5 + "CTG" + "CAG" * 5
    for _ in range(max(1, n // 2)):
        add_locus(b, rng, strs=(blk,))
    return b.finalize()


def flank_bases(n, lead=None):
    """One locus whose alleles have n flank bases (n_flank: leading + trailing flank of the left side); lead = bases of the left flank."""
    rng, b = _rng("flank_bases"), capi.Batch()
    lf = lead if lead is not None else max(16, n // 2)
    add_locus(b, rng, lf=lf, rf=n - lf, strs=("CAG" * 6, "CAG" * 8))
    return b.finalize()


def packed_reads(cols):
    """One locus, two reads whose left sides (seed to read start) have `cols` columns together: the second read's length is searched."""
    lib = capi.load_hmm()
    for n2 in range(100, 420):
        rng, b = _rng("packed_reads"), capi.Batch()
        L, R = _seq(rng, 16), _seq(rng, 420)
        strs = ["CAG" * 10, "CAG" * 12]
        ref = L + strs[0] + R
        reads = [(ref[:n], "".join(chr(ord("5") + (7 * j + 3 * i) % 40) for j in range(n)), 0, True) for i, n in enumerate((200, n2))]
        util.simple_locus(L, strs, R, 3, reads, batch=b)
        b.finalize()
        seeds = np.zeros(2, np.int32)
        assert lib.hipstr_calc_seed_bases(b.ptr, seeds.ctypes.data_as(capi._i32p)) == 0
        if int(seeds.sum()) == cols:
            return b
    raise AssertionError("no read length gives %d columns" % cols)


def list_breaks(k):
    """One locus whose allele is a 240-base period-4 block with k breaks in each visiting list: an interruption inside the block breaks a
    list's upstream match runs twice (at itself and one shift behind it), one in the block's first repeat unit once."""
    rng, b = _rng("list_breaks"), capi.Batch()
    blk = list(("ACGT" * 61)[:240])
    m = k // 2
    for i in range(m):
        at = (i + 1) * 240 // (m + 1)
        at -= at % 4
        blk[at] = "G"
    if k % 2:
        blk[1] = "T"
    # (the breaks of the insertion list: bases that differ from the base one period upstream)
    assert sum(blk[j] != blk[j - 4] for j in range(4, 240)) == k
    add_locus(b, rng, strs=("".join(blk),), period=4, read_len=120)
    return b.finalize()


def chunked():
    return capi.SynthBatch(n_loci=1, reads_per_locus=300, n_str_alleles=8, seed=3)


# ------------------------------------------------------------------ what a plan shows
def flank(which):
    return lambda p: (p["chunks"][0][which]["items"], p["chunks"][0][which]["route"])


def str_pairs(kernel):
    return lambda p: sum(c["str"]["pairs"][kernel] for c in p["chunks"])


def str_route(p):
    """The STR kernel that takes the batch's (read side, allele) pairs, when exactly one does."""
    ks = {k for c in p["chunks"] for k, v in c["str"]["pairs"].items() if v > 0}
    return ks.pop() if len(ks) == 1 else "/".join(sorted(ks))


def long_sides(p):
    c = p["chunks"][0]
    long_pairs = c["str"]["pairs"]["hs_str_kernel_long"]
    assert (c["str"]["n_long_sides"] > 0) == (long_pairs > 0), c["str"]
    return p["max_cols"], "hs_str_kernel_long" if c["str"]["n_long_sides"] > 0 else "hs_str_group_kernel_p"


def packing(p):
    """Columns of the locus' left-side reads and whether one workgroup of the grouped STR kernels takes them."""
    g = [x for x in p["chunks"][0]["str"]["groups"] if x[0] == 0]
    return sum(x[1] for x in g), {1: "one_group", 2: "two_groups"}.get(len(g), "%d groups" % len(g))


def list_form(p):
    """The form hs_str_group_kernel_rp evaluates the interrupted lists in, when it is one form."""
    s = p["chunks"][0]["str"]
    assert str_route(p) == "hs_str_group_kernel_rp", s["pairs"]
    forms = {k for k in ("pwk", "replay") if s["lists"][k] > 0}
    return None, {"pwk": "rp_list_closed_form", "replay": "rp_list_replay"}.get(forms.pop()) if len(forms) == 1 else "/".join(sorted(forms))


def combine_route(p):
    t = [i for i, v in enumerate(p["chunks"][0]["combine"]) if v > 0]
    assert len(t) == 1, p["chunks"][0]["combine"]
    return "combine_one" if t[0] == 0 else "combine_%d" % t[0]


def _cases():
    nf = lambda lim: lim["HS_CMB_MAX_FLANK"] // 64
    cs = [
        Case("lead_items_systolic", "HS_SYS_ITEMS", (-1, 0, 1), lambda lim, d: lead_items(lim["HS_SYS_ITEMS"] + d), flank("lead"),
             lambda lim, d: (lim["HS_SYS_ITEMS"] + d, "lead_systolic" if d <= 0 else "lead_latency"), {}),
        Case("trail_items_systolic", "HS_SYS_ITEMS", (-2, 0, 2), lambda lim, d: trail_items(lim["HS_SYS_ITEMS"] + d), flank("trail"),
             lambda lim, d: (lim["HS_SYS_ITEMS"] + d, "trail_systolic" if d <= 0 else "trail_latency"), {}),
        Case("lead_items_latency", "HS_LAT_ITEMS", (-1, 0, 1), lambda lim, d: lead_items_long(lim["HS_LAT_ITEMS"] + d), flank("lead"),
             lambda lim, d: (lim["HS_LAT_ITEMS"] + d, "lead_latency" if d <= 0 else "lead_default"), {}),
        Case("trail_items_latency", "HS_LAT_ITEMS", (-2, 0, 2), lambda lim, d: trail_items(lim["HS_LAT_ITEMS"] + d, long_read=True),
             flank("trail"), lambda lim, d: (lim["HS_LAT_ITEMS"] + d, "trail_latency" if d <= 0 else "trail_default"), {}),
        Case("side_cols_systolic", "HS_SYS_MAXCOLS", (-1, 0, 1), lambda lim, d: side_cols(lim["HS_SYS_MAXCOLS"] + d),
             lambda p: (p["max_cols"], p["chunks"][0]["lead"]["route"] + "+" + p["chunks"][0]["trail"]["route"]),
             lambda lim, d: (lim["HS_SYS_MAXCOLS"] + d, "lead_systolic+trail_systolic" if d <= 0 else "lead_latency+trail_latency"), {}),
        # (the quantity: rows after the first of the batch's longest flank rowset, 35/36/37 for a limit of 36)
        Case("trail_rows_short", "HS_SHORT_TRAIL_ROWS", (-1, 0, 1), lambda lim, d: deep_trail(lim["HS_SHORT_TRAIL_ROWS"] + d + 1),
             lambda p: (p["max_rows"] - 1, p["chunks"][0]["trail"]["route"]),
             lambda lim, d: (lim["HS_SHORT_TRAIL_ROWS"] + d, "trail_short" if d <= 0 else "trail_default"), {}),
        # a deep flank in another locus moves the 130 items of 16 rows to the default shape too: the limit is batch-wide.  The deep rowset
        # cannot belong to leading-flank items only: prep gives every flank option of a realigned allele to the leading flank of one side
        # and the trailing flank of the other, with the same number of rows (a flank of F bases is F rows either way), so the deepest
        # rowset of a batch always has trailing items too — here the second locus' one-read items
        Case("trail_rows_elsewhere", "HS_SHORT_TRAIL_ROWS", (0, 1), lambda lim, d: deep_trail(lim["HS_SHORT_TRAIL_ROWS"] + d + 1, elsewhere=True),
             lambda p: (p["max_rows"] - 1, p["chunks"][0]["trail"]["route"]),
             lambda lim, d: (lim["HS_SHORT_TRAIL_ROWS"] + d, "trail_short" if d <= 0 else "trail_default"), {}),
        # STR block
        Case("str_period", "HS_GRP_MAXP", (0, 1), lambda lim, d: str_block(lim["HS_GRP_MAXP"] + d, 60), lambda p: (None, str_route(p)),
             lambda lim, d: (None, "hs_str_group_kernel_p" if d <= 0 else "hs_str_group_kernel"), {}),
        Case("str_block_periodic", "HS_GRP_MAX_BLOCK", (0, 1), lambda lim, d: str_block(4, lim["HS_GRP_MAX_BLOCK"] + d),
             lambda p: (None, str_route(p)), lambda lim, d: (None, "hs_str_group_kernel_p"), {}),
        Case("str_block_period7", "HS_GRP_MAX_BLOCK", (0, 1), lambda lim, d: str_block(lim["HS_GRP_MAXP"] + 1, lim["HS_GRP_MAX_BLOCK"] + d),
             lambda p: (None, str_route(p)), lambda lim, d: (None, "hs_str_group_kernel" if d <= 0 else "hs_str_kernel_generic"), {}),
        Case("str_block_one_break", "HS_GRP_MAX_BLOCK", (0, 1), lambda lim, d: str_block(4, lim["HS_GRP_MAX_BLOCK"] + d, breaks=1),
             lambda p: (None, str_route(p)), lambda lim, d: (None, "hs_str_group_kernel_pw" if d <= 0 else "hs_str_kernel_generic"), {}),
        Case("str_block_three_breaks", "HS_GRP_MAX_BLOCK", (0, 1), lambda lim, d: str_block(4, lim["HS_GRP_MAX_BLOCK"] + d, breaks=3),
             lambda p: (None, str_route(p)), lambda lim, d: (None, "hs_str_group_kernel_rp" if d <= 0 else "hs_str_kernel_generic"), {}),
        # (the route as prep decided it: the chunk's count of read sides too long for a group, which the pair counts must agree with)
        Case("str_side_cols", "HS_GRP_COLS", (0, 1), lambda lim, d: side_cols(lim["HS_GRP_COLS"] + d), long_sides,
             lambda lim, d: (lim["HS_GRP_COLS"] + d, "hs_str_group_kernel_p" if d <= 0 else "hs_str_kernel_long"), {}),
        # one locus side whose two reads have 255 / 256 / 257 columns together: one workgroup of the grouped kernels, or two
        Case("str_group_packing", "HS_GRP_COLS", (-1, 0, 1), lambda lim, d: packed_reads(lim["HS_GRP_COLS"] + d), packing,
             lambda lim, d: (lim["HS_GRP_COLS"] + d, "one_group" if d <= 0 else "two_groups"), {}),
        # visiting lists with HS_PWK_MAX - 1 / HS_PWK_MAX / HS_PWK_MAX + 1 breaks: the K-level closed form of hs_str_group_kernel_rp, or
        # the list replayed entry by entry (both in hs_str_group_kernel_rp)
        Case("str_list_breaks", "HS_PWK_MAX", (-1, 0, 1), lambda lim, d: list_breaks(lim["HS_PWK_MAX"] + d), list_form,
             lambda lim, d: (None, "rp_list_closed_form" if d <= 0 else "rp_list_replay"), {}),
        Case("str_items_side_stream", "HS_SIDE_STREAM_ITEMS", (-2, 0, 2), lambda lim, d: str_items(lim["HS_SIDE_STREAM_ITEMS"] + d),
             lambda p: (p["chunks"][0]["str"]["items"], "str_side_stream" if p["chunks"][0]["str"]["side_stream"] else "str_chunk_stream"),
             lambda lim, d: (lim["HS_SIDE_STREAM_ITEMS"] + d, "str_side_stream" if d <= 0 else "str_chunk_stream"), {}),
        Case("str_per_read", "HIPSTR_STR_GROUP", (0,), lambda lim, d: str_block(3, 30), lambda p: (None, str_route(p)),
             lambda lim, d: (None, "hs_str_kernel"), {"HIPSTR_STR_GROUP": "0"}),
        # combine: every tier boundary below.  (The per-allele form for an empty leading or trailing flank has no case: prep refuses an
        # empty flank sequence, "empty flank sequence", so no batch reaches it.)
        Case("plan_chunks", "HIPSTR_WS_GIB", (0, 1), lambda lim, d: chunked(),
             lambda p: (None, p["chunks"][0]["routes"][0]), lambda lim, d: (None, "plan_one_chunk" if d <= 0 else "plan_chunks"), None),
    ]
    for t in (1, 2, 3, 4):
        cs.append(Case("combine_tier%d" % t, "64*%d" % t, (-1, 0, 1),
                       (lambda t: lambda lim, d: flank_bases(64 * t + d))(t), lambda p: (None, combine_route(p)),
                       (lambda t: lambda lim, d: (None, ("combine_%d" % t) if d <= 0 else
                                                  ("combine_%d" % (t + 1) if t < nf(lim) else "combine_one")))(t), {}))
    # band structure: one batch per coop shape (systolic: 63/64/65 and 128/129 rows) — thresholds of its own: the shape's R x W
    cs += [
        Case("bands_lead_latency", "R*W lead_latency", (0,), lambda lim, d: bands_batch(*lim["shapes"]["lead_latency"], "bll"),
             flank("lead"), lambda lim, d: (None, "lead_latency"), {"HIPSTR_FLANK_SYSTOLIC": "0"}),
        Case("bands_trail_latency", "R*W trail_latency", (0,), lambda lim, d: bands_batch(*lim["shapes"]["trail_latency"], "btl"),
             flank("trail"), lambda lim, d: (None, "trail_latency"), {"HIPSTR_FLANK_SYSTOLIC": "0"}),
        Case("bands_lead_default", "R*W lead_default", (0,), lambda lim, d: bands_batch(*lim["shapes"]["lead_default"], "bld", pad_items=70),
             flank("lead"), lambda lim, d: (None, "lead_default"), {}),
        Case("bands_trail_default", "R*W trail_default", (0,), lambda lim, d: bands_batch(*lim["shapes"]["trail_default"], "btd", pad_items=70),
             flank("trail"), lambda lim, d: (None, "trail_default"), {}),
        Case("bands_trail_short", "R*W trail_short", (0,), lambda lim, d: bands_batch(*lim["shapes"]["trail_short"], "bts", pad_items=70,
                                                                                   max_rows=lim["HS_SHORT_TRAIL_ROWS"]),
             flank("trail"), lambda lim, d: (None, "trail_short"), {}),
        Case("bands_systolic", "64 rows", (0,), lambda lim, d: systolic_bands(), flank("trail"), lambda lim, d: (None, "trail_systolic"), {}),
    ]
    return cs


def systolic_bands():
    rng, b = _rng("systolic_bands"), capi.Batch()
    for dpt in (1, 63, 64, 65, 128, 129, 2, 0):
        add_locus(b, rng, strs=("CAG" * 6, "CAG" * 7), rf=dpt + 1)
    return b.finalize()


CASES = _cases()
CHUNK_GIB = {0: None, 1: "0.001"}      # plan_chunks: the upload's own budget vs one that cuts the locus' 300 reads into three chunks


def case_env(case, d):
    if case.env is None:
        return {"HIPSTR_WS_GIB": CHUNK_GIB[d]} if CHUNK_GIB[d] else {}
    return case.env


def build(case, lim, d):
    return case.build(lim, d)
