"""Generates tests/golden/pool_*.npz (not pool_scatter_*: those are make_golden.py's) by running three one-locus batches of un-pooled reads
through the COMPILED REFERENCE's ReadPooler (ref_pool of oracle/_ref/libhipstr_ref.so).  Run where the reference is built only:
python tests/golden/make_golden_pool.py
Each fixture holds the batch's arrays and the reference's pool_index, n_pools, pool_quals and pool_qual_off; nothing of the reference's
source is stored.

  pool_many_members   300 reads of 40 bases drawn from 12 sequences: pools of tens of members, odd and even sizes
  pool_near_identical sequences that differ in the first base, in the last base, or by one trailing base
  pool_wide_quals     qualities over the whole printable range '!' .. '~'"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from hipstr_amd import capi   # noqa: E402
import pool_cases as pc       # noqa: E402
from util import batch_to_dict   # noqa: E402


def cases():
    rng = np.random.default_rng(20261019)
    seqs = [pc.rand_seq(rng, 40) for _ in range(12)]
    phred = lambda r, n: pc.rand_qual(r, n, 35, 73)
    many = [(seqs[i], phred(rng, 40)) for i in rng.choice(12, size=300, p=np.arange(1, 13) / 78.0)]
    base = pc.rand_seq(rng, 60)
    flip = lambda c: b"ACGT"[(b"ACGT".index(c) + 1) % 4:][:1]
    near = [base, flip(base[:1]) + base[1:], base[:-1] + flip(base[-1:]), base[:-1], base + b"A", base + b"C", base[1:]]
    near_reads = [(near[i], phred(rng, len(near[i]))) for i in rng.integers(0, len(near), 90)]
    wide = [(seqs[i], pc.rand_qual(rng, 40)) for i in rng.integers(0, 5, 120)]
    return dict(many_members=many, near_identical=near_reads, wide_quals=wide)


def main():
    ref = capi.load_ref()
    ref.ref_pool.restype = C.c_int; ref.ref_pool.argtypes = [capi._BP, capi._i32p, capi._i32p, C.c_char_p, capi._i32p, C.c_int32]
    for name, reads in cases().items():
        b = pc.batch_of([reads])
        R = len(reads)
        pool_index = np.zeros(R, np.int32); n_pools = np.zeros(1, np.int32); cap = 1 << 20
        pq = C.create_string_buffer(cap); pqo = np.zeros(R + 1, np.int32)
        assert ref.ref_pool(b.ptr, pool_index.ctypes.data_as(capi._i32p), n_pools.ctypes.data_as(capi._i32p), pq, pqo.ctypes.data_as(capi._i32p), cap) == 0
        P = int(n_pools[0])
        d = batch_to_dict(b)
        d.update(expect_pool_index=pool_index, expect_n_pools=n_pools, expect_pool_quals=np.frombuffer(pq.raw[:pqo[P]], np.uint8).copy(),
                 expect_pool_qual_off=pqo[:P + 1])
        np.savez_compressed(os.path.join(HERE, "pool_%s.npz" % name), **d)
        print("pool", name, "reads", R, "pools", P, "largest", int(np.bincount(pool_index).max()))


if __name__ == "__main__":
    main()
