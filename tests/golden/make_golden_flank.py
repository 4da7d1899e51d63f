"""Writes tests/golden/flank_<batch>.npz: for every batch of tests/flank_cases.py the case text (one case per (locus, flank): ref_seq, every
sample's strings, the parameters) and the records the REFERENCE's own DebruijnGraph gives for it — calc_kmer_length's result and, per task,
k, the paths in enumerate_paths' order and their weights — produced by `genotype_flow --debruijn-cases` (integration/genotype_flow.cpp,
built by `make -C oracle flow` where the reference tree exists).  Data only.

    python tests/golden/make_golden_flank.py            # every batch
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import flank_cases as fc      # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")


def main():
    for name, make in sorted(fc.BATCHES.items()):
        c = fc.build(make())
        text = fc.case_text(c)
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "records.txt")
            with open(src, "w") as f:
                f.write(text)
            subprocess.run([os.path.join(REFDIR, "flow_launcher"), os.path.join(REFDIR, "libflow_ref.so"), "--debruijn-cases", src, "--out", dst], check=True)
            with open(dst) as f:
                records = f.read()
        fc.parse_records(records)
        out = os.path.join(HERE, "flank_%s.npz" % name)
        np.savez_compressed(out, cases=np.frombuffer(text.encode(), np.uint8), records=np.frombuffer(records.encode(), np.uint8))
        print("%s: %d cases, %d bytes" % (out, text.count("case "), os.path.getsize(out)))


if __name__ == "__main__":
    main()
