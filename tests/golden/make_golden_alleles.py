"""Writes tests/golden/alleles_<batch>.npz: for every batch of tests/alleles_cases.py the case text (per locus the three blocks, the options
to remove and the strings to add) and the records the REFERENCE's own HapBlock / RepeatBlock / Haplotype give for it — the old haplotype
strings in reset() / next() order, the blocks after remove_alleles and add_alternate, the new haplotype strings in visit order — produced by
`genotype_flow --allele-cases` (integration/genotype_flow.cpp, built by `make -C oracle flow` where the reference tree exists).  Data only.

    python tests/golden/make_golden_alleles.py            # every batch
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alleles_cases as ac  # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")


def reference_records(text):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "records.txt")
        with open(src, "w") as f:
            f.write(text)
        subprocess.run([os.path.join(REFDIR, "flow_launcher"), os.path.join(REFDIR, "libflow_ref.so"), "--allele-cases", src, "--out", dst], check=True)
        with open(dst) as f:
            return f.read()


def main():
    for name, make in sorted(ac.BATCHES.items()):
        cases = make()
        text = ac.case_text(cases)
        assert [(c["blocks"], c["remove"], c["add"]) for c in ac.parse_cases(text)] == [(c["blocks"], c["remove"], c["add"]) for c in cases]
        records = reference_records(text)
        recs = ac.parse_records(records)
        assert list(recs) == [c["name"] for c in cases]
        out = os.path.join(HERE, "alleles_%s.npz" % name)
        np.savez_compressed(out, cases=np.frombuffer(text.encode(), np.uint8), records=np.frombuffer(records.encode(), np.uint8))
        print("%s: %d cases, %d bytes" % (out, len(cases), os.path.getsize(out)))


if __name__ == "__main__":
    main()
