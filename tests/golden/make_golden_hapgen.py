"""Writes tests/golden/hapgen_<batch>.npz: for every batch of tests/hapgen_cases.py the case text (per locus the chromosome, the region and
every read) and the records the REFERENCE's own HaplotypeGenerator gives for it — the status / failure_msg() and the three blocks after
fuse_haplotype_blocks — produced by `genotype_flow --hapgen-cases` (integration/genotype_flow.cpp, built by `make -C oracle flow` where the
reference tree exists).  Data only.

    python tests/golden/make_golden_hapgen.py            # every batch
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import hapgen_cases as hc      # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")


def reference_records(text, extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "records.txt")
        with open(src, "w") as f:
            f.write(text)
        subprocess.run([os.path.join(REFDIR, "flow_launcher"), os.path.join(REFDIR, "libflow_ref.so"), "--hapgen-cases", src, "--out", dst] + list(extra), check=True)
        with open(dst) as f:
            return f.read()


def main():
    for name, make in sorted(hc.BATCHES.items()):
        loci = make()
        text = hc.case_text(loci)
        records = reference_records(text)
        recs = hc.parse_records(records)
        assert list(recs) == [lc["name"] for lc in loci]
        out = os.path.join(HERE, "hapgen_%s.npz" % name)
        np.savez_compressed(out, cases=np.frombuffer(text.encode(), np.uint8), records=np.frombuffer(records.encode(), np.uint8))
        print("%s: %d cases, %d bytes" % (out, len(loci), os.path.getsize(out)))


if __name__ == "__main__":
    main()
