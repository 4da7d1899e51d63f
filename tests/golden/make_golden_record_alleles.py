"""Writes tests/golden/record_alleles_<batch>.npz: what the compiled reference's SeqStutterGenotyper::get_alleles and reorder_alleles
return on the cases of tests/record_alleles_cases.py, through `genotype_flow --record-cases` (integration/genotype_flow.cpp, built by
`make -C oracle flow` where the reference tree exists).  The fixtures hold the driver's output text only; the inputs follow from the
makers.  Data only.

    python tests/golden/make_golden_record_alleles.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import record_alleles_cases as ac  # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")


def main():
    for batch, make in ac.BATCHES.items():
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "out.txt")
            with open(src, "w", encoding="latin-1") as f:
                f.write(ac.cases_text(make()))
            subprocess.run([os.path.join(REFDIR, "flow_launcher"), os.path.join(REFDIR, "libflow_ref.so"), "--record-cases", src, "--out", dst], check=True)
            text = open(dst, "rb").read()
        assert len(ac.parse_results(text.decode("latin-1"))) == len(make())
        np.savez_compressed(ac.GOLDEN[batch], text=np.frombuffer(text, np.uint8))
        print("wrote", ac.GOLDEN[batch], os.path.getsize(ac.GOLDEN[batch]), "bytes")


if __name__ == "__main__":
    main()
