"""Writes tests/golden/record_pvalues.npz: the AB and FS values of the reference's own routines — cephes' bdtr and htslib's
kt_fisher_exact, compiled where they lie in the HipSTR tree into a temporary directory — on the inputs of tests/record_cases.py.
The fixture holds results only, as uint64 bit patterns; the inputs follow from the index rules there.

    python tests/golden/make_record_golden.py /path/to/HipSTR
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import record_cases as rc  # noqa: E402

CEPHES = "bdtr.c incbet.c incbi.c ndtri.c gamma.c mtherr.c const.c polevl.c isnan.c unity.c".split()

# The driver: compute_allele_bias (seq_stutter_genotyper.cpp:965-982) and :1371-1374 around the two routines, declared by prototype.
DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
double bdtr(int k, int n, double p);
double kt_fisher_exact(int n11, int n12, int n21, int n22, double* left, double* right, double* two);
int main(void){
  int a, b, r1, r2;
  while (scanf("%d %d %d %d", &a, &b, &r1, &r2) == 4){
    double ab, l, r, two, fs, pv;
    unsigned long long x, y;
    if (a + b == 0) ab = 1; else if (a == b) ab = 0.0; else { pv = 2*bdtr(a < b ? a : b, a + b, 0.5); ab = log10(pv < 1.0 ? pv : 1.0); }
    kt_fisher_exact(a - r1, r1, b - r2, r2, &l, &r, &two);
    fs = log10(two < 1.0 ? two : 1.0);
    memcpy(&x, &ab, 8); memcpy(&y, &fs, 8);
    printf("%llx %llx\n", x, y);
  }
  return 0;
}
"""


def run(exe, u1, u2, r1, r2):
    text = "".join("%d %d %d %d\n" % q for q in zip(u1.tolist(), u2.tolist(), r1.tolist(), r2.tolist()))
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split()
    v = np.array([int(x, 16) for x in out], np.uint64).reshape(-1, 2)
    assert len(v) == len(u1)
    return v[:, 0].copy(), v[:, 1].copy()


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "config.h"), "w").close()
        with open(os.path.join(tmp, "driver.c"), "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.run(["gcc", "-O2", "-w", "-I", tmp, "-I", os.path.join(ref, "lib", "htslib"), "-o", exe, os.path.join(tmp, "driver.c")] +
                       [os.path.join(ref, "lib", "cephes", c) for c in CEPHES] + [os.path.join(ref, "lib", "htslib", "kfunc.c"), "-lm"], check=True)
        a1, a2 = rc.ab_small()
        z = np.zeros_like(a1)
        ab_small, _ = run(exe, a1, a2, z, z)
        _, fs_small = run(exe, *rc.fs_small())
        ab_large, fs_large = run(exe, *rc.large())
    np.savez_compressed(rc.GOLDEN, ab_small=ab_small, fs_small=fs_small, ab_large=ab_large, fs_large=fs_large)
    print("wrote", rc.GOLDEN, os.path.getsize(rc.GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HIPSTR_REFERENCE", ""))
