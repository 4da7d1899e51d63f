"""Writes tests/golden/record_reads_cigars.npz and record_reads_histograms.npz: what the reference's own ExtractCigar
(extract_indels.cpp, compiled where it lies in the HipSTR tree into a temporary directory) and Genotyper::condense_read_counts
(genotyper.h, opened with `#define protected public`) return on the cases of tests/record_reads_cases.py.  The fixtures hold results only:
got / bp_diff per read, and the condensed strings of all samples as one text, a line each; the inputs follow from the makers there.

    python tests/golden/make_golden_record_reads.py /path/to/HipSTR
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import record_reads_cases as rc  # noqa: E402

# The driver: a line "C start region_start region_end n (op len)*" -> "got bp_diff" (bp_diff as the call left it, preset to 0);
# a line "H n (value)*" -> the condensed string.  condense_read_counts reads no member: it is called on raw storage of the class' size.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#define protected public
#include "genotyper.h"
#undef protected
#include "extract_indels.h"
int main(){
  std::string kind;
  void* mem = calloc(1, sizeof(Genotyper));
  while (std::cin >> kind){
    if (kind == "C"){
      int start, rs, re, n;
      std::cin >> start >> rs >> re >> n;
      std::vector<CigarOp> ops;
      for (int i = 0; i < n; i++){ char t; int len; std::cin >> t >> len; ops.push_back(CigarOp(t, len)); }
      int bp = 0;
      const bool got = ExtractCigar(ops, start, rs, re, bp);
      printf("%d %d\n", got ? 1 : 0, bp);
    } else {
      int n;
      std::cin >> n;
      std::vector<int> v(n);
      for (int i = 0; i < n; i++) std::cin >> v[i];
      printf("%s\n", ((Genotyper*)mem)->condense_read_counts(v).c_str());
    }
  }
  return 0;
}
"""


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.run(["g++", "-O1", "-w", "-std=c++11", "-I", os.path.join(ref, "src"), "-I", os.path.join(ref, "lib", "htslib"), "-I", os.path.join(ref, "lib"),
                        "-o", exe, os.path.join(tmp, "driver.cpp"), os.path.join(ref, "src", "extract_indels.cpp")], check=True)
        run = lambda text: subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()
        loci = rc.cigar_loci()
        lines = run(rc.cigar_text(loci))
        assert len(lines) == sum(len(l[3]) for l in loci)
        v = np.array([[int(x) for x in line.split()] for line in lines], np.int64).reshape(-1, 2)
        hist = run(rc.histogram_text(rc.histogram_loci()))
        assert len(hist) == sum(len(l) for l in rc.histogram_loci())
    np.savez_compressed(rc.GOLDEN_CIGARS, got=v[:, 0].astype(np.uint8), bp_diff=v[:, 1].astype(np.int32))
    np.savez_compressed(rc.GOLDEN_HISTOGRAMS, condensed=np.frombuffer("\n".join(hist).encode(), np.uint8))
    for p in (rc.GOLDEN_CIGARS, rc.GOLDEN_HISTOGRAMS):
        print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HIPSTR_REFERENCE", ""))
