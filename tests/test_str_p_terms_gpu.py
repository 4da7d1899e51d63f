"""GPU: the 13-term evaluation of hs_str_group_kernel_p (two terms in flight per lane: the table values of term k + 1 are requested under
the additions of term k) on the batches of tests/str_p_terms_cases.py, bit for bit against the oracle — one-shot and two resident passes
on one upload; the route of every batch asserted from the launch plan, so that no case passes through another kernel.  One case runs
with HIPSTR_DEBUG_REDO in a child process (the re-do mark path: every third chunk of columns is left to hs_str_kernel_generic)."""
import os
import subprocess
import sys

import pytest

import str_p_terms_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,P", sc.CASES, ids=["%s_p%d" % c for c in sc.CASES])
def test_terms_against_the_oracle(hmm, oracle, kind, P):
    assert sc.check_device(hmm, oracle, kind, P) > 0


def test_redo_mark_path_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIPSTR_DEBUG_REDO="3", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(here, "str_p_terms_cases.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "redo ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
