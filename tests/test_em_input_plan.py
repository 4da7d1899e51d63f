"""CPU: the size decisions of hipstr_em_train_dev's preparation (hipstr_amd/csrc/em_input_layout.h) as hipstr_debug_em_input_plan reports
them, on either side of every limit: a run of a wavefront's 64 reads +- 1, the scan's chunk of runs +- 1, the presence bitmap's span
limit +- 1 (and its word edges), the allele count beyond which the initial frequencies are left to the host's refusal.  The expected
values are worked out here from the limits the plan reports, which are themselves pinned to the header's text."""
import os
import re

import pytest

from hipstr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_limits():
    src = open(os.path.join(ROOT, "hipstr_amd", "csrc", "em_input_layout.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (HS_EMI_[A-Z_]+) (\d+)\b", src, re.M)}


def test_limits_are_the_headers(hmm_host):
    p = capi.em_input_plan(hmm_host, 1, 1, 0, 0, 1)
    hdr = _header_limits()
    for k, v in p["thresholds"].items():
        assert hdr[k] == v, k
    assert p["thresholds"] == dict(HS_EMI_THREADS=256, HS_EMI_WAVE=64, HS_EMI_SCAN_CHUNK=256, HS_EMI_SPAN_LIMIT=10000)
    # the span limit is the length of the table of integer logarithms hipstr_em_train refuses by (hipstr_debug_em_plan reports it)
    ep = capi.em_plan(hmm_host, period=[2], n_samples=[1], read_off=[0, 1], sample_label=[0], num_bps=[2], log_p1=[0.0], log_p2=[0.0])
    assert ep["thresholds"]["int_log_len"] == p["thresholds"]["HS_EMI_SPAN_LIMIT"]


@pytest.mark.parametrize("reads", [0, 1, 63, 64, 65, 127, 128, 129])
def test_run_steps(hmm_host, reads):
    p = capi.em_input_plan(hmm_host, 1, reads, 0, 0, 1)
    W = p["thresholds"]["HS_EMI_WAVE"]
    assert p["run_steps"] == -(-reads // W)
    assert p["last_step"] == (0 if reads == 0 else reads - (p["run_steps"] - 1) * W)
    assert 0 <= p["last_step"] <= W and (reads == 0 or p["last_step"] >= 1)


@pytest.mark.parametrize("runs", [0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513])
def test_scan_chunks_and_workgroups(hmm_host, runs):
    p = capi.em_input_plan(hmm_host, runs, 1, 0, 0, 1)
    CH = p["thresholds"]["HS_EMI_SCAN_CHUNK"]; per_wg = p["thresholds"]["HS_EMI_THREADS"] // 64
    assert p["scan_chunks"] == -(-runs // CH)
    assert p["scan_last_chunk"] == (0 if runs == 0 else runs - (p["scan_chunks"] - 1) * CH)
    assert p["run_workgroups"] == -(-runs // per_wg)


@pytest.mark.parametrize("lo", [0, -17, 5000])
def test_bitmap_span_limit(hmm_host, lo):
    L = capi.em_input_plan(hmm_host, 1, 1, 0, 0, 1)["thresholds"]["HS_EMI_SPAN_LIMIT"]
    for span, dev in ((0, True), (31, True), (32, True), (L - 2, True), (L - 1, True), (L, False), (L + 1, False), (2**31 - 1, False)):
        p = capi.em_input_plan(hmm_host, 1, 1, lo, lo + span, 2)
        assert p["device"] is dev, span
        assert p["bitmap_words"] == (span // 32 + 1 if dev else 0), span
    # the largest bitmap fits the header's LDS array
    assert capi.em_input_plan(hmm_host, 1, 1, lo, lo + L - 1, 2)["bitmap_words"] == (L + 31) // 32


def test_allele_count_limit(hmm_host):
    L = capi.em_input_plan(hmm_host, 1, 1, 0, 0, 1)["thresholds"]["HS_EMI_SPAN_LIMIT"]
    # hipstr_em_train refuses A + 1 >= the table's length: the device evaluates the frequencies for every count below that
    for A, dev in ((1, True), (L - 3, True), (L - 2, True), (L - 1, False), (L, False)):
        assert capi.em_input_plan(hmm_host, 1, 1, 0, L - 1, A)["device_priors"] is dev, A
    assert capi.em_input_plan(hmm_host, 1, 1, 0, L, 2)["device_priors"] is False          # no bitmap: nothing is evaluated there


def test_refused_arguments(hmm_host):
    for a in ((-1, 1, 0, 0, 1), (1, -1, 0, 0, 1), (1, 1, 1, 0, 1), (1, 1, 0, 0, 0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            capi.em_input_plan(hmm_host, *a)
