"""Times the flank reassembly in its two forms on the same commit and the same batch, and counts the bytes that cross the host link:

  device   hipstr_flank_assemble_dev on the resident traceback result
  host     hipstr_trace_dev_fetch(HIPSTR_TRACE_F_FLANKS) + hipstr_flank_assemble

The batch: the six flank cases of tests/flow_chain_flanks.py run through the resident chain up to the flank step (tests/flow_chain_flanks.py's
device backend), then their flank inputs — posterior batch, pooled batch, seeds, requests, pool indices, flank strings — tiled to about 1000
loci and put back on the device (hipstr_post_upload, hipstr_debug_trace_dev_from_host).  Both forms must give identical bytes; the tool stops
if they do not.  Needs a GPU.

    python tools/flank_timing.py [--loci 1000] [--reps 20] [--out profiles/flank_assemble_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hipstr_amd import capi  # noqa: E402
import flow_chain as fch  # noqa: E402
import flow_chain_flanks as ff  # noqa: E402


def six_loci(hmm, oracle):
    """The chain up to the flank step -> the flank inputs of the six loci as host arrays."""
    names = list(ff.CASES)
    be = ff.DeviceBackend(hmm)
    try:
        states = [fch.State(ff.Inputs(n), oracle) for n in names]
        k, pooled, seeds = fch.genotype_pass(states, be, oracle, None)
        asg, tr = ff._retrace(states, be, k, pooled, seeds, [True] * len(states))
        fl = capi.trace_dev_fetch(hmm, be.tds[tr], capi.TRACE_F_FLANKS, null_others=True)
        a = pooled.arrays
        return dict(n_alleles=np.array([s.A for s in states], np.int32), n_samples=k.n_samples.copy(), read_off=k.read_off.copy(), sample=k.sample.copy(),
                    seeds=np.asarray(seeds, np.int32).copy(), read_req=asg["read_req"].copy(), req_read=asg["req_read"].copy(), pool_index=np.asarray(k.pool_index, np.int32).copy(),
                    pool_off=np.asarray(k.pool_off, np.int32).copy(), flank_off=fl["flank_seq_off"][:2 * int(asg["n_req"]) + 1].copy(),
                    flank_seq=fl["flank_seq"].raw[:int(fl["flank_seq_off"][2 * int(asg["n_req"])])],
                    blk_nopts=a["blk_nopts"].copy(), opt_off=a["opt_off"].copy(), seq=a["seq"][:int(a["opt_off"][-1])], hap_off=a["hap_off"].copy())
    finally:
        be.close()


def tiled(d, times):
    """`times` copies of the six loci, locus after locus."""
    def offs(off):
        step = int(off[-1])
        return np.concatenate([[0]] + [off[1:] + i * step for i in range(times)]).astype(np.int32)
    n_req = len(d["req_read"]); n_pooled = int(d["pool_off"][-1])
    rr = np.concatenate([np.where(d["read_req"] >= 0, d["read_req"] + i * n_req, -1) for i in range(times)]).astype(np.int32)
    t = dict(n_alleles=np.tile(d["n_alleles"], times), n_samples=np.tile(d["n_samples"], times), read_off=offs(d["read_off"]), sample=np.tile(d["sample"], times),
             seeds=np.tile(d["seeds"], times), read_req=rr, req_read=np.concatenate([d["req_read"] + i * n_pooled for i in range(times)]).astype(np.int32),
             pool_index=np.tile(d["pool_index"], times), pool_off=offs(d["pool_off"]), flank_off=offs(d["flank_off"]), flank_seq=d["flank_seq"] * times + b"?",
             blk_nopts=np.tile(d["blk_nopts"], times), opt_off=offs(d["opt_off"]), seq=d["seq"] * times + b"?", hap_off=offs(d["hap_off"]))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=1000); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--out", default=None)
    o = ap.parse_args()
    hmm = capi.load_hmm(); oracle = capi.load_oracle()
    assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error().decode()
    d = six_loci(hmm, oracle)
    t = tiled(d, max(1, round(o.loci / 6)))
    nl = len(t["n_alleles"]); n = int(t["read_off"][-1])
    pb = capi.PostBatch(t["n_alleles"], t["n_samples"], t["read_off"], t["sample"], np.zeros(n), np.zeros(n), np.ones(n, np.int32),
                        np.zeros(int((np.diff(t["read_off"]).astype(np.int64) * t["n_alleles"]).sum())))
    s = capi.HipstrBatch(); s.n_loci = nl
    s.blk_nopts = t["blk_nopts"].ctypes.data_as(capi._i32p); s.opt_off = t["opt_off"].ctypes.data_as(capi._i32p); s.seq = t["seq"]
    s.hap_off = t["hap_off"].ctypes.data_as(capi._i32p); s.read_off = t["pool_off"].ctypes.data_as(capi._i32p)
    trace = dict(flank_seq_off=t["flank_off"], flank_seq=t["flank_seq"])
    a = dict(pb=pb, bptr=C.pointer(s), seed=t["seeds"], read_req=t["read_req"], req_read=t["req_read"], pool_index=t["pool_index"], **ff.FLANK_KW)
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd, hmm.hipstr_last_error().decode()
    td = capi.trace_dev_from_host(hmm, trace, len(t["req_read"]))
    try:
        dev = capi.run_flank(hmm, td=td, pd=pd, **a)
        caps = dev["need"]
        def device():
            return capi.run_flank(hmm, td=td, pd=pd, caps=caps, **a)
        def host():
            tr = capi.trace_dev_fetch(hmm, td, capi.TRACE_F_FLANKS, null_others=True)
            return capi.run_flank(hmm, trace=dict(flank_seq_off=tr["flank_seq_off"], flank_seq=tr["flank_seq"]), caps=caps, **a)
        def fetch_only():
            return capi.trace_dev_fetch(hmm, td, capi.TRACE_F_FLANKS, null_others=True)
        x, y = device(), host()
        assert x["rc"] == y["rc"] == 0
        for key in x["raw"]:
            same = (x["raw"][key] == y["raw"][key]) if isinstance(x["raw"][key], bytes) else np.array_equal(x["raw"][key], y["raw"][key])
            assert same, "the two forms differ in " + key
        last = capi.flank_last(hmm)
        ms = {}
        for name, fn in (("device", device), ("host", host), ("fetch", fetch_only)):
            fn(); ts = []
            for _ in range(o.reps):
                t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
            ms[name] = (float(np.median(ts)), float(np.min(ts)))
    finally:
        td.close(); hmm.hipstr_post_free(pd)
    n_req = len(t["req_read"]); n_tasks = 2 * int(t["n_samples"].sum())
    host_bytes = (2 * n_req + 1) * 4 + len(t["flank_seq"]) - 1
    lines = [
        "flank reassembly: hipstr_flank_assemble_dev against hipstr_trace_dev_fetch(FLANKS) + hipstr_flank_assemble",
        "batch: the six flank cases of tests/flow_chain_flanks.py tiled to %d loci; %d reads, %d requests, %d flank bytes, %d tasks" % (nl, n, n_req, len(t["flank_seq"]) - 1, n_tasks),
        "new options %d, samples realigned %d of %d; tasks the host twin assembled inside the device call: %d" % (
            int(x["opt_off"][2 * nl]), int(x["realign_sample"].sum()), len(x["realign_sample"]), last["host_tasks"]),
        "wall clock per call through the ctypes wrapper (output buffers allocated per call in both forms), median (min) of %d:" % o.reps,
        "  device form           %9.3f ms (%9.3f)   host link: %d bytes up, %d bytes down" % (ms["device"][0], ms["device"][1], last["bytes_up"], last["bytes_down"]),
        "  host form             %9.3f ms (%9.3f)   host link: 0 bytes up, %d bytes down" % (ms["host"][0], ms["host"][1], host_bytes),
        "    of which the fetch  %9.3f ms (%9.3f)" % ms["fetch"],
        "both forms gave identical bytes in every output array",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if o.out:
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
