#!/usr/bin/env python
"""bench.py — read x allele HMM alignments/sec (and STR loci/sec) on 1..8 MI355X.

    python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run, one rank per GPU)

A "step" is one pass of the hot path over one resident batch of synthetic loci: the forward-HMM kernels
(every pooled read x every candidate allele) followed by the diplotype-posterior kernel (workload c3: plus the
de novo stutter EM and the genotype calls of BASELINE configs[2]).  STR loci are independent, so ranks hold
disjoint loci of one seeded set, no collective touches the data path.  Default: weak scaling (per-GPU work
fixed, rank r takes loci [r*n, (r+1)*n)); --scaling strong splits the workload's loci over the ranks.
`value` = alignments of all ranks x K / max-over-ranks wall time of the K timed steps, with inputs already
resident in HBM; `ms_per_step` = that wall time / K.

A plain run sets up, warms up, times the K steps and prints the JSON line (metric, value, unit, ms_per_step, dtype,
config, ...); nothing else.  --dump-outputs DIR also writes what the timed path computed in its last step (see
dump_outputs).  --full adds every other measurement and check to the line, each taken after the timed steps: the
host-inclusive figure (SURVEY §8d's metric taken literally: host arrays in, results out, through the streaming
C-ABI) under "end_to_end", the stages around the forward pass, the per-kernel phase times and the blocks below,
host-side timings, the workload breakdowns of c3 / c4, the pinned-child runs and, with N > 1, every rank's rate and
the cross-device check of the ranks' results.

Also printed in the same JSON line with --full:
  roofline      dominant kernel: ALGORITHMIC bytes per launch (SURVEY.md §8d formula, computed from the batch)
                / average launch duration measured with HIP events on the launch stream, vs the 8 TB/s HBM peak;
                traffic = L2<->fabric bytes from the committed rocprofv3 --pmc passes (profiles/).  The path is an
                issue-bound FP64 max-plus recurrence, so the HBM fraction is ~4e-4 by construction.
  valu          the limiter that binds, from the committed counter passes of THIS build (profiles/*_sq_counters.json,
                checked against the kernel source hash): executed FP64 instructions against the FP64-VALU peak and
                the VALU pipe occupancy with measured per-class issue costs (profiles/*_valu_microbench.json).
  cpu_baseline  the compiled reference (oracle/_ref, kind "reference") or, if absent, the C oracle (kind "port")
                on this host: N = all host cores, one process per core on its own loci — the reference's documented
                scale-out mode (README.md:167-171) — and the single-core figure beside it; bounded sample; rank 0, N=1.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SEED = 20260928      # rng = mt19937(20260928 + locus); the GPU ranks and the CPU baseline take loci of this ONE seeded set

WORKLOADS = {
    # name: (loci, reads/locus, STR alleles, read length, flank length, STR bp, description)
    "ns": (1000, 500, 32, 150, 60, 40, "north-star shape of BASELINE configs[1] (SURVEY §8d NS): 1000 STR loci x 500 pooled 150bp reads x 32 candidate alleles"),
    "c1": (1, 50, 4, 150, 60, 40, "BASELINE configs[0]: 1 locus x 50 reads x 4 alleles"),
    "c2": (1000, 40, 32, 150, 60, 40, "BASELINE configs[1] at literal 30x depth: 1000 loci x 40 reads x 32 alleles"),
    "p30": (4000, 40, 8, 150, 35, 40, "production-like shape (SURVEY §8: flanks <= 35 bp, HaplotypeGenerator.cpp:349-361; ~10 alleles; 30x depth): 4000 loci x 40 reads x 8 alleles"),
    "c3": (10000, 600, 32, 150, 60, 40, "BASELINE configs[2] (SURVEY §8d C3-like): 10k loci x 600 reads (100 samples x 6) x 32 alleles, stutter EM + posteriors + genotype calls in the step"),
    "c4": (100, 5000, 32, 150, 60, 40, "BASELINE configs[3] per-locus shape (one GPU's shard): 100 loci x 1000 samples x 5 reads x 32 alleles; forward HMM + R x A^2 posteriors + genotype calls in the step"),
    "c5": (256, 200, 128, 250, 110, 100, "BASELINE configs[4] stress: 256 loci x 200 250bp reads x 128 alleles, ~100bp STR blocks"),
}


DUMP_BYTES = 60 << 20     # --dump-outputs: the data of all files together (under 64 MB with the .npy headers)


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy in float64 (the int32 outputs are exact in it).  An array longer than its share of
    DUMP_BYTES is replaced by a fixed sample of its elements (indices drawn with SEED, kept in index order), written as <name>_sample.npy:
    two builds run with the same arguments write the same elements and can be compared file by file."""
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BYTES // 8 // len(arrays)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64).ravel()
        if a.size > cap:
            a, name = a[np.sort(np.random.default_rng(SEED).choice(a.size, cap, replace=False))], name + "_sample"
        np.save(os.path.join(path, name + ".npy"), a)


def _cpu_worker(argv):
    """`bench.py --cpu-worker <workload> <first_locus> <n_loci>`: one process of the CPU baseline — the compiled reference (or the C
    oracle) on its own loci; prints alignments and seconds."""
    from hipstr_amd import capi
    try:                                  # (a parent pinned by --host-threads must not pin the CPU baseline)
        os.sched_setaffinity(0, range(os.cpu_count() or 1))
    except Exception:
        pass
    loci, P, A, L, F, sbp, _ = WORKLOADS[argv[0]]
    first, n = int(argv[1]), int(argv[2])
    if capi.have_ref():
        lib, pfx = capi.load_ref(), "ref_"
    else:
        lib, pfx = capi.load_oracle(), "oracle_"
    sb = capi.SynthBatch(n_loci=n, reads_per_locus=P, n_str_alleles=A, read_len=L, flank_len=F, str_bp=sbp, seed=SEED, first_locus=first)
    probs = np.zeros(sb.n_out); seeds = np.zeros(sb.n_reads, np.int32)
    t0 = time.perf_counter()
    rc = getattr(lib, pfx + "process_reads")(sb.ptr, probs.ctypes.data_as(capi._f64p), seeds.ctypes.data_as(capi._i32p))
    dt = time.perf_counter() - t0
    assert rc == 0
    print(json.dumps({"alignments": int((seeds >= 0).sum()) * (sb.n_out // sb.n_reads), "seconds": dt}))


def usable_cores():
    """CPUs this process may actually use: the affinity mask, capped by the container's cgroup v2 quota (cpu.max = "<quota> <period>")."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, -(-int(q) // int(p))))
    except Exception:
        pass
    return n


def device_identity(torch, local):
    """Where this rank's GPU sits: PCI address (hipDeviceGetPCIBusId through torch's device properties), its NUMA node from sysfs, the
    CPUs the rank may run on."""
    out = {"cpus_allowed": sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}
    try:
        pr = torch.cuda.get_device_properties(local)
        out["device_name"] = pr.name
        bus = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0), getattr(pr, "pci_device_id", 0))
        out["pci_bus_id"] = bus
        try:
            out["numa_node"] = int(open("/sys/bus/pci/devices/%s/numa_node" % bus).read().strip())
        except Exception:
            out["numa_node"] = None
    except Exception as ex:
        out["pci_bus_id"] = None; out["error"] = repr(ex)[:120]
    return out


def cpu_baseline(capi, wl_name, budget_s=20.0, n_loci=0):
    """The same hot path on the host CPU, bounded sample: (i) one core, (ii) every core — N independent processes, one per core,
    each on its own contiguous loci: the reference's documented way to use a multi-core box (README.md:167-171; it is single-threaded)."""
    import subprocess
    loci, P, A, L, F, sbp, _ = WORKLOADS[wl_name]
    loci = n_loci or loci
    kind = "reference" if capi.have_ref() else "port"
    def run_procs(n_procs, loci_each, first0):
        t0 = time.perf_counter()
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", wl_name, str(first0 + i * loci_each), str(loci_each)],
                                  stdout=subprocess.PIPE, universal_newlines=True) for i in range(n_procs)]
        outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
        wall = time.perf_counter() - t0
        return sum(o["alignments"] for o in outs), max(o["seconds"] for o in outs), wall
    # The sample is a slice of the SAME seeded set the GPU's step runs (seed 20260928, loci [0, loci) of rank 0 — a locus depends on
    # (seed, index) only, so these are byte for byte loci of the timed batch: SURVEY §8(d) "identical bytes go to the CPU and the GPU").
    # one core: size the sample from a single locus
    a1, s1, _ = run_procs(1, 1, 0)
    per_locus = s1
    n1 = max(1, min(16, loci, int(budget_s * 0.5 / max(per_locus, 1e-3))))
    first1 = min(1, max(0, loci - n1))
    a1, s1, _ = run_procs(1, n1, first1)
    cores = usable_cores()
    each = max(1, min(16, max(1, loci // cores), int(budget_s * 0.6 / max(per_locus, 1e-3))))
    n_procs = cores
    firstN = max(0, min(loci - n_procs * each, first1 + n1))         # behind the one-core sample where the set is large enough
    if n_procs * each > loci:                                        # a set with fewer loci than cores (c1): the processes share them round robin
        firstN = 0
    t0 = time.perf_counter()
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", wl_name, str((firstN + i * each) % max(1, loci - each + 1)), str(each)],
                              stdout=subprocess.PIPE, universal_newlines=True) for i in range(n_procs)]
    outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
    wallN = time.perf_counter() - t0
    aN, sN = sum(o["alignments"] for o in outs), max(o["seconds"] for o in outs)
    return {"value": aN / sN, "unit": "alignments/s", "cores": cores, "kind": kind,
            "sample": "%d processes x %d loci, loci [%d, %d) of the timed batch's own seeded set (seed %d; %d reads x %d alleles x %dbp per locus) = %d alignments; slowest process %.1f s (wall incl. start-up %.1f s); HapAligner::process_reads only"
                      % (cores, each, firstN, firstN + n_procs * each, SEED, P, A, L, aN, sN, wallN),
            "single_core": {"value": a1 / s1, "cores": 1, "sample": "loci [%d, %d) of the same set: %d alignments, %.1f s" % (first1, first1 + n1, a1, s1)},
            "same_bytes_as_gpu_batch": True, "seed": SEED,
            "host_cores_visible": os.cpu_count(), "host_cores_usable": cores}


def _profile_key(path):
    """profiles/r01_v10_x.json sorts after r01_v9_x.json: compare the numbers in the name, not the characters."""
    import re
    return [int(x) for x in re.findall(r"\d+", os.path.basename(path))]


def pipeline_stages(capi, hmm, sb, loci, P):
    """Short, separately timed runs of the other device stages of the path on the same kind of data (not part of `value`):
    Needleman-Wunsch in front of the HMM, the Viterbi traceback behind it, and the de novo stutter EM of BASELINE configs[2]."""
    import ctypes as C
    from hipstr_amd import gen
    out = {}
    # Needleman-Wunsch: one 150 bp read against a ~300 bp reference window per pair (realign(), AlignmentOps.cpp:14-26)
    pairs = gen.nw_pairs(7, n=4000, ref_len=(290, 310), read_len=(140, 150))
    capi.run_nw(hmm, "hipstr_", pairs[:64], False, unpack=False)
    t = {}
    capi.run_nw(hmm, "hipstr_", pairs, False, unpack=False, timing=t)
    out["needleman_wunsch"] = {"pairs_per_s": len(pairs) / t["call_s"], "cells_per_s": sum(len(r) * len(q) for r, q in pairs) / t["call_s"],
                               "pairs": len(pairs), "shape": "150 bp read x 300 bp window"}
    # traceback: every seeded read of the first loci against its source allele, alignment strings from the device NW
    nl = min(loci, 32)
    seeds = np.zeros(sb.n_reads, np.int32)
    hmm.hipstr_calc_seed_bases(sb.ptr, seeds.ctypes.data_as(capi._i32p))
    src = sb.src_allele()
    rr = [r for r in range(nl * P) if seeds[r] >= 0][:20000]; aa = [int(src[r]) for r in rr]          # (bounded: the output pools below hold 16 Mi characters)
    t0 = time.perf_counter()
    h2r = capi.hap_aln_info(hmm, "hipstr_", sb.ptr, cap=1 << 26)
    t_info = time.perf_counter() - t0
    capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr[:256], aa[:256], h2r, cap=1 << 24, unpack=False)
    calls = []
    for _ in range(3):                                         # (the first full-size call wakes the host pool and sizes the block caches)
        t = {}
        capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, cap=1 << 24, timing=t, unpack=False)
        calls.append(t["call_s"])
    out["traceback"] = {"tracebacks_per_s": len(rr) / sorted(calls)[1], "tracebacks_per_s_first_call": len(rr) / calls[0], "calls": 3, "of": "median",
                        "requests": len(rr), "loci": nl, "hap_aln_info_s_all_loci": t_info, "haplotypes": len(h2r)}
    # the whole per-locus chain of SeqStutterGenotyper::genotype + write_vcf_record on one batch of loci: forward pass -> posteriors
    # -> MAP diplotypes -> best haplotype per read (seq_stutter_genotyper.cpp:823-825) -> tracebacks -> genotype calls (GL/PL/Q)
    nc = max(1, min(loci, 64, 40000 // P))                     # (at most ~40000 tracebacks: the output pools below hold 16 Mi characters)
    cb = capi.SynthBatch(n_loci=nc, reads_per_locus=P, n_str_alleles=int(np.diff(np.ctypeslib.as_array(sb.ptr.contents.hap_off, shape=(loci + 1,)))[0]), seed=4242)
    A_c = np.diff(np.ctypeslib.as_array(cb.ptr.contents.hap_off, shape=(nc + 1,)))
    S_c = 5                                                    # samples per locus: reads dealt round-robin-by-block to 5 samples
    lab = np.tile(np.repeat(np.arange(S_c), P // S_c), nc)
    h2r_c = capi.hap_aln_info(hmm, "hipstr_", cb.ptr, cap=1 << 26)
    stage = {}
    def chain():
        t_a = time.perf_counter()
        dev = hmm.hipstr_hmm_upload(cb.ptr)
        hmm.hipstr_hmm_align(dev, None)
        pbc = capi.PostBatch(A_c, np.full(nc, S_c, np.int32), np.arange(nc + 1, dtype=np.int32) * P, lab, np.zeros(nc * P), np.zeros(nc * P),
                             np.ones(nc * P, np.int32), None)
        pdc = hmm.hipstr_post_upload(pbc.ptr, hmm.hipstr_hmm_dev_aln_probs(dev))
        hmm.hipstr_post_launch(pdc, None)
        stage["submit_s"] = time.perf_counter() - t_a          # prepare + upload + launches (asynchronous)
        t_a = time.perf_counter()
        ll = np.zeros(cb.n_out); sd = np.zeros(cb.n_reads, np.int32)
        hmm.hipstr_hmm_fetch(dev, ll.ctypes.data_as(capi._f64p), sd.ctypes.data_as(capi._i32p))
        post = np.zeros(int(pbc.post_off[-1])); tot = np.zeros(nc * S_c); gt = np.zeros(2 * nc * S_c, np.int32); lt = np.zeros(nc)
        hmm.hipstr_post_fetch(pdc, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p), lt.ctypes.data_as(capi._f64p))
        stage["forward_and_fetch_s"] = time.perf_counter() - t_a   # waits for the forward pass and the posteriors, copies them back
        # best haplotype of every read: the likelier of its sample's two MAP haplotypes
        gt = gt.reshape(-1, 2)
        rr_c, aa_c = [], []
        t_sel = time.perf_counter()
        for l in range(nc):
            a = int(A_c[l]); r0 = l * P
            LLl = ll[cb.out_off[l]:cb.out_off[l + 1]].reshape(P, a)
            g = gt[l * S_c + lab[r0:r0 + P]]
            best = np.where(LLl[np.arange(P), g[:, 0]] > LLl[np.arange(P), g[:, 1]], g[:, 0], g[:, 1])
            ok = sd[r0:r0 + P] >= 0
            rr_c.append(np.nonzero(ok)[0] + r0); aa_c.append(best[ok])
        rr_c = np.concatenate(rr_c).astype(np.int32); aa_c = np.concatenate(aa_c).astype(np.int32)
        stage["select_s"] = time.perf_counter() - t_sel
        tt = {}
        capi.run_trace(hmm, "hipstr_hmm_", cb.ptr, rr_c, aa_c, h2r_c, cap=1 << 24, unpack=False, timing=tt)
        stage["trace_s"] = tt["call_s"]
        # genotype calls: every haplotype its own variant here (one flank option), GL + PL
        t_gt = time.perf_counter()
        h2a = np.concatenate([np.arange(a, dtype=np.int32) for a in A_c]); nvv = A_c.astype(np.int32)
        rq = capi.HipstrGtRequest(nvv.ctypes.data_as(capi._i32p), h2a.ctypes.data_as(capi._i32p), 1, 1, 0)
        ns = nc * S_c; ngl = int(sum(int(a) * (int(a) + 1) // 2 for a in A_c)) * S_c
        k = [np.zeros(2 * ns, np.int32), np.zeros(2 * ns, np.int32)] + [np.zeros(ns) for _ in range(5)] + [np.zeros(ngl), np.zeros(ngl, np.int32), np.zeros(1)]
        o = capi.HipstrGtOut(*[a.ctypes.data_as(t) for a, (f, t) in zip(k, capi.HipstrGtOut._fields_)])
        hmm.hipstr_post_extract.restype = C.c_int; hmm.hipstr_post_extract.argtypes = [C.c_void_p, C.POINTER(capi.HipstrGtRequest), C.POINTER(capi.HipstrGtOut)]
        if hmm.hipstr_post_extract(pdc, C.byref(rq), C.byref(o)) != 0:
            raise SystemExit("hipstr_post_extract: " + hmm.hipstr_last_error().decode())
        stage["genotypes_s"] = time.perf_counter() - t_gt
        hmm.hipstr_post_free(pdc); hmm.hipstr_hmm_free(dev)
        return len(rr_c)
    chain()
    t0 = time.perf_counter()
    n_tr = chain()
    dt = time.perf_counter() - t0
    out["chain"] = {"loci_per_s": nc / dt, "loci": nc, "reads_per_locus": P, "samples_per_locus": S_c, "tracebacks": n_tr, "seconds": dt,
                    "stage_seconds": stage,
                    "stages": "upload + forward + posteriors + fetch + best-haplotype pick (numpy) + tracebacks + genotype calls, one batch, python-orchestrated"}
    # de novo stutter EM (configs[2] shape: ~100 samples at low depth per locus)
    n_em = 512
    kw = gen.em_case(5, n_loci=n_em, samples=(90, 100), reads_per_sample=(4, 8))
    capi.run_em(hmm, "hipstr_", **gen.em_case(6, n_loci=2))
    t0 = time.perf_counter()
    tr, st, it, ll = capi.run_em(hmm, "hipstr_", **kw)
    dt = time.perf_counter() - t0
    out["stutter_em"] = {"loci_per_s": n_em / dt, "locus_iterations_per_s": float(it.sum()) / dt, "loci": n_em, "trained": int(tr.sum()),
                         "shape": "90-100 samples x 4-8 reads"}
    return out


def c3_em_inputs(sb, loci, P, S):
    """The stutter EM's input for the configs[2] step (EMStutterGenotyper::train, em_stutter_genotyper.cpp:170-226): per read the observed
    STR size — its source allele's size difference from the reference allele, with PCR stutter of one repeat unit on 12 % of the reads —,
    reads dealt to S samples in blocks of P / S, no SNP phasing information.  Seeded: the same arrays for the same batch."""
    lab = np.tile(np.repeat(np.arange(S), P // S), loci).astype(np.int32)
    b = sb.ptr.contents
    nopt = np.ctypeslib.as_array(b.blk_nopts, shape=(3 * loci,)).reshape(loci, 3)
    opt_len = np.diff(np.ctypeslib.as_array(b.opt_off, shape=(int(nopt.sum()) + 1,)))
    period = np.ctypeslib.as_array(b.period, shape=(loci,))
    src = sb.src_allele().reshape(loci, P)
    opt_base = np.concatenate([[0], np.cumsum(nopt.sum(axis=1))])[:-1] + nopt[:, 0]          # first STR option of every locus
    rng = np.random.default_rng(5)
    size = np.stack([opt_len[opt_base[l] + src[l]] - opt_len[opt_base[l]] for l in range(loci)])       # bp difference from the reference allele
    u = rng.random(size.shape)
    size = size + np.where(u < 0.05, 1, np.where(u < 0.12, -1, 0)) * period[:, None]                    # PCR stutter on the observed sizes
    return dict(period=period, n_samples=np.full(loci, S, np.int32), read_off=np.arange(loci + 1, dtype=np.int32) * P, sample_label=lab,
                num_bps=size.ravel().astype(np.int32), log_p1=np.zeros(loci * P), log_p2=np.zeros(loci * P), haploid=np.zeros(loci, np.uint8))


def thread_cpu_seconds():
    """CPU seconds (user + system) of every thread of this process by thread id, with its name: /proc/self/task/<tid>/stat."""
    out = {}
    tck = os.sysconf("SC_CLK_TCK")
    try:
        for tid in os.listdir("/proc/self/task"):
            try:
                st = open("/proc/self/task/%s/stat" % tid).read()
                name = st[st.index("(") + 1:st.rindex(")")]
                f = st[st.rindex(")") + 2:].split()
                out[int(tid)] = (name, (int(f[11]) + int(f[12])) / tck)
            except Exception:
                pass
    except Exception:
        pass
    return out


def _name_thread(name):
    """The calling thread's name (comm) — cpu_seconds_by_thread tells the harness' own threads from the HIP runtime's, which inherit "python"."""
    try:
        C.CDLL(None).prctl(15, name, 0, 0, 0)
    except Exception:
        pass


def end_to_end(capi, hmm, sb, loci, steps, device, latency=True):
    """SURVEY §8(d)'s metric taken literally — wall time from host arrays in to aln_probs/seeds out (host flatten, H2D, kernels, D2H,
    the reference's output contract) — through the streaming C-ABI, fed the way the reference's caller produces work: ONE locus per
    submission (bam_processor.cpp:550-617).  `steps` passes over the batch go through one open stream back to back, a feeder
    thread submitting while this thread collects in order; reported beside `value`, never as `value` (inputs are host-resident)."""
    import threading
    _name_thread(b"bench-collect")
    st = capi.Stream(hmm, device=device, slots=int(os.environ.get("HIPSTR_BENCH_SLOTS", "8")), batch_alignments=int(os.environ.get("HIPSTR_BENCH_BATCH", "0")))        # 0: the library's own batch size (2 Mi pairs, up to 8 Mi for batches of few heavy loci)
    probs = np.zeros(max(sb.n_out, 1)); seeds = np.zeros(max(sb.n_reads, 1), np.int32)
    def one_pass_set(n):
        # feeder: every locus its own submission (hipstr_stream_submit_each: the per-region loop in C, as the reference's caller is C++);
        # collector: the results of a pass, in order, into one buffer (hipstr_stream_collect)
        # (round 6: the collector used to poll — a try / except / 0.2 ms sleep loop around 256-locus collects while the feeder was behind —
        # and that loop of the HARNESS took a third of the process' CPU under the 2-CPU pin, CPU the library's workers then did not have.
        # Now the feeder posts a semaphore per submitted pass and the collector makes one blocking C call per pass: ctypes releases the
        # GIL inside it, the wait sleeps inside the library.)
        submitted = threading.Semaphore(0)
        def feed():
            _name_thread(b"bench-feeder")
            for _ in range(n):
                st.submit_each(sb.ptr)
                submitted.release()
            st.flush()
        th = threading.Thread(target=feed); th.start()
        for _ in range(n):
            submitted.acquire()
            st.collect(loci, probs, seeds)
        th.join()
    # warm-up: kernels, and the block caches — a miss is a hipMalloc / hipHostMalloc of up to gigabytes (0.9 s seen) in the middle of the
    # stream; passes are repeated until one goes by without a new block from the driver (at most 12): the steady state of a long run
    warm = 0
    for _ in range(12):
        a0 = hmm.hipstr_debug_driver_allocs()
        one_pass_set(1); warm += 1
        if warm >= int(os.environ.get("HIPSTR_BENCH_E2E_WARMUP", "4")) and hmm.hipstr_debug_driver_allocs() == a0:
            break
    # the timed passes; taken again (at most twice) when a block-cache miss — a hipMalloc / hipHostMalloc next to running kernels, 0.1-0.9 s —
    # fell into them: how many batches are in flight varies with the box's load, so a new size class can still turn up after the warm-up
    for attempt in range(3):
        s0 = st.stats()
        a_timed0 = hmm.hipstr_debug_driver_allocs()
        tc0 = thread_cpu_seconds()
        c0 = time.process_time()
        t0 = time.perf_counter()
        one_pass_set(steps)
        dt = time.perf_counter() - t0
        cpu_s = time.process_time() - c0              # CPU seconds of ALL threads of the process over the timed passes
        tc1 = thread_cpu_seconds()
        s1 = st.stats()
        if hmm.hipstr_debug_driver_allocs() == a_timed0:
            break
    st.close()
    # one-locus latency: a 30x locus (40 reads x 32 alleles) and an NS locus through the one-shot call, median of 30
    lat = {}
    for name, (pp, aa) in ((("40x32", (40, 32)), ("500x32", (500, 32)), ("50x4", (50, 4))) if latency else ()):
        one = capi.SynthBatch(n_loci=1, reads_per_locus=pp, n_str_alleles=aa, seed=77)
        pr = np.zeros(one.n_out); sd = np.zeros(one.n_reads, np.int32)
        ts = []
        for _ in range(33):
            t1 = time.perf_counter()
            assert hmm.hipstr_hmm_process_reads(one.ptr, pr.ctypes.data_as(capi._f64p), sd.ctypes.data_as(capi._i32p)) == 0
            ts.append(time.perf_counter() - t1)
        lat[name] = {"median_ms": 1e3 * float(np.median(ts[3:])), "min_ms": 1e3 * float(np.min(ts[3:]))}
    return {"seconds": dt, "passes": steps, "ms_per_pass": 1e3 * dt / steps, "submissions": steps * loci, "loci_per_submission": 1,
            "batches": s1["batches"] - s0["batches"], "worker_host_seconds": s1["host_seconds"] - s0["host_seconds"],
            "collector_wait_seconds": s1["wait_seconds"] - s0["wait_seconds"],
            "process_cpu_seconds": cpu_s, "process_cpu_ms_per_pass": 1e3 * cpu_s / steps, "process_cpu_us_per_locus": 1e6 * cpu_s / (steps * loci),
            "cpu_seconds_by_role": {k[4:-8]: s1[k] - s0[k] for k in ("cpu_submit_seconds", "cpu_prepare_seconds", "cpu_upload_seconds", "cpu_collect_seconds")},
            # the threads that used the most CPU over the timed passes (10 ms clock ticks; name = the thread's comm; threads that ended meanwhile — the feeder — are missing)
            "cpu_seconds_by_thread": sorted(([tc1[t][0], round(tc1[t][1] - tc0.get(t, (None, 0.0))[1], 3)] for t in tc1), key=lambda x: -x[1])[:8],
            "warmup_passes": warm, "timed_attempts": attempt + 1, "driver_allocs_during_timed_passes": int(hmm.hipstr_debug_driver_allocs() - a_timed0),
            "one_locus_process_reads_latency": lat,
            "path": "hipstr_stream_submit_each (1 locus per submission) -> batches of 2-8 Mi alignments (the library's choice by loci per batch and host threads) -> prepare on host threads + H2D + table expansion + kernels + D2H, 8 slots -> hipstr_stream_collect in order"}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":
        return _cpu_worker(sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="ns", choices=sorted(WORKLOADS))
    ap.add_argument("--loci", type=int, default=0, help="override the number of loci (per GPU with weak scaling, in total with strong scaling)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"], help="weak: every rank takes the workload's loci; strong: they are split over the ranks")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="skip the short measurements of the stages around the forward pass")
    ap.add_argument("--host-threads", type=int, default=0,
                    help="give the process N host CPUs: the library's host threads (HIPSTR_HOST_THREADS) AND the affinity mask of every thread of the "
                         "process (feeder, stream workers, collector included) — what one rank has on a node whose cores are shared by 8 ranks")
    ap.add_argument("--e2e-only", action="store_true", help="only the end-to-end (stream) measurement; prints its block as one JSON line")
    ap.add_argument("--full", action="store_true",
                    help="every measurement and check beyond the headline (end-to-end, pipeline stages, CPU baseline, per-kernel and roofline "
                         "figures, host timings, workload breakdowns, pinned children, per-rank rates and the cross-device check)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed path computed in its last step to DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.host_threads > 0:
        # before any thread of the process exists (torch, the library's pool, the stream's workers): they inherit the mask
        cpus = sorted(os.sched_getaffinity(0))[:args.host_threads]
        os.sched_setaffinity(0, cpus)
        os.environ["HIPSTR_HOST_THREADS"] = str(args.host_threads)

    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1")); local = int(os.environ.get("LOCAL_RANK", "0"))
    rank_cpus = None
    # a rank's share of the node's usable CPUs, taken BEFORE the rank narrows its own mask (computed afterwards it would be the share of a
    # share on the ranks whose pinning succeeded and the full share on one whose pinning failed: ranks disagreeing on their thread count)
    cores_before_pin = usable_cores()
    if world > 1 and not args.host_threads and not os.environ.get("HIPSTR_BENCH_NO_PIN"):
        # one process per GPU: every rank keeps to its own slice of the node's usable CPUs — all of its threads (they inherit the mask: this
        # runs before torch, the library's pool and the stream's workers exist) — so that the ranks' host work does not migrate over each other
        lw = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        allowed = sorted(os.sched_getaffinity(0))
        per = max(1, min(usable_cores(), len(allowed)) // max(1, lw))
        mine = allowed[(local % lw) * per:(local % lw) * per + per] or allowed[:per]
        try:
            os.sched_setaffinity(0, mine); rank_cpus = mine
        except OSError:
            rank_cpus = None
    import torch
    import torch.distributed as dist
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run --nproc-per-node %d)" % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # HIPSTR_BENCH_SHARE_GPU=1 (testing only): all ranks use GPU 0 and rendezvous over gloo, to exercise the N>1 code path on a 1-GPU box
    share = os.environ.get("HIPSTR_BENCH_SHARE_GPU") == "1"
    if share:
        local = 0
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    # host threads of the library per rank: the usable cores of the node are shared by the ranks on it (each rank prepares its own batches)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    host_threads = max(1, cores_before_pin // max(1, local_world))
    if world > 1:
        os.environ.setdefault("HIPSTR_HOST_THREADS", str(host_threads))
    from hipstr_amd import capi
    hmm = capi.load_hmm()
    if hmm.hipstr_hmm_init(local) != 0:
        raise SystemExit("hipstr_hmm_init: " + hmm.hipstr_last_error().decode())

    wl = WORKLOADS[args.workload]
    loci, P, A, L, F, sbp, desc = wl
    if args.loci:
        loci = args.loci
    # --- this rank's loci of the ONE seeded set (a locus depends on (seed, index) only): weak scaling gives every rank `loci` of them,
    # strong scaling splits `loci` over the ranks; either way contiguous index ranges, rank order = locus order
    if args.scaling == "strong":
        first = loci * rank // world; loci = loci * (rank + 1) // world - first
    else:
        first = loci * rank
    t0 = time.perf_counter()
    sb = capi.SynthBatch(n_loci=loci, reads_per_locus=P, n_str_alleles=A, read_len=L, flank_len=F, str_bp=sbp, seed=SEED, first_locus=first)
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev = hmm.hipstr_hmm_upload(sb.ptr)
    if not dev:
        raise SystemExit("upload failed: " + hmm.hipstr_last_error().decode())
    torch.cuda.synchronize()
    t_upload_cold = time.perf_counter() - t0          # first call of the process: device and pinned blocks come from the driver
    if args.full:
        hmm.hipstr_hmm_free(dev)
        t0 = time.perf_counter()
        dev = hmm.hipstr_hmm_upload(sb.ptr)
        torch.cuda.synchronize()
        t_upload = time.perf_counter() - t0           # steady state: blocks from the library's caches
    n_aln = C.c_int64(0); algo = C.c_int64(0); cells = C.c_int64(0)
    hmm.hipstr_hmm_workload(dev, C.byref(n_aln), C.byref(algo), C.byref(cells))
    hap_off = np.ctypeslib.as_array(sb.ptr.contents.hap_off, shape=(loci + 1,))
    A_l = np.diff(hap_off)
    kinds = (C.c_int64 * 4)()
    hmm.hipstr_debug_allele_kinds(dev, kinds)
    n_kinds = max(1, kinds[0] + kinds[1] + kinds[2] + kinds[3])
    str_kinds = {"periodic_tabulated": kinds[1] / n_kinds, "one_or_two_interruptions_piecewise": kinds[2] / n_kinds, "more_interruptions_k_level_form_or_replay_in_group": kinds[3] / n_kinds,
                 "per_read_generic_kernel": kinds[0] / n_kinds,
                 "synth_overrides": {k: v for k, v in os.environ.items() if k.startswith("HIPSTR_SYNTH")}}
    if args.e2e_only:
        # a short resident measurement first (one warm pass, three timed): the child's end-to-end rate is quoted against the resident rate of
        # the same process on the same box
        hmm.hipstr_hmm_align(dev, None); torch.cuda.synchronize()
        t_r = time.perf_counter()
        for _ in range(3):
            hmm.hipstr_hmm_align(dev, None)
        torch.cuda.synchronize()
        resident = 3.0 * n_aln.value / (time.perf_counter() - t_r)
        hmm.hipstr_hmm_free(dev)
        e2e_passes = int(os.environ.get("HIPSTR_BENCH_E2E_PASSES", "0")) or max(2, min(args.steps, 5), min(128, int(1.2e8 // max(1.0, float(n_aln.value)))))      # (the override: experiments on run length)
        e = end_to_end(capi, hmm, sb, loci, e2e_passes, local, latency=False)
        e["alignments_per_s"] = n_aln.value * e["passes"] / e["seconds"]
        e["host_threads"] = args.host_threads or int(os.environ.get("HIPSTR_HOST_THREADS", "0")) or None
        e["cpus_allowed"] = len(os.sched_getaffinity(0))
        e["resident_alignments_per_s"] = resident
        e["fraction_of_resident_rate_same_process"] = e["alignments_per_s"] / resident
        print(json.dumps(e), flush=True)
        return
    if args.workload == "c4":
        # configs[3]: 1000 samples per locus, the locus' reads dealt to them in blocks of P / S; a step = forward HMM + posteriors of every
        # (sample, diplotype) + genotype calls (GL, PL) — seq_stutter_genotyper.cpp:603-671 without the allele rounds
        S = 1000
        lab = np.tile(np.repeat(np.arange(S), P // S), loci).astype(np.int32)
        pb = capi.PostBatch(A_l, np.full(loci, S, np.int32), np.arange(loci + 1, dtype=np.int32) * P, lab, np.zeros(loci * P), np.zeros(loci * P),
                            np.ones(loci * P, np.int32), None)
        h2a = np.concatenate([np.arange(a, dtype=np.int32) for a in A_l]); nvv = A_l.astype(np.int32)
        rq = capi.HipstrGtRequest(nvv.ctypes.data_as(capi._i32p), h2a.ctypes.data_as(capi._i32p), 1, 1, 0)
        ns = loci * S; ngl = int(sum(int(a) * (int(a) + 1) // 2 for a in A_l)) * S
        gt_k = [np.zeros(2 * ns, np.int32), np.zeros(2 * ns, np.int32)] + [np.zeros(ns) for _ in range(5)] + [np.zeros(ngl), np.zeros(ngl, np.int32), np.zeros(1)]
        gt_o = capi.HipstrGtOut(*[a.ctypes.data_as(t) for a, (f, t) in zip(gt_k, capi.HipstrGtOut._fields_)])
        hmm.hipstr_post_extract.restype = C.c_int; hmm.hipstr_post_extract.argtypes = [C.c_void_p, C.POINTER(capi.HipstrGtRequest), C.POINTER(capi.HipstrGtOut)]
    elif args.workload == "c3":
        # configs[2]: 100 samples per locus, the locus' reads dealt to them in blocks; a step = stutter EM on the observed STR sizes
        # (EMStutterGenotyper::train, all loci in lock step) + forward HMM + posteriors + genotype calls (GL, PL)
        S = 100
        lab = np.tile(np.repeat(np.arange(S), P // S), loci).astype(np.int32)
        pb = capi.PostBatch(A_l, np.full(loci, S, np.int32), np.arange(loci + 1, dtype=np.int32) * P, lab, np.zeros(loci * P), np.zeros(loci * P),
                            np.ones(loci * P, np.int32), None)
        em_kw = c3_em_inputs(sb, loci, P, S)
        h2a = np.concatenate([np.arange(a, dtype=np.int32) for a in A_l]); nvv = A_l.astype(np.int32)
        rq = capi.HipstrGtRequest(nvv.ctypes.data_as(capi._i32p), h2a.ctypes.data_as(capi._i32p), 1, 1, 0)
        ns = loci * S; ngl = int(sum(int(a) * (int(a) + 1) // 2 for a in A_l)) * S
        gt_k = [np.zeros(2 * ns, np.int32), np.zeros(2 * ns, np.int32)] + [np.zeros(ns) for _ in range(5)] + [np.zeros(ngl), np.zeros(ngl, np.int32), np.zeros(1)]
        gt_o = capi.HipstrGtOut(*[a.ctypes.data_as(t) for a, (f, t) in zip(gt_k, capi.HipstrGtOut._fields_)])
        hmm.hipstr_post_extract.restype = C.c_int; hmm.hipstr_post_extract.argtypes = [C.c_void_p, C.POINTER(capi.HipstrGtRequest), C.POINTER(capi.HipstrGtOut)]
    else:
        # posteriors: one sample per locus (configs[1]: "1 sample"), every pooled read its own read, no SNP phasing information
        pb = capi.PostBatch(A_l, np.ones(loci, np.int32), np.arange(loci + 1, dtype=np.int32) * P, np.zeros(loci * P, np.int32),
                            np.zeros(loci * P), np.zeros(loci * P), np.ones(loci * P, np.int32), None)
    pd = hmm.hipstr_post_upload(pb.ptr, hmm.hipstr_hmm_dev_aln_probs(dev))
    if not pd:
        raise SystemExit("posterior upload failed: " + hmm.hipstr_last_error().decode())
    em_stats = {}
    em_last = {}

    def step():
        if args.workload == "c3":
            t_em = time.perf_counter()
            tr, st_, it_, ll_ = capi.run_em(hmm, "hipstr_", **em_kw)
            em_stats["em_s"] = em_stats.get("em_s", 0.0) + time.perf_counter() - t_em
            em_stats["trained"] = int(tr.sum()); em_stats["iterations"] = int(it_.sum())
            em_last.update(em_trained=tr, em_stutter_params=st_, em_iterations=it_, em_log_likelihood=ll_)
        if hmm.hipstr_hmm_align(dev, None) != 0 or hmm.hipstr_post_launch(pd, None) != 0:
            raise SystemExit("launch failed: " + hmm.hipstr_last_error().decode())
        if args.workload == "c4":
            if hmm.hipstr_post_extract(pd, C.byref(rq), C.byref(gt_o)) != 0:
                raise SystemExit("hipstr_post_extract: " + hmm.hipstr_last_error().decode())
        if args.workload == "c3":
            torch.cuda.synchronize()               # the forward and posterior kernels are in flight: do not charge them to the calls
            t_gt = time.perf_counter()
            if hmm.hipstr_post_extract(pd, C.byref(rq), C.byref(gt_o)) != 0:
                raise SystemExit("hipstr_post_extract: " + hmm.hipstr_last_error().decode())
            em_stats["calls_s"] = em_stats.get("calls_s", 0.0) + time.perf_counter() - t_gt

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    em_stats.clear()
    if args.full:
        hmm.hipstr_hmm_profile(dev, 1)            # device events around every kernel group of the timed passes: the per-kernel figures
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if args.full:
        hmm.hipstr_hmm_profile(dev, 0)
        ms = (C.c_float * (4 * args.steps))()
        n_ms = hmm.hipstr_hmm_profile_read(dev, ms, args.steps)
        phase_ms = np.array(ms[:4 * n_ms], dtype=np.float64).reshape(-1, 4).mean(axis=0) if n_ms > 0 else np.full(4, np.nan)
        phase_names = ["hs_lead_kernel", "hs_str_kernel", "hs_trail_kernel", "hs_combine_kernel"]
        dom = int(np.nanargmax(phase_ms)) if n_ms > 0 else 1
        kernel_ms = float(phase_ms[dom])          # average duration of the dominant kernel (group) per pass

    if args.full or args.dump_outputs:
        # --- a D2H of the results after the timed region (sanity + the PCIe-inclusive figure for DESIGN.md)
        t0 = time.perf_counter()
        probs = np.zeros(sb.n_out); seeds = np.zeros(sb.n_reads, np.int32)
        assert hmm.hipstr_hmm_fetch(dev, probs.ctypes.data_as(capi._f64p), seeds.ctypes.data_as(capi._i32p)) == 0
        t_fetch = time.perf_counter() - t0
        if not os.environ.get("HIPSTR_BENCH_NOCHECK"):       # kernel ablation builds (timing only, results invalid) set this
            assert np.all(np.isfinite(probs)) and np.all(probs <= 1e-10), "forward scores must be finite log-likelihoods <= 0"

    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step (rank 0's loci): the forward scores and seeds, then the
        # genotype calls where the step makes them (c3, c4: the posteriors stay on the device), else the posteriors
        outs = {"aln_log_probs": probs, "seeds": seeds}
        if args.workload in ("c3", "c4"):
            outs.update(zip((f for f, _ in capi.HipstrGtOut._fields_), gt_k))
            outs.update(em_last)
        else:
            post = np.zeros(int(pb.post_off[-1])); tot = np.zeros(loci); gt = np.zeros(2 * loci, np.int32); lt = np.zeros(loci)
            if hmm.hipstr_post_fetch(pd, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p), lt.ctypes.data_as(capi._f64p)) != 0:
                raise SystemExit("hipstr_post_fetch: " + hmm.hipstr_last_error().decode())
            outs.update(log_post=post, sample_total_ll=tot, map_gt=gt, locus_total_ll=lt)
        dump_outputs(args.dump_outputs, outs)

    per_rank = None; e2e_multi = None; rank_info = None; cross_check = None
    if world > 1 and args.full:
        dev_t = "cpu" if share else "cuda"
        # every rank's own resident rate, and the end-to-end rate (host arrays in -> results out through the stream) of all ranks at once
        mine = torch.tensor([float(n_aln.value) * args.steps / elapsed], dtype=torch.float64, device=dev_t)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [float(x.item()) for x in allr]
        info = [None] * world
        dist.all_gather_object(info, {"rank": rank, "first_locus": int(first), "loci": int(loci), "alignments_per_step": int(n_aln.value),
                                      "host_threads": int(os.environ.get("HIPSTR_HOST_THREADS", host_threads)), "cpus": rank_cpus, "device": int(local)})
        rank_info = info
        if not args.no_pipeline:
            dist.barrier()
            e = end_to_end(capi, hmm, sb, loci, max(2, min(args.steps, 3)), local, latency=False)
            te = torch.tensor([e["seconds"]], dtype=torch.float64, device=dev_t); dist.all_reduce(te, op=dist.ReduceOp.MAX)
            ae = torch.tensor([float(n_aln.value) * e["passes"]], dtype=torch.float64, device=dev_t); dist.all_reduce(ae, op=dist.ReduceOp.SUM)
            e2e_multi = {"alignments_per_s": float(ae.item()) / float(te.item()), "seconds_max_over_ranks": float(te.item()), "passes": e["passes"],
                         "host_threads_per_rank": int(os.environ.get("HIPSTR_HOST_THREADS", host_threads))}
        # Self-check on first contact with a multi-GPU node: every rank's device must return, for a strided sample of
        # ITS loci, the bits rank 0's device returns for the same loci (regenerated there from (seed, index)); a mismatch ends every rank
        # loudly instead of printing a rate.  The devices' PCI addresses and NUMA nodes go into the line: a bad affinity shows in the first record.
        import hashlib
        def _dig(p_, s_):
            return hashlib.sha256(np.ascontiguousarray(p_).tobytes() + np.ascontiguousarray(s_).tobytes()).hexdigest()
        sample = sorted(set(int(x) for x in np.linspace(0, loci - 1, num=min(4, loci)))) if loci > 0 else []
        mine_chk = {"rank": rank, "first_locus": int(first), "sample": sample,
                    "digests": [_dig(probs[int(sb.out_off[l]):int(sb.out_off[l + 1])], seeds[l * P:(l + 1) * P]) for l in sample]}
        mine_chk.update(device_identity(torch, local))
        chk = [None] * world
        dist.all_gather_object(chk, mine_chk)
        verdict = [None]
        if rank == 0:
            bad = []
            for c in chk:
                if c["rank"] == 0:
                    continue
                for l, d in zip(c["sample"], c["digests"]):
                    one = capi.SynthBatch(n_loci=1, reads_per_locus=P, n_str_alleles=A, read_len=L, flank_len=F, str_bp=sbp, seed=SEED, first_locus=c["first_locus"] + l)
                    p0, s0 = capi.run_align(hmm, "hipstr_hmm_", one.ptr, fill=0.0)
                    if _dig(p0, s0) != d:
                        bad.append("rank %d (device %s) locus %d" % (c["rank"], c.get("pci_bus_id"), c["first_locus"] + l))
            verdict[0] = bad
        dist.broadcast_object_list(verdict, src=0)
        if verdict[0]:
            raise SystemExit("bench.py: results of " + "; ".join(verdict[0]) + " differ from rank 0's device on the same loci — no rate is reported")
        cross_check = {"loci_per_rank": len(sample), "ranks_checked_against_rank0": world - 1, "mismatches": 0,
                       "devices": [{k: c.get(k) for k in ("rank", "pci_bus_id", "numa_node", "device_name", "cpus_allowed")} for c in chk]}
    if world > 1:
        dev_t = "cpu" if share else "cuda"
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev_t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        cnt = torch.tensor([float(n_aln.value), float(loci)], dtype=torch.float64, device=dev_t)
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
        total_aln, total_loci = float(cnt[0].item()), float(cnt[1].item())
    else:
        total_aln, total_loci = float(n_aln.value), float(loci)

    def profile_for(files):
        """The newest committed profile summary collected on THIS workload (its `command` names it: bench.py --workload X, default ns) with
        THIS run's generator overrides (tools/profile_pass.sh writes the HIPSTR_SYNTH_* settings of a pass in front of the command: the
        interrupted-repeat modes have summaries of their own): counters of one workload are not scaled onto another."""
        import re
        mine = sorted("%s=%s" % (k, v) for k, v in os.environ.items() if k.startswith("HIPSTR_SYNTH"))
        for f in reversed(files):
            t = json.load(open(f))
            cmd = t.get("command", "")
            theirs = sorted(re.findall(r"HIPSTR_SYNTH\w*=\S+", cmd))
            if not theirs and re.search(r"_(imperfect|inherit)\d*_", os.path.basename(f)):
                continue            # (a summary of an interrupted-repeat pass from before the overrides were recorded)
            m = re.search(r"--workload\s+(\w+)", cmd)
            if (m.group(1) if m else "ns") == args.workload and theirs == mine:
                return t, f
        return None, None

    pass_traffic = {}
    STR_KERNELS = ("hs_str_", "hs_nd_")          # the STR phase: read-end sums + group kernels + per-read / generic kernels

    def pmc_traffic(kernel_key, n_alignments):
        """HBM-side traffic of the dominant kernel from the newest committed rocprofv3 PMC summary (profiles/*_pmc_traffic.json:
        FETCH_SIZE and WRITE_SIZE collected in separate --pmc passes, tools/pmc_traffic.py), scaled to this launch by alignments.
        FETCH_SIZE is doubled per MI355X_MICROARCH.md §HBM (gfx950 counts a 128-B request as 64 B) — an upper bound for the
        narrow accesses of these kernels; WRITE_SIZE is uncalibrated and taken raw."""
        import glob
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), key=_profile_key)
        t, src = profile_for(files)
        if t is None:
            return None, None
        keys = STR_KERNELS if kernel_key.startswith("hs_str") else (kernel_key,)
        hit = [v for name, v in t["kernels"].items() if name.startswith(keys)]            # a phase may be more than one kernel
        if not hit:
            return None, None
        per_aln = sum(2 * v["fetch_bytes_per_launch_raw"] + v["write_bytes_per_launch_raw"] for v in hit) / t["alignments_per_launch"]
        # the whole launch set (every kernel of a pass), raw and with the guide's FETCH x 2: the figure that stands next to the
        # algorithmic bytes of the launch set (VERDICT r05 weak 10 iii: the per-kernel figure alone mixes scopes)
        allk = list(t["kernels"].values())
        raw = sum(v["fetch_bytes_per_launch_raw"] + v["write_bytes_per_launch_raw"] for v in allk) / t["alignments_per_launch"]
        cor = sum(2 * v["fetch_bytes_per_launch_raw"] + v["write_bytes_per_launch_raw"] for v in allk) / t["alignments_per_launch"]
        pass_traffic.update(raw=raw * n_alignments, fetch_x2=cor * n_alignments, per_alignment_raw=raw, per_alignment_fetch_x2=cor)
        return per_aln * n_alignments, os.path.basename(src)

    def valu_block(phase_ms_now, n_alignments):
        """The limiter that binds, per phase, from the newest committed counter passes (profiles/r*_sq_counters.json: two rocprofv3 --pmc
        runs, tools/profile_pass.sh + tools/sq_counters.py) scaled to this launch by alignments and divided by the LIVE phase durations:
          fp64_frac_of_peak  executed FP64 add/max instructions x 4 cycles / (1024 SIMDs x 2.4 GHz x duration) = executed FP64 ops against
                             the 39.3 T FP64-VALU-op/s peak (256 CU x 4 SIMD x 16 lanes x 2.4 GHz)
          pipe_occupancy_*   VALU pipe time of ALL executed VALU instructions with the measured per-class issue costs
                             (profiles/r*_valu_microbench.json): low = every non-FP64 instruction 2 cycles, high = 4 cycles, est = split
                             by the kernel's static instruction histogram (profiles/r*_isa_histogram.json).
        profile_matches_build says whether the counters were collected on the kernel source this library was built from."""
        import glob
        import hashlib
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_sq_counters.json")), key=_profile_key)
        files = [f for f in files if "kernel_source_sha1" in open(f).read()]
        t, src_file = profile_for(files)
        if t is None:
            return None
        src = os.path.join(ROOT, "hipstr_amd", "csrc", "hmm_kernels.hip")
        same = os.path.exists(src) and hashlib.sha1(open(src, "rb").read()).hexdigest() == t.get("kernel_source_sha1")
        denom_per_ms = t["simds"] * t["clock_hz"] * 1e-3
        cyc = t["cycles_per_wave64_instruction"]
        phases = {}
        for ph, ms_now in phase_ms_now.items():
            key = STR_KERNELS if ph.startswith("hs_str") else (ph,)
            hit = [v for name, v in t["kernels"].items() if name.startswith(key)]     # a phase may be more than one kernel (the STR phase: read-end sums + group + generic)
            if not hit or not (ms_now == ms_now) or ms_now <= 0:
                continue
            sc = n_alignments / t["alignments_per_launch"]
            f64 = sum(v["fp64_arith_insts"] for v in hit) * sc; rest = sum(v["other_valu_insts"] for v in hit) * sc
            wide = sum(v["other_valu_insts"] * (v["static_histogram"]["wide_share_of_non_fp64"] or 1.0) for v in hit) * sc
            d = denom_per_ms * ms_now
            phases[ph] = {"valu_insts": f64 + rest, "fp64_insts": f64, "fp64_ops_per_s": f64 * 64 / (ms_now * 1e-3),
                          "fp64_frac_of_peak": f64 * cyc["fp64"] / d,
                          "pipe_occupancy_low": (f64 * cyc["fp64"] + rest * cyc["simple32"]) / d,
                          "pipe_occupancy_est": (f64 * cyc["fp64"] + wide * cyc["other"] + (rest - wide) * cyc["simple32"]) / d,
                          "pipe_occupancy_high": (f64 * cyc["fp64"] + rest * cyc["other"]) / d}
        tot_ms = sum(ms for ph, ms in phase_ms_now.items() if ph in phases)
        allf = sum(v["fp64_insts"] for v in phases.values())
        return {"fp64_valu_peak_ops_per_s": 256 * 4 * 16 * 2.4e9, "cycles_per_wave64_instruction": cyc,
                "pass_fp64_frac_of_peak": (allf * cyc["fp64"] / (denom_per_ms * tot_ms)) if tot_ms > 0 else None,
                "phases": phases, "source": os.path.basename(src_file), "profile_matches_build": bool(same)}

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = total_aln * args.steps / elapsed
        out = {
            "metric": "read x allele HMM alignments/sec", "value": value, "unit": "alignments/s",
            "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s: %s" % (args.workload, desc) if not args.loci else "%s with %d loci%s: %s" % (args.workload, args.loci, "/GPU" if args.scaling == "weak" else " in total", desc),
                       "loci_per_gpu": loci, "first_locus_rank0": first, "reads_per_locus": P, "alleles_per_locus": A, "read_len": L,
                       "alignments_per_step_per_gpu": n_aln.value, "sharding": "loci across ranks, no collective on the data path",
                       "str_allele_sides_by_kernel": str_kinds},
            "loci_per_sec": total_loci * args.steps / elapsed,
        }
    if rank == 0 and args.full:
        achieved = algo.value / (kernel_ms * 1e-3) / 1e9 if kernel_ms == kernel_ms else None
        traffic, traffic_src = pmc_traffic(phase_names[dom].split("<")[0], n_aln.value)
        valu = valu_block(dict(zip(phase_names, [float(x) for x in phase_ms])), n_aln.value) if n_ms > 0 else None
        out.update({
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                         "frac": (achieved / 8000.0) if achieved else None, "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_scope": "the dominant kernel's launches of one pass (FETCH_SIZE x 2 + WRITE_SIZE)",
                         "traffic_pass": ({"raw": pass_traffic["raw"], "fetch_x2": pass_traffic["fetch_x2"],
                                           "over_algorithmic_raw": pass_traffic["raw"] / max(1, algo.value), "over_algorithmic_fetch_x2": pass_traffic["fetch_x2"] / max(1, algo.value),
                                           "bytes_per_alignment_raw": pass_traffic["per_alignment_raw"], "bytes_per_alignment_fetch_x2": pass_traffic["per_alignment_fetch_x2"],
                                           "scope": "every kernel of the launch set, scaled to this batch by alignments"} if pass_traffic else None),
                         "pass_ms": float(phase_ms.sum()) if n_ms > 0 else None,
                         "kernel": phase_names[dom], "kernel_ms": kernel_ms,
                         "phase_ms": dict(zip(phase_names, [float(x) for x in phase_ms])), "algorithmic_bytes_per_launch": algo.value,
                         "bytes_per_alignment": algo.value / max(1, n_aln.value)},
            # the roof that binds (an FP64 max-plus recurrence — neither HBM nor MFMA): executed FP64 wave-instructions x 64
            # lanes / the LIVE kernel time, against 256 CU x 4 SIMD x 16 lanes x 2.4 GHz (tools/valu_microbench.hip: 4 cycles per wave64 FP64 op)
            "roofline_fp64": ({"bound": "fp64_valu_issue", "kernel": phase_names[dom],
                               "achieved": valu["phases"][phase_names[dom]]["fp64_ops_per_s"] / 1e12 if phase_names[dom] in valu["phases"] else None,
                               "peak": 256 * 4 * 16 * 2.4e9 / 1e12, "unit": "T FP64 op/s",
                               "frac": valu["phases"][phase_names[dom]]["fp64_frac_of_peak"] if phase_names[dom] in valu["phases"] else None,
                               "pass_frac": valu["pass_fp64_frac_of_peak"],
                               "phase_frac": {ph: v["fp64_frac_of_peak"] for ph, v in valu["phases"].items()},
                               "phase_valu_pipe_est": {ph: v["pipe_occupancy_est"] for ph, v in valu["phases"].items()},
                               # what a stream of INDEPENDENT FP64 instructions reaches on this device (profiles/r02_valu_microbench.json: cycles of one
                               # SIMD per wave64 v_add_f64 / v_max_f64, 8 register chains): 6.06 at one wavefront per SIMD, 4.94 at two, 4.47 at four —
                               # the nominal 4 is not reached by any occupancy; the trailing-flank kernel runs three per SIMD (168 registers)
                               "measured_issue_ceiling": {"cycles_per_fp64_inst": {"1_wave_per_simd": 6.06, "2_waves_per_simd": 4.94, "4_waves_per_simd": 4.47},
                                                          "frac_of_nominal_at_2_to_4_waves": [4 / 4.94, 4 / 4.47], "source": "profiles/r02_valu_microbench.json"},
                               "counters": valu["source"], "profile_matches_build": valu["profile_matches_build"]} if valu else None),
            "valu": valu,
            "host": {"synth_s": t_gen, "prepare_upload_s": t_upload, "prepare_upload_first_call_s": t_upload_cold, "fetch_s": t_fetch,
                     "value_incl_prepare_pcie": total_aln / world / (t_upload + elapsed / args.steps + t_fetch) * world},
        })
        if args.gpus == 1 and not args.no_pipeline:
            # passes: as many as the resident measurement, but at least ~120 M alignments' worth (about a second) — a stream that sees a few batches
            # measures its own fill and drain, not its rate (round 6: p30 under the 2-CPU pin 0.78-0.83 of resident over 31 passes, 0.87-0.94 over 150)
            e2e = end_to_end(capi, hmm, sb, loci, max(2, min(args.steps, 5), min(128, int(1.2e8 // max(1.0, float(n_aln.value))))), local)
            e2e["alignments_per_s"] = n_aln.value * e2e["passes"] / e2e["seconds"]
            e2e["fraction_of_resident_rate"] = e2e["alignments_per_s"] / value
            out["end_to_end"] = e2e
            # SURVEY §8(d)'s metric taken literally (host arrays in -> results out: host flatten + H2D + kernels + D2H), beside `value`
            # (inputs resident, as the bench contract defines it)
            out["value_end_to_end"] = e2e["alignments_per_s"]
            out["value_resident"] = value
            e2e["host_threads"] = int(os.environ.get("HIPSTR_HOST_THREADS", "0")) or usable_cores()
            out["pipeline"] = pipeline_stages(capi, hmm, sb, loci, P)
        if per_rank is not None:
            out["cross_device_check"] = cross_check
            out["per_rank_alignments_per_s"] = per_rank
            out["ranks"] = rank_info
            out["host_threads_per_rank"] = int(os.environ.get("HIPSTR_HOST_THREADS", host_threads))
        if e2e_multi is not None:
            out["end_to_end"] = e2e_multi
            out["value_end_to_end"] = e2e_multi["alignments_per_s"]
        if args.gpus == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(capi, args.workload, n_loci=loci)
        if args.workload == "c4":
            # shares of the step: the stages once more, each waited for (not part of the timed region)
            torch.cuda.synchronize(); t_a = time.perf_counter()
            hmm.hipstr_hmm_align(dev, None); torch.cuda.synchronize(); t_b = time.perf_counter()
            hmm.hipstr_post_launch(pd, None); torch.cuda.synchronize(); t_c = time.perf_counter()
            hmm.hipstr_post_extract(pd, C.byref(rq), C.byref(gt_o)); t_d = time.perf_counter()
            tot = t_d - t_a
            out["c4_step"] = {"samples_per_locus": 1000, "forward_hmm_s": t_b - t_a, "posterior_kernel_s": t_c - t_b, "genotype_calls_s": t_d - t_c,
                              "posterior_share": (t_c - t_b) / tot, "genotype_calls_share": (t_d - t_c) / tot,
                              "note": "hipstr_post_launch = hs_posterior_kernel (R x A^2 pair log-sum-exps per sample); genotype calls = hs_genotype_kernel + GL/PL copy back"}
        if em_stats:
            out["c3_step"] = {"stutter_em_s_per_step": em_stats.get("em_s", 0.0) / args.steps, "genotype_calls_s_per_step": em_stats.get("calls_s", 0.0) / args.steps,
                              "em_trained_loci": em_stats.get("trained"), "em_iterations": em_stats.get("iterations"), "samples_per_locus": 100}
        if args.gpus == 1 and not args.no_pipeline and "end_to_end" in out:
            # the same measurement with the host share one rank has when 8 ranks share this node's usable cores: a child process pinned
            # to usable_cores/8 CPUs (all of its threads) with as many library host threads
            if not args.host_threads and not os.environ.get("HIPSTR_BENCH_NO_SHARE"):
                import subprocess
                hmm.hipstr_hmm_trim()          # what this process' streams and calls cached and no longer use: the child needs the device memory (last measurement of the line: nothing after it pays for cold caches)
                n8 = max(1, usable_cores() // 8)
                cmd = [sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--steps", str(args.steps), "--e2e-only", "--host-threads", str(n8)]
                if args.loci:
                    cmd += ["--loci", str(args.loci)]
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
                    if r.returncode != 0 or not r.stdout.strip():
                        raise RuntimeError("child rc %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
                    sh = json.loads(r.stdout.strip().splitlines()[-1])
                    sh["fraction_of_resident_rate"] = sh["alignments_per_s"] / value
                    sh["note"] = "child process of this run pinned to %d of the node's %d usable CPUs (= usable/8: one rank's share at 8 GPUs), HIPSTR_HOST_THREADS=%d" % (n8, usable_cores(), n8)
                    out["end_to_end_host_share_8gpu"] = sh
                    out["value_end_to_end_host_share_8gpu"] = sh["alignments_per_s"]
                except Exception as ex:            # the line must not depend on it
                    out["end_to_end_host_share_8gpu"] = {"error": repr(ex)[:200]}
                # ... and the shape that is actually host-sensitive: thousands of small loci per batch (--workload p30: 4000 loci x 40 reads x 8
                # alleles, 35-bp flanks), the same pinned child; its resident rate is measured in the same process
                if args.workload == "ns" and not args.loci and not os.environ.get("HIPSTR_BENCH_NO_P30_SHARE"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--workload", "p30", "--steps", "5", "--e2e-only", "--host-threads", str(n8)]
                    try:
                        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
                        if r.returncode != 0 or not r.stdout.strip():
                            raise RuntimeError("child rc %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
                        sh = json.loads(r.stdout.strip().splitlines()[-1])
                        sh["fraction_of_resident_rate"] = sh["fraction_of_resident_rate_same_process"]
                        sh["note"] = "workload p30 (%s) in a child process pinned to %d of the node's %d usable CPUs, HIPSTR_HOST_THREADS=%d; resident rate of the same child" % (WORKLOADS["p30"][6], n8, usable_cores(), n8)
                        out["end_to_end_host_share_8gpu_p30"] = sh
                        out["value_end_to_end_host_share_8gpu_p30"] = sh["alignments_per_s"]
                    except Exception as ex:
                        out["end_to_end_host_share_8gpu_p30"] = {"error": repr(ex)[:200]}
    if rank == 0:
        print(json.dumps(out), flush=True)
    hmm.hipstr_post_free(pd)
    hmm.hipstr_hmm_free(dev)
    released = int(hmm.hipstr_hmm_trim())           # the caches' idle chunks back to the driver: a rank leaves the device as it found it
    if os.environ.get("HIPSTR_BENCH_VERBOSE"):
        st8 = (C.c_int64 * 12)(); hmm.hipstr_debug_cache_stats(st8)
        print("rank %d: released %d bytes, still held: device %d, pinned %d" % (rank, released, st8[0], st8[4]), file=sys.stderr, flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
