"""One hipstr_post_assign call at the chain shape (64 loci x 500 reads x 5 samples x 32 alleles) and at 1000 x 500 x 5, beside the host-side
pick it replaces (hipstr_hmm_fetch of the likelihood matrix + the numpy select of bench.py's chain).  Usage: python tools/assign_timing.py [OUT.json]  (default profiles/assign_stage_timing.json; needs an MI355X)."""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipstr_amd import capi

hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
P, S, A_str = 500, 5, 32
res = {"reads_per_locus": P, "samples_per_locus": S, "str_alleles": A_str, "shapes": []}
for nc in (64, 1000):
    cb = capi.SynthBatch(n_loci=nc, reads_per_locus=P, n_str_alleles=A_str, seed=4242)
    A_c = np.diff(np.ctypeslib.as_array(cb.ptr.contents.hap_off, shape=(nc + 1,)))
    lab = np.tile(np.repeat(np.arange(S), P // S), nc)
    dev = hmm.hipstr_hmm_upload(cb.ptr); assert dev
    assert hmm.hipstr_hmm_align(dev, None) == 0
    n = nc * P
    rng = np.random.default_rng(1)
    pbc = capi.PostBatch(A_c, np.full(nc, S, np.int32), np.arange(nc + 1, dtype=np.int32) * P, lab, -rng.random(n), -rng.random(n), np.ones(n, np.int32), None)
    pdc = hmm.hipstr_post_upload(pbc.ptr, hmm.hipstr_hmm_dev_aln_probs(dev)); assert pdc
    assert hmm.hipstr_post_launch(pdc, None) == 0
    seeds = np.zeros(n, np.int32); assert hmm.hipstr_calc_seed_bases(cb.ptr, seeds.ctypes.data_as(capi._i32p)) == 0
    pool = np.tile(np.arange(P), nc); pool_off = np.arange(nc + 1) * P
    # host-side pick: fetch + numpy select (bench.py chain)
    host = []
    for rep in range(5):
        t0 = time.perf_counter()
        ll = np.zeros(cb.n_out); sd = np.zeros(cb.n_reads, np.int32)
        hmm.hipstr_hmm_fetch(dev, ll.ctypes.data_as(capi._f64p), sd.ctypes.data_as(capi._i32p))
        post = np.zeros(int(pbc.post_off[-1])); tot = np.zeros(nc * S); gt = np.zeros(2 * nc * S, np.int32); lt = np.zeros(nc)
        hmm.hipstr_post_fetch(pdc, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p), lt.ctypes.data_as(capi._f64p))
        t1 = time.perf_counter()
        g2 = gt.reshape(-1, 2); rr_c, aa_c = [], []
        for l in range(nc):
            a = int(A_c[l]); r0 = l * P
            LLl = ll[cb.out_off[l]:cb.out_off[l + 1]].reshape(P, a)
            g = g2[l * S + lab[r0:r0 + P]]
            best = np.where(LLl[np.arange(P), g[:, 0]] > LLl[np.arange(P), g[:, 1]], g[:, 0], g[:, 1])
            ok = sd[r0:r0 + P] >= 0
            rr_c.append(np.nonzero(ok)[0] + r0); aa_c.append(best[ok])
        rr_c = np.concatenate(rr_c).astype(np.int32); aa_c = np.concatenate(aa_c).astype(np.int32)
        t2 = time.perf_counter()
        host.append((t1 - t0, t2 - t1))
    # device: the call alone (arrays prepared), with and without the request list
    def timed(**kw):
        ts = []
        for rep in range(9):
            t0 = time.perf_counter()
            o = capi.run_assign(hmm, pdc, seeds, n_reads=n, n_samp=nc * S, rule=capi.ASSIGN_RETRACE, **kw)
            ts.append(time.perf_counter() - t0)
        return o, ts
    o_req, t_req = timed(pool_index=pool, pool_off=pool_off)
    o_cnt, t_cnt = timed()
    # same picks as the host's (log_p terms aside: the host pick of bench.py ignores them; compare where they cannot matter)
    med = lambda v: sorted(v)[len(v) // 2]
    res["shapes"].append({"loci": nc, "reads": n, "ll_bytes": int(cb.n_out) * 8, "requests": o_req["n_req"],
                          "host_fetch_s": med([h[0] for h in host]), "host_numpy_select_s": med([h[1] for h in host]),
                          "host_pick_total_s": med([h[0] + h[1] for h in host]),
                          "post_assign_with_request_list_s": med(t_req), "post_assign_with_request_list_first_call_s": t_req[0],
                          "post_assign_counts_only_s": med(t_cnt), "calls": 9, "of": "median (python wrapper included: output arrays allocated per call)"})
    print(json.dumps(res["shapes"][-1]), flush=True)
    hmm.hipstr_post_free(pdc); hmm.hipstr_hmm_free(dev); cb.close()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "assign_stage_timing.json")
json.dump(res, open(OUT, "w"), indent=1)
