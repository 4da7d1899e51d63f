"""Cases of hipstr_post_extract_vcf (include/hipstr_hmm.h): posterior batches of a few loci, allele orders, and the numpy restatement of
write_vcf_record's index rules (seq_stutter_genotyper.cpp:1436-1481) that the call is held to — no reference binary prints the permuted
arrays, so the yardstick is hipstr_post_extract's own output (pinned to the oracle and the compiled reference by tests/test_genotypes_*.py)
gathered through those rules."""
import numpy as np


def post_batch(capi, seed, loci, reads_per_sample=5):
    """loci: (A haplotypes, V variants, S samples, haploid) each -> (PostBatch, n_variants, hap_to_allele).  Haplotype a carries variant
    a % V, so every variant is carried; a haploid locus gets log_p1 == log_p2."""
    rng = np.random.default_rng(seed)
    n_alleles = [l[0] for l in loci]; n_samples = [l[2] for l in loci]; haploid = [int(l[3]) for l in loci]
    label = np.concatenate([np.repeat(np.arange(S), reads_per_sample) for S in n_samples] + [np.zeros(0, np.int64)])
    read_off = np.concatenate([[0], np.cumsum([S * reads_per_sample for S in n_samples])])
    n = int(read_off[-1])
    lp1 = -rng.random(n); lp2 = -rng.random(n)
    for l, h in enumerate(haploid):
        if h:
            lp2[read_off[l]:read_off[l + 1]] = lp1[read_off[l]:read_off[l + 1]]
    ll = np.concatenate([-rng.random(S * reads_per_sample * A) * 30 for A, S in zip(n_alleles, n_samples)] + [np.zeros(0)])
    pb = capi.PostBatch(n_alleles=n_alleles, n_samples=n_samples, read_off=read_off, sample_label=label, log_p1=lp1, log_p2=lp2,
                        read_weight=np.ones(n, np.int32), log_aln_probs=ll, haploid=haploid)
    h2a = np.concatenate([np.arange(l[0]) % l[1] for l in loci]).astype(np.int32)
    return pb, np.asarray([l[1] for l in loci], np.int32), h2a


def orders(seed, n_variants, identity=False):
    """Per locus a permutation with the reference allele first -> (new_to_old, old_to_new), each [sum V]."""
    rng = np.random.default_rng(seed)
    n2o = []; o2n = []
    for V in n_variants:
        p = np.concatenate([[0], 1 + (np.arange(V - 1) if identity else rng.permutation(V - 1))]).astype(np.int32)
        inv = np.empty(V, np.int32); inv[p] = np.arange(V, dtype=np.int32)
        n2o.append(p); o2n.append(inv)
    return np.concatenate(n2o), np.concatenate(o2n)


def permute_gt_outputs(got, pb, n_variants, new_to_old, old_to_new):
    """The index rules of seq_stutter_genotyper.cpp:1436-1481 applied to run_post_extract_flat's output of hipstr_post_extract: what
    hipstr_post_extract_vcf must return for the same request (arrays that were not requested keep their fill)."""
    nl = pb.struct.n_loci
    hap = pb.a["haploid"] if pb.a["haploid"] is not None else np.zeros(nl, np.uint8)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in got.items()}
    gl_off, pgl_off = got["gl_off"], got["pgl_off"]
    s = 0; vo = 0
    for l in range(nl):
        V = int(n_variants[l])
        n2o = np.asarray(new_to_old[vo:vo + V], np.int64); o2n = np.asarray(old_to_new[vo:vo + V], np.int64)
        if hap[l]:
            gl_src = n2o; pgl_src = n2o
        else:
            i, j = np.tril_indices(V)                               # row-major over j <= i: i(i+1)/2 + j
            a = np.minimum(n2o[i], n2o[j]); b = np.maximum(n2o[i], n2o[j])
            gl_src = b * (b + 1) // 2 + a                           # :1450-1470
            pgl_src = (n2o[:, None] * V + n2o[None, :]).reshape(-1)  # :1472-1481
        for _ in range(int(pb.a["n_samples"][l])):
            g = got["best_gt"][s]
            out["best_gt"][s] = [o2n[x] if x >= 0 else x for x in g]
            g0, p0 = int(gl_off[s]), int(pgl_off[s])
            out["gls"][g0:g0 + len(gl_src)] = got["gls"][g0 + gl_src]
            out["pls"][g0:g0 + len(gl_src)] = got["pls"][g0 + gl_src]
            out["phased_gls"][p0:p0 + len(pgl_src)] = got["phased_gls"][p0 + pgl_src]
            s += 1
        vo += V
    return out
