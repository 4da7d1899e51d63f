"""CPU: per-locus, asymmetric stutter models (tests/stutter_models.py).
  a. the stutter_models_* cases of tests/cases.py can see what they are for — judged on the oracle, never on a device: most entries move when
     a locus' model is replaced by the default one or by its up / down mirror image, and the tracebacks carry artifacts of both signs;
  b. the host plumbing keeps a model with its locus: shard.subset_arrays, the flat batch format, the pooler's and the haplotype
     generator's output batches (host forms), the merge of the host preparation's fragments;
  c. a model outside the domain of the reference's StutterModel (stutter_model.h:35-39) is refused on the host, by the preparation and by
     the traceback's request check — nothing out of domain is ever handed to a device."""
import ctypes as C
import os

import numpy as np
import pytest

from hipstr_amd import capi, shard
import stutter_models as sm
import util
from cases import CASES

GOLD = sm.GOLD
MODEL_CASES = ["stutter_models_periodic", "stutter_models_interrupted", "stutter_models_inherited", "stutter_models_edges"]
FILL = -12345.678


# ---------------------------------------------------------------------------------------------------------------- the table
def test_models_are_in_the_reference_domain_and_distinct():
    assert len(sm.MODELS) == 10 and len(sm.NON_DEFAULT) == 9 and sm.MODELS["default"] == util.STUTTER
    for name, m in sm.MODELS.items():
        assert sm.in_domain(m), name
    rows = {tuple(m) for m in sm.MODELS.values()}
    assert len(rows) == 10
    for name in sm.NON_DEFAULT:       # asymmetric in frame: the mirror image is another model
        assert sm.swap_up_down(name) != sm.MODELS[name] and sm.swap_up_down(sm.swap_up_down(name)) == sm.MODELS[name], name
    d = np.load(os.path.join(GOLD, "scalars.npz"))
    assert list(d["pmf_params"][1]) == sm.MODELS["up_heavy"]
    assert sm.rotate([1, 2, 3], 1) == [2, 3, 1] and sm.rotate([1, 2, 3], -1) == [3, 1, 2]


def test_with_models_changes_the_models_only():
    b = CASES["synth_multiflank"]()
    m = sm.with_models(b, ["tiny", sm.MODELS["heavy"]])
    da, db = util.batch_to_dict(b), util.batch_to_dict(m)
    assert all(np.array_equal(da[k], db[k]) for k in da if k != "stutter")
    assert db["stutter"].reshape(-1, 6).tolist() == [sm.MODELS["tiny"], sm.MODELS["heavy"]] * 2
    assert np.array_equal(b.arrays["stutter"].reshape(-1, 6), [util.STUTTER] * 4)       # the source batch is left alone


# ---------------------------------------------------------------------------------------------------------------- a. the cases see
@pytest.fixture(scope="module")
def case_runs(oracle):
    """name -> (batch, oracle's aln_probs, seeds): computed once, shared, never changed."""
    out = {}
    for name in MODEL_CASES:
        b = util.batch_from_dict(np.load(os.path.join(GOLD, "align_%s.npz" % name)))
        out[name] = (b,) + capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
    return out


@pytest.mark.parametrize("name", MODEL_CASES)
def test_fixtures_hold_the_cases_of_the_case_file(name):
    """Six loci, one non-default model each; the golden file's inputs are what tests/cases.py builds."""
    d = np.load(os.path.join(GOLD, "align_%s.npz" % name))
    want = util.batch_to_dict(CASES[name]())
    assert all(np.array_equal(d[k], want[k]) for k in want)
    models = d["stutter"].reshape(-1, 6).tolist()
    assert len(models) == 6 and len({tuple(m) for m in models}) == 6
    assert all(m in [sm.MODELS[n] for n in sm.NON_DEFAULT] for m in models)
    t = np.load(os.path.join(GOLD, "trace_%s.npz" % name))
    assert int(t["n_traced"][0]) == 6
    assert [t["L%d_stutter" % i].tolist() for i in range(6)] == models


@pytest.mark.parametrize("name", MODEL_CASES)
def test_entries_move_with_the_model_and_with_its_mirror_image(oracle, case_runs, name):
    """At least half of the written entries of every locus differ from the same locus under the default model, and from it under the
    model with up and down exchanged (measured: 72 % and 67 % at the least; the shares are printed)."""
    b, own, seeds = case_runs[name]
    models = b.arrays["stutter"].reshape(-1, 6)
    dflt, s1 = capi.run_align(oracle, "oracle_", sm.with_models(b, ["default"]).ptr, fill=FILL)
    swap, s2 = capi.run_align(oracle, "oracle_", sm.with_models(b, [sm.swap_up_down(m) for m in models]).ptr, fill=FILL)
    assert np.array_equal(s1, seeds) and np.array_equal(s2, seeds)
    for l in range(len(models)):
        o, d, s = (sm.locus_rows(b, x, l) for x in (own, dflt, swap))
        written = o != FILL
        assert np.array_equal(written, d != FILL) and np.array_equal(written, s != FILL) and written.sum() >= 40, (name, l)
        share_d, share_s = float((o != d)[written].mean()), float((o != s)[written].mean())
        print("%s locus %d: %d written entries, %.0f %% differ from default, %.0f %% from the mirror image" % (name, l, written.sum(), 100 * share_d, 100 * share_s))
        assert share_d >= 0.5 and share_s >= 0.5, (name, l, share_d, share_s)


def test_tracebacks_hold_artifacts_of_both_signs_under_every_model(oracle, case_runs):
    """Over the oracle's tracebacks of every (seeded read, allele) pair of the four cases: at least 3 requests with stutter_size > 0 and at
    least 3 with stutter_size < 0 under every model (for each locus at that; the lowest count seen is 4)."""
    by_model = {n: [0, 0] for n in sm.NON_DEFAULT}
    names = {tuple(sm.MODELS[n]): n for n in sm.NON_DEFAULT}
    for case in MODEL_CASES:
        b, _, seeds = case_runs[case]
        a = b.arrays
        for l in range(len(a["period"])):
            one = shard.batch_from_arrays(shard.subset_arrays(a, l, l + 1))
            r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1]); A = int(a["hap_off"][l + 1] - a["hap_off"][l])
            rr = [r - r0 for r in range(r0, r1) if seeds[r] >= 0 and (a["realign_read"] is None or a["realign_read"][r])]
            tr = capi.run_trace(oracle, "oracle_", one.ptr, [r for r in rr for _ in range(A)], [k for _ in rr for k in range(A)],
                                util.synthetic_hap_to_ref(oracle, one.ptr), cap=1 << 22)
            sizes = [t["stutter_size"] for t in tr if t["stutter_size"] != -100000]           # HIPSTR_NO_STR_DATA
            up, down = sum(x > 0 for x in sizes), sum(x < 0 for x in sizes)
            assert up >= 3 and down >= 3, (case, l, up, down)
            m = by_model[names[tuple(a["stutter"][6 * l:6 * l + 6])]]
            m[0] += up; m[1] += down
    assert all(up >= 3 and down >= 3 for up, down in by_model.values()), by_model


# ---------------------------------------------------------------------------------------------------------------- b. host plumbing
@pytest.fixture(scope="module")
def nine():
    """Nine loci, nine different models."""
    return sm.synth(sm.NON_DEFAULT, n_loci=9, reads_per_locus=6, n_str_alleles=4, seed=311)


def test_subset_arrays_keeps_the_model_with_its_locus(oracle, nine):
    a = nine.arrays
    want, ws = capi.run_align(oracle, "oracle_", nine.ptr, fill=FILL)
    models = a["stutter"].reshape(-1, 6)
    assert len({tuple(m) for m in models.tolist()}) == 9
    off = capi.batch_dims(nine.ptr)[2]
    for lo in range(9):
        for hi in range(lo + 1, 10):
            cut = shard.subset_arrays(a, lo, hi)
            assert np.array_equal(cut["stutter"].reshape(-1, 6), models[lo:hi]), (lo, hi)
            if hi - lo <= 2:       # and the cut aligns as its loci did in the batch
                got, _ = capi.run_align(oracle, "oracle_", shard.batch_from_arrays(cut).ptr, fill=FILL)
                assert np.array_equal(got, want[off[lo]:off[hi]]), (lo, hi)


def test_flat_batch_format_keeps_the_models(hmm_host, nine, tmp_path):
    from test_batch_io import _api
    lib = _api(hmm_host)
    path = str(tmp_path / "models.hsb").encode()
    assert lib.hipstr_batch_write(path, nine.ptr) == 0
    f = lib.hipstr_batch_read(path)
    assert f, lib.hipstr_last_error()
    back = capi.batch_arrays(lib.hipstr_batch_file_batch(f))
    want = util.batch_to_dict(nine)
    assert np.array_equal(back["stutter"], want["stutter"]) and back["stutter"].reshape(-1, 6).tolist() == [sm.MODELS[n] for n in sm.NON_DEFAULT]
    for k in util._ARRAY_KEYS:
        assert np.array_equal(back[k], want[k]), k
    lib.hipstr_batch_file_free(f)


def test_pooled_batch_keeps_the_models(hmm_host, nine):
    pb = capi.PooledBatch(hmm_host, nine.ptr, capi.POOL_ON_HOST)
    got = pb.arrays()
    assert np.array_equal(got["period"], nine.arrays["period"]) and np.array_equal(got["stutter"], nine.arrays["stutter"])
    pb.close()


def hapgen_inputs():
    """Loci of the haplotype generator's golden batches, some of which it refuses, every one with a model of its own: (reads batch,
    request, models)."""
    import hapgen_cases as hc
    loci = hc.load_golden("unit_status")[0] + hc.load_golden("unit_extract")[0][:4] + hc.no_flagged_loci()
    names = list(sm.MODELS)
    models = [sm.MODELS[names[l % len(names)]] for l in range(len(loci))]
    loci = [dict(lc, stutter=m) for lc, m in zip(loci, models)]
    return hc.ReadsBatch(loci), hc.request_of(loci), models


def test_hapgen_batch_copies_the_model_of_the_source_locus(hmm_host):
    """hipstr_hapgen_batch(HIPSTR_HAPGEN_ON_HOST): output locus k is input locus locus[k]; with refused loci in front the two indices differ."""
    b, rq, models = hapgen_inputs()
    hb = capi.HapgenBatch(hmm_host, b.ptr, rq, capi.HAPGEN_ON_HOST)
    keep = hb.locus.tolist()
    assert 0 < len(keep) < len(models) and sum(k != l for k, l in enumerate(keep)) >= 3, keep
    assert hb.arrays()["stutter"].reshape(-1, 6).tolist() == [models[l] for l in keep]
    assert len({tuple(models[l]) for l in keep}) >= min(len(keep), 4)
    hb.close()


def _digest(lib, bptr, threads):
    sec, dig = C.c_double(), C.c_uint64()
    assert lib.hipstr_debug_prepare(bptr, threads, C.byref(sec), C.byref(dig)) == 0, lib.hipstr_last_error()
    return dig.value


def test_preparation_digest_with_one_and_with_four_threads(hmm_host):
    """prepare_batch cuts a batch into min(n_loci, 4 * threads) fragments for min(threads, n_loci / 4) threads and merges them, rebasing
    every fragment-local offset — the stutter pmf's (pmf_off) among them.  20 loci with 4 threads: 4 threads, 16 fragments; with one
    thread there is no fragment at all.  The digest covers the 13 pmf values per locus and every option's offsets."""
    models = sm.rotate(sm.NON_DEFAULT, 2)
    b = sm.synth(models, n_loci=20, reads_per_locus=5, n_str_alleles=5, n_flank_opts=2, seed=312)
    d1, d4 = _digest(hmm_host, b.ptr, 1), _digest(hmm_host, b.ptr, 4)
    assert d1 == d4
    # two loci exchange their models (in different fragments, and in one): another digest, again the same for both thread counts
    for i, j in ((3, 17), (8, 9)):
        m = [models[l % 9] for l in range(20)]
        m[i], m[j] = m[j], m[i]
        x = sm.with_models(b, m)
        e1, e4 = _digest(hmm_host, x.ptr, 1), _digest(hmm_host, x.ptr, 4)
        assert e1 == e4 and e1 != d1, (i, j)
    assert _digest(hmm_host, sm.with_models(b, sm.rotate(models, 1)).ptr, 4) != d4


# ---------------------------------------------------------------------------------------------------------------- c. out of domain
NAN, INF = float("nan"), float("inf")
OUT_OF_DOMAIN = {
    "in_geom_zero": (0, 0.0), "in_geom_one": (0, 1.0), "in_geom_negative": (0, -0.1), "in_geom_above_one": (0, 1.5),
    "out_geom_zero": (3, 0.0), "out_geom_one": (3, 1.0), "out_geom_negative": (3, -1e-9), "out_geom_above_one": (3, 2.0),
    "in_up_zero": (1, 0.0), "in_down_zero": (2, 0.0), "out_up_zero": (4, 0.0), "out_down_zero": (5, 0.0),
    "in_up_negative": (1, -0.05), "in_down_negative": (2, -1e-12), "out_up_negative": (4, -0.005), "out_down_negative": (5, -1.0),
    "sum_is_one": (None, [0.9, 0.5, 0.25, 0.7, 0.125, 0.125]), "sum_above_one": (2, 0.97),      # (binary fractions: the sum is 1 exactly)
    "in_geom_nan": (0, NAN), "in_up_nan": (1, NAN), "in_down_nan": (2, NAN), "out_geom_nan": (3, NAN), "out_up_nan": (4, NAN), "out_down_nan": (5, NAN),
    "in_geom_inf": (0, INF), "in_up_inf": (1, INF), "out_down_inf": (5, INF), "in_down_minus_inf": (2, -INF), "out_geom_minus_inf": (3, -INF),
}
REFUSAL = "stutter_model.h:35-39"
JUST_INSIDE = [[1.0 - 2.0 ** -53, 5e-324, 5e-324, 5e-324, 5e-324, 5e-324],
               [5e-324, 0.5, 0.25, 1.0 - 2.0 ** -53, 0.125, 0.125 - 2.0 ** -50]]        # the sum is 1 - 2^-50 exactly


def _violate(model, name):
    """`model` with the violation `name` put in."""
    i, v = OUT_OF_DOMAIN[name]
    m = [float(x) for x in model]
    if i is None:
        return list(v)
    m[i] = v
    return m


def test_the_violations_violate():
    for name in OUT_OF_DOMAIN:
        assert not sm.in_domain(_violate(util.STUTTER, name)), name
    assert all(sm.in_domain(m) for m in JUST_INSIDE)


@pytest.fixture(scope="module")
def three(oracle):
    """Three loci, the requests of two seeded reads per locus."""
    b = sm.synth(["up_heavy", "down_heavy", "flat_geom"], n_loci=3, reads_per_locus=6, n_str_alleles=3, seed=313)
    _, seeds = capi.run_align(oracle, "oracle_", b.ptr)
    ro = b.arrays["read_off"]
    reqs = [[r for r in range(ro[l], ro[l + 1]) if seeds[r] >= 0][:2] for l in range(3)]
    assert all(len(r) == 2 for r in reqs)
    return b, reqs


def _prepare_rc(lib, bptr):
    sec, dig = C.c_double(), C.c_uint64()
    rc = lib.hipstr_debug_prepare(bptr, 1, C.byref(sec), C.byref(dig))
    return rc, lib.hipstr_last_error().decode()


@pytest.mark.parametrize("name", sorted(OUT_OF_DOMAIN))
def test_out_of_domain_model_is_refused_by_the_preparation(hmm_host, three, name):
    b, _ = three
    for l in range(3):              # wherever the locus stands: the check reads its own six values
        models = b.arrays["stutter"].reshape(-1, 6).copy()
        models[l] = _violate(util.STUTTER, name)
        rc, why = _prepare_rc(hmm_host, sm.with_models(b, models).ptr)
        assert rc != 0 and REFUSAL in why, (name, l, rc, why)
    assert _prepare_rc(hmm_host, b.ptr)[0] == 0


@pytest.mark.parametrize("name", sorted(OUT_OF_DOMAIN))
def test_out_of_domain_model_is_refused_by_the_trace_request_check(hmm_host, three, name):
    """The traceback reads the model of the loci its requests name, and of no other: a request behind a refused locus is judged by
    its own locus' model."""
    b, reqs = three
    models = b.arrays["stutter"].reshape(-1, 6).copy()
    models[1] = _violate(util.STUTTER, name)
    x = sm.with_models(b, models)
    for rr in (reqs[1], reqs[2] + reqs[1], reqs[0] + reqs[1][:1] + reqs[2]):
        with pytest.raises(RuntimeError, match=REFUSAL):
            capi.trace_plan(hmm_host, x.ptr, rr, [0] * len(rr))
    for rr in (reqs[0], reqs[2], reqs[2] + reqs[0]):
        assert capi.trace_plan(hmm_host, x.ptr, rr, [1] * len(rr))


def test_a_locus_behind_a_refused_one_is_judged_by_its_own_model(hmm_host, three):
    """Locus 1 out of domain: the batch is refused; the cuts in front of it and behind it are taken, each under its own model (the digest
    of the cut behind equals that of the same locus cut from the sound batch, and moves with that locus' model alone)."""
    b, _ = three
    models = b.arrays["stutter"].reshape(-1, 6).copy()
    models[1] = [0.9, 0.05, 0.05, 1.0, 0.005, 0.005]
    x = sm.with_models(b, models)
    rc, why = _prepare_rc(hmm_host, x.ptr)
    assert rc != 0 and REFUSAL in why
    cut = lambda batch, lo, hi: shard.batch_from_arrays(shard.subset_arrays(batch.arrays, lo, hi))
    for lo, hi in ((0, 1), (2, 3)):
        assert _digest(hmm_host, cut(x, lo, hi).ptr, 1) == _digest(hmm_host, cut(b, lo, hi).ptr, 1)
    assert _prepare_rc(hmm_host, cut(x, 1, 3).ptr)[0] != 0 and _prepare_rc(hmm_host, cut(x, 0, 2).ptr)[0] != 0
    moved = sm.with_models(b, ["up_heavy", "down_heavy", "heavy"])
    assert _digest(hmm_host, cut(moved, 2, 3).ptr, 1) != _digest(hmm_host, cut(b, 2, 3).ptr, 1)
    assert _digest(hmm_host, cut(moved, 0, 2).ptr, 1) == _digest(hmm_host, cut(b, 0, 2).ptr, 1)


def test_models_at_the_edge_of_the_domain_are_taken(hmm_host, three):
    b, reqs = three
    x = sm.with_models(b, JUST_INSIDE + [sm.MODELS["em_clamp"]])
    assert _prepare_rc(hmm_host, x.ptr)[0] == 0
    assert capi.trace_plan(hmm_host, x.ptr, reqs[0] + reqs[1], [0] * 4)
