"""Stutter models other than the one every other case runs under (util.STUTTER: the same for all loci, symmetric in up and down), and the
helpers that lay them over a batch locus by locus.  Shared by tests/cases.py (the stutter_models_* fixtures), tests/test_stutter_models.py
and tests/test_stutter_models_gpu.py.  Array order is the library's: in-frame geom, up, down, then out-of-frame geom, up, down.

Every model satisfies the reference's constructor asserts (stutter_model.h:35-39): geoms inside (0, 1), up / down > 0, their sum < 1."""
import contextlib
import glob
import os

import numpy as np

from util import STUTTER, batch_from_dict, batch_to_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MODELS = {
    "default":    list(STUTTER),
    "up_heavy":   [0.8, 0.10, 0.02, 0.6, 0.01, 0.02],              # the second parameter set of scalars.npz
    "down_heavy": [0.85, 0.01, 0.2, 0.6, 0.002, 0.03],
    "flat_geom":  [0.3, 0.15, 0.25, 0.5, 0.05, 0.05],              # step log(0.7) = -0.36 nats: all 13 terms stay above LOG_THRESH
    "em_clamp":   [0.999, 0.003, 0.04, 0.999, 1e-4, 3e-4],         # the 0.999 cap of em_stutter_genotyper.cpp:117-118: step log(0.001) = LOG_THRESH itself
    "tiny":       [0.95, 1e-9, 1e-6, 0.9, 1e-12, 1e-10],           # artifacts 14 to 27 nats down
    "heavy":      [0.5, 0.3, 0.39, 0.5, 0.15, 0.15],               # no-artifact term log(0.01)
}


def _trained_models():
    """Real outputs of EMStutterGenotyper::train: rows of the committed EM goldens with expect_trained set, asymmetric in frame."""
    out = {}
    for name, row in (("em_no_snps", 1), ("em_deep", 1), ("em_haploid_mix", 3)):
        d = np.load(os.path.join(GOLD, name + ".npz"))
        assert d["expect_trained"][row], (name, row)
        out["%s_%d" % (name, row)] = [float(x) for x in d["expect_stutter"][row]]
    return out


MODELS.update(_trained_models())
NON_DEFAULT = [n for n in MODELS if n != "default"]       # nine names


def in_domain(m):
    """The reference's constructor asserts (stutter_model.h:35-39)."""
    m = np.asarray(m, float)
    return bool(np.all(np.isfinite(m)) and 0 < m[0] < 1 and 0 < m[3] < 1 and min(m[1], m[2], m[4], m[5]) > 0 and m[1] + m[2] + m[4] + m[5] < 1)


def model(m):
    """A model by name or as six numbers."""
    v = MODELS[m] if isinstance(m, str) else [float(x) for x in m]
    assert len(v) == 6
    return v


def with_models(batch, models):
    """A new capi.Batch equal to `batch` except that locus l carries models[l % len(models)] (names of MODELS or six numbers each)."""
    d = batch_to_dict(batch)
    n = len(d["period"])
    d["stutter"] = np.array([model(models[l % len(models)]) for l in range(n)], np.float64).reshape(-1)
    return batch_from_dict(d)


def swap_up_down(m):
    """The model with up and down exchanged, in frame and out of frame."""
    g, u, d, og, ou, od = model(m)
    return [g, d, u, og, od, ou]


def rotate(models, k):
    """The model list rotated by k: locus l gets what locus l + k had."""
    models = list(models)
    k %= len(models)
    return models[k:] + models[:k]


@contextlib.contextmanager
def synth_env(**kw):
    """The generator's environment switches (HIPSTR_SYNTH_<NAME>) set for the block — None: unset, the generator's default — and put
    back afterwards."""
    keys = {"HIPSTR_SYNTH_" + k.upper(): (None if v is None else str(v)) for k, v in kw.items()}
    old = {k: os.environ.get(k) for k in keys}
    for k, v in keys.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def synth(models, imperfect=None, inherit=None, period=None, **kw):
    """with_models(synth_to_batch(SynthBatch(**kw)), models) under the given generator switches (None: the generator's default)."""
    from hipstr_amd import capi
    from util import synth_to_batch
    with synth_env(imperfect=imperfect, inherit=inherit, period=period):
        b = synth_to_batch(capi.SynthBatch(**kw))
    return with_models(b, models)


def locus_rows(batch, values, l):
    """The entries of locus l in an aln_probs array of the batch."""
    a = batch.arrays
    P = np.diff(a["read_off"]).astype(np.int64); A = np.diff(a["hap_off"]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(P * A)])
    return values[off[l]:off[l + 1]]
