"""GPU: the LeNet kernels against the float64 reference of tests/lenet_f64.py, within its forward-error
bound -- layer-isolating probes, integer probes (bit for bit), power-of-two scaling (bit for bit), the
batch sizes at every ip1 split-K change, Xavier networks on realistic images and one detect.

PATHS names the one LeNet path (bf16 three-term split, banded convolutions).  Each test prints
max(|err| / bound) per path and input class ("RATIO ..." lines, pytest -s)."""
import numpy as np
import pytest

import lenet_f64 as L
from conftest import scene_params
from agile_grasp2_amd.weights import make_lenet_weights

pytestmark = pytest.mark.gpu

PATHS = ("bands",)
SCALES = (-8, -4, 4, 8)


def detector(w, **kw):
    from agile_grasp2_amd import capi
    d = capi.Detector(**kw)
    d.lenet_load(w)
    return d


def logits(w, imgs):
    d = detector(w)
    try:
        return d.lenet_forward(imgs).astype(np.float64)
    finally:
        d.close()


def ratio(got, want, b):
    err = np.abs(got - want)
    assert np.all((err == 0) | (b > 0)), "a logit the bound calls exact is not"
    return float((err / np.where(b > 0, b, 1.0)).max())


def report(cls, ratios):
    for path, r in ratios.items():
        print(f"RATIO {cls} {path} {r:.3g}")
    return ratios


@pytest.mark.parametrize("layer", ["conv1", "conv2", "ip1", "ip2"])
def test_layer_probes_within_bound(layer):
    ratios = dict.fromkeys(PATHS, 0.0)
    for tag, w, imgs in L.layer_probes(layer):
        want = L.forward_f64(w, imgs)
        b = L.bound(w, imgs)
        for path in PATHS:
            ratios[path] = max(ratios[path], ratio(logits(w, imgs), want, b))
    report(f"probe-{layer}", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("deep", [False, True])
def test_integer_probes_bit_exact(deep):
    w, imgs = L.integer_probe(deep=deep)
    want = L.forward_f64(w, imgs)
    for path in PATHS:
        got = logits(w, imgs)
        assert np.array_equal(got, want), (path, np.abs(got - want).max())


def test_power_of_two_scaling_bit_exact():
    for tag, w, imgs in L.realistic_inputs():
        for path in PATHS:
            base = logits(w, imgs)
            for s in SCALES:
                got = logits(L.scaled(w, s), imgs)
                assert np.array_equal(got, np.ldexp(base, 4 * s)), (tag, path, s)


@pytest.mark.parametrize("path", PATHS)
def test_split_k_batches_bit_exact(path):
    """Both integer probes, their images dealt across batches on each side of every split change:
    every split must add up to the float64 logits bit for bit."""
    probes = [L.integer_probe(seed=3, n_img=64), L.integer_probe(seed=4, n_img=64, deep=True)]
    wants = [L.forward_f64(w, imgs) for w, imgs in probes]
    for (w, imgs), want in zip(probes, wants):
        d = detector(w)
        try:
            for n in L.SPLIT_BATCHES:
                idx = (np.arange(n) * 37 + n) % len(imgs)
                got = d.lenet_forward(imgs[idx]).astype(np.float64)
                assert np.array_equal(got, want[idx]), (path, n, L.split_x3(n))
        finally:
            d.close()


def test_realistic_inputs_within_bound(small_scene):
    from agile_grasp2_amd import capi
    xyz, ws, idx = small_scene
    d = capi.Detector(**scene_params(ws))
    d.set_cloud(xyz)
    d.compute_normals()
    n = len(d.generate_hypotheses(sample_idx=idx, seed=5))
    scene_imgs = d.render_images(0, n)
    d.close()
    assert n > 50
    cases = []
    for tag, w, imgs in L.realistic_inputs():
        cases += [(f"{tag}-zero", w, imgs[:1]), (f"{tag}-255", w, imgs[1:2]),
                  (f"{tag}-dense", w, imgs[2:8]), (f"{tag}-sparse", w, imgs[8:]),
                  (f"{tag}-scene", w, scene_imgs)]
    for cls, w, imgs in cases:
        want = L.forward_f64(w, imgs)
        b = L.bound(w, imgs)
        r = report(cls, {path: ratio(logits(w, imgs), want, b) for path in PATHS})
        assert max(r.values()) <= 1.0, (cls, r)


def test_detect_scores_within_bound(small_scene):
    """The scores of one detect (logit 1 - logit 0 of every hypothesis) against forward_f64 of the
    oracle's images of the same records."""
    from agile_grasp2_amd import capi
    from oracle import api
    xyz, ws, idx = small_scene
    prm = scene_params(ws, min_score_diff=-1e30, num_selected=1000)
    w = make_lenet_weights(7)
    d = capi.Detector(**prm)
    o = api.Oracle(**dict(prm, num_threads=8))
    for x in (d, o):
        x.set_cloud(xyz)
        x.compute_normals()
        x.lenet_load(w)
    _, ga = d.detect(sample_idx=idx, seed=5, do_prune=False)
    d.close()
    hyps = o.generate_hypotheses(sample_idx=idx, seed=5)
    imgs = o.render_images(0, len(hyps))
    assert len(ga) == len(hyps) > 20
    assert np.array_equal(ga["sample_slot"], hyps["sample_slot"])
    assert np.array_equal(ga["orientation"], hyps["orientation"])
    want = L.forward_f64(w, imgs)
    b = L.bound(w, imgs)
    s = want[:, 1] - want[:, 0]
    bs = b[:, 0] + b[:, 1] + 2 * L.U * (np.abs(s) + b[:, 0] + b[:, 1])   # + the fp32 subtraction
    r = report("detect-scores", {"bands": ratio(ga["score"].astype(np.float64), s, bs)})
    assert r["bands"] <= 1.0, r
