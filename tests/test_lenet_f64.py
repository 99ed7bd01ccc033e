"""CPU checks of tests/lenet_f64.py: the three-term split, the forward-error bound (met by every fp32
restatement, violated by every lossy mutant of the bf16 path), the integer and power-of-two probes, and
the ip1 split-K rules the GPU tests have to reach."""
import os
import re

import numpy as np
import pytest

import lenet_f64 as L
import np_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (-8, -4, 4, 8)


def _oracle(w, imgs):
    from oracle import api
    o = api.Oracle(num_threads=8)
    o.lenet_load(w)
    return o.lenet_forward(imgs)


def _implementations(w, imgs):
    return {"oracle": _oracle(w, imgs), "torch": ref.lenet_torch(w, imgs), "x3_emulate": L.x3_emulate(w, imgs)}


def _ratio(got, want, b):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.all((err == 0) | (b > 0))          # a logit with bound 0 must be exact
    return float((err / np.where(b > 0, b, 1.0)).max())


def _sweep_values():
    """fp32 bit patterns: every biased exponent 0 .. 254 with mantissas 0, all ones, one low bit and
    random ones; both signs; the largest finite value."""
    rng = np.random.default_rng(0)
    mants = np.concatenate([[0, 0x7FFFFF, 1, 0x400001, 0x00FFFF, 0x7F0000], rng.integers(0, 1 << 23, 26)])
    exps = np.arange(0, 255, dtype=np.uint64)
    bits = (exps[:, None] << np.uint64(23)) | mants.astype(np.uint64)[None, :]
    bits = np.concatenate([bits.ravel(), [0x7F7FFFFF]]).astype(np.uint32)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    return bits.view(np.float32)


def test_split3_sweep_of_bit_patterns():
    """h + m + l == v exactly for every fp32 value that is a multiple of 2^-133 -- every value of
    biased exponent >= 17, +-0, powers of two, all-ones mantissas, the largest finite value.  Below
    that the split loses the bits under 2^-133, the lowest bit a bf16 holds: the sum is v truncated
    towards zero to a multiple of 2^-133 (a subnormal v keeps only h).  Every term is a bf16 (low 16
    bits zero) of v's sign."""
    v = _sweep_values()
    h, m, l = L.split3(v)
    for t in (h, m, l):
        assert not (t.view(np.uint32) & 0xFFFF).any()
        assert np.all((t == 0) | (np.signbit(t) == np.signbit(v)))
    s = h.astype(np.float64) + m + l                      # exact: 24 bits of one value
    v64 = v.astype(np.float64)
    q = 2.0 ** -133
    assert np.array_equal(s, np.trunc(v64 / q) * q)
    big = (v.view(np.uint32) & 0x7F800000) >= (17 << 23)
    assert np.array_equal(s[big], v64[big])
    assert big.sum() > 0.9 * len(v)
    assert np.array_equal(s[v == 0], v64[v == 0])
    sub = ((v.view(np.uint32) & 0x7F800000) == 0) & (v != 0)
    assert np.all(m[sub] == 0) and np.all(l[sub] == 0)
    # the l term is never dropped silently above 2^-133: m and l are nonzero for full mantissas
    full = L.full_mantissa(np.random.default_rng(1), (1000,))
    fh, fm, fl = L.split3(full)
    assert np.all(fm != 0) and np.all(fl != 0)


def test_three_term_split_with_round_to_nearest_is_exact_too():
    """Why rounding only matters for the lossy mutants: three round-to-nearest terms also carry all
    24 bits (the remainder of each rounding is at most half an ulp, with the sign as a spare bit)."""
    v = _sweep_values()
    v = v[(v.view(np.uint32) & 0x7F800000) >= (17 << 23)]
    v = v[np.abs(v) < 2.0 ** 127]                          # (rounding up the largest values overflows)
    h, m, l = L.split3(v, rne=True)
    assert np.array_equal(h.astype(np.float64) + m + l, v.astype(np.float64))


@pytest.mark.parametrize("layer", ["conv1", "conv2", "ip1", "ip2"])
def test_fp32_restatements_meet_the_bound_on_layer_probes(layer):
    ratios = {}
    for tag, w, imgs in L.layer_probes(layer):
        want = L.forward_f64(w, imgs)
        b = L.bound(w, imgs)
        assert (want != 0).mean() > 0.25, tag          # the probes do reach the logits
        for name, got in _implementations(w, imgs).items():
            ratios[name] = max(ratios.get(name, 0.0), _ratio(got, want, b))
    print(layer, ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_fp32_restatements_meet_the_bound_on_xavier_networks():
    for tag, w, imgs in L.realistic_inputs():
        want = L.forward_f64(w, imgs)
        b = L.bound(w, imgs)
        ratios = {name: _ratio(got, want, b) for name, got in _implementations(w, imgs).items()}
        print(tag, ratios)
        assert max(ratios.values()) <= 1.0, (tag, ratios)
        assert min(ratios.values()) > 0                 # (the check is not vacuous)


def test_every_mutant_violates_the_bound_on_a_layer_probe():
    """Each lossy variant of the bf16 path exceeds the bound by 10x or more on at least one
    layer-isolating probe; the one actually built stays inside it."""
    worst = {v: 0.0 for v in L.MUTANTS}
    for tag, w, imgs in L.all_layer_probes():
        want = L.forward_f64(w, imgs)
        b = L.bound(w, imgs)
        assert _ratio(L.x3_emulate(w, imgs), want, b) <= 1.0, tag
        for v in L.MUTANTS:
            worst[v] = max(worst[v], _ratio(L.x3_emulate(w, imgs, v), want, b))
    print(worst)
    for v, r in worst.items():
        assert r >= 10.0, (v, r)


@pytest.mark.parametrize("deep", [False, True])
def test_integer_probes_are_bit_exact(deep):
    w, imgs = L.integer_probe(deep=deep)
    want = L.forward_f64(w, imgs)
    assert (want != 0).all()
    for name, got in _implementations(w, imgs).items():
        assert np.array_equal(got.astype(np.float64), want), name
    if deep:   # every dropped or mis-split term changes a logit
        for v in L.MUTANTS:
            assert not np.array_equal(L.x3_emulate(w, imgs, v).astype(np.float64), want), v
    # a swapped pair of conv1 taps is an O(1) error
    ws = dict(w, conv1_w=w["conv1_w"].copy())
    ws["conv1_w"][:, :, 0, [0, 1]] = ws["conv1_w"][:, :, 0, [1, 0]]
    assert np.abs(L.forward_f64(ws, imgs) - want).max() >= 0.25


def test_power_of_two_scaling_is_exact():
    """s = +-4, +-8 keep every bf16-term product of the Xavier inputs normal, and the logits of every
    restatement scale by exactly 2^(4 s)."""
    for tag, w, imgs in L.realistic_inputs():
        base = _implementations(w, imgs)
        for s in SCALES:
            ws = L.scaled(w, s)
            assert L.smallest_term_product(ws, imgs) >= 2.0 ** -126, (tag, s)
            for name, got in _implementations(ws, imgs).items():
                assert np.array_equal(got, np.ldexp(base[name], 4 * s)), (tag, s, name)


def test_split_rule_restates_the_kernels():
    """fc1_x3_ksplit above is the rule of ag2_device.h, and the ip1 launch applies it to 128-image tiles."""
    dev = open(os.path.join(ROOT, "agile_grasp2_amd", "csrc", "ag2_device.h")).read()
    assert "const int splits[7] = {1, 3, 5, 9, 15, 25, 45};" in dev
    assert re.search(r"mtiles \* 4 \* splits\[i\] >= 448\) return splits\[i\];\s+return kFc1X3MaxSplit;", dev)
    assert "constexpr int kFc1X3MaxSplit = 45;" in dev
    src = open(os.path.join(ROOT, "agile_grasp2_amd", "csrc", "k_lenet.hip")).read()
    assert "constexpr int kFxBM = 128;" in src and "mtiles = (int)((n + kFxBM - 1) / kFxBM)" in src
    assert "ksplit = d_n ? kFc1X3MaxSplit : fc1_x3_ksplit(mtiles);" in src


def test_split_batches_reach_every_split_on_both_sides_of_every_change():
    rule = L.split_x3
    changes = [n for n in range(2, 20000) if rule(n) != rule(n - 1)]
    assert rule(changes[-1]) == 1 and all(rule(n) == 1 for n in range(changes[-1], 20000, 97))
    for n in changes:
        assert n - 1 in L.SPLIT_BATCHES and n in L.SPLIT_BATCHES, n
        assert (n - 1) % 128 == 0
    assert {rule(n) for n in L.SPLIT_BATCHES} == {rule(n) for n in range(1, 20000)}
    assert changes == [513, 897, 1537, 2817, 4737, 14209]
