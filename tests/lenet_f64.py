"""Float64 reference, forward-error bound and bf16-split emulation of the LeNet scorer (tests only).

forward_f64 runs the network of caffe/test_1batch2.prototxt (conv1 20@5x5 -> max 2/2 -> conv2 50@5x5
-> max 2/2 -> ip1 500 -> ReLU -> ip2 2) in float64 on HWC u8 images, like np_reference.lenet_torch.
bound gives, per logit, how far any of the fp32 implementations may lie from it.

Derivation of bound
-------------------
Every layer computes y = sum_k w_k x_k + b from inputs x^ = x + d with |d| <= e_in.  Its computed
output y^ differs from the exact y by
  (a) the input error                   |sum_k w_k d_k| <= |W| e_in,
  (b) the products the three-term split drops (conv2 and ip1 of the bf16 path only, below),
  (c) rounding: every fp32 operation on a nonzero operand adds at most 2u |its result|, u = 2^-24.
      The factor 2 covers truncating adders: the rounding of the MFMA's 16-k step is not documented
      and has not been measured.  Summing S nonzero summands, in any order or tree (split-K partial
      sums and the shuffle tree of ip2 included), is S - 1 operations; with the bias one more; with
      an inexact product one more per product.  So with R operations, the standard argument gives
      |error| <= gamma(R) (|W| |x^| + |b|), gamma(R) = 2uR / (1 - 2uR).
  Hence   e_out <= |W| e_in + gamma(R) (|W| (|x| + e_in) + |b|) + D(W) (|x| + e_in).
R is counted per output from the nonzero pattern: summand k counts as nonzero when |x_k| + e_k > 0
and w_k != 0.  Each nonzero product contributes the largest count of any implementation:
  * conv1, bf16 path: the u8 pixel is one exact bf16 term and products are exact: one summand per
    nonzero split term of w.  The oracle and torch: one summand and, unless w is a power of two, one
    product rounding.
  * conv2 and ip1, bf16 path: x^ and w are split into (h, m, l); the six products hl, lh, mm, hm, mh, hh
    are kept.  Per product the summands are 3 [w_h != 0] + 2 [w_m != 0] + [w_l != 0] (x^'s own terms
    are unknown, so all three are assumed present).  This is at least the fp32 count of 2.
  * ip2 (fmaf chain + shuffle tree on every path): one summand, plus one product rounding unless
    w is a power of two.
An output with exactly one nonzero summand whose weight is a power of two is exact on every path: the
product is exact, and on the bf16 path its three summands are x^'s split terms times w, whose partial
sums are truncations of x^ w.  Its R is 0 (plus one if its bias is nonzero).  Max-pooling and ReLU are
1-Lipschitz: e passes through them (pooled: the max of e over the window); the bf16 path adds the bias
after pooling, which gives the same rounded value since rounding is monotonic.
(b): truncation keeps 8 significant bits per term, so |x_m| < 2^-7 |x| and |x_l| < 2^-15 |x|.  The
dropped products ml, lm, ll are therefore below
  D(w) |x|,  D(w) = 2^-7 |w_l| + 2^-15 |w_m| + 2^-15 |w_l|   (< 2^-21 |w|; 0 when w is one bf16 term).
Range: split3 is exact for every fp32 value whose lowest set bit is at or above 2^-133 (the lowest bit
a bf16 can hold); below that, l loses bits, and a subnormal value keeps only h.  The bound does not
model that range: bound() refuses weights whose split is not exact, and the activations of these
tests stay far above it (tests/test_lenet_f64.py documents the subnormal behaviour).

x3_emulate restates the bf16 path in torch fp32 (split, kept products, fp32 sums in another order)
with mutant variants; it only serves to show on the CPU that the bound tells right from wrong.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from agile_grasp2_amd.weights import SHAPES, make_lenet_weights

U = 2.0 ** -24
CHUNK = 64                        # images per float64 block (memory)
PAIRS6 = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))   # (x term, w term): hl, lh, mm, hm, mh, hh
MUTANTS = ("split2", "split2_rne", "split1", "split1_rne", "no_hl_lh")


# ---- the three-term split ------------------------------------------------------------------------

def _round16(v: np.ndarray, rne: bool) -> np.ndarray:
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    if rne:
        b = b + 0x7FFF + ((b >> 16) & 1)
    return (b & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split3(v, terms: int = 3, rne: bool = False) -> list[np.ndarray]:
    """split3 of k_lenet.hip: each term is the running remainder cut to its top 16 bits (a bf16);
    terms < 3 or rne=True give the mutant splits."""
    r = np.asarray(v, dtype=np.float32)
    out = []
    for _ in range(terms):
        t = _round16(r, rne)
        out.append(t)
        r = (r - t).astype(np.float32)        # exact
    return out


def _weight_terms(w: np.ndarray):
    h, m, l = split3(w)
    if not np.array_equal(h.astype(np.float64) + m + l, w.astype(np.float64)):
        raise ValueError("bound: a weight is outside the range where split3 is exact")
    nz = (h != 0).astype(np.float64) + (m != 0) + (l != 0)
    kept = 3.0 * (h != 0) + 2.0 * (m != 0) + (l != 0)
    mant = np.frexp(w.astype(np.float64))[0]
    np2 = ((w != 0) & (np.abs(mant) != 0.5)).astype(np.float64)
    drop = 2.0 ** -7 * np.abs(l) + 2.0 ** -15 * np.abs(m) + 2.0 ** -15 * np.abs(l)
    return nz, kept, np2, drop.astype(np.float64)


# ---- float64 forward -----------------------------------------------------------------------------

def _planar(imgs: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(imgs).astype(np.float64)).permute(0, 3, 1, 2).contiguous()


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _apply(layer: str, x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    if layer in ("conv1", "conv2"):
        return F.conv2d(x, w, b)
    return F.linear(x.flatten(1), w, b)


def forward_f64(w: dict, imgs: np.ndarray, intermediates: bool = False):
    """Logits (n, 2) in float64; with intermediates=True also a dict of every layer's output before
    pooling / ReLU ("conv1", "conv2", "ip1") and after ("pool1", "pool2", "relu1")."""
    tw = {k: _t(v) for k, v in w.items()}
    outs, acts = [], {}
    with torch.no_grad():
        for i in range(0, len(imgs), CHUNK):
            a = {}
            a["conv1"] = F.conv2d(_planar(imgs[i:i + CHUNK]), tw["conv1_w"], tw["conv1_b"])
            a["pool1"] = F.max_pool2d(a["conv1"], 2)
            a["conv2"] = F.conv2d(a["pool1"], tw["conv2_w"], tw["conv2_b"])
            a["pool2"] = F.max_pool2d(a["conv2"], 2)
            a["ip1"] = F.linear(a["pool2"].flatten(1), tw["ip1_w"], tw["ip1_b"])
            a["relu1"] = F.relu(a["ip1"])
            outs.append(F.linear(a["relu1"], tw["ip2_w"], tw["ip2_b"]).numpy())
            if intermediates:
                for k, v in a.items():
                    acts.setdefault(k, []).append(v.numpy())
    logits = np.concatenate(outs) if outs else np.zeros((0, 2))
    if intermediates:
        return logits, {k: np.concatenate(v) for k, v in acts.items()}
    return logits


def forward_abs(w: dict, imgs: np.ndarray) -> dict:
    """The magnitude M = |W| |x| + |b| of every output of every layer ("conv1", "conv2", "ip1",
    "ip2"), x the exact activations of forward_f64."""
    _, a = forward_f64(w, imgs, intermediates=True)
    ins = {"conv1": _planar(imgs), "conv2": _t(a["pool1"]), "ip1": _t(a["pool2"]), "ip2": _t(a["relu1"])}
    with torch.no_grad():
        return {ly: _apply(ly, ins[ly].abs(), _t(np.abs(w[ly + "_w"])), _t(np.abs(w[ly + "_b"]))).numpy()
                for ly in ins}


def _layer_bound(layer, w, b, x, e):
    """(e_out, |x_out| + e_out) of one layer before pooling: x, e its exact input and input bound."""
    nz, kept, np2, drop = _weight_terms(w)
    nonzero = (w != 0).astype(np.float64)
    if layer == "conv1":
        cnt = np.maximum(nz, 1 + np2)
    elif layer in ("conv2", "ip1"):
        cnt = kept
    else:
        cnt = nonzero + np2
    xa = x.abs() + e
    ind = (xa > 0).to(torch.float64)
    with torch.no_grad():
        prop = _apply(layer, e, _t(np.abs(w)))
        mag = _apply(layer, xa, _t(np.abs(w)))
        s = _apply(layer, ind, _t(cnt))
        n_all = _apply(layer, ind, _t(nonzero))
        n_np2 = _apply(layer, ind, _t(nonzero * np2))
        bias_nz = _t((b != 0).astype(np.float64))
        shape = (1, -1, 1, 1) if layer in ("conv1", "conv2") else (1, -1)
        exact = (n_all == 1) & (n_np2 == 0)
        r = torch.where(exact, torch.zeros_like(s), torch.clamp(s - 1, min=0)) + bias_nz.view(shape)
        gamma = 2 * U * r / (1 - 2 * U * r)
        e_out = prop + gamma * (mag + _t(np.abs(b)).view(shape))
        if layer in ("conv2", "ip1"):
            e_out = e_out + _apply(layer, xa, _t(drop))
    return e_out


def bound(w: dict, imgs: np.ndarray) -> np.ndarray:
    """Per-logit forward-error bound (n, 2) of every fp32 implementation of the network (see the
    module docstring)."""
    w = {k: np.asarray(v, dtype=np.float32) for k, v in w.items()}
    tw = {k: _t(v) for k, v in w.items()}
    out = []
    with torch.no_grad():
        for i in range(0, len(imgs), CHUNK):
            x = _planar(imgs[i:i + CHUNK])
            e = torch.zeros_like(x)
            for ly in ("conv1", "conv2", "ip1", "ip2"):
                e_new = _layer_bound(ly, w[ly + "_w"], w[ly + "_b"], x, e)
                x = _apply(ly, x, tw[ly + "_w"], tw[ly + "_b"])
                e = e_new
                if ly in ("conv1", "conv2"):
                    x, e = F.max_pool2d(x, 2), F.max_pool2d(e, 2)
                elif ly == "ip1":
                    x = F.relu(x)
            out.append(e.numpy())
    return np.concatenate(out) if out else np.zeros((0, 2))


# ---- emulation of the bf16 path and its mutants -------------------------------------------------

def _terms_of(v: np.ndarray, variant: str) -> list[np.ndarray]:
    n = {"split2": 2, "split2_rne": 2, "split1": 1, "split1_rne": 1}.get(variant, 3)
    return split3(v, n, rne=variant.endswith("_rne"))


def x3_emulate(w: dict, imgs: np.ndarray, variant: str = "x3") -> np.ndarray:
    """Logits of the bf16 path restated in torch fp32: conv1 as the exact products of the u8 pixels
    with the weight terms, conv2 and ip1 as the six kept products of the split activations and
    weights, bias after pooling, ip2 in fp32.  variant: "x3" (as built) or one of MUTANTS."""
    pairs = tuple(p for p in PAIRS6 if variant != "no_hl_lh" or p not in ((0, 2), (2, 0)))
    f32 = {k: np.asarray(v, dtype=np.float32) for k, v in w.items()}

    def layer(ly, x: np.ndarray, pool: bool):
        wt = [torch.from_numpy(t) for t in _terms_of(f32[ly + "_w"], variant)]
        if ly == "conv1":
            xt, use = [torch.from_numpy(x)], [(0, k) for k in range(len(wt))]
        else:
            xt = [torch.from_numpy(t) for t in _terms_of(x, variant)]
            use = [(a, k) for a, k in pairs if a < len(xt) and k < len(wt)]
        acc = None
        for a, k in use:
            y = _apply(ly, xt[a], wt[k])
            acc = y if acc is None else acc + y
        if pool:
            acc = F.max_pool2d(acc, 2)
        shape = (1, -1, 1, 1) if pool else (1, -1)
        return (acc + torch.from_numpy(f32[ly + "_b"]).view(shape)).numpy()

    out = []
    with torch.no_grad():
        for i in range(0, len(imgs), CHUNK):
            x = np.ascontiguousarray(imgs[i:i + CHUNK].astype(np.float32).transpose(0, 3, 1, 2))
            x = layer("conv1", x, True)
            x = layer("conv2", x, True)
            x = np.maximum(layer("ip1", x, False), np.float32(0))
            y = F.linear(torch.from_numpy(x), torch.from_numpy(f32["ip2_w"]), torch.from_numpy(f32["ip2_b"]))
            out.append(y.numpy())
    return np.concatenate(out) if out else np.zeros((0, 2), np.float32)


# ---- probe networks ------------------------------------------------------------------------------

def full_mantissa(rng, shape, exp: int = 0) -> np.ndarray:
    """Positive fp32 values 2^exp (1 + a 2^-7 + b 2^-15 + c 2^-23), b, c in [128, 256): all 24
    significand bits in use and every split term nonzero, m near 2^-8 and l near 2^-16 of the value."""
    a = rng.integers(0, 128, size=shape)
    b = rng.integers(128, 256, size=shape)
    c = rng.integers(128, 256, size=shape)
    v = (1 + a * 2.0 ** -7 + b * 2.0 ** -15 + c * 2.0 ** -23) * 2.0 ** exp
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def zero_weights() -> dict:
    return {k: np.zeros(s, dtype=np.float32) for k, s in SHAPES.items()}


def _ip1_pick(w, n, ch):
    """ip1 output n reads channel ch of pool2 at the positions (3i, 3j): a lit 2x2 block of pool2
    cells meets at most one of them."""
    for yy in range(0, 12, 3):
        for xx in range(0, 12, 3):
            w["ip1_w"][n, ch * 144 + yy * 12 + xx] = 1.0


def _pixel_images(n, salt, rows=60):
    """One lit pixel per image: every row, columns and channels moved across the batch, pixel
    values with few and with many set bits."""
    vals = (255, 1, 171, 96, 37, 254, 129, 7)
    imgs = np.zeros((n, 60, 60, 3), dtype=np.uint8)
    for i in range(n):
        y = (i * 7 + salt) % rows
        x = (i * 17 + 3 * salt) % 60
        imgs[i, y, x, (i + salt) % 3] = vals[(i + salt) % len(vals)]
    return imgs


def layer_probes(layer: str, n_img: int = 40, seed: int = 0) -> list[tuple[str, dict, np.ndarray]]:
    """Networks whose logits each depend on one or a few products of ONE layer (full-mantissa
    weights there), routed by weights 1.0 (split (1, 0, 0), exact) through the others, on images
    with one lit pixel.  Everything reaching the ReLU is positive.  Returns (tag, weights, images)."""
    rng = np.random.default_rng(seed)
    probes = []
    if layer == "conv1":
        # conv1 dense; conv2 channel o reads conv1 channel o % 20 at tap (0, 0); ip1 output o picks
        # conv2 channel o; the logits are ip1 outputs a, b (+ 20: a second path through channel a)
        for k in range(5):
            w = zero_weights()
            w["conv1_w"] = full_mantissa(rng, SHAPES["conv1_w"], -1)
            for o in range(50):
                w["conv2_w"][o, o % 20, 0, 0] = 1.0
                _ip1_pick(w, o, o)
            for j, a in enumerate((4 * k, 4 * k + 1)):
                w["ip2_w"][j, a] = 1.0
                w["ip2_w"][j, a + 22] = 1.0          # conv1 channel a + 2 (a + 22 = (a + 2) mod 20 + 20)
            probes.append((f"conv1/{k}", w, _pixel_images(n_img, 5 * k)))
    elif layer == "conv2":
        # conv1 routes input channel c to conv1 channel 3 v + c through a full-mantissa weight (full-
        # mantissa activations); conv2 dense; ip1 output o picks conv2 channel o
        for v in range(7):
            w = zero_weights()
            g = full_mantissa(rng, (3,), -2)
            for c in range(3):
                if 3 * v + c < 20:
                    w["conv1_w"][3 * v + c, c, 0, 0] = g[c]
            w["conv2_w"] = full_mantissa(rng, SHAPES["conv2_w"], -3)
            for o in range(50):
                _ip1_pick(w, o, o)
            w["ip2_w"][0, (7 * v) % 50] = 1.0
            w["ip2_w"][1, (7 * v + 25) % 50] = 1.0
            probes.append((f"conv2/{v}", w, _pixel_images(n_img, 3 * v)))
    elif layer == "ip1":
        # one lit pixel -> exactly one pool2 feature (channel 3 v + c, cell (y / 4, x / 4)); ip1 dense
        for v in (0, 5, 11, 15):
            w = zero_weights()
            for c in range(3):
                w["conv1_w"][c, c, 0, 0] = 1.0
                w["conv2_w"][3 * v + c, c, 0, 0] = 1.0
            w["ip1_w"] = full_mantissa(rng, SHAPES["ip1_w"], -8)
            w["ip2_w"][0, [v, 100 + v, 200 + v]] = 1.0
            w["ip2_w"][1, 499 - v] = 1.0
            probes.append((f"ip1/{v}", w, _pixel_images(n_img, v, rows=48)))
    elif layer == "ip2":
        w = zero_weights()
        for c in range(3):
            w["conv1_w"][c, c, 0, 0] = 1.0
            w["conv2_w"][c, c, 0, 0] = 1.0
        for n in range(500):                    # ip1 output n copies one pool2 feature of channel n % 3
            w["ip1_w"][n, (n % 3) * 144 + (n * 7) % 144] = 1.0
        w["ip2_w"] = full_mantissa(rng, SHAPES["ip2_w"], -1)
        probes.append(("ip2", w, _pixel_images(n_img, 1, rows=48)))
    else:
        raise ValueError(layer)
    return probes


def all_layer_probes(n_img: int = 40):
    return [p for ly in ("conv1", "conv2", "ip1", "ip2") for p in layer_probes(ly, n_img)]


def integer_probe(seed: int = 0, n_img: int = 48, deep: bool = False):
    """Small integer weights times a power of two per layer, biases in the same units, images of a
    few lit pixels: every partial sum, in any order, is an integer number of its layer's unit below
    2^24, so every implementation must return the float64 logits bit for bit.  Every conv1 tap has
    its own weight, so a swapped tap is an O(1) error.  deep=True: conv2 biases of 2^18 .. 2^19 units
    with low bits set make the ip1 inputs 19-20-bit integers, so all three of their split terms are
    nonzero and a dropped or mis-split term changes the logits; ip1 and ip2 are then sparse enough to
    stay below 2^24 units."""
    rng = np.random.default_rng(seed)

    def ints(shape, density, hi):
        v = rng.integers(1, hi + 1, size=shape) * rng.choice([-1, 1], size=shape)
        return (v * (rng.uniform(size=shape) < density)).astype(np.float64)

    w = {}
    w["conv1_w"] = (np.arange(1500).reshape(20, 3, 5, 5) % 29 - 14) * 2.0 ** -2   # distinct per tap
    w["conv1_b"] = rng.integers(-64, 64, size=20) * 2.0 ** -2
    w["conv2_w"] = ints(SHAPES["conv2_w"], 0.06, 3) * 2.0 ** -1
    if deep:
        w["conv2_b"] = (rng.integers(2 ** 18, 2 ** 19, size=50) | 0x155) * 2.0 ** -3
        w["ip1_w"] = ints(SHAPES["ip1_w"], 0.0015, 1) * 2.0
        w["ip1_b"] = rng.integers(-2 ** 20, 2 ** 20, size=500) * 2.0 ** -2
        w["ip2_w"] = np.zeros(SHAPES["ip2_w"])
        for j in range(2):
            w["ip2_w"][j, rng.choice(500, 3, replace=False)] = rng.choice([-1, 1], 3)
    else:
        w["conv2_b"] = rng.integers(-512, 512, size=50) * 2.0 ** -3
        w["ip1_w"] = ints(SHAPES["ip1_w"], 0.004, 2) * 2.0
        w["ip1_b"] = rng.integers(-2048, 2048, size=500) * 2.0 ** -2
        w["ip2_w"] = ints(SHAPES["ip2_w"], 0.5, 3)
    w["ip2_b"] = rng.integers(-4096, 4096, size=2) * 2.0 ** -2
    w = {k: v.astype(np.float32) for k, v in w.items()}
    imgs = np.zeros((n_img, 60, 60, 3), dtype=np.uint8)
    for i in range(n_img):
        k = 1 + i % 12
        ys, xs, cs = rng.integers(0, 60, k), rng.integers(0, 60, k), rng.integers(0, 3, k)
        imgs[i, ys, xs, cs] = rng.integers(1, 64, k)
    units = {"conv1": 2.0 ** -2, "conv2": 2.0 ** -3, "ip1": 2.0 ** -2, "ip2": 2.0 ** -2}
    m = forward_abs(w, imgs)
    for ly, unit in units.items():
        assert m[ly].max() / unit < 2 ** 24, (ly, m[ly].max() / unit)
    return w, imgs


def scaled(w: dict, s: int) -> dict:
    """Every weight times 2^s, the biases of layer l (1-based) times 2^(l s): the logits scale by
    exactly 2^(4 s) as long as every split term and product stays normal."""
    out = {}
    for i, ly in enumerate(("conv1", "conv2", "ip1", "ip2")):
        out[ly + "_w"] = np.ldexp(np.asarray(w[ly + "_w"], np.float32), s).astype(np.float32)
        out[ly + "_b"] = np.ldexp(np.asarray(w[ly + "_b"], np.float32), (i + 1) * s).astype(np.float32)
    return out


def smallest_term_product(w: dict, imgs: np.ndarray) -> float:
    """A lower bound on every nonzero bf16-term product of the bf16 path on these inputs (min |x term|
    x min |w term| per layer); scaling is exact when it stays >= 2^-126."""
    _, a = forward_f64(w, imgs, intermediates=True)
    ins = {"conv1": None, "conv2": a["pool1"], "ip1": a["pool2"], "ip2": a["relu1"]}
    lo = np.inf
    for ly, x in ins.items():
        wt = np.abs(np.concatenate([t.ravel() for t in split3(w[ly + "_w"])]).astype(np.float64))
        wmin = wt[wt > 0].min() if (wt > 0).any() else np.inf
        if x is None:
            xmin = 1.0
        else:
            xt = np.abs(np.concatenate([t.ravel() for t in split3(x.astype(np.float32))]).astype(np.float64))
            xmin = xt[xt > 0].min() if (xt > 0).any() else np.inf
        lo = min(lo, wmin * xmin)
    return lo


def random_images(rng, n, density=0.1):
    m = rng.uniform(0, 1, size=(n, 60, 60, 3)) < density
    return (m * rng.integers(0, 256, size=(n, 60, 60, 3))).astype(np.uint8)


def realistic_inputs(seed: int = 0):
    """Xavier networks at two seeds on all-zero, all-255, dense random and sparse random images."""
    rng = np.random.default_rng(seed)
    imgs = np.concatenate([np.zeros((1, 60, 60, 3), np.uint8), np.full((1, 60, 60, 3), 255, np.uint8),
                           rng.integers(0, 256, size=(6, 60, 60, 3), dtype=np.uint8),
                           random_images(rng, 8)])
    return [(f"xavier{s}", make_lenet_weights(s), imgs) for s in (11, 29)]


# ---- split-K rules --------------------------------------------------------------------------------

def fc1_x3_ksplit(mtiles: int) -> int:
    """fc1_x3_ksplit of ag2_device.h: split of ip1's K for mtiles 128-image tiles (bf16 path)."""
    for s in (1, 3, 5, 9, 15, 25, 45):
        if mtiles * 4 * s >= 448:
            return s
    return 45


def split_x3(n: int) -> int:
    return fc1_x3_ksplit((n + 127) // 128)


# batch sizes on each side of every change of the rule, up to the first batch that gets split 1; the
# pairs 1600 / 1601, 2688 / 2689 and 8128 / 8129 (changes of an earlier rule for 64-image tiles) stay as
# further sizes
SPLIT_BATCHES = (1, 512, 513, 896, 897, 1536, 1537, 1600, 1601, 2688, 2689, 2816, 2817, 4736, 4737,
                 8128, 8129, 14208, 14209)
