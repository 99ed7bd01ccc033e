"""A rank of a multi-GPU job in any call order (ag2_detect without a result buffer, export, all-gather, merge; or the
one-process gather).  From its second call on a rank's detect launches its tail at the shapes its previous call left,
and whether they held travels in the exported header {count, cap, status, images scored}: every export of that
detect must carry the check, and its statistics must be taken up from that detect -- whatever the caller reads in
between (counters, stage times), exports twice, abandons, or merges into a larger pinned block.

Two ranks on the one GPU (two contexts on device 0, adjacent export buffers for the all-gather), each with its own
samples on the busy cloud.  Every order runs once where the shapes hold (third step on the same cloud; held against
the documented order on twin contexts and against the numpy merge of the exported bytes) and once where they do not
(rank 1 moves from the bare table to the busy cloud: status 1, RetryStep on every merge, one redone detect on rank
1, and the repeated step gives what two fresh contexts give)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from agile_grasp2_amd import scene, sharding  # noqa: E402
from conftest import scene_params  # noqa: E402

S = 2500            # samples per rank
CAP = S * 8         # exchange capacity: every slot, never cut
GROW = 4            # the growing merge: a world x cap_records this many times what came before on the context
PER = sharding.compact_bytes(CAP)
PER_BIG = sharding.compact_bytes(GROW * CAP)
RETRY = "retry"
ORDERS = ["documented", "counters_before_export", "times_before_export", "counters_before_merge", "export_again",
          "abandoned", "gather", "grow"]


@functools.lru_cache(maxsize=None)
def _env():
    from agile_grasp2_amd.weights import make_lenet_weights
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    bare, ws1 = scene.make_scene(seed=21, n_target=60000, kind="plane")
    busy, ws2 = scene.make_scene(seed=22, n_target=60000, kind="tabletop")
    wsu = [min(ws1[0], ws2[0]), max(ws1[1], ws2[1]), min(ws1[2], ws2[2]), max(ws1[3], ws2[3]),
           min(ws1[4], ws2[4]), max(ws1[5], ws2[5])]
    lo, hi = bare.min(axis=0), bare.max(axis=0)
    inner = np.flatnonzero((bare[:, 0] > lo[0] + 0.2) & (bare[:, 0] < hi[0] - 0.2) &
                           (bare[:, 1] > lo[1] + 0.2) & (bare[:, 1] < hi[1] - 0.2)).astype(np.int32)
    i_bare = inner[scene.draw_samples(1, len(inner), S)]    # no hand finds anything to close around
    i_busy = [scene.draw_samples(2, busy.shape[0], S), scene.draw_samples(3, busy.shape[0], S)]   # one per rank
    assert not np.array_equal(i_busy[0], i_busy[1])
    dbuf = C.c_void_p()
    assert hip.hipMalloc(C.byref(dbuf), 2 * PER_BIG) == 0   # (freed with the process)
    return dict(hip=hip, w=make_lenet_weights(7), bare=bare, busy=busy, wsu=wsu, i_bare=i_bare, i_busy=i_busy,
                buf=dbuf.value)


def _make(nsel):
    from agile_grasp2_amd import capi
    e = _env()
    d = capi.Detector(**scene_params(e["wsu"], num_selected=nsel, min_score_diff=-1e30))
    d.lenet_load(e["w"])
    return d


def _detect(d, r, kind):
    """rank r's detect (no local selection): kind 'busy' (its own samples) or 'bare' (the empty table)"""
    e = _env()
    d.set_cloud(e[kind])
    d.compute_normals()
    d.detect(sample_idx=e["i_busy"][r] if kind == "busy" else e["i_bare"], slot_base=r * S, seed=4, do_prune=False,
             want_all=False, local_select=False)


def _export(d, r, per=PER, cap=CAP):
    d.export_selected_compact_device(_env()["buf"] + r * per, per, cap)


def _sync():
    assert _env()["hip"].hipDeviceSynchronize() == 0   # (what the all-gather orders: every export before any merge)


def _merge(d, per=PER, cap=CAP):
    from agile_grasp2_amd import capi
    assert per == sharding.compact_bytes(cap)
    try:
        return d.merge_selected_device(_env()["buf"], 2, cap)
    except capi.RetryStep as ex:
        assert "every rank repeats" in str(ex)
        return RETRY


def _raw(per=PER):
    raw = np.zeros(2 * per, dtype=np.uint8)
    assert _env()["hip"].hipMemcpy(raw.ctypes.data_as(C.c_void_p), _env()["buf"], 2 * per, 2) == 0
    return raw


def _headers(per=PER):
    return _raw(per).reshape(2, per)[:, :16].copy().view(np.uint32)


def _numpy_merge(nsel, per=PER, cap=CAP):
    from agile_grasp2_amd import capi
    flat, cut = sharding.unpack_compact(_raw(per), 2, cap, capi.HYP_DTYPE)
    assert not cut
    order = sorted(range(len(flat)), key=lambda i: (-flat["score"][i], i))
    return flat[order if nsel < 0 else order[:nsel]], len(flat)


def _documented(dets, kinds):
    for r, d in enumerate(dets):
        _detect(d, r, kinds[r])
        _export(d, r)
    _sync()
    return [_merge(d) for d in dets]


def _counts(d):
    c = d.counters()
    return dict(n_scored=int(c.n_scored), n_selected=int(c.n_selected), one_trip=int(c.detect_one_trip),
                redone=int(c.detect_redone))


def _run_order(order, dets, kinds):
    """Step 3 of the case in the given call order.  Returns (merge results of this step, what a re-export and the
    merge after it gave, or None, the exchange geometry the headers were left in)."""
    per, cap = (PER_BIG, GROW * CAP) if order == "grow" else (PER, CAP)
    for r, d in enumerate(dets):
        _detect(d, r, kinds[r])
    if order == "abandoned":
        return None, None, (per, cap)
    if order in ("counters_before_export", "gather"):
        for d in dets:
            d.counters()
    if order == "times_before_export":
        for d in dets:
            d.times()
    if order == "gather":
        root = dets[0]
        root.gather_begin(2, cap)
        for r, d in enumerate(dets):
            root.gather_selected(d, r)
        from agile_grasp2_amd import capi
        try:
            res = [root.merge_gathered()]
        except capi.RetryStep:
            res = [RETRY]
        # the same detect exported again, into the all-gather buffer: still checked
        for r, d in enumerate(dets):
            _export(d, r, per, cap)
        _sync()
        return res, [_merge(d, per, cap) for d in dets], (per, cap)
    for r, d in enumerate(dets):
        _export(d, r, per, cap)
    _sync()
    if order == "counters_before_merge":
        for d in dets:
            d.counters()
    res = [_merge(d, per, cap) for d in dets]
    again = None
    if order == "export_again":
        for r, d in enumerate(dets):
            _export(d, r, per, cap)
        _sync()
        again = [_merge(d, per, cap) for d in dets]
    return res, again, (per, cap)


@functools.lru_cache(maxsize=None)
def _twin(nsel):
    """The documented order on two contexts: two steps, then the third -- the shapes hold (both ranks busy)."""
    dets = [_make(nsel), _make(nsel)]
    for _ in range(3):
        res = _documented(dets, ["busy", "busy"])
    h = _headers()
    want, n_total = _numpy_merge(nsel)
    out = dict(res=[(a.tobytes(), n) for a, n in res], counts=[_counts(d) for d in dets], hdr=h.copy(),
               merged=want.tobytes(), n_total=n_total)
    for d in dets:
        d.close()
    assert out["counts"][0]["one_trip"] == 2 and out["counts"][1]["one_trip"] == 2
    assert all(c["redone"] == 0 for c in out["counts"]) and (h[:, 2] == 0).all() and (h[:, 3] > 600).all()
    return out


@functools.lru_cache(maxsize=None)
def _fresh(nsel):
    """One documented step of two fresh contexts, both ranks busy: what a repeated step must give."""
    dets = [_make(nsel), _make(nsel)]
    res = _documented(dets, ["busy", "busy"])
    for d in dets:
        d.close()
    return [(a.tobytes(), n) for a, n in res]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_shapes_held_any_call_order_merges_what_the_documented_order_merges(order):
    nsel = -1 if order == "grow" else 20
    twin = _twin(nsel)
    dets = [_make(nsel), _make(nsel)]
    for _ in range(2):
        _documented(dets, ["busy", "busy"])
    res, again, (per, cap) = _run_order(order, dets, ["busy", "busy"])
    if order == "abandoned":        # its statistics count (one trip), and the next step is one trip as well
        res = _documented(dets, ["busy", "busy"])
        per, cap = PER, CAP
        counts_want = [dict(c, one_trip=c["one_trip"] + 1) for c in twin["counts"]]
    else:
        counts_want = twin["counts"]
    for got in res + (again or []):
        assert got != RETRY, order
        assert (got[0].tobytes(), got[1]) == twin["res"][0], order
    assert twin["res"][1] == twin["res"][0]
    want, n_total = _numpy_merge(nsel, per, cap)
    assert want.tobytes() == twin["merged"] and n_total == twin["n_total"] == res[0][1]
    h = _headers(per)
    assert (h[:, 2] == 0).all() and (h[:, 0] == twin["hdr"][:, 0]).all() and (h[:, 3] == twin["hdr"][:, 3]).all()
    for r, d in enumerate(dets):
        got = _counts(d)
        assert got == counts_want[r], (order, r, got, counts_want[r])
        assert got["n_scored"] == h[r, 3]
        assert d.times().total_ms > 0
    for d in dets:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_shapes_not_held_any_call_order_makes_every_rank_repeat(order):
    nsel = -1 if order == "grow" else 20
    dets = [_make(nsel), _make(nsel)]
    for _ in range(2):                              # rank 1 on the bare table: its shapes have room for 256 images
        first = _documented(dets, ["busy", "bare"])
    assert first[0] != RETRY and [_counts(d)["one_trip"] for d in dets] == [1, 1]
    redone0 = [_counts(d)["redone"] for d in dets]
    assert redone0 == [0, 0]
    res, again, (per, cap) = _run_order(order, dets, ["busy", "busy"])
    if order != "abandoned":
        h = _headers(per)
        assert h[0, 2] == 0 and h[0, 3] > 600 and h[1, 2] == 1 and h[1, 0] == 0 and h[1, 3] > 256, (order, h)
        assert res and all(x == RETRY for x in res), order
        if again is None:                           # a re-export of the same detect, and the merge after it
            for r, d in enumerate(dets):
                _export(d, r, per, cap)
            _sync()
            again = [_merge(d, per, cap) for d in dets]
            h2 = _headers(per)
            assert (h2 == h).all(), order
        assert all(x == RETRY for x in again), order
        assert [_counts(d)["redone"] for d in dets] == [0, 1], order
    # the repeated step (abandoned: the next one, whose detect takes up the abandoned one's statistics and so runs
    # step by step on rank 1 -- no retry)
    redo = _documented(dets, ["busy", "busy"])
    assert all(x != RETRY for x in redo), order
    assert [_counts(d)["redone"] for d in dets] == [0, 1], order
    fresh = _fresh(nsel)
    assert fresh[0] == fresh[1]
    for got in redo:
        assert (got[0].tobytes(), got[1]) == fresh[0], order
    for d in dets:
        d.close()
