"""CPU: the layer between graphed.LoopGraph and the attacks' captured loops — graphed.loop_key, DeviceLoop and LoopCache —
as plain Python (there is no capture without a GPU: policy only), and the two small functions that moved with it,
CW's bisect_weights and adv_utils.own_adv_kind."""
import copy
import gc
import importlib
import itertools
import weakref

import numpy as np
import pytest
import torch

graphed = importlib.import_module("3dpointcloudattack_amd.graphed")
ops = importlib.import_module("3dpointcloudattack_amd.ops")
cw = importlib.import_module("3dpointcloudattack_amd.attack.CW.CW_attack")
adv_utils = importlib.import_module("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")


def test_loop_cache_drops_the_oldest_inserted_even_after_a_hit():
    cache = graphed.LoopCache(4)
    loops = {k: object() for k in "abcde"}
    for k in "abcd":
        assert cache.put(k, loops[k]) is loops[k]
    assert len(cache) == 4 and cache.get("a") is loops["a"]           # a hit does not refresh "a"
    cache["e"] = loops["e"]                                           # item assignment is put()
    assert len(cache) == 4 and cache.get("a") is None
    assert list(cache.values()) == [loops[k] for k in "bcde"]
    assert graphed.LoopCache().max_entries == 4


def test_loop_cache_of_one_replaces():
    cache = graphed.LoopCache(max_entries=1)
    assert len(cache) == 0 and not cache and cache.get("a") is None and list(cache.values()) == []
    cache.put("a", 1)
    cache.put("b", 2)
    assert len(cache) == 1 and cache.get("a") is None and cache.get("b") == 2 and list(cache.values()) == [2]


def test_loop_key_follows_weights_and_kernel_flavour():
    m = torch.nn.BatchNorm1d(4)
    k0 = graphed.loop_key(m, "cpu", 3, 64, ("logits", 0.0))
    assert k0 == graphed.loop_key(m, torch.device("cpu"), 3, 64, ("logits", 0.0))
    assert k0[:3] == (3, 64, ("logits", 0.0)) and k0[3:] == ("cpu", bool(ops._det()), graphed.weights_key(m))
    assert k0 != graphed.loop_key(m, "cpu", 3, 65, ("logits", 0.0))
    with ops.deterministic(not ops._det()):
        assert graphed.loop_key(m, "cpu", 3, 64, ("logits", 0.0)) != k0
    assert graphed.loop_key(m, "cpu", 3, 64, ("logits", 0.0)) == k0
    m.load_state_dict(copy.deepcopy(m.state_dict()))
    k1 = graphed.loop_key(m, "cpu", 3, 64, ("logits", 0.0))
    assert k1 != k0
    with torch.no_grad():
        m.running_mean.add_(1.0)
    assert graphed.loop_key(m, "cpu", 3, 64, ("logits", 0.0)) != k1


class _Counting(graphed.DeviceLoop):
    def __init__(self, log):
        super().__init__("k", "cpu", counts=(1, 16))
        self.bufs["log"] = log

    def body(self):
        self.bufs["log"].append("pass")


def _loops(log):
    return graphed.DeviceLoop("k", "cpu", counts=(1, 16), body=lambda: log.append("pass")), _Counting(log)


@pytest.mark.parametrize("which", [0, 1], ids=["closure", "method"])
def test_uncaptured_loop_calls_the_body(which):
    log = []
    loop = _loops(log)[which]
    assert loop.key == "k" and loop.graphs is None
    loop.bufs["x"] = 3
    assert loop.x == 3 and not hasattr(loop, "y")                      # a buffer reads as an attribute
    for n in (0, 1, 17):
        del log[:]
        loop.run(n)
        assert log == ["pass"] * n


class _FakeGraph:
    def __init__(self, n, log):
        self.n, self.log = n, log

    def replay(self):
        self.log.append(self.n)


def test_captured_loop_replays_and_does_not_capture_again():
    log, rewound = [], []
    loop = _loops(log)[0]
    fake = graphed.LoopGraph.__new__(graphed.LoopGraph)     # no capture without a GPU: fake graphs, the policy alone
    fake.graphs = {n: _FakeGraph(n, log) for n in (16, 4, 1)}
    loop.graphs = fake
    assert loop.capture(rewind=lambda: rewound.append(1)) is False and loop.graphs is fake and not rewound
    loop.run(37)
    assert log == [16, 16, 4, 1]                                      # replays only: the body would log "pass"


class _Owner:
    pass


@pytest.mark.parametrize("which", [0, 1], ids=["closure", "method"])
def test_a_loop_dies_with_the_owner_of_its_cache_without_the_cycle_collector(which):
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        owner = _Owner()
        owner.lr = 0.5
        owner.cache = graphed.LoopCache(1)
        log = []
        if which == 0:
            lr = owner.lr                                             # what the body needs, as a local: not the owner
            loop = graphed.DeviceLoop("k", "cpu", body=lambda: log.append(lr))
        else:
            loop = _Counting(log)
        owner.cache.put("k", loop)
        loop.run(2)
        assert len(log) == 2
        ref = weakref.ref(loop)
        del loop
        assert ref() is not None
        del owner
        assert ref() is None
    finally:
        if was:
            gc.enable()


@pytest.mark.parametrize("first_step", [True, False], ids=["first_step", "later_step"])
@pytest.mark.parametrize("untargeted", [True, False], ids=["untargeted", "targeted"])
def test_bisect_weights_equals_the_loop_it_replaces(untargeted, first_step):
    """All 2^3 combinations of (hit, score != -1, bestdist <= o_bestdist), one per sample of a batch of 8, against the
    reference's per-sample lines restated here; exact float64 equality."""
    combos = list(itertools.product([True, False], repeat=3))
    B = len(combos)
    assert B == 8
    lab, bs = np.zeros((B,), dtype=np.int64), np.zeros((B,), dtype=np.int64)
    bd, obd = np.zeros((B,)), np.full((B,), 0.25)
    for e, (hit, scored, closer) in enumerate(combos):
        bs[e] = 7 if scored else -1
        equal = hit != untargeted                                     # a hit: score != label (untargeted) / == label (targeted)
        lab[e] = bs[e] if equal else 3                                # (a label of -1 only to reach every combination)
        bd[e] = 0.125 if closer else 0.5
        assert ((bs[e] != lab[e]) if untargeted else (bs[e] == lab[e])) == hit and (bs[e] != -1) == scored
    if first_step:
        lower, upper, cur = np.zeros((B,)), np.ones((B,)) * 80., np.ones((B,)) * 10.
    else:
        lower, upper = np.linspace(0., 7., B), np.linspace(80., 31., B)
        cur = (lower + upper) / 2. + 0.3
    want = [a.copy() for a in (lower, upper, cur)]
    for e in range(B):                                                # attack/CW/CW_attack.py:182-200 of the reference
        if untargeted:
            ok = bs[e] != lab[e] and bs[e] != -1 and bd[e] <= obd[e]
        else:
            ok = bs[e] == lab[e] and bs[e] != -1 and bd[e] <= obd[e]
        if ok:
            want[0][e] = max(want[0][e], want[2][e])
        else:
            want[1][e] = min(want[1][e], want[2][e])
        want[2][e] = (want[0][e] + want[1][e]) / 2.
    hit = (bs != lab) if untargeted else (bs == lab)
    ok = hit & (bs != -1) & (bd <= obd)
    assert ok.any() and not ok.all()
    cw.bisect_weights(lower, upper, cur, ok)
    for got, w in zip((lower, upper, cur), want):
        assert got.dtype == np.float64 and np.array_equal(got, w)


def test_own_adv_kind_is_what_cw_maps():
    holder = cw.CW.__new__(cw.CW)
    for af, want in ((adv_utils.UntargetedLogitsAdvLoss(kappa=30.), ("untargeted_logits", 30.0)),
                     (adv_utils.LogitsAdvLoss(kappa=5), ("logits", 5.0)),
                     (adv_utils.CrossEntropyAdvLoss(), ("cross_entropy", 0.0))):
        holder.adv_func = af
        got = adv_utils.own_adv_kind(af)
        assert got == want and got == holder._own_adv_kind() and isinstance(got[1], float)
    holder.adv_func = lambda logits, target: logits.sum()
    assert adv_utils.own_adv_kind(holder.adv_func) is None and holder._own_adv_kind() is None
