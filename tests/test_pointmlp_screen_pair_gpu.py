"""GPU parity, no tolerances: the fp16-screened tower forward with its candidates rechecked one lane per (channel,
candidate) PAIR (recheck="pair", csrc/pointmlp_screen.hip) against the same launch rechecked by channel and against the
exact fp32 kernel. A wave owns up to 128 channels; its pairs, channels ascending, fill trips of 64 lanes, so a channel's
pairs can straddle a trip boundary and meet again in the channel's LDS key. The cases below put that boundary through a
channel, fill the 2048-entry schedule, leave waves and schedules empty, and mix screened and fallen blocks in one wave."""
import importlib
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import hip_pointnet
from test_pointmlp_screen_gpu import _host_h2
from test_pointmlp_screen_prepared_gpu import _assert_same, _flat, _packed, _weights

pytestmark = pytest.mark.gpu

TILE = 128
PCAP = 16       # PMH_PCAP: candidates per (tile, channel) before the channel's block runs the exact block


def _run(ops, x, w, relu_last, x_cf=True, **kw):
    a = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, fold=False, **kw)
    b = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, want_masks=True, **kw)
    return _flat(a) + _flat(b)


def _stats(ops, x, w, recheck="pair", relu_last=False, **kw):
    dbg = {}
    ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, screen_dbg=dbg, form="fp16", recheck=recheck, **kw)
    return dbg["stats"].cpu().numpy().astype(np.int64)


def _assert_parity(ops, x, wp, bitwise_nan=False, **kw):
    """pair == channel and pair == exact: part_val, part_idx, pooled, argidx and the masks, relu_last both ways, both
    point layouts; the image must have been there (or the fp16 form was not what ran)."""
    for relu_last in (False, True):
        for x_cf, xx in ((True, x), (False, x.transpose(1, 2).contiguous())):
            pr = _run(ops, xx, wp, relu_last, x_cf=x_cf, form="fp16", recheck="pair", **kw)
            assert len(wp[7]) == 4 and wp[7][3] == (wp[4].data_ptr(), wp[4]._version) and ops._pm_w3_h(wp[7][0]) is not None
            ch = _run(ops, xx, wp, relu_last, x_cf=x_cf, form="fp16", recheck="channel", **kw)
            ex = _run(ops, xx, wp, relu_last, x_cf=x_cf, exact=True, **kw)
            torch.cuda.synchronize()
            _assert_same(ch, pr, f"pair vs channel (relu_last={relu_last}, x_cf={x_cf})", bitwise_nan)
            _assert_same(ex, pr, f"pair vs exact (relu_last={relu_last}, x_cf={x_cf})", bitwise_nan)
    assert ops.pointmlp3_pair_recheck_ready(x.device)     # so the pair kernel is what the named launches ran


def _one(dev):
    return (torch.randn(1, 3, 1, generator=torch.Generator().manual_seed(11)) * 0.5).to(dev)


# n candidates in EVERY channel (checked with the CPU restatement of the screen at jitter 1e-4 .. 1e-6; asserted below
# through stats). n = 3: a wave's pairs 63, 64, 65 are one channel's. C3 = 288: wave 0 has two slots, 192 pairs, three
# full trips with a cut at both boundaries; the other waves one slot and a half-filled last trip. n = 16, C3 = 1024:
# the whole 2048-entry schedule.
@pytest.mark.parametrize("C3", [288, 1024])
@pytest.mark.parametrize("n", [3, 5, 7, 16])
def test_pairs_straddle_a_trip_boundary(ops, dev, n, C3):
    wp = _packed(_weights(dev, C3, 5))
    g = torch.Generator().manual_seed(11)
    one = torch.randn(1, 3, 1, generator=g) * 0.5
    x = (one + 1e-5 * torch.randn(1, 3, n, generator=g)).to(dev).contiguous()
    _assert_parity(ops, x, wp)
    for recheck in ("pair", "channel"):
        st = _stats(ops, x, wp, recheck)
        assert st[..., 1].sum() == 0, f"{recheck}: {st[..., 1].sum()} blocks fell back"
        assert st[..., 0].sum() == n * C3, f"{recheck}: {st[..., 0].sum()} candidates, not {n} in each of {C3} channels"
    _, pi = ops.pointmlp3_max_fwd_raw(x, wp, False, fold=False, form="fp16", recheck="pair")
    wins = np.bincount(pi.cpu().numpy().ravel(), minlength=n)
    print(f"[pair recheck] n={n} C3={C3}: winners per position {wins.tolist()}")
    assert (wins > 0).sum() >= 2          # the winner sits on either side of a boundary


@pytest.mark.parametrize("C3", [288, 1024])
@pytest.mark.parametrize("n", [3, 5, 7, 16])
def test_exact_ties_across_a_boundary(ops, dev, n, C3):
    """n identical points: n candidates per channel, all with the same key value; the lowest index wins."""
    wp = _packed(_weights(dev, C3, 5))
    x = _one(dev).expand(1, 3, n).contiguous()
    _assert_parity(ops, x, wp)
    st = _stats(ops, x, wp)
    assert st[..., 1].sum() == 0 and st[..., 0].sum() == n * C3
    _, pi = ops.pointmlp3_max_fwd_raw(x, wp, False, fold=False, form="fp16", recheck="pair")
    assert int(pi.abs().max()) == 0


def test_duplicated_halves(ops, dev):
    """Each point again at a higher index: both copies of every winner are rechecked, the lower index wins."""
    C3 = 256
    wp = _packed(_weights(dev, C3, 5))
    g = torch.Generator().manual_seed(11)
    torch.randn(1, 3, 1, generator=g)
    half = torch.randn(2, 3, 64, generator=g).to(dev) * 0.5
    x = torch.cat([half, half], dim=2).contiguous()
    _assert_parity(ops, x, wp)
    _, idx = ops.pointmlp3_max_fwd_raw(x, wp, False, form="fp16", recheck="pair")
    assert int(idx.max()) < 64
    st = _stats(ops, x, wp)
    assert st[..., 0].sum() >= 2 * 2 * C3 - 64 * st[..., 1].sum()


def test_screened_slot_next_to_a_fallen_one(ops, dev):
    """C3 = 512: every wave has two slots. 16 copies of Q and 17 of P; W3's rows make every channel of blocks 0-7 prefer
    Q by far (16 candidates: screened, full slots) and every channel of blocks 8-15 prefer P (17: the block falls back),
    so each wave schedules one full slot and skips the other."""
    C3 = 512
    w = _weights(dev, C3, 5)
    g = torch.Generator().manual_seed(13)
    Q, P = (torch.randn(1, 3, 1, generator=g) * 0.5).to(dev), (torch.randn(1, 3, 1, generator=g) * 0.5).to(dev)
    x = torch.cat([Q.expand(1, 3, PCAP), P.expand(1, 3, PCAP + 1)], dim=2).contiguous()
    _, _, masks = ops.pointmlp3_max_fwd_raw(x, w, False, want_masks=True, exact=True)
    h2 = _host_h2(x, w, masks[1])[0]                                    # [33, 128] float64
    d = h2[0] - h2[PCAP]                                                # h2(Q) - h2(P)
    assert float(d.norm()) > 0.05 * float(h2[0].norm())                 # the margin |d|^2 is far above E ~ 2^-10 |h2| |d|
    sign = torch.cat([torch.ones(C3 // 2), -torch.ones(C3 // 2)]).double()
    rows = sign[:, None] * d[None, :] / d.norm() + 1e-3 * torch.randn(C3, 128, generator=g).double()
    w[4] = (rows * torch.linspace(0.5, 2.0, C3).double()[:, None]).float().to(dev).contiguous()
    wp = _packed(w)                       # the images are made from the edited weights
    _assert_parity(ops, x, wp)
    for recheck in ("pair", "channel"):
        st = _stats(ops, x, wp, recheck)
        assert st[..., 1].sum() == C3 // 64, f"{recheck}: {st[..., 1].sum()} blocks fell back, not 8"
        assert st[..., 0].sum() == PCAP * (C3 // 2), f"{recheck}: {st[..., 0].sum()} candidates, not 16 * 256"
    _, pi = ops.pointmlp3_max_fwd_raw(x, wp, False, fold=False, form="fp16", recheck="pair")
    pi = pi.cpu().numpy().ravel()
    assert (pi[:C3 // 2] == 0).all() and (pi[C3 // 2:] == PCAP).all()   # the first copy of Q, the first copy of P


# C3 = 32: one block, seven waves with nothing to do; 96: three waves with one half-filled trip each
@pytest.mark.parametrize("N", [1, 33, 128, 200])
@pytest.mark.parametrize("C3", [32, 96])
def test_idle_waves_and_short_schedules(ops, dev, N, C3):
    B = 1 + (N + C3 // 32) % 3
    torch.manual_seed(B * 100003 + N * 101 + C3)
    wp = _packed(_weights(dev, C3, N + C3))
    x = torch.randn(B, 3, N, device=dev) * 0.5
    _assert_parity(ops, x, wp)
    st = _stats(ops, x, wp)
    ntiles = (N + TILE - 1) // TILE
    assert st[..., 1].sum() == 0 and B * ntiles * C3 <= st[..., 0].sum() <= PCAP * B * ntiles * C3


@pytest.mark.parametrize("variant", ["plain", "T", "T_head"])
def test_variants(ops, dev, variant):
    B, N, C3 = 2, 200, 1024
    torch.manual_seed(B * 100003 + N * 101 + C3)
    wp = _packed(_weights(dev, C3, N + C3))
    x = torch.randn(B, 3, N, device=dev) * 0.5
    kw = {}
    if variant == "T":
        kw["T"] = torch.eye(3, device=dev)[None] + 0.3 * torch.randn(B, 3, 3, device=dev)
    elif variant == "T_head":
        K = 256
        kw["T_head"] = (torch.randn(B, K, device=dev), (torch.randn(9, K, device=dev) / K ** 0.5).contiguous(),
                        torch.eye(3, device=dev).reshape(9).contiguous())
    _assert_parity(ops, x, wp, **kw)
    assert np.array_equal(_stats(ops, x, wp, "pair", **kw), _stats(ops, x, wp, "channel", **kw))


@pytest.mark.parametrize("case", ["nan_coord", "inf_coord", "huge_coord", "w3_nan", "w3_inf", "w3_tiny", "w3_huge"])
def test_non_finite_and_extreme(ops, dev, case):
    B, N, C3 = 2, 200, 256
    torch.manual_seed(7)
    w = _weights(dev, C3, 3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    if case == "nan_coord":
        x[0, 1, 17] = float("nan")
    elif case == "inf_coord":
        x[1, 2, 150] = float("inf")
    elif case == "huge_coord":
        x[0, :, 5] = 1e30
        x[1, :, 140] = -1e30
    elif case == "w3_nan":
        w[4][37, 5] = float("nan")
    elif case == "w3_inf":
        w[4][200, 127] = float("-inf")
    elif case == "w3_tiny":
        w[4] = (w[4] * 1e-38).contiguous()
    elif case == "w3_huge":
        w[4] = (w[4] * 1e30).contiguous()
    wp = _packed(w)                       # the images are made from the edited weights
    _assert_parity(ops, x, wp, bitwise_nan=True)
    assert np.array_equal(_stats(ops, x, wp, "pair"), _stats(ops, x, wp, "channel"))


def test_replayed_graph_and_weight_reload(ops, dev):
    """Eager, capture, replays; then new weights: a new image is made, and the old graph still replays on the old one."""
    graphed = importlib.import_module("3dpointcloudattack_amd.graphed")
    pn = importlib.import_module("3dpointcloudattack_amd.model.pointnet")
    ort = importlib.import_module("oracle.ref_torch")
    torch.manual_seed(5)
    x = torch.randn(4, 3, 300, device=dev) * 0.5

    def run(model, **kw):
        pk = pn.fused_pack(model)
        return ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True, **kw), pk

    model, _ = hip_pointnet(3, dev)
    ref = [t.clone() for t in _flat(run(model, exact=True)[0])]
    eager, pk = run(model, form="fp16", recheck="pair")
    eager = [t.clone() for t in _flat(eager)]
    pack = pk["tower_s"][7]
    assert ops.pointmlp3_pair_recheck_ready(dev)
    _assert_same(ref, eager, "eager pair vs exact")
    graph = torch.cuda.CUDAGraph()
    with graphed.capture_guard() as keep:
        with torch.cuda.graph(graph):
            out, pk_old = run(model, form="fp16", recheck="pair")
    out = _flat(out)
    old_ptr = pack[0].untyped_storage().data_ptr()

    def replay_equals(want):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(want, out, "replay")

    replay_equals(eager)
    model.load_state_dict(ort.seeded_state_dict(model, 4))
    new, pk_new = run(model, form="fp16", recheck="pair")
    new = _flat(new)
    pack_new = pk_new["tower_s"][7]
    assert pack_new is not pack and pack_new[0].untyped_storage().data_ptr() != old_ptr
    _assert_same(_flat(run(model, exact=True)[0]), new, "new weights: pair vs exact")
    assert not torch.equal(new[0], eager[0])
    replay_equals(eager)
    del keep, pk_old


FRESH = r'''
import importlib, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
ops = importlib.import_module("3dpointcloudattack_amd.ops")
from test_pointmlp_screen_prepared_gpu import _flat, _packed, _weights
dev = torch.device("cuda:0")
torch.manual_seed(3)
wp = _packed(_weights(dev, 288, 9))
x = torch.randn(2, 3, 200, device=dev) * 0.5
run = lambda **kw: _flat(ops.pointmlp3_max_fwd_raw(x, wp, False, want_masks=True, form="fp16", **kw))
eager = [t.clone() for t in run(recheck="channel")]     # makes the images; the channel instantiation is now usable
assert not ops.pointmlp3_pair_recheck_ready(dev)
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
graph = torch.cuda.CUDAGraph()
with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
        out = run(recheck="pair")                           # the pair instantiation's first use: inside a capture
assert not ops.pointmlp3_pair_recheck_ready(dev)        # so it was not launched: the channel recheck was captured
graph.replay()
torch.cuda.synchronize()
assert all(torch.equal(a, b) for a, b in zip(eager, out))
after = run(recheck="pair")                                 # outside a capture: now the pair instantiation
torch.cuda.synchronize()
assert ops.pointmlp3_pair_recheck_ready(dev)
assert all(torch.equal(a, b) for a, b in zip(eager, after))
print("fresh capture ok")
'''


def test_first_use_inside_a_capture_takes_the_channel_recheck():
    import os
    out = subprocess.run([sys.executable, "-c", FRESH % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "fresh capture ok" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
