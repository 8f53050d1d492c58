"""GPU: attack/additional_exp CW with device_loop=True, device_rng=True — the loop's rotations and resampling tables drawn
by pc3d_eot_draw_f32 in front of every block of iterations. Pinned to the host-table loop (itself pinned to autograd and to
the reference by tests/test_eot_loop_gpu.py) by feeding that loop the same tables; EOT + renorm + z-only, 2 x 18 iterations:
one block of 16 and two single replays per binary step."""
import importlib
import random

import numpy as np
import pytest
import torch

from helpers import hip_pointnet, unit_cloud

pytestmark = pytest.mark.gpu
M = importlib.import_module
SEED, STEPS, ITERS = 77, 2, 18
SHAPES = {"B3_K192": (3, 192), "B1_K64": (1, 64)}
_DATA = {}


def _mods():
    return (M("3dpointcloudattack_amd.attack.additional_exp.CW_attack"), M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils"), M("3dpointcloudattack_amd.ops"))


def _data(dev, shape):
    if shape not in _DATA:
        B, K = SHAPES[shape]
        net, _ = hip_pointnet(0, dev)
        rng = np.random.default_rng(9)
        pcs = torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)]))
        with torch.no_grad():
            lg = net(pcs.transpose(1, 2).contiguous().to(dev))[0]
        _DATA[shape] = dict(net=net, pcs=pcs, tgt=lg.topk(2, dim=1)[1][:, 1].cpu(), org=lg.argmax(1).cpu())
    return _DATA[shape]


def _make(dev, shape, resample, device_rng=True, seed=SEED, graph=True, device_loop=True, eot=True, dist_func=None,
          binary_step=STEPS, num_iter=ITERS, block=None):
    cwm, adv, dist, _ = _mods()
    df = cwm.PerSampleDist(dist.ChamferDist()) if dist_func is None else dist_func
    atk = cwm.CW(_data(dev, shape)["net"], cwm.AdvLossAdapter(adv.LogitsAdvLoss(0.), adv.UntargetedLogitsAdvLoss(0.)), df,
                 binary_step=binary_step, num_iter=num_iter, whether_target=True, whether_1d=True, whether_3Dtransform=eot,
                 whether_renormalization=True, whether_resample=resample, graph=graph, device_loop=device_loop,
                 device_rng=device_rng, seed=seed)
    if block is not None:
        atk.LOOP_BLOCK = block
    return atk


def _attack(dev, shape, atk):
    """One attack() under the host seeds 2000: (result, torch's generator state, Python's generator state before / after)."""
    d = _data(dev, shape)
    torch.manual_seed(2000)
    random.seed(2000)
    before = random.getstate()
    out = atk.attack(d["pcs"], d["tgt"], d["org"])
    return out, torch.get_rng_state(), (before, random.getstate())


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _tables(atk):
    c = next(iter(atk._loop_cache.values())).bufs
    return [None if c[nm] is None else c[nm].cpu().numpy().copy() for nm in ("rot", "idx", "inv")]


def _tables_equal(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("resample", [False, True], ids=["views", "resample"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_drawn_loop(dev, shape, resample):
    cwm, _, _, ops = _mods()
    B, K = SHAPES[shape]
    pcs = _data(dev, shape)["pcs"].numpy()
    atk = _make(dev, shape, resample)
    assert atk.draw_base == 0 and atk.last_draws is None
    first, gen_first, (py0, py1) = _attack(dev, shape, atk)
    assert atk.last_path == "device_loop" and atk.last_draws == "device" and atk.draw_seconds == 0.0
    assert py0 == py1                                                     # nothing consumed from Python's random
    c = next(iter(atk._loop_cache.values())).bufs
    assert c["rot_pin"] is None and c["idx_pin"] is None and c["inv_pin"] is None
    assert (c["idx"] is not None) == resample and (c["inv"] is not None) == resample
    bd, ba, sn = first
    assert bd.shape == (B,) and ba.shape == (B, K, 3) and 0 <= sn <= B and np.isfinite(ba).all()
    assert np.array_equal(ba[..., :2].astype(np.float32), pcs[..., :2])
    assert np.all(np.abs(ba[..., 2] - pcs[..., 2]) <= 0.4 + 1e-6)
    assert atk.draw_base == STEPS * ITERS
    tab_first = _tables(atk)

    # torch's generator: the start noise alone, as the same attack without views leaves it
    plain = _make(dev, shape, resample, eot=False)
    _, gen_plain, _ = _attack(dev, shape, plain)
    assert plain.last_path == "device_loop" and plain.last_draws is None and plain.draw_base == 0
    assert torch.equal(gen_first, gen_plain)

    # the tables as the last binary step left them: its block of 16 filled rows 0 .. 15, its block of two rows 16 and 17,
    # with the draws n = 18 .. 35
    want = [torch.zeros_like(c[nm]) if c[nm] is not None else None for nm in ("rot", "idx", "inv")]
    ops.eot_draw(SEED, (STEPS - 1) * ITERS, (0, ITERS), *want)
    for got, w in zip(tab_first, want):
        if w is not None:
            assert np.array_equal(got[:ITERS], w.cpu().numpy()[:ITERS])

    # a second call without resetting: other draws; after draw_base = 0 the first run again
    second, _, _ = _attack(dev, shape, atk)
    assert atk.draw_base == 2 * STEPS * ITERS
    assert not _tables_equal(tab_first, _tables(atk))
    atk.draw_base = 0
    again, gen_again, (py0, py1) = _attack(dev, shape, atk)
    assert _same(first, again) and _tables_equal(tab_first, _tables(atk))
    assert torch.equal(gen_first, gen_again) and py0 == py1

    eager, _, _ = _attack(dev, shape, _make(dev, shape, resample, graph=False))
    assert _same(first, eager)                                            # graph replay == eager launches
    small, _, _ = _attack(dev, shape, _make(dev, shape, resample, block=4))
    assert _same(first, small)                                            # five blocks of draws == two: every row is the right one

    # the host-table loop on the same tables: bit-equal results
    host = _make(dev, shape, resample, device_rng=False)
    drawn = [0]

    def same_tables(c, half, count, K_):
        E = c["plan"]["E"]
        rot = torch.zeros((count, E, 3, 3), dtype=torch.float32, device=dev)
        idx = torch.zeros((count, E, K_), dtype=torch.int32, device=dev) if c["idx_pin"] is not None else None
        inv = torch.zeros((count, E, K_, 2), dtype=torch.int32, device=dev) if c["inv_pin"] is not None else None
        ops.eot_draw(SEED, drawn[0], (0, count), rot, idx, inv)
        for nm, t in (("rot_pin", rot), ("idx_pin", idx), ("inv_pin", inv)):
            if t is not None:
                c[nm][half, :count].copy_(t.cpu())
        drawn[0] += count

    host._draw_block = same_tables
    fed, _, _ = _attack(dev, shape, host)
    assert host.last_path == "device_loop" and host.last_draws == "host" and drawn[0] == STEPS * ITERS and host.draw_base == 0
    assert (next(iter(host._loop_cache.values())).bufs["idx_pin"] is not None) == resample
    assert _same(first, fed)


def test_seeds(dev):
    """Another seed gives other tables; seed=None takes torch's initial seed at the first use; the seed keys the state."""
    _, _, _, ops = _mods()
    shape = "B1_K64"
    runs = {}
    for seed in (SEED, SEED + 1, None):
        atk = _make(dev, shape, True, seed=seed, graph=False, binary_step=1, num_iter=2)
        _attack(dev, shape, atk)
        assert atk.last_draws == "device" and atk.draw_base == 2
        runs[seed] = (atk, [t[:2] for t in _tables(atk)])
    assert runs[None][0].seed == 2000                                     # torch.manual_seed(2000) & (2^63 - 1)
    for a, b in ((SEED, SEED + 1), (SEED, None)):
        assert not np.array_equal(runs[a][1][1], runs[b][1][1]) and not np.array_equal(runs[a][1][0], runs[b][1][0])
    for seed, used in ((SEED, SEED), (SEED + 1, SEED + 1), (None, 2000)):
        c = next(iter(runs[seed][0]._loop_cache.values())).bufs
        want = [torch.zeros_like(c[nm]) for nm in ("rot", "idx", "inv")]
        ops.eot_draw(used, 0, (0, 2), *want)
        assert _tables_equal(runs[seed][1], [w.cpu().numpy()[:2] for w in want])
    atk = runs[SEED][0]
    state = next(iter(atk._loop_cache.values()))
    atk.seed = SEED + 1
    atk.draw_base = 0
    _attack(dev, shape, atk)
    assert next(iter(atk._loop_cache.values())) is not state and _tables_equal([t[:2] for t in _tables(atk)], runs[SEED + 1][1])


def test_elsewhere_the_host_draws(dev):
    """ChamferkNNDist, and device_loop=False: the autograd path with the host's draws, bit-equal to device_rng=False under
    the same host seeds; without views nobody draws."""
    cwm, _, dist, _ = _mods()
    shape = "B3_K192"
    for kw in (dict(dist_func=cwm.PerSampleDist(dist.ChamferkNNDist())), dict(device_loop=False)):
        res = []
        for flag in (True, False):
            atk = _make(dev, shape, True, device_rng=flag, binary_step=1, num_iter=2, **kw)
            res.append(_attack(dev, shape, atk))
            assert atk.last_path == "autograd" and atk.last_draws == "host" and atk.draw_base == 0
        assert _same(res[0][0], res[1][0])
        assert torch.equal(res[0][1], res[1][1]) and res[0][2][1] == res[1][2][1]      # both generators consumed alike
        assert res[0][2][0] != res[0][2][1]                                             # ... and Python's was consumed
    atk = _make(dev, shape, False, device_loop=False, eot=False, binary_step=1, num_iter=1)
    _attack(dev, shape, atk)
    assert atk.last_path == "autograd" and atk.last_draws is None
