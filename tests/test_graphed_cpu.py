"""CPU: the hipGraph victim wrapper (3dpointcloudattack_amd/graphed.py) as plain Python — which models it wraps, that it
stays out of state_dicts, copies and pickles, and that attribute access falls through to the victim."""
import copy
import importlib
import io
import pickle

import torch

graphed = importlib.import_module("3dpointcloudattack_amd.graphed")
pointnet = importlib.import_module("3dpointcloudattack_amd.model.pointnet")


def test_wrap_only_deterministic_victims_and_cache_on_the_model():
    m = pointnet.PointNetCls(k=5, feature_transform=False).eval()
    g = graphed.wrap(m)
    assert isinstance(g, graphed.GraphedVictim) and graphed.wrap(m) is g and graphed.wrap(g) is g
    assert graphed.wrap(m, enable=False) is m
    assert graphed.wrap(torch.nn.Linear(3, 3)).__class__ is torch.nn.Linear        # no deterministic_forward declared
    assert "_pc3d_graphed" not in dict(m.named_modules()) and not any("graphed" in k for k in m.state_dict())
    assert hasattr(g, "fused_loss_and_grad") and g.deterministic_forward is True    # falls through to the victim
    assert set(g.state_dict()) == set(m.state_dict())
    g.load_state_dict(m.state_dict())


def test_copies_and_pickles_drop_the_captures():
    m = pointnet.PointNetCls(k=5, feature_transform=False).eval()
    g = graphed.wrap(m)
    g._slots["fake"] = [object()]
    g.stats["captures"] = 3
    m2 = copy.deepcopy(m)
    g2 = m2.__dict__["_pc3d_graphed"]
    assert g2 is not g and g2.model is m2 and g2._slots == {} and graphed.wrap(m2) is g2
    g._slots.clear()                                    # the fake entry is not picklable, as real captures are not
    g._slots["k"] = ["capture"]
    buf = io.BytesIO()
    pickle.dump(g, buf)
    g3 = pickle.loads(buf.getvalue())
    assert g3._slots == {} and g3.stats["captures"] == 0
    for a, b in zip(g3.model.state_dict().values(), m.state_dict().values()):
        assert torch.equal(a, b)


def test_unwrap_only_a_graphed_victim():
    m = pointnet.PointNetCls(k=5, feature_transform=False).eval()
    assert graphed.unwrap(graphed.wrap(m)) is m and graphed.unwrap(m) is m
    holder = torch.nn.Sequential()
    holder.model = m                                    # any other module with a .model attribute is left as it is
    assert graphed.unwrap(holder) is holder


def test_weights_key_follows_loads_and_in_place_updates():
    m = torch.nn.BatchNorm1d(4)
    k0 = graphed.weights_key(m)
    assert len(k0) == len(list(m.parameters())) + len(list(m.buffers())) and graphed.weights_key(m) == k0
    m.load_state_dict(copy.deepcopy(m.state_dict()))
    k1 = graphed.weights_key(m)
    assert k1 != k0
    with torch.no_grad():
        m.running_mean.add_(1.0)
    assert graphed.weights_key(m) != k1


def test_loop_graph_run_takes_the_largest_counts_that_fit():
    class Fake:
        def __init__(self, n, log):
            self.n, self.log = n, log

        def replay(self):
            self.log.append(self.n)

    log = []
    loop = graphed.LoopGraph.__new__(graphed.LoopGraph)     # no capture without a GPU: the replay policy alone
    loop.graphs = {n: Fake(n, log) for n in (4, 1, 16)}
    loop.run(37)
    assert log == [16, 16, 4, 1]
    del log[:]
    loop.run(0)
    loop.run(3)
    assert log == [1, 1, 1]
