"""Parameter containers of PU-Net's shared MLPs (DUP_Net/pytorch_modules.py of the reference): the same module tree, hence
the same ``state_dict`` keys (``layer{i}.conv.weight`` / ``.bias``, ``layer{i}.bn.bn.*`` with batch norm). On the device
path only the parameters are read (``SharedMLP.layers()``); calling a container runs the plain torch modules."""
from typing import List, Tuple

import torch.nn as nn


class BatchNorm2d(nn.Sequential):
    def __init__(self, in_size: int, name: str = ""):
        super(BatchNorm2d, self).__init__()
        self.add_module(name + "bn", nn.BatchNorm2d(in_size))
        nn.init.constant_(self[0].weight, 1.0)
        nn.init.constant_(self[0].bias, 0)


class Conv2d(nn.Sequential):
    """1x1 convolution [+ batch norm] [+ activation] ([+ instance norm]); with preact the order is reversed."""

    def __init__(self, in_size: int, out_size: int, *, kernel_size: Tuple[int, int] = (1, 1),
                 stride: Tuple[int, int] = (1, 1), padding: Tuple[int, int] = (0, 0), activation=nn.ReLU(inplace=True),
                 bn: bool = False, init=nn.init.kaiming_normal_, bias: bool = True, preact: bool = False, name: str = "",
                 instance_norm=False):
        super(Conv2d, self).__init__()
        bias = bias and (not bn)
        conv = nn.Conv2d(in_size, out_size, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias)
        init(conv.weight)
        if bias:
            nn.init.constant_(conv.bias, 0)
        width = in_size if preact else out_size
        post = []
        if bn:
            post.append((name + "bn", BatchNorm2d(width)))
        if activation is not None:
            post.append((name + "activation", activation))
        if not bn and instance_norm:
            post.append((name + "in", nn.InstanceNorm2d(width, affine=False, track_running_stats=False)))
        if preact:
            for k, m in post:
                self.add_module(k, m)
        self.add_module(name + "conv", conv)
        if not preact:
            for k, m in post:
                self.add_module(k, m)
        self.has_bn, self.has_in, self.preact = bn, (not bn and instance_norm), preact
        self.has_act = activation is not None


class SharedMLP(nn.Sequential):
    def __init__(self, args: List[int], *, bn: bool = False, activation=nn.ReLU(inplace=True), preact: bool = False,
                 first: bool = False, name: str = "", instance_norm: bool = False):
        super(SharedMLP, self).__init__()
        for i in range(len(args) - 1):
            plain = not first or not preact or (i != 0)
            self.add_module(name + "layer{}".format(i),
                            Conv2d(args[i], args[i + 1], bn=plain and bn, activation=activation if plain else None,
                                   preact=preact, instance_norm=instance_norm))

    def layers(self):
        """[(W [O,I], b [O], relu: bool), ...] for the device path; raises for anything but conv (+ ReLU)."""
        out = []
        for layer in self:
            if layer.has_bn or layer.has_in or layer.preact:
                raise NotImplementedError("PU-Net on the device path: use_bn / instance_norm / preact variants are not implemented")
            conv = [m for m in layer if isinstance(m, nn.Conv2d)][0]
            act = [m for m in layer if not isinstance(m, nn.Conv2d)]
            if act and not isinstance(act[0], nn.ReLU):
                raise NotImplementedError("PU-Net on the device path: ReLU is the only activation implemented")
            w = conv.weight.detach().reshape(conv.weight.shape[0], -1)
            out.append((w, conv.bias.detach(), bool(act)))
        return out
