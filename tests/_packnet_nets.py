"""What the host and GPU tests of the PackNet ResNet-50 / SphereNet-20 share: the fixtures' folder, digests, and the nets built the way
tests/golden/make_packnet_nets_golden.py builds the reference's."""
import json
import os
import zlib

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def crc(t):
    return zlib.crc32(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())


def topology():
    with open(os.path.join(GOLDEN, 'packnet_nets_topology.json')) as f:
        return json.load(f)


def build(arch, topo=None):
    """The net as the generator builds the reference's: torch.manual_seed, the factory, then the heads in the fixture's order."""
    import cpg_amd.packnet_models as pm
    topo = topo or topology()
    torch.manual_seed(topo['seed'])
    net = pm.factory(arch)(dataset_history=[], dataset2num_classes={})
    for dataset, n in topo[arch]['heads']:
        net.add_dataset(dataset, n)
    net.set_dataset(topo[arch]['heads'][0][0])
    return net


def covered(net, prefix='module.'):
    return [(prefix + n, m) for n, m in net.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear)) and 'classifiers' not in n]
