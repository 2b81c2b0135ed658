"""SphereNet-20 of the PackNet baseline stack (counterpart of packnet_models/spherenet.py:93-241).

20 biased 3x3 convolutions with one nn.PReLU each, in four stride-2 stages of residual pairs; no width multiplier, no piggymasks.
Attribute names (`conv1_1`, `relu1_1`, ..., `flatten`, `classifiers.i`) and their registration order are the reference's
(:188-237), and so is the initialisation: nn.Conv2d's constructor draws first, then kaiming normal (fan_out) / zero bias over every
Conv2d and 0.25 over every PReLU (:144-152), heads in add_dataset only (:165-181) -- `torch.manual_seed(s)` gives the reference's
weights bit for bit (tests/golden/packnet_nets_topology.json).  The `face_verification` head is the 25 088 -> 512 embedding layer in
front of AngleLinear, every other head one 25 088 -> classes layer (:154-163); both linear layers are models.layers.HeadLinear (an
nn.Linear on the library's GEMMs), as in the CPG SphereNet.

The trunk runs exactly as models.spherenet.SphereNet._trunk does: conv -> PReLU pairs through conv_prelu (the PReLU's backward
delivers the conv's bias gradient), the first pair of a residual unit through conv_prelu_skip (both gradients of the unit's input meet
in the conv's input-gradient epilogue), the unit's sum inside the second PReLU's kernel.

AngleLinear / AngleLoss are the CPG module's (cpg_amd.models.spherenet): the reference's PackNet AngleLoss (:22-53) calls `F` without
importing it and cannot run.
"""
import torch.nn as nn

from ..models import layers as nl
from ..models.fused_bn import conv_prelu, conv_prelu_skip
from ..models.spherenet import _STAGES, AngleLinear, AngleLoss
from ..models.vgg import View
from .layers import PlainConv2d

__all__ = ['SphereNet20', 'spherenet20', 'AngleLoss', 'AngleLinear']

FLAT = 512 * 7 * 7


class SphereNet20(nn.Module):
    def __init__(self, dataset_history, dataset2num_classes, shared_layer_info={}, init_weights=True):
        super().__init__()
        self.make_feature_layers()
        self.shared_layer_info = shared_layer_info
        self.datasets = dataset_history
        self.classifiers = nn.ModuleList()
        self.dataset2num_classes = dataset2num_classes
        if self.datasets:
            self._reconstruct_classifiers()
        if init_weights != '':                          # (packnet_models/spherenet.py:106: anything but the empty string)
            self._initialize_weights()

    def make_feature_layers(self):
        """conv{s}_{i} / relu{s}_{i} in the reference's registration order (packnet_models/spherenet.py:188-237)."""
        cin = 3
        for stage, c, units in _STAGES:
            setattr(self, 'conv%d_1' % stage, PlainConv2d(cin, c, 3, 2, 1))
            setattr(self, 'relu%d_1' % stage, nn.PReLU(c))
            for i in range(2, 2 * units + 2):
                setattr(self, 'conv%d_%d' % (stage, i), PlainConv2d(c, c, 3, 1, 1))
                setattr(self, 'relu%d_%d' % (stage, i), nn.PReLU(c))
            cin = c
        self.flatten = View(-1, FLAT)

    def _trunk(self, x):
        """packnet_models/spherenet.py:111-123 (= :128-140)."""
        for stage, _, units in _STAGES:
            x = conv_prelu(getattr(self, 'conv%d_1' % stage), getattr(self, 'relu%d_1' % stage), x)
            for u in range(units):
                a, b = 2 * u + 2, 2 * u + 3
                y, skip = conv_prelu_skip(getattr(self, 'conv%d_%d' % (stage, a)), getattr(self, 'relu%d_%d' % (stage, a)), x)
                x = conv_prelu(getattr(self, 'conv%d_%d' % (stage, b)), getattr(self, 'relu%d_%d' % (stage, b)), y, res=skip)
        return self.flatten(x)

    def forward(self, x):
        return self.classifier(self._trunk(x))

    def forward_to_embeddings(self, x):
        return self.classifier[0](self._trunk(x))

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.PReLU):
                nn.init.constant_(m.weight, 0.25)

    @staticmethod
    def _head(dataset, num_classes):
        if 'face_verification' in dataset:
            return nn.Sequential(nl.HeadLinear(FLAT, 512), AngleLinear(512, num_classes))
        return nl.HeadLinear(FLAT, num_classes)

    def _reconstruct_classifiers(self):
        for dataset, num_classes in self.dataset2num_classes.items():
            self.classifiers.append(self._head(dataset, num_classes))

    def add_dataset(self, dataset, num_classes):
        """Append a head for a new task (packnet_models/spherenet.py:165-181)."""
        if dataset in self.datasets:
            return
        self.datasets.append(dataset)
        self.dataset2num_classes[dataset] = num_classes
        head = self._head(dataset, num_classes)
        self.classifiers.append(head)
        if isinstance(head, nn.Sequential):
            nn.init.normal_(head[0].weight, 0, 0.01)
            nn.init.constant_(head[0].bias, 0)
            nn.init.normal_(head[1].weight, 0, 0.01)
        else:
            nn.init.normal_(head.weight, 0, 0.01)
            nn.init.constant_(head.bias, 0)

    def set_dataset(self, dataset):
        assert dataset in self.datasets
        self.classifier = self.classifiers[self.datasets.index(dataset)]


def spherenet20(dataset_history=[], dataset2num_classes={}, shared_layer_info={}, **kwargs):
    return SphereNet20(dataset_history, dataset2num_classes, shared_layer_info, **kwargs)
