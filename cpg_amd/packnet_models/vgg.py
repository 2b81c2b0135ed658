"""VGG16-BN of the PackNet baseline stack (counterpart of packnet_models/vgg.py:25-123,192-232).

No width multiplier, no piggymasks, one `nn.Linear(4096, classes)` head per task: module order, names (`features.N`, `classifiers.i`),
parameter shapes and the initialisation sequence equal the reference's, so `torch.manual_seed(s)` gives its weights and its mask and
state_dict keys line up (pinned by tests/golden/packnet_topology.json).  The trunk's layers are packnet_models.layers.PlainConv2d /
PlainLinear -- nn.Conv2d / nn.Linear subclasses on the library's kernels -- inside the FusedSequential of the CPG models.  The
vgg11..vgg19 factories of the reference are used by none of its scripts and are not provided.
"""
import torch.nn as nn

from ..models.fused_bn import FusedSequential
from ..models.vgg import View
from .layers import PlainConv2d, PlainLinear

__all__ = ['VGG', 'vgg16_bn', 'vgg16_bn_cifar100']

CFG_D = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']
HEAD_IN = 4096


def _conv_stack(cfg, bias):
    mods, cin = [], 3
    for v in cfg:
        if v == 'M':
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        mods += [PlainConv2d(cin, v, kernel_size=3, padding=1, bias=bias), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
        cin = v
    return mods


def make_layers_cifar100(cfg):
    """32x32 input, bias-free convs, two FC layers without Dropout (packnet_models/vgg.py:74-96)."""
    return FusedSequential(*(_conv_stack(cfg, bias=False) + [View(-1, 512), PlainLinear(512, 4096), nn.ReLU(True),
                                                             PlainLinear(4096, 4096), nn.ReLU(True)]))


def make_layers(cfg):
    """224x224 input, biased convs, Dropout after each FC (packnet_models/vgg.py:98-123)."""
    return FusedSequential(*(_conv_stack(cfg, bias=True) + [View(-1, 512 * 7 * 7), PlainLinear(512 * 7 * 7, 4096), nn.ReLU(True),
                                                            nn.Dropout(), PlainLinear(4096, 4096), nn.ReLU(True), nn.Dropout()]))


class VGG(nn.Module):
    """Shared trunk + one head per task (packnet_models/vgg.py:25-72)."""
    head_in = HEAD_IN

    def __init__(self, features, dataset_history, dataset2num_classes, init_weights=True):
        super().__init__()
        self.features = features
        self.datasets, self.classifiers = dataset_history, nn.ModuleList()
        self.dataset2num_classes = dataset2num_classes
        if self.datasets:
            self._reconstruct_classifiers()
        if init_weights:
            self._initialize_weights()

    def forward(self, x):
        return self.classifier(self.features(x))

    def _initialize_weights(self):
        # traversal order and distributions of packnet_models/vgg.py:43-54 (RNG parity; the heads that exist are drawn too)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)

    def _reconstruct_classifiers(self):
        for num_classes in self.dataset2num_classes.values():
            self.classifiers.append(PlainLinear(self.head_in, num_classes))

    def add_dataset(self, dataset, num_classes):
        """Append a head for a new task (packnet_models/vgg.py:60-67)."""
        if dataset in self.datasets:
            return
        self.datasets.append(dataset)
        self.dataset2num_classes[dataset] = num_classes
        head = PlainLinear(self.head_in, num_classes)
        self.classifiers.append(head)
        nn.init.normal_(head.weight, 0, 0.01)
        nn.init.constant_(head.bias, 0)

    def set_dataset(self, dataset):
        """Select the active head (packnet_models/vgg.py:69-72)."""
        assert dataset in self.datasets
        self.classifier = self.classifiers[self.datasets.index(dataset)]


def vgg16_bn(pretrained=False, dataset_history=[], dataset2num_classes={}, **kwargs):
    if pretrained:
        kwargs['init_weights'] = False
    return VGG(make_layers(CFG_D), dataset_history, dataset2num_classes, **kwargs)


def vgg16_bn_cifar100(pretrained=False, dataset_history=[], dataset2num_classes={}, **kwargs):
    if pretrained:
        kwargs['init_weights'] = False
    return VGG(make_layers_cifar100(CFG_D), dataset_history, dataset2num_classes, **kwargs)
