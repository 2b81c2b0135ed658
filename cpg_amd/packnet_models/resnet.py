"""Bottleneck ResNets of the PackNet baseline stack (counterpart of packnet_models/resnet.py:59-257).

No width multiplier, no piggymasks, one `Linear(2048, classes)` head per task.  Module names and registration order (`conv1`, `bn1`,
`layerN.M.conv{1,2,3}` / `bnK` / `downsample.{0,1}`, `classifiers.i`: packnet_models/resnet.py:123-137,173-187), parameter shapes and
the initialisation sequence equal the reference's -- the init loop visits every nn.Conv2d (kaiming normal, fan_out) and norm layer
but no head (:144-149), `zero_init_residual` follows (:154-159), heads are drawn in add_dataset only (:189-195; those rebuilt by
_reconstruct_classifiers keep nn.Linear's constructor values, :161-163) --, so `torch.manual_seed(s)` gives its weights bit for bit
and its mask and state_dict keys line up (pinned by tests/golden/packnet_nets_topology.json).  The layers are
packnet_models.layers.PlainConv2d (an nn.Conv2d on the library's kernels) and the forward is the CPG ResNet's (models/resnet.py
here): stem conv -> BatchNorm -> ReLU -> MaxPool as conv_bn_act_pool, each block as conv_bn_act_skip / conv_bn_act / conv_bn_add_act;
the heads are stock nn.Linear, as the CPG ResNet's.

resnet18 / resnet34 raise: the reference's PackNet ResNet builds EVERY head as nn.Linear(2048, n) (:163,:193), a BasicBlock trunk ends
512 wide, so its own resnet18 cannot run a forward pass.  The resnext* factories are selected by none of its scripts and are not
provided (the grouped kernels take no statistics epilogue).
"""
import torch.nn as nn

from ..models.fused_bn import FusedSequential, conv_bn_act, conv_bn_act_pool, conv_bn_act_skip, conv_bn_add_act
from .layers import PlainConv2d

__all__ = ['ResNet', 'Bottleneck', 'resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152']

HEAD_IN = 2048                          # packnet_models/resnet.py:163,193 -- whatever the block type


def conv3x3(in_planes, out_planes, stride=1, groups=1, dilation=1):
    return PlainConv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False, dilation=dilation)


def conv1x1(in_planes, out_planes, stride=1):
    return PlainConv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class Bottleneck(nn.Module):
    """packnet_models/resnet.py:59-99."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        width = int(planes * (base_width / 64.)) * groups
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = norm_layer(width)
        self.conv2 = conv3x3(width, width, stride, groups, dilation)
        self.bn2 = norm_layer(width)
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        # as models.resnet.Bottleneck: the block input reaches the second branch through conv1's autograd node, which adds that branch's
        # gradient in its own input-gradient epilogue
        out, skip = conv_bn_act_skip(self.conv1, self.bn1, self.relu, x)
        identity = skip if self.downsample is None else self.downsample(skip)
        out = conv_bn_act(self.conv2, self.bn2, self.relu, out)
        return conv_bn_add_act(self.conv3, self.bn3, self.relu, out, identity)


class ResNet(nn.Module):
    """Shared trunk + one head per task (packnet_models/resnet.py:102-216)."""

    def __init__(self, block, layers, dataset_history, dataset2num_classes, num_classes=1000, zero_init_residual=False, groups=1,
                 width_per_group=64, replace_stride_with_dilation=None, norm_layer=None):
        super().__init__()
        self._norm_layer = norm_layer or nn.BatchNorm2d
        self.inplanes = 64
        self.dilation = 1
        rswd = replace_stride_with_dilation or [False, False, False]
        if len(rswd) != 3:
            raise ValueError('replace_stride_with_dilation should be None or a 3-element tuple, got {}'.format(rswd))
        self.groups = groups
        self.base_width = width_per_group
        self.conv1 = PlainConv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = self._norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=rswd[0])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=rswd[1])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=rswd[2])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.datasets, self.classifiers = dataset_history, nn.ModuleList()
        self.dataset2num_classes = dataset2num_classes
        if self.datasets:
            self._reconstruct_classifiers()
        # traversal order and distributions of packnet_models/resnet.py:144-149 (RNG parity; no head is drawn here)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)

    def _reconstruct_classifiers(self):
        for num_classes in self.dataset2num_classes.values():
            self.classifiers.append(nn.Linear(HEAD_IN, num_classes))

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False):
        norm_layer = self._norm_layer
        downsample = None
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = FusedSequential(conv1x1(self.inplanes, planes * block.expansion, stride), norm_layer(planes * block.expansion))
        stack = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            stack.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation,
                               norm_layer=norm_layer))
        return nn.Sequential(*stack)

    def add_dataset(self, dataset, num_classes):
        """Append a head for a new task (packnet_models/resnet.py:189-195)."""
        if dataset in self.datasets:
            return
        self.datasets.append(dataset)
        self.dataset2num_classes[dataset] = num_classes
        head = nn.Linear(HEAD_IN, num_classes)
        self.classifiers.append(head)
        nn.init.normal_(head.weight, 0, 0.01)
        nn.init.constant_(head.bias, 0)

    def set_dataset(self, dataset):
        assert dataset in self.datasets
        self.classifier = self.classifiers[self.datasets.index(dataset)]

    def forward(self, x):
        x = conv_bn_act_pool(self.conv1, self.bn1, self.relu, self.maxpool, x)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x)
        return self.classifier(x.view(x.size(0), -1))


def _factory(depths):
    def build(dataset_history=[], dataset2num_classes={}, **kwargs):
        return ResNet(Bottleneck, depths, dataset_history, dataset2num_classes, **kwargs)
    return build


def _basic_block(name):
    def build(*args, **kwargs):
        raise NotImplementedError('packnet_models.%s: the reference builds every head of its PackNet ResNet as nn.Linear(2048, classes) '
                                  '(packnet_models/resnet.py:163,193) and a BasicBlock trunk ends 512 wide, so this net cannot run a '
                                  'forward pass there either (4x512 times 2048xN); use resnet50 / resnet101 / resnet152' % name)
    build.__name__ = name
    return build


resnet18, resnet34 = _basic_block('resnet18'), _basic_block('resnet34')
resnet50 = _factory([3, 4, 6, 3])
resnet101 = _factory([3, 4, 23, 3])
resnet152 = _factory([3, 8, 36, 3])
