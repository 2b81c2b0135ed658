"""Model zoo of the PackNet / from-scratch baseline stack (reference: packnet_models/__init__.py).

    factory(name)       every net of the stack by the reference's name: vgg16_bn_cifar100, vgg16_bn (packnet_cifar100_main_normal.py,
                        packnet_imagenet_main.py's VGG path), resnet50 / resnet101 / resnet152 (packnet_imagenet_main.py's ResNet path,
                        packnet_models.resnet) and spherenet20 (packnet_face_main.py, packnet_models.spherenet).  resnet18 / resnet34 raise
                        NotImplementedError there: the reference gives every PackNet ResNet a 2048-wide head, which a BasicBlock trunk
                        cannot feed.  The resnext* factories, which no reference script selects, are not provided.
                        cpg_amd.baselines.BaselineSession(arch=name) goes through it.

The package's flat attributes are what they were: the two VGG factories, and `resnet18`, `resnet50`, `spherenet20` as names that raise
NotImplementedError -- tests/test_packnet_host.py::test_out_of_scope_factories_say_so pins exactly that, and stays as it is.  The nets
themselves are `packnet_models.resnet.resnet50`, `packnet_models.spherenet.spherenet20` and `factory(...)`.
"""
from . import layers, resnet, spherenet  # noqa: F401
from ..models.spherenet import AngleLoss  # noqa: F401
from .vgg import *  # noqa: F401,F403

_NETS = {'vgg16_bn_cifar100': vgg16_bn_cifar100, 'vgg16_bn': vgg16_bn, 'spherenet20': spherenet.spherenet20,  # noqa: F405
         **{n: getattr(resnet, n) for n in ('resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152')}}


def factory(name):
    """The factory of the net the reference's packnet_models calls `name` (KeyError for a name it does not have or that is not provided)."""
    return _NETS[name]


def _out_of_scope(name):
    def stub(*args, **kwargs):
        raise NotImplementedError('packnet_models.%s: as an attribute of this package the name stays out of scope (it always raised, and an '
                                  'existing test pins that); the PackNet ResNet / SphereNet baselines are packnet_models.factory(%r), '
                                  'packnet_models.resnet and packnet_models.spherenet' % (name, name))
    stub.__name__ = name
    return stub


resnet18, resnet50, spherenet20 = (_out_of_scope(n) for n in ('resnet18', 'resnet50', 'spherenet20'))
