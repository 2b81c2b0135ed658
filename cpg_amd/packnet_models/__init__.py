"""Model zoo of the PackNet / from-scratch baseline stack (reference: packnet_models/__init__.py).

Provided: vgg16_bn_cifar100 and vgg16_bn.  The PackNet ResNet-18/50 and SphereNet-20 factories -- and with them
packnet_imagenet_main.py's ResNet path, packnet_face_main.py and the PackNet Manager.evalLFW -- are out of scope:
asking for them raises NotImplementedError.
"""
from . import layers  # noqa: F401
from ..models.spherenet import AngleLoss  # noqa: F401
from .vgg import *  # noqa: F401,F403


def _out_of_scope(name):
    def factory(*args, **kwargs):
        raise NotImplementedError('packnet_models.%s: the PackNet ResNet / SphereNet baselines (packnet_imagenet_main.py ResNet path, '
                                  'packnet_face_main.py, PackNet Manager.evalLFW) are out of scope (DESIGN section 7)' % name)
    factory.__name__ = name
    return factory


resnet18, resnet50, spherenet20 = (_out_of_scope(n) for n in ('resnet18', 'resnet50', 'spherenet20'))
