"""ctypes binding of libcpg_hip.so (include/cpg_hip.h) -- the only bridge between the Python
mirror of the reference's classes and the HIP kernels.

There is NO CPU fallback: if the shared library is missing or a tensor is not a contiguous
fp32/uint8 HIP tensor, the call raises.  (The CPU oracle under oracle/ is test infrastructure
and is never imported from here.)
"""
import ctypes
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CPG_HIP_LIB') or os.path.join(_HERE, 'lib', 'libcpg_hip.so')   # override: A/B kernel experiments

ABI_VERSION = 3         # include/cpg_hip.h: CPG_ABI_VERSION
CPG_OK = 0
CPG_E_KRANGE = 2
CPG_E_INVALID = -1
MODE_FINETUNE = 0
MODE_PRUNE = 1



class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ('N', 'C', 'H', 'W', 'K', 'R', 'S', 'stride_h', 'stride_w', 'pad_h', 'pad_w', 'dil_h', 'dil_w', 'groups')]


class PruneResult(ctypes.Structure):
    _fields_ = [('n_candidates', ctypes.c_int64), ('k', ctypes.c_int64), ('n_released', ctypes.c_int64),
                ('cutoff', ctypes.c_float), ('status', ctypes.c_int32)]


class SgdItem(ctypes.Structure):                  # cpg_sgd_item
    _fields_ = [('w', ctypes.c_void_p), ('gw', ctypes.c_void_p), ('momentum_buf', ctypes.c_void_p), ('owner', ctypes.c_void_p),
                ('n', ctypes.c_int64)]


class AdamItem(ctypes.Structure):                 # cpg_adam_item
    _fields_ = [('pm', ctypes.c_void_p), ('gpm', ctypes.c_void_p), ('exp_avg', ctypes.c_void_p), ('exp_avg_sq', ctypes.c_void_p),
                ('owner', ctypes.c_void_p), ('n', ctypes.c_int64)]


class ResampleItem(ctypes.Structure):            # cpg_resample_item
    _fields_ = [('src_off', ctypes.c_int64), ('src_h', ctypes.c_int32), ('src_w', ctypes.c_int32), ('crop_y', ctypes.c_int32),
                ('crop_x', ctypes.c_int32), ('crop_h', ctypes.c_int32), ('crop_w', ctypes.c_int32), ('dst_off', ctypes.c_int64),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32)]


class TensorItem(ctypes.Structure):             # cpg_tensor_item
    _fields_ = [('src_off', ctypes.c_int64)] + [(n, ctypes.c_int32) for n in
                                                ('src_h', 'src_w', 'y0', 'x0', 'flip', 'cut_y0', 'cut_y1', 'cut_x0', 'cut_x1', 'reserved')]


PRUNE_RESULT_BYTES = ctypes.sizeof(PruneResult)
assert PRUNE_RESULT_BYTES == 32
assert ctypes.sizeof(ResampleItem) == ctypes.sizeof(TensorItem) == 48

# name -> (restype, argtypes); mirrors include/cpg_hip.h one to one (tests/test_abi_and_host.py compares every slot with the header)
_vp, _int, _i32, _i64, _sz, _f32, _f64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float,
                                         ctypes.c_double)
_desc = ctypes.POINTER(ConvDesc)
_SIGNATURES = {
    'cpg_version': (_int, []),
    'cpg_set_shared_chip_hint': (_int, [_i32]),
    'cpg_get_shared_chip_hint': (_i32, []),
    'cpg_set_option': (_int, [ctypes.c_char_p, _i32]),
    'cpg_get_option': (_int, [ctypes.c_char_p, ctypes.POINTER(_i32)]),
    'cpg_last_error': (ctypes.c_char_p, []),
    'cpg_binarize_mask_weight': (_int, [_vp, _vp, _f32, _vp, _i64, _vp]),
    'cpg_conv2d_workspace_bytes': (_sz, [_desc]),
    'cpg_conv2d_fwd': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_dgrad': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_dgrad_add_supported': (_i32, [_desc]),
    'cpg_conv2d_dgrad_add': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_wgrad': (_int, [_desc, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_pack_bytes': (_sz, [_desc, _i32]),
    'cpg_conv2d_pack': (_int, [_desc, _vp, _vp, _f32, _i32, _vp, _sz, _i32, _vp, _sz, _vp]),
    'cpg_conv2d_use_packed': (_int, [_vp, _sz]),
    'cpg_bn_relu_bwd_reduce': (_int, [_vp] * 9 + [_i32] * 3 + [_vp, _sz, _vp]),
    'cpg_conv2d_wgrad_rider_supported': (_i32, [_desc]),
    'cpg_conv2d_wgrad_attach_bn_bwd': (_int, [_vp] * 4 + [_i32] * 3),
    'cpg_conv2d_fwd_pool_max_supported': (_i32, [_desc]),
    'cpg_conv2d_fwd_attach_pool_max': (_int, [_vp, _sz]),
    'cpg_linear_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'cpg_linear_fwd': (_int, [_vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_linear_dgrad': (_int, [_vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_linear_wgrad': (_int, [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_route_grads': (_int, [_vp, _vp, _vp, _i32, _f32, _vp, _i32, _i64, _vp]),
    'cpg_rank_prune_workspace_bytes': (_sz, []),
    'cpg_rank_prune': (_int, [_vp, _vp, _i32, _f64, _i64, _vp, _vp, _sz, _vp]),
    'cpg_rank_prune_zero': (_int, [_vp, _vp, _i32, _f64, _i64, _vp, _vp, _sz, _vp]),
    'cpg_mask_hist': (_int, [_vp, _vp, _i32, _i64, _vp, _vp]),
    'cpg_apply_mask': (_int, [_vp, _vp, _i32, _i64, _vp]),
    'cpg_zero_pruned': (_int, [_vp, _vp, _i64, _vp]),
    'cpg_claim_free': (_int, [_vp, _i32, _i64, _vp]),
    'cpg_owned_num_blocks': (_i64, [_i64]),
    'cpg_owned_block_counts': (_int, [_vp, _i32, _i32, _i64, _vp, _vp]),
    'cpg_pack_owned': (_int, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp]),
    'cpg_unpack_owned': (_int, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp]),
    'cpg_sgd_route_step': (_int, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _i32, _i32, _i64, _vp]),
    'cpg_multi_tensor_max': (_i32, []),
    'cpg_sgd_route_step_multi': (_int, [ctypes.POINTER(SgdItem), _i32, _i32, _f32, _f32, _f32, _i32, _i32, _vp]),
    'cpg_adam_route_step_multi': (_int, [ctypes.POINTER(AdamItem), _i32, _i32, _i32, _f64, _f64, _f64, _f64, _i32, _vp]),
    'cpg_sgd_route_zero_step': (_int, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _i32, _i32, _i64, _vp]),
    'cpg_sgd_route_zero_step_multi': (_int, [ctypes.POINTER(SgdItem), _i32, _i32, _f32, _f32, _f32, _i32, _i32, _vp]),
    'cpg_step_stats_workspace_bytes': (_sz, [ctypes.POINTER(_i64), _i32]),
    'cpg_sgd_route_step_multi_stats': (_int, [ctypes.POINTER(SgdItem), _i32, _i32, _f32, _f32, _f32, _i32, _i32, _i64, _vp, _vp, _sz, _vp, _vp]),
    'cpg_sgd_route_zero_step_multi_stats': (_int, [ctypes.POINTER(SgdItem), _i32, _i32, _f32, _f32, _f32, _i32, _i32, _i64, _vp, _vp, _sz, _vp,
                                                   _vp]),
    'cpg_adam_route_step_multi_stats': (_int, [ctypes.POINTER(AdamItem), _i32, _i32, _i32, _f64, _f64, _f64, _f64, _i32, _f32, _i64, _vp, _vp,
                                               _sz, _vp, _vp]),
    'cpg_adam_route_step': (_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _f64, _f64, _i32, _i64, _vp]),
    'cpg_bn_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'cpg_bn_relu_fwd_train': (_int, [_vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_bn_relu_fwd_eval': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    'cpg_bn_relu_pool_fwd': (_int, [_vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_bn_relu_pool_bwd': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_bn_relu_pool_attach_max': (_int, [_vp, _sz]),
    'cpg_bn_relu_pool_fwd_from_max': (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _f32, _f32] + [_vp] * 6 + [_i32] * 4 + [_vp]),
    'cpg_bn_relu_pool_bwd_from_max': (_int, [_vp] * 10 + [_i32] * 5 + [_vp, _sz, _vp]),
    'cpg_bn_relu_bwd': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_conv2d_winograd': (_i32, [_desc, _i32]),
    'cpg_conv2d_bnstats_tiles': (_i32, [_desc]),
    'cpg_conv2d_fwd_bnstats': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    'cpg_conv2d_fwd_bn_eval_supported': (_i32, [_desc]),
    'cpg_conv2d_fwd_bn_eval': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_fwd_bn_eval_pool_supported': (_i32, [_desc]),
    'cpg_conv2d_fwd_bn_eval_pool': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_fwd_bn_eval_add_supported': (_i32, [_desc]),
    'cpg_conv2d_fwd_bn_eval_add': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_fwd_prelu_eval_supported': (_i32, [_desc, _i32]),
    'cpg_conv2d_fwd_prelu_eval': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_bf16_supported': (_i32, [_desc]),
    'cpg_conv2d_bf16_workspace_bytes': (_sz, [_desc]),
    'cpg_conv2d_fwd_bf16': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_wgrad_bf16_supported': (_i32, [_desc]),
    'cpg_conv2d_wgrad_bf16_workspace_bytes': (_sz, [_desc]),
    'cpg_conv2d_wgrad_bf16': (_int, [_desc, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_fwd_bf16x3': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_dgrad_bf16x3': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_wgrad_bf16x3': (_int, [_desc, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_dgrad_bf16': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _sz, _vp]),
    'cpg_conv2d_dgrad_bnbwd_tiles': (_i32, [_desc]),
    'cpg_conv2d_dgrad_bnbwd': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    'cpg_bn_bwd_from_partials': (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_bn_bwd_finalize_partials': (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    'cpg_stem_bn_supported': (_i32, [_desc]),
    'cpg_stem_bn_tiles': (_i32, [_desc]),
    'cpg_stem_bn_stats': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _sz, _vp]),
    'cpg_stem_bn_relu_fwd': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cpg_stem_bn_relu_bwd_reduce': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'cpg_stem_bn_relu_bwd_apply': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cpg_stem_bn_wgrad_workspace': (_sz, [_desc]),
    'cpg_stem_bn_relu_bwd_wgrad': (_int, [_desc, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'cpg_bn_stats_finalize_count': (_int, [_vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cpg_bn_stats_finalize': (_int, [_vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp]),
    'cpg_bn_add_relu_mask_bytes': (_sz, [_i32, _i32, _i32]),
    'cpg_bn_add_relu_fwd': (_int, [_vp, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp]),
    'cpg_bn_relu_pool3_supported': (_i32, [_i32, _i32]),
    'cpg_bn_relu_pool3_fwd': (_int, [_vp] * 6 + [_i32] * 4 + [_vp]),
    'cpg_bn_relu_pool3_bwd': (_int, [_vp] * 9 + [_i32] * 5 + [_vp, _sz, _vp]),
    'cpg_bn_add_relu_bwd': (_int, [_vp] * 11 + [_i32] * 4 + [_vp, _sz, _vp, _vp]),
    'cpg_prelu_fwd': (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    'cpg_prelu_bwd_bias': (_int, [_vp] * 6 + [_i32] * 4 + [_vp, _sz, _vp]),
    'cpg_prelu_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'cpg_prelu_bwd': (_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    'cpg_image_resample_workspace_bytes': (_sz, [ctypes.POINTER(ResampleItem), _i32]),
    'cpg_image_resample': (_int, [_vp, _i64, ctypes.POINTER(ResampleItem), _i32, _vp, _i64, _vp, _sz, _vp]),
    'cpg_image_to_tensor': (_int, [_vp, _i64, ctypes.POINTER(TensorItem), _i32, _i32, _i32, ctypes.POINTER(_f32), ctypes.POINTER(_f32), _vp,
                                           _i64, _vp]),
    'cpg_pair_distance': (_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
    'cpg_pair_sweep': (_int, [_vp, _vp, _i64, ctypes.POINTER(_f64), _i32, _i32, _vp, _vp, _vp]),
    'cpg_pair_fold_mean': (_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp]),
    'cpg_pair_distance_centred': (_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    'cpg_pair_sweep_folds': (_int, [_vp, _i64, _vp, _i64, ctypes.POINTER(_f64), _i32, _i32, _vp, _vp, _vp]),
    'cpg_pair_val_max_thresholds': (_i32, []),
    'cpg_pair_val_workspace_bytes': (_sz, [_i32]),
    'cpg_pair_val_table': (_int, [_vp, _i64, _vp, _i64, ctypes.POINTER(_f64), _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_pair_val_at': (_int, [_vp, _i64, _vp, _i64, ctypes.POINTER(_f64), _i32, _vp, _vp]),
    'cpg_loss_heads_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'cpg_softmax_xent_fwd': (_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    'cpg_softmax_xent_fwd_bwd': (_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'cpg_angle_head_fwd': (_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _f64] + [_vp] * 7 + [_sz, _vp]),
    'cpg_angle_head_bwd': (_int, [_vp] * 7 + [_i32, _i32, _i32, _i32, _f32, _f64, _vp, _vp, _vp, _sz, _vp]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


class CpgHipError(RuntimeError):
    def __init__(self, fn, code, text):
        super().__init__('%s failed with status %d: %s' % (fn, code, text))
        self.code = code


def lib():
    """Load libcpg_hip.so once; raise (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'cpg_amd: %s is missing -- build it with `python -m cpg_amd.build` (hipcc, gfx950). '
                'There is no CPU fallback for the masked-layer / prune path.' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if handle.cpg_version() != ABI_VERSION:
            raise RuntimeError('cpg_amd: ABI version mismatch (library %d, binding %d)' % (handle.cpg_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(fn_name, code):
    if code != CPG_OK:
        text = lib().cpg_last_error()
        raise CpgHipError(fn_name, code, text.decode(errors='replace') if text else '')


def call(name, *args):
    """One status-returning entry point: looked up on lib() at call time (a profiler may have put a proxy there), raised on failure under
    its own name."""
    rc = getattr(_lib if _lib is not None else lib(), name)(*args)
    if rc != CPG_OK:
        check(name, rc)


def call_armed(arms, name, *args):
    """call() of ONE entry point with the calling thread armed first; arms: (attach entry point, its arguments) pairs, each made through
    call() under its own name.  The library disarms itself inside the entry point that consumes a value; if anything raises on the way
    there (a later arm that is refused, an interrupt) or in it, every channel of `arms` is disarmed again (NULL pointers and zeros, on
    the library handle directly), so that no LATER call of this thread picks up a value that was not meant for it."""
    try:
        for arm, arm_args in arms:
            call(arm, *arm_args)
        call(name, *args)
    except BaseException:
        for arm, _ in arms:
            getattr(lib(), arm)(*(None if t is _vp else 0 for t in _SIGNATURES[arm][1]))
        raise


def use_packed(pk):
    """The arm of call_armed for a packed weight operand (None: no arm)."""
    return () if pk is None else (('cpg_conv2d_use_packed', (dptr(pk), pk.numel() * 4)),)


OPT_UNSET = -(1 << 31)
_WINO_KERNEL = {'block': 0, 'wave': 1, 'pair': 2, '64': 3}


def get_option(name):
    """Current value of a library switch (include/cpg_hip.h: cpg_get_option); None when it was never given."""
    v = ctypes.c_int32(0)
    call('cpg_get_option', name.encode(), ctypes.byref(v))
    return None if v.value == OPT_UNSET else v.value


def set_option(name, value):
    """Set (value None: unset) a library switch through the C ABI.  The table is filled from the environment once, at load time; this is
    the only way to change it afterwards.  CPG_WINO_KERNEL also takes its environment spelling ('block' | 'wave' | 'pair' | '64')."""
    if isinstance(value, str):
        value = _WINO_KERNEL[value] if name == 'CPG_WINO_KERNEL' else int(value)
    call('cpg_set_option', name.encode(), OPT_UNSET if value is None else int(value))
    _PACK_BYTES.clear()                     # which kernel family (hence which packed operand) a shape gets depends on the switches


_PACK_BYTES = {}


def pack_bytes(d, which):
    """cpg_conv2d_pack_bytes per (shape, pass), memoised: the answer depends on the shape and the library options only (set_option
    clears the table)."""
    key = (d.N, d.C, d.H, d.W, d.K, d.R, d.S, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, d.groups, which)
    v = _PACK_BYTES.get(key)
    if v is None:
        v = _PACK_BYTES[key] = int(lib().cpg_conv2d_pack_bytes(ctypes.byref(d), which))
    return v


class option(object):
    """`with option('CPG_NO_WINO', 1): ...` -- a library switch for the duration of a block (tests, A/B tools)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def stream_ptr():
    """hipStream_t of torch's current stream on the current device."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t, dtype=torch.float32, name='tensor'):
    """Device pointer of a contiguous HIP tensor of the expected dtype (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('cpg_amd: %s lives on %s; the masked-layer kernels only run on a HIP device '
                           '(no CPU fallback -- move the module with .cuda())' % (name, t.device))
    if t.dtype != dtype:
        raise TypeError('cpg_amd: %s must be %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError('cpg_amd: %s must be contiguous' % name)
    return ctypes.c_void_p(t.data_ptr())


def workspace(nbytes, device):
    """Scratch buffer from torch's caching allocator (stream-ordered reuse, no hipMalloc in steady state)."""
    if nbytes == 0:
        return None, 0
    buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return buf, buf.numel() * 4


def _selftest():
    h = lib()
    print('libcpg_hip.so ABI', h.cpg_version(), 'exports', len(EXPORTS))


if __name__ == '__main__':
    _selftest()
    sys.exit(0)
