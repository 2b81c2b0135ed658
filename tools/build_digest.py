#!/usr/bin/env python3
"""Fingerprint of a build, for refactors that must leave the kernels and the planners alone.  Prints one JSON object:

  device   for each .hip of cpg_amd.build.SOURCES the sha256 of the .text, .rodata and .note sections of its gfx950 device ELF
           (code, constants, kernel descriptors and metadata; the ELF as a whole also carries a per-compile __hip_cuid_* symbol)
  planner  a sha256 over the answers of every host-only query entry point of the C ABI, for a fixed sweep of conv descriptors under
           the default option table, every boolean CPG_* switch set one at a time, CPG_WINO_KERNEL 0-3 and every --set NAME=VALUE
           (the integer switches: each one more setting of the sweep, applied alone); `pairs` counts the (descriptor, option setting) pairs

Two trees whose digests agree launch the same device code with the same plans.  Needs hipcc and a built library, no GPU.

    python tools/build_digest.py [--no-device] [--no-planner] [--set CPG_WINO_TAIL=0 --set CPG_WINO_NW=8 ...]
"""
import argparse
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpg_amd import build  # noqa: E402

SECTIONS = ('.text', '.rodata', '.note')


def device_hashes(src, tmp):
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), 'lib', 'llvm', 'bin')
    stem = os.path.join(tmp, os.path.splitext(src)[0])
    cc = subprocess.run([build._hipcc()] + build.FLAGS + ['--offload-device-only', '-x', 'hip', '-c', os.path.join(build.CSRC, src), '-o', stem + '.o'],
                        stderr=subprocess.PIPE)
    if cc.returncode != 0:                                # (warnings of a good compile are the build's business, not this tool's)
        raise RuntimeError('%s: device-only compile failed\n%s' % (src, cc.stderr.decode(errors='replace')))
    subprocess.check_call([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                           '--input=' + stem + '.o', '--output=' + stem + '.elf'])
    out = {}
    for sec in SECTIONS:
        subprocess.check_call([os.path.join(llvm, 'llvm-objcopy'), '-O', 'binary', '--only-section=' + sec, stem + '.elf', stem + sec])
        out[sec] = hashlib.sha256(open(stem + sec, 'rb').read()).hexdigest()
    return out


def device_digest():
    hips = [s for s in build.SOURCES if s.endswith('.hip')]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(hips, pool.map(lambda s: device_hashes(s, tmp), hips)))


def conv(N, C, H, W, K, R, stride=1, groups=1):
    return (N, C, H, W, K, R, R, stride, stride, R // 2, R // 2, 1, 1, groups)


def descriptors():
    vgg = [(3, 64, 224), (64, 64, 224), (64, 128, 112), (128, 128, 112), (128, 256, 56), (256, 256, 56), (256, 512, 28), (512, 512, 28),
           (512, 512, 14)]
    out = []
    for N in (256, 32):
        for mult in (1.0, 1.5):                          # (the reference's raw width multiplier: int(v * sqrt(m)) channels)
            r = mult ** 0.5
            out += [conv(N, c if c == 3 else int(c * r), h, h, int(k * r), 3) for c, k, h in vgg]
        # ResNet-50 @224: the stem, then per stage (input channels, width, map of the stage's input, stride of its first block)
        out.append(conv(N, 3, 224, 224, 64, 7, 2))
        for cin, wd, h, s in ((64, 64, 56, 1), (256, 128, 56, 2), (512, 256, 28, 2), (1024, 512, 14, 2)):
            ho = h // s
            out += [conv(N, cin, h, h, wd, 1), conv(N, wd, h, h, wd, 3, s), conv(N, wd, ho, ho, 4 * wd, 1), conv(N, cin, h, h, 4 * wd, 1, s),
                    conv(N, 4 * wd, ho, ho, wd, 1), conv(N, wd, ho, ho, wd, 3)]
        # SphereNet-20 @112 x 96: a stride-2 3x3 into each stage, 3x3 residual units inside
        h, w, c = 112, 96, 3
        for k in (64, 128, 256, 512):
            out.append((N, c, h, w, k, 3, 3, 2, 2, 1, 1, 1, 1, 1))
            h, w, c = h // 2, w // 2, k
            out.append((N, c, h, w, c, 3, 3, 1, 1, 1, 1, 1, 1, 1))
    chans = (3, 16, 64, 78, 512)
    for R in (1, 3, 7):
        for s in (1, 2):
            for H, W in [(m, m) for m in (7, 14, 28, 56, 112, 224)] + [(15, 9)]:
                for C in chans:
                    for K in chans:
                        for g in (1, 4):
                            out.append((32, C, H, W, K, R, R, s, s, R // 2, R // 2, 1, 1, g))
    return out


LINEAR = [(b, i, o) for b in (256, 32) for i, o in ((25088, 4096), (4096, 4096), (4096, 1000), (2048, 1000), (512 * 7 * 6, 512), (512, 10))]


def option_settings(extra=()):
    # the boolean switches of cpg_common.h's Opt enum are the OPT_NO_* / OPT_DISABLE_* entries; OPT_X is spelled CPG_X
    text = open(os.path.join(build.CSRC, 'cpg_common.h')).read()
    enum = text[text.index('enum Opt {'):text.index('OPT_COUNT')]
    booleans = ['CPG_' + n for n in re.findall(r'^\s*OPT_((?:NO|DISABLE)_\w+),', enum, re.M)]
    return [None] + [(b, 1) for b in booleans] + [('CPG_WINO_KERNEL', v) for v in range(4)] + list(extra)


def planner_digest(extra=()):
    from cpg_amd import _lib as L
    lib = L.lib()
    descs = []
    for t in descriptors():
        d = L.ConvDesc()
        for (name, _), v in zip(L.ConvDesc._fields_, t):
            setattr(d, name, v)
        descs.append(ctypes.byref(d))
    queries = [(lib.cpg_conv2d_workspace_bytes, ())] + [(lib.cpg_conv2d_winograd, (m,)) for m in range(4)] + \
              [(getattr(lib, n), ()) for n in ('cpg_conv2d_bnstats_tiles', 'cpg_conv2d_dgrad_bnbwd_tiles', 'cpg_conv2d_dgrad_add_supported',
                                               'cpg_conv2d_fwd_bn_eval_supported', 'cpg_conv2d_fwd_bn_eval_add_supported',
                                               'cpg_conv2d_wgrad_rider_supported')] + \
              [(lib.cpg_conv2d_fwd_prelu_eval_supported, (r,)) for r in range(2)] + \
              [(lib.cpg_conv2d_pack_bytes, (p,)) for p in range(3)] + \
              [(getattr(lib, n), ()) for n in ('cpg_conv2d_bf16_supported', 'cpg_conv2d_bf16_workspace_bytes', 'cpg_conv2d_wgrad_bf16_supported',
                                               'cpg_conv2d_wgrad_bf16_workspace_bytes', 'cpg_stem_bn_supported', 'cpg_stem_bn_tiles',
                                               'cpg_stem_bn_wgrad_workspace')]
    h = hashlib.sha256()
    pairs = 0
    settings = option_settings(extra)
    for setting in settings:
        if setting is not None:
            L.set_option(*setting)
        for d in descs:
            h.update((','.join(str(int(fn(d, *extra))) for fn, extra in queries) + '\n').encode())
            pairs += 1
        for shape in LINEAR:
            h.update(('%d\n' % lib.cpg_linear_workspace_bytes(*shape)).encode())
        if setting is not None:
            L.set_option(setting[0], None)
    return {'sha256': h.hexdigest(), 'pairs': pairs, 'descriptors': len(descs), 'option_settings': len(settings)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--no-device', action='store_true')
    ap.add_argument('--no-planner', action='store_true')
    ap.add_argument('--set', action='append', default=[], metavar='NAME=VALUE', dest='settings',
                    help='one more option setting of the planner sweep, applied alone (repeatable)')
    a = ap.parse_args()
    extra = []
    for s in a.settings:
        name, eq, value = s.partition('=')
        if not eq or not name.startswith('CPG_') or not re.fullmatch(r'-?\d+', value):
            ap.error('--set takes NAME=VALUE with a CPG_* switch and an integer, not %r' % s)
        extra.append((name, int(value)))
    out = {}
    if not a.no_device:
        out['device'] = device_digest()
    if not a.no_planner:
        out['planner'] = planner_digest(extra)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
