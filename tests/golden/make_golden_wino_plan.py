#!/usr/bin/env python3
"""Generate tests/golden/wino_plan_queries.npz: what the public planning queries answered for 3x3 s1 p1 layers BEFORE the Winograd
forward / input-gradient host side was rebuilt around one plan (conv3x3_wino.hip: WinoPlan).  tests/test_wino_plan_host.py holds every
later tree to these answers, row for row.

Run it against a build of the commit BEFORE that change (CPG_HIP_LIB selects the library; no GPU is needed, the queries launch nothing):

    CPG_HIP_LIB=/path/to/parent/libcpg_hip.so python tests/golden/make_golden_wino_plan.py

The fixture holds the sweep itself (descriptors, option settings, query names) next to the answers, so the test reads one file.
The tail's bytes reach a caller only through cpg_conv2d_workspace_bytes, a maximum over routes; the script counts the rows that differ
between the default and CPG_WINO_TAIL=0 and refuses to write a fixture in which none does.
"""
import ctypes
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

BATCHES = (1, 11, 32, 256)
CHANNELS = ((3, 64), (8, 16), (16, 16), (16, 64), (64, 64), (64, 128), (96, 128), (78, 78), (128, 64), (156, 313), (512, 512))
MAPS = ((2, 2), (7, 7), (14, 14), (15, 9), (16, 24), (28, 28), (56, 56))
# each applied alone; '' is the default option table
SETTINGS = [('', 0)] + [('CPG_WINO_KERNEL', v) for v in range(4)] + [('CPG_WINO_TAIL', 0), ('CPG_WG3_SHARE', 0), ('CPG_WINO_NW', 8), ('CPG_NO_WINO', 1),
                                                                      ('CPG_NO_WINO_ODD', 1), ('CPG_NO_POOL_MAX', 1), ('CPG_NO_WINO_WGRAD', 1)]
# (query, extra integer argument or -1)
QUERIES = [('cpg_conv2d_workspace_bytes', -1), ('cpg_conv2d_bnstats_tiles', -1)] + [('cpg_conv2d_pack_bytes', p) for p in range(3)] + \
          [('cpg_conv2d_winograd', m) for m in (0, 1, 3)] + \
          [(n, -1) for n in ('cpg_conv2d_fwd_pool_max_supported', 'cpg_conv2d_dgrad_add_supported', 'cpg_conv2d_fwd_bn_eval_supported',
                             'cpg_conv2d_fwd_bn_eval_pool_supported')] + [('cpg_conv2d_fwd_prelu_eval_supported', r) for r in range(2)]


def descriptors():
    return np.array([(N, C, H, W, K) for N in BATCHES for C, K in CHANNELS for H, W in MAPS], np.int64)


def answers(L, descs, settings, queries):
    """[setting][descriptor][query] from the loaded library; every setting is applied alone and taken back."""
    lib = L.lib()
    out = np.zeros((len(settings), len(descs), len(queries)), np.int64)
    for si, (name, value) in enumerate(settings):
        if name:
            L.set_option(name, int(value))
        try:
            for di, (N, C, H, W, K) in enumerate(descs):
                d = L.ConvDesc()
                d.N, d.C, d.H, d.W, d.K, d.R, d.S = int(N), int(C), int(H), int(W), int(K), 3, 3
                d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = d.groups = 1
                for qi, (q, extra) in enumerate(queries):
                    out[si, di, qi] = int(getattr(lib, q)(ctypes.byref(d), *(() if extra < 0 else (int(extra),))))
        finally:
            if name:
                L.set_option(name, None)
    return out


def main():
    from cpg_amd import _lib as L
    descs = descriptors()
    got = answers(L, descs, SETTINGS, QUERIES)
    tail_off = [s[0] for s in SETTINGS].index('CPG_WINO_TAIL')
    rows = np.flatnonzero((got[0] != got[tail_off]).any(axis=1))
    print('library', L.LIB_PATH)
    print('%d descriptors x %d settings x %d queries' % (len(descs), len(SETTINGS), len(QUERIES)))
    print('rows that differ between the default and CPG_WINO_TAIL=0: %d' % len(rows))
    for di in rows:
        print('  N C H W K = %s: workspace %d -> %d bytes' % (tuple(int(v) for v in descs[di]), got[0, di, 0], got[tail_off, di, 0]))
    if len(rows) == 0:
        raise SystemExit('no row shows the tail: extend the sweep')
    path = os.path.join(OUT, 'wino_plan_queries.npz')
    np.savez_compressed(path, descs=descs, setting_names=np.array([s[0] for s in SETTINGS]), setting_values=np.array([s[1] for s in SETTINGS], np.int64),
                        query_names=np.array([q[0] for q in QUERIES]), query_args=np.array([q[1] for q in QUERIES], np.int64), answers=got,
                        tail_rows=rows.astype(np.int64))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
