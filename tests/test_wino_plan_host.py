"""The public planning queries of the 3x3 s1 p1 layers answer what they answered before the Winograd forward / input-gradient host side
was rebuilt around one plan (conv3x3_wino.hip: WinoPlan): tests/golden/wino_plan_queries.npz, recorded from a build of the commit before
that change by tests/golden/make_golden_wino_plan.py, row for row.  No GPU: the queries launch nothing."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

import cpg_amd._lib as L


def _maker():
    spec = importlib.util.spec_from_file_location('make_golden_wino_plan', os.path.join(GOLDEN, 'make_golden_wino_plan.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def fixture():
    return load_golden('wino_plan_queries')


def test_fixture_is_the_sweep_the_script_makes(fixture):
    mk = _maker()
    assert np.array_equal(fixture['descs'], mk.descriptors())
    assert list(zip(fixture['setting_names'].tolist(), fixture['setting_values'].tolist())) == [(n, v) for n, v in mk.SETTINGS]
    assert list(zip(fixture['query_names'].tolist(), fixture['query_args'].tolist())) == [(q, a) for q, a in mk.QUERIES]
    assert fixture['answers'].shape == (len(mk.SETTINGS), len(mk.descriptors()), len(mk.QUERIES))


def test_fixture_shows_the_tail(fixture):
    """The tail's bytes reach a caller only through cpg_conv2d_workspace_bytes: some rows must differ between the default and CPG_WINO_TAIL=0,
    the hand-computed (256, 512, 512, 14, 14) among them."""
    names = fixture['setting_names'].tolist()
    a = fixture['answers']
    rows = np.flatnonzero((a[0] != a[names.index('CPG_WINO_TAIL')]).any(axis=1))
    assert len(rows) > 0 and np.array_equal(rows, fixture['tail_rows'])
    assert [256, 512, 14, 14, 512] in fixture['descs'][rows].tolist()


def test_answers_equal_the_parents_row_for_row(fixture):
    mk = _maker()
    settings = list(zip(fixture['setting_names'].tolist(), fixture['setting_values'].tolist()))
    queries = list(zip(fixture['query_names'].tolist(), fixture['query_args'].tolist()))
    got = mk.answers(L, fixture['descs'], settings, queries)
    want = fixture['answers']
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ['%s=%s N,C,H,W,K=%s %s(%d): %d, recorded %d' % (settings[s] + (fixture['descs'][d].tolist(),) + queries[q] + (got[s, d, q], want[s, d, q]))
                           for s, d, q in bad[:8]]
