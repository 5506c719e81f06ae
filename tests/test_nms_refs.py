"""CPU tests of tests/nms_refs.py: the statements of hvr_nms / hvr_nms_first / hvr_multiclass_nms reproduce the recorded vectors of
the reference (g3_nms index for index, g8_det row for row) and the oracle on the tied full-size case; every case the GPU test
(tests/test_nms_kernels_gpu.py) runs meets the conditions it is listed for and is moved by every planted mistake that applies to it;
the recorded seeds are the first that do.  A case with neither a condition nor a mistake is not in the lists."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import nms_refs as R
from tests.golden import cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def O():
    if not os.path.exists(os.path.join(ROOT, 'oracle', 'libhvr_oracle.so')):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'oracle')], check=True)
    from oracle import hvr_oracle
    return hvr_oracle


def gold(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


# ------------------------------------------------------------------------------------------------ recorded vectors
def test_greedy_nms_reproduces_every_g3_case():
    g = gold('g3_nms')
    seen = 0
    for name, dets, thr in C.nms_cases():
        d = dets.numpy()
        if name + '_dets' in g.files:
            assert np.array_equal(d, g[name + '_dets'])
        assert R.greedy_nms(d, thr) == g[name + '_keep'].tolist(), name
        seen += 1
    assert seen == 12
    # IoU exactly 0.5 at thr 0.5: >= suppresses, the planted > does not
    tie = g['tie_iou_half_dets']
    assert R.greedy_nms(tie, 0.5) != R.greedy_nms(tie, 0.5, mistake='gt') == R.greedy_nms(tie, 0.5, ge=False)


def test_multiclass_nms_reproduces_g8():
    g = gold('g8_det')
    info = {}
    dets, labels = R.multiclass_nms(g['bboxes'], g['scores'], 0.001, 0.3, 300, info=info)
    assert info['total'] > 300 and info['cut']
    assert labels.tolist() == g['det_labels'].tolist()
    assert np.array_equal(dets, g['det_bboxes'])


def test_multiclass_nms_equals_the_oracle_on_the_tied_full_size_case(O):
    """the inputs of test_parity_gpu.test_multiclass_nms_full_size_with_ties, and the reference's negative max_num (bbox_nms.py:55-59)"""
    g = torch.Generator().manual_seed(77)
    n, ncls = 300, 31
    xy = torch.rand((n, 2), generator=g) * torch.tensor([900.0, 500.0])
    wh = torch.rand((n, 2), generator=g) * 120 + 8
    boxes = torch.cat([xy, xy + wh], 1)
    scores = (torch.softmax(torch.randn((n, ncls), generator=g) * 2, 1) * 64).round() / 64
    for max_num in (300, 100, 7, -1, -7):
        want_b, want_l = O.multiclass_nms(boxes, scores, 0.001, 0.3, max_num)
        info = {}
        dets, labels = R.multiclass_nms(boxes.numpy(), scores.numpy(), 0.001, 0.3, max_num, info=info)
        assert labels.tolist() == want_l.tolist() and np.array_equal(dets, want_b.numpy()), max_num
        if max_num in (100, 7):
            assert info['cut_tie']


def test_negative_max_num_on_a_gpu_case_equals_the_oracle(O):
    """the statement's reading of the wrapper's negative path at the second shape the GPU test pins it at (R = 64)"""
    b, s = R.mc_inputs(64, 31)
    for max_num in (-1, -7):
        want_b, want_l = O.multiclass_nms(torch.from_numpy(b.copy()), torch.from_numpy(s.copy()), R.MC_SCORE_THR, 0.5, max_num)
        dets, labels = R.multiclass_nms(b, s, R.MC_SCORE_THR, 0.5, max_num)
        assert len(labels) == R.mc_list(64, 31, 0.5)[1]['total'] + max_num > 0
        assert labels.tolist() == want_l.tolist() and np.array_equal(dets, want_b.numpy())


# ------------------------------------------------------------------------------------------------ hvr_nms / hvr_nms_first cases
FAM_N = sorted(set((c[0], c[1]) for c in R.NMS_CASES) | set((c[0], c[1]) for c in R.FIRST_CASES))


@pytest.mark.parametrize('fam,n', FAM_N)
def test_seeds_are_the_first_that_qualify(fam, n):
    """R.qualifies: every hvr_nms and hvr_nms_first case of (family, n) meets its conditions (nms_conditions; max_keep = survivors
    reaches the cap in the last, ragged chunk) and is moved by every mistake of nms_mistakes / first_mistakes."""
    seed = R.seed_of(fam, n)
    for s in range(1, seed):
        assert not R.qualifies(fam, n, s)[0], (fam, n, s)
    ok, why = R.qualifies(fam, n, seed)
    assert ok, (fam, n, seed, why)


def test_no_case_is_kept_for_its_count():
    """every listed case has a condition to check or a mistake that moves it (qualifies holds both to their word)"""
    for fam, n, thr, ge in R.NMS_CASES:
        info = R.case_sweep(fam, n, thr, ge)[1]
        assert len(R.nms_conditions(fam, n, thr, ge, info)) + len(R.nms_mistakes(fam, n, thr, ge)) > 0, (fam, n, thr, ge)
    for fam, n, thr, k in R.FIRST_CASES:
        sweep, info = R.case_sweep(fam, n, thr, True)
        mk = R.first_keep(n, k, info['survivors'])
        ci = {}
        R.cut_sweep(sweep, mk, None, ci)
        # (its condition: where the cap is reached -- test_the_cap_is_reached_in_every_place_on_both_routes needs them all)
        assert R.cap_place(n, ci) in ('first', 'middle', 'last', 'never')
        assert mk >= 1


def test_the_cap_is_reached_in_every_place_on_both_routes():
    """max_keep <= 1024 is the greedy kernel, above it the mask + capped sweep.  Each route sees the cap reached in the first chunk
    (impossible above 1024: 64 boxes a chunk), a middle chunk, the last ragged chunk, and never."""
    places = {'greedy': set(), 'sweep': set()}
    for fam, n, thr, k in R.FIRST_CASES:
        sweep, info = R.case_sweep(fam, n, thr, True)
        mk = R.first_keep(n, k, info['survivors'])
        ci = {}
        R.cut_sweep(sweep, mk, None, ci)
        places['greedy' if mk <= 1024 else 'sweep'].add(R.cap_place(n, ci))
    assert places['greedy'] == {'first', 'middle', 'last', 'never'}, places
    assert places['sweep'] == {'middle', 'last', 'never'}, places


def test_both_readings_of_word_64_occur_at_4097():
    got = set()
    for fam in ('dense', 'sparse', 'ties', 'degenerate'):
        info = R.case_sweep(fam, 4097, R.thr_of(fam, 4097) if fam in ('dense', 'sparse') else 0.5, True)[1]
        got.add('survives' if info['last_survivor_pos'] == 4096 else 'suppressed')
        assert info['last_survivor_pos'] == 4096 or info['cross_half']
    assert got == {'survives', 'suppressed'}


def test_integer_families_are_exact_and_the_float_family_is_decided():
    for fam, n in FAM_N:
        d = R.case_dets(fam, n)
        if fam == 'float':
            assert R.float_margin(d, 0.5) > R.FLOAT_MARGIN
            continue
        assert np.array_equal(d[:, :4], np.round(d[:, :4])) and R.max_area(d) < 2 ** 24 and float(np.abs(d[:, :4]).max()) < 2 ** 12
        assert float(d[:, 4].min()) > 0       # no zero of either sign among the scores
        if fam == 'degenerate':
            w, h = d[:, 2] - d[:, 0] + 1, d[:, 3] - d[:, 1] + 1
            assert ((w == 0) | (h == 0)).sum() > n // 8 and ((w < 0) | (h < 0)).sum() > n // 8
    for (Rr, ncls) in R.MC_SHAPES:
        b, s = R.mc_inputs(Rr, ncls)
        assert np.array_equal(b, np.round(b)) and R.max_area(np.concatenate([b, s[:, :1]], 1)) < 2 ** 24
        assert np.array_equal(s * 64, np.round(s * 64)) and float(s.min()) > 0


def test_degenerate_family_reaches_nan_and_negative_unions():
    """two empty boxes: 0 / 0 = NaN, suppresses nothing; an inverted box never intersects (the width clamps to 0) and its negative area
    can make the union negative: the quotient is -0.0"""
    d = R.case_dets('degenerate', 1025)
    b = d[:, :4]
    area = R._area(b, True)
    nan = neg = 0
    for i in range(0, 200):
        ovr = R.iou_rows(b[i], area[i], b[i + 1:], area[i + 1:])
        nan += int(np.isnan(ovr).sum())
        neg += int((np.signbit(ovr) & (ovr == 0)).sum())
    assert nan > 0 and neg > 0


# ------------------------------------------------------------------------------------------------ hvr_multiclass_nms cases
@pytest.mark.parametrize('Rr,ncls,layout', [(r, c, 'dense') for r, c in R.MC_SHAPES] + [(r, c, 'sparse') for r, c in R.MC_BOUNDARY_SHAPES])
def test_multiclass_seeds_are_the_first_that_qualify(Rr, ncls, layout):
    """R.mc_qualifies: the conditions of mc_conditions at both IoU thresholds (scores ON score_thr, an empty class between full ones,
    IoUs exactly on 0.5, a tie at a cut) and every (case, max_num) moved by every mistake of mc_mistakes; the sparse layout's list is
    longer than both max_num of the sp2 boundary."""
    seed = R.MC_SEEDS.get((Rr, ncls, layout), 1)
    for s in range(1, seed):
        assert not R.mc_qualifies(Rr, ncls, layout, s)[0], s
    ok, why = R.mc_qualifies(Rr, ncls, layout, seed)
    assert ok, why


def test_the_sp2_boundary_follows_the_launchers_formula():
    """next_pow2(9000) = next_pow2(128 * 128) = 16384 candidates take 128 KiB of the 160 KiB - 3072 the merge kernel may use: a select
    list of 2048 entries (16 KiB) fits beside them, one of 4096 does not."""
    for Rr, ncls in R.MC_BOUNDARY_SHAPES:
        m = R.mc_sp2_boundary(Rr, ncls)
        assert R.mc_sp2(Rr, ncls, m) == m == 2048 and R.mc_sp2(Rr, ncls, m + 1) == 0
        assert R.mc_list(Rr, ncls, 0.5, 'sparse')[1]['total'] > m + 1
    assert R.mc_sp2(300, 31, 9000) == 0 and R.mc_sp2(64, 2, 64) == 0 and R.mc_sp2(64, 2, 63) == 64
