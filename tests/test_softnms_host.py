"""Host-side checks of the Soft-NMS read-out (no GPU): the numpy restatement tests/softnms_refs.py is pinned to the recorded outputs
of the reference's compiled soft_nms_cpu / multiclass_nms(type='soft_nms') bit for bit (tests/golden/g20_soft_nms.npz), the C ABI
bookkeeping of the new exports, and the argument errors of the public surface."""
import os
import re

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import box_ops, native, ops
from tests import softnms_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['hvr_soft_nms_workspace_bytes', 'hvr_soft_nms', 'hvr_multiclass_soft_nms_workspace_bytes', 'hvr_multiclass_soft_nms']
CODE = {1: 'linear', 2: 'gaussian'}


def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_soft_nms.npz'))


def params(g, key):
    iou_thr, code, sigma, min_score = [float(v) for v in g[key]]
    return dict(iou_thr=iou_thr, method=CODE[int(code)], sigma=sigma, min_score=min_score)


def test_fixture_holds_the_cases_the_read_out_is_specified_on():
    g = gold()
    assert str(g['cython_version']) and str(g['numpy_version'])
    assert [str(n) for n in g['single_names']] == ['n%d_%s' % (n, k) for n in (1, 2, 7, 64, 65, 150, 300, 512) for k in ('cont', 'quant')]
    assert [params(g, 'param_' + str(p)) for p in g['param_names']] == [
        dict(iou_thr=0.3, method='linear', sigma=0.5, min_score=1e-3), dict(iou_thr=0.5, method='linear', sigma=0.5, min_score=0.05),
        dict(iou_thr=0.3, method='gaussian', sigma=0.5, min_score=1e-3), dict(iou_thr=0.5, method='gaussian', sigma=0.3, min_score=0.05)]
    assert [str(n) for n in g['mc_names']] == ['r300', 'r32', 'none'] and g['mc_max_nums'].tolist() == [300, 100, -1]
    assert g['mc_r300_scores'].shape == (300, 31) and g['mc_r32_scores'].shape == (32, 31)
    assert {params(g, 'mc_cfg_' + str(c))['method'] for c in g['mc_cfg_names']} == {'linear', 'gaussian'}
    assert not (g['mc_none_scores'][:, 1:] > float(g['mc_score_thr'])).any()
    # exact ties are part of the quantised lists: equal boxes and equal scores
    q = g['sl_n300_quant_dets']
    assert np.unique(q, axis=0).shape[0] < 300 and np.unique(q[:, 4]).size <= 10


def test_refs_docstring_case():
    g = gold()
    new, inds = R.soft_nms(g['doc_dets'], float(g['doc_iou_thr']), sigma=float(g['doc_sigma']))
    assert len(inds) == len(new) == 3
    assert np.array_equal(inds, g['doc_inds']) and np.array_equal(new[:, 4].view(np.int32), g['doc_scores'].view(np.int32))


def test_refs_soft_nms_equals_reference_bit_for_bit():
    g = gold()
    margin = int(g['ulp_margin'])
    for name in [str(n) for n in g['single_names']]:
        dets = g['sl_%s_dets' % name]
        n, kind = int(name[1:].split('_')[0]), name.split('_')[1]
        assert np.array_equal(dets, R.clustered_dets(int(g['sl_%s_seed' % name]), n, quantised=kind == 'quant'))   # rebuilt from its seed
        for p in [str(p) for p in g['param_names']]:
            prm, info = params(g, 'param_' + p), {}
            new, inds = R.soft_nms(dets, info=info, **prm)
            assert np.array_equal(inds, g['sl_%s_%s_inds' % (name, p)]), (name, p)
            assert np.array_equal(new[:, 4].view(np.int32), g['sl_%s_%s_scores' % (name, p)].view(np.int32)), (name, p)
            assert np.array_equal(new[:, :4], dets[inds, :4])
            if prm['method'] == 'gaussian':        # the fixture's own margin conditions
                assert info['min_gap_ulp'] > margin and info['min_thr_ulp'] > margin, (name, p, info['min_gap_ulp'], info['min_thr_ulp'])


def test_refs_multiclass_equals_reference_bit_for_bit():
    g = gold()
    thr = float(g['mc_score_thr'])
    for name in [str(n) for n in g['mc_names']]:
        boxes, scores = g['mc_%s_boxes' % name], g['mc_%s_scores' % name]
        for c in [str(c) for c in g['mc_cfg_names']]:
            cfg = dict(type='soft_nms', **params(g, 'mc_cfg_' + c))
            for mx in g['mc_max_nums'].tolist():
                tag = 'mc_%s_%s_%s' % (name, c, 'm1' if mx < 0 else str(mx))
                info = {}
                d, l = R.multiclass(boxes, scores, thr, cfg, mx, info=info)
                assert np.array_equal(l, g[tag + '_labels']) and np.array_equal(info['rows'], g[tag + '_rows']), tag
                assert np.array_equal(d[:, 4].view(np.int32), g[tag + '_scores'].view(np.int32)), tag
                assert np.array_equal(d[:, :4], boxes[g[tag + '_rows']]) and not info['cut_ties']
                assert d.shape[0] == (0 if name == 'none' else d.shape[0]) and (mx < 0 or d.shape[0] <= mx)


def test_refs_round_form_on_a_hand_case():
    """Three boxes, linear: the second overlaps the first at IoU 0.68 -> rescored 0.8 * (1 - IoU); min_score removes it when high."""
    dets = np.array([[0, 0, 99, 99, 0.9], [0, 0, 99, 67, 0.8], [200, 200, 299, 299, 0.7]], np.float32)
    new, inds = R.soft_nms(dets, 0.5, 'linear', min_score=0.05)
    assert inds.tolist() == [0, 2, 1] and abs(new[2, 4] - 0.8 * (1 - 0.68)) < 1e-6
    new, inds = R.soft_nms(dets, 0.5, 'linear', min_score=0.3)
    assert inds.tolist() == [0, 2]
    new, inds = R.soft_nms(dets, 0.7, 'linear', min_score=0.05)          # IoU below iou_thr: weight 1
    assert inds.tolist() == [0, 1, 2] and new[1, 4] == np.float32(0.8)
    with pytest.raises(ValueError, match='Invalid method for SoftNMS'):
        R.soft_nms(dets, 0.5, 'greedy')


def test_new_exports_are_declared_bound_and_present():
    header = open(os.path.join(ROOT, 'include', 'hvr_hip.h')).read()
    capi = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'capi.hip')).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\b%s\(' % sym, header), '%s is not declared in include/hvr_hip.h' % sym
        assert re.search(r'\b%s\(' % sym, capi), '%s is not defined in capi.hip' % sym
        assert sym in native.SYMBOLS, '%s is not bound in native.py' % sym
        assert hasattr(native.lib(), sym)
    assert native.ABI_VERSION == native.lib().hvr_abi_version() == 7          # 7: hvr_sample_pos_neg's neg_pos_ub is a double
    assert native.SYMBOLS['hvr_multiclass_nms'] == (native._i, [native._vp, native._vp, native._i, native._i, native._f, native._f, native._i,
                                                                native._vp, native._vp, native._vp, native._vp, native._sz, native._vp])
    assert hvrnet_amd.soft_nms is ops.soft_nms and callable(native.soft_nms) and callable(native.multiclass_soft_nms)


def test_workspace_sizes_cover_the_per_class_lists():
    lib = native.lib()
    for P, Rn, ncls in ((1, 300, 31), (4, 300, 31), (3, 512, 31), (1, 1, 2)):
        assert lib.hvr_multiclass_soft_nms_workspace_bytes(P, Rn, ncls) >= P * (ncls - 1) * (Rn * 8 + 4)
    assert lib.hvr_soft_nms_workspace_bytes(512) > 0


def test_argument_errors_of_the_public_surface():
    dets = torch.tensor([[0., 0., 9., 9., 0.5], [0., 0., 9., 9., 0.9]])
    with pytest.raises(NotImplementedError):
        ops.soft_nms(dets, 0.5)                                            # CPU tensors: no fallback, like ops.nms
    with pytest.raises(ValueError, match='Invalid method for SoftNMS: greedy'):
        ops.soft_nms(dets, 0.5, method='greedy')
    with pytest.raises(TypeError):
        ops.soft_nms(dets.numpy(), 0.5)
    boxes, scores = torch.zeros((4, 4)), torch.full((4, 3), 1 / 3)
    with pytest.raises(ValueError, match='Invalid method for SoftNMS'):
        box_ops.multiclass_nms(boxes, scores, 0.001, dict(type='soft_nms', iou_thr=0.5, method='hard'), 10)
    with pytest.raises(NotImplementedError, match='outside the HVR hot path'):
        box_ops.multiclass_nms(boxes, scores, 0.001, dict(type='matrix_nms', iou_thr=0.5), 10)
    with pytest.raises(NotImplementedError, match='outside the HVR hot path'):
        native.readout_nms(boxes, scores, 0.001, dict(type='matrix_nms', iou_thr=0.5), 10)


def test_softnms_source_is_plain_cpp():
    src = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'softnms.hip')).read()
    assert 'asm' not in src and '__builtin_amdgcn_s_' not in src          # ballots, shuffles and vector stores only
    from tests.test_host_logic import build_units, check_regs
    assert build_units()['softnms'] == {'nofma', 'remarks'}, 'softnms.hip must be built without contraction (the ua expression)'
    for kernel in ('_ZN3hvr21soft_nms_class_kernelEPKfilS1_iliiffiffPfPiS3_S2_PxS3_', '_ZN3hvr21soft_nms_merge_kernelEPKfiiS1_PKiS3_iiPfPxPi'):
        rule = check_regs().rule_for(kernel)                                # (row of the table, bytes of scratch allowed)
        assert rule is not None and rule[1] == 0, kernel
