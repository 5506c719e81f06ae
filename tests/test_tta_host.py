"""Host-side checks of the test-time-augmentation path (no GPU): the plain-torch restatement tests/tta_refs.py is pinned to the
reference's recorded outputs bit for bit, FrameIngestAug's metas / order, the forward dispatch on nested metas, and the C ABI
bookkeeping of the new exports."""
import os
import re

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import native
from hvrnet_amd.detectors import BaseDetector
from hvrnet_amd.pipelines import FrameIngest, FrameIngestAug, rescale_size
from hvrnet_amd.window import FIRST, VideoWindowRunner
from tests import tta_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['hvr_ingest_frame_flip', 'hvr_merge_aug_proposals_workspace_bytes', 'hvr_merge_aug_proposals', 'hvr_map_aug_rois',
               'hvr_merge_aug_dets']


def gold(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


def _metas(g, prefix):
    return [dict(img_shape=(int(h), int(w), 3), scale_factor=float(s), flip=bool(f))
            for h, w, s, f in zip(g[prefix + '_img_h'], g[prefix + '_img_w'], g[prefix + '_scale'], g[prefix + '_flip'])]


def test_refs_box_mappings_equal_reference_bit_for_bit():
    g = gold('g18_merge_augs')
    b = torch.as_tensor(g['tr_boxes'])
    shape, s = tuple(int(v) for v in g['tr_img_shape']), float(g['tr_scale'])
    assert np.array_equal(R.bbox_flip(b, shape).numpy(), g['tr_flip'])
    assert np.array_equal(R.bbox_flip(b.reshape(32, 8), shape).numpy(), g['tr_flip8'])
    assert np.array_equal(R.bbox_mapping(b, shape, s, False).numpy(), g['tr_map'])
    assert np.array_equal(R.bbox_mapping(b, shape, s, True).numpy(), g['tr_map_flip'])
    assert np.array_equal(R.bbox_mapping_back(b, shape, s, False).numpy(), g['tr_back'])
    assert np.array_equal(R.bbox_mapping_back(b, shape, s, True).numpy(), g['tr_back_flip'])


def test_refs_merge_aug_proposals_equal_reference_bit_for_bit():
    g = gold('g18_merge_augs')
    thr = float(g['mp_nms_thr'])
    names = [str(n) for n in g['mp_names']]
    assert names == ['a2_300', 'a4_300', 'a2_32', 'a4_32', 'a4_300_short']
    for name in names:
        metas = _metas(g, 'mp_' + name)
        props = [torch.as_tensor(g['mp_%s_props_%d' % (name, a)]) for a in range(len(metas))]
        max_num = int(g['mp_%s_max_num' % name])
        merged, src = R.merge_aug_proposals(props, metas, thr, max_num, return_index=True)
        assert np.array_equal(merged.numpy(), g['mp_%s_merged' % name]) and np.array_equal(src.numpy(), g['mp_%s_src' % name])
        # the fixture's own conditions: the case is decided by arithmetic, and the generator rebuilds it from its seed
        assert R.margins_ok(props, metas, thr, max_num)
        scales = sorted({m['scale_factor'] for m in metas}, reverse=True)
        short = (2, 187) if name.endswith('short') else None
        again = R.random_aug_proposals(int(g['mp_%s_seed' % name]), R.aug_metas((600, 1000), scales, True), max(p.shape[0] for p in props), short=short)
        assert all(torch.equal(a, b) for a, b in zip(again, props))
    assert _metas(g, 'mp_a4_300_short')[2]['scale_factor'] == 0.8 and g['mp_a4_300_short_props_2'].shape[0] == 187


def test_refs_merge_aug_bboxes_equal_reference_bit_for_bit():
    g = gold('g18_merge_augs')
    for name in ('a4', 'a2'):
        metas = _metas(g, 'mb_' + name)
        boxes = [torch.as_tensor(b) for b in g['mb_%s_boxes' % name]]
        scores = [torch.as_tensor(s) for s in g['mb_%s_scores' % name]]
        assert scores[0].shape[1] == 31
        mb, ms = R.merge_aug_bboxes(boxes, scores, [[m] for m in metas])
        assert np.array_equal(mb.numpy(), g['mb_%s_merged_boxes' % name]) and np.array_equal(ms.numpy(), g['mb_%s_merged_scores' % name])
        assert np.array_equal(R.merge_aug_scores(scores).numpy(), g['mb_%s_merged_scores_only' % name])


def test_refs_nms_keeps_ge_semantics_and_index_order():
    dets = torch.tensor([[0., 0., 9., 9., 0.5], [0., 0., 9., 9., 0.9], [20., 20., 29., 29., 0.7], [0., 0., 9., 19., 0.6]])
    assert R.nms(dets, 0.5).tolist() == [1, 2]          # IoU(1, 3) = 100 / 200 = 0.5 is suppressed: >=
    assert R.nms(dets, 0.500001).tolist() == [1, 2, 3]


def test_frame_ingest_aug_metas_order_and_sizes():
    aug = FrameIngestAug(img_scale=[(1000, 600), (800, 480)], flip=True, device='cpu')
    metas = aug.metas(720, 1280)
    assert [(m['flip']) for m in metas] == [False, True, False, True]                    # scale outer, flip inner
    for m, scale in zip(metas, [(1000, 600), (1000, 600), (800, 480), (800, 480)]):
        nh, nw, f = rescale_size(720, 1280, scale)
        assert m['img_shape'] == (nh, nw, 3) and m['scale_factor'] == f and m['ori_shape'] == (720, 1280, 3)
        assert m['pad_shape'] == (-(-nh // 16) * 16, -(-nw // 16) * 16, 3)
    assert [m['img_shape'][:2] for m in metas] == [(563, 1000), (563, 1000), (450, 800), (450, 800)]
    one = FrameIngestAug(img_scale=(1000, 600), flip=False, device='cpu')
    assert len(one.ingests) == 1 and one.metas(600, 1000)[0]['flip'] is False
    assert FrameIngest(device='cpu').meta(600, 1000)['flip'] is False and FrameIngest(flip=True, device='cpu').meta(600, 1000)['flip'] is True
    assert [m['scale_factor'] for m in FrameIngestAug(img_scale=[(1000, 600), (800, 480)], device='cpu').metas(600, 1000)] == [1.0, 0.8]


class _Recorder(BaseDetector):
    def forward_feat(self, **kw):
        return ('plain', kw)

    def forward_feat_aug(self, **kw):
        return ('aug', kw)


def test_forward_dispatches_nested_metas_to_forward_feat_aug():
    det = _Recorder()
    flat = [dict(flip=False)] * 3
    nested = [[dict(flip=False), dict(flip=True)]] * 3
    kind, kw = det(img=None, img_meta=flat, forward_feat=True, return_loss=False, x=[1, 2, 3], rescale=True)
    assert kind == 'plain' and kw['img_meta'] is flat
    kind, kw = det(img=None, img_meta=nested, forward_feat=True, return_loss=False, x=[[1, 2]] * 3, rescale=True)
    assert kind == 'aug' and kw['img_meta'] is nested and kw['rescale'] is True and kw['x'] == [[1, 2]] * 3
    for cls in (hvrnet_amd.HNMBRCNN, hvrnet_amd.SelsaRCNN):
        for name in ('forward_feat_aug', 'aug_test_rpn_merged', 'aug_test_bboxes'):
            assert callable(getattr(cls, name))


def test_window_runner_aug_form_needs_cache_frames_off():
    class _Model(object):
        def __call__(self, **kw):
            assert kw.get('backbone_feat') and isinstance(kw['img'], list) and len(kw['img']) == len(kw['img_meta'])
            return [(im,) for im in kw['img']]

        frame_tensors = None

    imgs, metas = ['a0', 'a1'], [dict(flip=False), dict(flip=True)]
    with pytest.raises(NotImplementedError):
        VideoWindowRunner(_Model(), 3, cache_frames=True).step(imgs, metas, FIRST, 0)
    runner = VideoWindowRunner(_Model(), 3)
    assert runner.step(imgs, metas, FIRST, 0) == []
    assert list(runner.feats) == [['a0', 'a1']] * 2 and list(runner.metas) == [metas] * 2


def test_new_exports_are_declared_bound_and_present():
    header = open(os.path.join(ROOT, 'include', 'hvr_hip.h')).read()
    capi = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'capi.hip')).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\b%s\(' % sym, header), '%s is not declared in include/hvr_hip.h' % sym
        assert re.search(r'\b%s\(' % sym, capi), '%s is not defined in capi.hip' % sym
        assert sym in native.SYMBOLS, '%s is not bound in native.py' % sym
        assert hasattr(native.lib(), sym)
    assert native.ABI_VERSION == native.lib().hvr_abi_version() == 7          # 7: hvr_sample_pos_neg's neg_pos_ub is a double
    assert native.SYMBOLS['hvr_ingest_frame'] == (native._i, [native._vp, native._i, native._i, native._i64, native._vp, native._i, native._i,
                                                              native._i, native._i, native._vp, native._vp, native._i, native._vp])
    for name in ('bbox_flip', 'bbox_mapping', 'bbox_mapping_back', 'merge_aug_proposals', 'merge_aug_bboxes', 'merge_aug_scores',
                 'FrameIngestAug'):
        assert hasattr(hvrnet_amd, name)


def test_tta_sources_use_no_scalar_memory_writes():
    src = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'tta.hip')).read()
    assert 'asm' not in src and '__builtin_amdgcn_s_' not in src          # plain C++ and vector stores only
