"""Host-side checks of the Seq-NMS read-out (no GPU).  The reference tree has no Seq-NMS: the specification in DESIGN.md is the
contract, tests/seqnms_refs.py restates it twice (the plain dynamic programme and an exhaustive chain search that shares only the
IoU helper), and this file pins the restatement -- to the exhaustive search, to the recorded greedy keep lists on one frame, to hand
cases -- plus the C ABI bookkeeping of the new exports, the argument errors of the public surface and the window runner's hand-over."""
import os
import re

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import native, ops
from hvrnet_amd.config import selsa_config
from hvrnet_amd.window import VideoWindowRunner
from tests import seqnms_refs as R
from tests.golden import cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['hvr_seq_nms_workspace_bytes', 'hvr_seq_nms', 'hvr_seq_nms_phases']
F32 = np.float32


def gold(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


def same(a, b):
    (da, la, na), (db, lb, nb) = a, b
    return np.array_equal(na, nb) and np.array_equal(la, lb) and np.array_equal(da.view(np.int32), db.view(np.int32))


def test_plain_loop_equals_exhaustive_search_on_tiny_cases():
    ties = long_paths = 0
    for seed in range(240):
        boxes, scores, thr = R.tiny_case(seed)
        for rescore, link, nms in (('avg', 0.5, 0.3), ('max', 0.3, 0.5)):
            info = {}
            ref = R.seq_nms_ref(boxes, scores, thr, link, nms, 6, rescore, info=info)
            assert same(ref, R.seq_nms_exhaustive(boxes, scores, thr, link, nms, 6, rescore)), (seed, rescore)
            long_paths += info.get('long_paths', 0)
        flat = boxes.reshape(-1, 4)
        ties += len(np.unique(flat, axis=0)) < len(flat) and len(np.unique(scores[:, :, 1:])) < scores[:, :, 1:].size
    assert ties > 120 and long_paths > 200          # duplicated boxes, equal scores and real sequences are the common case here


def one_frame(dets, thr, max_num=None):
    dets = np.asarray(dets, F32)
    n = dets.shape[0]
    assert (dets[:, 4] > 0).all()
    scores = np.zeros((1, n, 2), F32)
    scores[0, :, 1] = dets[:, 4]
    d, l, k = R.seq_nms_ref(dets[None, :, :4], scores, 0.0, 0.5, thr, max_num or n, 'avg')
    return d[0, :k[0]], dets


def test_one_frame_is_greedy_nms_on_the_recorded_keep_lists():
    g = gold('g3_nms')
    for name, dets, thr in C.nms_cases():
        if dets.shape[0] > 512:
            continue
        out, dets = one_frame(dets.numpy(), thr)
        keep = np.sort(g[name + '_keep'])
        assert np.array_equal(out.view(np.int32), dets[keep].view(np.int32)), name      # class-major, ascending row; scores untouched
    g = gold('g17_nms_random')
    for seed in range(5):
        out, dets = one_frame(C.boxes(500, 4000 + seed).numpy(), 0.5)
        assert np.array_equal(out.view(np.int32), dets[np.sort(g['seed%d_keep' % seed])].view(np.int32)), seed


def test_hand_case_one_path_of_three():
    boxes = np.tile(np.array([10, 10, 50, 50], F32), (3, 1, 1))
    scores = np.zeros((3, 1, 2), F32)
    scores[:, 0, 1] = [0.9, 0.2, 0.7]
    info = {}
    d, l, n = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 4, 'avg', info=info)
    want = F32(F32(F32(0.9) + F32(F32(0.2) + F32(0.7))) / F32(3))
    assert n.tolist() == [1, 1, 1] and info['paths'] == info['long_paths'] == 1
    assert d[:, 0, 4].view(np.int32).tolist() == [want.view(np.int32)] * 3 and np.array_equal(d[:, 0, :4], boxes[:, 0])
    assert not d[:, 1:].any() and not l.any()
    d, l, n = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 4, 'max')
    assert d[:, 0, 4].view(np.int32).tolist() == [F32(0.9).view(np.int32)] * 3
    with pytest.raises(ValueError, match='Invalid rescore for Seq-NMS'):
        R.seq_nms_ref(boxes, scores, 0.05, rescore='mean')


def test_retirement_drops_overlaps_of_a_path_box_only_at_nms_thr():
    boxes = np.zeros((3, 2, 4), F32)
    boxes[:, 0] = [10, 10, 50, 50]
    boxes[:, 1] = [500, 500, 510, 510]              # far away, never a candidate in frames 0 and 2
    boxes[1, 1] = [10, 10, 50, 30]                  # IoU with the path box: 41 * 21 / (41 * 41) = 0.512
    scores = np.zeros((3, 2, 2), F32)
    scores[:, 0, 1] = [0.9, 0.2, 0.7]
    scores[1, 1, 1] = 0.1                           # weaker than the path box of its frame: the path goes through row 0
    iou = R.iou_plus1(boxes[1, :1], boxes[1, 1:])[0, 0]
    assert abs(iou - 21.0 / 41.0) < 1e-6
    d, l, n = R.seq_nms_ref(boxes, scores, 0.05, 0.6, 0.5, 4, 'avg')       # link 0.6: the weak box does not join a path
    assert n.tolist() == [1, 1, 1]                                          # dropped: IoU 0.512 >= 0.5
    d, l, n = R.seq_nms_ref(boxes, scores, 0.05, 0.6, 0.52, 4, 'avg')
    assert n.tolist() == [1, 2, 1]                                          # below nms_thr: survives, alone, with its own score
    assert d[1, 1, 4] == F32(0.1) and np.array_equal(d[1, 1, :4], boxes[1, 1])


def test_degenerate_boxes_terminate_and_are_kept_once():
    boxes, scores = R.degenerate_video()
    with np.errstate(invalid='ignore'):
        self_iou = np.diag(R.iou_plus1(boxes[0], boxes[0]))
    assert np.isnan(self_iou).any() and (self_iou[~np.isnan(self_iou)] != 1).any()      # self-overlap would not retire these
    for rescore in ('avg', 'max'):
        info = {}
        d, l, n = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 8, rescore, info=info)
        assert n.tolist() == [5, 5, 5]                                                   # every candidate exactly once
        keep = info['kept'][0][0]
        assert keep.all() and info['paths'] <= 15
        for t in range(3):
            assert np.array_equal(d[t, :5, :4].view(np.int32), boxes[t].view(np.int32))


def test_new_exports_are_declared_bound_and_present():
    header = open(os.path.join(ROOT, 'include', 'hvr_hip.h')).read()
    capi = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'capi.hip')).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\b%s\(' % sym, header), '%s is not declared in include/hvr_hip.h' % sym
        assert re.search(r'\b%s\(' % sym, capi), '%s is not defined in capi.hip' % sym
        assert sym in native.SYMBOLS, '%s is not bound in native.py' % sym
        assert hasattr(native.lib(), sym)
    assert native.ABI_VERSION == native.lib().hvr_abi_version()                # additions only
    assert native.SYMBOLS['hvr_seq_nms'] == (native._i, [native._vp, native._vp, native._i, native._i, native._i, native._f, native._f,
                                                         native._f, native._i, native._i, native._vp, native._vp, native._vp, native._vp,
                                                         native._sz, native._vp])
    assert hvrnet_amd.seq_nms is ops.seq_nms and callable(native.seq_nms)


def test_workspace_is_monotone_and_covers_the_tables():
    ws = native.lib().hvr_seq_nms_workspace_bytes
    assert ws(60, 300, 31) >= 2 * 60 * 300 * 5 * 8 + 30 * 60 * 300 * 10
    for F, Rn, ncls in ((1, 1, 2), (3, 64, 3), (60, 300, 31)):
        assert ws(F + 1, Rn, ncls) >= ws(F, Rn, ncls) and ws(F, Rn + 1, ncls) >= ws(F, Rn, ncls) and ws(F, Rn, ncls + 1) >= ws(F, Rn, ncls)
        assert F * Rn < 192 or ws(2 * F, Rn, ncls) > ws(F, Rn, ncls) and ws(F, Rn + 64, ncls) > ws(F, Rn, ncls) and ws(F, Rn, 2 * ncls) > ws(F, Rn, ncls)


def test_c_abi_refuses_what_is_outside_the_limits_before_any_launch():
    lib = native.lib()
    n = (native.ctypes.c_int32 * 4)()
    call = lambda F, Rn, ncls, thr=0.05, rescore=1, max_num=10: lib.hvr_seq_nms(None, None, F, Rn, ncls, thr, 0.5, 0.3, rescore, max_num, None, None,
                                                                               native.ctypes.cast(n, native._vp), None, 0, None)
    assert call(0, 8, 3) == -1 and call(2, 8, 3, rescore=3) == -1 and call(2, 8, 3, thr=-0.5) == -1 and call(2, 8, 3, max_num=0) == -1   # HVR_EINVAL
    assert call(2, 513, 3) == -2 and call(2, 8, 1) == -2 and call(2, 8, 200) == -2 and call(70000, 8, 3) == -2                           # HVR_EUNSUPPORTED
    assert call(2, 8, 3) == -1 and b'null pointer' in lib.hvr_last_error()


def test_argument_errors_of_the_public_surface():
    boxes, scores = torch.zeros((2, 4, 4)), torch.full((2, 4, 3), 0.3)
    with pytest.raises(NotImplementedError):
        ops.seq_nms(boxes, scores, 0.05)                                   # CPU tensors: no fallback, like every other op
    with pytest.raises(ValueError, match='Invalid rescore for Seq-NMS: mean'):
        ops.seq_nms(boxes, scores, 0.05, rescore='mean')
    with pytest.raises(TypeError):
        ops.seq_nms(boxes.numpy(), scores.numpy(), 0.05)

    class Model(object):
        test_cfg = selsa_config(frame_interval=1, nms_post=32).test_cfg

    assert VideoWindowRunner(Model(), 3).seq_nms is None                   # both configs: no key, nothing changes
    assert VideoWindowRunner(Model(), 3, seq_nms=dict(link_iou_thr=0.4)).seq_nms == dict(link_iou_thr=0.4)
    assert VideoWindowRunner(Model(), 3, seq_nms={}).seq_nms == {}          # an empty dict switches it ON, with the defaults
    with pytest.raises(ValueError, match='Invalid rescore'):
        VideoWindowRunner(Model(), 3, seq_nms=dict(rescore='mean'))
    with pytest.raises(ValueError, match='link_iou_thr and rescore'):
        VideoWindowRunner(Model(), 3, seq_nms=dict(iou_thr=0.5))
    Model.test_cfg.rcnn['seq_nms'] = dict(link_iou_thr=0.5, rescore='max')
    assert VideoWindowRunner(Model(), 3).seq_nms == dict(link_iou_thr=0.5, rescore='max')       # the config key is the default
    Model.test_cfg.rcnn.nms['type'] = 'soft_nms'
    with pytest.raises(ValueError, match="nms type must be 'nms'"):
        VideoWindowRunner(Model(), 3)
    runner = VideoWindowRunner(type('M', (), {})(), 3, seq_nms=dict(rescore='avg'))
    with pytest.raises(NotImplementedError, match='test-time-augmentation'):
        runner.step([0, 1], [None, None], 0, 0)


class _Ids(object):
    """id-only model, as window.window_frames uses: frames are integers, a window's 'read-out' is its deque content."""
    frame_tensors = None

    def __init__(self):
        self.calls, self.raw_flags = [], []

    def __call__(self, **kw):
        if kw.get('backbone_feat'):
            return [kw['img']]
        self.raw_flags.append(kw.get('raw', False))
        return list(kw['x'])

    def seq_nms_video(self, raws, **kw):
        self.calls.append((list(raws), kw))
        return [('post', r) for r in raws]


@pytest.mark.parametrize('frames,window', [(1, 3), (2, 3), (5, 3), (9, 5), (4, 7)])
def test_runner_hands_the_whole_video_to_the_post_processor_once(frames, window):
    from hvrnet_amd.window import window_frames
    model = _Ids()
    out = VideoWindowRunner(model, window, seq_nms=dict(link_iou_thr=0.4, rescore='max')).run_video(range(frames), [None] * frames)
    want = window_frames(frames, window)
    assert len(model.calls) == 1 and model.calls[0][1] == dict(link_iou_thr=0.4, rescore='max')
    assert model.calls[0][0] == [want[o] for o in range(frames)]           # one entry per video frame, in frame order
    assert out == {o: ('post', want[o]) for o in range(frames)} and all(model.raw_flags)
    plain = _Ids()
    assert VideoWindowRunner(plain, window).run_video(range(frames), [None] * frames) == want and not plain.calls and not any(plain.raw_flags)


def test_raw_read_out_of_a_window_with_a_short_frame_takes_the_exact_path():
    from hvrnet_amd.detectors import _WindowDetector, _pad_rows
    short = _WindowDetector._raw_readout(None, None, None, None, None, False, torch.tensor([32, 31, 32], dtype=torch.int32), 32, lambda: 'exact')
    assert short == 'exact'

    class Head(object):
        def get_det_bboxes(self, rois, cls_score, bbox_pred, img_shape, scale_factor, rescale=False, cfg=None):
            assert cfg is None
            return (torch.zeros((2, 4)), torch.ones((2, 3))) if cls_score is None else ([torch.zeros((2, 4))] * 2, [torch.ones((2, 3))] * 2)

    det = type('D', (), dict(bbox_head=Head()))()
    meta = dict(img_shape=(4, 4, 3), scale_factor=1.0)
    full = torch.tensor([32, 32, 32], dtype=torch.int32)
    one = _WindowDetector._raw_readout(det, None, None, None, meta, False, full, 32, None)               # one branch: a bare pair from the head
    two = _WindowDetector._raw_readout(det, None, [0, 0], [0, 0], meta, False, None, None, None)       # two branches: lists from the head
    assert [len(one), len(two)] == [1, 2] and all(b.shape == (2, 4) and s.shape == (2, 3) for b, s in one + two)
    x = torch.ones((3, 5))
    assert _pad_rows(x, 3) is x and _pad_rows(x, 6).shape == (6, 5) and not _pad_rows(x, 6)[3:].any()
    with pytest.raises(ValueError, match='nms_post'):
        _pad_rows(x, 2)


def test_seqnms_source_is_plain_cpp_and_registered():
    src = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'seqnms.hip')).read()
    assert 'asm' not in src and '__builtin_amdgcn_s_' not in src          # ballots, shuffles and vector stores only
    from tests.test_host_logic import build_units, check_regs
    assert build_units()['seqnms'] == {'nofma', 'remarks'}                 # no contraction (w * h in the union), remarks kept
    for kernel in ('_ZN3hvr19seq_nms_link_kernelEPK15HIP_vector_typeIfLj4EEPKiiiiiffPyS6_', '_ZN3hvr19seq_nms_path_kernelEPKfPKiiiiifiPKyS5_PfPsS6_PyS8_S8_P15HIP_vector_typeIiLj2EEPi',
                   '_ZN3hvr26seq_nms_tube_prefix_kernelEPKiiiPiS2_', '_ZN3hvr20seq_nms_merge_kernelEPKfiiiiS1_PKyiiPfPxPiPKiiPK15HIP_vector_typeIiLj2EES8_S8_S6_PS9_IiLj4EES4_i'):
        rule = check_regs().rule_for(kernel)                                # (row of the table, bytes of scratch allowed)
        assert rule is not None and rule[1] == 0, kernel
