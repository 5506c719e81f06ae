"""Host-side checks of the batched Seq-NMS read-out with tube outputs (no GPU).  tests/seqnms_tube_refs.py restates
8d + 8e as a plain loop that records its paths; this file pins that restatement -- to seq_nms_ref (tests/seqnms_refs.py, unchanged)
on the per-frame lists, to the tube invariants, to the chains of the exhaustive search, to the problem boundary -- plus the C ABI
bookkeeping of the new exports and the argument errors of the new Python surface.  Every comparison is exact."""
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
from tests import seqnms_tube_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['hvr_seq_nms_batched_workspace_bytes', 'hvr_seq_nms_batched']
F32 = np.float32


def same3(a, b):
    (da, la, na), (db, lb, nb) = a[:3], b[:3]
    return np.array_equal(na, nb) and np.array_equal(la, lb) and np.array_equal(da.view(np.int32), db.view(np.int32))


def inputs():
    """(name, boxes, scores, score_thr, max_num, settings): the tiny cases, the tracks-plus-clutter video and the quantised video."""
    for seed in range(200):
        b, s, thr = R.tiny_case(seed)
        yield 'tiny%d' % seed, b, s, thr, 6, (('avg', 0.5, 0.3), ('max', 0.3, 0.5))
    b, s = R.video(7, 17, 130, 4)
    yield 'video', b, s, 0.05, 130, (('avg', 0.5, 0.3),)
    b, s = R.quantised_video(11, 5, 65, 3)
    yield 'quantised', b, s, 0.1, 65, (('avg', 0.5, 0.3), ('max', 0.5, 0.5))


def check_tube_invariants(boxes, scores, score_thr, link, nms, rescore, out, info, what):
    """one problem, max_num not cutting: every kept (class, frame, row) in exactly one tube, members in consecutive frames linked at
    IoU >= link, table rows follow the rule, ids dense and class-major."""
    dets, labels, n, ids, tubes, tsc, start = out
    paths = info['paths'][0]
    assert start.tolist() == [0, sum(len(p) for p in paths)] and len(tubes) == start[1], what
    k = 0
    seen = set()
    for c, cls_paths in enumerate(paths):                      # ids dense, class-major, selection order within a class
        for t0, rows, val in cls_paths:
            assert tubes[k].tolist() == [0, c, t0, len(rows)] and tsc[k].view(np.int32) == F32(val).view(np.int32), (what, k)
            for d, r in enumerate(rows):
                assert (c, t0 + d, r) not in seen and scores[t0 + d, r, c + 1] > F32(score_thr), (what, k)
                seen.add((c, t0 + d, r))
                if d:
                    iou = R.iou_plus1(boxes[t0 + d - 1, rows[d - 1]][None], boxes[t0 + d, r][None])[0, 0]
                    assert iou >= F32(link), (what, k)
            if rescore == 'max':
                assert val == max(scores[t0 + d, r, c + 1] for d, r in enumerate(rows)), (what, k)
            else:                                              # the root's sum: one f32 add per frame, backward in time; one f32 division
                acc = F32(0)
                for d in range(len(rows) - 1, -1, -1):
                    acc = F32(scores[t0 + d, rows[d], c + 1] + acc)
                assert F32(val).view(np.int32) == F32(acc / F32(len(rows))).view(np.int32), (what, k)
            k += 1
    # the output rows: each carries the id of the tube that holds its (class, frame, row), with the tube's score
    rows_out = 0
    for t in range(boxes.shape[0]):
        assert (ids[t, n[t]:] == -1).all() and (ids[t, :n[t]] >= 0).all(), (what, t)
        for q in range(n[t]):
            i = ids[t, q]
            p, c, t0, ln = tubes[i]
            assert c == labels[t, q] and t0 <= t < t0 + ln and dets[t, q, 4].view(np.int32) == tsc[i].view(np.int32), (what, t, q)
            r = paths[c][i - sum(len(pp) for pp in paths[:c])][1][t - t0]
            assert np.array_equal(dets[t, q, :4], boxes[t, r]), (what, t, q)
            rows_out += 1
    assert rows_out == len(seen), what                         # exactly one tube per kept box, no kept box without one
    return len(tubes), int((tubes[:, 3] > 1).sum())


def test_restatement_equals_seq_nms_ref_and_tube_invariants_hold():
    n_tubes = n_long = 0
    for name, boxes, scores, thr, max_num, settings in inputs():
        for rescore, link, nms in settings:
            info = {}
            out = T.seq_nms_tubes_ref(boxes, scores, [boxes.shape[0]], thr, link, nms, max_num, rescore, info=info)
            assert same3(out, R.seq_nms_ref(boxes, scores, thr, link, nms, max_num, rescore)), (name, rescore)
            if name.startswith('tiny'):
                full = T.seq_nms_tubes_ref(boxes, scores, [boxes.shape[0]], thr, link, nms, 2 * boxes.shape[1], rescore, info={})
                a, b = check_tube_invariants(boxes, scores, thr, link, nms, rescore, full, info, name)
            else:
                a, b = check_tube_invariants(boxes, scores, thr, link, nms, rescore, out, info, name)
            n_tubes, n_long = n_tubes + a, n_long + b
    assert n_long > 200 and n_tubes > n_long


def test_per_problem_results_equal_seq_nms_ref_on_the_slices():
    boxes, scores = R.video(7, 17, 130, 4)
    counts = [5, 1, 11]
    out = T.seq_nms_tubes_ref(boxes, scores, counts, 0.05, 0.5, 0.3, 130, 'avg')
    f0 = 0
    for p, Fn in enumerate(counts):
        ref = R.seq_nms_ref(boxes[f0:f0 + Fn], scores[f0:f0 + Fn], 0.05, 0.5, 0.3, 130, 'avg')
        assert same3([o[f0:f0 + Fn] for o in out[:3]], ref), p
        rows = out[4][out[6][p]:out[6][p + 1]]
        assert (rows[:, 0] == p).all() and (rows[:, 2] + rows[:, 3] <= Fn).all() and (rows[:, 2] >= 0).all()
        assert out[3][f0:f0 + Fn].max() == len(rows) - 1                       # ids are problem-local and dense (max_num = R cuts nothing)
        f0 += Fn
    assert out[6][-1] == len(out[4]) == len(out[5])


def test_tubes_equal_the_chains_of_the_exhaustive_search():
    long_paths = 0
    for seed in range(200):
        boxes, scores, thr = R.tiny_case(seed)
        for rescore, link, nms in (('avg', 0.5, 0.3), ('max', 0.3, 0.5)):
            info = {}
            T.seq_nms_tubes_ref(boxes, scores, [boxes.shape[0]], thr, link, nms, 6, rescore, info=info)
            want = T.exhaustive_chains(boxes, scores, thr, link, nms, rescore)
            got = info['paths'][0]
            assert len(got) == len(want) == 2
            for g, w in zip(got, want):
                assert [(t0, rows) for t0, rows, _ in g] == [(t0, rows) for t0, rows, _ in w], (seed, rescore)
                assert [v.view(np.int32) for _, _, v in g] == [v.view(np.int32) for _, _, v in w], (seed, rescore)
                long_paths += sum(len(rows) > 1 for _, rows, _ in g)
    assert long_paths > 200


def boundary_case():
    """One frame of three boxes (two overlapping, one apart), twice: identical boxes in both frames link at any threshold."""
    frame = np.array([[10, 10, 50, 50], [12, 12, 52, 52], [200, 200, 240, 240]], F32)
    scores = np.zeros((1, 3, 2), F32)
    scores[0, :, 1] = [0.9, 0.6, 0.5]
    return np.stack([frame, frame]), np.concatenate([scores, scores])


def test_problem_boundary_two_one_frame_problems_against_one_two_frame_problem():
    boxes, scores = boundary_case()
    split = T.seq_nms_tubes_ref(boxes, scores, [1, 1], 0.05, 0.5, 0.3, 4, 'avg')
    greedy = R.seq_nms_ref(boxes[:1], scores[:1], 0.05, 0.5, 0.3, 4, 'avg')          # one frame: per-class greedy NMS
    assert greedy[2].tolist() == [2]
    for p in range(2):
        assert same3([o[p:p + 1] for o in split[:3]], greedy)
    assert split[6].tolist() == [0, 2, 4] and (split[4][:, 3] == 1).all() and split[4][:, 0].tolist() == [0, 0, 1, 1]
    assert split[3][:, :2].tolist() == [[0, 1], [0, 1]] and split[5].tolist() == [F32(0.9), F32(0.5), F32(0.9), F32(0.5)]
    joined = T.seq_nms_tubes_ref(boxes, scores, [2], 0.05, 0.5, 0.3, 4, 'avg')
    assert joined[6].tolist() == [0, 2] and joined[4].tolist() == [[0, 0, 0, 2], [0, 0, 0, 2]]          # two linked tubes of two boxes
    assert joined[3][:, :2].tolist() == [[0, 1], [0, 1]]
    assert not np.array_equal(joined[4], split[4][:2])                                 # the two readings are told apart


def test_max_num_cut_keeps_the_length_and_max_tubes_caps_the_table():
    boxes, scores = R.video(31, 4, 96, 3, clutter=0.9)
    full = T.seq_nms_tubes_ref(boxes, scores, [4], 0.05, 0.5, 0.3, 96, 'avg')
    cut = T.seq_nms_tubes_ref(boxes, scores, [4], 0.05, 0.5, 0.3, 8, 'avg')
    assert cut[2].tolist() == [8] * 4 and full[2].min() > 8
    assert np.array_equal(cut[4], full[4]) and np.array_equal(cut[5], full[5]) and np.array_equal(cut[6], full[6])   # the table ignores the cut
    assert (cut[3][:, :8] >= 0).all() and set(cut[3].ravel().tolist()) < set(full[3].ravel().tolist())
    total = int(full[6][-1])
    capped = T.seq_nms_tubes_ref(boxes, scores, [4], 0.05, 0.5, 0.3, 96, 'avg', max_tubes=total - 5, fill=(-7, -7.0))
    assert np.array_equal(capped[4], full[4][:total - 5]) and capped[6].tolist() == full[6].tolist() and np.array_equal(capped[3], full[3])
    roomy = T.seq_nms_tubes_ref(boxes, scores, [4], 0.05, 0.5, 0.3, 96, 'avg', max_tubes=total + 3, fill=(-7, -7.0))
    assert (roomy[4][total:] == -7).all() and (roomy[5][total:] == F32(-7)).all() and np.array_equal(roomy[4][:total], full[4])


def test_new_exports_are_declared_bound_and_present():
    header = open(os.path.join(ROOT, 'include', 'hvr_hip.h')).read()
    capi = open(os.path.join(ROOT, 'hvrnet_amd', 'csrc', 'capi.hip')).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\b%s\(' % sym, header), '%s is not declared in include/hvr_hip.h' % sym
        assert re.search(r'\b%s\(' % sym, capi), '%s is not defined in capi.hip' % sym
        assert sym in native.SYMBOLS, '%s is not bound in native.py' % sym
        assert hasattr(native.lib(), sym)
    assert native.ABI_VERSION == native.lib().hvr_abi_version() == 7           # 7: hvr_sample_pos_neg's neg_pos_ub is a double
    assert callable(native.seq_nms_batched) and hvrnet_amd.seq_nms is ops.seq_nms
    ws, wsb = native.lib().hvr_seq_nms_workspace_bytes, native.lib().hvr_seq_nms_batched_workspace_bytes
    assert wsb(1, 60, 300, 31, 0) == ws(60, 300, 31)                           # the P = 1, no-tubes case is today's call
    assert wsb(4, 60, 300, 31, 1) >= ws(60, 300, 31) + 30 * 60 * 300 * 8 + 2 * 4 * 30 * 4
    assert wsb(8, 60, 300, 31, 1) >= wsb(4, 60, 300, 31, 1) >= wsb(4, 60, 300, 31, 0)


def test_c_abi_refuses_what_is_outside_the_limits_before_any_launch():
    lib = native.lib()
    ct = native.ctypes
    n = (ct.c_int32 * 8)()
    np_ = ct.cast(n, native._vp)
    some = ct.cast((ct.c_int32 * 8)(), native._vp)

    def call(P, F, Rn, ncls, thr=0.05, rescore=1, max_num=10, tube=(None, None, None, None), max_tubes=0, n_out=np_):
        return lib.hvr_seq_nms_batched(None, None, P, None, F, Rn, ncls, thr, 0.5, 0.3, rescore, max_num, None, None, n_out, tube[0], tube[1],
                                       tube[2], tube[3], max_tubes, None, 0, None)
    EINVAL, EUNSUPPORTED = -1, -2
    assert call(0, 4, 8, 3) == EINVAL and call(3, 2, 8, 3) == EINVAL                      # P >= 1, Ftot >= P
    assert call(1, 0, 8, 3) == EINVAL and call(2, 4, 8, 3, rescore=3) == EINVAL and call(2, 4, 8, 3, thr=-0.5) == EINVAL
    assert call(2, 4, 8, 3, max_num=0) == EINVAL and call(2, 4, 8, 3, n_out=None) == EINVAL
    assert call(2, 4, 513, 3) == EUNSUPPORTED and call(2, 4, 8, 1) == EUNSUPPORTED and call(2, 4, 8, 200) == EUNSUPPORTED
    assert call(2, 70000, 8, 3) == EUNSUPPORTED
    for k in range(1, 4):                                                                  # any mix of NULL and non-NULL tube pointers
        assert call(2, 4, 8, 3, tube=(some,) * k + (None,) * (4 - k)) == EINVAL and b'tube outputs' in lib.hvr_last_error()
        assert call(2, 4, 8, 3, tube=(None,) * k + (some,) * (4 - k)) == EINVAL
    assert call(2, 4, 8, 3, tube=(some,) * 4, max_tubes=-1) == EINVAL and b'max_tubes' in lib.hvr_last_error()
    assert call(2, 4, 8, 3) == EINVAL and b'null pointer' in lib.hvr_last_error()          # within the limits: stopped at the NULL buffers
    assert call(2, 4, 8, 3, tube=(some,) * 4, max_tubes=5) == EINVAL and b'null pointer' in lib.hvr_last_error()


def test_argument_errors_of_the_python_surface():
    boxes, scores = torch.zeros((4, 4, 4)), torch.full((4, 4, 3), 0.3)
    with pytest.raises(NotImplementedError):
        ops.seq_nms(boxes, scores, 0.05, frame_counts=[2, 2], tubes=True)      # CPU tensors: no fallback, like every other op
    with pytest.raises(NotImplementedError):
        native.seq_nms_batched(boxes, scores, [2, 2], 0.05)
    with pytest.raises(TypeError):
        ops.seq_nms(boxes, scores, 0.05, 0.5, 0.3, 300, 'avg', [2, 2])          # frame_counts and tubes are keyword-only
    with pytest.raises(ValueError, match='Invalid rescore for Seq-NMS: mean'):
        native.seq_nms_batched(boxes, scores, [4], 0.05, rescore='mean')
    for bad in ([2, 1], [4, 0], [5, -1], [], [2, 2, 1], 4):
        with pytest.raises(ValueError, match='frame_counts'):
            native._frame_start(bad, 4, 'cpu')
    counts, starts = native._frame_start([1, 2, 1], 4, 'cpu')
    assert counts == (1, 2, 1) and starts.tolist() == [0, 1, 3, 4] and starts.dtype == torch.int32
    assert native._frame_start((1, 2, 1), 4, 'cpu')[1] is starts               # built once per (device, counts)

    class Model(object):
        test_cfg = selsa_config(frame_interval=1, nms_post=32).test_cfg

    assert VideoWindowRunner(Model(), 3, seq_nms=dict(tubes=True)).seq_nms == dict(tubes=True)
    assert VideoWindowRunner(Model(), 3, seq_nms=dict(tubes=True))._seq_nms_args() == (True, dict(tubes=True))
    assert VideoWindowRunner(Model(), 3, seq_nms=dict(rescore='max', tubes=False))._seq_nms_args() == (False, dict(rescore='max'))
    with pytest.raises(ValueError, match='link_iou_thr and rescore'):
        VideoWindowRunner(Model(), 3, seq_nms=dict(tube=True))
    Model.test_cfg.rcnn['seq_nms'] = dict(link_iou_thr=0.5, tubes=True)         # the config key takes it too
    assert VideoWindowRunner(Model(), 3).seq_nms == dict(link_iou_thr=0.5, tubes=True)
    runner = VideoWindowRunner(type('M', (), {})(), 3, seq_nms=dict(tubes=True))
    with pytest.raises(NotImplementedError, match='test-time-augmentation'):
        runner.step([0, 1], [None, None], 0, 0)


class _Ids(object):
    """id-only model (as tests/test_seqnms_host.py): frames are integers, a window's 'read-out' is its deque content."""
    frame_tensors = None

    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        return [kw['img']] if kw.get('backbone_feat') else list(kw['x'])

    def seq_nms_video(self, raws, **kw):
        self.calls.append(('video', [list(raws)], kw))
        res = [('post', r) for r in raws]
        return (res, ('tubes', kw['frame_offsets'])) if kw.get('tubes') else res

    def seq_nms_videos(self, videos, **kw):
        self.calls.append(('videos', [list(v) for v in videos], kw))
        res = [[('post', r) for r in v] for v in videos]
        return (res, [('tubes', o) for o in kw['frame_offsets']]) if kw.get('tubes') else res


def test_runner_passes_tubes_on_and_batches_the_videos_once():
    from hvrnet_amd.window import window_frames
    model = _Ids()
    runner = VideoWindowRunner(model, 3, seq_nms=dict(link_iou_thr=0.4, tubes=True))
    out = runner.run_video(range(5), [None] * 5)
    want5, want3 = window_frames(5, 3), window_frames(3, 3)
    assert out == {o: ('post', want5[o]) for o in range(5)} and runner.tubes == ('tubes', list(range(5)))
    assert model.calls == [('video', [[want5[o] for o in range(5)]], dict(link_iou_thr=0.4, tubes=True, frame_offsets=list(range(5))))]
    model.calls = []
    outs = runner.run_videos([range(5), range(3)], [[None] * 5, [None] * 3])
    assert len(model.calls) == 1 and model.calls[0][0] == 'videos'            # ONE post-processing call for both videos
    assert model.calls[0][1] == [[want5[o] for o in range(5)], [want3[o] for o in range(3)]]
    assert outs == [{o: ('post', want5[o]) for o in range(5)}, {o: ('post', want3[o]) for o in range(3)}]
    assert runner.tubes == [('tubes', list(range(5))), ('tubes', list(range(3)))]
    plain = _Ids()
    outs = VideoWindowRunner(plain, 3, seq_nms=dict(rescore='max')).run_videos([range(5), range(3)], [[None] * 5, [None] * 3])
    assert plain.calls[0][2] == dict(rescore='max') and [sorted(o) for o in outs] == [list(range(5)), list(range(3))]
    off = _Ids()
    assert VideoWindowRunner(off, 3).run_videos([range(5), range(3)], [[None] * 5, [None] * 3]) == [want5, want3] and not off.calls
