"""Seq-NMS read-out on the GPU (hvrnet_amd/csrc/seqnms.hip) against the host restatement of its specification
(tests/seqnms_refs.py: seq_nms_ref, the plain loop).  The specification is bit-reproducible by construction -- one f32 add per frame,
an exact max, one f32 division -- so every comparison is exact: counts and labels equal, boxes and scores equal bit for bit.  There is
no tolerance anywhere in this file.  Nothing here reads the reference tree."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import graphs, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config, selsa_config  # noqa: E402
from hvrnet_amd.window import VideoWindowRunner, window_frames  # noqa: E402
from tests import seqnms_refs as R  # noqa: E402

DEV = 'cuda:0'
F32 = np.float32


def device(boxes, scores, *a, **kw):
    out = native.seq_nms(torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV), *a, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(boxes, scores, score_thr, link_thr, nms_thr, max_num, rescore, what, info=None):
    """device == seq_nms_ref: n and labels exact, dets bit for bit (the zero rows behind n included).  -> the reference's triple."""
    want = R.seq_nms_ref(boxes, scores, score_thr, link_thr, nms_thr, max_num, rescore, info=info)
    got = device(boxes, scores, score_thr, link_thr, nms_thr, max_num, rescore)
    assert got[2].dtype == np.int32 and got[1].dtype == np.int64 and got[0].shape == want[0].shape
    assert np.array_equal(got[2], want[2]), '%s: counts %s, expected %s' % (what, got[2].tolist(), want[2].tolist())
    assert np.array_equal(got[1], want[1]), '%s: labels differ' % what
    bad = got[0].view(np.int32) != want[0].view(np.int32)
    assert not bad.any(), '%s: %d det values differ bit-wise, first at %s' % (what, int(bad.sum()), np.argwhere(bad)[0].tolist())
    return want


@pytest.mark.parametrize('Rn', [1, 63, 64, 65, 130])
def test_lane_and_word_boundaries(Rn):
    boxes, scores = R.video(100 + Rn, 3, Rn, 3, tracks=min(3, max(Rn // 3, 1)), pad=0 if Rn < 4 else 2)
    info = {}
    want = check(boxes, scores, 0.05, 0.5, 0.3, Rn, 'avg', 'R=%d' % Rn, info)
    assert want[2].sum() > 0 and (Rn < 63 or info['long_paths'] > 0)
    check(boxes, scores, 0.05, 0.5, 0.3, Rn, 'max', 'R=%d max' % Rn)


@pytest.fixture(scope='module')
def tracks():
    return R.video(7, 17, 130, 4)


@pytest.mark.parametrize('thr', [(0.5, 0.3), (0.3, 0.5)], ids=['link5_nms3', 'link3_nms5'])
@pytest.mark.parametrize('rescore', ['avg', 'max'])
def test_tracks_plus_clutter(tracks, rescore, thr):
    boxes, scores = tracks
    info = {}
    want = check(boxes, scores, 0.05, thr[0], thr[1], 130, rescore, 'tracks %s %s' % (rescore, thr), info)
    # sequences were found (three tracks, some frames missed) and singletons dominate, as in a real video
    assert info['long_paths'] >= 3 and info['paths'] > info['long_paths'] and want[2].min() > 0
    print('tracks %s link %.1f nms %.1f: %d paths, %d longer than one box, %d kept' % (rescore, thr[0], thr[1], info['paths'],
                                                                                       info['long_paths'], int(want[2].sum())))


def test_ties_equal_boxes_and_equal_scores():
    boxes, scores = R.quantised_video(11, 5, 65, 3)
    flat = boxes.reshape(-1, 4)
    assert len(np.unique(flat, axis=0)) <= 12 and len(np.unique(scores)) <= 4
    for rescore, link, nms in (('avg', 0.5, 0.3), ('max', 0.5, 0.5), ('avg', 0.3, 0.7)):
        info = {}
        check(boxes, scores, 0.1, link, nms, 65, rescore, 'ties %s' % rescore, info)
        assert info['long_paths'] > 0


def test_empty_classes_frames_and_short_videos():
    boxes, scores = R.video(21, 5, 70, 4)
    scores[:, :, 2] = 0.01                        # a class without candidates
    scores[2] = 0                                 # an all-empty frame in the middle: paths break there
    info = {}
    want = check(boxes, scores, 0.05, 0.5, 0.3, 70, 'avg', 'empty frame', info)
    assert want[2][2] == 0 and want[2][[0, 1, 3, 4]].min() > 0 and not (want[1] == 1).any() and info['long_paths'] > 0
    kept_by_class = info['kept']
    assert not kept_by_class[1][0].any()
    for Fn in (1, 2):
        check(boxes[:Fn], scores[:Fn], 0.05, 0.5, 0.3, 70, 'avg', 'F=%d' % Fn)
    nothing = np.zeros_like(scores)
    got = device(boxes, nothing, 0.05, 0.5, 0.3, 70, 'avg')
    assert not got[2].any() and not got[0].any() and not got[1].any()


def test_max_num_cut():
    boxes, scores = R.video(31, 4, 96, 3, clutter=0.9)
    want = check(boxes, scores, 0.05, 0.5, 0.3, 8, 'avg', 'max_num=8')
    full = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 96, 'avg')
    assert want[2].tolist() == [8] * 4 and full[2].min() > 8
    assert all((np.diff(want[0][t, :8, 4]) <= 0).all() for t in range(4))           # score descending after the cut
    q = R.quantised_video(32, 3, 64, 3)                                             # equal scores at the cut: list position decides
    check(q[0], q[1], 0.1, 0.5, 0.3, 5, 'max', 'max_num=5 with ties')


def test_full_row_count_31_classes():
    boxes, scores = R.video(41, 3, 300, 31, tracks=6, clutter=0.9, low=0.04)
    info = {}
    want = check(boxes, scores, 0.05, 0.5, 0.3, 300, 'avg', 'R=300 ncls=31', info)
    per_class = (scores[:, :, 1:] > 0.05).sum(1)
    assert per_class.max() <= 24 and per_class.min() >= 1 and len(np.unique(want[1])) > 20 and info['long_paths'] > 0


def test_full_width_512():
    boxes, scores = R.video(51, 2, 512, 2, tracks=5, clutter=0.3, pad=0)
    assert (scores[1, 448:, 1] > 0.05).any()                                         # the last word has candidates
    check(boxes, scores, 0.05, 0.5, 0.3, 512, 'avg', 'R=512')
    with pytest.raises(native.HvrError, match='R <= 512'):
        native.seq_nms(torch.zeros((2, 513, 4), device=DEV), torch.zeros((2, 513, 2), device=DEV), 0.05)


def test_one_frame_equals_greedy_multiclass_nms():
    boxes, scores = R.video(61, 1, 300, 31, tracks=8, clutter=0.95)
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    for mx in (300, 40):
        want = native.multiclass_nms(b[0], s[0], 0.001, 0.3, mx)
        got = ops.seq_nms(b, s, 0.001, link_iou_thr=0.5, nms_iou_thr=0.3, max_num=mx)
        assert int(want[2].item()) == int(got[2][0].item()) > 30
        assert torch.equal(got[1][0], want[1]) and torch.equal(got[0][0].view(torch.int32), want[0].view(torch.int32))


def test_degenerate_boxes_return():
    boxes, scores = R.degenerate_video()
    for rescore in ('avg', 'max'):
        want = check(boxes, scores, 0.05, 0.5, 0.3, 8, rescore, 'degenerate %s' % rescore)
        assert want[2].tolist() == [5, 5, 5]


def test_rows_behind_n_are_zero_and_calls_repeat():
    boxes, scores = R.video(71, 4, 80, 3)
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    one = native.seq_nms(b, s, 0.05, 0.5, 0.3, 120, 'avg')
    # the second call writes into buffers poisoned beforehand: every byte of the result, the zero rows behind n included, is the call's
    poisoned = (torch.full((4, 120, 5), 7.0, device=DEV), torch.full((4, 120), 7, dtype=torch.long, device=DEV),
                torch.full((4,), 7, dtype=torch.int32, device=DEV))
    two = native.seq_nms(b, s, 0.05, 0.5, 0.3, 120, 'avg', out=poisoned)
    assert all(x is y for x, y in zip(two, poisoned)) and all(torch.equal(x, y) for x, y in zip(one, two))
    n = two[2].tolist()
    assert 0 < max(n) < 120
    for t, k in enumerate(n):
        assert not two[0][t, k:].any() and not two[1][t, k:].any() and (two[0][t, :k, 4] > 0).all()
    ref = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 120, 'avg')
    assert np.array_equal(two[0].cpu().numpy().view(np.int32), ref[0].view(np.int32)) and np.array_equal(two[2].cpu().numpy(), ref[2])


def test_call_is_capturable_and_replays_to_the_same_bytes():
    boxes, scores = R.video(81, 6, 100, 4)
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        want = [t.clone() for t in native.seq_nms(b, s, 0.05, 0.5, 0.3, 100, 'avg')]      # also warms the stream's workspace up
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graphs._capture(graph, stream=stream):
        out = native.seq_nms(b, s, 0.05, 0.5, 0.3, 100, 'avg')
    for _ in range(2):
        for t in out:
            t.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out, want))
    ref = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 100, 'avg')
    assert np.array_equal(out[0].cpu().numpy().view(np.int32), ref[0].view(np.int32)) and np.array_equal(out[2].cpu().numpy(), ref[2])


# ------------------------------------------------------------------------------------------------------ through the window loop
def _pad(x, rows):
    out = np.zeros((rows, x.shape[1]), F32)
    out[:x.shape[0]] = x
    return out


def _same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x, F32).reshape(-1, 5).view(np.int32), np.asarray(y, F32).reshape(-1, 5).view(np.int32))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize('kind', ['hvr', 'selsa'])
def test_config1_video_through_the_window_runner(kind):
    """T = 3, N = 32, f32, seeded weights, a 5-frame video: the runner with seq_nms == the raw read-outs collected by hand + seq_nms_ref."""
    T, N = 3, 32
    make = hvr_config if kind == 'hvr' else selsa_config
    model = hvrnet_amd.build_model(make(frame_interval=1, nms_post=N), S.synth_state_dict(kind), torch.float32, DEV)
    frames = [S.synth_frame(i, seed=5, img_hw=(480, 800), pad_hw=(480, 800)).to(DEV) for i in range(5)]
    meta = dict(ori_shape=(600, 1000, 3), img_shape=(480, 800, 3), pad_shape=(480, 800, 3), scale_factor=0.8, flip=False)
    metas = [dict(meta) for _ in frames]
    cfg = model.test_cfg.rcnn
    sq = dict(link_iou_thr=0.5, rescore='avg')
    nb = 2 if kind == 'hvr' else 1
    with torch.no_grad():
        before = VideoWindowRunner(model, T, rescale=True).run_video(frames, metas)
        got = VideoWindowRunner(model, T, rescale=True, seq_nms=sq).run_video(frames, metas)
        cached = VideoWindowRunner(model, T, rescale=True, cache_frames=True, seq_nms=sq).run_video(frames, metas)
        after = VideoWindowRunner(model, T, rescale=True).run_video(frames, metas)
        # by hand: the windows of the loop, each read out raw
        c4 = [model(img=f, img_meta=[m], backbone_feat=True)[0] for f, m in zip(frames, metas)]
        win = window_frames(len(frames), T)
        raws = [model(x=[c4[i] for i in win[o]], img=None, img_meta=[metas[i] for i in win[o]], forward_feat=True, return_loss=False,
                      rescale=True, raw=True) for o in range(len(frames))]
    assert sorted(got) == sorted(cached) == list(range(len(frames))) and all(len(r) == nb for r in raws)
    n_det = 0
    for b in range(nb):
        boxes = np.stack([_pad(r[b][0].cpu().numpy(), N) for r in raws])
        scores = np.stack([_pad(r[b][1].cpu().numpy(), N) for r in raws])
        assert boxes.shape == (5, N, 4) and scores.shape == (5, N, 31)
        d, l, n = R.seq_nms_ref(boxes, scores, cfg.score_thr, sq['link_iou_thr'], cfg.nms.iou_thr, cfg.max_per_img, sq['rescore'])
        for o in range(len(frames)):
            want = [d[o, :n[o]][l[o, :n[o]] == c] for c in range(30)]
            for name, res in (('runner', got), ('per-frame cache', cached)):
                have = res[o][b] if kind == 'hvr' else res[o]
                assert _same_results(have, want), '%s %s: frame %d branch %d differs from seq_nms_ref on the raw read-outs' % (kind, name, o, b)
            n_det += int(n[o])
    assert n_det > 0
    # without the key: today's results, before and after
    assert model.test_cfg.rcnn.get('seq_nms') is None and VideoWindowRunner(model, T).seq_nms is None
    for o in before:
        for x, y in zip(before[o] if kind == 'hvr' else [before[o]], after[o] if kind == 'hvr' else [after[o]]):
            assert _same_results(x, y)
    # the config key is the runner's default
    model.test_cfg.rcnn['seq_nms'] = dict(sq)
    with torch.no_grad():
        by_key = VideoWindowRunner(model, T, rescale=True).run_video(frames, metas)
    for o in got:
        for x, y in zip(by_key[o] if kind == 'hvr' else [by_key[o]], got[o] if kind == 'hvr' else [got[o]]):
            assert _same_results(x, y)
    print('%s: %d detections over 5 frames x %d branches equal seq_nms_ref on the raw read-outs' % (kind, n_det, nb))
