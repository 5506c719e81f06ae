"""Batched Seq-NMS with tube outputs on the GPU (hvrnet_amd/csrc/seqnms.hip through native.seq_nms_batched) against the host
restatement of DESIGN.md 8d + 8e (tests/seqnms_tube_refs.py: seq_nms_tubes_ref).  All seven outputs -- dets, labels, n, tube_ids, the
tube table, its scores and the prefix counts -- are compared bit for bit; there is no tolerance anywhere in this file.  Nothing here
reads the reference tree."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import graphs, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config, selsa_config  # noqa: E402
from hvrnet_amd.window import VideoWindowRunner, window_frames  # noqa: E402
from tests import seqnms_refs as R  # noqa: E402
from tests import seqnms_tube_refs as T  # noqa: E402
from tests.test_seqnms_tubes_host import boundary_case  # noqa: E402

DEV = 'cuda:0'
F32 = np.float32
NAMES = ('dets', 'labels', 'n', 'tube_ids', 'tubes', 'tube_scores', 'tube_start')


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def device(boxes, scores, counts, *a, **kw):
    out = native.seq_nms_batched(torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV), counts, *a, tubes=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(boxes, scores, counts, score_thr, link_thr, nms_thr, max_num, rescore, what, info=None):
    """device == seq_nms_tubes_ref on all seven outputs, bit for bit (max_tubes = the true total).  -> the reference's outputs."""
    want = T.seq_nms_tubes_ref(boxes, scores, counts, score_thr, link_thr, nms_thr, max_num, rescore, info=info)
    got = device(boxes, scores, counts, score_thr, link_thr, nms_thr, max_num, rescore, max_tubes=len(want[4]))
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, '%s: %s is %s %s, expected %s %s' % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = bits(g) != bits(w)
        assert not bad.any(), '%s: %d values of %s differ, first at %s' % (what, int(bad.sum()), name, np.argwhere(bad)[0].tolist())
    return want


def long_tubes(want):
    return int((want[4][:, 3] > 1).sum())


@pytest.mark.parametrize('Rn', [1, 63, 64, 65, 130])
def test_lane_and_word_boundaries(Rn):
    boxes, scores = R.video(100 + Rn, 3, Rn, 3, tracks=min(3, max(Rn // 3, 1)), pad=0 if Rn < 4 else 2)
    want = check(boxes, scores, [3], 0.05, 0.5, 0.3, Rn, 'avg', 'R=%d' % Rn)
    assert want[2].sum() > 0 and (Rn < 63 or long_tubes(want) > 0)
    check(boxes, scores, [3], 0.05, 0.5, 0.3, Rn, 'max', 'R=%d max' % Rn)


@pytest.fixture(scope='module')
def tracks():
    return R.video(7, 17, 130, 4)


@pytest.mark.parametrize('thr', [(0.5, 0.3), (0.3, 0.5)], ids=['link5_nms3', 'link3_nms5'])
def test_tracks_plus_clutter(tracks, thr):
    boxes, scores = tracks
    want = check(boxes, scores, [17], 0.05, thr[0], thr[1], 130, 'avg', 'tracks %s' % (thr,))
    assert long_tubes(want) >= 3 and len(want[4]) > long_tubes(want)
    print('tracks link %.1f nms %.1f: %d tubes, %d longer than one box' % (thr[0], thr[1], len(want[4]), long_tubes(want)))


def test_ragged_batch_equals_three_single_calls():
    boxes, scores = R.video(7, 22, 130, 4)
    counts = [1, 17, 4]
    want = check(boxes, scores, counts, 0.05, 0.5, 0.3, 130, 'avg', 'ragged (1, 17, 4)')
    assert np.diff(want[6]).min() > 0 and long_tubes(want) >= 3
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    plain = native.seq_nms_batched(b, s, counts, 0.05, 0.5, 0.3, 130, 'avg')          # no tubes: the same detections
    f0 = 0
    for p, Fn in enumerate(counts):
        one = native.seq_nms(b[f0:f0 + Fn], s[f0:f0 + Fn], 0.05, 0.5, 0.3, 130, 'avg')
        alone = T.seq_nms_tubes_ref(boxes[f0:f0 + Fn], scores[f0:f0 + Fn], [Fn], 0.05, 0.5, 0.3, 130, 'avg')
        for k in range(3):
            assert np.array_equal(bits(one[k].cpu().numpy()), bits(want[k][f0:f0 + Fn])), 'problem %d: %s differs from native.seq_nms on the slice' % (p, NAMES[k])
            assert torch.equal(plain[k][f0:f0 + Fn], one[k]), 'problem %d without tubes: %s' % (p, NAMES[k])
        rows = want[4][want[6][p]:want[6][p + 1]]
        assert np.array_equal(rows[:, 1:], alone[4][:, 1:]) and (rows[:, 0] == p).all() and np.array_equal(want[3][f0:f0 + Fn], alone[3])
        f0 += Fn
    assert len(plain) == 3


def test_problem_boundary():
    boxes, scores = boundary_case()
    split = check(boxes, scores, [1, 1], 0.05, 0.5, 0.3, 4, 'avg', 'two one-frame problems')
    joined = check(boxes, scores, [2], 0.05, 0.5, 0.3, 4, 'avg', 'one two-frame problem')
    assert split[6].tolist() == [0, 2, 4] and (split[4][:, 3] == 1).all()            # identical frames, yet no link across the boundary
    assert joined[6].tolist() == [0, 2] and (joined[4][:, 3] == 2).all()
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    for p in range(2):                                                               # each problem: greedy NMS of its frame
        want = native.multiclass_nms(b[p], s[p], 0.05, 0.3, 4)
        assert np.array_equal(bits(want[0].cpu().numpy()), bits(split[0][p])) and int(want[2].item()) == split[2][p] == 2


def test_full_row_count_31_classes():
    boxes, scores = R.video(41, 4, 300, 31, tracks=6, clutter=0.9, low=0.04)
    want = check(boxes, scores, [3, 1], 0.05, 0.5, 0.3, 300, 'avg', 'R=300 ncls=31 F=4')
    assert len(np.unique(want[4][:, 1])) > 20 and long_tubes(want) > 0 and want[6][1] > want[6][2] - want[6][1] > 0


def test_full_width_512():
    boxes, scores = R.video(51, 2, 512, 2, tracks=5, clutter=0.3, pad=0)
    assert (scores[1, 448:, 1] > 0.05).any()                                         # the last word has candidates
    want = check(boxes, scores, [2], 0.05, 0.5, 0.3, 512, 'avg', 'R=512')
    assert long_tubes(want) > 0
    with pytest.raises(native.HvrError, match='R <= 512'):
        native.seq_nms_batched(torch.zeros((2, 513, 4), device=DEV), torch.zeros((2, 513, 2), device=DEV), [1, 1], 0.05, tubes=True)


def test_max_num_cut():
    boxes, scores = R.video(31, 4, 96, 3, clutter=0.9)
    want = check(boxes, scores, [4], 0.05, 0.5, 0.3, 8, 'avg', 'max_num=8')
    full = T.seq_nms_tubes_ref(boxes, scores, [4], 0.05, 0.5, 0.3, 96, 'avg')
    assert want[2].tolist() == [8] * 4 and full[2].min() > 8
    assert (want[3][:, :8] >= 0).all() and np.array_equal(want[4], full[4])           # the table (lengths included) ignores the cut
    for t in range(4):                                                               # the surviving rows carry the ids they have uncut
        for q in range(8):
            hit = np.flatnonzero((full[0][t, :full[2][t]].view(np.int32) == want[0][t, q].view(np.int32)).all(1) & (full[1][t, :full[2][t]] == want[1][t, q]))
            assert want[3][t, q] in full[3][t, hit]
    q = R.quantised_video(32, 3, 64, 3)                                              # equal scores at the cut: list position decides
    cut = check(q[0], q[1], [2, 1], 0.1, 0.5, 0.3, 5, 'max', 'max_num=5 with ties')
    assert cut[2].max() == 5 and cut[3].shape == (3, 5)


def test_max_tubes_cap_leaves_the_rows_behind_it_untouched():
    boxes, scores = R.video(71, 6, 80, 3)
    counts = [4, 2]
    want = T.seq_nms_tubes_ref(boxes, scores, counts, 0.05, 0.5, 0.3, 80, 'avg')
    total = int(want[6][-1])
    assert total > 40 and want[6][1] < total - 7 < total
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    for cap in (total - 7, int(want[6][1]) - 3, 0, total + 5):
        out = (torch.empty((6, 80, 5), device=DEV), torch.empty((6, 80), dtype=torch.long, device=DEV), torch.empty(6, dtype=torch.int32, device=DEV),
               torch.full((6, 80), 9, dtype=torch.int32, device=DEV), torch.full((cap, 4), -7, dtype=torch.int32, device=DEV),
               torch.full((cap,), -7.0, device=DEV), torch.full((3,), 9, dtype=torch.int32, device=DEV))
        got = native.seq_nms_batched(b, s, counts, 0.05, 0.5, 0.3, 80, 'avg', tubes=True, max_tubes=cap, out=out)
        torch.cuda.synchronize()
        assert all(x is y for x, y in zip(got, out))
        ref = T.seq_nms_tubes_ref(boxes, scores, counts, 0.05, 0.5, 0.3, 80, 'avg', max_tubes=cap, fill=(-7, -7.0))
        for name, g, w in zip(NAMES, got, ref):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w)), 'max_tubes=%d: %s differs' % (cap, name)
        assert got[6].tolist() == want[6].tolist()                                   # the prefix counts stay exact, whatever the cap
        if cap > total:
            assert (got[4][total:] == -7).all() and (got[5][total:] == -7).all()     # canary behind the total


def test_empty_classes_frames_and_degenerate_boxes():
    boxes, scores = R.video(21, 5, 70, 4)
    scores[:, :, 2] = 0.01                        # a class without candidates: its id base equals the next class's
    scores[2] = 0                                 # an all-empty frame in the middle: tubes break there
    want = check(boxes, scores, [5], 0.05, 0.5, 0.3, 70, 'avg', 'empty frame')
    assert want[2][2] == 0 and (want[3][2] == -1).all() and not (want[4][:, 1] == 1).any() and long_tubes(want) > 0
    assert ((want[4][:, 2] + want[4][:, 3] <= 2) | (want[4][:, 2] >= 3)).all()       # no tube spans the empty frame
    check(boxes, scores, [2, 1, 2], 0.05, 0.5, 0.3, 70, 'avg', 'empty frame as a problem of its own')
    nothing = np.zeros_like(scores)
    got = device(boxes, nothing, [2, 3], 0.05, 0.5, 0.3, 70, 'avg')
    assert not got[2].any() and not got[0].any() and (got[3] == -1).all() and got[6].tolist() == [0, 0, 0]
    boxes, scores = R.degenerate_video()
    for rescore in ('avg', 'max'):
        want = check(boxes, scores, [3], 0.05, 0.5, 0.3, 8, rescore, 'degenerate %s' % rescore)
        assert want[2].tolist() == [5, 5, 5] and want[4][:, 3].sum() == 15
        check(boxes, scores, [1, 2], 0.05, 0.5, 0.3, 8, rescore, 'degenerate %s, two problems' % rescore)


def test_call_is_capturable_and_replays_to_the_same_bytes():
    boxes, scores = R.video(81, 6, 100, 4)
    counts = [2, 4]
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        want = [t.clone() for t in native.seq_nms_batched(b, s, counts, 0.05, 0.5, 0.3, 100, 'avg', tubes=True)]   # also warms the workspace up
    stream.synchronize()
    total = int(want[6][-1].item())
    graph = torch.cuda.CUDAGraph()
    with graphs._capture(graph, stream=stream):
        out = native.seq_nms_batched(b, s, counts, 0.05, 0.5, 0.3, 100, 'avg', tubes=True)
    for _ in range(2):
        for t in out:
            t.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(out, want)):
            assert torch.equal(x[:total], y[:total]) if k in (4, 5) else torch.equal(x, y), NAMES[k]
        assert (out[4][total:] == 3).all() and (out[5][total:] == 3).all() and out[4].shape[0] == 3 * 6 * 100 > total   # untouched behind the total
    ref = T.seq_nms_tubes_ref(boxes, scores, counts, 0.05, 0.5, 0.3, 100, 'avg')
    for k, name in enumerate(NAMES):
        g = out[k].cpu().numpy()
        assert np.array_equal(bits(g[:total] if k in (4, 5) else g), bits(ref[k])), name


def test_old_path_is_intact():
    """tubes=False, frame_counts=None: today's triple through today's entry point, the same bytes as seq_nms_ref."""
    boxes, scores = R.video(71, 4, 80, 3)
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    calls = []
    old, batched = native.seq_nms, native.seq_nms_batched
    native.seq_nms = lambda *a, **kw: calls.append('seq_nms') or old(*a, **kw)
    native.seq_nms_batched = lambda *a, **kw: calls.append('seq_nms_batched') or batched(*a, **kw)
    try:
        plain = ops.seq_nms(b, s, 0.05, 0.5, 0.3, 120, 'avg')
        both = hvrnet_amd.seq_nms(b, s, 0.05, 0.5, 0.3, 120, 'avg', frame_counts=[4], tubes=True)
        split = ops.seq_nms(b, s, 0.05, 0.5, 0.3, 120, 'avg', frame_counts=[3, 1])
    finally:
        native.seq_nms, native.seq_nms_batched = old, batched
    assert calls == ['seq_nms', 'seq_nms_batched', 'seq_nms_batched'] and len(plain) == 3 and len(both) == 7 and len(split) == 3
    ref = R.seq_nms_ref(boxes, scores, 0.05, 0.5, 0.3, 120, 'avg')
    for k in range(3):
        assert np.array_equal(bits(plain[k].cpu().numpy()), bits(ref[k])) and torch.equal(plain[k], both[k]), NAMES[k]
    assert not torch.equal(split[2], plain[2]) or not torch.equal(split[0], plain[0])         # the boundary changes this video's result


# ------------------------------------------------------------------------------------------------------ through the window loop
def _same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x, F32).reshape(-1, 5).view(np.int32), np.asarray(y, F32).reshape(-1, 5).view(np.int32))
                                    for x, y in zip(a, b))


def _pad(x, rows):
    out = np.zeros((rows, x.shape[1]), F32)
    out[:x.shape[0]] = x
    return out


@pytest.mark.parametrize('kind', ['hvr', 'selsa'])
def test_config1_videos_through_the_window_runner(kind):
    """T = 3, N = 32, f32, seeded weights, a 5-frame and a 3-frame video."""
    T_, N = 3, 32
    make = hvr_config if kind == 'hvr' else selsa_config
    model = hvrnet_amd.build_model(make(frame_interval=1, nms_post=N), S.synth_state_dict(kind), torch.float32, DEV)
    frames = [S.synth_frame(i, seed=5, img_hw=(480, 800), pad_hw=(480, 800)).to(DEV) for i in range(5)]
    meta = dict(ori_shape=(600, 1000, 3), img_shape=(480, 800, 3), pad_shape=(480, 800, 3), scale_factor=0.8, flip=False)
    metas = [dict(meta) for _ in frames]
    short, short_metas = frames[2:], metas[2:]
    cfg = model.test_cfg.rcnn
    sq = dict(link_iou_thr=0.5, rescore='avg')
    nb = 2 if kind == 'hvr' else 1
    branches = (lambda r: r) if kind == 'hvr' else (lambda r: [r])
    with torch.no_grad():
        plain = VideoWindowRunner(model, T_, rescale=True, seq_nms=sq).run_video(frames, metas)
        plain_short = VideoWindowRunner(model, T_, rescale=True, seq_nms=sq).run_video(short, short_metas)
        runner = VideoWindowRunner(model, T_, rescale=True, seq_nms=dict(sq, tubes=True))
        got = runner.run_video(frames, metas)
        tube_data = runner.tubes
        both = runner.run_videos([frames, short], [metas, short_metas])
        both_tubes = runner.tubes
        c4 = [model(img=f, img_meta=[m], backbone_feat=True)[0] for f, m in zip(frames, metas)]
        win = window_frames(len(frames), T_)
        raws = [model(x=[c4[i] for i in win[o]], img=None, img_meta=[metas[i] for i in win[o]], forward_feat=True, return_loss=False,
                      rescale=True, raw=True) for o in range(len(frames))]
    # tubes=True changes no detection; run_videos equals run_video on each video
    assert sorted(got) == sorted(plain) == list(range(5)) and sorted(both[1]) == list(range(3)) and len(both) == 2
    for o in range(5):
        for x, y, z in zip(branches(plain[o]), branches(got[o]), branches(both[0][o])):
            assert _same_results(x, y) and _same_results(x, z), 'frame %d' % o
    for o in range(3):
        for x, z in zip(branches(plain_short[o]), branches(both[1][o])):
            assert _same_results(x, z), 'short video, frame %d' % o
    # every id points at a table row of its class whose frame span covers the frame
    n_ids = n_long = 0
    for data, res, Fv in ((tube_data, got, 5), (both_tubes[0], both[0], 5), (both_tubes[1], both[1], 3)):
        for b, td in enumerate(data if kind == 'hvr' else [data]):
            table = td['tubes']
            assert table.shape[1] == 4 and len(td['scores']) == len(table) and len(td['ids']) == Fv and (table[:, 0] == b).all()
            members = np.zeros(len(table), np.int64)
            for o in range(Fv):
                dets = branches(res[o])[b]
                assert len(td['ids'][o]) == len(dets) == 30
                for c in range(30):
                    ids = td['ids'][o][c]
                    assert len(ids) == len(dets[c])
                    for i, det in zip(ids, dets[c]):
                        _, lab, start, ln = table[i]
                        assert lab == c and start <= o < start + ln and F32(det[4]).view(np.int32) == F32(td['scores'][i]).view(np.int32)
                        members[i] += 1
                        n_ids += 1
            assert (members <= table[:, 3]).all()             # (max_per_img may cut members away; it never adds one)
            n_long += int((table[:, 3] > 1).sum())
    assert n_ids > 0
    assert all(np.array_equal(x['tubes'], y['tubes']) for x, y in zip(tube_data if kind == 'hvr' else [tube_data], both_tubes[0] if kind == 'hvr' else [both_tubes[0]]))
    # the batched branches equal native.seq_nms run per branch on the raw read-outs
    for b in range(nb):
        bx = torch.as_tensor(np.stack([_pad(r[b][0].cpu().numpy(), N) for r in raws])).to(DEV)
        sc = torch.as_tensor(np.stack([_pad(r[b][1].cpu().numpy(), N) for r in raws])).to(DEV)
        d, l, n = [t.cpu().numpy() for t in native.seq_nms(bx, sc, cfg.score_thr, sq['link_iou_thr'], cfg.nms.iou_thr, cfg.max_per_img, sq['rescore'])]
        for o in range(5):
            want = [d[o, :n[o]][l[o, :n[o]] == c] for c in range(30)]
            assert _same_results(branches(got[o])[b], want), '%s: frame %d branch %d differs from native.seq_nms on the branch alone' % (kind, o, b)
    print('%s: %d ids checked over the videos, %d tubes longer than one box' % (kind, n_ids, n_long))
