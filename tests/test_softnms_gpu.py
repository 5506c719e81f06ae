"""Soft-NMS read-out on the GPU (test_cfg.rcnn.nms type='soft_nms'): the kernels against the reference's recorded outputs
(tests/golden/g20_soft_nms.npz) and the numpy restatement (tests/softnms_refs.py), and the detector paths end to end.  Nothing here
reads the reference tree.

The rule for scores ("rule of 1"): the index sequence, the count, the labels and the boxes are exact; a linear score is bit-exact; a
gaussian score is expected bit-exact and asserted within one f32 ulp per rescoring the entry received -- each weight is one correctly
rounded f32 of an f64 exp whose last bit may differ between the device's math library and numpy's.  Every test prints how many scores
differ at all.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import box_ops, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config, selsa_config  # noqa: E402
from hvrnet_amd.graphs import GraphedClip  # noqa: E402
from hvrnet_amd.window import VideoWindowRunner  # noqa: E402
from tests import softnms_refs as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
CODE = {1: 'linear', 2: 'gaussian'}
LINEAR = dict(type='soft_nms', iou_thr=0.5, min_score=0.05)
GAUSSIAN = dict(type='soft_nms', iou_thr=0.5, method='gaussian', sigma=0.5, min_score=0.05)


def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_soft_nms.npz'))


def params(g, key):
    iou_thr, code, sigma, min_score = [float(v) for v in g[key]]
    return dict(iou_thr=iou_thr, method=CODE[int(code)], sigma=sigma, min_score=min_score)


def check_scores(got, want, decays, method, what):
    """-> number of scores that differ at all."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, '%s: %s scores, expected %s' % (what, got.shape, want.shape)
    differ = int((got.view(np.int32) != want.view(np.int32)).sum())
    dev = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = R.score_tolerance(want, np.asarray(decays), method)
    assert np.all(dev <= tol), '%s (%s): %d scores differ, worst %.3g against a bar of %.3g' % (
        what, method, differ, dev.max(), tol[np.argmax(dev - tol)])
    return differ


# ------------------------------------------------------------------------------------------------------ 1. single lists
def test_soft_nms_single_lists_match_reference_golden():
    g = gold()
    out, inds = ops.soft_nms(torch.as_tensor(g['doc_dets']).to(DEV), float(g['doc_iou_thr']), sigma=float(g['doc_sigma']))
    assert len(inds) == len(out) == 3 and inds.dtype == torch.long
    assert np.array_equal(inds.cpu().numpy(), g['doc_inds']) and np.array_equal(out[:, 4].cpu().numpy(), g['doc_scores'])
    total = differ = 0
    for name in [str(n) for n in g['single_names']]:
        dets = g['sl_%s_dets' % name]
        for p in [str(p) for p in g['param_names']]:
            prm, info = params(g, 'param_' + p), {}
            out, inds = ops.soft_nms(torch.as_tensor(dets).to(DEV), **prm)
            want_inds, want_scores = g['sl_%s_%s_inds' % (name, p)], g['sl_%s_%s_scores' % (name, p)]
            assert inds.cpu().numpy().tolist() == want_inds.tolist(), '%s %s: other boxes / order' % (name, p)
            R.soft_nms(dets, info=info, **prm)
            out = out.cpu().numpy()
            assert np.array_equal(out[:, :4], dets[want_inds, :4])
            differ += check_scores(out[:, 4], want_scores, info['decays'], prm['method'], '%s %s' % (name, p))
            total += len(want_inds)
    print('soft_nms single lists: %d of %d scores differ from the recorded ones' % (differ, total))


def test_soft_nms_native_zeroes_the_rows_behind_the_count_and_rejects_513():
    dets = torch.as_tensor(R.clustered_dets(11, 200)).to(DEV)
    out, inds, n = native.soft_nms(dets, 0.5, 'gaussian', 0.3, 0.05)
    k = int(n.item())
    assert 0 < k < 200 and not out[k:].any() and not inds[k:].any()
    with pytest.raises(native.HvrError, match='512'):
        native.soft_nms(torch.zeros((513, 5), device=DEV), 0.5)
    out, inds = ops.soft_nms(torch.zeros((0, 5), device=DEV), 0.5)
    assert out.shape == (0, 5) and inds.shape == (0,)


# -------------------------------------------------------------------------------------------------------- 2. multiclass
def _mc_check(boxes, scores, thr, cfg, mx, want=None, what=''):
    db, dl = box_ops.multiclass_nms(torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV), thr, cfg, mx)
    info = {}
    wd, wl = R.multiclass(boxes, scores, thr, cfg, mx, info=info)
    if want is not None:
        assert np.array_equal(wl, want[1]) and np.array_equal(wd[:, 4].view(np.int32), want[0].view(np.int32)) and np.array_equal(info['rows'], want[2])
    db, dl = db.cpu().numpy(), dl.cpu().numpy()
    assert dl.tolist() == wl.tolist(), '%s: labels / order differ' % what
    assert np.array_equal(db[:, :4], wd[:, :4]), '%s: other boxes' % what
    return check_scores(db[:, 4], wd[:, 4], info['decays'], cfg.get('method', 'linear'), what), len(wl)


def test_multiclass_soft_nms_matches_reference_golden():
    g = gold()
    thr = float(g['mc_score_thr'])
    differ = total = 0
    for name in [str(n) for n in g['mc_names']]:
        boxes, scores = g['mc_%s_boxes' % name], g['mc_%s_scores' % name]
        for c in [str(c) for c in g['mc_cfg_names']]:
            cfg = dict(type='soft_nms', **params(g, 'mc_cfg_' + c))
            for mx in g['mc_max_nums'].tolist():
                tag = 'mc_%s_%s_%s' % (name, c, 'm1' if mx < 0 else str(mx))
                d, n = _mc_check(boxes, scores, thr, cfg, mx, (g[tag + '_scores'], g[tag + '_labels'], g[tag + '_rows']), tag)
                differ, total = differ + d, total + n
                if name == 'none':
                    assert n == 0
    print('multiclass soft_nms: %d of %d scores differ from the recorded ones' % (differ, total))
    # the remaining nms_cfg keys default as in nms_wrapper.soft_nms: (iou_thr) alone == linear, sigma 0.5, min_score 1e-3
    boxes, scores = g['mc_r32_boxes'], g['mc_r32_scores']
    a = box_ops.multiclass_nms(torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV), thr, dict(type='soft_nms', iou_thr=0.3), 100)
    b = box_ops.multiclass_nms(torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV), thr,
                               dict(type='soft_nms', iou_thr=0.3, method='linear', sigma=0.5, min_score=1e-3), 100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('cfg', [LINEAR, GAUSSIAN], ids=['linear', 'gaussian'])
def test_multiclass_soft_nms_sizes_and_batches(cfg):
    """R = 1, R = 512 (the limit), no candidate at all, uniform scores (every class carries every row: the benchmark's case), P = 3
    problems in one launch == three launches; R = 513 is an error, not a wrong answer."""
    for seed, Rn in ((5, 1), (6, 512), (7, 300)):
        boxes, scores = R.clustered_dets(seed, Rn)[:, :4], R.class_scores(seed + 100, Rn, 31)
        for mx in (300, 100):
            d, n = _mc_check(boxes, scores, 0.001, cfg, mx, what='R=%d max_num=%d' % (Rn, mx))
            print('R = %d, max_num %d: %d detections, %d scores differ' % (Rn, mx, n, d))
    boxes = R.clustered_dets(8, 300)[:, :4]
    flat = np.random.RandomState(9).uniform(0.030, 0.034, (300, 31)).astype(np.float32)
    d, n = _mc_check(boxes, flat, 0.001, cfg, 300, what='uniform scores')
    assert n > 0
    none = np.zeros((32, 31), np.float32)
    dets, labels, cnt = native.multiclass_soft_nms(torch.as_tensor(boxes[:32]).to(DEV), torch.as_tensor(none).to(DEV), 0.001, cfg['iou_thr'], 50,
                                                   cfg.get('method', 'linear'), cfg.get('sigma', 0.5), cfg['min_score'])
    assert int(cnt.item()) == 0 and not dets.any() and not labels.any()
    # P = 3
    prob = [(R.clustered_dets(20 + i, 300)[:, :4], R.class_scores(30 + i, 300, 31, sharp=(1.0, 4.0, 0.01)[i])) for i in range(3)]
    kw = dict(method=cfg.get('method', 'linear'), sigma=cfg.get('sigma', 0.5), min_score=cfg['min_score'])
    B = torch.as_tensor(np.stack([p[0] for p in prob])).to(DEV)
    Sc = torch.as_tensor(np.stack([p[1] for p in prob])).to(DEV)
    dets, labels, cnt = native.multiclass_soft_nms(B, Sc, 0.001, cfg['iou_thr'], 300, **kw)
    assert dets.shape == (3, 300, 5) and labels.shape == (3, 300) and cnt.shape == (3,)
    for i in range(3):
        d1, l1, c1 = native.multiclass_soft_nms(B[i], Sc[i], 0.001, cfg['iou_thr'], 300, **kw)
        assert int(c1.item()) == int(cnt[i].item()) > 0 and torch.equal(d1, dets[i]) and torch.equal(l1, labels[i])
        assert not dets[i, int(cnt[i].item()):].any()
    with pytest.raises(native.HvrError, match='512'):
        native.multiclass_soft_nms(torch.zeros((513, 4), device=DEV), torch.zeros((513, 31), device=DEV), 0.001, 0.5, 300)


# ------------------------------------------------------------------------------------------------------ 3. greedy untouched
def test_greedy_read_out_is_untouched():
    boxes = torch.as_tensor(R.clustered_dets(40, 300)[:, :4]).to(DEV)
    scores = torch.as_tensor(R.class_scores(41, 300, 31)).to(DEV)
    for mx in (300, 100):
        want = native.multiclass_nms(boxes, scores, 0.001, 0.3, mx)
        got = native.readout_nms(boxes, scores, 0.001, dict(type='nms', iou_thr=0.3), mx)
        k = int(want[2].item())
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        db, dl = box_ops.multiclass_nms(boxes, scores, 0.001, dict(type='nms', iou_thr=0.3), mx)
        assert torch.equal(db, want[0][:k]) and torch.equal(dl, want[1][:k])
        db2, dl2 = box_ops.multiclass_nms(boxes, scores, 0.001, dict(iou_thr=0.3), mx)            # type defaults to 'nms'
        assert torch.equal(db2, db) and torch.equal(dl2, dl)
    with pytest.raises(NotImplementedError):
        box_ops.multiclass_nms(boxes, scores, 0.001, dict(type='fast_nms', iou_thr=0.3), 100)


# --------------------------------------------------------------------------------------------------- 4 / 5. the detector paths
class Recorder(object):
    """Records, in call order, the (boxes, scores) every read-out of the model decodes (what get_det_bboxes(cfg=None) returns) on
    their way into BBoxHead._nms (one call per window and branch) or BBoxHead._nms_clips (one call per branch with the W clips of
    a call), with the stream they were enqueued on; `expected()` applies the restatement to them on the host."""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __enter__(self):
        head = self.model.bbox_head
        real, real_clips = type(head)._nms, type(head)._nms_clips

        def rec(boxes, scores, cfg, defer=False):
            self.calls.append((boxes.detach().clone(), scores.detach().clone(), torch.cuda.current_stream().cuda_stream))
            return real(head, boxes, scores, cfg, defer)

        def rec_clips(boxes, scores, cfg):
            for b_, s_ in zip(boxes, scores):
                self.calls.append((b_.detach().clone(), s_.detach().clone(), torch.cuda.current_stream().cuda_stream))
            return real_clips(head, boxes, scores, cfg)

        head._nms, head._nms_clips = rec, rec_clips
        return self

    def __exit__(self, *a):
        del self.model.bbox_head._nms, self.model.bbox_head._nms_clips

    def expected(self):
        torch.cuda.synchronize()
        cfg = self.model.test_cfg.rcnn
        nms = cfg.nms.to_dict()
        out = []
        for boxes, scores, stream in self.calls:
            info = {}
            d, l = R.multiclass(boxes.cpu().numpy(), scores.cpu().numpy(), cfg.score_thr, nms, cfg.max_per_img, info=info)
            out.append((d, l, info, stream))
        return out


def _branch_matches(branch, exp, method):
    d, l, info = exp[:3]
    differ = 0
    for c, got in enumerate(branch):
        got = np.asarray(got).reshape(-1, 5)
        sel = l == c
        if got.shape[0] != int(sel.sum()) or not np.array_equal(got[:, :4], d[sel, :4]):
            return None
        dev = np.abs(got[:, 4].astype(np.float64) - d[sel, 4].astype(np.float64))
        if np.any(dev > R.score_tolerance(d[sel, 4], info['decays'][sel], method)):
            return None
        differ += int((got[:, 4] != d[sel, 4]).sum())
    return differ


def check_windows(windows, rec, what, batched=False):
    """windows: the results in call order, each a list of its branches (a branch = a list of per-class arrays).  Branch b of window w
    must equal the restatement on the inputs of ITS OWN recorded read-out: the calls come window by window, a window's branches in
    order -- except that the two-stream read-out enqueues branch 1 (side stream) before branch 0, which shows in the recorded streams;
    a batched call (`_nms_clips`) records branch by branch, the clips of a branch in order."""
    exps = rec.expected()
    method = rec.model.test_cfg.rcnn.nms.get('method', 'linear')
    W, nb = len(windows), len(windows[0])
    assert len(exps) == W * nb > 0, '%s: %d read-outs recorded for %d windows of %d branches' % (what, len(exps), W, nb)
    differ = n_det = 0
    for w, win in enumerate(windows):
        group = [exps[b * W + w] for b in range(nb)] if batched else exps[w * nb:(w + 1) * nb]
        if not batched and nb == 2 and group[0][3] != group[1][3]:
            group = group[::-1]
        for b, (br, e) in enumerate(zip(win, group)):
            m = _branch_matches(br, e, method)
            assert m is not None, '%s: window %d branch %d differs from the restatement on its own read-out (%d detections, %d expected)' % (
                what, w, b, sum(len(r) for r in br), len(e[1]))
            differ += m
            n_det += len(e[1])
    assert n_det > 0
    print('%s (%s): %d windows x %d branches, %d detections, %d scores differ from the restatement' % (what, method, W, nb, n_det, differ))
    rec.calls = []


def _branches(kind, res):
    return list(res) if kind == 'hvr' else [res]


@pytest.mark.parametrize('nms', [LINEAR, GAUSSIAN], ids=['linear', 'gaussian'])
@pytest.mark.parametrize('kind', ['hvr', 'selsa'])
def test_config1_windows_with_soft_nms(kind, nms):
    """T = 3, N = 32, f32, seeded weights: forward_feat (rescale both ways, immediate and deferred), the per-frame cache
    (forward_feat_frames through VideoWindowRunner(cache_frames=True)), forward_feat_aug (A = 2) and the plain VideoWindowRunner."""
    T = 3
    make = hvr_config if kind == 'hvr' else selsa_config
    model = hvrnet_amd.build_model(make(frame_interval=1, nms_post=32), S.synth_state_dict(kind), torch.float32, DEV)
    model.test_cfg.rcnn.nms = dict(nms)
    frames = [S.synth_frame(i, seed=5, img_hw=(480, 800), pad_hw=(480, 800)).to(DEV) for i in range(5)]
    meta = dict(ori_shape=(600, 1000, 3), img_shape=(480, 800, 3), pad_shape=(480, 800, 3), scale_factor=0.8, flip=False)
    metas = [dict(meta) for _ in frames]
    with torch.no_grad(), Recorder(model) as rec:
        c4 = [model(img=f, img_meta=[m], backbone_feat=True)[0] for f, m in zip(frames, metas)]
        for rescale in (True, False):
            res = model(x=c4[:T], img=None, img_meta=metas[:T], forward_feat=True, return_loss=False, rescale=rescale)
            check_windows([_branches(kind, res)], rec, '%s forward_feat rescale=%s' % (kind, rescale))
            pend = model(x=c4[:T], img=None, img_meta=metas[:T], forward_feat=True, return_loss=False, rescale=rescale, defer=True)
            later = pend.result()
            assert not pend.respeculated
            rec.calls = []
            for a, b in zip(_branches(kind, res), _branches(kind, later)):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'deferred != immediate'
        got = VideoWindowRunner(model, T, rescale=True, cache_frames=True).run_video(frames, metas)
        check_windows([_branches(kind, got[off]) for off in sorted(got)], rec, '%s per-frame cache' % kind)
        plain = VideoWindowRunner(model, T, rescale=True).run_video(frames, metas)
        check_windows([_branches(kind, plain[off]) for off in sorted(plain)], rec, '%s VideoWindowRunner' % kind)
        for off in plain:
            for a, b in zip(_branches(kind, plain[off]), _branches(kind, got[off])):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'cached frame loop != clip mode at frame %d' % off
        # A = 2: the flip pair
        x = [[c, model(img=torch.flip(f, dims=[3]), img_meta=[dict(meta, flip=True)], backbone_feat=True)[0]] for c, f in zip(c4[:T], frames[:T])]
        nested = [[dict(meta), dict(meta, flip=True)] for _ in range(T)]
        rec.calls = []
        aug = model(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True)
        check_windows([_branches(kind, aug)], rec, '%s forward_feat_aug A=2' % kind)


FT, FN = 15, 300


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('nms', [LINEAR, GAUSSIAN], ids=['linear', 'gaussian'])
def test_full_size_window_with_soft_nms(nms, dtype):
    """T = 15, N = 300, one benchmark clip (608 x 1008): restatement on the window's own decoded scores; deferred == immediate; a window
    captured into a hipGraph and replayed == eager bit for bit (capture succeeding = the path holds no host read); in f32 a call with
    4 clips == the four single calls."""
    model = hvrnet_amd.build_model(hvr_config(frame_interval=FT // 2, nms_post=FN), S.synth_state_dict('hvr'), dtype, DEV)
    model.test_cfg.rcnn.nms = dict(nms)
    metas = [S.synth_meta() for _ in range(FT)]
    n_clips = 4 if dtype == torch.float32 else 2
    clips = [torch.cat([S.synth_frame(100 * c + i) for i in range(FT)], 0).to(DEV) for c in range(n_clips)]
    with torch.no_grad():
        c4 = [model(img=clip, img_meta=metas, backbone_feat=True)[0] for clip in clips]
        with Recorder(model) as rec:
            eager = model(x=c4[0], img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
            check_windows([list(eager)], rec, 'full size %s' % str(dtype))
        pend = model(x=c4[0], img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True, defer=True)
        later = pend.result()
        assert not pend.respeculated
        for a, b in zip(eager, later):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'deferred != immediate'
        g = GraphedClip(model, clips[0], metas, rescale=True)
        for c in (1, 0):
            p = g.run(clips[c])
            got = p.result()
            assert not p.respeculated
            want = model(x=c4[c], img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
            for a, b in zip(got, want):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'graph replay != eager (clip %d)' % c
        if dtype == torch.float32:
            singles = [model(x=x, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True) for x in c4]
            model.bbox_head.grouped_exact = True       # the relation core's sums in the per-clip association (bbox_heads.py)
            with Recorder(model) as rec:
                batch = model.forward_feat_clips(torch.cat(c4, 0), metas * n_clips, n_clips, rescale=True)
                check_windows([list(batch[w]) for w in range(n_clips)], rec, 'clips = %d call' % n_clips, batched=True)
            for w in range(n_clips):
                for a, b in zip(batch[w], singles[w]):
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'clips=%d call != single call (clip %d)' % (n_clips, w)
