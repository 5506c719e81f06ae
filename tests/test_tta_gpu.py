"""Multi-scale / flip test-time augmentation on the GPU: the new kernels against the reference's recorded outputs
(tests/golden/g18_merge_augs.npz, g19_tta_config1.npz) and against the plain-torch restatement (tests/tta_refs.py), and the
detector path `forward_feat_aug` end to end.  Nothing here reads the reference tree.

Error bars are derived from the number format: a mapped-back coordinate differs from the recorded one by at most the rounding
of one division (1 ulp, `np.spacing`), an averaged box by (A + 2) ulp of the largest coordinate (un-flip, division, A - 1
additions, one division), an averaged score by (A + 1) ulp of 1.0.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import box_ops, native, parity, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config, selsa_config  # noqa: E402
from hvrnet_amd.pipelines import FrameIngest, FrameIngestAug, rescale_size  # noqa: E402
from hvrnet_amd.window import VideoWindowRunner  # noqa: E402
from tests import tta_refs as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def gold(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


def _metas(g, prefix):
    return [dict(img_shape=(int(h), int(w), 3), scale_factor=float(s), flip=bool(f))
            for h, w, s, f in zip(g[prefix + '_img_h'], g[prefix + '_img_w'], g[prefix + '_scale'], g[prefix + '_flip'])]


def _aug_lists(metas):
    return [m['img_shape'][1] for m in metas], [m['scale_factor'] for m in metas], [m['flip'] for m in metas]


def _stack_props(props_per_frame, mx):
    """[frame][aug] lists of [n,5] -> (proposals [A,T,mx,5], counts [A,T]) on the device."""
    T, A = len(props_per_frame), len(props_per_frame[0])
    out = torch.zeros((A, T, mx, 5))
    cnt = torch.zeros((A, T), dtype=torch.int32)
    for t, augs in enumerate(props_per_frame):
        for a, p in enumerate(augs):
            out[a, t, :p.shape[0]] = p
            cnt[a, t] = p.shape[0]
    return out.to(DEV), cnt.to(DEV)


def _check_merged(got, want, src, props, metas, what):
    """rows and order exact (scores are the source rows' scores, bit for bit); coordinates exact where the source augmentation
    has scale_factor 1, within one ulp of the coordinate elsewhere.  -> largest deviation in ulp."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, '%s: %s rows, expected %s' % (what, got.shape, want.shape)
    assert np.array_equal(got[:, 4].view(np.uint32), want[:, 4].view(np.uint32)), '%s: other source boxes / order' % what
    bounds = np.cumsum([0] + [p.shape[0] for p in props])
    aug = np.searchsorted(bounds, np.asarray(src), side='right') - 1
    scale = np.array([metas[a]['scale_factor'] for a in aug])
    exact = scale == 1.0
    assert np.array_equal(got[exact, :4], want[exact, :4]), '%s: scale-1 rows must be bit-identical' % what
    ulp = np.spacing(np.abs(want[:, :4]).astype(np.float32))
    dev = np.abs(got[:, :4].astype(np.float64) - want[:, :4].astype(np.float64))
    worst = float(np.max(np.where(ulp > 0, dev / np.where(ulp > 0, ulp, 1), 0.0))) if got.size else 0.0
    assert np.all(dev <= ulp), '%s: a coordinate is %.2f ulp off (bar: 1 ulp, one division)' % (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------ 1. ingest
@pytest.mark.parametrize('src_hw,scale', [((720, 1280), (1000, 600)), ((600, 1000), (1000, 600)), ((480, 854), (801, 481)),
                                          ((375, 500), (800, 480)), ((97, 131), (333, 200))])
def test_ingest_flip_mirrors_before_padding(src_hw, scale):
    """hvr_ingest_frame_flip: flip=0 is hvr_ingest_frame bit for bit; flip=1 is that result with the [:new_h, :new_w] region mirrored
    and zero padding on the right / at the bottom.  Sizes include an odd new_w (450 x 801) and new_w == pad_w (1000, 640)."""
    g = torch.Generator().manual_seed(src_hw[0] * 7 + src_hw[1])
    frame = torch.randint(0, 256, (src_hw[0], src_hw[1], 3), generator=g, dtype=torch.uint8).to(DEV)
    nh, nw, _ = rescale_size(src_hw[0], src_hw[1], scale)
    ph, pw = -(-nh // 16) * 16, -(-nw // 16) * 16
    mean, std = (103.06, 115.90, 123.15), (1.0, 1.0, 1.0)
    plain = native.ingest_frame(frame, (nh, nw), (ph, pw), mean, std, False)
    same = native.ingest_frame(frame, (nh, nw), (ph, pw), mean, std, False, flip=False)
    flipped = native.ingest_frame(frame, (nh, nw), (ph, pw), mean, std, False, flip=True)
    assert torch.equal(plain, same)
    want = torch.zeros_like(plain)
    want[:, :, :nh, :nw] = torch.flip(plain[:, :, :nh, :nw], dims=[3])
    assert torch.equal(flipped, want)
    assert not flipped[:, :, nh:, :].any() and not flipped[:, :, :, nw:].any()
    out = FrameIngest(img_scale=scale, flip=True, device=DEV)(frame)
    assert out['img_meta']['flip'] is True and torch.equal(out['img'], flipped)


def test_ingest_flip_sizes_cover_odd_and_unpadded_width():
    sizes = [rescale_size(h, w, s) for (h, w), s in [((720, 1280), (1000, 600)), ((600, 1000), (1000, 600)), ((480, 854), (801, 481)),
                                                       ((375, 500), (800, 480)), ((97, 131), (333, 200))]]
    assert any(nw % 2 == 1 for _, nw, _ in sizes) and any(nw % 16 == 0 for _, nw, _ in sizes) and any(nw % 16 for _, nw, _ in sizes)


def test_frame_ingest_aug_order_and_single_upload():
    frame = torch.randint(0, 256, (720, 1280, 3), dtype=torch.uint8)
    aug = FrameIngestAug(img_scale=[(1000, 600), (800, 480)], flip=True, device=DEV)
    out = aug(frame)
    assert [(m['img_shape'][1], m['flip']) for m in out['img_meta']] == [(1000, False), (1000, True), (800, False), (800, True)]
    for a in (0, 2):
        nh, nw = out['img_meta'][a]['img_shape'][:2]
        assert torch.equal(out['img'][a + 1][:, :, :nh, :nw], torch.flip(out['img'][a][:, :, :nh, :nw], dims=[3]))
    one = FrameIngest(img_scale=(800, 480), device=DEV)(frame)
    assert torch.equal(one['img'], out['img'][2])


# ------------------------------------------------------------------------------------------- 2. merge_aug_proposals
def test_merge_aug_proposals_matches_reference_golden():
    """Every G18 case through hvr_merge_aug_proposals and through box_ops.merge_aug_proposals.
    Measured on MI355X: 0 ulp in every case (the division rounds as the recording host's)."""
    g = gold('g18_merge_augs')
    thr = float(g['mp_nms_thr'])
    for name in [str(n) for n in g['mp_names']]:
        metas = _metas(g, 'mp_' + name)
        props = [torch.as_tensor(g['mp_%s_props_%d' % (name, a)]) for a in range(len(metas))]
        max_num = int(g['mp_%s_max_num' % name])
        want, src = g['mp_%s_merged' % name], g['mp_%s_src' % name]
        mx = max(p.shape[0] for p in props)
        P, Cn = _stack_props([props], mx)
        merged, cnt = native.merge_aug_proposals(P, Cn, *_aug_lists(metas), thr, max_num)
        k = int(cnt.item())
        assert k == want.shape[0]
        assert not merged[0, k:].any()
        worst = _check_merged(merged[0, :k].cpu().numpy(), want, src, props, metas, name)
        print('merge_aug_proposals %s: %d rows, worst coordinate deviation %.2f ulp' % (name, k, worst))
        api = box_ops.merge_aug_proposals([p.to(DEV) for p in props], metas, dict(nms_thr=thr, max_num=max_num))
        assert torch.equal(api, merged[0, :k])


def test_merge_aug_proposals_batched_window():
    """T = 15 frames, A = 4, mx = 300 in one launch: equals the helper frame by frame and T single-frame launches bit for bit;
    one frame has an augmentation that kept fewer rows, one frame (60 boxes per augmentation) merges to fewer than max_num."""
    metas = R.aug_metas((600, 1000), (1.0, 0.8), True)
    T, mx, thr = 15, 300, 0.7
    frames = []
    for t in range(T):
        kw = dict(short=(1, 211)) if t == 4 else {}
        frames.append(R.random_case(5000 + 200 * t, metas, 60 if t == 9 else mx, thr, mx, **kw)[1])
    P, Cn = _stack_props(frames, mx)
    merged, cnt = native.merge_aug_proposals(P, Cn, *_aug_lists(metas), thr, mx)
    counts = cnt.tolist()
    worst = 0.0
    for t in range(T):
        want, src = R.merge_aug_proposals(frames[t], metas, thr, mx, return_index=True)
        assert counts[t] == want.shape[0]
        worst = max(worst, _check_merged(merged[t, :counts[t]].cpu().numpy(), want.numpy(), src.numpy(), frames[t], metas, 'frame %d' % t))
        assert not merged[t, counts[t]:].any()
        one, c1 = native.merge_aug_proposals(P[:, t:t + 1].contiguous(), Cn[:, t:t + 1].contiguous(), *_aug_lists(metas), thr, mx)
        assert int(c1.item()) == counts[t] and torch.equal(one[0], merged[t])
    assert counts[9] < mx, 'the 4 x 60-box frame merges to fewer than max_num proposals'
    print('merge_aug_proposals batched: counts %s, worst coordinate deviation %.2f ulp' % (counts, worst))


def test_merge_aug_proposals_rejects_more_than_8192_boxes():
    P = torch.zeros((9, 1, 1000, 5), device=DEV)
    Cn = torch.zeros((9, 1), dtype=torch.int32, device=DEV)
    with pytest.raises(native.HvrError, match='8192'):
        native.merge_aug_proposals(P, Cn, [1000] * 9, [1.0] * 9, [False] * 9, 0.7, 300)


# ----------------------------------------------------------------------------- 3. map_aug_rois / merge_aug_dets
def test_box_mappings_match_reference_golden():
    g = gold('g18_merge_augs')
    b = torch.as_tensor(g['tr_boxes']).to(DEV)
    shape, s = tuple(int(v) for v in g['tr_img_shape']), float(g['tr_scale'])
    for got, key in ((box_ops.bbox_flip(b, shape), 'tr_flip'), (box_ops.bbox_flip(b.reshape(32, 8), shape), 'tr_flip8'),
                     (box_ops.bbox_mapping(b, shape, s, False), 'tr_map'), (box_ops.bbox_mapping(b, shape, s, True), 'tr_map_flip'),
                     (box_ops.bbox_mapping_back(b, shape, s, False), 'tr_back'), (box_ops.bbox_mapping_back(b, shape, s, True), 'tr_back_flip')):
        want = g[key]
        ulp = np.spacing(np.float32(np.abs(want).max()))
        dev = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
        print('%s: max deviation %.3g (%.2f ulp of the largest coordinate)' % (key, dev, dev / ulp))
        assert got.shape == want.shape and dev <= 3 * ulp      # the A = 1 case of the (A + 2) ulp bar; flips alone are exact
        if key.startswith('tr_flip'):
            assert np.array_equal(got.cpu().numpy(), want)


def _det_metas(A):
    if A == 1:
        return R.aug_metas((600, 1000), (1.0,), False)
    return R.aug_metas((600, 1000), {2: (1.0,), 4: (1.0, 0.8), 6: (1.0, 0.8, 1.2)}[A], True)


@pytest.mark.parametrize('A', [1, 2, 4, 6])
def test_map_rois_and_merge_dets_match_helper(A):
    """R = 300, 31 classes.  A = 1 without flip at scale 1 is the identity bit for bit; otherwise boxes within (A + 2) ulp of the
    largest coordinate, scores within (A + 1) ulp of 1.0.  Measured on MI355X: 0 ulp for boxes, rois and scores at every A."""
    metas = _det_metas(A)
    Rn, ncls, T = 300, 31, 3
    boxes, scores = R.random_dets(77 + A, metas, Rn, ncls)
    mb, ms = native.merge_aug_dets(torch.stack(boxes).to(DEV), torch.stack(scores).to(DEV), *_aug_lists(metas))
    wb, ws = R.merge_aug_bboxes(boxes, scores, [[m] for m in metas])
    if A == 1:
        assert torch.equal(mb.cpu(), boxes[0]) and torch.equal(ms.cpu(), scores[0])
    ulp_b = float(np.spacing(np.float32(wb.abs().max().item())))
    ulp_s = float(np.spacing(np.float32(1.0)))
    db = (mb.cpu().double() - wb.double()).abs().max().item()
    ds = (ms.cpu().double() - ws.double()).abs().max().item()
    print('merge_aug_dets A=%d: boxes %.2f ulp, scores %.2f ulp' % (A, db / ulp_b, ds / ulp_s))
    assert db <= (A + 2) * ulp_b and ds <= (A + 1) * ulp_s
    api_b, api_s = box_ops.merge_aug_bboxes([b.to(DEV) for b in boxes], [s.to(DEV) for s in scores], [[m] for m in metas], None)
    assert torch.equal(api_b, mb) and torch.equal(api_s, ms)
    assert torch.equal(box_ops.merge_aug_scores([s.to(DEV) for s in scores]), ms)
    # bbox_mapping + bbox2roi of T frames' merged proposals into every augmentation
    merged = torch.stack([torch.cat([wb, ws[:, :1]], 1)] * T)
    merged[1, :, :4] += 0.37
    rois = native.map_aug_rois(merged.to(DEV), *_aug_lists(metas))
    assert rois.shape == (A, T * Rn, 5)
    worst = 0.0
    for a, m in enumerate(metas):
        want = torch.cat([torch.cat([torch.full((Rn, 1), float(t)), R.bbox_mapping(merged[t, :, :4], m['img_shape'], m['scale_factor'], m['flip'])], 1)
                          for t in range(T)], 0)
        got = rois[a].cpu()
        assert torch.equal(got[:, 0], want[:, 0])
        if A == 1:
            assert torch.equal(got, want)
        ulp = float(np.spacing(np.float32(want[:, 1:].abs().max().item())))
        worst = max(worst, (got[:, 1:].double() - want[:, 1:].double()).abs().max().item() / ulp)
    print('map_aug_rois A=%d: %.2f ulp' % (A, worst))
    assert worst <= A + 2


def test_merge_aug_bboxes_matches_reference_golden():
    g = gold('g18_merge_augs')
    for name in ('a4', 'a2'):
        metas = _metas(g, 'mb_' + name)
        A = len(metas)
        mb, ms = native.merge_aug_dets(torch.as_tensor(g['mb_%s_boxes' % name]).to(DEV), torch.as_tensor(g['mb_%s_scores' % name]).to(DEV),
                                       *_aug_lists(metas))
        wb, ws = g['mb_%s_merged_boxes' % name], g['mb_%s_merged_scores' % name]
        ulp_b, ulp_s = float(np.spacing(np.float32(np.abs(wb).max()))), float(np.spacing(np.float32(1.0)))
        db = np.abs(mb.cpu().numpy().astype(np.float64) - wb).max()
        ds = np.abs(ms.cpu().numpy().astype(np.float64) - ws).max()
        print('merge_aug_bboxes %s vs reference: boxes %.2f ulp, scores %.2f ulp' % (name, db / ulp_b, ds / ulp_s))
        assert db <= (A + 2) * ulp_b and ds <= (A + 1) * ulp_s
        assert np.abs(ms.cpu().numpy().astype(np.float64) - g['mb_%s_merged_scores_only' % name]).max() <= (A + 1) * ulp_s


# ------------------------------------------------------------------------------------------------ 4-9. the detector path
@pytest.fixture(scope='module')
def O():
    import subprocess
    if not os.path.exists(os.path.join(ROOT, 'oracle', 'libhvr_oracle.so')):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'oracle')], check=True)
    from oracle import hvr_oracle
    return hvr_oracle


def close(a, b, rtol, atol):
    torch.testing.assert_close(torch.as_tensor(np.asarray(a.detach().float().cpu() if isinstance(a, torch.Tensor) else a)).float(),
                               torch.as_tensor(np.asarray(b.detach().float().cpu() if isinstance(b, torch.Tensor) else b)).float(),
                               rtol=rtol, atol=atol)


def _g19_inputs(g, T=3):
    """The frames G19 was recorded on, rebuilt from the seed: per augmentation (scale outer, flip inner) T frames and metas."""
    imgs, metas = [], []
    for a in range(len(g['img_w'])):
        ih, iw, ph, pw = int(g['img_h'][a]), int(g['img_w'][a]), int(g['pad_h'][a]), int(g['pad_w'][a])
        fr = []
        for i in range(T):
            im = S.synth_frame(i, seed=int(g['frame_seed']), img_hw=(ih, iw), pad_hw=(ph, pw))
            if bool(g['flip'][a]):
                im = im.clone()
                im[:, :, :ih, :iw] = torch.flip(im[:, :, :ih, :iw], dims=[3])
            fr.append(im)
        imgs.append(fr)
        metas.append([dict(ori_shape=(600, 1000, 3), img_shape=(ih, iw, 3), pad_shape=(ph, pw, 3), scale_factor=float(g['scale'][a]),
                           flip=bool(g['flip'][a])) for _ in range(T)])
    return imgs, metas


def _nested(model, imgs, metas):
    """-> (x[t][a] C4 maps, img_meta[t][a]) through the detector's own backbone_feat entry with a list of images."""
    A, T = len(imgs), len(imgs[0])
    x, nested = [], []
    for t in range(T):
        feats = model(img=[imgs[a][t].to(DEV) for a in range(A)], img_meta=[metas[a][t] for a in range(A)], backbone_feat=True)
        x.append([f[0] for f in feats])
        nested.append([metas[a][t] for a in range(A)])
    return x, nested


def _flat(res):
    """bbox2result list -> (labels, [n,5] rows) in class order."""
    return np.concatenate([np.full(len(r), i) for i, r in enumerate(res)]), np.concatenate([np.asarray(r).reshape(-1, 5) for r in res], 0)


def _check_dets(res, want_b, want_l, what):
    labels, rows = _flat(res)
    want_b, want_l = np.asarray(want_b), np.asarray(want_l)
    order = np.argsort(want_l, kind='stable')              # bbox2result groups by class, keeping the in-class order
    assert labels.tolist() == want_l[order].tolist(), '%s: class indices differ' % what
    es = np.abs(rows[:, 4] - want_b[order][:, 4]).max()
    eb = np.abs(rows[:, :4] - want_b[order][:, :4]).max()
    print('%s: %d detections, max score err %.3g, max box err %.3g px (bars 1e-3, %.3g)' % (what, len(labels), es, eb, parity.box_bar(1000.0)))
    close(rows[:, 4], want_b[order][:, 4], 0, 1e-3)
    close(rows[:, :4], want_b[order][:, :4], 0, parity.box_bar(1000.0))


def test_tta_config1_end_to_end_matches_reference_golden(O):
    """G19: HNMBRCNN.forward_feat_aug of the reference, T = 3, key frame 1, 32 proposals, A = 4 (1000 x 600 and 800 x 480, flip off /
    on), f32.  (a) the fixture's merged proposals through aug_test_bboxes, (b) the whole call with nothing injected; both branches;
    SelsaRCNN against the composed helper; rescale=False = rescale=True times aug 0's scale_factor.
    Measured on MI355X (bars: scores 1e-3, boxes 2.3e-3 px): (a) scores 1.3e-6 / 5.1e-7, boxes 1.8e-4 / 2.4e-4 px; (b) scores 1.4e-6 /
    1.2e-6, boxes 1.5e-3 / 1.7e-3 px; SelsaRCNN scores 4.3e-7, boxes 4.5e-4 px; class indices exact everywhere."""
    g = gold('g19_tta_config1')
    assert not bool(g['composed'])
    imgs, metas = _g19_inputs(g)
    model = hvrnet_amd.build_model(hvr_config(frame_interval=1, nms_post=32), S.synth_state_dict('hvr'), torch.float32, DEV)
    with torch.no_grad():
        x, nested = _nested(model, imgs, metas)
        feats, img_metas = model._aug_split(x, nested)
        # (a) from the reference's merged proposals
        c5 = model.aug_shared_feats(feats, img_metas)
        dets, labels = model.aug_test_bboxes(c5, img_metas, [torch.as_tensor(p).to(DEV) for p in g['merged']], model.test_cfg.rcnn)
        for b in range(2):
            _check_dets(box_ops.bbox2result(dets[b], labels[b], 31), g['det_bboxes_%d' % b], g['det_labels_%d' % b], 'G19 (a) branch %d' % b)
        # (b) nothing injected
        props, counts = model.aug_test_rpn(feats, img_metas)
        assert counts.tolist() == [[32] * 3] * 4
        close(props, g['props'], 1e-4, 2e-2)
        merged, mcounts = model.aug_test_rpn_merged(feats, img_metas)
        assert mcounts.tolist() == [32] * 3
        close(merged, g['merged'], 1e-4, 2e-2)
        pend = model(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True, defer=True)
        results = pend.result()
        assert not pend.respeculated and len(results) == 2
        for b in range(2):
            _check_dets(results[b], g['det_bboxes_%d' % b], g['det_labels_%d' % b], 'G19 (b) branch %d' % b)
        # rescale=False: the reference multiplies by img_metas[0][0]['scale_factor'] -- put the 0.8 augmentations first
        xr, nr = [list(reversed(f)) for f in x], [list(reversed(m)) for m in nested]
        up = model(x=xr, img=None, img_meta=nr, forward_feat=True, return_loss=False, rescale=True)
        down = model(x=xr, img=None, img_meta=nr, forward_feat=True, return_loss=False, rescale=False)
        assert nr[0][0]['scale_factor'] == 0.8
        for b in range(2):
            for u, d in zip(up[b], down[b]):
                assert np.array_equal(d[:, 4], u[:, 4]) and np.array_equal(d[:, :4], u[:, :4] * np.float32(0.8))
        # SelsaRCNN (one branch) against the CPU composition on the same C4 maps
        sd = S.synth_state_dict('selsa')
        ms = hvrnet_amd.build_model(selsa_config(frame_interval=1, nms_post=32), sd, torch.float32, DEV)
        res = ms(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True)
        c4_cpu = [f.float().cpu().contiguous() for f in feats]
        want, inter = R.aug_window_forward(O, c4_cpu, img_metas, sd, 'selsa', 1, 32, 3, dict(O.RPN_TEST_CFG, nms_post=32, max_num=32), O.RCNN_TEST_CFG)
        assert len(res) == 30
        _check_dets(res, inter['dets'][0][0].numpy(), inter['dets'][0][1].numpy(), 'SelsaRCNN vs the composed helper')


def test_tta_single_augmentation_equals_forward_feat():
    """A = 1, no flip, scale 1: forward_feat_aug = forward_feat on G10's frames (the merge NMS at 0.7 removes nothing from one
    augmentation's already-NMSed proposals; mapping and averaging are identities)."""
    T = 3
    imgs = [S.synth_frame(i).to(DEV) for i in range(T)]
    metas = [S.synth_meta() for _ in range(T)]
    model = hvrnet_amd.build_model(hvr_config(frame_interval=1, nms_post=32), S.synth_state_dict('hvr'), torch.float32, DEV)
    with torch.no_grad():
        c4 = [model(img=im, img_meta=[m], backbone_feat=True)[0] for im, m in zip(imgs, metas)]
        plain = model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
        aug = model(x=[[c] for c in c4], img=None, img_meta=[[m] for m in metas], forward_feat=True, return_loss=False, rescale=True)
    for b in range(2):
        lp, rp = _flat(plain[b])
        _check_dets(aug[b], rp, lp, 'A = 1 branch %d' % b)


def _small_model_and_window(dtype=torch.float32, seed=3):
    model = hvrnet_amd.build_model(hvr_config(frame_interval=1, nms_post=32), S.synth_state_dict('hvr'), dtype, DEV)
    metas = []
    imgs = []
    for flip in (False, True):
        fr = []
        for i in range(3):
            im = S.synth_frame(i, seed=seed, img_hw=(480, 800), pad_hw=(480, 800))
            fr.append(torch.flip(im, dims=[3]) if flip else im)
        imgs.append(fr)
        metas.append([dict(ori_shape=(600, 1000, 3), img_shape=(480, 800, 3), pad_shape=(480, 800, 3), scale_factor=0.8, flip=flip) for _ in range(3)])
    with torch.no_grad():
        x, nested = _nested(model, imgs, metas)
    return model, x, nested


def test_tta_short_frame_respeculates_to_the_exact_result():
    """A flip pair whose frame 0 carries few, heavily overlapping proposals: its merged count is below max_num, the speculative
    window is discarded when the counts arrive (`respeculated`) and the result is the exact, ragged path's."""
    model, x, nested = _small_model_and_window()
    real = model.aug_test_rpn

    def few(feats, img_metas, group_maps=None):
        props, counts = real(feats, img_metas, group_maps)
        props = props.clone()
        props[:, 0, 5:] = props[:, 0, :1] + torch.arange(27, device=props.device).view(1, 27, 1) * 1e-3   # 27 copies of the best box
        props[:, 0, 5:, 4] = props[:, 0, 5:6, 4] * 0.5
        return props, counts

    model.aug_test_rpn = few
    try:
        with torch.no_grad():
            pend = model(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True, defer=True)
            got = pend.result()
            merged, mcounts = model.aug_test_rpn_merged(*model._aug_split(x, nested))
            exact = model.forward_feat_aug(x, nested, rescale=True, speculate=False)
    finally:
        del model.aug_test_rpn
    assert mcounts.tolist()[0] < 32, mcounts.tolist()
    assert pend.respeculated
    for b in range(2):
        for a_, b_ in zip(got[b], exact[b]):
            assert np.array_equal(a_, b_)
    with torch.no_grad():      # unpatched: the window is re-run exactly when some frame merged to fewer than max_num proposals
        normal = model(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True, defer=True)
        normal.result()
        _, plain_counts = model.aug_test_rpn_merged(*model._aug_split(x, nested))
    print('short frame: merged counts %s (patched), %s (as ingested)' % (mcounts.tolist(), plain_counts.tolist()))
    assert normal.respeculated == (min(plain_counts.tolist()) < 32)


def test_tta_deferred_window_reads_nothing_back():
    """forward_feat_aug(defer=True) enqueues the window without a host synchronisation, as forward_feat(defer=True) does: both run
    under torch's sync debug mode 'error'."""
    model, x, nested = _small_model_and_window(torch.bfloat16)
    flat_x, flat_m = [f[0] for f in x], [m[0] for m in nested]
    with torch.no_grad():
        model.forward_feat(flat_x, flat_m, rescale=True)            # warm-up: workspaces, streams, packed weights
        model.forward_feat_aug(x, nested, rescale=True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            p0 = model.forward_feat(flat_x, flat_m, rescale=True, defer=True)
            p1 = model.forward_feat_aug(x, nested, rescale=True, defer=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert len(p0.result()) == 2 and len(p1.result()) == 2


def test_tta_video_window_runner_emits_forward_feat_aug():
    """7-frame synthetic video, window 3, the flip pair of one scale per frame: the runner's results equal forward_feat_aug called by
    hand on the same windows, padded first / last windows included."""
    from hvrnet_amd.window import window_frames
    model = hvrnet_amd.build_model(hvr_config(frame_interval=1, nms_post=32), S.synth_state_dict('hvr'), torch.float32, DEV)
    n = 7
    frames, metas = [], []
    for i in range(n):
        im = S.synth_frame(i, seed=5, img_hw=(480, 800), pad_hw=(480, 800)).to(DEV)
        frames.append([im, torch.flip(im, dims=[3])])
        metas.append([dict(ori_shape=(600, 1000, 3), img_shape=(480, 800, 3), pad_shape=(480, 800, 3), scale_factor=0.8, flip=f) for f in (False, True)])
    with torch.no_grad():
        got = VideoWindowRunner(model, 3, rescale=True).run_video(frames, metas)
        c4 = [[f[0] for f in model(img=frames[i], img_meta=metas[i], backbone_feat=True)] for i in range(n)]
        wins = window_frames(n, 3)
        assert sorted(got) == list(range(n)) == sorted(wins)
        assert wins[0] == [0, 0, 1] and wins[n - 1] == [n - 2, n - 1, n - 1]
        for off, ids in wins.items():
            want = model.forward_feat_aug([c4[i] for i in ids], [metas[i] for i in ids], rescale=True)
            for b in range(2):
                for a_, b_ in zip(got[off][b], want[b]):
                    assert np.array_equal(a_, b_), 'frame %d' % off
    with pytest.raises(NotImplementedError):
        VideoWindowRunner(model, 3, cache_frames=True).step(frames[0], metas[0], 0, 0)


# ------------------------------------------------------------------------------------------------------- 6. full size
FT, FN = 15, 300
FULL_SCALES = [((600, 1000), (608, 1008), 1.0), ((480, 800), (480, 800), 0.8)]
SPLIT = native.SPLIT


def _full_frames(seed=0):
    imgs, metas = [], []
    for img_hw, pad_hw, s in FULL_SCALES:
        for flip in (False, True):
            fr = []
            for i in range(FT):
                im = S.synth_frame(i, seed=seed, img_hw=img_hw, pad_hw=pad_hw)
                if flip:
                    im = im.clone()
                    im[:, :, :img_hw[0], :img_hw[1]] = torch.flip(im[:, :, :img_hw[0], :img_hw[1]], dims=[3])
                fr.append(im)
            imgs.append(fr)
            metas.append([dict(ori_shape=(600, 1000, 3), img_shape=img_hw + (3,), pad_shape=pad_hw + (3,), scale_factor=s, flip=flip) for _ in range(FT)])
    return imgs, metas


@pytest.fixture(scope='module')
def full_clip(O):
    """One synthetic clip at T = 15, 608 x 1008 and 480 x 800, flip off / on, and the CPU composition of its augmented window
    (oracle.clip_forward's stages + tests/tta_refs.py); the oracle's 60 backbone frames run once per module."""
    imgs, metas = _full_frames()
    sd = S.synth_state_dict('hvr')
    with torch.no_grad():
        c4 = [torch.cat([O.resnet_c4(f, sd) for f in imgs[a]], 0) for a in range(len(imgs))]
        want, inter = R.aug_window_forward(O, c4, metas, sd, 'hvr', FT // 2, FN, FT, dict(O.RPN_TEST_CFG, nms_post=FN, max_num=FN), O.RCNN_TEST_CFG)
    return dict(imgs=imgs, metas=metas, sd=sd, want=want, inter=inter)


@pytest.mark.parametrize('dtype', [torch.float32, SPLIT], ids=['f32', 'f16x2'])
def test_tta_full_size_window_matches_the_cpu_composition(O, full_clip, dtype):
    """T = 15, mx = 300, A = 4 (608 x 1008 and 480 x 800, flip off / on) in the two modes that carry the tolerance, judged by the frozen
    rule of hvrnet_amd/parity.py: classes exact, scores within 1e-3, boxes within 1e-3 px + 1.3e-6 x extent of the CPU composition; a
    frame whose merged proposal list differs from the CPU's has to be an NMS pair within NMS_TIE_BAND of the threshold, and the window
    with the CPU's merged proposals injected has to be inside the bar.
    Measured on MI355X (synthetic clip 0): all 15 merged lists equal the CPU's in both modes (no tie to judge), 300 merged proposals per
    frame; f32: scores within 1.4e-6, boxes within 7.9e-4 / 7.5e-4 px (branch / final); f16x2: scores within 1.5e-6, boxes within
    1.53e-3 / 7.8e-4 px against the 2.30e-3 px bar at the 998 px extent; with the CPU's merged proposals injected 1.8e-4 / 3.1e-4 px."""
    model = hvrnet_amd.build_model(hvr_config(frame_interval=FT // 2, nms_post=FN), full_clip['sd'], dtype, DEV)
    with torch.no_grad():
        x, nested = _nested(model, full_clip['imgs'], full_clip['metas'])
        feats, img_metas = model._aug_split(x, nested)
        merged, counts = model.aug_test_rpn_merged(feats, img_metas)
        got = model(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True)
        counts = counts.tolist()
        got_m = [merged[t, :counts[t]].cpu().numpy() for t in range(FT)]
        want_m = [m.numpy() for m in full_clip['inter']['merged']]
        same = parity.proposal_lists_equal(got_m, want_m)
        stats = [parity.strict(g_, w_) for g_, w_ in zip(got, full_clip['want'])]
        ties = parity.nms_threshold_ties(got_m, want_m)
        dets, labels = model.aug_test_bboxes(model.aug_shared_feats(feats, img_metas), img_metas, [m.to(DEV) for m in full_clip['inter']['merged']],
                                             model.test_cfg.rcnn)
        injected = [parity.strict(box_ops.bbox2result(d, l, 31), w_) for d, l, w_ in zip(dets, labels, full_clip['want'])]
    print('\n[tta full size %s] merged counts %s; frames whose merged list differs: %s; ties: %s; read-out: %s; with the CPU merged proposals '
          'injected: %s' % ('f32' if dtype == torch.float32 else 'f16x2', counts, [i for i, s_ in enumerate(same) if not s_],
                            [(t_['frame'], t_['iou'], t_['is_tie']) for t_ in ties], stats, injected))
    for st in injected:
        assert st['n'] > 0 and parity.within_tolerance(st), st
    assert all(t_['is_tie'] for t_ in ties), ties
    if all(same):
        for st in stats:
            assert st['n'] > 0 and parity.within_tolerance(st), st


def test_tta_full_size_window_bf16_is_well_formed(full_clip):
    """bf16, the benchmarked dtype: the augmented window runs and returns well-formed results (no tolerance claimed)."""
    model = hvrnet_amd.build_model(hvr_config(frame_interval=FT // 2, nms_post=FN), full_clip['sd'], torch.bfloat16, DEV)
    with torch.no_grad():
        x, nested = _nested(model, full_clip['imgs'], full_clip['metas'])
        res = model(x=x, img=None, img_meta=nested, forward_feat=True, return_loss=False, rescale=True)
    assert len(res) == 2
    for branch in res:
        assert len(branch) == 30 and 0 < sum(len(r) for r in branch) <= 300
        for r in branch:
            assert r.shape[1] == 5 and np.isfinite(r).all() and (r[:, 4] > 0.001).all() and (r[:, 4] <= 1).all()
            # delta2bbox's corners are centre -+ (size - 1) / 2 with size > 0: x2 - x1 > -1 (a box thinner than a pixel is inverted), and
            # clipping, the monotone mappings back and the mean keep that
            assert (r[:, 2] - r[:, 0] > -1).all() and (r[:, 3] - r[:, 1] > -1).all() and r[:, :4].min(initial=0) >= 0 and r[:, :4].max(initial=0) <= 1000
