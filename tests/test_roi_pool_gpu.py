"""GPU tests of RoIPool: the forward kernel (hvr_roi_pool_fwd, with and without the argmax) bit for bit against the statement of
tests/roi_pool_refs.py in bf16, f16 and f32, the split-half chain, the refusals, the argmax backward (exact on integer gradients, inside
the summation bound on normal ones), ops.roi_pool / ops.RoIPool as an autograd Function, an HVR window whose roi_layer is RoIPool
(eager / graphed, the cached per-frame path, two clips in one call, its RoI features against the statement) and the training entry
points that differentiate through it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config, selsa_config  # noqa: E402
from tests import roi_pool_refs as R  # noqa: E402
from tests.golden import cases as C  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
GUARD_ROWS = 8
SENTINEL = 7777
HVR_EINVAL, HVR_EUNSUPPORTED = -1, -2          # include/hvr_hip.h


def _feat(case, dtype):
    return torch.from_numpy(case['feat']).to(dtype).to(DEV).contiguous()


def _pool_guarded(feat, rois, PH, PW, with_argmax):
    """The kernel into sentinel-filled buffers with guard rows behind out (and argmax, allocated by the wrapper: checked for sentinels
    of its own kind, every element in [-1, H * W)).  -> (out, argmax or None)"""
    K, Cn = rois.shape[0], feat.shape[3]
    n = K * PH * PW * Cn
    buf = torch.full((n + GUARD_ROWS * PH * PW * Cn,), SENTINEL, dtype=feat.dtype, device=DEV)
    r = native.roi_pool_fwd(feat, rois, PH, PW, R.SCALE, with_argmax=with_argmax, out=buf[:n].view(K, PH, PW, Cn))
    torch.cuda.synchronize()
    out = r[0] if with_argmax else r
    assert out.data_ptr() == buf.data_ptr()
    assert not bool((out == SENTINEL).any()), 'an output element was not written'
    assert bool((buf[n:] == SENTINEL).all()), 'guard rows behind the output were written'
    return out, (r[1] if with_argmax else None)


def _argmax_guarded(feat, rois, PH, PW):
    """The C entry itself with a sentinel-filled, guarded argmax buffer."""
    K, Cn = rois.shape[0], feat.shape[3]
    n = K * PH * PW * Cn
    out = torch.empty((K, PH, PW, Cn), dtype=feat.dtype, device=DEV)
    abuf = torch.full((n + GUARD_ROWS * PH * PW * Cn,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = native.lib().hvr_roi_pool_fwd(native._ptr(feat), native._ptr(rois), native._ptr(out), native._ptr(abuf), feat.shape[0], feat.shape[1],
                                       feat.shape[2], Cn, K, PH, PW, R.SCALE, native._dt(feat), native._stream())
    assert rc == 0, native.lib().hvr_last_error()
    torch.cuda.synchronize()
    assert not bool((abuf[:n] == SENTINEL).any()), 'an argmax element was not written'
    assert bool((abuf[n:] == SENTINEL).all()), 'guard rows behind the argmax were written'
    return out, abuf[:n].view(K, PH, PW, Cn)


# ------------------------------------------------------------------------------------------------ forward vs statement
@pytest.mark.parametrize('mode', sorted(DTYPES))
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_forward_equals_the_statement_bit_for_bit(mode, name):
    case = R.make_case(name)
    feat, rois = _feat(case, DTYPES[mode]), torch.from_numpy(case['rois']).to(DEV)
    assert torch.equal(feat.double().cpu(), torch.from_numpy(case['feat']))            # the stored values ARE the statement's
    for (PH, PW) in R.OUT_SIZES:
        val, arg, rec = R.statement(name, PH, PW)
        want = torch.from_numpy(val).to(DTYPES[mode])
        plain, _ = _pool_guarded(feat, rois, PH, PW, False)
        with_arg, a1 = _pool_guarded(feat, rois, PH, PW, True)
        out2, a2 = _argmax_guarded(feat, rois, PH, PW)
        nbad = int((plain.cpu().view(torch.int16 if mode != 'f32' else torch.int32) != want.view(torch.int16 if mode != 'f32' else torch.int32)).sum())
        abad = int((a1.cpu() != torch.from_numpy(arg)).sum())
        print('%s %s %dx%d: %d of %d values and %d argmax differ; %d empty bins, largest bin %d px' % (
            name, mode, PH, PW, nbad, want.numel(), abad, int(rec['empty'].sum()), int(rec['area'].max())))
        assert nbad == 0 and abad == 0
        assert torch.equal(plain, with_arg) and torch.equal(plain, out2) and torch.equal(a1, a2)       # the two forms agree
        assert a1.dtype == torch.int32 and int(a1.min()) == -1 and int(a1.max()) < R.H * R.W


def test_split_half_maps_are_pooled_in_f32_and_handed_back_split():
    case = R.make_case('c64')
    rois = torch.from_numpy(case['rois']).to(DEV)
    f32 = _feat(case, torch.float32) * 1.0001220703125        # (x (1 + 2^-13): values that need the lo half)
    fs = native.cast(f32, SPLIT)
    assert fs.dtype == SPLIT
    back = native.cast(fs, torch.float32)
    want, want_arg = native.roi_pool_fwd(back, rois, 7, 7, R.SCALE, with_argmax=True)
    got = native.roi_pool_fwd(fs, rois, 7, 7, R.SCALE)
    got2, arg2 = native.roi_pool_fwd(fs, rois, 7, 7, R.SCALE, with_argmax=True)
    assert got.dtype == SPLIT and torch.equal(got, native.cast(want, SPLIT)) and torch.equal(got2, got) and torch.equal(arg2, want_arg)
    assert float(native.cast(got, torch.float32).abs().max()) > 0.3
    # through the module, as the window hands a split-half map over (logical NCHW over physical NHWC)
    y = ops.RoIPool(7, R.SCALE)(fs.permute(0, 3, 1, 2), rois)
    assert torch.equal(y.permute(0, 2, 3, 1), got)


def test_the_batch_index_selects_the_frame_and_no_rois_give_an_empty_result():
    case = R.make_case('c96')
    feat, rois = _feat(case, torch.bfloat16), torch.from_numpy(case['rois']).to(DEV)
    a, aa = native.roi_pool_fwd(feat, rois, 7, 7, R.SCALE, with_argmax=True)
    swapped = rois.clone()
    swapped[:, 0] = 1 - swapped[:, 0]                         # (-1 <-> 2: both stay outside [0, B))
    b, ba = native.roi_pool_fwd(feat.flip(0).contiguous(), swapped, 7, 7, R.SCALE, with_argmax=True)
    assert torch.equal(a, b) and torch.equal(aa, ba) and float(a.float().abs().max()) > 0.3
    e, ea = native.roi_pool_fwd(feat, rois[:0], 7, 7, R.SCALE, with_argmax=True)
    assert tuple(e.shape) == (0, 7, 7, 96) and tuple(ea.shape) == (0, 7, 7, 96) and ea.dtype == torch.int32
    assert tuple(native.roi_pool_fwd(feat, rois[:0], 2, 3, R.SCALE).shape) == (0, 2, 3, 96)
    g = native.roi_pool_bwd(torch.zeros((0, 7, 7, 96), device=DEV), rois[:0], ea, (2, 9, 11, 96))
    assert tuple(g.shape) == (2, 9, 11, 96) and not bool(g.any())


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_with_a_message_and_nothing_is_written():
    lib = native.lib()
    rois = torch.tensor([[0, 0.0, 0.0, 40.0, 40.0]], device=DEV)
    x36 = torch.zeros((1, 5, 5, 36), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(native.HvrError, match='C=36 is not a multiple of 8'):
        native.roi_pool_fwd(x36, rois, 3, 3, 1 / 16)
    x6 = torch.zeros((1, 5, 5, 6), dtype=torch.float32, device=DEV)
    with pytest.raises(native.HvrError, match='C=6 is not a multiple of 4'):
        native.roi_pool_fwd(x6, rois, 3, 3, 1 / 16)
    x = torch.zeros((1, 5, 5, 64), dtype=torch.float32, device=DEV)
    out = torch.full((1, 3, 3, 64), float(SENTINEL), device=DEV)
    arg = torch.full((1, 3, 3, 64), SENTINEL, dtype=torch.int32, device=DEV)
    P = native._ptr

    def fwd(B=1, H=5, W=5, Cn=64, K=1, PH=3, PW=3, dtype=native.HVR_F32):
        return lib.hvr_roi_pool_fwd(P(x), P(rois), P(out), P(arg), B, H, W, Cn, K, PH, PW, 1 / 16, dtype, native._stream())

    def bwd(B=1, H=5, W=5, Cn=64, K=1, PH=3, PW=3):
        return lib.hvr_roi_pool_bwd(P(out), P(rois), P(arg), P(x), B, H, W, Cn, K, PH, PW, native._stream())

    assert fwd(dtype=native.HVR_F16S) == HVR_EUNSUPPORTED and b'split-half' in lib.hvr_last_error()
    for kw in (dict(PH=0), dict(PW=-1), dict(H=0), dict(W=0), dict(Cn=0), dict(K=-1), dict(B=-1)):
        assert fwd(**kw) == HVR_EINVAL and b'hvr_roi_pool_fwd: bad shape' in lib.hvr_last_error(), kw
        assert bwd(**kw) == HVR_EINVAL and b'hvr_roi_pool_bwd: bad shape' in lib.hvr_last_error(), kw
    assert fwd(dtype=9) == HVR_EINVAL and b'bad dtype' in lib.hvr_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((arg == SENTINEL).all()) and not bool(x.any())      # no kernel ran
    assert fwd(K=0) == 0 and bwd(K=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((arg == SENTINEL).all())
    assert lib.hvr_abi_version() == 7


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('name', ['c8', 'c96', 'c256'])
def test_backward_equals_the_statement(name):
    case = R.make_case(name)
    Cn = case['C']
    feat, rois = _feat(case, torch.float32), torch.from_numpy(case['rois']).to(DEV)
    for (PH, PW) in R.OUT_SIZES:
        val, arg, rec = R.statement(name, PH, PW)
        argd = torch.from_numpy(arg).to(DEV)
        # small integers: every sum is exact in f32, whatever order the atomics land in
        go = R.grad_out_ints(arg.shape, 31)
        want, n, sabs = R.backward_statement(go, case['rois'], arg, R.B, R.H, R.W)
        assert sabs.max() < 2 ** 24 and n.max() > 1
        got = native.roi_pool_bwd(torch.from_numpy(go).float().to(DEV), rois, argd, (R.B, R.H, R.W, Cn))
        assert got.dtype == torch.float32 and torch.equal(got.double().cpu(), torch.from_numpy(want))
        # seeded normal gradients: (n - 1) * 2^-24 * sum |g| bounds a sum of n f32 terms in any order (each of the n - 1 additions
        # rounds a partial sum of magnitude <= sum |g| by at most 2^-24 relative)
        go = R.grad_out_normal(arg.shape, 32)
        want, n, sabs = R.backward_statement(go, case['rois'], arg, R.B, R.H, R.W)
        got = native.roi_pool_bwd(torch.from_numpy(go).float().to(DEV), rois, argd, (R.B, R.H, R.W, Cn)).double().cpu().numpy()
        bound = np.maximum(n - 1, 0) * 2.0 ** -24 * sabs
        err = np.abs(got - want)
        print('%s %dx%d: worst |got - ref| / bound = %.3f over %d elements with n > 1, n max %d' % (
            name, PH, PW, float((err[n > 1] / bound[n > 1]).max()), int((n > 1).sum()), int(n.max())))
        assert (err <= bound).all()
        assert (got[n == 0] == 0).all() and (n == 0).any()                       # nothing points there: exactly 0
        assert (got[n == 1] == want[n == 1]).all()
        # the malformed, off-map and bad-batch RoIs contribute nothing
        if name != 'wide':
            ks = [case['family'][f] for f in ('malformed_x', 'malformed_y', 'malformed_zero', 'off_left', 'off_bottom', 'batch_minus', 'batch_past')]
            only = np.zeros_like(go)
            only[ks] = go[ks]
            g = native.roi_pool_bwd(torch.from_numpy(only).float().to(DEV), rois, argd, (R.B, R.H, R.W, Cn))
            assert not bool(g.any())


# ------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize('mode', ['bf16', 'f32'])
def test_ops_roi_pool_layouts_backward_and_dtypes(mode):
    case = R.make_case('c64')
    dt = DTYPES[mode]
    fmap, rois = _feat(case, dt), torch.from_numpy(case['rois']).to(DEV)
    cl = fmap.permute(0, 3, 1, 2)                                                  # channels_last: logical NCHW over physical NHWC
    assert ops._channels_last(cl)
    want, want_arg = native.roi_pool_fwd(fmap, rois, 7, 7, R.SCALE, with_argmax=True)
    with torch.no_grad():
        y_cl = ops.roi_pool(cl, rois, 7, R.SCALE)
        y_nchw = ops.roi_pool(cl.contiguous(), rois, (7, 7), R.SCALE)
        y_mod = ops.RoIPool(7, R.SCALE)(cl, rois)
    assert tuple(y_cl.shape) == (40, 64, 7, 7) and ops._channels_last(y_cl) and y_cl.dtype == dt
    assert torch.equal(y_cl.permute(0, 2, 3, 1), want) and torch.equal(y_nchw, y_cl) and torch.equal(y_mod, y_cl)
    with pytest.raises(ValueError, match='wrong roi size'):
        ops.roi_pool(cl, rois[:, :4], 7, R.SCALE)
    go = torch.from_numpy(R.grad_out_ints((40, 7, 7, 64), 41)).to(dt).to(DEV)
    g_native = native.roi_pool_bwd(go, rois, want_arg, (R.B, R.H, R.W, 64))
    for nchw in (False, True):
        x = (cl.contiguous() if nchw else cl).detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        r = rois.clone().requires_grad_(True)
        y = ops.RoIPool(7, R.SCALE)(x, r)
        assert torch.equal(y.detach(), y_cl)
        y.backward(go.permute(0, 3, 1, 2))
        assert x.grad is not None and x.grad.dtype == dt and tuple(x.grad.shape) == tuple(x.shape)
        assert torch.equal(x.grad.permute(0, 2, 3, 1), native.cast(g_native, dt)) and bool(x.grad.any())
        assert r.grad is None


# ------------------------------------------------------------------------------------------------ a window with RoIPool
HW, PAD = (150, 250), (160, 256)          # the reduced window of tests/test_dpool_gpu.py
T, NPROP = 3, 24
ROI_LAYER = dict(type='RoIPool', out_size=7)
_models = {}


def _window_model(dtype):
    if dtype not in _models:
        cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
        cfg.model.backbone['depth'] = 50
        cfg.model.shared_head['depth'] = 50
        cfg.model.bbox_roi_extractor['roi_layer'] = dict(ROI_LAYER)
        _models[dtype] = hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr', depth=50), dtype, DEV)
    return _models[dtype]


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _clip(seed):
    return torch.cat([S.synth_frame(seed + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)


def test_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    assert isinstance(model.bbox_roi_extractor.roi_layers[0], ops.RoIPool)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [_clip(10 * c) for c in range(2)]
    first = [_eager(model, clip, metas) for clip in clips]
    again = [_eager(model, clip, metas) for clip in clips]
    g = GraphedClip(model, clips[0], metas, rescale=True)
    n_det = 0
    for rep in range(2):
        for clip, want, want2 in zip(clips, first, again):
            got = g.run(clip).result()
            assert len(got) == len(want) == 2
            assert all(_same(a, b) for a, b in zip(want, want2)), 'two eager calls differ'
            assert all(_same(a, b) for a, b in zip(got, want)), 'graph replay differs from the eager window'
            n_det += sum(len(r) for r in got[-1])
    assert n_det > 0


def test_cached_frame_path_gives_the_clip_paths_fc1_rows():
    model = _window_model(torch.bfloat16)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = _clip(40)
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        w = model.window_tensors(c4, metas, speculate=True)
        f1 = model.bbox_head.fc1_rows(w['roi_feats'])
        assert tuple(f1.shape) == (T * NPROP, 1024) and ops._channels_last(w['roi_feats'])
        for i in range(T):
            e = model.frame_tensors(c4[i:i + 1], metas[i])
            assert torch.equal(e['f1'], f1[i * NPROP:(i + 1) * NPROP]), i
    assert float(f1.float().abs().max()) > 0


def test_window_roi_feats_equal_the_statement_in_f32_and_two_clips_run_in_one_call():
    model = _window_model(torch.float32)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [_clip(70), _clip(90)]
    with torch.no_grad():
        c4 = [model(img=clip, img_meta=metas, backbone_feat=True)[0] for clip in clips]
        w = model.window_tensors(c4[0], metas)
        fmap = w['c5'].permute(0, 2, 3, 1)
        assert fmap.is_contiguous() and fmap.dtype == torch.float32
        rois = w['rois'].contiguous()
        got = w['roi_feats'].permute(0, 2, 3, 1)
        val, arg, rec = R.pool_statement(fmap.cpu().numpy(), rois.cpu().numpy(), 7, 7, 1 / 16)
        assert torch.equal(got.cpu(), torch.from_numpy(val)) and not rec['empty'].all() and float(got.abs().max()) > 0
        _, a = native.roi_pool_fwd(fmap, rois, 7, 7, 1 / 16, with_argmax=True)
        assert torch.equal(a.cpu(), torch.from_numpy(arg))
        # two clips in one call: the batch index runs over 2 * T frames
        w2 = model.window_tensors(torch.cat(c4, 0), metas * 2, speculate=True, clips=2)
        fmap2, rois2 = w2['c5'].permute(0, 2, 3, 1), w2['rois'].contiguous()
        assert fmap2.shape[0] == 2 * T and int(rois2[:, 0].max()) == 2 * T - 1 and rois2.shape[0] == 2 * T * NPROP
        val2, _, _ = R.pool_statement(fmap2.cpu().numpy(), rois2.cpu().numpy(), 7, 7, 1 / 16)
        assert torch.equal(w2['roi_feats'].permute(0, 2, 3, 1).cpu(), torch.from_numpy(val2))
        batch = model.forward_feat_clips(torch.cat(c4, 0), metas * 2, 2, rescale=True)
        assert len(batch) == 2 and sum(len(r) for c in range(2) for r in batch[c][-1]) > 0


# ------------------------------------------------------------------------------------------------ training
def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().float().cpu(), b.detach().float().cpu(), rtol=rtol, atol=atol)


def _pool_by_gather(c5, rois, out_size, scale):
    """RoIPool as plain torch on the device forward's argmax: a gather that torch autograd differentiates.  c5 physical NHWC."""
    Tn, h, w, Cn = c5.shape
    K = rois.shape[0]
    with torch.no_grad():
        val, arg = native.roi_pool_fwd(c5.detach().contiguous(), rois, out_size, out_size, scale, with_argmax=True)
    frames = rois[:, 0].long()
    assert int(frames.min()) >= 0 and int(frames.max()) < Tn and int(arg.max()) >= 0
    picked = torch.gather(c5.reshape(Tn, h * w, Cn)[frames], 1, arg.clamp(min=0).long().view(K, -1, Cn)).view(K, out_size, out_size, Cn)
    picked = torch.where(arg >= 0, picked, torch.zeros((), dtype=picked.dtype, device=picked.device))      # an empty bin is 0 and carries no gradient
    assert torch.equal(picked.detach(), val)
    return picked.permute(0, 3, 1, 2)


def test_selsa_training_step_on_sampled_rois_through_roi_pool_matches_a_gather_step():
    """The setup of test_selsa_rcnn_training_step_on_sampled_rois_matches_the_oracle (tests/test_parity_gpu.py) with roi_layer = RoIPool:
    forward_train_sampled against a second step on the same model chained by hand from its own parts, the pooling a torch gather at the
    device forward's argmax.  That test's bars: losses close(1e-3, 1e-5), gradients 1e-2 of the tensor's largest entry."""
    sd = S.synth_state_dict('selsa')
    n, Tn = 8, 3
    cfg = selsa_config(frame_interval=1, nms_post=n)
    cfg.model.bbox_roi_extractor['roi_layer'] = dict(ROI_LAYER)
    model = hvrnet_amd.enable_training(hvrnet_amd.build_model(cfg, sd, torch.float32, DEV))
    g = torch.Generator().manual_seed(85)
    imgs = torch.randn((Tn, 3, 64, 96), generator=g) * 50.0
    xy = torch.rand((Tn * n, 2), generator=g) * torch.tensor([60.0, 36.0])
    wh = torch.rand((Tn * n, 2), generator=g) * 30 + 6
    rois = torch.cat([torch.arange(Tn).repeat_interleave(n)[:, None].float(), xy, xy + wh], 1).to(DEV)
    labels, lw, bt, bw = [t.to(DEV) for t in C.head_train_case(n=n)]
    cur = dict(start=n, length=n)
    watch = ['backbone.layer2.0.conv1.weight', 'backbone.layer3.5.conv2.weight', 'shared_head.layer4.2.conv3.weight',
             'shared_head.new_layer_1.conv.weight', 'bbox_head.fc_new_1.bias', 'bbox_head.selsa_1.q_data_fc_1.weight',
             'bbox_head.selsa_2.linear_out_2.weight', 'bbox_head.fc_cls.weight', 'bbox_head.fc_reg.bias']
    model.bbox_head.sampler_num, model.bbox_head.t_dim = n, Tn
    params = dict(model.named_parameters())
    got = model.forward_train_sampled(imgs.to(DEV), rois, cur, labels, lw, bt, bw)     # (the parent commit raises NotImplementedError here)
    got['total'].sum().backward()
    grads = {k: params[k].grad.detach().clone() for k in watch}
    for p in model.parameters():
        p.grad = None
    layer = model.bbox_roi_extractor.roi_layers[0]
    c4 = model.backbone.forward_train_nhwc(imgs.to(DEV))
    c5 = model.shared_head.forward_train_nhwc(c4)
    feats = _pool_by_gather(c5, rois, layer.out_size[0], layer.spatial_scale)
    want = model.bbox_head.loss_train(model.bbox_head.forward_train(feats, cur), labels, lw, bt, bw)
    want['total'].sum().backward()
    for k in ('loss_cls', 'loss_bbox', 'acc'):
        print(k, float(got[k].sum()), float(want[k].sum()))
        close(got[k], want[k], 1e-3, 1e-5)
    for k in watch:
        w = params[k].grad
        assert w is not None and grads[k] is not None, k
        print(k, 'max |grad| %.4g, max diff %.4g' % (float(w.abs().max()), float((grads[k] - w).abs().max())))
        close(grads[k], w, 1e-2, 1e-2 * w.abs().max().item())
        if k.startswith('backbone.'):
            assert float(grads[k].abs().max()) > 0 and float(w.abs().max()) > 0, k


def test_selsa_forward_train_runs_one_iteration_through_roi_pool():
    from hvrnet_amd.config import selsa_train_config
    n_post, n_sel, Tn = 24, 16, 3
    cfg = selsa_train_config(nms_post=n_post, rcnn_sampler_num=n_sel, t_dim=Tn)
    cfg.train_cfg.rpn.sampler.num = 16
    cfg.model.bbox_roi_extractor['roi_layer'] = dict(ROI_LAYER)
    model = hvrnet_amd.enable_training(hvrnet_amd.build_model(cfg, S.synth_state_dict('selsa'), torch.float32, DEV))
    g = torch.Generator().manual_seed(91)
    hw = (128, 192)
    imgs = torch.randn((Tn, 3) + hw, generator=g) * 50.0
    metas = [dict(img_shape=hw + (3,), pad_shape=hw + (3,), scale_factor=1.0, flip=False) for _ in range(Tn)]
    gt_b = torch.tensor([[16., 24., 90., 100.], [100., 30., 170., 110.], [40., 60., 103., 123.]]).to(DEV)
    gt_l = torch.tensor([5, 12, 30]).to(DEV)
    got = model(imgs.to(DEV), metas, return_loss=True, gt_bboxes=[gt_b] * Tn, gt_labels=[gt_l] * Tn)
    losses = [v if isinstance(v, torch.Tensor) else sum(v) for k, v in got.items() if 'loss' in k]
    assert len(losses) >= 4 and all(bool(torch.isfinite(v).all()) for v in losses)
    sum(v.sum() for v in losses).backward()
    gw = dict(model.named_parameters())['backbone.layer3.5.conv2.weight'].grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
