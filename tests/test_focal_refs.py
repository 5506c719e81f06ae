"""CPU checks of the sigmoid focal loss statements (tests/focal_refs.py) and of the host side of the feature: the statement against an
independent autograd evaluation and against the reference's own numbers (tests/golden/focal.npz), the f32 emulation inside every
bound, every listed mistake outside one, the module / registry / head surface, and the C ABI's new symbols.  No GPU."""
import os

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import native, registry
from tests import focal_refs as R
from tests import train_loss_refs as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GA = [(2.0, 0.25), (0.0, 0.5), (1.5, 0.75)]
SHAPES = [(1, 1), (7, 1), (5, 3), (64, 80), (257, 12)]


def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'focal.npz'))


def inside(got, ref, bound):
    err = (got.double() - ref).abs()
    return bool((err <= bound).all())


@pytest.mark.parametrize('family', ['normal', 'saturated'])
@pytest.mark.parametrize('gamma,alpha', GA)
def test_statement_equals_an_independent_autograd_evaluation(family, gamma, alpha):
    for N, C in SHAPES:
        x = R.logits_family(family, N, C, seed=N * 3 + C)
        t = R.targets_for(N, C, seed=N).clamp(min=0)
        ref, _ = R.focal_statement(x, t, gamma, alpha)
        l, g = R.focal_autograd_f64(x, t, gamma, alpha)
        assert bool(((ref['l'] - l).abs() <= 1e-12 * l.abs()).all()), (N, C)
        assert bool(((ref['g'] - g).abs() <= 1e-12 * g.abs()).all()), (N, C)


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('gamma,alpha', GA)
def test_f32_emulation_lies_inside_the_bound(family, gamma, alpha):
    for N, C in SHAPES:
        x = R.logits_family(family, N, C, seed=N * 3 + C)
        t = R.targets_for(N, C, seed=N)
        ref, bound = R.focal_statement(x, t, gamma, alpha)
        got = R.focal_f32(x, t, gamma, alpha)
        assert bool(torch.isfinite(got['l']).all() and torch.isfinite(got['g']).all())
        assert inside(got['l'], ref['l'], bound['l']) and inside(got['g'], ref['g'], bound['g']), (N, C)
        assert bool((got['l'][t < 0] == 0).all() and (got['g'][t < 0] == 0).all())
    for (H, W, A, ld), counts in (((6, 5, 12, 64), (7, 40)), ((4, 5, 3, 15), (0, 9))):
        c = R.rpn_focal_case(H, W, A, ld, counts, seed=5, family=family)
        ref, bound = R.rpn_focal_statement(gamma=gamma, alpha=alpha, w_cls=2.0, w_bbox=0.5, **c)
        got = R.rpn_focal_f32(gamma=gamma, alpha=alpha, w_cls=2.0, w_bbox=0.5, **c)
        assert inside(got['out2'], ref['out2'], bound['out2']) and inside(got['d_o'], ref['d_o'], bound['d_o'])


def _mistake_inputs():
    """The stated inputs a mistake has to show on: the three families elementwise and reduced, and two RPN cases."""
    for family in R.FAMILIES:
        x = R.logits_family(family, 40, 5, seed=3)
        yield 'elem', family, x, R.targets_for(40, 5, seed=3)
    for family in R.FAMILIES:
        yield 'rpn', family, R.rpn_focal_case(6, 5, 12, 64, (7, 40), seed=5, family=family), None
        yield 'rpn', family, R.rpn_focal_case(4, 5, 3, 15, (0, 9), seed=6, family=family), None


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_mistake_leaves_the_bound(mistake):
    caught = 0
    for kind, family, a, b in _mistake_inputs():
        if kind == 'elem':
            ref, bound = R.focal_statement(a, b, 2.0, 0.25)
            bad, _ = R.focal_statement(a, b, 2.0, 0.25, mistake=mistake)
            caught += not (inside(bad['l'], ref['l'], bound['l']) and inside(bad['g'], ref['g'], bound['g']))
            w = R.row_weights(a.shape[0], seed=1)
            ref, bound = R.focal_loss_statement(a, a.shape[1], b, w, 2.0, 0.25, 1.0, 7.0)
            bad, _ = R.focal_loss_statement(a, a.shape[1], b, w, 2.0, 0.25, 1.0, 7.0, mistake=mistake)
            caught += not (inside(bad['out1'], ref['out1'], bound['out1']) and inside(bad['d'], ref['d'], bound['d']))
        else:
            ref, bound = R.rpn_focal_statement(gamma=2.0, alpha=0.25, **a)
            bad, _ = R.rpn_focal_statement(gamma=2.0, alpha=0.25, mistake=mistake, **a)
            caught += not (inside(bad['out2'], ref['out2'], bound['out2']) and inside(bad['d_o'], ref['d_o'], bound['d_o']))
    assert caught >= 1, mistake


def test_gamma_zero_alpha_half_is_half_the_bce_statement():
    """gamma = 0, alpha = 0.5: l = 0.5 bce.  rpn_loss_statement with counts (1, 0) divides its BCE sum by 2."""
    c = L.rpn_case(7, 3, 15, (1, 0), seed=4)
    c['label_w'] = torch.ones_like(c['label_w'])
    bce, _ = L.rpn_loss_statement(**c)
    M = 21
    x = c['o'][:, :3].reshape(M, 1)
    ref, _ = R.focal_statement(x, c['labels'], 0.0, 0.5)
    assert abs(float(ref['l'].sum()) - float(bce['out2'][0])) <= 1e-12 * abs(float(bce['out2'][0]))
    assert bool(((ref['g'][:, 0] - bce['d_o'][:, :3].reshape(-1)).abs() <= 1e-12).all())


def test_statement_reproduces_the_reference_numbers():
    """Tolerance 1e-9 relative: the reference's f64 run forms 1 - sigmoid(x) by subtraction, which at the fixture's |x| <= 12 keeps
    2^-53 / (1 - p) <= 2e-11 per factor (times gamma); the statement has no such cancellation."""
    g = golden()
    for k in ('a', 'b', 'c'):
        x, t, w = torch.as_tensor(g[k + '.x']), torch.as_tensor(g[k + '.t']), torch.as_tensor(g[k + '.w'])
        gamma, alpha = (float(v) for v in g[k + '.gamma_alpha'])
        N, C = x.shape
        ref, _ = R.focal_statement(x, t, gamma, alpha)
        assert np.allclose(ref['l'].numpy(), g[k + '.none'], rtol=1e-9, atol=1e-300), k
        for name, avg in (('mean', float(N * C)), ('mean_avg', float(g[k + '.avg'])), ('sum', 1.0)):
            red, _ = R.focal_loss_statement(x, C, t, w, gamma, alpha, 1.0, avg)
            assert abs(float(red['out1']) - float(g[k + '.' + name])) <= 1e-9 * abs(float(g[k + '.' + name])), (k, name)
        red, _ = R.focal_loss_statement(x, C, t, w, gamma, alpha, 1.0, 1.0)
        assert np.allclose(red['d'].numpy(), g[k + '.grad_sum'], rtol=1e-9, atol=1e-300), k


def test_host_restatement_of_the_sampling_free_targets_reproduces_the_reference():
    g = golden()
    lab, lw, bt, bw, (npos, nneg) = R.anchor_target_host(torch.as_tensor(g['at.anchors']), None, torch.as_tensor(g['at.gt_bboxes']),
                                                          tuple(g['at.img_shape']), R.AT_CFG)
    assert (npos, nneg) == (int(g['at.num_pos']), int(g['at.num_neg'])) and npos >= 2 and nneg >= 2
    assert np.array_equal(lab.numpy(), g['at.labels']) and np.array_equal(lw.numpy(), g['at.label_weights'])
    assert np.array_equal(bw.numpy(), g['at.bbox_weights']) and np.allclose(bt.numpy(), g['at.bbox_targets'], rtol=0, atol=1e-6)
    a = g['at.anchors']
    h, w = g['at.img_shape'][:2]
    ins = (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < w) & (a[:, 3] < h)
    assert (~ins).any() and (lw.numpy()[~ins] == 0).all()                       # outside the image: weight 0
    assert int(ins.sum()) > npos + nneg and int((lw.numpy() > 0).sum()) == npos + nneg     # the ignore band: weight 0 too


def test_focal_loss_module_registry_and_argument_errors():
    assert registry.LOSSES.get('FocalLoss') is hvrnet_amd.FocalLoss is hvrnet_amd.losses.FocalLoss
    m = registry.build_loss(dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.4, reduction='sum', loss_weight=2.0))
    assert (m.use_sigmoid, m.gamma, m.alpha, m.reduction, m.loss_weight) == (True, 1.5, 0.4, 'sum', 2.0)
    d = hvrnet_amd.FocalLoss()
    assert (d.use_sigmoid, d.gamma, d.alpha, d.reduction, d.loss_weight) == (True, 2.0, 0.25, 'mean', 1.0)
    with pytest.raises(AssertionError):
        hvrnet_amd.FocalLoss(use_sigmoid=False)
    x, t = torch.zeros(3, 2), torch.zeros(3, dtype=torch.long)
    with pytest.raises(ValueError):
        m(x, t, avg_factor=3.0)                          # 'sum' with an avg_factor
    with pytest.raises(ValueError):
        d(x, t, avg_factor=3.0, reduction_override='sum')
    with pytest.raises(AssertionError):
        d(x, t, reduction_override='median')
    for red in ('none', 'mean', 'sum'):
        with pytest.raises(NotImplementedError, match='GPU only'):
            d(x, t, reduction_override=red)
    from hvrnet_amd import ops
    with pytest.raises(NotImplementedError, match='GPU only'):
        ops.sigmoid_focal_loss(x, t, 2.0, 0.25)
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.focal_loss(x, t)
    for fn, args in ((native.sigmoid_focal_loss_fwd, (x, t, 2.0, 0.25)), (native.sigmoid_focal_loss_bwd, (x, t, x, 2.0, 0.25)),
                     (native.rpn_focal_loss, (torch.zeros(1, 5), 1, t[:1], x[:1, 0], torch.zeros(1, 4), torch.zeros(1, 4),
                                              torch.zeros(2, dtype=torch.int32), 1.0, 2.0, 0.25))):
        with pytest.raises(NotImplementedError, match='GPU only'):
            fn(*args)


def test_rpn_head_sampling_follows_the_classification_loss():
    from hvrnet_amd.rpn_head import RPNHead
    focal = RPNHead(16, feat_channels=16, anchor_strides=[16], loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25))
    plain = RPNHead(16, feat_channels=16, anchor_strides=[16])
    assert focal.sampling is False and plain.sampling is True
    assert isinstance(focal.loss_cls, hvrnet_amd.FocalLoss) and (focal.loss_cls.gamma, focal.loss_cls.alpha) == (2.0, 0.25)
    assert list(focal.state_dict()) == list(plain.state_dict())
    with pytest.raises(NotImplementedError, match='GHMC'):
        RPNHead(16, feat_channels=16, anchor_strides=[16], loss_cls=dict(type='GHMC', use_sigmoid=True))
    from hvrnet_amd import targets as T
    assert isinstance(T.build_sampler(dict(type='PseudoSampler')), T.PseudoSampler)


def test_c_abi_has_the_focal_symbols_and_keeps_its_version():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib = native.lib()
    for sym in ('hvr_sigmoid_focal_loss_fwd', 'hvr_sigmoid_focal_loss_bwd', 'hvr_focal_loss', 'hvr_focal_loss_splits',
                'hvr_focal_loss_workspace_bytes', 'hvr_rpn_focal_loss'):
        assert hasattr(lib, sym) and sym in native.SYMBOLS, sym
    assert lib.hvr_abi_version() == native.ABI_VERSION == 7


def test_splits_equal_their_restatement():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib = native.lib()
    for N in (1, 2, 7, 64, 257, 683, 1000, 2049, 4099, 150000, 5000000):
        for C in (1, 3, 12, 31, 80):
            S, rows = R.focal_loss_splits(N, C)
            assert native.focal_loss_splits(N, C) == S and 1 <= S <= min(N, 2048) and (S - 1) * rows < N <= S * rows, (N, C)
            assert lib.hvr_focal_loss_workspace_bytes(N, C) == (4 * S + 255) // 256 * 256
    assert native.focal_loss_splits(0, 3) == 0 and native.focal_loss_splits(3, -1) == 0
