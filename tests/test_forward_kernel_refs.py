"""CPU tests of tests/forward_kernel_refs.py: the f64 statements against torch's own f64 operators, the bounds against independent
f32 evaluations in several summation orders, the exact-sum builders, and the catalogue of kernel mistakes -- each one shown to fall
outside the bound / bracket on real-statistics operands, to break equality on the exact-sum operands, or (stores past the last row)
to touch the guard rows.  Small versions of the descriptors the window issues."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import forward_kernel_refs as R
from tests import train_loss_refs as L


def _conv_torch(x, w, bias, resid, relu, stride, pad, dil):
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), bias, stride, pad, dil).permute(0, 2, 3, 1)
    if resid is not None:
        y = y + resid
    return y.clamp(min=0) if relu else y


CONVS = [  # B, H, W, Cin, Cout, k, stride, pad, dil
    (2, 9, 11, 64, 128, 3, 1, 1, 1), (1, 10, 13, 32, 64, 3, 1, 2, 2), (2, 9, 12, 64, 96, 1, 2, 0, 1), (1, 13, 17, 3, 64, 7, 2, 3, 1),
    (1, 8, 9, 32, 32, 3, 2, 1, 1)]


@pytest.mark.parametrize('B,H,W,Cin,Cout,k,stride,pad,dil', CONVS)
def test_conv_statement_is_the_f64_convolution(B, H, W, Cin, Cout, k, stride, pad, dil):
    g = torch.Generator().manual_seed(k * 100 + Cin)
    x = torch.randn((B, H, W, Cin), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, k, k, Cin), generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    want = _conv_torch(x, w, b, None, False, stride, pad, dil)
    r = torch.randn(want.shape, generator=g, dtype=torch.float64)
    ref, mag, absxw = R.conv_statement(x, w, b, r, True, stride, pad, dil)
    assert ref.shape == want.shape
    assert (ref - (want + r).clamp(min=0)).abs().max() < 1e-12 * float(mag.max())
    assert (absxw - _conv_torch(x.abs(), w.abs(), None, None, False, stride, pad, dil)).abs().max() < 1e-12 * float(mag.max())
    assert torch.allclose(mag, absxw + b.abs() + r.abs(), rtol=1e-14, atol=0)


def test_tail_stem_and_pool_statements():
    g = torch.Generator().manual_seed(5)
    h = torch.randn((2, 5, 6, 64), generator=g, dtype=torch.float64)
    x = torch.randn((2, 10, 11, 64), generator=g, dtype=torch.float64)
    w = torch.randn((128, 128), generator=g, dtype=torch.float64)
    b = torch.randn(128, generator=g, dtype=torch.float64)
    ref = R.tail_statement(h, x, w, b, 2)[0]
    want = (h @ w[:, :64].t() + x[:, ::2, ::2][:, :5, :6] @ w[:, 64:].t() + b).clamp(min=0)
    assert (ref - want).abs().max() < 1e-12
    wn = torch.randn((64, 128), generator=g, dtype=torch.float64)
    bn = torch.randn(64, generator=g, dtype=torch.float64)
    t = R.tail_next_statement(h, x, None, w, b, wn, bn, 2, 'bf16')
    assert torch.equal(t['y_stored'], want.float().bfloat16().double()) or (t['y_stored'] - want).abs().max() < 2.0 ** -8 * want.abs().max()
    assert (t['hn'][0] - (t['y_stored'] @ wn.t() + bn).clamp(min=0)).abs().max() < 1e-11
    ident = torch.randn((2, 5, 6, 128), generator=g, dtype=torch.float64)
    t2 = R.tail_next_statement(h, None, ident, w[:, :64], b, wn, bn, 1, 'f16')
    assert (t2['y'][0] - (h @ w[:, :64].t() + b + ident).clamp(min=0)).abs().max() < 1e-12
    img = torch.randn((2, 3, 21, 30), generator=g)
    ws = torch.randn((64, 7, 7, 3), generator=g, dtype=torch.float64) * 0.1
    bs = torch.randn(64, generator=g, dtype=torch.float64)
    ref, bound = R.stem_statement(img, ws, bs, 'f32')
    want = F.max_pool2d(F.conv2d(img.double(), ws.permute(0, 3, 1, 2), bs, 2, 3).clamp(min=0), 3, 2, 1).permute(0, 2, 3, 1)
    assert ref.shape == want.shape and (ref - want).abs().max() < 1e-12 and float(bound.min()) > 0
    cols, OH, OW = R.im2col_stem_statement(img, 192)
    assert (cols[:, :147] @ ws.reshape(64, 147).t()).view(2, OH, OW, 64).sub(F.conv2d(img.double(), ws.permute(0, 3, 1, 2), None, 2, 3).permute(0, 2, 3, 1)).abs().max() < 1e-12
    assert not bool(cols[:, 147:].any())


@pytest.mark.parametrize('Mq,Mk', [(37, 300), (5, 128), (16, 129)])
def test_relation_statement_is_softmax_times_v(Mq, Mk):
    g = torch.Generator().manual_seed(Mq)
    q, k, v = (torch.randn((m, 64), generator=g) for m in (Mq, Mk, Mk))
    ref, bound = R.relation_statement(q, k, v, 0.125, 'f32')
    want = torch.softmax(0.125 * (q.double() @ k.double().t()), 1) @ v.double()
    assert (ref - want).abs().max() < 1e-13 and float(bound.min()) > 0
    G = 3
    qg, kg, vg = (torch.randn((G * m, 64), generator=g) for m in (Mq, Mk, Mk))
    rg, _ = R.relation_grouped_statement(qg, kg, vg, 0.125, G, 'bf16', grouped_apply=True)
    for i in range(G):
        want = torch.softmax(0.125 * (qg[i * Mq:(i + 1) * Mq].double() @ kg[i * Mk:(i + 1) * Mk].double().t()), 1) @ vg[i * Mk:(i + 1) * Mk].double()
        assert (rg[i * Mq:(i + 1) * Mq] - want).abs().max() < 1e-13


# ------------------------------------------------------------------------------------------------ f32 evaluations in several orders
def _f32_sum(terms, order):
    """terms [M, N, K] f32, summed along K in f32: 'seq' one chain; ('blk', n) chains of n joined in sequence (n = 256: the two-level form)."""
    M, N, K = terms.shape
    if order == 'seq':
        acc = torch.zeros((M, N), dtype=torch.float32)
        for i in range(K):
            acc = acc + terms[:, :, i]
        return acc
    n = order[1]
    assert K % n == 0
    t = terms.view(M, N, K // n, n)
    blk = torch.zeros((M, N, K // n), dtype=torch.float32)
    for i in range(n):
        blk = blk + t[..., i]
    return _f32_sum(blk, 'seq')


ORDERS = ['seq', ('blk', 32), ('blk', 256)]


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('order', ORDERS, ids=['sequential', 'blocked32', 'two_level256'])
def test_the_bound_admits_f32_sums_in_any_order(mode, order):
    """The product of a [24, 2304] by w [16, 2304]^T (a layer-3 3x3's K) evaluated in f32 -- rounded products for the f32 mode, the
    three half products per term for split half -- in one chain, in blocks of 32, and in the two-level form (blocks of 256, under the
    tile-hint-18 bound where the mode has it): every element inside the bound (the worst ratio, printed, is ~1e-3: a worst-case bound at this K is blind to single products, which is what the exact-sum family is for)."""
    a, w = R.real_operands((24, 2304), (16, 2304), mode, seed=11)
    g = torch.Generator().manual_seed(3)
    bias = torch.randn(16, generator=g).double()
    ref, mag, absxw = R.gemm_statement(a, w, bias, None, False)
    if mode == 'f16x2':
        (ah, al), (wh, wl) = R.split_parts(a, R.ACT_SCALE), R.split_parts(w, R.WEIGHT_SCALE)
        parts = [(ah, wh), (ah, wl), (al, wh)]
        terms = torch.cat([(x[:, None, :] * y[None, :, :]).float() for x, y in parts], 2)     # exact products of halves
        terms = terms.view(24, 16, 3, 2304).permute(0, 1, 3, 2).reshape(24, 16, 3 * 2304)    # k-major: hi hi, hi lo, lo hi per k
        order = order if order == 'seq' else ('blk', 3 * order[1])
    else:
        terms = (a[:, None, :] * w[None, :, :]).float()       # f32 mode: one rounding per product; 16-bit modes: exact
    got = (_f32_sum(terms, order) + bias.float()).double()
    two = order != 'seq' and order[1] in (256, 768) and mode in ('f32', 'f16x2')
    bound = R.mfma_bound(mag, absxw, 2304, mode, two_level=two)
    ratio = float(((got - ref).abs() / bound).max())
    print('RATIO f32-evaluation %s %s %.3g' % (order, mode, ratio))
    assert 0.0 < ratio <= 1.0
    if two:
        assert float((bound / R.mfma_bound(mag, absxw, 2304, mode)).max()) < 0.2      # the two-level bound is the tighter one


def test_the_relation_bound_admits_an_f32_evaluation():
    for mode in ('f32', 'bf16', 'f16'):
        q, k = L.relation_inputs(37, 300, 64, R.STORE[mode], 4, peaky=False)
        v = torch.randn((300, 64), generator=torch.Generator().manual_seed(9)).to(R.STORE[mode])
        ref, bound = R.relation_statement(q, k, v, 0.125, mode)
        P = torch.softmax((q.float() @ k.float().t()) * 0.125, 1)
        if mode != 'f32':
            P = P.to(R.STORE[mode]).float()
        got = (P @ v.float()).double()
        ratio = float(((got - ref).abs() / bound).max())
        print('RATIO relation f32-evaluation %s %.3g' % (mode, ratio))
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ exact-sum builders
@pytest.mark.parametrize('mode,family', [('bf16', 'plain'), ('f16', 'plain'), ('f32', 'plain'), ('f16x2', 'plain'), ('f16x2', 'lo_act'),
                                         ('f16x2', 'lo_weight')])
def test_exact_builders_keep_their_promise(mode, family):
    """The builder's operands satisfy assert_exact at a long K (the RPN 3x3's 9 216), an f32 evaluation in two orders equals the
    statement bit for bit, 16-bit results include rounding ties, and the split-half families carry the cross term they are for."""
    c = R.exact_case((40, 9216), (24, 9216), mode, seed=21, family=family)
    a, w, bias = c['a'], c['w'], c['bias']
    resid = R.exact_resid((40, 24), c['g'])
    ref, mag, absxw = R.gemm_statement(a, w, bias, resid, True)
    R.assert_exact(a, w, mag, c['q'], mode, ref)
    for order in ('seq', ('blk', 256)):
        terms = (a[:, None, :] * w[None, :, :]).float()
        got = (_f32_sum(terms, order) + bias.float() + resid.float()).clamp(min=0).double()
        assert torch.equal(got, ref)
    if mode in ('bf16', 'f16'):
        big = R.gemm_statement(a * 1.0, w, bias, None, False)[0]
        assert R.count_ties(big, mode) > 0
    if family != 'plain':
        ah, al = R.split_parts(a, R.ACT_SCALE)
        wh, wl = R.split_parts(w, R.WEIGHT_SCALE)
        assert bool(al.any()) == (family == 'lo_act') and bool(wl.any()) == (family == 'lo_weight')
        assert torch.equal(ah + al, a) and torch.equal(wh + wl, w)
    with pytest.raises(AssertionError):
        R.assert_exact(a * 3, w * 3, mag * 9 * 2.0 ** 12, c['q'], mode)
    with pytest.raises(AssertionError):
        R.assert_exact(a + c['q'] / 2, w, mag, c['q'], mode)


@pytest.mark.parametrize('family', R.TAIL_NEXT_FAMILIES)
def test_exact_tail_next_builder(family):
    """The identity-form tail + next conv1 on its exact families: both products satisfy the exact-sum conditions, and each split-half
    family carries the cross term it is for -- shown by the statement with that term dropped being unequal, the other one equal."""
    mode = 'f16x2'
    c = R.exact_tail_next_case((2, 9, 11, 64), (256, 64), (64, 256), mode, 17, family)
    t = R.tail_next_statement(c['h'], None, c['resid'], c['w'], c['bias'], c['wn'], c['bn'], 1, mode)
    R.assert_exact(c['h'], c['w'], t['y'][1], c['q'], mode, t['y'][0])
    ys, wn = t['y_stored'], c['wn']
    assert float(t['hn'][1].max()) <= 2.0 ** 24 * c['q'] ** 3 / (1 + 2.0 ** -10)
    assert bool((R.store_true(wn.float(), mode, 'weight') == wn).all())
    yh, yl = R.split_parts(ys, R.ACT_SCALE)
    wh, wl = R.split_parts(wn, R.WEIGHT_SCALE)
    assert torch.equal(yh + yl, ys) and torch.equal(wh + wl, wn)
    hh, hl = R.split_parts(c['h'], R.ACT_SCALE)
    w3h, w3l = R.split_parts(c['w'], R.WEIGHT_SCALE)
    first = dict(plain=(False, False), lo_act=(True, False), lo_weight=(False, True), hn_lo_weight=(False, False))[family]
    assert (bool(hl.any()), bool(w3l.any())) == first
    second = dict(plain=None, lo_act=(True, False), lo_weight=(True, False), hn_lo_weight=(False, True))[family]
    if second is not None:
        assert (bool(yl.any()), bool(wl.any())) == second
        flat = ys.reshape(-1, 256)
        full = R.gemm_statement(flat, wn, c['bn'], None, True)[0]
        seen = 'no_lo_hi' if second[0] else 'no_hi_lo'                        # the mistake that drops the term this family carries
        blind = 'no_hi_lo' if second[0] else 'no_lo_hi'
        assert not torch.equal(R.gemm_statement(flat, wn, c['bn'], None, True, mistake=seen)[0], full)
        assert torch.equal(R.gemm_statement(flat, wn, c['bn'], None, True, mistake=blind)[0], full)


@pytest.mark.parametrize('family', ['plain', 'lo_act', 'lo_weight'])
def test_exact_stem_builder(family):
    mode = 'f16x2'
    c = R.exact_stem_case((2, 3, 37, 45), mode, 19, family)
    x = c['img'].permute(0, 2, 3, 1)
    ref, mag, _ = R.conv_statement(x, c['w'], c['bias'], None, True, 2, 3, 1)
    R.assert_exact(x, c['w'], mag, c['q'], mode, ref, qw=c['qw'])
    assert bool((c['img'].to(torch.float16).double() + (c['img'] - c['img'].to(torch.float16).double()).to(torch.float16).double() == c['img']).all())
    scaled = c['w'] * (R.WEIGHT_SCALE * R.ACT_SCALE)                          # stem_split_weights: planes of w x 2^10
    hi = scaled.to(torch.float16).double()
    lo = (scaled - hi).to(torch.float16).double()
    assert torch.equal(hi + lo, scaled) and float(scaled.abs().max()) < 65504
    img_lo = (c['img'] - c['img'].to(torch.float16).double())
    assert (bool(img_lo.any()), bool(lo.any())) == dict(plain=(False, False), lo_act=(True, False), lo_weight=(False, True))[family]
    pooled, _ = R.stem_statement(c['img'].float(), c['w'], c['bias'], mode)
    assert float(pooled.abs().max()) < 65504 / R.ACT_SCALE


def test_permutation_case_is_exact():
    sc = R.permutation_scale()
    assert float(torch.tensor(sc, dtype=torch.float32) * torch.tensor(R.LOG2E_F32, dtype=torch.float32)) == 2.0 ** -5
    for mode in ('bf16', 'f16x2'):
        q, k, v, sel = R.permutation_case(300, 4500, 1024, mode, 3)
        logits2 = (q.double() @ k.double().t()) * 2.0 ** -5                   # log2 units
        assert bool((logits2 == logits2.round()).all())
        top = logits2.max(1).values
        assert bool((top == 2 * R.PERM_MARGIN_LOG2).all()) and bool((logits2.argmax(1) == sel).all())
        second = logits2.scatter(1, sel[:, None], -1.0).max(1).values
        assert float((top - second).min()) == R.PERM_MARGIN_LOG2 > 150.0
        assert float(torch.exp2(torch.tensor(-R.PERM_MARGIN_LOG2, dtype=torch.float32))) == 0.0
        ref, _ = R.relation_statement(q[:64], k, v, sc, mode)
        assert torch.equal(ref, v[sel[:64]].double())
        assert R.seams_crossed(sel, 4500) and not R.seams_crossed(sel[:5], 4500)
        for seam in (128, 256, 288):                                           # the row-tile seams inside 300 rows: the rows on their two
            assert int(sel[seam - 1]) != int(sel[seam])                        # sides exist and select different keys
    q2, k2, v2, sel2 = R.permutation_case(4500, 4500, 1024, 'bf16', 3)        # the full stage (stride 1): every row seam of 128 / 256 / 288 /
    for tile in (128, 256, 288, 352):                                          # 352 rows has rows on both sides selecting different keys
        for seam in range(tile, 4500, tile):
            assert int(sel2[seam - 1]) != int(sel2[seam])
    assert R.seams_crossed(sel2, 4500) and len(set((sel2 // 128).tolist())) == 36
    qg, kg, vg, selg = R.permutation_case(300, 4500, 1024, 'bf16', 3, groups=4)
    assert qg.shape[0] == 1200 and int(selg.max()) < 18000 and not torch.equal(selg[:300] + 4500, selg[300:600])


# ------------------------------------------------------------------------------------------------ the catalogue of mistakes
def _caught(ref_stmt, bad_stmt, bound, mode, out_f32=False, store_mistake=None):
    """real / exact families share this: the mistaken statement stored as a perfect kernel would store it, against the bracket of the
    right one.  -> number of elements outside."""
    lo, hi = R.stored_bracket(ref_stmt, bound, mode, out_f32)
    M = ref_stmt.reshape(-1, ref_stmt.shape[-1]).shape[0]
    buf = R.emulate_store(bad_stmt.reshape(M, -1), mode, mistake=store_mistake, out_f32=out_f32)
    got = buf[:M].view(ref_stmt.shape)
    return R.compare(got, lo, hi, ref_stmt)[1], buf, M


def _conv_case(desc, mode, family, seed=31):
    B, H, W, Cin, Cout, k, stride, pad, dil = desc
    if family == 'real':
        x, w = R.real_operands((B, H, W, Cin), (Cout, k, k, Cin), mode, seed)
        g = torch.Generator().manual_seed(seed + 1)
        bias = torch.randn(Cout, generator=g).double() * 0.3
        OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        resid = R.store_true(torch.randn((B, OH, OW, Cout), generator=g), mode)
        return x, w, bias, resid, None
    c = R.exact_case((B, H, W, Cin), (Cout, k, k, Cin), mode, seed, family=family)
    OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return c['a'], c['w'], c['bias'], R.exact_resid((B, OH, OW, Cout), c['g']), c['q']


# mistake -> (the family that must catch it, kind of statement, mode)
CATALOGUE = {
    'k_drop': ('exact', 'conv', 'bf16'), 'k_twice': ('exact', 'conv', 'bf16'), 'tap_border': ('exact', 'conv', 'bf16'),
    'dil1': ('exact', 'conv_dil', 'bf16'), 'rows_past_M': ('guard', 'conv', 'bf16'), 'skip_last_tile': ('real', 'conv', 'bf16'),
    'bias_last_chunk': ('real', 'conv', 'bf16'), 'resid_after_relu': ('real', 'conv', 'bf16'), 'shortcut_odd': ('real', 'tail', 'bf16'),
    'hn_unrounded': ('exact', 'tail_next', 'bf16'), 'trunc_store': ('exact', 'conv', 'bf16'), 'no_hi_lo': ('exact_lo_weight', 'gemm', 'f16x2'),
    'no_lo_hi': ('exact_lo_act', 'gemm', 'f16x2'), 'alpha_on_bias': ('real', 'gemm', 'f16x2'),
    'block_weight_skipped': ('real', 'relation', 'bf16'), 'group_offset': ('permutation', 'relation_grouped', 'bf16'),
}
CONV3 = (2, 9, 11, 64, 128, 3, 1, 1, 1)
CONV_DIL = (1, 10, 13, 64, 64, 3, 1, 2, 2)


def _run(kind, mode, family, mistake):
    """-> (elements outside the bracket / unequal, guard rows intact) of `mistake` under `family` ('real', 'plain', 'lo_act', 'lo_weight')."""
    real = family == 'real'
    stmt_mistake = None if mistake in ('trunc_store', 'rows_past_M') else mistake
    store_mistake = mistake if mistake in ('trunc_store', 'rows_past_M') else None
    if kind in ('conv', 'conv_dil'):
        desc = CONV3 if kind == 'conv' else CONV_DIL
        x, w, bias, resid, q = _conv_case(desc, mode, family)
        args = (x, w, bias, resid, True, desc[6], desc[7], desc[8])
        ref, mag, absxw = R.conv_statement(*args)
        bad = R.conv_statement(*args, mistake=stmt_mistake, mode=mode)[0]
        K = desc[3] * desc[5] ** 2
    elif kind == 'gemm':
        if real:
            a, w = R.real_operands((200, 512), (96, 512), mode, 41)
            bias, q = torch.randn(96, generator=torch.Generator().manual_seed(2)).double(), None
        else:
            c = R.exact_case((200, 512), (96, 512), mode, 41, family=family)
            a, w, bias, q = c['a'], c['w'], c['bias'], c['q']
        ref, mag, absxw = R.gemm_statement(a, w, bias, None, True)
        bad = R.gemm_statement(a, w, bias, None, True, mistake=stmt_mistake, mode=mode)[0]
        x, K = a, 512
    elif kind == 'tail':
        g = torch.Generator().manual_seed(43)
        if real:
            h, w = R.real_operands((2, 5, 6, 64), (256, 128), mode, 43)
            xx = R.store_true(torch.randn((2, 10, 12, 64), generator=g).clamp(min=0), mode)
            bias, q = torch.randn(256, generator=g).double() * 0.3, None
        else:
            c = R.exact_case((2, 5, 6, 64), (256, 128), mode, 43)
            h, w, bias, q = c['a'], c['w'], c['bias'], c['q']
            xx = R._ints((2, 10, 12, 64), -15, 15, c['g']) * q
        ref, mag, absxw = R.tail_statement(h, xx, w, bias, 2)
        bad = R.tail_statement(h, xx, w, bias, 2, mistake=stmt_mistake)[0]
        x, K = h, 128
    elif kind == 'tail_next':
        if real:
            h, w = R.real_operands((2, 5, 6, 64), (256, 64), mode, 45)
            g = torch.Generator().manual_seed(46)
            resid = R.store_true(torch.randn((2, 5, 6, 256), generator=g).clamp(min=0), mode)
            wn = R.store_true(torch.randn((64, 256), generator=g) / 16, mode, 'weight')
            bias, bn, q = torch.randn(256, generator=g).double() * 0.3, torch.randn(64, generator=g).double() * 0.3, None
        else:
            c = R.exact_case((2, 5, 6, 64), (256, 64), mode, 45)
            h, w, bias, q = c['a'], c['w'], c['bias'], c['q']
            resid = R.exact_resid((2, 5, 6, 256), c['g'])
            wn = R._ints((64, 256), -3, 3, c['g']) * q
            bn = R._ints((64,), -64, 64, c['g']) * q ** 3 * 2 ** 8
        t = R.tail_next_statement(h, None, resid, w, bias, wn, bn, 1, mode)
        tb = R.tail_next_statement(h, None, resid, w, bias, wn, bn, 1, mode, mistake=stmt_mistake)
        if not real:
            R.assert_exact(h, w, t['y'][1], q, mode, t['y'][0])
            assert float(t['hn'][1].max()) <= 2.0 ** 24 * q ** 3        # the second product: multiples of q^3, exact in f32 in any order
        ylo, yhi = R.stored_bracket(t['y'][0], R.mfma_bound(t['y'][1], t['y'][2], 64, mode), mode)
        ref, mag, absxw = t['hn']
        bad = tb['hn'][0]
        extra = R.hn_extra(ylo, yhi, t['y_stored'], wn)
        bound = R.mfma_bound(mag, absxw, 256, mode) + extra
        n, buf, M = _caught(ref, bad, bound if real else torch.zeros_like(ref), mode)
        return n, R.guard_intact(buf, M)
    else:
        raise AssertionError(kind)
    if not real:
        R.assert_exact(x, w, mag, q, mode, ref)
    bound = R.mfma_bound(mag, absxw, K, mode) if real else torch.zeros_like(ref)       # exact family: equality with RN(ref)
    n, buf, M = _caught(ref, bad, bound, mode, store_mistake=store_mistake)
    return n, R.guard_intact(buf, M)


def _run_relation(kind, family, mistake):
    mode = 'bf16'
    if family == 'permutation':
        q, k, v, sel = R.permutation_case(40, 600, 64, mode, 5, groups=3 if kind == 'relation_grouped' else 1)
        sc = R.permutation_scale()
    else:
        G = 3 if kind == 'relation_grouped' else 1
        q, k = L.relation_inputs(40 * G, 600 * G, 64, torch.bfloat16, 7, peaky=False)
        v = torch.randn((600 * G, 64), generator=torch.Generator().manual_seed(8)).bfloat16()
        sc = 0.125
    if kind == 'relation_grouped':
        ref, bound = R.relation_grouped_statement(q, k, v, sc, 3, mode, grouped_apply=True)
        bad = R.relation_grouped_statement(q, k, v, sc, 3, mode, grouped_apply=True, mistake=mistake)[0]
    else:
        ref, bound = R.relation_statement(q, k, v, sc, mode)
        bad = R.relation_statement(q, k, v, sc, mode, mistake=mistake)[0]
    if family == 'permutation':
        assert torch.equal(ref, v[sel].double())
        bound = torch.zeros_like(ref)
    return _caught(ref, bad, bound, mode)[0]


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_mistake_of_the_catalogue_is_caught(mistake):
    """Each mistake of the issue's catalogue under both operand families; the family CATALOGUE names must catch it (elements outside
    the bracket of the right statement, stored values unequal to RN(exact statement), or guard rows overwritten), and the right
    statement itself passes under both.  Prints which families catch it."""
    want, kind, mode = CATALOGUE[mistake]
    if kind.startswith('relation'):
        res = {fam: _run_relation(kind, fam, mistake) for fam in ('real', 'permutation')}
        clean = {fam: _run_relation(kind, fam, None) for fam in ('real', 'permutation')}
        print('MISTAKE %-22s real: %d outside, permutation: %d unequal' % (mistake, res['real'], res['permutation']))
        assert clean == {'real': 0, 'permutation': 0}
        assert res[want] > 0
        return
    fams = ['real', 'plain'] + (['lo_act', 'lo_weight'] if mode == 'f16x2' else [])
    res = {fam: _run(kind, mode, fam, mistake) for fam in fams}
    clean = {fam: _run(kind, mode, fam, None) for fam in fams}
    print('MISTAKE %-22s %s' % (mistake, {f: ('%d bad' % r[0]) + ('' if r[1] else ', guard rows written') for f, r in res.items()}))
    assert all(r == (0, True) for r in clean.values()), clean
    if want == 'guard':
        assert not res['real'][1] and not res['plain'][1]
    elif want == 'real':
        assert res['real'][0] > 0
    elif want == 'exact':
        assert res['plain'][0] > 0
    else:
        assert res[want[len('exact_'):]][0] > 0
        other = 'lo_weight' if want.endswith('lo_act') else 'lo_act'
        assert res[other][0] == 0 and res['real'][0] == 0        # only its own exact family sees this cross term: the bound is blind to it


def test_catalogue_is_complete():
    assert set(CATALOGUE) == set(R.MISTAKES) and len(R.MISTAKES) == 16
