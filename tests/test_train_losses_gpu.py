"""The arithmetic kernels of the training step against the f64 statements of tests/train_loss_refs.py, called through the
native.* wrappers at the shapes training runs and at the edges where they branch: det_loss (plain and OHEM form), rpn_loss,
ce_rows, relation_probs, relation_dscore, sgd_step, relu_bwd, scale_rows.

Every bound is the derived one of train_loss_refs (u = 2^-24; nothing is measured against the device), every element of every
output is compared, and every test asserts from the launch arithmetic that the branch it names ran.  The only quantity compared
after rounding to a count is the top-1 accuracy (the case builders assert that no row has a tie).  Each comparison prints
`RATIO <kernel> <dtype> <worst error / bound>` (pytest -s shows it).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native  # noqa: E402
from tests import train_loss_refs as L  # noqa: E402

DEV = 'cuda:0'
NAMES = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'half'}


def dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def check(kernel, dtype, got, ref, bound):
    """Every element of `got` within `bound` of `ref` (f64 tensors on the device); prints the worst error / bound."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('RATIO %s %s %.4g' % (kernel, NAMES.get(dtype, dtype), worst))
    assert bool(torch.isfinite(got.double()).all()), kernel
    assert worst <= 1.0, '%s: %d of %d elements over the bound, worst error / bound %g' % (kernel, int((ratio > 1).sum()), ratio.numel(), worst)
    return worst


def check_bracket(kernel, dtype, got, lo, hi, ref, bound):
    """got within [lo, hi] (the bracket of a rounded result); the printed ratio is |got - ref| / (the wider half of the bracket)."""
    g = got.double()
    out = (g < lo) | (g > hi)
    half = torch.maximum(hi - ref, ref - lo).clamp(min=1e-300)
    ratio = torch.where(g == ref, torch.zeros_like(g), (g - ref).abs() / half)
    worst = float(ratio.max())
    print('RATIO %s %s %.4g' % (kernel, NAMES[dtype], worst))
    assert bool(torch.isfinite(g).all()), kernel
    assert not bool(out.any()), '%s: %d of %d elements outside the bracket, worst %g' % (kernel, int(out.sum()), g.numel(), worst)


# ------------------------------------------------------------------------------------------------ det loss, ce rows
def _det_on_device(case):
    return {k: dev(v) for k, v in case.items()}


def _det_call(c, sel):
    args = (c['logits'], c['cls_off'], c['reg_off'], c['ncls'], c['labels'], c['label_w'], c['bbox_t'], c['bbox_w'])
    if sel is None:
        return native.det_loss(*args, beta=c['beta'])
    return native.det_loss_sampled(*args, torch.tensor(sel, dtype=torch.int32, device=DEV), beta=c['beta'])


@pytest.mark.parametrize('name,p', L.det_params(), ids=lambda v: v if isinstance(v, str) else '')
def test_det_loss_against_f64(name, p):
    """det_loss_kernel, plain and sampled form: the three outputs and every element of dlogits (zero outside the class and delta
    columns) within the derived bounds; R on both sides of the 256-thread stride (1, 255, 256, 257), the row count the detector
    passes (4 500) and 20 000; three column layouts; the special cases of train_loss_refs.det_params.  A second call is bit-identical
    (one workgroup, fixed order)."""
    case, sel = L.det_build(p)
    c = _det_on_device(case)
    out3, dl = _det_call(c, sel)
    ref, bound = L.det_loss_statement(c['logits'], c['cls_off'], c['reg_off'], c['ncls'], c['labels'], c['label_w'], c['bbox_t'], c['bbox_w'],
                                      c['beta'], sel_counts=sel)
    R, ldl = case['logits'].shape
    # the branch this case names ran: rows per thread from the launch (one workgroup of 256), the divisor of the sampled form
    assert L.block_chain(R, 256, 8) == -(-R // 256) + 8 and (-(-R // 256) > 1) == (R > 256)
    if sel is not None:
        assert ref['rows'] == max(sum(sel), 1) and (p['sel'] != 'zero' or ref['rows'] == 1.0)
    if p['kind'] == 'no_pos':
        assert float(ref['out3'][1]) == 0.0 and float(out3[1]) == 0.0
    if p['kind'] == 'zero_w':
        assert float(ref['out3'][0]) == 0.0 and float(out3[0]) == 0.0 and not bool(dl[:, c['cls_off']:c['cls_off'] + c['ncls']].any())
    kernel = 'det_loss' if sel is None else 'det_loss_sampled'
    check(kernel + '.loss', torch.float32, out3[:2], ref['out3'][:2], bound['out3'][:2])
    assert round(float(out3[2]) * ref['rows'] / 100.0) == ref['count'], (float(out3[2]), ref['count'], ref['rows'])
    check(kernel + '.acc', torch.float32, out3[2:], ref['out3'][2:], bound['out3'][2:])
    check(kernel + '.dlogits', torch.float32, dl, ref['dlogits'], bound['dlogits'])
    live = torch.zeros(ldl, dtype=torch.bool, device=DEV)
    live[c['cls_off']:c['cls_off'] + c['ncls']] = True
    live[c['reg_off']:c['reg_off'] + 4] = True
    assert int(live.sum()) < ldl and bool((dl[:, ~live] == 0).all())            # padding columns: exactly zero
    out3b, dlb = _det_call(c, sel)
    assert torch.equal(out3, out3b) and torch.equal(dl, dlb)


@pytest.mark.parametrize('kind', ['plain', 'big'])
@pytest.mark.parametrize('cls_off', [0, 4])
@pytest.mark.parametrize('R', [1, 256, 257, 4500])
def test_ce_rows_against_f64(R, cls_off, kind):
    """ce_rows_kernel per row: R across the 256-row workgroup boundary (grid = ceil(R / 256)), class columns at an offset, logits
    scaled to +-80 and (plain, R >= 64) one row at +-1e4."""
    layout = L.DET_LAYOUTS[0] if cls_off == 0 else L.DET_LAYOUTS[1]
    case = L.det_case(R, layout, 1.0, seed=R + cls_off, kind=kind)
    assert case['cls_off'] == cls_off and (R + 255) // 256 == (2 if R in (257,) else (18 if R == 4500 else 1))
    logits, labels = dev(case['logits']), dev(case['labels'])
    got = native.ce_rows(logits, cls_off, case['ncls'], labels)
    ref, bound = L.ce_rows_statement(logits, cls_off, case['ncls'], labels)
    check('ce_rows', torch.float32, got, ref, bound)
    if kind == 'plain' and R >= 64:
        assert float(ref.max()) > 1e4


# ------------------------------------------------------------------------------------------------ rpn loss
@pytest.mark.parametrize('big', [False, True], ids=['n3', 'pm90'])
@pytest.mark.parametrize('counts', L.RPN_COUNTS, ids=lambda c: 'c%d_%d' % c)
@pytest.mark.parametrize('shape', L.RPN_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_rpn_loss_against_f64(shape, counts, big):
    """rpn_loss_kernel: M = rows * A not a multiple of the 1 024 lanes, the real 38 x 63 and 50 x 84 maps, A = 1, ldo = 5 A exactly,
    counts with zeros (the max(c, 1) of the average factor), logits to +-90 (both sigmoid branches), x = 0 and the smooth-L1
    branch points on purpose; every element of d_o, padding columns included (exactly zero); a second call bit-identical."""
    rows, A, ldo = shape
    c = L.rpn_case(rows, A, ldo, counts, seed=rows + A + counts[1] + int(big), big=big)
    M = rows * A
    assert (M % 1024 != 0) and L.block_chain(M, 1024, 10) == -(-M // 1024) + 10
    d = {k: dev(v) for k, v in c.items()}
    out2, d_o = native.rpn_loss(d['o'], A, d['labels'], d['label_w'], d['bbox_t'], d['bbox_w'], d['counts'], c['beta'])
    ref, bound = L.rpn_loss_statement(d['o'], A, d['labels'], d['label_w'], d['bbox_t'], d['bbox_w'], counts, c['beta'])
    assert float(ref['out2'][0]) > 0
    check('rpn_loss.loss', torch.float32, out2, ref['out2'], bound['out2'])
    check('rpn_loss.d_o', torch.float32, d_o, ref['d_o'], bound['d_o'])
    assert bool((d_o[:, 5 * A:] == 0).all())
    out2b, d_ob = native.rpn_loss(d['o'], A, d['labels'], d['label_w'], d['bbox_t'], d['bbox_w'], d['counts'], c['beta'])
    assert torch.equal(out2, out2b) and torch.equal(d_o, d_ob)


def test_rpn_loss_padding_columns_are_written():
    """Columns 5 A .. ldo of d_o belong to no anchor; the wrapper hands the kernel an uninitialised buffer and the gradient flows
    on into the RPN convolution's backward, where a NaN bit pattern in those columns would poison every product.  A NaN-filled
    tensor of d_o's size is freed just before the call so that the caching allocator hands the same block back."""
    rows, A, ldo = 2394, 12, 64
    c = L.rpn_case(rows, A, ldo, (128, 128), seed=5)
    d = {k: dev(v) for k, v in c.items()}
    junk = torch.full((rows, ldo), float('nan'), device=DEV)
    ptr = junk.data_ptr()
    del junk
    _, d_o = native.rpn_loss(d['o'], A, d['labels'], d['label_w'], d['bbox_t'], d['bbox_w'], d['counts'], c['beta'])
    assert d_o.data_ptr() == ptr, 'the allocator did not hand the NaN-filled block back: the test would see nothing'
    assert bool((d_o[:, 5 * A:] == 0).all())


def test_rpn_loss_rejects_wrong_sizes_before_any_launch():
    """A bbox_targets of the wrong length (or label weights) must raise in the wrapper: the kernel would read past the end."""
    rows, A, ldo = 7, 3, 15
    c = L.rpn_case(rows, A, ldo, (0, 256), seed=1)
    d = {k: dev(v) for k, v in c.items()}
    with pytest.raises(AssertionError, match='four values per anchor'):
        native.rpn_loss(d['o'], A, d['labels'], d['label_w'], d['bbox_t'][:-1], d['bbox_w'], d['counts'], c['beta'])
    with pytest.raises(AssertionError, match='one value per anchor'):
        native.rpn_loss(d['o'], A, d['labels'], d['label_w'][:-1], d['bbox_t'], d['bbox_w'], d['counts'], c['beta'])
    # a non-f32 tensor is converted, not reinterpreted
    a, _ = native.rpn_loss(d['o'], A, d['labels'], d['label_w'].double(), d['bbox_t'].double(), d['bbox_w'].double(), d['counts'], c['beta'])
    b, _ = native.rpn_loss(d['o'], A, d['labels'], d['label_w'], d['bbox_t'], d['bbox_w'], d['counts'], c['beta'])
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ relation probs / dscore
def _probs(q, k, scale, nan_prefill=True):
    Mq, Mk = q.shape[0], k.shape[0]
    out = torch.full((Mq, native.relation_ldp(Mk)), float('nan'), dtype=q.dtype, device=DEV) if nan_prefill else None
    return native.relation_probs(q, k, scale, out=out)


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
@pytest.mark.parametrize('Mq,Mk,D,pad', L.relation_cases(), ids=lambda v: str(v))
def test_relation_probs_against_f64(Mq, Mk, D, pad, dtype):
    """hvr_relation_probs element by element: Mk of one key, around one 128-key block, not a multiple of 4, 64 and 65 blocks (the
    t += 64 loops of the normalising sweep), 128 blocks (the largest supported), the 4 500 x 4 500 window; Q / K contiguous and as
    row slices of wider matrices; a row whose block maxima differ by more than exp2's f32 range; the output buffer full of NaN
    before the call (padding columns must come out exactly zero); every row sums to one within its summed bound."""
    q, k = L.relation_inputs(Mq, Mk, D, dtype, seed=Mq + Mk, device=DEV, pad=pad)
    assert (q.stride(0) > D) == (pad > 0) and k.stride(0) == D + pad
    sc = L.relation_scale(D)
    got = _probs(q, k, sc)
    P, bound, nt = L.relation_probs_statement(q, k, sc)
    assert got.shape == (Mq, nt * 128) and nt == -(-Mk // 128) and nt <= 128
    if Mk in (8320, L.MAX_KEYS):
        assert nt > 64                                        # the sweep's lanes loop a second time
    assert bool((got[:, Mk:] == 0).all())                     # also where the buffer held NaN
    lo, hi = L.relation_probs_bracket(P, bound, dtype)
    check_bracket('relation_probs', dtype, got, lo, hi, P, bound)
    assert bool(((got.double().sum(1) - 1).abs() <= (hi - lo).sum(1)).all())
    if Mk >= 2 and D == 1024 and nt > 1:
        S0 = sc * (q[0].double() @ k.double().t())
        assert float(S0[Mk - 1] - S0[:128].max()) / math.log(2) > 300 and float(got[0, Mk - 1]) == 1.0


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
def test_relation_probs_rejects_a_depth_the_tile_engine_cannot_step(dtype):
    """D must be a multiple of the tile engine's K-step (32 f32 / 64 two-byte elements): rejected by design, with its message."""
    q, k = L.relation_inputs(37, 129, 1000 if dtype != torch.float32 else 1008, dtype, seed=1, device=DEV, peaky=False)
    with pytest.raises(native.HvrError, match='not a multiple of the %d-element K-step' % native.kstep(dtype)):
        native.relation_probs(q, k, 1 / 32)


def test_relation_rejects_more_than_16384_keys():
    """Mk > 16 384 (more than 128 key blocks) is HVR_EUNSUPPORTED at both entry points that normalise P in a sweep, before
    anything is launched: hvr_relation_probs and the split-half forward for Mq >= 1 024.  (Inputs are uninitialised: nothing reads
    them.)"""
    Mk = L.MAX_KEYS + 1
    for dtype in L.RELATION_DTYPES:
        q, k = torch.empty((4, 64), dtype=dtype, device=DEV), torch.empty((Mk, 64), dtype=dtype, device=DEV)
        with pytest.raises(native.HvrError, match=r'\(-2\).*relation probs: Mk=16385 exceeds the 16384 keys'):
            native.relation_probs(q, k, 0.125)
    q = torch.empty((1024, 64), dtype=native.SPLIT, device=DEV)
    k = torch.empty((Mk, 64), dtype=native.SPLIT, device=DEV)
    with pytest.raises(native.HvrError, match=r'\(-2\).*split-half relation: Mk=16385 exceeds the 16384 keys'):
        native.relation_fwd(q, k, k, 0.125)
    with pytest.raises(native.HvrError, match=r'\(-2\).*split-half relation: Mk=16385 exceeds the 16384 keys'):
        native.relation_fwd_grouped(torch.cat([q, q]), torch.cat([k, k]), torch.cat([k, k]), 0.125, 2)


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
@pytest.mark.parametrize('cancel', [False, True], ids=['plain', 'cancel'])
@pytest.mark.parametrize('Mq,Mk,D,pad', L.relation_cases(), ids=lambda v: str(v))
def test_relation_dscore_against_f64(Mq, Mk, D, pad, cancel, dtype):
    """relation_dscore_kernel element by element at the same sizes, dO / O as row slices of wider matrices, and with dP = delta
    (1 + 2^-10 noise): heavy cancellation in dP - delta, which the bound carries through sum|dO O|."""
    P, dP, dO, O = L.dscore_inputs(Mq, Mk, D, dtype, seed=Mq + Mk + int(cancel), device=DEV, cancel=cancel)
    assert dO.stride(0) == D + 64 and O.stride(0) == D + 32 and -(-D // 1024) == (1 if D <= 1024 else 2)
    sc = L.relation_scale(D)
    got = native.relation_dscore(P, dP, dO, O, sc)
    ref, bound = L.relation_dscore_statement(P, dP, dO, O, sc)
    lo, hi = L.bracket(ref, bound, dtype)
    check_bracket('relation_dscore' + ('.cancel' if cancel else ''), dtype, got, lo, hi, ref, bound)
    assert bool((got[:, Mk:] == 0).all())


# ------------------------------------------------------------------------------------------------ sgd step
def _sgd_check(n, gscale, tag):
    p, g, buf = L.sgd_case(n, seed=n)
    stale_buf = L.sgd_case(n, seed=n, stale=True)[2]
    H = L.SGD_HYPER
    for name, max_norm, first, stale in L.sgd_configs(g, gscale):
        b0 = stale_buf if stale else buf
        pd, gd, bd = p.to(DEV), g.to(DEV), b0.to(DEV)
        p0, g0, b00 = pd.clone(), gd.clone(), bd.clone()
        native.sgd_step(pd, gd, bd, H['lr'], H['mom'], H['wd'], grad_scale=gscale, max_norm=max_norm, first_step=first)
        (rp, rb), (bp, bb), clip = L.sgd_statement(p0, g0, b00, gscale=gscale, max_norm=max_norm, first=first, **H)
        check('sgd.param.' + tag, torch.float32, pd, rp, bp)
        check('sgd.buffer.' + tag, torch.float32, bd, rb, bb)
        assert torch.equal(gd, g0)
        if name in ('ulp_below', 'at_norm', 'ulp_above'):
            assert abs(clip - 1.0) < 4 * L.U
        if name == 'far_below':
            assert clip < 2e-3
        if name == 'first_stale':
            assert float(b00.abs().max()) > 1e3 * float(rb.abs().max())     # a stale buffer would have shown
        if name == 'far_below':                                             # two more steps: the state carries over correctly
            for _ in range(2):
                p1, b1 = pd.clone(), bd.clone()
                native.sgd_step(pd, gd, bd, H['lr'], H['mom'], H['wd'], grad_scale=gscale, max_norm=max_norm, first_step=False)
                (rp, rb), (bp, bb), _ = L.sgd_statement(p1, g0, b1, gscale=gscale, max_norm=max_norm, first=False, **H)
                check('sgd.param.' + tag, torch.float32, pd, rp, bp)
                check('sgd.buffer.' + tag, torch.float32, bd, rb, bb)


@pytest.mark.parametrize('gscale', [1.0, 0.125])
@pytest.mark.parametrize('n', L.SGD_SIZES)
def test_sgd_step_against_f64(n, gscale):
    """hvr_sgd_step after ONE call, parameter and momentum buffer element-wise: n below, at and above the float4 width (the n & 3
    tail of the sum of squares), a million elements; no clipping, far above / below the norm, max_norm within one ulp of the norm
    on both sides; first_step over a buffer of large stale values; grad_scale inside the norm; then two more steps, each
    compared from the state before it."""
    assert (n & 3) == {1: 1, 3: 3, 4: 0, 5: 1, 1000003: 3}[n]
    _sgd_check(n, gscale, 'small' if n < 8 else '1M')


def test_sgd_step_flat_buffer_size():
    """The flat buffer of the HVR detector (dist_train.FlatParams): 44 M elements, so every lane of the 1 024 x 256 sum-of-squares
    grid loops (n / 4 > 262 144 float4) and the update's grid is grid-strided if capped."""
    n = L.hvr_flat_numel()
    assert n // 4 > L.SUMSQ_PARTS * 256 and L.sumsq_chain(n) > L.sumsq_chain(1000003) and n > L.GRID_CAP_THREADS > 1000003
    _sgd_check(n, 0.125, 'flat')


# ------------------------------------------------------------------------------------------------ relu_bwd, scale_rows
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
@pytest.mark.parametrize('n', [4, 1020, 4500 * 1024])
def test_relu_bwd_bit_exact(n, dtype):
    """dy where y > 0 else +0, bit for bit: y holds +0, -0, the smallest positive subnormal of the type (positive: the gradient
    passes) and its negative; dy is NaN on half of the y <= 0 positions (the result there is 0, as torch.where gives)."""
    dy, y = L.relu_case(n, dtype, seed=n)
    got = native.relu_bwd(dy.to(DEV), y.to(DEV)).cpu()
    want = L.relu_bwd_statement(dy, y)
    assert ((n + 3) // 4 > L.GRID_CAP_THREADS) == (n == 4500 * 1024)      # the largest case runs the grid-stride loop
    assert torch.equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
@pytest.mark.parametrize('R,C', [(64, 576), (2048, 512), (1, 4)])
def test_scale_rows_bit_exact(R, C, dtype):
    """(w.float() * s[:, None]).to(dtype) bit for bit -- the f32 product rounded to f32, then to the type -- on inputs with exact
    rounding ties in bulk and with ties whose exact product lies off the tie (where one rounding of the exact product, a
    mixed-precision fma, gives the other neighbour).  For half: equal to pack_conv_weight of the same weights as a 1 x 1 conv, so
    the two ways of folding a BatchNorm scale cannot drift apart."""
    w, s, tie, inexact = L.scale_rows_case(R, C, dtype, seed=R + C)
    got = native.scale_rows(w.to(DEV), s.to(DEV)).cpu()
    want = L.scale_rows_statement(w, s)
    assert torch.equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    if dtype != torch.float32 and R > 1:
        assert int(tie.sum()) > R * C // 16
        one = L.scale_rows_single_rounding(w, s)
        if dtype == torch.float16 or R >= 2048:
            assert int((one.float() != want.float()).sum()) > 0      # the case can tell the two apart
    if dtype != torch.float32:
        packed = native.pack_conv_weight(w.float().view(R, C, 1, 1).to(DEV), s.to(DEV), dtype).cpu().view(R, C)
        assert torch.equal(_bits(packed), _bits(want))
