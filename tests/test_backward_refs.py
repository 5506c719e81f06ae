"""CPU tests of tests/backward_refs.py: the f64 statements of ConvFunction.backward / LinearFunction.backward against torch.autograd
on f64 operands, the bounds against independent f32 evaluations of the same sums in three orders, the exact-sum builder's promise,
and the catalogue of mistakes -- each one shown outside a bracket or bound, or unequal on the exact-sum operands, at a shape of the
GPU list (tests/test_backward_gpu.py runs the same cases on the device)."""
import pytest
import torch
import torch.nn.functional as F

from tests import backward_refs as BR
from tests import forward_kernel_refs as R
from tests import train_kernel_refs as K


# ------------------------------------------------------------------------------------------------ statements == autograd (f64)
SMALL = [  # B, H, W, Cin, Cout, k, stride, pad, dil
    (2, 7, 9, 8, 12, 3, 1, 1, 1), (1, 9, 8, 8, 6, 3, 1, 2, 2), (2, 7, 9, 6, 10, 3, 1, 0, 1), (2, 7, 9, 6, 10, 3, 1, 2, 1),
    (2, 5, 6, 16, 8, 1, 1, 0, 1), (2, 13, 19, 8, 12, 1, 2, 0, 1), (1, 6, 8, 4, 4, 1, 3, 0, 1)]


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('B,H,W,Cin,Cout,k,stride,pad,dil', SMALL)
def test_conv_statement_is_autograd_of_the_f64_conv(B, H, W, Cin, Cout, k, stride, pad, dil, relu):
    g = torch.Generator().manual_seed(H * 100 + k + pad)
    rnd = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    x, w = rnd(B, Cin, H, W).requires_grad_(True), rnd(Cout, Cin, k, k).requires_grad_(True)
    s, t = rnd(Cout), rnd(Cout).requires_grad_(True)
    z = F.conv2d(x, w * s.view(-1, 1, 1, 1), None, stride, pad, dil) + t.view(1, -1, 1, 1)
    r = rnd(*z.shape).requires_grad_(True)
    y = z + r
    y = y.clamp(min=0) if relu else y
    dy = rnd(*y.shape)
    y.backward(dy)
    nhwc = lambda a: a.detach().permute(0, 2, 3, 1).contiguous()
    w_eff = (w.detach() * s.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
    st = BR.conv_backward_statement(nhwc(x), w_eff, s, nhwc(y), nhwc(dy), relu, stride, pad, dil, None)
    for got, want in ((st['dx'], nhwc(x.grad)), (st['dw'], w.grad), (st['dt'], t.grad), (st['dr'], nhwc(r.grad)), (st['dz'], nhwc(r.grad))):
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the magnitudes: the same sums over absolute values
    xa, wa = x.detach().abs().requires_grad_(True), (w.detach() * s.view(-1, 1, 1, 1)).abs().requires_grad_(True)
    F.conv2d(xa, wa, None, stride, pad, dil).backward(st['dz'].abs().permute(0, 3, 1, 2))
    assert float((st['dx_mag'] - nhwc(xa.grad)).abs().max()) <= 1e-12 * float(xa.grad.max())
    assert float((st['dw_mag'] - wa.grad).abs().max()) <= 1e-12 * float(wa.grad.max())
    if stride > 1:                                                # off the lattice: exactly zero, value and bound
        off = torch.ones((H, W), dtype=torch.bool)
        off[::stride, ::stride] = False
        assert not bool(st['dx'][:, off].any()) and not bool(st['dx_mag'][:, off].any())


@pytest.mark.parametrize('M,Kd,N,relu', [(5, 8, 12, True), (37, 16, 8, False), (9, 12, 12, True)])
def test_linear_statement_is_autograd_of_f64_linear(M, Kd, N, relu):
    g = torch.Generator().manual_seed(M)
    rnd = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    x, w, b, r = (rnd(*sh).requires_grad_(True) for sh in ((M, Kd), (N, Kd), (N,), (M, N)))
    y = F.linear(x, w, b) + r
    y = y.clamp(min=0) if relu else y
    dy = rnd(M, N)
    y.backward(dy)
    st = BR.linear_backward_statement(x.detach(), w.detach(), y.detach(), dy, relu, None)
    for got, want in ((st['dx'], x.grad), (st['dw'], w.grad), (st['db'], b.grad), (st['dr'], r.grad)):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.allclose(st['dx_mag'], st['dz'].abs() @ w.detach().abs(), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ f32 evaluations in three orders
def _seq(terms):
    acc = torch.zeros(terms.shape[:-1], dtype=torch.float32)
    for i in range(terms.shape[-1]):
        acc = acc + terms[..., i]
    return acc


def _f32_sum(terms, order):
    """terms [..., n] f32 summed along n in f32: 'seq' one chain; 'blk64' chains of 64 joined in sequence (zero padded: the K-step
    padding); 'slice8' eight contiguous K slices (the last ragged) summed on their own, their partials added in sequence (split-K)."""
    n = terms.shape[-1]
    if order == 'seq':
        return _seq(terms)
    if order == 'blk64':
        t = F.pad(terms, (0, -n % 64))
        return _seq(_seq(t.view(*t.shape[:-1], -1, 64)))
    per = -(-n // 8)
    return _seq(torch.stack([_seq(terms[..., a:a + per]) for a in range(0, n, per)], -1))


def _case(name, mode, seed=5, exact=False):
    o = BR.conv_operands(name, mode, seed, exact)
    w_eff = K.pack_statement(o['w'], o['s'], R.STORE[mode])
    y = BR.stored_y(o, w_eff, mode)
    return o, w_eff, y


@pytest.mark.parametrize('mode', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('order', ['seq', 'blk64', 'slice8'])
def test_the_bound_admits_f32_sums_in_any_order(mode, order):
    """The first conv case's dX (864 terms) at a corner, two border and five interior pixels, and its dW (468 terms, times s, alone and
    added to a gradient g0) at 8 x 45 elements, evaluated in f32 -- products rounded once in the f32 mode, exact otherwise -- in one
    chain, in blocks of 64 and in eight K slices: every element inside the bracket / bound."""
    o, w_eff, y = _case('k3_res', mode)
    st = BR.conv_statement_of(o, w_eff, y, mode)
    dz, w, x = st['dz'], w_eff.double(), o['x'].double()
    B, OH, OW, Cout = dz.shape
    Cin, pad = w.shape[3], o['pad']
    prod = lambda a, b: (a * b).float()          # the f64 product is exact: ONE rounding in the f32 mode, none for 16-bit operands
    # dX: gather form over (ky, kx, o)
    pix = [(0, 0, 0), (0, 0, 7), (1, 5, 0), (0, 6, 9), (1, 12, 17), (0, 3, 3), (1, 7, 11), (0, 11, 16)]
    terms = torch.zeros((len(pix), Cin, 9 * Cout), dtype=torch.float32)
    for i, (b, iy, ix) in enumerate(pix):
        for ky in range(3):
            for kx in range(3):
                oy, ox = iy + pad - ky, ix + pad - kx
                if 0 <= oy < OH and 0 <= ox < OW:
                    terms[i, :, (ky * 3 + kx) * Cout:(ky * 3 + kx + 1) * Cout] = prod(dz[b, oy, ox][None, :], w[:, ky, kx, :].t())
    acc = _f32_sum(terms, order)
    got = acc.double() if mode == 'f32' else acc.to(R.STORE[mode]).double()
    lo, hi = BR.dx_bracket(st, mode)
    sel = lambda t: torch.stack([t[b, iy, ix] for b, iy, ix in pix])
    ratio, bad, _ = R.compare(got, sel(lo), sel(hi), sel(st['dx']))
    print('RATIO f32-evaluation dx %s %s %.3g' % (order, mode, ratio))
    assert bad == 0 and ratio > 0.0
    # dW
    cols = R._patches(x, 3, 3, 1, pad, 1)[0]                                       # [P, 9 Cin]
    os_, js = torch.arange(0, Cout, 12), torch.arange(0, 9 * Cin, 13)
    t2 = prod(dz.reshape(-1, Cout).t()[os_][:, None, :], cols.t()[js][None, :, :])   # [8, 45, P]
    s32 = o['s'][os_][:, None]
    dwg = _f32_sum(t2, order) * s32
    ky, kx, c = js // Cin // 3, js // Cin % 3, js % Cin
    pick = lambda t: t[os_][:, c, ky, kx]
    ref, bound = pick(st['dw']), pick(BR.dw_bound(st, mode, o['s']))
    ratio, bad = BR.within(dwg.double(), ref, bound)
    print('RATIO f32-evaluation dw %s %s %.3g' % (order, mode, ratio))
    assert bad == 0 and ratio > 0.0
    g0 = torch.randn(dwg.shape, generator=torch.Generator().manual_seed(2))
    full = torch.zeros_like(st['dw'])
    full[os_[:, None], c, ky, kx] = g0.double()
    ratio, bad = BR.within((g0 + dwg).double(), g0.double() + ref, pick(BR.dw_bound(st, mode, o['s'], g0=full)))
    assert bad == 0


# ------------------------------------------------------------------------------------------------ the exact-sum family
@pytest.mark.parametrize('mode', ['bf16', 'f16'])
@pytest.mark.parametrize('name', ['k3_res', 'k1_s2'])
def test_exact_operands_keep_their_promise(name, mode):
    o, w_eff, y = _case(name, mode, exact=True)
    assert torch.equal(w_eff.double(), (o['w'] * o['s'].view(-1, 1, 1, 1)).permute(0, 2, 3, 1).double())      # the pack rounds nothing
    for t in (o['x'], o['dy']):
        assert torch.equal(t.double().float().to(t.dtype), t)
    st = BR.conv_statement_of(o, w_eff, y, mode)
    BR.assert_exact_backward(st, o['s'], mode)
    assert 0.2 < float((st['dz'] != 0).double().mean()) < 0.8 and float((y == 0).double().mean()) > 0.2     # the gate is live
    if name == 'k3_res':
        assert R.count_ties(st['dx'], mode) > 0                    # RN against truncation shows


# ------------------------------------------------------------------------------------------------ the catalogue of mistakes
# mistake -> (conv / linear case, the outputs of which at least one must catch it on real-statistics operands)
CATALOGUE = {
    'taps_not_reversed': ('k3_res', ('dx',)), 'dx_pad_forward': ('k3_pad0', ('dx',)), 'dx_dil1': ('k3_dil2', ('dx',)),
    'mask_from_dy': ('k3_res', ('dz',)), 'mask_ge': ('k3_res', ('dz',)), 'dy_unrounded': ('k1_f32_48', ('dz', 'dw', 'dt')),
    'wgrad_no_scale': ('k3_res', ('dw',)), 'wgrad_scale_by_cin': ('k3_res', ('dw',)), 'wgrad_taps_swapped': ('k3_res', ('dw',)),
    'wgrad_dil1': ('k3_dil2', ('dw',)), 'pad_rows_live': ('k3_res', ('dw',)), 'wgrad_last_slice_dropped': ('k3_res', ('dw',)),
    'stride_scatter_offset': ('k1_s2', ('dx',)), 'accumulate_overwrites': ('k3_res', ('dw',)), 'dr_unmasked': ('k3_res', ('dr',)),
    'linear_dw_transposed': ('m37', ('dw',)), 'db_row_sums': ('m37', ('db',)),
}
MODE = 'bf16'


def _outside(st, sb, mode, s, g0, mistake, exact=False):
    """The mistaken statement `sb`, stored as a perfect kernel would store it, against the right statement's brackets and bounds
    (exact: against RN(statement) / the statement itself).  -> {output: elements outside or unequal}"""
    zero = lambda t: torch.zeros_like(t)
    out = dict(dz=int((sb['dz'] != st['dz']).sum()), dr=int((sb['dr'] != st['dr']).sum()))
    M = st['dx'].reshape(-1, st['dx'].shape[-1]).shape[0]
    lo, hi = (R.stored_bracket(st['dx'], zero(st['dx']), mode) if exact else BR.dx_bracket(st, mode))
    got = R.emulate_store(sb['dx'].reshape(M, -1), mode)[:M].view(st['dx'].shape)
    out['dx'] = R.compare(got, lo, hi, st['dx'])[1]
    ref = BR.delivered(st['dw'], g0)
    b = zero(ref) if exact else BR.dw_bound(st, mode, s, g0)
    out['dw'] = BR.within(BR.delivered(sb['dw'], g0, mistake).float().double(), ref, b)[1]
    key = 'dt' if 'dt' in st else 'db'
    cref, cb = BR.colsum_bound(st['dz'])
    out[key] = BR.within(sb[key].float().double(), cref, zero(cb) if exact else cb)[1]
    return out


def _run(mistake, name, exact=False):
    g = torch.Generator().manual_seed(77)
    if name in BR.LINEAR_CASES:
        o = BR.linear_operands(name, MODE, 9)
        wc = o['w'].to(R.STORE[MODE])
        r = None if o['resid'] is None else o['resid'].double()
        y = R.round_stored(R.gemm_statement(o['x'].double(), wc.double(), o['b'], r, o['relu'])[0], MODE)
        f = lambda m: BR.linear_backward_statement(o['x'], wc, y, o['dy'], o['relu'], MODE, m)
        s, g0 = None, None
    else:
        o, w_eff, y = _case(name, MODE, exact=exact)
        f = lambda m: BR.conv_statement_of(o, w_eff, y, MODE, m)
        s = o['s']
        g0 = torch.randint(-64, 65, o['w'].shape, generator=g).float() / 16 if mistake == 'accumulate_overwrites' else None
    st = f(None)
    if exact:
        BR.assert_exact_backward(st, s, MODE)
    return _outside(st, f(mistake), MODE, s, g0, mistake, exact), _outside(st, st, MODE, s, g0, None, exact)


@pytest.mark.parametrize('mistake', BR.MISTAKES)
def test_every_mistake_of_the_catalogue_is_caught(mistake):
    """Each mistake at the case CATALOGUE names, on real-statistics operands: at least one of the named outputs has elements outside its
    bracket / bound (dz, dr: unequal), and the right statement has none anywhere.  The conv mistakes that do not need an f32 dy run on
    the exact-sum operands as well, where the check is equality."""
    name, outputs = CATALOGUE[mistake]
    bad, clean = _run(mistake, name)
    print('MISTAKE %-26s %-10s real  %s' % (mistake, name, bad))
    assert not any(clean.values()), clean
    assert all(bad[k] > 0 for k in outputs), bad
    if name in ('k3_res', 'k1_s2'):
        bad_e, clean_e = _run(mistake, name, exact=True)
        print('MISTAKE %-26s %-10s exact %s' % (mistake, name, bad_e))
        assert not any(clean_e.values()), clean_e
        assert all(bad_e[k] > 0 for k in outputs), bad_e


def test_pad_forward_needs_its_cases():
    """'dx_pad_forward' is invisible where pad == dil (K - 1) / 2 (the first case) and shows at pad 0 and at pad 2."""
    assert not any(_run('dx_pad_forward', 'k3_res')[0].values())
    for name in ('k3_pad0', 'k3_pad2', 'k3_pad0_c64', 'k3_pad2_c64'):
        assert _run('dx_pad_forward', name)[0]['dx'] > 0


def test_catalogue_is_complete():
    assert set(CATALOGUE) == set(BR.MISTAKES) and len(BR.MISTAKES) == 17
    assert all(name in BR.CONV_CASES or name in BR.LINEAR_CASES for name, _ in CATALOGUE.values())
