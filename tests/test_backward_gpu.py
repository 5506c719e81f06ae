"""train_ops.ConvFunction.backward and train_ops.LinearFunction.backward as whole operations against the f64 statements of
tests/backward_refs.py: every element of dX inside its bracket, of dW / db / dt inside its bound, the residual gradient and the
off-lattice pixels of a strided dX bit-equal, on the two-byte routes training runs (hvr_relu_bwd_t + hvr_im2col_t into
hvr_gemm_splitk and hvr_unpack_conv_wgrad, the rotated-weight hvr_conv2d_nhwc, _pad_cols / transpose_pad padding to a K-step of 64)
and in f32; gradient delivery into a parameter's buffer (added / written over zeros); the parked route with NaN-filled slabs; and
the exact-sum family, where dX must be RN(statement) and dW exactly s * sum.  Each comparison prints
`RATIO <case> <output> <mode> <max |got - ref| / bound>`; no ratio is a pass criterion beyond <= 1 (no element outside)."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

from hvrnet_amd import native, train_ops as TO  # noqa: E402
from tests import backward_refs as BR  # noqa: E402
from tests import forward_kernel_refs as R  # noqa: E402

DEV = 'cuda:0'
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ['bf16', 'f16', 'f32']
RUNNABLE = [n for n in BR.CONV_CASES if n not in BR.REFUSED_CONV_CASES]


def _ratio(case, output, mode, ratio, bad):
    print('RATIO %s %s %s %.4g' % (case, output, mode, ratio))
    assert bad == 0, (case, output, mode, bad, ratio)


def _dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


def _conv(name, dt, seed=5, exact=False, w_grad=None, reuse=None):
    """One forward + backward of CONV_CASES[name] through ConvFunction -> (operands on the device, leaves, statement).
    reuse: an earlier result whose parameter and scale tensor this call takes again (the weight table keys on both)."""
    mode = R.mode_of(dt)
    o = BR.conv_operands(name, mode, seed, exact)
    x, resid = _dev(o['x'], True), _dev(o['resid'], True)
    w = torch.nn.Parameter(o['w'].to(DEV)) if reuse is None else reuse['w']
    w.grad = w_grad
    s, t, dy = _dev(o['s']) if reuse is None else reuse['s'], _dev(o['t'], o['out_f32']), _dev(o['dy'])
    y = TO.ConvFunction.apply(x, w, s, t, resid, o['relu'], o['stride'], o['pad'], o['dil'], o['out_f32'])
    assert y.dtype == (torch.float32 if o['out_f32'] else dt)
    y.backward(dy)
    torch.cuda.synchronize()
    w_eff = native.pack_conv_weight(w.detach().contiguous(), s, dt)
    st = BR.conv_backward_statement(x.detach(), w_eff, s, y.detach(), dy, o['relu'], o['stride'], o['pad'], o['dil'], mode)
    return dict(o=o, x=x, w=w, s=s, t=t, resid=resid, mode=mode), st


def _check_data_gradients(name, c, st):
    """dX inside its bracket; the residual gradient equal to dz; a strided dX exactly zero off the lattice; dt inside the colsum bound."""
    mode, o = c['mode'], c['o']
    lo, hi = BR.dx_bracket(st, mode)
    assert c['x'].grad.dtype == c['x'].dtype and c['x'].grad.shape == c['x'].shape
    ratio, bad, _ = R.compare(c['x'].grad, lo, hi, st['dx'])
    _ratio(name, 'dx', mode, ratio, bad)
    if c['resid'] is not None:
        assert torch.equal(c['resid'].grad.double(), st['dr'])
    if o['stride'] > 1:
        off = torch.ones(c['x'].shape[1:3], dtype=torch.bool, device=DEV)
        off[::o['stride'], ::o['stride']] = False
        assert int(off.sum()) > 0 and torch.equal(c['x'].grad[:, off], torch.zeros_like(c['x'].grad[:, off]))
    if o['out_f32']:
        ref, b = BR.colsum_bound(st['dz'])
        ratio, bad = BR.within(c['t'].grad, ref, b)
        _ratio(name, 'dt', mode, ratio, bad)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', RUNNABLE)
def test_conv_backward_against_f64(name, dt):
    c, st = _conv(name, dt)
    _check_data_gradients(name, c, st)
    assert c['w'].grad.dtype == torch.float32
    ratio, bad = BR.within(c['w'].grad, st['dw'], BR.dw_bound(st, c['mode'], c['s']))
    _ratio(name, 'dw', c['mode'], ratio, bad)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', BR.REFUSED_CONV_CASES)
def test_conv_refuses_an_input_channel_count_off_the_k_step(name, dt):
    """Cin = 72 is a multiple of neither K-step (64 two-byte, 32 f32): the forward refuses, loudly, before anything is launched."""
    o = BR.conv_operands(name, R.mode_of(dt), 5)
    x, w = _dev(o['x'], True), torch.nn.Parameter(o['w'].to(DEV))
    with pytest.raises(native.HvrError, match='Cin=72 is not a multiple of %d' % native.kstep(dt)):
        TO.ConvFunction.apply(x, w, _dev(o['s']), _dev(o['t']), _dev(o['resid']), o['relu'], o['stride'], o['pad'], o['dil'], False)
    torch.cuda.synchronize()


def _linear(name, dt, w_grad=None, b_grad=None):
    mode = R.mode_of(dt)
    o = BR.linear_operands(name, mode, 9)
    x, resid, dy = _dev(o['x'], True), _dev(o['resid'], True), _dev(o['dy'])
    w, b = torch.nn.Parameter(o['w'].to(DEV)), torch.nn.Parameter(o['b'].to(DEV))
    w.grad, b.grad = w_grad, b_grad
    y = TO.linear(x, w, b, resid, o['relu'], o['out_f32'])
    y.backward(dy)
    torch.cuda.synchronize()
    st = BR.linear_backward_statement(x.detach(), native.cast(w.detach(), dt), y.detach(), dy, o['relu'], mode)
    return dict(o=o, x=x, w=w, b=b, resid=resid, mode=mode), st


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', list(BR.LINEAR_CASES))
def test_linear_backward_against_f64(name, dt):
    c, st = _linear(name, dt)
    mode = c['mode']
    lo, hi = BR.dx_bracket(st, mode)
    assert c['x'].grad.dtype == dt
    ratio, bad, _ = R.compare(c['x'].grad, lo, hi, st['dx'])
    _ratio(name, 'dx', mode, ratio, bad)
    if c['resid'] is not None:
        assert torch.equal(c['resid'].grad.double(), st['dr'])
    ratio, bad = BR.within(c['w'].grad, st['dw'], BR.dw_bound(st, mode))
    _ratio(name, 'dw', mode, ratio, bad)
    ref, b = BR.colsum_bound(st['dz'])
    ratio, bad = BR.within(c['b'].grad, ref, b)
    _ratio(name, 'db', mode, ratio, bad)


# ------------------------------------------------------------------------------------------------ gradient delivery
def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


class _AllPristine(set):
    """wgrad_direct's `pristine` set for a call whose parameters are all pristine (their ids are only known once the helper has
    made them); `claimed` records which ones the Functions took out."""

    def __init__(self):
        super().__init__()
        self.claimed = set()

    def __contains__(self, key):
        return key not in self.claimed

    def discard(self, key):
        self.claimed.add(key)


@pytest.mark.parametrize('how', ['added_to_a_gradient', 'written_over_zeros'])
@pytest.mark.parametrize('name', ['k3_res', 'k1_s2'])
def test_conv_weight_gradient_delivered_into_the_parameter(name, how):
    """wgrad_direct(True): the weight gradient lands in the parameter's .grad -- g0 + statement within the accumulate bound when the
    buffer held g0, the statement itself when the parameter was pristine (zeros) -- and autograd is handed none."""
    shape = BR.conv_operands(name, 'bf16', 5)['w'].shape
    g0 = _seeded(shape, 21) if how == 'added_to_a_gradient' else torch.zeros(shape, device=DEV)
    buf = g0.clone()
    seeded = how == 'added_to_a_gradient'
    pristine = None if seeded else _AllPristine()
    prev = TO.wgrad_direct(True, pristine)
    try:
        c, st = _conv(name, torch.bfloat16, w_grad=buf)
    finally:
        TO.wgrad_direct(prev)
    assert c['w'].grad is buf
    if not seeded:
        assert pristine.claimed == {id(c['w'])}
    ratio, bad = BR.within(buf, BR.delivered(st['dw'], g0), BR.dw_bound(st, 'bf16', c['s'], g0 if seeded else None))
    _ratio(name, 'dw.' + how, 'bf16', ratio, bad)
    _check_data_gradients(name, c, st)


@pytest.mark.parametrize('how', ['added_to_a_gradient', 'written_over_zeros'])
def test_linear_gradients_delivered_into_the_parameters(how):
    M, Kd, N = BR.LINEAR_CASES['m37'][:3]
    seeded = how == 'added_to_a_gradient'
    gw0 = _seeded((N, Kd), 22) if seeded else torch.zeros((N, Kd), device=DEV)
    gb0 = _seeded((N,), 23) if seeded else torch.zeros(N, device=DEV)
    wbuf, bbuf = gw0.clone(), gb0.clone()
    pristine = None if seeded else _AllPristine()
    prev = TO.wgrad_direct(True, pristine)
    try:
        c, st = _linear('m37', torch.bfloat16, w_grad=wbuf, b_grad=bbuf)
    finally:
        TO.wgrad_direct(prev)
    assert c['w'].grad is wbuf and c['b'].grad is bbuf
    if not seeded:
        assert pristine.claimed == {id(c['w']), id(c['b'])}
    ratio, bad = BR.within(wbuf, BR.delivered(st['dw'], gw0), BR.dw_bound(st, 'bf16', None, gw0 if seeded else None))
    _ratio('m37', 'dw.' + how, 'bf16', ratio, bad)
    ref, b = BR.colsum_bound(st['dz'], gb0 if seeded else None)
    ratio, bad = BR.within(bbuf, BR.delivered(ref, gb0), b)
    _ratio('m37', 'db.' + how, 'bf16', ratio, bad)


def test_parked_weight_gradients_do_not_read_their_slabs_pad_columns():
    """wgrad_defer: three convs of the first case's shape, each with its own parameter.  Iteration 1 counts and wgrad_flush sizes the
    slabs (torch.empty); before iteration 2 every dzt / cols slab is filled with NaN bit patterns: a kernel that left columns
    P .. ldp - 1 of its out= slot unwritten would feed them to the batched product.  Every gradient finite and inside the dW bound."""
    dt, name = torch.bfloat16, 'k3_res'
    shape = BR.conv_operands(name, 'bf16', 5)['w'].shape
    bufs = [torch.zeros(shape, device=DEV) for _ in range(3)]
    prev_direct, prev_defer = TO.wgrad_direct(True), TO._wq['on']
    TO.wgrad_reset()
    try:
        for it in range(2):
            TO.wgrad_defer(True)
            if it == 1:
                classes = list(TO._wq['classes'].values())
                assert len(classes) == 1 and classes[0]['cap'] == 3 and classes[0]['dzt'].shape[2] == 512
                for c in classes:
                    for slab in (c['dzt'], c['cols']):
                        slab.view(torch.int16).fill_(0x7fc0)            # a bf16 quiet NaN
                        assert bool(torch.isnan(slab).all())
            for b in bufs:
                b.zero_()
            runs = [_conv(name, dt, seed=5 + i, w_grad=bufs[i]) for i in range(3)]
            if it == 1:
                assert TO._wq['classes'][next(iter(TO._wq['classes']))]['n'] == 3       # all three parked
                assert all(not bool(b.any()) for b in bufs)                            # nothing delivered before the flush
            TO.wgrad_flush()
            torch.cuda.synchronize()
    finally:
        TO.wgrad_direct(prev_direct)
        TO.wgrad_reset()
        TO.wgrad_defer(prev_defer)
    for i, (c, st) in enumerate(runs):
        assert c['w'].grad is bufs[i] and bool(torch.isfinite(bufs[i]).all())
        ratio, bad = BR.within(bufs[i], st['dw'], BR.dw_bound(st, 'bf16', c['s']))
        _ratio('%s.parked%d' % (name, i), 'dw', 'bf16', ratio, bad)
        _check_data_gradients('%s.parked%d' % (name, i), c, st)


def test_conv_backward_with_operands_from_the_weight_table():
    """prep_begin / prep_end as dist_train.train_iteration calls them: the first iteration records the layer, the second takes its
    packed operand and the rotated dX operand out of the table (hvr_pack_conv_weights_multi + hvr_transpose_multi).  Cout = 96: the
    table's rotated operand is padded to the dX conv's K-step like the one the layer makes for itself.  Same statement, same bounds."""
    name, dt = 'k3_res', torch.bfloat16
    owner = object()
    prev = TO.prep_enable(True)
    try:
        TO.prep_begin(owner)
        first, _ = _conv(name, dt)
        g_first = first['w'].grad.clone()
        TO.prep_end()
        (entry,) = TO._prep['entries'].values()
        assert entry['eff'] is not None and tuple(entry['aux'].shape) == (64, 3, 3, 96)
        TO.prep_begin(owner)
        assert TO._prep['valid'] and TO.table_operand(first['w'], first['s'], (96, 64, 3, 3), dt) is entry['eff']
        c, st = _conv(name, dt, reuse=first)
        TO.prep_end()
    finally:
        TO.prep_reset()
        TO.prep_enable(prev)
    assert torch.equal(entry['eff'], native.pack_conv_weight(c['w'].detach(), c['s'], dt))
    _check_data_gradients(name + '.table', c, st)
    ratio, bad = BR.within(c['w'].grad, st['dw'], BR.dw_bound(st, 'bf16', c['s']))
    _ratio(name + '.table', 'dw', 'bf16', ratio, bad)
    assert torch.equal(c['x'].grad, first['x'].grad) and torch.equal(c['w'].grad, g_first)


# ------------------------------------------------------------------------------------------------ the exact-sum family
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('name', ['k3_res', 'k1_s2'])
def test_exact_sums_come_back_bit_for_bit(name, dt):
    """Integer operands times a quantum, integer dy, s a power of two: every partial sum of either product is an f32 number in any
    order, so dX is RN(statement) and dW is s * sum, bit for bit."""
    c, st = _conv(name, dt, exact=True)
    BR.assert_exact_backward(st, c['s'].cpu(), c['mode'])
    assert torch.equal(c['x'].grad.double(), st['dx'].float().to(dt).double())
    assert torch.equal(c['w'].grad.double(), st['dw'])
    assert torch.equal(c['resid'].grad.double(), st['dr'])
    print('RATIO %s.exact dx %s 0\nRATIO %s.exact dw %s 0' % (name, c['mode'], name, c['mode']))


# ------------------------------------------------------------------------------------------------ the old f32 comparison, new bound
@pytest.mark.parametrize('cfg', [dict(k=3, s=1, p=1, d=1), dict(k=3, s=1, p=2, d=2), dict(k=1, s=1, p=0, d=1), dict(k=1, s=2, p=0, d=1)],
                         ids=['k3', 'k3_dil2', 'k1', 'k1_s2'])
def test_conv_bn_backward_operands_through_the_f64_bound(cfg):
    """The operands of test_kernels_gpu.test_conv_bn_backward_matches_autograd (f32, Cin 64, Cout 96, 13 x 18) held to the derived
    bound instead of that test's fixed tolerances."""
    B, Cin, Cout, H, W = 2, 64, 96, 13, 18
    k, st_, p, d = cfg['k'], cfg['s'], cfg['p'], cfg['d']
    rnd = lambda shape, seed, scale=1.0: torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    x, w = rnd((B, Cin, H, W), 71), rnd((Cout, Cin, k, k), 72, 0.05)
    sc, sh = torch.rand(Cout, generator=torch.Generator().manual_seed(73)) + 0.5, rnd((Cout,), 74, 0.1)
    OH, OW = (H - 1) // st_ + 1, (W - 1) // st_ + 1
    res, go = rnd((B, Cout, OH, OW), 75), rnd((B, Cout, OH, OW), 76)
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().to(DEV)
    xd, rd, wd = nhwc(x).requires_grad_(True), nhwc(res).requires_grad_(True), w.to(DEV).requires_grad_(True)
    s = sc.to(DEV)
    y = TO.ConvFunction.apply(xd, wd, s, sh.to(DEV), rd, True, st_, p, d)
    y.backward(nhwc(go))
    torch.cuda.synchronize()
    w_eff = native.pack_conv_weight(wd.detach(), s, torch.float32)
    st = BR.conv_backward_statement(xd.detach(), w_eff, s, y.detach(), nhwc(go), True, st_, p, d, 'f32')
    name = 'autograd_operands.k%d_s%d_d%d' % (k, st_, d)
    lo, hi = BR.dx_bracket(st, 'f32')
    ratio, bad, _ = R.compare(xd.grad, lo, hi, st['dx'])
    _ratio(name, 'dx', 'f32', ratio, bad)
    ratio, bad = BR.within(wd.grad, st['dw'], BR.dw_bound(st, 'f32', s))
    _ratio(name, 'dw', 'f32', ratio, bad)
    assert torch.equal(rd.grad.double(), st['dr'])
