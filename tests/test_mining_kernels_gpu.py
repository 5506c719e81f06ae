"""The selection kernels and the triplet term of the training step (targets.hip) against the statements of tests/mining_refs.py:
hvr_sample_pos_neg, hvr_mining_argreduce, hvr_triplet_margin, called through the C entry points on buffers the test owns (every
output carries guard rows filled with a sentinel behind it) and through the native.* / train_ops wrappers.

Index outputs are compared for equality; the triplet's distances, loss and gradients against the derived bounds of
mining_refs.triplet_statement (nothing is measured against the device; tests/test_mining_refs.py shows each bound wide enough for
an independent f32 evaluation and every listed mistake ten bounds away).  Each comparison prints
`RATIO <call> <mode> <worst error / bound>` (pytest -s shows it); for an index output the figure is 0 or inf.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native, train_ops as TO  # noqa: E402
from tests import mining_refs as M  # noqa: E402

DEV = 'cuda:0'
GUARD = 3
SENT_I = -7777
SENT_F = -12345.5
NAMES = {torch.float32: 'f32', torch.bfloat16: 'bf16'}


def _guarded(shape, dtype, fill):
    """(buffer with GUARD extra leading-dimension rows, all `fill`; the view the kernel is given)"""
    buf = torch.full((shape[0] + GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device=DEV)
    return buf, buf[:shape[0]]


def _guard_intact(buf, rows, fill):
    return bool((buf[rows:] == fill).all())


def _check_val(call, mode, got, val):
    worst, at, over = M.ratio(got.cpu(), val)
    print('RATIO %s %s %.4g' % (call, mode, worst))
    assert worst <= 1.0, '%s %s: %d of %d elements over the bound, worst error / bound %g at flat index %d (got %r, statement %r +- %r)' % (
        call, mode, over, val.v.numel(), worst, at, float(got.reshape(-1)[at]), float(val.v.reshape(-1)[at]), float(val.e.reshape(-1)[at]))
    return worst


# ------------------------------------------------------------------------------------------------ sampler
def _sample_raw(cls, keys, num, ep, ub):
    inds_buf, inds = _guarded((num,), torch.long, SENT_I)
    counts_buf, counts = _guarded((2,), torch.int32, SENT_I)
    rc = native.lib().hvr_sample_pos_neg(native._ptr(cls), native._ptr(keys), cls.numel(), int(num), int(ep), float(ub), native._ptr(inds),
                                         native._ptr(counts), native._stream())
    native._check(rc, 'hvr_sample_pos_neg')
    assert _guard_intact(inds_buf, num, SENT_I) and _guard_intact(counts_buf, 2, SENT_I), 'sampler wrote behind its outputs'
    return inds.cpu(), counts.cpu()


def _sampler_compare(calls, mode):
    bad = []
    total = 0
    for cls, keys, num, ep, ub in calls:
        want, (n_pos, n_neg) = M.sample_statement(cls, keys, num, ep, ub)
        inds, counts = _sample_raw(cls.to(DEV), keys.to(DEV), num, ep, ub)
        c = counts.tolist()
        total += 1
        # rows of inds behind counts[0] + counts[1] are left unwritten by the kernel: only the counted prefix is compared
        if c != [n_pos, n_neg] or not torch.equal(inds[:n_pos + n_neg], want):
            first = [i for i in range(min(sum(c), want.numel())) if int(inds[i]) != int(want[i])][:1] if c == [n_pos, n_neg] else []
            bad.append('n %d num %d expected_pos %d ub %g: counts %s, statement %s, first differing row %s'
                       % (cls.numel(), num, ep, ub, c, [n_pos, n_neg], first))
    print('RATIO sample_pos_neg %s %s' % (mode, 'inf' if bad else '0'))
    assert not bad, '%d of %d calls differ: %s' % (len(bad), total, '; '.join(bad[:4]))
    return total


@pytest.mark.parametrize('n', M.SAMPLE_N)
def test_sampler_against_statement(n):
    """One 1 024-thread workgroup, segment ceil(n / 1024): n on both sides of 64 (one wavefront), of 1 024 (segment 1 -> 2) and of
    2 048 (2 -> 3), and 5 000.  Key families: continuous, quarter steps, negative, all equal, +-0.0 mixed with +-inf, and keys that
    share their upper 24 bits (only the last radix pass separates them).  Without a cap: expected on each side of both group sizes,
    the negatives filling up after a short positive group, num > n; then neg_pos_ub 0, 2 and 1e10 (a product beyond int: no cap).
    tests/test_mining_refs.py asserts the sizes these calls actually sample (mining_refs.sample_configs)."""
    assert (n + 1023) // 1024 == {1: 1, 63: 1, 64: 1, 65: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2049: 3, 5000: 5}[n]
    assert _sampler_compare(M.sample_calls(n), 'n%d' % n) >= 40


def test_sampler_fractional_cap_is_the_double_product():
    """int(neg_pos_ub * np) as the reference's Python computes it: 0.29 x 100 -> 28, 1.16 x 25 -> 28, 0.21 x 300 -> 63 (an f32 product
    gives 29, 29, 62).  Through the C entry and through native.sample_pos_neg."""
    _sampler_compare(M.sample_calls(None), 'fractional_ub')
    for (ub, n_pos), cap in zip(M.SAMPLE_FRACTIONAL, (28, 28, 63)):
        cls, keys, num, ep = M.sample_fractional_case(ub, n_pos)
        want, wc = M.sample_statement(cls, keys, num, ep, ub)
        inds, counts = native.sample_pos_neg(cls.to(DEV), keys.to(DEV), num, ep, ub)
        assert counts.tolist() == [n_pos, cap] == list(wc) and torch.equal(inds[:n_pos + cap].cpu(), want)


def test_sampler_signed_zeros_tie():
    """-0.0 and +0.0 are one key: the lower index wins whatever the sign.  Eight candidates per group, zeros of alternating sign."""
    cls = torch.tensor([1, 0] * 8)
    keys = torch.tensor([0.0, 0.0, -0.0, -0.0] * 4)
    for ep in (1, 2, 3, 5):
        inds, counts = _sample_raw(cls.to(DEV), keys.to(DEV), 2 * ep, ep, -1.0)
        want, wc = M.sample_statement(cls, keys, 2 * ep, ep, -1.0)
        assert counts.tolist() == [ep, ep] == list(wc)
        assert inds.tolist() == want.tolist() == [2 * i for i in range(ep)] + [2 * i + 1 for i in range(ep)]


# ------------------------------------------------------------------------------------------------ mining
def _mining_raw(view, labels, all_labels):
    Mq, Mk = view.shape
    out_buf, out = _guarded((Mq, 4), torch.long, SENT_I)
    rc = native.lib().hvr_mining_argreduce(native._ptr(view), Mq, Mk, view.stride(0), native._ptr(labels), native._ptr(all_labels), native._ptr(out),
                                           native._stream())
    native._check(rc, 'hvr_mining_argreduce')
    assert _guard_intact(out_buf, Mq, SENT_I), 'mining wrote behind its output'
    return out.cpu()


@pytest.mark.parametrize('Mk', M.MINING_MK)
def test_mining_against_statement(Mk):
    """One wavefront per row, four rows per block: Mq in {1, 3, 4, 5, 9}, Mk on both sides of one and two 64-lane strides.  aff is
    a column slice of a wider buffer -- pitch Mk + 3 filled with +3e38 outside the slice, pitch Mk rounded up to 4 filled with -3e38
    (a read past the row would win the maximum / the minimum).  Continuous and quarter-step values, rows holding +-inf, labels that
    match no key / every key, exactly one candidate, the maximum duplicated 64 apart, negative and large int64 labels.  All four
    columns of every row are compared."""
    bad = []
    total = 0
    for Mq in M.MINING_MQ:
        for kind in M.MINING_KINDS:
            aff, labels, all_labels = M.mining_case(Mq, Mk, kind)
            want = M.mining_statement(aff, labels, all_labels)
            lab, alab = labels.to(DEV), all_labels.to(DEV)
            for pitch, fill in ((Mk + 3, M.BIG_F32), ((Mk + 3) // 4 * 4, -M.BIG_F32)):
                buf = torch.full((Mq, pitch), fill)
                buf[:, :Mk] = aff
                view = buf.to(DEV)[:, :Mk]
                assert view.stride(0) == pitch
                got = _mining_raw(view, lab, alab)
                total += 1
                if not torch.equal(got, want):
                    r = int((got != want).any(1).nonzero()[0])
                    bad.append('Mq %d Mk %d %s pitch %d: row %d got %s, statement %s' % (Mq, Mk, kind, pitch, r, got[r].tolist(), want[r].tolist()))
            assert torch.equal(native.mining_argreduce(view, lab, alab).cpu(), want)
    print('RATIO mining_argreduce Mk%d %s' % (Mk, 'inf' if bad else '0'))
    assert not bad, '%d of %d calls differ: %s' % (len(bad), total, '; '.join(bad[:4]))


# ------------------------------------------------------------------------------------------------ triplet
TRIPLET = [(name, c, dt) for name, c in M.triplet_cases() for dt in M.TRIPLET_DTYPES]
IDS = ['%s-%s' % (name, NAMES[dt]) for name, c, dt in TRIPLET]
DT_CODE = {torch.float32: native.HVR_F32, torch.bfloat16: native.HVR_BF16}


def _triplet_raw(q, k, a, p, m, margin, need_grad=True, dtype_code=None, ldq=None, ldk=None, ws_bytes=None):
    """hvr_triplet_margin on guarded buffers -> (rc, ws [n, 3], out2, dq, dk, guards intact)."""
    (Mq, D), Mk, n = q.shape, k.shape[0], a.numel()
    ws_buf, ws = _guarded((n, 3), torch.float32, SENT_F)
    out_buf, out2 = _guarded((2,), torch.float32, SENT_F)
    dq_buf, dq = _guarded((Mq, D), torch.float32, SENT_F)
    dk_buf, dk = _guarded((Mk, D), torch.float32, SENT_F)
    rc = native.lib().hvr_triplet_margin(native._ptr(q), q.stride(0) if ldq is None else ldq, native._ptr(k), k.stride(0) if ldk is None else ldk,
                                         D, Mq, Mk, native._ptr(a), native._ptr(p), native._ptr(m), n, float(margin),
                                         native._dt(q) if dtype_code is None else dtype_code, native._ptr(ws), n * 12 if ws_bytes is None else ws_bytes,
                                         native._ptr(out2), native._ptr(dq if need_grad else None), native._ptr(dk if need_grad else None),
                                         native._stream())
    torch.cuda.synchronize()
    intact = _guard_intact(ws_buf, n, SENT_F) and _guard_intact(out_buf, 2, SENT_F) and _guard_intact(dq_buf, Mq, SENT_F) and \
        _guard_intact(dk_buf, Mk, SENT_F)
    return rc, ws, out2, dq, dk, intact


def _untouched(*bufs):
    return all(bool((b == SENT_F).all()) for b in bufs)


@pytest.mark.parametrize('name,c,dt', TRIPLET, ids=IDS)
def test_triplet_against_statement(name, c, dt):
    """triplet_dist_kernel (one wavefront per triple, four per block, lanes stride D by 64) and triplet_grad_kernel (256 lanes reduce
    the n losses, one lane per column walks the triples): D on both sides of 64 and 256, n on both sides of 4 and 256; rows
    contiguous and pitched (ld = D + 8, a slice of a NaN-filled buffer) give identical bits; distances, clamped l, loss, active count
    (exact), dq and dk within the derived bounds, rows no active triple names exactly zero; need_grad=False and the native wrapper
    return the same out2 bits."""
    case = M.triplet_case(name, c, dt)
    ref = M.triplet_statement(**case)
    assert ref['decision'] > 10.0                                    # (asserted for every case on the host as well)
    a, p, m = case['a'].to(DEV), case['p'].to(DEV), case['m'].to(DEV)
    mode = NAMES[dt]
    first = None
    for layout in ('contiguous', 'pitched'):
        q, k = case['q'].to(DEV), case['k'].to(DEV)
        if layout == 'pitched':
            q, k = M.pitched(q), M.pitched(k)
            assert q.stride(0) == c['D'] + M.PITCH_PAD and k.stride(0) == c['D'] + M.PITCH_PAD
        rc, ws, out2, dq, dk, intact = _triplet_raw(q, k, a, p, m, case['margin'])
        native._check(rc, 'hvr_triplet_margin')
        assert intact, 'triplet wrote behind an output'
        if first is None:
            first = (ws.clone(), out2.clone(), dq.clone(), dk.clone())
            call = 'triplet.%s' % name
            _check_val(call + '.dp', mode, ws[:, 0], ref['dp'])
            _check_val(call + '.dn', mode, ws[:, 1], ref['dn'])
            _check_val(call + '.l', mode, ws[:, 2], ref['l'].clamp(min=0.0))
            assert int(out2[1]) == int(ref['active'].sum()) and torch.equal(ws[:, 2].cpu() > 0, ref['active'])
            _check_val(call + '.out2', mode, out2, ref['out2'])
            _check_val(call + '.dq', mode, dq, ref['dq'])
            _check_val(call + '.dk', mode, dk, ref['dk'])
            assert not bool(dq.cpu()[ref['count_q'] == 0].any()) and not bool(dk.cpu()[ref['count_k'] == 0].any())
            if c['kind'] == 'all_inactive':
                assert out2.tolist() == [0.0, 0.0] and not bool(dq.any()) and not bool(dk.any())
            if c['kind'] == 'exact_zero':
                i = min(1, c['n'] - 1)
                assert float(ws[i, 2]) == 0.0 and float(ws[i, 0]) == float(ws[i, 1])
        else:
            for x, y in zip(first, (ws, out2, dq, dk)):
                assert torch.equal(x, y), 'pitched rows change the result'
        rc, _, out2_ng, dq_ng, dk_ng, intact = _triplet_raw(q, k, a, p, m, case['margin'], need_grad=False)
        native._check(rc, 'hvr_triplet_margin')
        assert intact and torch.equal(out2_ng, out2) and _untouched(dq_ng, dk_ng)
        w2, wq, wk = native.triplet_margin(q, k, a, p, m, case['margin'])
        assert torch.equal(w2, out2) and torch.equal(wq, dq) and torch.equal(wk, dk)
        w2, wq, wk = native.triplet_margin(q, k, a, p, m, case['margin'], need_grad=False)
        assert torch.equal(w2, out2) and wq is None and wk is None


@pytest.mark.parametrize('name', ['n257-collide', 'equal_row'])
def test_triplet_backward_on_bf16_is_the_f32_gradient_rounded_once(name):
    """train_ops.triplet_margin on bf16 operands: loss and active count are the kernel's f32 out2, the gradients its f32 dq / dk
    rounded to bf16 once (to nearest even)."""
    c = dict(M.triplet_cases())[name]
    case = M.triplet_case(name, c, torch.bfloat16)
    a, p, m = case['a'].to(DEV), case['p'].to(DEV), case['m'].to(DEV)
    q, k = case['q'].to(DEV).requires_grad_(True), case['k'].to(DEV).requires_grad_(True)
    out2, dq, dk = native.triplet_margin(q.detach(), k.detach(), a, p, m, case['margin'])
    loss, active = TO.triplet_margin(q, k, a, p, m, case['margin'])
    loss.backward()
    assert float(loss.detach()) == float(out2[0]) and float(active) == float(out2[1])
    assert q.grad.dtype == torch.bfloat16 and k.grad.dtype == torch.bfloat16
    assert torch.equal(q.grad, dq.to(torch.bfloat16)) and torch.equal(k.grad, dk.to(torch.bfloat16))
    assert bool(dq.any()) and bool((dq != dq.to(torch.bfloat16).float()).any())        # (the rounding is not vacuous)


def test_triplet_refusals_launch_nothing():
    """f16 and split-half operands, ld < D and a short workspace are refused with HvrError before any launch: the sentinel-filled
    outputs stay untouched."""
    c = dict(M.triplet_cases())['D65-plain']
    case = M.triplet_case('D65-plain', c, torch.float32)
    q, k = case['q'].to(DEV), case['k'].to(DEV)
    a, p, m = case['a'].to(DEV), case['p'].to(DEV), case['m'].to(DEV)
    D, n = c['D'], c['n']
    refusals = [dict(dtype_code=native.HVR_F16), dict(dtype_code=native.HVR_F16S), dict(ldq=D - 1), dict(ldk=D - 1), dict(ws_bytes=n * 12 - 4)]
    for kw in refusals:
        rc, ws, out2, dq, dk, intact = _triplet_raw(q, k, a, p, m, 10.0, **kw)
        assert rc != 0, kw
        with pytest.raises(native.HvrError):
            native._check(rc, 'hvr_triplet_margin')
        assert intact and _untouched(ws, out2, dq, dk), kw
    with pytest.raises(native.HvrError):
        native.triplet_margin(q.half(), k.half(), a, p, m, 10.0)
    with pytest.raises(native.HvrError):
        native.triplet_margin(torch.zeros((7, 64), dtype=native.SPLIT, device=DEV), torch.zeros((9, 64), dtype=native.SPLIT, device=DEV), a, p, m, 10.0)
    rc, ws, out2, dq, dk, intact = _triplet_raw(q, k, a, p, m, 10.0)                     # (the same call without a fault goes through)
    assert rc == 0 and intact and not _untouched(out2)
