"""GPU tests of the greedy NMS read-out kernels (hvrnet_amd/csrc/nms.hip) through the C ABI: hvr_nms (sort, n x n bit mask, one-wave
sweep), hvr_nms_first (the greedy kernel up to max_keep = 1024, the capped mask / sweep route above) and hvr_multiclass_nms (class
kernel + merge kernel), each against the host statement of tests/nms_refs.py at the sort kernel's 1024-thread edge, the sweep's
word-64 hand-over, the size limit, R at the lane and word edges, 1 and 128 foreground classes, and both sides of the merge's
select / sort switch.  The inputs are the integer-coordinate families on which the statement is exact (plus one float family at sizes
the older tests already cover): EVERY comparison here is exact -- index lists and counts equal, det rows equal bit for bit.  What each
case exercises, and that a planted mistake would change its answer, is checked on the CPU in tests/test_nms_refs.py.

Buffers: every output is over-allocated and poisoned; `keep` must stay poisoned behind n_keep, guard words behind keep, the count
and the workspace (handed over with its exact size) must stay untouched; refused calls write nothing at all."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native  # noqa: E402
from hvrnet_amd.box_ops import multiclass_nms  # noqa: E402
from tests import nms_refs as R  # noqa: E402

DEV = 'cuda:0'
GUARD = 64                      # guard words / rows behind every buffer
POISON64 = -0x0123456789ABCDEF
POISON32 = 0x5A5A5A5A
POISON_F = 7777.0
WS_BYTE = 0xA5
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _workspace(need):
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    ws[need:] = WS_BYTE
    return ws


def _nms_buffers(n):
    keep = torch.full((n + GUARD,), POISON64, dtype=torch.long, device=DEV)
    cnt = torch.full((1 + GUARD,), POISON32, dtype=torch.int32, device=DEV)
    return keep, cnt


def _run_nms(dets, thr, ge, max_keep=None):
    """hvr_nms (max_keep None) / hvr_nms_first on dets [n,5] (numpy) -> the keep list; asserts the buffer discipline"""
    lib = native.lib()
    n = len(dets)
    d = torch.from_numpy(np.array(dets, dtype=np.float32)).to(DEV)      # (a copy: the cases' arrays are read-only)
    keep, cnt = _nms_buffers(n)
    need = lib.hvr_nms_workspace_bytes(n)
    ws = _workspace(need)
    if max_keep is None:
        rc = lib.hvr_nms(_ptr(d), n, float(thr), int(ge), _ptr(keep), _ptr(cnt), _ptr(ws), need, native._stream())
    else:
        rc = lib.hvr_nms_first(_ptr(d), n, float(thr), int(ge), int(max_keep), _ptr(keep), _ptr(cnt), _ptr(ws), need, native._stream())
    assert rc == 0, lib.hvr_last_error()
    torch.cuda.synchronize()
    cnt_h, keep_h = cnt.cpu(), keep.cpu()
    k = int(cnt_h[0])
    assert 0 <= k <= n
    assert bool((keep_h[k:] == POISON64).all()), 'keep was written behind n_keep'
    assert bool((cnt_h[1:] == POISON32).all()), 'the words behind n_keep were written'
    assert bool((ws[need:] == WS_BYTE).all()), 'the bytes behind the workspace were written'
    return keep_h[:k].tolist()


# ------------------------------------------------------------------------------------------------ hvr_nms
def test_one_box_survives():
    """n = 1: a one-element sort, one ragged chunk.  (No mistake can change this answer: it is run as the size edge it is.)"""
    d = R.family('sparse', 1, 1)
    for ge in (True, False):
        assert _run_nms(d, 0.5, ge) == [0]
    assert _run_nms(d, 0.5, True, 1) == [0] and _run_nms(d, 0.5, True, 1025) == [0]


@pytest.mark.parametrize('fam,n,thr,ge', R.NMS_CASES, ids=['%s-%d-%.2f-%s' % (f, n, t, 'ge' if g else 'gt') for f, n, t, g in R.NMS_CASES])
def test_nms_equals_the_statement(fam, n, thr, ge):
    sweep, info = R.case_sweep(fam, n, thr, ge)
    want = R.cut_sweep(sweep)
    got = _run_nms(R.case_dets(fam, n), thr, ge)
    print('%s n=%d thr=%.3f ge=%d: %d survivors, %d IoUs on thr, last survivor at %d' % (fam, n, thr, ge, info['survivors'],
                                                                                         info['exact_hits'], info['last_survivor_pos']))
    assert len(got) == len(want) and got == want


# ------------------------------------------------------------------------------------------------ hvr_nms_first
FIRST_FAM_N = sorted(set((c[0], c[1]) for c in R.FIRST_CASES))


@pytest.mark.parametrize('fam,n', FIRST_FAM_N)
def test_nms_first_equals_the_statement_on_both_routes(fam, n):
    """max_keep <= 1024: nms_greedy_kernel; above: mask + sweep with the survivor cap.  Each result against the statement; and the
    1024 result (greedy kernel) against the 1025 result (capped sweep) on the same input by containment: the first is the 1024 best
    in score order of the second."""
    cases = [(thr, k) for (f, m, thr, k) in R.FIRST_CASES if (f, m) == (fam, n)]
    dets = R.case_dets(fam, n)
    got = {}
    for thr, k in cases:
        sweep, info = R.case_sweep(fam, n, thr, True)
        mk = R.first_keep(n, k, info['survivors'])
        ci = {}
        want = R.cut_sweep(sweep, mk, None, ci)
        got[k] = _run_nms(dets, thr, True, mk)
        print('%s n=%d max_keep=%d (%s): cap %s' % (fam, n, mk, 'greedy kernel' if mk <= 1024 else 'mask + capped sweep', R.cap_place(n, ci)))
        assert len(got[k]) == len(want) and got[k] == want, (k, mk)
    a, b = got[1024], got[1025]
    order = R.visiting_order(dets[:, 4])
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    assert a == sorted(sorted(b, key=lambda i: rank[i])[:1024])


# ------------------------------------------------------------------------------------------------ refusals of hvr_nms / hvr_nms_first
def _refused(call, rc_want, word):
    lib = native.lib()
    rc = call()
    msg = lib.hvr_last_error()
    torch.cuda.synchronize()
    assert rc == rc_want and msg and word in msg, (rc, msg)


def test_nms_refusals_write_nothing():
    lib = native.lib()
    n = 8193
    d = torch.zeros((n, 5), device=DEV)
    keep, cnt = _nms_buffers(n)
    need = lib.hvr_nms_workspace_bytes(8192)
    ws = torch.full((need + 256,), WS_BYTE, dtype=torch.uint8, device=DEV)
    s = native._stream()
    _refused(lambda: lib.hvr_nms(_ptr(d), n, 0.5, 1, _ptr(keep), _ptr(cnt), _ptr(ws), ws.numel(), s), EUNSUPPORTED, b'8192')
    _refused(lambda: lib.hvr_nms_first(_ptr(d), n, 0.5, 1, 10, _ptr(keep), _ptr(cnt), _ptr(ws), ws.numel(), s), EUNSUPPORTED, b'8192')
    _refused(lambda: lib.hvr_nms_first(_ptr(d), 100, 0.5, 1, 0, _ptr(keep), _ptr(cnt), _ptr(ws), ws.numel(), s), EINVAL, b'max_keep')
    _refused(lambda: lib.hvr_nms(_ptr(d), 8192, 0.5, 1, _ptr(keep), _ptr(cnt), _ptr(ws), need - 1, s), EWORKSPACE, b'workspace')
    _refused(lambda: lib.hvr_nms_first(_ptr(d), 8192, 0.5, 1, 10, _ptr(keep), _ptr(cnt), _ptr(ws), need - 1, s), EWORKSPACE, b'workspace')
    assert bool((keep == POISON64).all()) and bool((cnt == POISON32).all()) and bool((ws == WS_BYTE).all())


# ------------------------------------------------------------------------------------------------ hvr_multiclass_nms
def _mc_buffers(max_num):
    dets = torch.full((max_num + GUARD, 5), POISON_F, dtype=torch.float32, device=DEV)
    labels = torch.full((max_num + GUARD,), POISON64, dtype=torch.long, device=DEV)
    n_out = torch.full((1 + GUARD,), POISON32, dtype=torch.int32, device=DEV)
    return dets, labels, n_out


def _run_mc(boxes, scores, score_thr, iou_thr, max_num):
    """hvr_multiclass_nms -> (dets [k,5], labels [k]) numpy; asserts zero rows behind n_out and untouched guards"""
    lib = native.lib()
    Rr, ncls = scores.shape
    b = torch.from_numpy(np.array(boxes, dtype=np.float32)).to(DEV)
    s = torch.from_numpy(np.array(scores, dtype=np.float32)).to(DEV)
    dets, labels, n_out = _mc_buffers(max_num)
    need = lib.hvr_multiclass_nms_workspace_bytes(Rr, ncls)
    assert need > 0
    ws = _workspace(need)
    rc = lib.hvr_multiclass_nms(_ptr(b), _ptr(s), Rr, ncls, float(score_thr), float(iou_thr), int(max_num), _ptr(dets), _ptr(labels),
                                _ptr(n_out), _ptr(ws), need, native._stream())
    assert rc == 0, lib.hvr_last_error()
    torch.cuda.synchronize()
    dh, lh, nh = dets.cpu(), labels.cpu(), n_out.cpu()
    k = int(nh[0])
    assert 0 <= k <= max_num
    assert not bool(dh[k:max_num].any()) and not bool(lh[k:max_num].any()), 'rows behind n_out are not zero'
    assert bool((dh[max_num:] == POISON_F).all()) and bool((lh[max_num:] == POISON64).all()), 'guard rows behind max_num were written'
    assert bool((nh[1:] == POISON32).all()) and bool((ws[need:] == WS_BYTE).all())
    return dh[:k].numpy(), lh[:k].numpy()


def _same(got, want, what):
    assert got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    assert got[1].tolist() == want[1].tolist(), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


@pytest.mark.parametrize('iou_thr', R.MC_IOUS)
@pytest.mark.parametrize('Rr,ncls', R.MC_SHAPES)
def test_multiclass_nms_equals_the_statement(Rr, ncls, iou_thr):
    """max_num in {1, 7, 100, total - 1, total, total + 1}: the cut by radix select, no cut, and (max_num >= (ncls - 1) R) the
    in-place form; classes without a candidate between full ones, scores ON score_thr, IoUs ON 0.5, ties at the cut."""
    boxes, scores = R.mc_inputs(Rr, ncls)
    lst, info = R.mc_list(Rr, ncls, iou_thr)
    print('R=%d ncls=%d iou %.1f: %d candidates, %d survivors, %d classes without a candidate' % (
        Rr, ncls, iou_thr, sum(info['candidates']), info['total'], sum(1 for c in info['candidates'] if c == 0)))
    for max_num in R.mc_max_nums(info['total']):
        want = R.cut_list(boxes, lst, max_num)
        _same(_run_mc(boxes, scores, R.MC_SCORE_THR, iou_thr, max_num), want, (Rr, ncls, iou_thr, max_num))


@pytest.mark.parametrize('Rr,ncls', R.MC_BOUNDARY_SHAPES)
def test_multiclass_nms_on_both_sides_of_the_select_sort_switch(Rr, ncls):
    """run_multiclass_nms gives the merge kernel a select list of sp2 = next_pow2(max_num) entries unless
    next_pow2((ncls - 1) R) * 8 + sp2 * 8 exceeds the kernel's 160 KiB - 3072 of LDS (or max_num covers every candidate); then it sorts
    the whole list in place.  R.mc_sp2 restates that rule; the boundary is the largest max_num it gives a select list."""
    m = R.mc_sp2_boundary(Rr, ncls)
    assert R.mc_sp2(Rr, ncls, m) > 0 and R.mc_sp2(Rr, ncls, m + 1) == 0
    boxes, scores = R.mc_inputs(Rr, ncls, 'sparse')
    lst, info = R.mc_list(Rr, ncls, 0.5, 'sparse')
    assert info['total'] > m + 1
    for max_num in (m, m + 1):
        _same(_run_mc(boxes, scores, R.MC_SCORE_THR, 0.5, max_num), R.cut_list(boxes, lst, max_num), (Rr, ncls, max_num))


def test_multiclass_nms_refusals_launch_nothing_and_write_nothing():
    """max_num <= 0 (HVR_EINVAL); ncls < 2, more than 128 foreground classes, R > 512, a candidate list the merge kernel's LDS cannot
    hold (HVR_EUNSUPPORTED, the limit named).  dets, labels and n_out keep their poison; the workspace query answers 0 outside the
    envelope."""
    lib = native.lib()
    b = torch.zeros((600, 4), device=DEV)
    s = torch.zeros((600 * 130,), device=DEV)
    dets, labels, n_out = _mc_buffers(8)
    ws = torch.full((1 << 20,), WS_BYTE, dtype=torch.uint8, device=DEV)
    st = native._stream()

    def call(Rr, ncls, max_num):
        return lambda: lib.hvr_multiclass_nms(_ptr(b), _ptr(s), Rr, ncls, 0.1, 0.5, max_num, _ptr(dets), _ptr(labels), _ptr(n_out), _ptr(ws),
                                              ws.numel(), st)
    _refused(call(64, 31, 0), EINVAL, b'max_num > 0')
    _refused(call(64, 31, -3), EINVAL, b'max_num > 0')
    _refused(call(64, 1, 8), EUNSUPPORTED, b'1 .. 128 foreground classes')
    _refused(call(64, 0, 8), EUNSUPPORTED, b'1 .. 128 foreground classes')
    _refused(call(4, 130, 8), EUNSUPPORTED, b'1 .. 128 foreground classes')
    _refused(call(513, 2, 8), EUNSUPPORTED, b'R <= 512')
    limit = 1           # the longest list: next_pow2(list) * 8 bytes <= the merge kernel's LDS (include/hvr_hip.h says 16384)
    while limit * 2 * 8 <= R.MC_LDS_CAP:
        limit *= 2
    assert limit == 128 * 128       # (the largest case test_multiclass_nms_equals_the_statement runs sits exactly on it)
    _refused(call(512, 129, 8), EUNSUPPORTED, b'%d' % limit)
    _refused(call(129, 129, 8), EUNSUPPORTED, b'%d' % limit)      # 128 x 129 = 16512 candidates, the first R above the limit
    assert bool((dets == POISON_F).all()) and bool((labels == POISON64).all()) and bool((n_out == POISON32).all())
    assert bool((ws == WS_BYTE).all())
    for Rr, ncls in ((64, 1), (4, 130), (513, 2), (512, 129), (0, 31)):
        assert lib.hvr_multiclass_nms_workspace_bytes(Rr, ncls) == 0
    assert lib.hvr_multiclass_nms_workspace_bytes(128, 129) > 0 and lib.hvr_multiclass_nms_workspace_bytes(512, 33) > 0
    assert lib.hvr_multiclass_nms_workspace_bytes(512, 34) == 0


def test_rpn_proposals_refuses_empty_shapes_and_caps():
    """T <= 0, A <= 0, nms_post <= 0 and max_num <= 0 each reached a launch (an empty grid, or a gather that wrote a negative count):
    HVR_EINVAL before anything is launched, proposals and counts untouched."""
    lib = native.lib()
    T, H, W, A = 1, 4, 4, 3
    cls = torch.zeros((T, H, W, A), device=DEV)
    reg = torch.zeros((T, H, W, 4 * A), device=DEV)
    props = torch.full((T, 8, 5), POISON_F, device=DEV)
    counts = torch.full((T,), POISON32, dtype=torch.int32, device=DEV)
    base = (ctypes.c_float * (A * 4))(*([0.0, 0.0, 15.0, 15.0] * A))
    mm, ss = (ctypes.c_float * 4)(0, 0, 0, 0), (ctypes.c_float * 4)(1, 1, 1, 1)
    ws = torch.full((lib.hvr_rpn_workspace_bytes(T, H, W, A, 6000),), WS_BYTE, dtype=torch.uint8, device=DEV)

    def call(**kw):
        f = dict(T=T, A=A, nms_post=8, max_num=8)
        f.update(kw)
        d = native.RpnDesc(cls=cls.data_ptr(), reg=reg.data_ptr(), T=f['T'], H=H, W=W, A=f['A'], anchor_stride=16,
                           base_anchors=ctypes.cast(base, ctypes.c_void_p), means=ctypes.cast(mm, ctypes.c_void_p),
                           stds=ctypes.cast(ss, ctypes.c_void_p), img_h=64.0, img_w=64.0, wh_ratio_clip=16 / 1000, nms_pre=6000,
                           nms_post=f['nms_post'], max_num=f['max_num'], nms_thr=0.7, proposals=props.data_ptr(), counts=counts.data_ptr(),
                           cls_pitch=A, reg_pitch=4 * A)
        return lambda: lib.hvr_rpn_proposals(ctypes.byref(d), _ptr(ws), ws.numel(), native._stream())
    for kw, word in ((dict(T=0), b'T >= 1'), (dict(T=-2), b'T >= 1'), (dict(A=0), b'A >= 1'), (dict(nms_post=0), b'nms_post > 0'),
                     (dict(nms_post=-1), b'nms_post > 0'), (dict(max_num=0), b'max_num > 0'), (dict(max_num=-5), b'max_num > 0')):
        _refused(call(**kw), EINVAL, word)
    assert bool((props == POISON_F).all()) and bool((counts == POISON32).all()) and bool((ws == WS_BYTE).all())


# ------------------------------------------------------------------------------------------------ the Python wrapper's negative path
@pytest.mark.parametrize('max_num', [-1, -7])
def test_wrapper_negative_max_num_at_a_second_shape(max_num):
    """box_ops.multiclass_nms with the reference's default max_num = -1 (and -7) at R = 64: every survivor sorted by score, the last
    |max_num| dropped (bbox_nms.py:55-59 as written; tests/test_nms_refs.py holds the statement's reading to the oracle's)."""
    boxes, scores = R.mc_inputs(64, 31)
    want = R.multiclass_nms(boxes, scores, R.MC_SCORE_THR, 0.5, max_num)
    db, dl = multiclass_nms(torch.from_numpy(boxes.copy()).to(DEV), torch.from_numpy(scores.copy()).to(DEV), R.MC_SCORE_THR,
                            dict(type='nms', iou_thr=0.5), max_num)
    _same((db.cpu().numpy(), dl.cpu().numpy()), want, max_num)
