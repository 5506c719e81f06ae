"""The f64 references of tests/train_kernel_refs.py checked on the host, without a GPU: the RoIAlign interpolation matrix against
the CPU oracle's C restatement (forward and backward), the colsum / pack / fma statements against hand-derived values; and, for
each reference, one plausible kernel mistake applied to it on the CPU, which must move the result by at least ten times the
bound the GPU tests (test_train_kernels_gpu.py) allow."""
import os

import pytest
import torch

from tests import train_kernel_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def O():
    import subprocess
    if not os.path.exists(os.path.join(ROOT, 'oracle', 'libhvr_oracle.so')):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'oracle')], check=True)
    from oracle import hvr_oracle
    return hvr_oracle


def _rois(B, H, W):
    return torch.cat([R.roi_cases(B, H, W, 40, 21), R.edge_rois(B, H, W), R.adaptive_rois(B, H, W)])


def _nhwc_rows(t):
    """[N, C, h, w] -> [N * h * w, C] (the reference's row order)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


CASES = [(2, 15, 15, 8, 2), (3, 38, 63, 8, 2), (2, 15, 15, 8, 0), (3, 38, 63, 8, 0)]


@pytest.mark.parametrize('B,H,W,C,sn', CASES)
def test_roi_matrix_forward_equals_the_oracle(O, B, H, W, C, sn):
    """A F (f64) against oracle.hvr_oracle.roi_align (the C restatement, f32) within the forward bound C_ROI (m + 4) u (A|F|)."""
    rois = _rois(B, H, W)
    F = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(B + H + sn))
    A = R.roi_align_matrix(rois, B, H, W, 7, 7, 1 / 16, sn)
    ref, tol = R.roi_forward_bound(A, _nhwc_rows(F))
    want = _nhwc_rows(O.roi_align(F, rois, 7, 1 / 16, sn)).double()
    empty = (A.sn_h * A.sn_w == 0).repeat_interleave(49)
    assert torch.equal(torch.isnan(want).any(1), empty) and torch.isnan(want[empty]).all()      # 0 / 0 where a bin has no samples
    err = (want[~empty] - ref[~empty]).abs()
    assert bool((err <= tol[~empty]).all()), 'max err %g, bound there %g' % (err.max(), tol[~empty][err.argmax() // C, err.argmax() % C])
    assert float(ref.abs().max()) > 0.1


@pytest.mark.parametrize('B,H,W,C,sn', CASES)
def test_roi_matrix_backward_equals_the_oracle(O, B, H, W, C, sn):
    """A^T G (f64) against O.roi_align_backward within C_ROI (n_cell + 4) u (A^T|G|); the border rules all occur."""
    rois = _rois(B, H, W)
    G = torch.randn((rois.shape[0], C, 7, 7), generator=torch.Generator().manual_seed(5 + B + sn))
    A = R.roi_align_matrix(rois, B, H, W, 7, 7, 1 / 16, sn)
    ref, tol = R.roi_backward_bound(A, _nhwc_rows(G))
    assert torch.allclose(torch.sparse.mm(A.sparse().t(), _nhwc_rows(G).double()), ref, rtol=1e-12, atol=1e-12)   # (the chunked product)
    want = _nhwc_rows(O.roi_align_backward(G, rois, (B, C, H, W), 1 / 16, sn)).double()
    err = (want - ref).abs()
    assert bool((err <= tol).all()), 'max err %g' % float(err.max())
    assert bool((want[tol == 0] == 0).all()) and float(ref.abs().max()) > 0.1
    st = A.stats
    for k in ('y_neg', 'x_neg', 'y_clamped', 'x_clamped', 'y_dead_only', 'x_dead_only', 'live'):
        assert st[k] > 0, (k, st)


@pytest.mark.parametrize('mistake', ['offset', 'border'])
def test_roi_mistakes_exceed_the_bound_tenfold(mistake):
    """A sample offset of s bin / 2 instead of (s + 1/2) bin / 2, or a window (-1, size - 1] instead of (-1, size]: the backward it
    gives differs from the reference by more than ten times the bound, in both sample modes."""
    B, H, W, C = 3, 38, 63, 4
    rois = _rois(B, H, W)
    G = torch.randn((rois.shape[0] * 49, C), generator=torch.Generator().manual_seed(1))
    for sn in (2, 0):
        A = R.roi_align_matrix(rois, B, H, W, 7, 7, 1 / 16, sn)
        ref, tol = R.roi_backward_bound(A, G)
        kw = dict(off_frac=0.0) if mistake == 'offset' else dict(border_mut=True)
        bad = R.apply_T(R.roi_align_matrix(rois, B, H, W, 7, 7, 1 / 16, sn, **kw), G)
        assert float((bad - ref).abs().max()) >= 10 * float(tol.max()), (mistake, sn)


def test_merge_path_statistics_follow_the_kernel_rule():
    """sn == 2 x 2 in NHWC is the merge path; bins under one cell merge taps; NCHW never takes it."""
    rois = R.edge_rois(1, 38, 63)
    A = R.roi_align_matrix(rois, 1, 38, 63, 7, 7, 1 / 16, 2)
    st = R.merge_path_stats(A, True)
    assert st['merge_bins'] == A.rows and st['general_bins'] == 0 and 0 < st['merging_bins'] <= A.rows
    assert R.merge_path_stats(A, False) == dict(merge_bins=0, merging_bins=0, general_bins=A.rows)
    A0 = R.roi_align_matrix(R.adaptive_rois(2, 38, 63), 2, 38, 63, 7, 7, 1 / 16, 0)
    st0 = R.merge_path_stats(A0, True)
    assert st0['merge_bins'] > 0 and st0['general_bins'] > 0
    assert sorted(set(zip(A0.sn_h.tolist(), A0.sn_w.tolist()))) == [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 3)]


# ------------------------------------------------------------------------------- colsum
def test_colsum_slices_rule():
    assert [R.colsum_slices(M, N) for M, N in ((1, 1), (24, 1024), (64, 35), (65, 31), (900, 1024), (4500, 1024), (4500, 1025),
                                               (20000, 1), (20000, 31))] == [1, 1, 1, 2, 15, 64, 61, 256, 256]


@pytest.mark.parametrize('M,N', [(65, 31), (900, 1024), (4500, 1025), (20000, 31)])
def test_colsum_order_within_bound_and_slice_mistake_exceeds_it(M, N):
    """The kernel's summation order, emulated in f32, is within (chain + 1) u sum|x| of the f64 sum; slice y starting at row y
    instead of 4 y (rows summed twice or never) misses by more than ten times that bound."""
    x = torch.randn((M, N), generator=torch.Generator().manual_seed(M + N)) * 3 + 1
    ref, tol = R.colsum_bound(x)
    ok = R.colsum_emulated(x).double()
    assert bool(((ok - ref).abs() <= tol).all())
    bad = R.colsum_emulated(x, slice_start=1).double()
    assert float((bad - ref).abs().max()) >= 10 * float(tol.max())


# ------------------------------------------------------------------------------- pack / unpack
def test_pack_flat_equals_the_statement_and_the_straddle_mistake_is_caught():
    """pack_flat (the multi kernel's element-wise rule) is bit-exact with the per-layer torch statement; decomposing a straddling
    group with its first item's Cin changes elements, which a bit-exact comparison catches."""
    g = torch.Generator().manual_seed(3)
    shapes = [(7, 12, 1, 1), (5, 3, 3, 3), (4, 6, 3, 3), (3, 8, 1, 1)]
    ws = [torch.randn(s, generator=g) for s in shapes]
    ss = [torch.rand(s[0], generator=g) + 0.5 for s in shapes]
    firsts = [0]
    for w in ws[:-1]:
        firsts.append(firsts[-1] + w.numel())
    for dtype in (torch.bfloat16, torch.float16):
        want = torch.cat([R.pack_statement(w, s, dtype).reshape(-1) for w, s in zip(ws, ss)])
        assert torch.equal(R.pack_flat(ws, ss, firsts, dtype).view(torch.int16), want.view(torch.int16))
        bad = R.pack_flat(ws, ss, firsts, dtype, straddle_uses_first_item=True)
        assert int((bad.view(torch.int16) != want.view(torch.int16)).sum()) > 0
    fast, slow, straddle = R.pack_groups([(c, i, kh * kw) for c, i, kh, kw in shapes], firsts, [0] * 4)
    assert straddle == 3 and fast == 0 and slow == (firsts[-1] + ws[-1].numel() + 7) // 8


def test_fma_statement_finds_the_double_rounding_cases():
    """fma_f32: 1 + 2^-23 + 2^-24 (1 - 2^-36) lies just under an f32 midpoint; f64 rounds it onto the midpoint and the f32 tie
    then goes to the even neighbour 1 + 2^-22 -- one ulp off.  The statement returns 1 + 2^-23 and flags it."""
    a = torch.tensor([2.0 ** -24 * (1 + 2.0 ** -18), 0.75, 3.0])
    s = torch.tensor([1 - 2.0 ** -18, 0.5, -1.0])
    d = torch.tensor([1 + 2.0 ** -23, 2.0, 3.0])
    exact, risky, wrong = R.fma_f32(a, s, d)
    assert exact.tolist() == [1 + 2.0 ** -23, 2.375, 0.0]
    assert risky.tolist() == [True, False, False] and wrong.tolist() == [True, False, False]
    assert (a.double() * s.double() + d.double()).float()[0].item() == 1 + 2.0 ** -22
    # a multiply rounded before the add (no fused multiply-add): a bit-exact comparison catches it on random data
    g = torch.Generator().manual_seed(4)
    a, s, d = torch.randn(4096, generator=g), torch.rand(4096, generator=g) + 0.5, torch.randn(4096, generator=g)
    exact, _, _ = R.fma_f32(a, s, d)
    assert int(((a * s + d) != exact).sum()) > 0
