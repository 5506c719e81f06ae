"""The training step's kernels against the f64 statements of tests/train_kernel_refs.py, at the shapes training runs and at the
edges where they branch: RoIAlign backward (roi_align.hip), the bias gradient hvr_colsum, and the weight side of an iteration
(pack_conv_weight / pack_conv_weights_multi, transpose_multi, unpack_conv_wgrad / unpack_conv_wgrads_multi).

Every test states its bound and asserts, from the kernel's documented selection rule, that the branch it targets ran.
Bounds (u = 2^-24, the f32 unit roundoff):
  * RoIAlign backward, per element: C_ROI (n_cell + 4) u (A^T|G|) + E^T|G|, C_ROI = 2: n_cell f32 atomics in any order, up to five
    roundings inside one contribution; E: where a fused multiply-add may move a sample coordinate (train_kernel_refs docstring);
  * colsum, per column: (longest chain of f32 additions + 1) u sum|x|, the chain from colsum_slices;
  * pack / transpose / unpack: bit for bit (one rounding, or none); accumulate: the correctly rounded fma.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native, ops  # noqa: E402
from tests import train_kernel_refs as R  # noqa: E402

DEV = 'cuda:0'
PH = PW = 7
SCALE = 1 / 16


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).to(dtype)


def _rows_nhwc(t):
    """a [N, h, w, C] tensor -> [N * h * w, C]"""
    return t.reshape(-1, t.shape[-1])


def _roi_bwd_check(rois, B, H, W, C, sn, layout, seed, A=None):
    """native.roi_align_bwd in `layout` against A^T G, element by element; -> (A, G rows, bound, kernel rows) for further checks."""
    A = A or R.roi_align_matrix(rois, B, H, W, PH, PW, SCALE, sn).to(DEV)
    K = rois.shape[0]
    G = _randn((K * PH * PW, C), seed)                                  # rows (roi, ph, pw), channels last
    if layout == native.LAYOUT_NHWC:
        got = _rows_nhwc(native.roi_align_bwd(G.view(K, PH, PW, C), rois.to(DEV), (B, H, W, C), SCALE, sn, layout))
    else:
        g_nchw = G.view(K, PH, PW, C).permute(0, 3, 1, 2).contiguous()
        got = _rows_nhwc(native.roi_align_bwd(g_nchw, rois.to(DEV), (B, C, H, W), SCALE, sn, layout).permute(0, 2, 3, 1))
    ref, tol = R.roi_backward_bound(A, G)
    err = (got.double() - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), '%d elements over the bound; worst excess %g (err %g, bound %g)' % (
        int(bad.sum()), float((err - tol).max()), float(err.flatten()[(err - tol).argmax()]), float(tol.flatten()[(err - tol).argmax()]))
    assert float(ref.abs().max()) > 0.1
    return A, G, tol, got


LAYOUTS = [('nhwc', native.LAYOUT_NHWC), ('nchw', native.LAYOUT_NCHW)]


@pytest.mark.parametrize('layout_name,layout', LAYOUTS)
@pytest.mark.parametrize('B,K', [(3, 900), (15, 4500)])
def test_roi_align_backward_training_size(B, K, layout_name, layout):
    """sample_num = 2 on 38 x 63 x 1 024 maps, 7 x 7 bins: the training step's RoIAlign backward.  NHWC takes the 2 x 2 merge path
    for every bin (and bins under two cells merge taps); NCHW the general loop; both run the grid-stride loop (more than
    65 536 x 256 output elements)."""
    H, W, C = 38, 63, 1024
    rois = R.roi_cases(B, H, W, K, 31 + K)
    A, G, tol, got = _roi_bwd_check(rois, B, H, W, C, 2, layout, seed=K)
    st = R.merge_path_stats(A, layout == native.LAYOUT_NHWC)
    if layout == native.LAYOUT_NHWC:
        assert st['merge_bins'] == K * PH * PW and st['merging_bins'] > K, st
    else:
        assert st['general_bins'] == K * PH * PW
    assert K * C * PH * PW > 65536 * 256
    if K == 4500 and layout == native.LAYOUT_NHWC:
        # adjoint identity at full size: <F, bwd(G)> = <fwd(F), G>, accumulated in f64 from the device outputs; bound: |F|.bwd bound +
        # |G|.fwd bound (the forward's own f32 sums: C_ROI (m + 4) u A|F| + E|F|)
        F = _randn((B * H * W, C), 77)
        fwd = _rows_nhwc(native.roi_align_fwd(F.view(B, H, W, C), rois.to(DEV), PH, PW, SCALE, 2, native.LAYOUT_NHWC))
        _, tol_f = R.roi_forward_bound(A, F)
        lhs = float((F.double() * got.double()).sum())
        rhs = float((fwd.double() * G.double()).sum())
        bound = float((F.double().abs() * tol).sum() + (G.double().abs() * tol_f).sum())
        assert abs(lhs - rhs) <= bound + 1e-12 * abs(lhs), (lhs, rhs, bound)


@pytest.mark.parametrize('layout_name,layout', LAYOUTS)
@pytest.mark.parametrize('sn', [2, 0])
def test_roi_align_backward_edges(sn, layout_name, layout):
    """The border rules of make_tap / axis_tap and both branches: bins under one cell and of one to two cells, samples on the clamped
    last row / column, in (-1, 0], outside on one axis only; malformed and zero-width RoIs; four frames.  sample_num = 0 mixes
    RoIs whose adaptive grid is 2 x 2 (merge path in NHWC) with 1 x 1, 1 x 2, 2 x 1, 1 x 3 and 3 x 3 (general loop)."""
    B, H, W, C = 4, 38, 63, 96
    rois = torch.cat([R.edge_rois(B, H, W), R.adaptive_rois(B, H, W), R.roi_cases(B, H, W, 60, 41)])
    A, _, _, _ = _roi_bwd_check(rois, B, H, W, C, sn, layout, seed=5 + sn)
    for k in ('y_neg', 'x_neg', 'y_clamped', 'x_clamped', 'y_dead_only', 'x_dead_only', 'live'):
        assert A.stats[k] > 0, (k, A.stats)
    st = R.merge_path_stats(A, layout == native.LAYOUT_NHWC)
    if layout == native.LAYOUT_NHWC:
        assert st['merge_bins'] > 0 and st['merging_bins'] > 0, st
    if sn == 0 or layout == native.LAYOUT_NCHW:
        assert st['general_bins'] > 0, st


@pytest.mark.parametrize('channels_last', [True, False])
def test_roi_align_backward_bf16_maps(channels_last):
    """bf16 maps through ops.roi_align: the gradient is accumulated in f32 and cast once to bf16.  Rounding is monotone, so the cast
    of any f32 value within the bound of A^T G lies between bf16(ref - bound) and bf16(ref + bound); where that bracket is one
    value, the gradient is exactly the reference rounded once."""
    B, H, W, C = 3, 38, 63, 256
    rois = R.roi_cases(B, H, W, 900, 51)
    feat = _randn((B, C, H, W), 52, torch.bfloat16)
    if channels_last:
        feat = feat.contiguous(memory_format=torch.channels_last)
    f = feat.detach().requires_grad_(True)
    out = ops.roi_align(f, rois.to(DEV), PH, SCALE, 2)
    G = _randn((rois.shape[0] * PH * PW, C), 53, torch.bfloat16)
    out.backward(G.view(-1, PH, PW, C).permute(0, 3, 1, 2))
    assert f.grad.dtype == torch.bfloat16
    A = R.roi_align_matrix(rois, B, H, W, PH, PW, SCALE, 2).to(DEV)
    ref, tol = R.roi_backward_bound(A, G)
    got = f.grad.permute(0, 2, 3, 1).reshape(-1, C)
    lo, hi = (ref - tol).float().bfloat16(), (ref + tol).float().bfloat16()
    assert bool(((got.float() >= lo.float()) & (got.float() <= hi.float())).all())
    once = ref.float().bfloat16()
    pinned = lo == hi
    assert float(pinned.double().mean()) > 0.9 and torch.equal(got[pinned], once[pinned])


# ------------------------------------------------------------------------------- hvr_colsum
# (M, N, slices): S = 1 (one row block or many columns), S > 1, S = 256 (capped)
COLSUM = [(1, 1, 1), (1, 1025, 1), (24, 1024, 1), (64, 35, 1), (65, 31, 2), (900, 1024, 15), (4500, 1024, 64), (4500, 1025, 61),
          (2000, 35, 32), (20000, 1, 256), (20000, 31, 256), (17000, 35, 256), (20000, 1025, 61)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('M,N,S', COLSUM)
def test_colsum_against_f64(M, N, S, dtype):
    """hvr_colsum on a column slice of a wider matrix (row stride N + 13) and on a contiguous copy, against the f64 column sums
    within (chain + 1) u sum|x|; the slice count follows colsum_slices and the workspace is needed exactly when S > 1; `out=`
    and a second call are bit-identical (fixed summation order)."""
    assert R.colsum_slices(M, N) == S
    assert native.lib().hvr_colsum_workspace_bytes(M, N) == (0 if S == 1 else S * N * 4)
    scale = (torch.arange(N + 13, device=DEV) % 7 + 1).float()
    wide = (_randn((M, N + 13), M * 7 + N) * scale + 0.25).to(dtype)
    for x in (wide[:, :N], wide[:, :N].contiguous()):
        got = native.colsum(x)
        ref, tol = R.colsum_bound(x)
        err = (got.double() - ref).abs()
        assert bool((err <= tol).all()), 'max err %g, bound %g' % (float(err.max()), float(tol[err.argmax()]))
        out = torch.full((N,), float('nan'), device=DEV)
        assert native.colsum(x, out=out) is out
        assert torch.equal(out, got) and torch.equal(native.colsum(x), got)


def test_colsum_rejects_a_short_workspace_and_split_half():
    M, N = 4500, 1024
    need = native.lib().hvr_colsum_workspace_bytes(M, N)
    x = _randn((M, N), 3)
    db = torch.empty(N, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L, p = native.lib(), native._ptr

    def call(w, nbytes, t=x):
        native._check(L.hvr_colsum(p(t), p(db), M, N, t.stride(0), native._dt(t), p(w), nbytes, native._stream()), 'hvr_colsum')
    with pytest.raises(native.HvrError):
        call(ws, need - 4)
    with pytest.raises(native.HvrError):
        call(None, 0)
    with pytest.raises(native.HvrError):
        call(ws, need, t=torch.zeros((M, N), dtype=native.SPLIT, device=DEV))
    call(ws, need)
    assert torch.equal(db, native.colsum(x))


# ------------------------------------------------------------------------------- weight pack
SENT16 = 0x7FC1          # a NaN pattern in both bf16 and half: never produced by the packs below
ULP_BITS = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def _ties(n, dtype, g):
    """n f32 values placed exactly half-way between two neighbours of dtype (normal and, for half, subnormal ones), both signs."""
    if dtype == torch.float32:
        return torch.randn(n, generator=g)
    mant, emin = ULP_BITS[dtype]
    base = (torch.randn(n, generator=g) * 4).to(dtype).float()
    _, e = torch.frexp(base)
    ulp = torch.pow(2.0, (torch.clamp(e - 1, min=emin) - mant).float())
    t = base + torch.sign(base) * ulp / 2
    if dtype == torch.float16:
        t[: n // 8] = (torch.randint(0, 64, (n // 8,), generator=g).float() + 0.5) * 2.0 ** -24 * torch.sign(torch.randn(n // 8, generator=g))
    return t


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize('shape', [(64, 32, 3, 3), (10, 6, 3, 3), (256, 1024, 1, 1), (7, 3, 7, 7)])
def test_pack_conv_weight_bit_exact(shape, dtype):
    """pack_conv_weight = (w * s) permuted to [Cout][KH][KW][Cin] and rounded once: bit for bit the torch statement, with output
    channels 0 / 1 (scale 1 and 1/2) made of exact rounding ties of the target format (ties go to even)."""
    g = torch.Generator().manual_seed(sum(shape))
    w = torch.randn(shape, generator=g)
    s = torch.rand(shape[0], generator=g) + 0.5
    per = w[0].numel()
    s[0], s[1] = 1.0, 0.5
    w[0] = _ties(per, dtype, g).view(w[0].shape)
    w[1] = 2 * _ties(per, dtype, g).view(w[1].shape)
    want = R.pack_statement(w, s, dtype)
    got = native.pack_conv_weight(w.to(DEV), s.to(DEV), dtype).cpu()
    ib = torch.int16 if dtype != torch.float32 else torch.int32
    assert got.shape == want.shape and torch.equal(got.view(ib), want.view(ib))
    if dtype != torch.float32:   # the ties really are ties: half of them round down, half up (to even)
        tie = w[0].permute(1, 2, 0).reshape(-1)
        assert bool((tie != tie.to(dtype).float()).all())


def _pack_table(shapes, misaligned, dtype, seed):
    """One packed-operand buffer holding every item's output behind a guard band of sentinels; item i's output starts one element
    (2 bytes) past a 16-byte boundary when misaligned[i].  -> (items, ws, ss, buffer, [(offset, n)], firsts)."""
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(s, generator=g) for s in shapes]
    ss = [torch.rand(s[0], generator=g) + 0.5 for s in shapes]
    offs, cur = [], 0
    for w, m in zip(ws, misaligned):
        cur = (cur + 8 + 7) // 8 * 8 + (1 if m else 0)          # >= 8 guard elements, then aligned or 2 bytes off
        offs.append((cur, w.numel()))
        cur += w.numel()
    buf = torch.full((cur + 16,), SENT16, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    wd = [w.to(DEV) for w in ws]
    sd = [s.to(DEV) for s in ss]
    firsts, first, items = [], 0, []
    for (o, n), w, s, shp in zip(offs, wd, sd, shapes):
        firsts.append(first)
        items.append(native.PackItem(w=w.data_ptr(), scale=s.data_ptr(), out=buf.data_ptr() + 2 * o, first=first, Cout=shp[0], Cin=shp[1],
                                     KK=shp[2] * shp[3]))
        first += n
    return items, ws, ss, (wd, sd), buf, offs, firsts


def _many_shapes(n, seed):
    g = torch.Generator().manual_seed(seed)
    cins = [3, 6, 8, 12, 16, 24, 32, 64]
    return [(int(torch.randint(1, 40, (1,), generator=g)), cins[int(torch.randint(0, len(cins), (1,), generator=g))],
             *((3, 3) if bool(torch.rand(1, generator=g) < 0.4) else (1, 1))) for _ in range(n)]


PACK_TABLES = {
    'mixed': ([(64, 32, 3, 3), (5, 3, 3, 3), (16, 6, 1, 1), (9, 12, 3, 3), (7, 16, 1, 1), (64, 64, 1, 1), (3, 8, 3, 3)],
              [False, False, False, False, False, True, False]),
    'one_item': ([(64, 24, 3, 3)], [False]),
    'one_item_misaligned': ([(32, 16, 1, 1)], [True]),
    'hundred': (_many_shapes(100, 9), [i % 17 == 5 for i in range(100)]),
}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('table', sorted(PACK_TABLES))
def test_pack_conv_weights_multi_bit_exact(table, dtype):
    """pack_conv_weights_multi on hand-built tables: Cin % 8 == 0 next to Cin in {3, 6, 12}, item totals that are not multiples of 8
    (groups straddle items), outputs 2 bytes off 16-byte alignment, a one-item table and a hundred-item one (the table search).
    Bit for bit the torch statement; the guard bands around every output keep their sentinels.  Branches, from the kernel's rule:
    the fast eight-wide path and the element-wise one both run, the latter on straddling groups."""
    shapes, mis = PACK_TABLES[table]
    items, ws, ss, keep, buf, offs, firsts = _pack_table(shapes, mis, dtype, len(shapes))
    total = firsts[-1] + offs[-1][1]
    native.pack_conv_weights_multi(native.items_to_device(items, DEV), len(items), total, dtype)
    host = buf.cpu()
    guard = torch.ones(host.numel(), dtype=torch.bool)
    for (o, n), w, s in zip(offs, ws, ss):
        want = R.pack_statement(w, s, dtype).reshape(-1).view(torch.int16)
        assert torch.equal(host[o:o + n], want), (table, o)
        guard[o:o + n] = False
    assert bool((host[guard] == SENT16).all())
    fast, slow, straddle = R.pack_groups([(c, i, kh * kw) for c, i, kh, kw in shapes], firsts,
                                         [(buf.data_ptr() + 2 * o) % 16 for o, _ in offs])
    if table == 'one_item':
        assert fast == (total + 7) // 8 and slow == 0
    elif table == 'one_item_misaligned':
        assert fast == 0 and slow == (total + 7) // 8
    else:
        assert fast > 0 and slow > 0 and straddle > 0, (fast, slow, straddle)


# ------------------------------------------------------------------------------- transpose_multi
def test_transpose_multi_bit_exact_with_padding_and_pitches():
    """transpose_multi: dst[c][r] = src[r][c] for r < R, c < C as 64 x 64 tiles of 16-bit words, zeros in columns R .. dcols - 1 and
    nothing written past dcols.  R and C not multiples of 64 (C % 8 == 0), dcols > R (whole tiles of padding), lds > C, ldd > dcols,
    and per-tap entries reading inside a wider row as train_ops builds them.  first_tile / tiles_c as train_ops sets them."""
    g = torch.Generator().manual_seed(11)
    # (R, C, lds, dcols, ldd, src column offset)
    spec = [(70, 72, 80, 136, 144, 0), (130, 8, 24, 136, 136, 8), (40, 40, 120, 40, 120, 40), (200, 136, 136, 256, 264, 0),
            (1, 64, 64, 64, 72, 0), (64, 200, 200, 72, 80, 0)]
    srcs, dsts, items, tile0 = [], [], [], 0
    guard = 24
    for R_, C_, lds, dcols, ldd, coff in spec:
        assert C_ % 8 == 0 and dcols % 8 == 0 and ldd % 8 == 0 and lds % 8 == 0 and coff % 8 == 0
        src = torch.randint(-32768, 32767, (R_, lds), generator=g, dtype=torch.int16).to(DEV)
        dbuf = torch.full(((C_ + 2) * ldd + guard,), SENT16, dtype=torch.int16, device=DEV)
        tiles_c, tiles_r = (C_ + 63) // 64, (dcols + 63) // 64
        items.append(native.TransposeItem(src=src.data_ptr() + 2 * coff, dst=dbuf.data_ptr() + 2 * ldd, lds=lds, ldd=ldd, R=R_, C=C_,
                                          first_tile=tile0, tiles_c=tiles_c, dcols=dcols))
        tile0 += tiles_r * tiles_c
        srcs.append(src)
        dsts.append(dbuf)
    native.transpose_multi(native.items_to_device(items, DEV), len(items), tile0)
    pad_tiles = 0
    for (R_, C_, lds, dcols, ldd, coff), src, dbuf in zip(spec, srcs, dsts):
        host = dbuf.cpu()
        want = torch.full_like(host, SENT16)
        body = want[ldd:ldd + C_ * ldd].view(C_, ldd)
        body[:, :dcols] = 0
        body[:, :R_] = src.cpu()[:, coff:coff + C_].t()
        assert torch.equal(host, want), (R_, C_, dcols)
        pad_tiles += sum(1 for tr in range((dcols + 63) // 64) if tr * 64 >= R_)
    assert pad_tiles > 0 and any(d > r for r, _, _, d, _, _ in spec)


# ------------------------------------------------------------------------------- weight-gradient unpack
def _unpack_inputs(Cout, Cin, KK, g, plant=True):
    """a [Cout][KK][Cin] product, scale, and the gradient it is added to; channel 0 plants exact double-rounding cases of a * s + d
    (a = 2^-24 (1 + 2^-18) 2^k, s = 1 - 2^-18, d = (1 + 2^-23) 2^k: the exact sum lies just under an f32 midpoint)."""
    a = torch.randn((Cout, KK, Cin), generator=g)
    s = torch.rand(Cout, generator=g) + 0.5
    d = torch.randn((Cout, Cin, KK), generator=g)
    if plant:
        s[0] = 1 - 2.0 ** -18
        k = torch.randint(-8, 8, (KK, Cin), generator=g).float()
        a[0] = 2.0 ** -24 * (1 + 2.0 ** -18) * torch.pow(2.0, k)
        d[0] = ((1 + 2.0 ** -23) * torch.pow(2.0, k)).t()
    return a, s, d


def _unpack_want(a, s, d):
    """(a * s -> [Cout][Cin][KK] in f32, fma(a, s, d) correctly rounded, risky mask, double-rounding-wrong mask, f64-then-f32)."""
    ap = a.permute(0, 2, 1)
    sv = s.view(-1, 1, 1).expand_as(ap)
    exact, risky, wrong = R.fma_f32(ap, sv, d)
    return ap * sv, exact, risky, wrong, (ap.double() * sv.double() + d.double()).float()


def _check_accumulated(got, exact, risky, wrong, twice):
    """bit for bit the correctly rounded fma; against the f64 sum rounded to f32 once more: equal except where double rounding can
    apply, and there within one ulp.  -> the number of elements that hit it."""
    assert torch.equal(got.view(torch.int32), exact.view(torch.int32))
    assert torch.equal(got[~risky], twice[~risky])
    ulp = (torch.nextafter(twice, torch.full_like(twice, float('inf'))) - twice).abs()
    assert bool(((got[risky] - twice[risky]).abs() <= ulp[risky]).all())
    return int(wrong.sum())


@pytest.mark.parametrize('shape', [(64, 32, 3, 3), (10, 6, 3, 3), (256, 1024, 1, 1), (5, 3, 7, 7)])
def test_unpack_conv_wgrad_against_f64(shape):
    """unpack_conv_wgrad: written, bit for bit f32 a * s; accumulated, the fma a * s + d rounded once -- the f64 statement rounded to
    f32 differs only at the planted double-rounding elements, which are all hit (reported in the assertion)."""
    Cout, Cin, KH, KW = shape
    KK = KH * KW
    g = torch.Generator().manual_seed(Cout + Cin)
    a, s, d = _unpack_inputs(Cout, Cin, KK, g)
    prod, exact, risky, wrong, twice = _unpack_want(a, s, d)
    got = native.unpack_conv_wgrad(a.reshape(Cout, -1).to(DEV), s.to(DEV), shape).cpu()
    assert torch.equal(got.view(Cout, Cin, KK).view(torch.int32), prod.view(torch.int32))
    acc = d.view(shape).to(DEV)
    native.unpack_conv_wgrad(a.reshape(Cout, -1).to(DEV), s.to(DEV), shape, accumulate_into=acc)
    hits = _check_accumulated(acc.cpu().view(Cout, Cin, KK), exact, risky, wrong, twice)
    assert hits == KK * Cin, 'double rounding cases: %d of %d planted' % (hits, KK * Cin)


@pytest.mark.parametrize('accumulate', [False, True])
def test_unpack_conv_wgrads_multi_elementwise_fallback(accumulate):
    """unpack_conv_wgrads_multi with item totals that are not multiples of 4 and outputs 4 bytes past a 16-byte boundary inside one
    larger buffer: groups straddle items or are misaligned and take the element-wise path, the others the four-wide path (both
    asserted from the kernel's rule).  Written: bit for bit a * s; accumulated: the correctly rounded fma.  Guards keep their bits."""
    shapes = [(5, 3, 3, 3), (7, 6, 1, 1), (3, 5, 3, 3), (16, 8, 1, 1), (4, 10, 3, 3), (9, 7, 1, 1)]
    g = torch.Generator().manual_seed(17)
    ins = [_unpack_inputs(c, i, kh * kw, g, plant=(n == 0)) for n, (c, i, kh, kw) in enumerate(shapes)]
    offs, cur = [], 0
    for n, (c, i, kh, kw) in enumerate(shapes):
        cur = (cur + 4 + 3) // 4 * 4 + (1 if n % 2 == 0 else 0)       # even items 4 bytes off 16-byte alignment
        offs.append(cur)
        cur += c * i * kh * kw
    SENT = -12345.5
    out = torch.full((cur + 8,), SENT, device=DEV)
    for o, (a, s, d) in zip(offs, ins):
        out[o:o + d.numel()] = d.reshape(-1).to(DEV)
    dws = [a.reshape(-1).to(DEV) for a, _, _ in ins]
    sds = [s.to(DEV) for _, s, _ in ins]
    items, firsts, first = [], [], 0
    for (c, i, kh, kw), o, dw, sd in zip(shapes, offs, dws, sds):
        firsts.append(first)
        items.append(native.PackItem(w=out.data_ptr() + 4 * o, scale=sd.data_ptr(), out=dw.data_ptr(), first=first, Cout=c, Cin=i, KK=kh * kw))
        first += c * i * kh * kw
    native.unpack_conv_wgrads_multi(native.items_to_device(items, DEV), len(items), first, accumulate=accumulate)
    host = out.cpu()
    guard = torch.ones(host.numel(), dtype=torch.bool)
    hits = 0
    for (c, i, kh, kw), o, (a, s, d) in zip(shapes, offs, ins):
        n = c * i * kh * kw
        guard[o:o + n] = False
        prod, exact, risky, wrong, twice = _unpack_want(a, s, d)
        got = host[o:o + n].view(c, i, kh * kw)
        if accumulate:
            hits += _check_accumulated(got, exact, risky, wrong, twice)
        else:
            assert torch.equal(got.view(torch.int32), prod.view(torch.int32))
    assert bool((host[guard] == SENT).all())
    vec, slow, straddle = R.unpack_groups([(c, i, kh * kw) for c, i, kh, kw in shapes], firsts, [(out.data_ptr() + 4 * o) % 16 for o in offs])
    assert vec > 0 and slow > 0 and straddle > 0, (vec, slow, straddle)
    if accumulate:
        assert hits == shapes[0][1] * shapes[0][2] * shapes[0][3], hits
