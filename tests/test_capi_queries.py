"""Every shape-only query of the C ABI against a recorded table (-m "not gpu": the queries touch no device).

The kernel a product takes (hvr_conv2d_path, the four hvr_bottleneck_*_supported), the few-row / split-K scratch sizes and every
device workspace size are functions of shapes alone.  Captured graphs, the per-stream workspace cache and ResNet.stage_route's
bit-identity claims depend on them, so a change that restates a workspace layout or a kernel route must leave all of them where they
are.  `enumerate_queries` evaluates them over a fixed grid -- the window's layer shapes at 1 / 4 / 15 / 60 frames, the smallest shapes
on either side of every threshold the C side names, zero and negative arguments, a few descriptors that are rejected outright (the
negative code is the answer) -- and the test compares the answers with tests/golden/capi_queries.json.

The table is recorded from a build of the commit BEFORE the change under test, never from the code under test:

    python tests/test_capi_queries.py --record --lib <that build's libhvr_hip.so>

The library reads its HVR_* environment switches once per process; the table holds the answers with none of them set, and the test
refuses to run with one of those the queries read (HVR_CONV_SPLITK, HVR_EXPAND, HVR_CONV3, HVR_BIGTILE) in the environment.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, ROOT)

from hvrnet_amd import native  # noqa: E402
from hvrnet_amd.native import (CloseSampledDesc, ConvDesc, GemmDesc, TailDesc, TailNextDesc, TailNextLiveDesc)  # noqa: E402

TABLE = os.path.join(ROOT, 'tests', 'golden', 'capi_queries.json')
SWITCHES = ('HVR_CONV_SPLITK', 'HVR_EXPAND', 'HVR_CONV3', 'HVR_BIGTILE')

PH = 1 << 20                      # placeholder address, 128-byte aligned (native._PH)
DTYPES = (0, 1, 2, 3)             # HVR_F32, HVR_BF16, HVR_F16, HVR_F16S
HINTS = (0, 13, 16, 17, 18)       # library's choice, kExpandHint, kBigHint, kBigForce, kTwoLevelHint
FLAGS = tuple(itertools.product((1, 0), (1, 0), (0, 1)))   # (bias, resid, out_f32)
FRAMES = (1, 4, 15, 60)


def _load(path):
    handle = ctypes.CDLL(path)
    for name, (res, args) in native.SYMBOLS.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


def _key(*v):
    return ' '.join(str(x) for x in v)


# ---- the grids ----
def _conv_layers():
    """(H, W, Cin, Cout, k, stride, pad, dil, has_residual) of the window's backbone, res5 head and RPN convs at 608 x 1008."""
    out = []
    for (h, w, cin_prev, planes, s, d) in ((152, 252, 64, 64, 1, 1), (152, 252, 256, 128, 2, 1), (76, 126, 512, 256, 2, 1), (38, 63, 1024, 512, 1, 2)):
        oh, ow = (h - 1) // s + 1, (w - 1) // s + 1
        out += [(h, w, cin_prev, planes, 1, 1, 0, 1, 0),                 # first block's reducing 1x1
                (h, w, planes, planes, 3, s, d, d, 0),                   # its 3x3 (strided in stages 2 and 3, dilated in res5)
                (oh, ow, planes, planes, 3, 1, d, d, 0),                 # the other blocks' 3x3
                (oh, ow, planes, 4 * planes, 1, 1, 0, 1, 1),             # expanding 1x1 + residual
                (oh, ow, 4 * planes, planes, 1, 1, 0, 1, 0),             # the other blocks' reducing 1x1
                (h, w, cin_prev, 4 * planes, 1, s, 0, 1, 0)]             # projection shortcut
    out.append((38, 63, 1024, 512, 3, 1, 1, 1, 0))                       # the RPN's 3x3
    return out


# (B, H, W, Cin, Cout, k, stride, pad, dil): the smallest shapes on either side of the thresholds capi.hip and the *_supported predicates name
CONV_EDGES = [
    (1, 1, 127, 64, 256, 1, 1, 0, 1), (1, 1, 128, 64, 256, 1, 1, 0, 1),           # 128 pixels: one row panel
    (1, 31, 33, 64, 64, 3, 1, 1, 1), (1, 32, 32, 64, 64, 3, 1, 1, 1),             # four 16 x 16 tiles of the 64-channel 3x3
    (1, 64, 80, 512, 256, 1, 1, 0, 1), (1, 9, 569, 512, 256, 1, 1, 0, 1),         # 160 / 164 tiles of 128 x 64 (the few-row forms)
    (1, 64, 80, 448, 256, 1, 1, 0, 1),                                            # 7 K-steps (they want 8)
    (1, 19, 32, 256, 256, 3, 1, 1, 1), (1, 19, 32, 1024, 256, 1, 1, 0, 1),        # few rows, long K: K-parallel waves / K slices
    (15, 38, 63, 128, 256, 1, 1, 0, 1), (15, 38, 63, 128, 192, 1, 1, 0, 1),       # N >= 2 K
    (15, 38, 63, 256, 512, 1, 1, 0, 1), (15, 38, 63, 256, 448, 1, 1, 0, 1),
    (1, 256, 256, 256, 1024, 1, 1, 0, 1), (1, 255, 257, 256, 1024, 1, 1, 0, 1),   # K = 256 with M = 65 536 / 65 535
    (1, 85, 288, 1024, 512, 1, 1, 0, 1), (1, 84, 288, 1024, 512, 1, 1, 0, 1),     # 170 / 168 big tiles (alone on the chip)
    (1, 96, 288, 1024, 256, 1, 1, 0, 1), (1, 95, 288, 1024, 256, 1, 1, 0, 1),     # 96 / 95 big tiles (a throughput caller)
    (1, 38, 63, 288, 256, 1, 1, 0, 1),                                            # 9 K-steps of 32: no two-level blocks; not a bf16 K-step multiple
    # rejected outright
    (1, 38, 63, 100, 256, 1, 1, 0, 1),                                            # Cin is no K-step multiple
    (1, 1, 1, 64, 64, 3, 1, 0, 1),                                                # empty output
    (4096, 256, 256, 64, 64, 1, 1, 0, 1),                                         # an input of 2 GiB and more
    (0, 38, 63, 64, 256, 1, 1, 0, 1), (-1, 38, 63, 64, 256, 1, 1, 0, 1),
]

# (M, N, K)
GEMM_SHAPES = [
    (4500, 1024, 12544), (300, 1024, 12544), (4500, 1024, 1024), (300, 1024, 1024), (300, 124, 1024), (4500, 1056, 1024),
    (5120, 256, 512), (5121, 256, 512), (5120, 256, 448), (24480, 512, 1024), (24192, 512, 1024), (27648, 256, 1024), (27360, 256, 1024),
    (4608, 1024, 8192), (4609, 1024, 8192), (3456, 1024, 8192), (3457, 1024, 8192), (4608, 1024, 8128), (64, 64, 64),
    (300, 1024, 100), (300, 6, 1024), (0, 1024, 1024), (300, 1024, -64),
]
GEMM_FLAGS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1))


def _conv_desc(B, H, W, Cin, Cout, k, stride, pad, dil, dtype, hint, bias, resid, out_f32, zero=True):
    return ConvDesc(x=PH, w=PH, y=PH, B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=k, KW=k, stride=stride, pad=pad, dil=dil,
                    bias=PH if bias else None, resid=PH if resid else None, relu=1, out_f32=out_f32, dtype=dtype, staging=1, tile_hint=hint,
                    zero=PH if zero else None)


def _conv_answers(L, d):
    return [int(L.hvr_conv2d_path(ctypes.byref(d))), int(L.hvr_conv2d_splitk_workspace_bytes(ctypes.byref(d)))]


def _convs(L):
    """shape -> [path, split-K bytes] per (dtype, hint[, (bias, resid, out_f32)]) in the order of DTYPES x HINTS [x FLAGS]"""
    out = {}
    for frames in FRAMES:
        for (h, w, cin, cout, k, s, p, dl, res) in _conv_layers():
            row = []
            for dt, hint in itertools.product(DTYPES, HINTS):
                row += _conv_answers(L, _conv_desc(frames, h, w, cin, cout, k, s, p, dl, dt, hint, 1, res, 0))
            out[_key('layer', frames, h, w, cin, cout, k, s, p, dl, res)] = row
    for shape in CONV_EDGES:
        row = []
        for dt, hint, (bias, resid, f32) in itertools.product(DTYPES, HINTS, FLAGS):
            row += _conv_answers(L, _conv_desc(*shape, dt, hint, bias, resid, f32))
        out[_key('edge', *shape)] = row
    # rejected outright: no zero page for a conv that pads, a dtype that is none, a null descriptor
    out['no-zero-page'] = _conv_answers(L, _conv_desc(1, 38, 63, 64, 64, 3, 1, 1, 1, 1, 0, 1, 0, 0, zero=False))
    out['bad-dtype'] = _conv_answers(L, _conv_desc(1, 38, 63, 64, 64, 1, 1, 0, 1, 7, 0, 1, 0, 0))
    out['null'] = [int(L.hvr_conv2d_path(None)), int(L.hvr_conv2d_splitk_workspace_bytes(None))]
    return out


def _gemms(L):
    """shape -> few-row bytes per (dtype, hint, (bias, resid, out_f32)); split-K bytes per dtype / (dtype, count)"""
    out = {}
    for (M, N, K) in GEMM_SHAPES:
        row = []
        for dt, hint, (bias, resid, f32) in itertools.product(DTYPES, HINTS + (14, 15), GEMM_FLAGS):
            d = GemmDesc(A=PH, B=PH, C=PH, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=PH if bias else None, resid=PH if resid else None, ldr=N,
                         relu=1, out_f32=f32, dtype=dt, staging=1, tile_hint=hint)
            row.append(int(L.hvr_gemm_fewrow_workspace_bytes(ctypes.byref(d))))
        out[_key('fewrow', M, N, K)] = row
    out['fewrow null'] = [int(L.hvr_gemm_fewrow_workspace_bytes(None))]
    for M, N, K in itertools.product((64, 256, 1792, 0), (576, 1664, 1792, 2304), (1984, 2048, 143616, -64)):
        out[_key('splitk', M, N, K)] = [int(L.hvr_gemm_splitk_workspace_bytes(M, N, K, dt)) for dt in DTYPES + (7,)] + \
            [int(L.hvr_gemm_splitk_batched_workspace_bytes(M, N, K, dt, c)) for dt in DTYPES + (7,) for c in (0, 1, 3, 8)]
    return out


def _stages(frames):
    """(B, OH, OW, C1, Cout, Cn, (H2, W2, C2), stride2) of each stage's first (projection) block, Cn the next block's width"""
    return [(frames, 152, 252, 64, 256, 64, (152, 252, 64), 1), (frames, 76, 126, 128, 512, 128, (152, 252, 256), 2),
            (frames, 38, 63, 256, 1024, 256, (76, 126, 512), 2), (frames, 38, 63, 512, 2048, 512, (38, 63, 1024), 1)]


def _tail(dt, B, OH, OW, C1, Cout, x_hwc, stride2, relu=1):
    H2, W2, C2 = x_hwc if x_hwc is not None else (OH, OW, 0)
    return TailDesc(h=PH, x=PH if x_hwc is not None else None, w=PH, y=PH, B=B, OH=OH, OW=OW, C1=C1, H2=H2, W2=W2, C2=C2,
                    stride2=stride2 if x_hwc is not None else 1, Cout=Cout, bias=PH, relu=relu, dtype=dt)


def _tail_next(dt, B, OH, OW, C1, Cout, Cn, x_hwc, stride2, relu=1):
    return TailNextDesc(tail=_tail(dt, B, OH, OW, C1, Cout, x_hwc, stride2, relu), resid=PH if x_hwc is None else None, wn=PH, bias_n=PH, hn=PH,
                        Cn=Cn, alpha=1.0, beta=1.0)


def _fused(L):
    """the four hvr_bottleneck_*_supported, per dtype"""
    out = {}
    small = [(1, 8, 15, 64, 256, 64, (8, 15, 64), 1), (1, 8, 16, 64, 256, 64, (8, 16, 64), 1), (1, 256, 256, 256, 1024, 256, (512, 512, 512), 2),
             (1, 255, 257, 256, 1024, 256, (510, 514, 512), 2), (1, 16, 16, 64, 256, 128, (16, 16, 64), 1), (1, 16, 16, 128, 512, 64, (32, 32, 256), 2),
             (1, 16, 16, 96, 256, 64, (16, 16, 32), 1), (1, 16, 16, 64, 320, 64, (16, 16, 64), 1)]
    for f in FRAMES + (0,):
        for (B, OH, OW, C1, Cout, Cn, x_hwc, s2) in (_stages(f) + (small if f == 1 else [])):
            k = _key(B, OH, OW, C1, Cout, Cn, *x_hwc, s2)
            out['tail ' + k] = [int(L.hvr_bottleneck_tail_supported(ctypes.byref(_tail(dt, B, OH, OW, C1, Cout, x_hwc, s2)))) for dt in DTYPES]
            out['next-proj ' + k] = [int(L.hvr_bottleneck_tail_next_supported(ctypes.byref(_tail_next(dt, B, OH, OW, C1, Cout, Cn, x_hwc, s2))))
                                     for dt in DTYPES]
            out['next-ident ' + k] = [int(L.hvr_bottleneck_tail_next_supported(ctypes.byref(_tail_next(dt, B, OH, OW, C1, Cout, Cn, None, 1))))
                                      for dt in DTYPES]
            out['live ' + k] = [int(L.hvr_bottleneck_tail_next_live_supported(ctypes.byref(
                TailNextLiveDesc(next=_tail_next(dt, B, OH, OW, C1, Cout, Cn, None, 1), live_stride=ls)))) for dt in DTYPES for ls in (2, 1, 0)]
            # the stage's last block closed on the pixels a stride-2 consumer reads, and the same product at full resolution (stride 1)
            LH, LW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
            out['sampled ' + k] = [int(L.hvr_bottleneck_close_sampled_supported(ctypes.byref(
                CloseSampledDesc(h=PH, w=PH, resid=PH, y=PH, B=B, OH=oh, OW=ow, C1=C1, Cout=Cout, RH=rh, RW=rw, rstride=rs, bias=PH, relu=1, dtype=dt,
                                 alpha=1.0, beta=1.0)))) for dt in DTYPES for (oh, ow, rh, rw, rs) in ((LH, LW, OH, OW, 2), (OH, OW, OH, OW, 1), (OH, OW, OH, OW, 2))]
    out['sampled N<2K'] = [int(L.hvr_bottleneck_close_sampled_supported(ctypes.byref(
        CloseSampledDesc(h=PH, w=PH, resid=PH, y=PH, B=4, OH=19, OW=32, C1=256, Cout=cout, RH=38, RW=63, rstride=2, bias=PH, relu=1, dtype=dt))))
        for dt in DTYPES for cout in (512, 448, 256)]
    # rejected outright: the next block reads the activated output; the live form is the identity form; null descriptors
    out['next no-relu'] = [int(L.hvr_bottleneck_tail_next_supported(ctypes.byref(_tail_next(1, 4, 152, 252, 64, 256, 64, None, 1, relu=0))))]
    out['live projection'] = [int(L.hvr_bottleneck_tail_next_live_supported(ctypes.byref(
        TailNextLiveDesc(next=_tail_next(1, 4, 152, 252, 64, 256, 64, (152, 252, 64), 1), live_stride=2))))]
    out['null'] = [int(L.hvr_bottleneck_tail_supported(None)), int(L.hvr_bottleneck_tail_next_supported(None)),
                   int(L.hvr_bottleneck_tail_next_live_supported(None)), int(L.hvr_bottleneck_close_sampled_supported(None))]
    return out


def _workspaces(L):
    out = {}
    # relation: 96 output tiles (Mq = 1 408 / 1 409 at D = 1024) and 8 key blocks (Mk = 896 / 897) on both sides
    for Mq, Mk, D in itertools.product((300, 1023, 1024, 1408, 1409, 4500, 1, 0, -1), (4500, 896, 897, 16384, 16385, 1, 0, -1), (1024, 1020, 64, 0)):
        out[_key('relation', Mq, Mk, D)] = [int(L.hvr_relation_workspace_bytes(Mq, Mk, D, dt)) for dt in DTYPES] + \
            [int(L.hvr_relation_grouped_workspace_bytes(g, Mq, Mk, D, dt)) for dt in DTYPES for g in (1, 4, 0, -1)] + \
            [int(L.hvr_relation_probs_workspace_bytes(Mq, Mk))]
    out['nms'] = [int(L.hvr_nms_workspace_bytes(n)) for n in (0, 1, 63, 64, 65, 300, 2000, 6000, 8192, 8193, -1)]
    for T, (H, W, A, pre) in itertools.product((1, 4, 5, 15, 60, 0, -1), ((38, 63, 12, 6000), (38, 63, 12, 0), (38, 63, 12, 8192), (38, 63, 12, 8193), (8, 8, 3, 6000),
                                                                          (1, 8192, 1, 0), (1, 8193, 1, 0), (64, 4, 32, 0), (0, 63, 12, 6000), (38, 63, 0, 6000), (38, 63, 12, -1))):
        out[_key('rpn', T, H, W, A, pre)] = [int(L.hvr_rpn_workspace_bytes(T, H, W, A, pre))]
    for T, (H, W, pre) in itertools.product((1, 4, 15, 60, 0, -1), ((38, 63, 2000), (38, 63, 0), (64, 128, 0), (64, 128, 8192), (1, 8193, 0), (1, 8193, 2000), (0, 63, 0), (38, -1, 0), (1, 1, -1))):
        out[_key('ga_rpn', T, H, W, pre)] = [int(L.hvr_ga_rpn_workspace_bytes(T, H, W, pre))]
    # the candidate-list cap of the merge kernels: (ncls - 1) R <= 16 384
    ncls = (2, 31, 33, 34, 55, 56, 129, 130, 1, 0, -1)
    for R in (1, 300, 512, 513, 0, -1):
        out[_key('multiclass', R)] = [int(L.hvr_multiclass_nms_workspace_bytes(R, c)) for c in ncls] + \
            [int(L.hvr_multiclass_soft_nms_workspace_bytes(P, R, c)) for P in (1, 4, 64, 0, -1) for c in ncls]
        out[_key('seq', R)] = [int(L.hvr_seq_nms_workspace_bytes(F, R, c)) for F in (1, 15, 65535, 0, -1) for c in ncls] + \
            [int(L.hvr_seq_nms_batched_workspace_bytes(P, F, R, c, tubes)) for P in (1, 4, 65535, 0, -1) for F in (4, 60, 65535, 0) for c in ncls for tubes in (0, 1, 2)]
    out['soft_nms'] = [int(L.hvr_soft_nms_workspace_bytes(n)) for n in (0, 1, 512, 513, -1)]
    return out


def enumerate_queries(L):
    """section -> {shape: [answers]} over the fixed grid, from library handle L"""
    return {'conv': _convs(L), 'gemm': _gemms(L), 'fused': _fused(L), 'workspace': _workspaces(L)}


def test_shape_only_queries_answer_as_recorded():
    """Run with none of the HVR_* switches set (the library reads them once per process and the table holds the defaults' answers)."""
    set_ = [s for s in SWITCHES if s in os.environ]
    assert not set_, 'the recorded table holds the answers without %s' % ', '.join(set_)
    if not os.path.exists(native.LIB_PATH):
        native.build()
    got = enumerate_queries(native.lib())
    with open(TABLE) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    n, bad = 0, []
    for sec in sorted(want):
        assert sorted(got[sec]) == sorted(want[sec]), 'the grid of section %r is not the recorded one' % sec
        for k, w in want[sec].items():
            g = got[sec][k]
            assert len(g) == len(w), (sec, k)
            n += len(w)
            bad += [(sec, k, i, g[i], w[i]) for i in range(len(w)) if g[i] != w[i]]
    assert n >= 3000, n
    assert not bad, '%d of %d answers moved; (section, shape, index, now, recorded): %r' % (len(bad), n, bad[:20])


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--record', action='store_true', help='write the table')
    ap.add_argument('--lib', required=True, help="libhvr_hip.so of a build of the commit before the change under test")
    ap.add_argument('--out', default=TABLE)
    a = ap.parse_args()
    assert a.record, 'nothing to do without --record'
    assert not [s for s in SWITCHES if s in os.environ], 'record with none of %s set' % ', '.join(SWITCHES)
    table = enumerate_queries(_load(a.lib))
    with open(a.out, 'w') as f:
        json.dump(table, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print('%d answers in %d rows -> %s (%d bytes)' % (sum(len(v) for s in table.values() for v in s.values()), sum(len(s) for s in table.values()),
                                                     a.out, os.path.getsize(a.out)))
