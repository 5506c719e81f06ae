"""Plain float64 statement of the grouped 3x3 convolution (hvr_conv3x3_grouped, include/hvr_hip.h; native.conv3x3_grouped on either
route), written independently of the HIP code and of torch's conv dispatch, with the bounds that tests/test_gconv_refs.py (CPU) and
tests/test_gconv_gpu.py (GPU) hold the kernels to.

The rule: x [B, H, W, C], w [C, 3, 3, Cg] with Cg = C / groups; output channel oc belongs to group oc // Cg and reads the input
channels [g Cg, (g + 1) Cg) of that group; pad == dil; bias f32 [C]; optional ReLU.  The statement is a direct sum: the patch matrix by
index arithmetic (forward_kernel_refs._patches), each output channel's 9 Cg inputs gathered by its group index, one f64 contraction.

Error model and brackets: forward_kernel_refs (mfma_bound, stored_bracket) with the chain 9 Cg + E_EPI.  Why 9 Cg although the grouped
kernel runs K = 160 (Cg <= 16: five K-steps of two taps x 16 channels) or 288 (Cg = 32) products per output and the dense route
K = 9 C: every product the rule does not contain has an exact zero weight (the block-diagonal padding inside a 16-channel tile, the
tenth tap, the zeros of the dense weight), so it is an exact 0 (finite activations), and adding an exact 0 to a partial sum changes
nothing under any rounding rule, truncation included.  A partial sum made only of such products is 0 as well.  So in any summation
order -- K-steps, K slices, wave partials -- the additions that can round are those that join non-zero terms, at most 9 Cg of them
behind one accumulator (split half: 3 x 9 Cg, chain() counts them); the epilogue adds E_EPI operations (+ bias; alpha and beta on the
dense route in split half).  No bound contains a value measured on a device.

`mistake=` states a plausible kernel mistake exactly (MISTAKES); the CPU tests show each outside the bracket on real-statistics operands
and unequal on the exact family.
"""
import torch

from tests import forward_kernel_refs as F

CGS = (4, 8, 16, 32)
MISTAKES = ('group_offset', 'dense', 'group_interleaved', 'tap_border', 'dil1', 'stride_phase', 'bias_other_group')
# (B, H, W, C, Cg, stride, dil): the geometries of tests/test_gconv_gpu.py
SMALL = [(2, 5, 7, 64, cg, s, d) for cg in CGS for s in (1, 2) for d in (1, 2)]
ODD = [(3, 19, 23, 128, 4, 1, 1)]                      # 1 311 rows: no multiple of any tile; two 32-channel blocks per pixel-tile pair
RES5 = [(1, 6, 5, 1024, 32, 1, 2), (1, 4, 4, 2048, 32, 1, 1)]
GEOMETRIES = SMALL + ODD + RES5


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def gconv_statement(x, w, bias=None, relu=False, stride=1, dil=1, mistake=None):
    """x [B, H, W, C], w [C, 3, 3, Cg], bias [C] -> (ref, mag, sum|x||w|), f64 [B, OH, OW, C].
    Mistakes: 'group_offset' every group reads the NEXT group's input channels; 'dense' the group index is ignored (every output reads the
    first Cg input channels); 'group_interleaved' the group of oc taken as oc % groups; 'tap_border' the centre tap masked at the right /
    bottom border; 'dil1' the last tap read at dilation 1; 'stride_phase' stride-2 outputs taken at the odd pixels; 'bias_other_group' the
    bias of the channel Cg further on."""
    assert mistake is None or mistake in MISTAKES, mistake
    x, w = x.double(), w.double()
    B, H, W, C = x.shape
    Cg = w.shape[3]
    G = C // Cg
    assert tuple(w.shape) == (C, 3, 3, Cg) and G * Cg == C
    s = stride
    if mistake == 'stride_phase' and stride == 2:
        s = 1
    cols, OH, OW = F._patches(x, 3, 3, s, dil, dil, mistake if mistake in ('tap_border', 'dil1') else None)
    if mistake == 'stride_phase' and stride == 2:
        full = cols.view(B, OH, OW, -1)
        OH2, OW2 = out_hw(H, W, 2)
        iy = (torch.arange(OH2, device=x.device) * 2 + 1).clamp(max=OH - 1)
        ix = (torch.arange(OW2, device=x.device) * 2 + 1).clamp(max=OW - 1)
        cols, OH, OW = full[:, iy][:, :, ix].reshape(B * OH2 * OW2, -1), OH2, OW2
    M = cols.shape[0]
    cols = cols.view(M, 9, G, Cg)
    oc = torch.arange(C, device=x.device)
    grp = oc // Cg
    if mistake == 'group_offset':
        grp = (grp + 1) % G
    elif mistake == 'dense':
        grp = torch.zeros_like(grp)
    elif mistake == 'group_interleaved':
        grp = oc % G
    wk = w.reshape(C, 9, Cg)
    acc = torch.empty((M, C), dtype=torch.float64, device=x.device)
    absxw = torch.empty_like(acc)
    step = max(1, (1 << (26 if x.is_cuda else 22)) // max(1, M * 9 * Cg))   # output channels per round: the gathered operand stays below 32 MB (device: 512 MB)
    for c0 in range(0, C, step):
        sel = cols[:, :, grp[c0:c0 + step], :]                    # [M, 9, n, Cg]: each output channel's own inputs
        acc[:, c0:c0 + step] = torch.einsum('mtnc,ntc->mn', sel, wk[c0:c0 + step])
        absxw[:, c0:c0 + step] = torch.einsum('mtnc,ntc->mn', sel.abs(), wk[c0:c0 + step].abs())
    b = None if bias is None else bias.double()
    if b is not None and mistake == 'bias_other_group':
        b = b[(oc + Cg) % C]
    ref, mag = F._epilogue(acc, absxw, b, None, relu, None)
    shp = (B, OH, OW, C)
    return ref.view(shp), mag.view(shp), absxw.view(shp)


def gconv_bound(mag, absxw, Cg, mode):
    """Bound on the f32 value before the store: chain 9 Cg + E_EPI (module docstring)."""
    return F.mfma_bound(mag, absxw, 9 * Cg, mode)


def gconv_bracket(ref, mag, absxw, Cg, mode):
    return F.stored_bracket(ref, gconv_bound(mag, absxw, Cg, mode), mode)


def by_slices(x, w, bias=None, relu=False, stride=1, dil=1):
    """The same rule a second way: each group a forward_kernel_refs.conv_statement on its channel slices (the CPU test holds the two equal)."""
    C, Cg = w.shape[0], w.shape[3]
    outs = [F.conv_statement(x[..., g * Cg:(g + 1) * Cg], w[g * Cg:(g + 1) * Cg], None if bias is None else bias[g * Cg:(g + 1) * Cg],
                             None, relu, stride, dil, dil)[0] for g in range(C // Cg)]
    return torch.cat(outs, 3)


# ------------------------------------------------------------------------------------------------ operand families
def real_case(geom, mode, seed, device='cpu'):
    """Real-statistics operands (forward_kernel_refs.real_operands: activations behind a ReLU, weights N(0, 1 / sqrt(9 Cg))) and a bias of
    the size a folded BatchNorm shift has.  -> dict(x, w, bias) of f64 true values as `mode` stores them."""
    B, H, W, C, Cg, s, d = geom
    x, w = F.real_operands((B, H, W, C), (C, 3, 3, Cg), mode, seed, device=device)
    g = torch.Generator().manual_seed(seed + 7)
    bias = (torch.randn((C,), generator=g) * 0.3).double().to(device)
    return dict(x=x, w=w, bias=bias)


def exact_families(mode):
    return ('plain', 'lo_act', 'lo_weight') if mode == 'f16x2' else ('plain',)


def exact_gconv_case(geom, mode, seed, family='plain', device='cpu'):
    """Exact-sum operands (forward_kernel_refs.exact_case with K = 9 Cg): every partial sum is an f32 number in any order, so either route
    must return round-to-nearest of the statement, and the two routes each other's bits.  -> dict(x, w, bias, q)"""
    B, H, W, C, Cg, s, d = geom
    c = F.exact_case((B, H, W, C), (C, 3, 3, Cg), mode, seed, family=family, device=device)
    return dict(x=c['a'], w=c['w'], bias=c['bias'], q=c['q'])


# ------------------------------------------------------------------------------------------------ a Bottleneck as a chain of statements
def block_chain(x, p, stride, dil, style='pytorch', downsample=False):
    """A grouped Bottleneck in f64 over FOLDED weights p = dict(c1=(w [width,1,1,Cin], b), c2=(w [width,3,3,Cg], b), c3=(w [4 planes,1,1,width], b),
    ds=(w, b) when `downsample`): conv1 + ReLU, the grouped 3x3 + ReLU, conv3 + shortcut + ReLU.  x [B, H, W, Cin] -> [B, OH, OW, 4 planes]."""
    s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
    h = F.conv_statement(x, p['c1'][0], p['c1'][1], None, True, s1, 0, 1)[0]
    h = gconv_statement(h, p['c2'][0], p['c2'][1], True, s2, dil)[0]
    idt = F.conv_statement(x, p['ds'][0], p['ds'][1], None, False, stride, 0, 1)[0] if downsample else x.double()
    return F.conv_statement(h, p['c3'][0], p['c3'][1], idt, True, 1, 0, 1)[0]
