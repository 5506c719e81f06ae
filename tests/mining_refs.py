"""Plain float64 / exact-integer statements of the selection kernels and the triplet term of the training step (targets.hip),
written independently of the HIP code, with the bounds that tests/test_mining_refs.py (CPU) and tests/test_mining_kernels_gpu.py
(GPU) hold the kernels to:

  sample_kernel (hvr_sample_pos_neg), mining_argreduce_kernel (hvr_mining_argreduce),
  triplet_dist_kernel + triplet_grad_kernel (hvr_triplet_margin).

The sampler and the mining are pure selections: their statements return indices, compared for equality.  The triplet statement
carries every quantity as a readout_refs.Val (value, bound on |f32 result - value|), with the constants of train_loss_refs
(U, SECOND, TINY, SQRTF_ULP, DIV_ULP, ULP; f32v for scalars the kernel receives as `float`).  A bound never contains a value
measured on the device.  Every statement takes a `mistake`: a plausible kernel mistake applied to the statement, which the CPU
tests show to be caught on the case named for it (MISTAKE_CASE_*).
"""
import math

import torch

from tests import train_loss_refs as L
from tests.readout_refs import Val, ratio  # noqa: F401  (ratio: re-exported for the two test files)

U, SECOND, TINY, ULP = L.U, L.SECOND, L.TINY, L.ULP
f32v = L.f32v


# ================================================================================================ sampler
def _smallest(idx, keys, expected, mistake):
    """The `expected` members of idx (ascending) with the numerically smallest keys, ties to the lower index -> ascending indices."""
    if expected <= 0:
        return idx[:0]
    if idx.numel() <= expected:
        return idx
    k = keys[idx].double() + 0.0                                # -0.0 + 0.0 = +0.0: signed zeros tie
    if mistake == 'signed_zero_ordered':                        # -0.0 strictly below +0.0 (the sign bit ranked)
        k = torch.where((keys[idx] == 0) & torch.signbit(keys[idx]), torch.full_like(k, -5e-324), k)
    src = idx.flip(0) if mistake == 'tie_highest_index' else idx
    k = k.flip(0) if mistake == 'tie_highest_index' else k
    order = torch.sort(k, stable=True).indices                  # stable: equal keys keep the order of src
    return torch.sort(src[order[:expected]]).values


def sample_statement(cls, keys, num, expected_pos, neg_pos_ub, mistake=None):
    """BaseSampler.sample's index logic -> (inds int64: positives then negatives, each ascending; (np, nn)).
    From each group (cls > 0, then cls == 0) the `expected` members with the numerically smallest keys (-0.0 equals +0.0, ties to
    the lower index; all members when the group is not larger).  expected_neg = num - np and, if neg_pos_ub >= 0, also
    min(., int(neg_pos_ub * max(1, np))) in Python double on the caller's value."""
    assert not bool(torch.isnan(keys).any()), 'NaN keys are unspecified'
    cls, keys = cls.cpu(), keys.cpu()
    pos = _smallest(torch.nonzero(cls > 0).reshape(-1), keys, int(expected_pos), mistake)
    n_pos = pos.numel()
    expected_neg = num - (int(expected_pos) if mistake == 'neg_expected_ignores_np' else n_pos)
    if neg_pos_ub >= 0:
        ub = int(neg_pos_ub * max(1, n_pos))
        if mistake == 'ub_in_f32':
            ub = int(torch.tensor(neg_pos_ub, dtype=torch.float32) * torch.tensor(float(max(1, n_pos)), dtype=torch.float32))
        expected_neg = min(expected_neg, ub)
    neg = _smallest(torch.nonzero(cls == 0).reshape(-1), keys, expected_neg, mistake)
    return torch.cat([pos, neg]), (n_pos, neg.numel())


MISTAKES_SAMPLE = ('tie_highest_index', 'signed_zero_ordered', 'ub_in_f32', 'neg_expected_ignores_np')

SAMPLE_N = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 5000]
SAMPLE_FAMILIES = ['continuous', 'coarse', 'negative', 'all_equal', 'zeros_infs', 'low_byte']
SAMPLE_UBS = (-1.0, 0.0, 2.0)
BIG_UB = 1e10                                                   # ub * np is beyond int: the cap must act as no cap
# (neg_pos_ub, positives sampled): int(ub * np) in double is 28, 28, 63; in f32 29, 29, 62
SAMPLE_FRACTIONAL = [(0.29, 100), (1.16, 25), (0.21, 300)]


def sample_keys(family, n, g):
    r = torch.rand(n, generator=g)
    if family == 'continuous':
        return r
    if family == 'coarse':                                      # quarter steps: many ties
        return (r * 4).floor() / 4
    if family == 'negative':                                    # the OHEM use: -loss
        return -(r * 8).floor() / 3 + 1
    if family == 'all_equal':
        return torch.full((n,), 0.375)
    if family == 'zeros_infs':
        vals = torch.tensor([-0.0, 0.0, -0.0, 0.0, float('inf'), float('-inf'), 0.5, -0.5])     # half zeros: the middle cuts fall among them
        return vals[torch.randint(0, 8, (n,), generator=g)]
    assert family == 'low_byte'                                 # the top 24 bits shared: only the lowest byte separates the keys
    bits = torch.randint(0, 256, (n,), generator=g, dtype=torch.int32) | 0x3F000000
    return bits.view(torch.float32)


def sample_case(n, family, seed=None, few_pos=False):
    """(cls int64 [n] in {-1, 0, 1, 2}, keys f32 [n]); few_pos: nine in ten boxes negative."""
    g = torch.Generator().manual_seed(1000 * SAMPLE_FAMILIES.index(family) + n if seed is None else seed)
    cls = torch.randint(-1, 3, (n,), generator=g)
    if few_pos:
        cls[torch.rand(n, generator=g) < 0.9] = 0
    return cls, sample_keys(family, n, g)


def sample_configs(cls):
    """(num, expected_pos, neg_pos_ub).  Without a cap (ub -1), so that the sizes named are the sizes sampled: expected_pos on each
    side of the positives (0, 1, P - 1, P, P + 1) with a roomy num -- at P + 1 the negatives fill up what the positives leave --,
    expected_neg = num - np on each side of the negatives (0, 1, N - 1, N, N + 1), and num > n (both groups taken whole).  Then the
    caps on a roomy call: ub 0 (no negatives), 2, BIG_UB (a product beyond int: no cap), and ub 2 with num > n."""
    n = cls.numel()
    P, N = int((cls > 0).sum()), int((cls == 0).sum())
    out = []
    for ep in (0, 1, P - 1, P, P + 1):
        if ep >= 0:
            out.append((min(ep, P) + max(1, N // 2), ep, -1.0))
    ep = P // 2
    for en in (0, 1, N - 1, N, N + 1):
        if en >= 0 and ep + en > 0:
            out.append((ep + en, ep, -1.0))
    out.append((n + 7, P + 1, -1.0))
    for ub in SAMPLE_UBS[1:] + (BIG_UB,):
        out.append((ep + max(1, N // 2), ep, ub))
    out.append((n + 7, P + 1, 2.0))
    return [(num, ep, ub) for num, ep, ub in out if 0 <= ep <= num]


def sample_calls(n):
    """every (cls, keys, num, expected_pos, ub) the GPU test runs at size n; n None: the fractional caps.  Every key family with the
    classes drawn evenly, the continuous and the negative family also with few positives (the "take them all" branch)."""
    if n is None:
        for ub, n_pos in SAMPLE_FRACTIONAL:
            cls, keys, num, ep = sample_fractional_case(ub, n_pos)
            yield cls, keys, num, ep, ub
        return
    for fam, few in [(f, False) for f in SAMPLE_FAMILIES] + [('continuous', True), ('negative', True)]:
        cls, keys = sample_case(n, fam, few_pos=few)
        for num, ep, ub in sample_configs(cls):
            yield cls, keys, num, ep, ub


def sample_fractional_case(ub, n_pos):
    """cls with 2 n_pos positives and many negatives, expected_pos = n_pos, a roomy num: np = n_pos and the cap decides."""
    n = 2 * n_pos + 400
    g = torch.Generator().manual_seed(n_pos)
    cls = torch.zeros(n, dtype=torch.long)
    cls[torch.randperm(n, generator=g)[: 2 * n_pos]] = 1
    cls[torch.randperm(n, generator=g)[:20]] = -1
    n_pos_all = int((cls > 0).sum())
    assert n_pos_all >= n_pos and int((cls == 0).sum()) > int(ub * n_pos) + 2
    return cls, torch.rand(n, generator=g), n_pos + 200, n_pos


# ================================================================================================ mining
def _lowest(mask, highest=False):
    """per row the lowest (highest) column where mask holds; Mk where it holds nowhere"""
    Mk = mask.shape[1]
    idx = torch.arange(Mk, device=mask.device)[None, :].expand_as(mask)
    if highest:
        return torch.where(mask, idx, torch.full_like(idx, -1)).max(1).values
    return torch.where(mask, idx, torch.full_like(idx, Mk)).min(1).values


def mining_statement(aff, labels, all_labels, mistake=None):
    """hard-proposal mining -> int64 [Mq, 4], from the reference's own construction (masked_fill with -+inf), then the LOWEST index
    among the extrema:
      [r, 0] = [r, 2] = first argmax over keys whose label differs from row r's (masked-out keys count as -inf),
      [r, 1] = first argmin over keys with row r's label (masked-out keys count as +inf),
      [r, 3] = first argmax of the same masked row over the keys other than [r, 2]; 0 when Mk == 1.
    A row without candidates therefore answers 0 (0, 1 for the pair), a row with one candidate the lowest other index as its
    second pick.  +-inf affinities are legal values; NaN is excluded."""
    assert not bool(torch.isnan(aff).any()), 'NaN affinities are unspecified'
    Mq, Mk = aff.shape
    a = aff.double()
    diff = all_labels[None, :] != labels[:, None]
    hi = a.masked_fill(~diff, float('-inf'))
    lo = a.masked_fill(diff if mistake != 'min_over_other_group' else ~diff, float('inf'))
    high = mistake == 'tie_highest_index'
    first = _lowest(hi == hi.max(1, keepdim=True).values, high)
    low = _lowest(lo == lo.min(1, keepdim=True).values, high)
    cols = torch.arange(Mk, device=aff.device)[None, :]
    if Mk > 1:
        other = cols != first[:, None]
        rest = hi.masked_fill(~other, float('-inf'))
        at_max = rest == rest.max(1, keepdim=True).values
        second = _lowest(at_max if mistake == 'second_may_repeat_first' else at_max & other, high)
    else:
        second = torch.zeros_like(first)
    if mistake == 'no_candidate_answers_last':
        none_d, none_s = ~diff.any(1), ~(~diff).any(1)
        first = torch.where(none_d, torch.full_like(first, Mk - 1), first)
        second = torch.where(none_d, torch.full_like(first, max(Mk - 2, 0)), second)
        low = torch.where(none_s, torch.full_like(low, Mk - 1), low)
    return torch.stack([first, low, first, second], 1)


MISTAKES_MINING = ('tie_highest_index', 'second_may_repeat_first', 'min_over_other_group', 'no_candidate_answers_last')
MISTAKE_CASE_MINING = {'tie_highest_index': 'coarse', 'second_may_repeat_first': 'one_diff', 'min_over_other_group': 'continuous',
                       'no_candidate_answers_last': 'all_same'}
MINING_MQ = [1, 3, 4, 5, 9]
MINING_MK = [1, 2, 63, 64, 65, 127, 128, 129, 300]
MINING_KINDS = ['continuous', 'coarse', 'all_same', 'one_diff', 'dup64']
MINING_LABELS = [-3, 0, 1, 2 ** 40 + 1]                         # negative and large int64 labels
BIG_F32 = 3.0e38


def mining_case(Mq, Mk, kind, seed=None, infs=True):
    """(aff f32 [Mq, Mk], labels int64 [Mq], all_labels int64 [Mk]).
    continuous / coarse (quarter steps): random labels out of MINING_LABELS; with infs, row 0 holds +inf and -inf entries (each twice
    when Mk allows) and the last row's label (77) matches no key.
    all_same: every key carries one label; rows alternate between that label (no different-label candidate) and another (no
    same-label candidate).
    one_diff: every key but one carries label 5, that one label 4; rows alternate 5 (exactly one different-label candidate: the
    second pick is the lowest other index) and 4 (exactly one same-label candidate); the lone key sits at index 0 for odd Mq.
    dup64: the row maximum (and minimum) duplicated bit for bit at indices j and j + 64 (the same lane, a lower index), labels so
    that both copies are candidates."""
    g = torch.Generator().manual_seed(100 * Mq + Mk + 7 * MINING_KINDS.index(kind) if seed is None else seed)
    aff = torch.randn((Mq, Mk), generator=g) * 4
    pool = torch.tensor(MINING_LABELS)
    labels = pool[torch.randint(0, 4, (Mq,), generator=g)]
    all_labels = pool[torch.randint(0, 4, (Mk,), generator=g)]
    if kind == 'coarse':
        aff = (aff * 4).round() / 4
    if kind in ('continuous', 'coarse') and infs:
        at = torch.randperm(Mk, generator=g)
        aff[0, at[:2]] = float('inf')
        aff[0, at[2:4]] = float('-inf')
        labels[Mq - 1] = 77
    if kind == 'all_same':
        all_labels[:] = 2 ** 40 + 1
        labels = torch.where(torch.arange(Mq) % 2 == 0, 2 ** 40 + 1, -3)
    if kind == 'one_diff':
        all_labels[:] = 5
        all_labels[0 if Mq % 2 else Mk // 2] = 4
        labels = torch.where(torch.arange(Mq) % 2 == 0, 5, 4)
    if kind == 'dup64':
        all_labels[:] = torch.where(torch.arange(Mk) % 2 == 0, 0, 1)          # j and j + 64 share a label
        labels = torch.arange(Mq) % 2
        for r in range(Mq):
            js = [(j + 3 * r) % (Mk - 64) for j in range(max(Mk - 64, 0))]
            jmax = [j for j in js if j % 2 != r % 2][:1]                      # a different-label key (the other parity) ...
            jmin = [j for j in js if j % 2 == r % 2][:1]                      # ... and a same-label key
            for j in jmax:
                aff[r, j] = aff[r, j + 64] = 100.0 + r
            for j in jmin:
                aff[r, j] = aff[r, j + 64] = -100.0 - r
    return aff.float(), labels.long(), all_labels.long()


# ================================================================================================ triplet
def _sqrt(x):
    """sqrtf of a non-negative Val: the interval's image plus SQRTF_ULP ulp."""
    v = x.v.sqrt()
    e_in = torch.maximum((x.v + x.e).sqrt() - v, v - (x.v - x.e).clamp(min=0.0).sqrt())
    return Val(v, e_in + L.SQRTF_ULP * ULP * (v + e_in))


def _div(a, b, unchecked=False):
    """a / b at DIV_ULP ulp."""
    if not unchecked:
        assert bool((b.v.abs() > b.e).all()), 'divisor not bounded away from zero'
    v = a.v / b.v
    e_in = (a.e + v.abs() * b.e) / (b.v.abs() - b.e)
    return Val(v, e_in + L.DIV_ULP * ULP * (v.abs() + e_in))


def _chain_sum(t, dim, chain):
    """A sum of the Val t along dim whose longest chain of additions is `chain`: the terms' own errors, plus chain u sum |term as
    computed|, second-order terms covered by SECOND."""
    return Val(t.v.sum(dim), SECOND * (t.e.sum(dim) + chain * U * (t.v.abs() + t.e).sum(dim)))


def _scatter_sum(rows, t, idx, count):
    """out[idx[i]] += t[i] over the rows of t, in f32, sequentially per output row: chain = count[row] additions."""
    D = t.v.shape[1]
    v = torch.zeros((rows, D), dtype=torch.float64).index_add_(0, idx, t.v)
    e = torch.zeros((rows, D), dtype=torch.float64).index_add_(0, idx, t.e)
    mag = torch.zeros((rows, D), dtype=torch.float64).index_add_(0, idx, t.v.abs() + t.e)
    return Val(v, SECOND * (e + count.double()[:, None] * U * mag))


def triplet_statement(q, k, a, p, m, margin, mistake=None):
    """hvr_triplet_margin on the kernel's own f32 / bf16 operands -> dict of Vals dp, dn, l [n], out2 [2] = (loss, active), dq [Mq, D],
    dk [Mk, D], plus `active` (bool [n]), `exact` (bool [n]) and `decision` = min over the non-exact triples of |l_i| / bound.
      e = (x - y) + 1e-6f: two roundings.  s = sum_d e_d^2: each square rounded, lane chain ceil(D / 64) and a 6-level tree.
      d = sqrtf(s) at SQRTF_ULP.  l = (dp - dn) + margin: two roundings; active where l > 0.
      A triple whose positive and negative rows are bit-equal (p == m included) computes dp and dn by the same operations on the
      same numbers: dp - dn is exactly 0 and l exactly the f32 margin (`exact`; bound 0).
      loss = sum_active l * (1 / max(#active, 1)): 256 lanes (chain ceil(n / 256)) and an 8-level tree, one division at DIV_ULP,
      one multiply.  #active is an integer below 2^24: exact.
      gradient element: g (up - un) onto dq[a], -g up onto dk[p], g un onto dk[m], with up = e_p / dp, un = e_n / dn (one
      division at DIV_ULP each), g = 1 / max(#active, 1): a subtraction and a multiply (dq), a multiply (dk), then a chain as
      long as the number of ACTIVE triples naming that row (counted from the indices; dk: as positive plus as negative).
      Rows no active triple names are exactly zero (bound 0)."""
    Mq, D = q.shape
    Mk = k.shape[0]
    n = a.numel()
    a, p, m = a.cpu().long(), p.cpu().long(), m.cpu().long()
    qd, kd = q.detach().cpu().double(), k.detach().cpu().double()
    eps = 0.0 if mistake == 'eps_dropped' else f32v(1e-6)
    mg = f32v(margin)
    x, y, z = Val(qd[a]), Val(kd[p]), Val(kd[m])
    ep, en = (x - y) + eps, (x - z) + eps
    chain = L.block_chain(D, 64, 6)
    dp, dn = _sqrt(_chain_sum(ep * ep, 1, chain)), _sqrt(_chain_sum(en * en, 1, chain))
    l = (dp - dn) + mg
    exact = (kd[p] == kd[m]).all(1)
    l = Val(torch.where(exact, torch.full_like(l.v, mg), l.v), torch.where(exact, torch.zeros_like(l.e), l.e))
    active = l.v >= 0 if mistake == 'active_is_ge' else l.v > 0
    rest = ~exact
    decision = float((l.v.abs() / l.e.clamp(min=1e-300))[rest].min()) if bool(rest.any()) else float('inf')
    lr = l.clamp(min=0.0)
    cnt = int(active.sum())
    denom = float(n) if mistake == 'mean_over_n' else float(max(cnt, 1))
    tot = _chain_sum(lr, 0, L.block_chain(n, 256, 8))
    loss_v = tot.v / denom
    loss = Val(loss_v, SECOND * (tot.e / denom + (L.DIV_ULP * ULP + U) * (loss_v.abs() + tot.e / denom)) + TINY * float(cnt > 0))
    out2 = Val(torch.stack([loss.v, torch.tensor(float(cnt), dtype=torch.float64)]), torch.stack([loss.e, torch.zeros((), dtype=torch.float64)]))

    g = Val(torch.tensor(1.0 / denom, dtype=torch.float64), torch.tensor(L.DIV_ULP * ULP / denom, dtype=torch.float64))
    sel = torch.ones(n, dtype=torch.bool) if mistake == 'inactive_in_gradient' else active
    ia, ip, im = a[sel], p[sel], m[sel]
    bad = mistake == 'eps_dropped'
    if mistake == 'grad_not_divided_by_distance':
        up, un = ep[sel], en[sel]
    else:
        up, un = _div(ep[sel], Val(dp.v[sel][:, None], dp.e[sel][:, None]), bad), _div(en[sel], Val(dn.v[sel][:, None], dn.e[sel][:, None]), bad)
    tq, tp, tn = (up - un) * g, (up * g).neg(), un * g
    if mistake == 'dk_signs_swapped':
        tp, tn = tp.neg(), tn.neg()
    cq = torch.bincount(ia, minlength=Mq)
    ck = torch.bincount(ip, minlength=Mk) + torch.bincount(im, minlength=Mk)
    if mistake == 'collision_overwrites':                      # the last triple naming a row wins
        dq = Val(torch.zeros((Mq, D), dtype=torch.float64))
        dk = Val(torch.zeros((Mk, D), dtype=torch.float64))
        for i in range(ia.numel()):
            dq.v[ia[i]], dk.v[ip[i]] = tq.v[i], tp.v[i]
            dk.v[im[i]] = tn.v[i]
    else:
        dq = _scatter_sum(Mq, tq, ia, cq)
        both = Val(torch.cat([tp.v, tn.v]), torch.cat([tp.e, tn.e]))
        dk = _scatter_sum(Mk, both, torch.cat([ip, im]), ck)
    return dict(dp=dp, dn=dn, l=l, out2=out2, dq=dq, dk=dk, active=active, exact=exact, decision=decision, count_q=cq, count_k=ck)


MISTAKES_TRIPLET = ('eps_dropped', 'mean_over_n', 'active_is_ge', 'inactive_in_gradient', 'collision_overwrites', 'dk_signs_swapped',
                    'grad_not_divided_by_distance')


def triplet_f32(q, k, a, p, m, margin, order):
    """The same function by plain PyTorch in f32 with autograd: order 0 sums the squares with torch's own reduction, order 1 over
    the reversed columns in two halves.  -> (dp, dn, out2, dq, dk) f32."""
    qf, kf = q.detach().cpu().float().requires_grad_(True), k.detach().cpu().float().requires_grad_(True)
    eps = torch.tensor(1e-6, dtype=torch.float32)

    def dist(x, y):
        e = (x - y) + eps
        s = e * e
        if order == 0:
            return torch.sqrt(s.sum(1))
        s = s.flip(1)
        h = s.shape[1] // 2
        return torch.sqrt(s[:, :h].sum(1) + s[:, h:].sum(1))
    dp, dn = dist(qf[a], kf[p]), dist(qf[a], kf[m])
    l = torch.relu((dp - dn) + torch.tensor(margin, dtype=torch.float32))
    active = (l > 0).sum()
    loss = l.sum() * (1.0 / active.clamp(min=1).float())
    loss.backward()
    return dp.detach(), dn.detach(), torch.stack([loss.detach(), active.float()]), qf.grad, kf.grad


TRIPLET_MQ, TRIPLET_MK = 7, 9
TRIPLET_D = [1, 63, 64, 65, 255, 256, 257, 1024]
TRIPLET_N = [1, 3, 4, 5, 255, 256, 257, 600]
TRIPLET_DTYPES = [torch.float32, torch.bfloat16]


def triplet_cases():
    """(name, dict(D, n, kind)) of every triplet input set; each runs in f32 and bf16, with contiguous and pitched rows.
    plain: margin 10, every index random (all active).  collide: positives from three rows, margin 0.5, a quarter of the negatives
    far away (inactive triples).  mixed: as collide with all key rows.  exact_zero: margin 0 and p == m for triple 1 (l == 0
    exactly: inactive).  equal_row: anchor row of triple 0 bit-equal to its positive row (d = 1e-6 sqrt(D)).  all_inactive:
    margin -100."""
    out = [('D%d-plain' % D, dict(D=D, n=5, kind='plain')) for D in TRIPLET_D]
    out += [('n%d-collide' % n, dict(D=65, n=n, kind='collide')) for n in TRIPLET_N]
    out += [('mixed', dict(D=65, n=257, kind='mixed')), ('exact_zero', dict(D=65, n=5, kind='exact_zero')),
            ('equal_row', dict(D=65, n=5, kind='equal_row')), ('equal_row_D256', dict(D=256, n=4, kind='equal_row')),
            ('all_inactive', dict(D=65, n=257, kind='all_inactive'))]
    return out


MISTAKE_CASE_TRIPLET = {'eps_dropped': 'equal_row', 'mean_over_n': 'mixed', 'active_is_ge': 'exact_zero', 'inactive_in_gradient': 'mixed',
                        'collision_overwrites': 'n255-collide', 'dk_signs_swapped': 'D65-plain', 'grad_not_divided_by_distance': 'D65-plain'}
TRIPLET_MARGIN = {'plain': 10.0, 'collide': 0.5, 'mixed': 0.5, 'exact_zero': 0.0, 'equal_row': 10.0, 'all_inactive': -100.0}
PITCH_PAD = 8


def triplet_case(name, c, dtype):
    """-> dict(q [Mq, D], k [Mk, D] in dtype (contiguous), a, p, m int64 [n], margin)."""
    D, n, kind = c['D'], c['n'], c['kind']
    # (with these seeds every non-exact triple's |l| stands ten bounds clear of zero: test_mining_refs.py asserts it for every case)
    g = torch.Generator().manual_seed(17 * D + n + (1 if dtype == torch.bfloat16 else 0))
    q = torch.randn((TRIPLET_MQ, D), generator=g) * 0.3
    k = torch.randn((TRIPLET_MK, D), generator=g) * 0.3
    a = torch.randint(0, TRIPLET_MQ, (n,), generator=g)
    p = torch.randint(0, 3 if kind == 'collide' else TRIPLET_MK, (n,), generator=g)
    m = torch.randint(0, TRIPLET_MK, (n,), generator=g)
    if kind in ('collide', 'mixed'):
        k[6:] = k[6:] * 6                                       # far rows: triples whose negative is one of them are inactive
    q, k = q.to(dtype), k.to(dtype)
    if kind == 'exact_zero':
        m[min(1, n - 1)] = p[min(1, n - 1)]
    if kind == 'equal_row':
        a[0], p[0] = 2, 4
        q[2] = k[4]
        m[0] = 5
    return dict(q=q, k=k, a=a, p=p, m=m, margin=TRIPLET_MARGIN[kind])


def pitched(t, pad=PITCH_PAD, fill=float('nan')):
    """t [R, D] as a column slice of a buffer `pad` columns wider, filled with `fill` outside the slice."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]
