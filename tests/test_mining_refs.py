"""The statements and bounds of tests/mining_refs.py checked on the host, without a GPU, on every input set the GPU tests use:
  * against torch in f64: the triplet against F.pairwise_distance with autograd and the AvgNonZero reduction (1e-12 relative), the
    sampler against oracle/hvr_oracle.py::sample_pos_neg, the mining (tie-free finite inputs) against the masked_fill + topk lines
    of the reference's hardest_proposal_mining restated here;
  * the triplet bound is wide enough: two independent f32 evaluations (torch f32, two summation orders) lie inside it;
  * the mistakes are caught: every listed triplet mistake moves an output by ten bounds on the case named for it, every sampler and
    mining mistake changes an index on its case;
  * the active decision: every non-exact triple of every triplet case has |l| above ten bounds, so nothing is left out of a comparison.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import mining_refs as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def O():
    import subprocess
    if not os.path.exists(os.path.join(ROOT, 'oracle', 'libhvr_oracle.so')):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'oracle')], check=True)
    from oracle import hvr_oracle
    return hvr_oracle


# ------------------------------------------------------------------------------------------------ sampler
def test_sample_statement_equals_the_oracle(O):
    """oracle/hvr_oracle.py::sample_pos_neg takes a fraction: (ep + 0.5) / num makes int(num * fraction) == ep."""
    calls = 0
    for cls, keys, num, ep, ub in (c for n in M.SAMPLE_N + [None] for c in M.sample_calls(n)):
        frac = (ep + 0.5) / num
        assert int(num * frac) == ep
        pos, neg = O.sample_pos_neg(cls, keys, num, frac, ub)
        inds, (n_pos, n_neg) = M.sample_statement(cls, keys, num, ep, ub)
        assert (n_pos, n_neg) == (pos.numel(), neg.numel()), (cls.numel(), num, ep, ub)
        assert torch.equal(inds, torch.cat([pos, neg])), (cls.numel(), num, ep, ub)
        calls += 1
    assert calls > 800


def test_sample_cases_reach_what_they_name():
    """Both signs of zero and both infinities among the candidates of the zeros family; the low-byte keys share their upper 24 bits and
    differ; the configurations stand on both sides of both group sizes and include num > n; the fractional caps bind."""
    cls, keys = M.sample_case(1025, 'zeros_infs')
    for grp in (cls > 0, cls == 0):
        kk = keys[grp]
        assert bool(((kk == 0) & torch.signbit(kk)).any()) and bool(((kk == 0) & ~torch.signbit(kk)).any())
        assert bool((kk == float('inf')).any()) and bool((kk == float('-inf')).any())
    bits = M.sample_case(1025, 'low_byte')[1].view(torch.int32)
    assert int((bits >> 8).unique().numel()) == 1 and int((bits & 255).unique().numel()) > 200
    for ub, n_pos in M.SAMPLE_FRACTIONAL:
        cls, keys, num, ep = M.sample_fractional_case(ub, n_pos)
        _, (got_pos, got_neg) = M.sample_statement(cls, keys, num, ep, ub)
        assert got_pos == n_pos and got_neg == int(ub * n_pos) < num - n_pos


@pytest.mark.parametrize('n', [x for x in M.SAMPLE_N if x >= 63])
def test_sample_calls_sample_the_sizes_they_name(n):
    """What the statement RETURNS over the calls of one size (after the cap, not before it): per family, np reaches 0, 1, P - 1 with a
    cut inside the group, P exactly and P through the take-all branch (expected P + 1); nn reaches 0, 1, N - 1 with a cut inside,
    N exactly and N through the take-all branch; num > n takes both groups whole; after a short positive group the negatives fill
    up to num - P; ub 0 leaves no negative, ub 2 caps at 2 np where more were asked for, the huge ub caps nothing."""
    for fam, few in [(f, False) for f in M.SAMPLE_FAMILIES] + [('continuous', True), ('negative', True)]:
        cls, keys = M.sample_case(n, fam, few_pos=few)
        P, N = int((cls > 0).sum()), int((cls == 0).sum())
        assert P >= 2 and N >= 3
        seen_p, seen_n, flags = set(), set(), set()
        for num, ep, ub in M.sample_configs(cls):
            _, (n_pos, n_neg) = M.sample_statement(cls, keys, num, ep, ub)
            asked = num - n_pos
            if ub < 0:
                seen_p.add((n_pos, ep > P))
                seen_n.add((n_neg, asked > N))
                if ep > P and n_neg == num - P > num - ep:
                    flags.add('filled_up')
                if num > n and (n_pos, n_neg) == (P, N):
                    flags.add('both_whole')
            elif ub == 0.0 and asked > 0 and n_neg == 0:
                flags.add('ub0')
            elif ub == 2.0 and n_neg == 2 * max(1, n_pos) < min(asked, N):
                flags.add('ub2_binds')
            elif ub == M.BIG_UB and n_neg == min(asked, N) > 0:
                flags.add('big_ub_no_cap')
        assert seen_p >= {(0, False), (1, False), (P - 1, False), (P, False), (P, True)}, (fam, few, seen_p)
        assert seen_n >= {(0, False), (1, False), (N - 1, False), (N, False), (N, True)}, (fam, few, seen_n)
        want = {'filled_up', 'both_whole', 'ub0', 'big_ub_no_cap'} | ({'ub2_binds'} if 2 * (P // 2) < N // 2 else set())
        assert flags >= want, (fam, few, flags)
    cls, _ = M.sample_case(n, 'continuous', few_pos=True)
    assert int((cls > 0).sum()) < n // 4                                        # few positives


def test_the_cap_differs_between_double_and_f32():
    """int(neg_pos_ub * np): the reference's Python double against the f32 product of an f32 argument, and the double product of
    the f32 argument (converting inside the kernel would not help: the argument has to arrive as a double)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    assert int(0.29 * 100) != int(f32(0.29) * f32(100.0))
    for ub, n_pos, dbl, sgl in ((0.29, 100, 28, 29), (1.16, 25, 28, 29), (0.21, 300, 63, 62)):
        assert int(ub * n_pos) == dbl and int(f32(ub) * f32(float(n_pos))) == sgl
    assert int(float(f32(0.21)) * 300) == 62


@pytest.mark.parametrize('n', [x for x in M.SAMPLE_N if x >= 63] + [None])
def test_sampler_mistakes_change_an_index_on_the_gpu_calls(n):
    """Every listed mistake changes a count or an index on at least one call the GPU test makes at this size: ties to the highest
    index, signed zeros ranked and the negatives' expectation taken from expected_pos at every n >= 63, the f32 cap on each of the
    three fractional calls (n None)."""
    calls = list(M.sample_calls(n))
    for mistake in M.MISTAKES_SAMPLE:
        changed = 0
        for cls, keys, num, ep, ub in calls:
            want, wc = M.sample_statement(cls, keys, num, ep, ub)
            got, gc = M.sample_statement(cls, keys, num, ep, ub, mistake=mistake)
            changed += int(wc != gc or not torch.equal(want, got))
        if n is None:
            assert changed == (len(calls) if mistake == 'ub_in_f32' else 0), (mistake, changed)
        elif mistake != 'ub_in_f32':                   # (the caps of these calls, 0, 2 and 1e10, are exact in f32)
            assert changed >= 3, (mistake, n, changed)


# ------------------------------------------------------------------------------------------------ mining
def _mining_calls():
    for Mk in M.MINING_MK:
        for Mq in M.MINING_MQ:
            for kind in M.MINING_KINDS:
                yield (Mq, Mk, kind) + M.mining_case(Mq, Mk, kind)


def test_mining_statement_equals_the_reference_lines_on_tie_free_rows():
    """hrnmp_bbox_head.py: masked_fill(-inf) + topk(1) / topk(2), masked_fill(+inf) + topk(1, largest=False) -- on continuous finite
    affinities, for the rows with at least two different-label and one same-label key (elsewhere -inf ties, whose topk order is
    unspecified)."""
    rows = 0
    for Mk in M.MINING_MK:
        for Mq in M.MINING_MQ:
            aff, labels, all_labels = M.mining_case(Mq, Mk, 'continuous', infs=False)
            assert bool(torch.isfinite(aff).all()) and all(aff[r].unique().numel() == Mk for r in range(Mq))
            got = M.mining_statement(aff, labels, all_labels)
            same = all_labels[None, :] == labels[:, None]
            k = min(2, Mk)
            sm = aff.masked_fill(same, float('-inf')).topk(k, dim=1).indices
            nsm = aff.masked_fill(~same, float('inf')).topk(1, dim=1, largest=False).indices
            ok_d, ok_s = (~same).sum(1) >= 2, same.sum(1) >= 1
            assert Mk < 2 or (torch.equal(got[ok_d][:, 2:], sm[ok_d]) and torch.equal(got[ok_d, 0], sm[ok_d, 0]))
            assert torch.equal(got[ok_s, 1], nsm[ok_s, 0])
            rows += int(ok_d.sum())
    assert rows > 100


def test_mining_statement_on_the_rows_without_choice():
    """no candidate: 0, or (0, 1); one candidate: that key and the lowest other index; Mk == 1: second pick 0; +-inf are values."""
    inf = float('inf')
    aff = torch.tensor([[1.0, 5.0, 3.0, 5.0], [-inf, 2.0, inf, inf], [0.0, 0.0, 0.0, 0.0]])
    got = M.mining_statement(aff, torch.tensor([7, 1, 2]), torch.tensor([1, 1, 2, 1]))
    assert got[0].tolist() == [1, 0, 1, 3]                                      # label 7 matches no key: argmin over nothing -> 0
    assert got[1].tolist() == [2, 0, 2, 0]                                      # one different key (index 2); second: lowest other
    assert got[2].tolist() == [0, 2, 0, 1]                                      # ties: lowest index, the second the next
    got = M.mining_statement(aff[:, :1], torch.tensor([7, 1, 2]), torch.tensor([1]))
    assert got.tolist() == [[0, 0, 0, 0]] * 3
    got = M.mining_statement(aff, torch.tensor([1, 1, 1]), torch.tensor([1, 1, 1, 1]))
    assert got[:, [0, 2, 3]].tolist() == [[0, 0, 1]] * 3 and got[:, 1].tolist() == [0, 0, 0]
    got = M.mining_statement(torch.tensor([[inf, -inf, -inf, inf]]), torch.tensor([0]), torch.tensor([1, 1, 0, 0]))
    assert got.tolist() == [[0, 2, 0, 1]]            # a candidate at -inf ties with the masked keys: the lowest index among them


def test_mining_cases_reach_what_they_name():
    seen = dict(no_diff=0, no_same=0, one_diff=0, inf=0, dup=0)
    for Mq, Mk, kind, aff, labels, all_labels in _mining_calls():
        diff = all_labels[None, :] != labels[:, None]
        seen['no_diff'] += int((diff.sum(1) == 0).sum())
        seen['no_same'] += int(((~diff).sum(1) == 0).sum())
        seen['one_diff'] += int((diff.sum(1) == 1).sum()) if Mk > 2 else 0
        seen['inf'] += int(torch.isinf(aff).any(1).sum())
        if kind == 'dup64' and Mk > 64:
            hi = aff.masked_fill(~diff, float('-inf'))
            at = hi == hi.max(1, keepdim=True).values
            first = M.mining_statement(aff, labels, all_labels)[:, 0]
            dup = at.sum(1) == 2
            seen['dup'] += int((dup & at[torch.arange(Mq), (first + 64).clamp(max=Mk - 1)]).sum())
        assert int(all_labels.min()) < 0 or kind in ('one_diff', 'dup64', 'all_same') or Mk < 8
    assert all(v >= 20 for v in seen.values()), seen


@pytest.mark.parametrize('mistake', M.MISTAKES_MINING)
def test_mining_mistakes_change_an_index(mistake):
    aff, labels, all_labels = M.mining_case(9, 300, M.MISTAKE_CASE_MINING[mistake])
    assert not torch.equal(M.mining_statement(aff, labels, all_labels), M.mining_statement(aff, labels, all_labels, mistake=mistake))


# ------------------------------------------------------------------------------------------------ triplet
TRIPLET = [(name, c, dt) for name, c in M.triplet_cases() for dt in M.TRIPLET_DTYPES]
IDS = ['%s-%s' % (name, 'bf16' if dt == torch.bfloat16 else 'f32') for name, c, dt in TRIPLET]
_cache = {}


def _statement(name, c, dt):
    key = (name, dt)
    if key not in _cache:
        case = M.triplet_case(name, c, dt)
        _cache[key] = (case, M.triplet_statement(**case))
    return _cache[key]


def _inside(got, val, what):
    worst, at, over = M.ratio(got, val)
    assert worst <= 1.0, '%s: worst error / bound %g at flat index %d, %d over' % (what, worst, at, over)


@pytest.mark.parametrize('name,c,dt', TRIPLET, ids=IDS)
def test_triplet_statement_equals_torch_in_f64(name, c, dt):
    case, ref = _statement(name, c, dt)
    q, k = case['q'].double().requires_grad_(True), case['k'].double().requires_grad_(True)
    a, p, m = case['a'], case['p'], case['m']
    eps = M.f32v(1e-6)
    dp = F.pairwise_distance(q[a], k[p], 2, eps)
    dn = F.pairwise_distance(q[a], k[m], 2, eps)
    l = F.relu(dp - dn + M.f32v(case['margin']))
    l = torch.where(ref['exact'], torch.full_like(l, max(M.f32v(case['margin']), 0.0)), l)     # (f64 leaves ~1e-17 where f32 leaves 0)
    active = (l > 0).sum()
    loss = l.sum() / active.clamp(min=1)
    loss.backward()
    tol = lambda t: 1e-12 * t.abs() + 1e-300
    assert bool(((ref['dp'].v - dp.detach()).abs() <= tol(dp.detach())).all()) and bool(((ref['dn'].v - dn.detach()).abs() <= tol(dn.detach())).all())
    assert int(ref['out2'].v[1]) == int(active) == int(ref['active'].sum())
    assert abs(float(ref['out2'].v[0] - loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for got, want in ((ref['dq'].v, q.grad), (ref['dk'].v, k.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-14 * max(float(want.abs().max()), 1e-30))


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('name,c,dt', TRIPLET, ids=IDS)
def test_triplet_f32_evaluations_lie_inside_the_bound(name, c, dt, order):
    case, ref = _statement(name, c, dt)
    dp, dn, out2, dq, dk = M.triplet_f32(case['q'], case['k'], case['a'], case['p'], case['m'], case['margin'], order)
    _inside(dp, ref['dp'], 'dp')
    _inside(dn, ref['dn'], 'dn')
    _inside(out2, ref['out2'], 'out2')
    _inside(dq, ref['dq'], 'dq')
    _inside(dk, ref['dk'], 'dk')


@pytest.mark.parametrize('name,c,dt', TRIPLET, ids=IDS)
def test_triplet_active_decision_is_clear_and_cases_reach_what_they_name(name, c, dt):
    """|l| above ten bounds for every triple whose l is not exact: the active count is decided and no triple is excluded."""
    case, ref = _statement(name, c, dt)
    assert ref['decision'] > 10.0, ref['decision']
    n, kind = c['n'], c['kind']
    n_act = int(ref['active'].sum())
    if kind in ('plain', 'equal_row'):
        assert n_act == n
    if kind == 'mixed' or (kind == 'collide' and n >= 255):
        assert 0 < n_act < n
    if kind == 'collide' and n >= 255:
        assert int(ref['count_k'][:3].max()) >= n // 8 and int(ref['count_q'].max()) >= n // 16
    if kind == 'exact_zero':
        i = min(1, n - 1)
        assert bool(ref['exact'][i]) and float(ref['l'].v[i]) == 0.0 and float(ref['l'].e[i]) == 0.0 and not bool(ref['active'][i])
        assert 0 < n_act < n
    if kind == 'equal_row':
        assert torch.equal(case['q'][2], case['k'][4])
        want = M.f32v(1e-6) * c['D'] ** 0.5
        assert abs(float(ref['dp'].v[0]) - want) <= 1e-6 * want
    if kind == 'all_inactive':
        assert n_act == 0 and float(ref['out2'].v[0]) == 0.0 and float(ref['out2'].e[0]) == 0.0
        assert not bool(ref['dq'].v.any()) and not bool(ref['dk'].v.any()) and not bool(ref['dq'].e.any())
    unnamed_q = ref['count_q'] == 0
    assert not bool(ref['dq'].v[unnamed_q].any()) and not bool(ref['dq'].e[unnamed_q].any())


def _moved(wrong, ref):
    d = (wrong.v - ref.v).abs()
    return bool((~torch.isfinite(wrong.v) | (d >= 10 * ref.e) & (d > 0)).any())


@pytest.mark.parametrize('dt', M.TRIPLET_DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('mistake', M.MISTAKES_TRIPLET)
def test_triplet_mistakes_move_an_output_by_ten_bounds(mistake, dt):
    name = M.MISTAKE_CASE_TRIPLET[mistake]
    c = dict(M.triplet_cases())[name]
    case, ref = _statement(name, c, dt)
    wrong = M.triplet_statement(mistake=mistake, **case)
    assert any(_moved(wrong[key], ref[key]) for key in ('out2', 'dq', 'dk')), mistake
