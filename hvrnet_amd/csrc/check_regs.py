"""Build-time check on the kernels' register allocation (run by build.sh on the compiler's -Rpass-analysis=kernel-resource-usage
remarks of every unit that units.txt builds with `remarks`).

RULES is the whole policy: one row per kernel family, the first row whose pattern matches a kernel's mangled name decides.  A kernel
no row matches is not gated; the check names the units in which that is true of every kernel, and it fails when a row matches no
kernel of the build (a stale row gates nothing and would go unnoticed).
"""
import os
import re
import sys

SERIAL = 'a serial sweep, scratch traffic inside its dependency chain is a silent slowdown'

# (pattern of the mangled name, bytes of scratch per lane allowed, reason).  Allowance 0: no VGPR spill and no scratch at all.
# An allowance above 0 covers values parked OUTSIDE the K loop only (checked in the .s: no scratch access between the loop's
# barriers); anything beyond it fails the build.
RULES = [
    (r'_ZN3hvr17expand_res_kernel', 0, 'expand.hip: sized for two workgroups per CU, a spill means it no longer fits'),
    (r'_ZN3hvr19expand_split_kernel', 0, 'expand_split.hip: sized for two workgroups per CU, a spill means it no longer fits'),
    (r'_ZN3hvr19mc_nms_', 0, 'nms.hip, the per-class read-out and its merge: ' + SERIAL),
    (r'_ZN3hvr15nms_', 0, 'nms.hip, the sort and the mask kernels: ' + SERIAL),
    (r'_ZN3hvr16nms_', 0, 'nms.hip, the greedy sweep with its prefetched IoU rows: ' + SERIAL),
    (r'_ZN3hvr17rpn_', 0, 'nms.hip, the proposal gather / select: ' + SERIAL),
    (r'_ZN3hvr25relation_scores_bt', 0, 'relation_bt.hip: the one-round scores kernel keeps 176 accumulators per lane'),
    (r'_ZN3hvr14pc_tile_kernelI(?:t|NS_5f16_tE)Li4ELi0E', 32,
     'pc_gemm.hip <4, LINEAR, 3>: the fattest compute waves park a few epilogue addresses before the loop'),
    (r'_ZN3hvr14pc_tile_kernelI(?:t|NS_5f16_tE)Li2ELi2E', 256,
     'pc_gemm.hip <2, APPLY, 4>: the folded accumulators are parked between the last block and the epilogue\'s LDS staging'),
    (r'_ZN3hvr14pc_tile_kernel', 0, 'pc_gemm.hip, every other shape: a big accumulator tile, scratch would land in the K loop'),
    (r'_ZN3hvr15big_tile_kernel', 0, 'bigtile.hip: a big accumulator tile, scratch would land in the K loop'),
    (r'_ZN3hvr\d+tta_', 0, 'tta.hip, the augmentation merge: ' + SERIAL),
    (r'_ZN3hvr\d+soft_nms_', 0, 'softnms.hip, the Soft-NMS rounds: ' + SERIAL),
    (r'_ZN3hvr\d+seq_nms_', 0, 'seqnms.hip, the Seq-NMS frame sweep: ' + SERIAL),
    (r'_ZN3hvr\d+deform_im2col_', 0, 'dcn.hip: the sampler keeps four corner vectors in flight per lane'),
    (r'_ZN3hvr\d+deform_roi_pool_', 0, 'dpool.hip: a row of samples, 4 x sample_per_part corner vectors, in flight per lane'),
    (r'_ZN3hvr\d+roi_pool_fwd_', 0, 'roi_pool.hip: a lane keeps the running maxima and indices of its 16-byte piece and the unrolled '
     'walk\'s loads in registers, a spill would sit inside the walk over a bin\'s pixels'),
    (r'_ZN3hvr\d+gconv3x3_', 0, 'gconv3x3.hip: a wave\'s weights stay in registers for its whole life, a spill would put them behind '
     'every tile\'s loads'),
    (r'_ZN3hvr\d+res2_conv3x3_', 0, 'res2.hip: a wave keeps two units\' accumulators and the loads of a whole tap in flight, a spill '
     'would sit inside the K loop'),
    (r'_ZN3hvr\d+gcb_pool_', 0, 'gcb.hip: a wave keeps acc[C / 64] and two pixels\' pieces in registers for its whole run, a spill '
     'would sit on the one pass over the map'),
    (r'_ZN3hvr\d+gn_stats_', 0, 'gn.hip: a lane keeps the running partials of its pieces and two steps\' loads in registers for its '
     'whole run, a spill would sit on the one pass over the map'),
    (r'_ZN3hvr\d+gn_apply_', 0, 'gn.hip: the apply keeps its channels\' mean, scale and shift in registers, a spill would sit on the '
     'one pass over the map'),
    (r'_ZN3hvr\d+gen_attn_', 0, 'gen_attn.hip: a wave keeps its queries, 16 scores and the d / 16 output accumulators in registers '
     'across the key loop, a spill would sit between the two MFMA chains'),
    (r'_ZN3hvr\d+focal_(?:elem|fused)_', 0, 'focal.hip: a lane keeps one 16-byte piece of logits and its results across three library '
     'calls per element, a spill would sit on the one pass over the logits'),
    (r'_ZN3hvr\d+(?:reg_elem|box_pair)_', 0, 'reg_loss.hip: a lane keeps 16-byte pieces of pred, target and weight and the four gradients of a box '
     'pair in registers, a spill would sit on the one pass over the inputs'),
    (r'_ZN3hvr\d+ghm_(?:hist|loss)_', 0, 'ghm.hip: two passes over the elements with a library call each, a spill would sit on the pass'),
    (r'_ZN3hvr\d+fpn_merge_', 0, 'fpn.hip, the top-down merge: a lane keeps the 16-byte pieces of its pixel\'s chain of up to four laterals in '
     'flight, a spill would sit on the one pass over the maps'),
    (r'_ZN3hvr\d+roi_align_levels_', 0, 'fpn.hip, RoIAlign behind the level select: the pipelined form keeps a bin\'s 16 corner vectors in flight, '
     'a spill would sit inside the gather chain the form exists to overlap'),
]

# The tile engine (gemm.hip, gemm_f16.hip) is gated by template arguments, not by name alone.  Kernels that use loads the compiler
# does not track keep the destination registers untouched until the hand-counted wait has passed; a register spill in such a kernel
# could store a destination before its load has landed.  Only VGPR spills are looked at here, not the scratch size.
TILE_KERNEL = r'_ZN3hvr11tile_kernelI(?:t|f|NS_5f16_tE|NS_6f16s_tE)Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)E'


def tile_has_untracked_loads(name):
    m = re.match(TILE_KERNEL, name)
    if not m:
        return False
    wm, wn, fm, fn, epi, glds, respre, ns = [int(x) for x in m.groups()]
    bn = wn * fn * 16
    # untracked: the pipelined relation apply pass (its block weights), and the pipelined residual kernels that prefetch the residual
    # tile, i.e. every RESPRE kernel with NS > 2 except the 144 x 256 shapes.
    # the split-half K-step keeps three fragment sets on the B side: its pipelined shapes are sized to fit without scratch traffic
    # in the loop (the 6-wave 144 x 256 ring does not and is never chosen for split operands, gemm.hip: choose_tile)
    split_pipe = 'f16s_t' in name and ns > 2 and not (wm == 3 and fn == 8)
    return epi == 2 or (ns > 2 and respre == 1 and bn != 256) or split_pipe


def rule_for(name):
    """(row, allowance) of the rule that gates the kernel `name`, or None.  Row len(RULES) is the tile engine's; its allowance is None."""
    for i, (pattern, allow, _) in enumerate(RULES):
        if re.match(pattern, name):
            return i, allow
    if tile_has_untracked_loads(name):
        return len(RULES), None
    return None


def main(*paths):
    bad, hits, per_unit = [], [0] * (len(RULES) + 1), []
    for p in paths:
        unit, seen = os.path.basename(p).split('.')[0], 0
        blocks = re.split(r'remark: (?:\S+ )?Function Name: ', open(p).read())[1:]   # (with -save-temps the remarks carry file:line:col)
        for b in blocks:
            name = b.split()[0]
            rule = rule_for(name)
            if rule is None:
                continue
            seen += 1
            hits[rule[0]] += 1
            spill = int(re.search(r'VGPRs Spill: (\d+)', b).group(1))
            scratch = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', b).group(1))
            allow = rule[1]
            if allow is None:
                if spill:
                    bad.append('%s: %d VGPRs spilled' % (name, spill))
            elif scratch > allow or (spill and not allow):
                bad.append('%s: %d VGPRs spilled, %d bytes of scratch' % (name, spill, scratch))
        per_unit.append((unit, seen, len(blocks)))
    if not sum(hits):
        sys.exit('check_regs: no kernel recognised in the remarks (format change?)')
    stale = [(RULES[i][0] if i < len(RULES) else TILE_KERNEL) for i, n in enumerate(hits) if not n]
    if stale:
        sys.exit('check_regs: these rules match no kernel of the build (stale):\n  ' + '\n  '.join(stale))
    if bad:
        sys.exit('check_regs: these kernels must not spill:\n  ' + '\n  '.join(bad))
    print('check_regs: kernels gated per unit: ' + ', '.join('%s %d of %d' % u for u in per_unit))
    print('check_regs: no rule gates any kernel of: ' + (' '.join(u for u, seen, _ in per_unit if not seen) or '(none)'))
    print('check_regs: %d kernels checked (untracked loads / serial sweeps / big accumulator tiles), none spills' % sum(hits))


if __name__ == '__main__':
    main(*sys.argv[1:])
