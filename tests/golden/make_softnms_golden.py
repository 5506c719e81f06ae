"""Generates tests/golden/g20_soft_nms.npz by running the REFERENCE's own Soft-NMS (build container only; needs the reference tree at
make_golden.REF, oracle/_ref, Cython and a C compiler):

    python tests/golden/make_softnms_golden.py

The reference's mmdet/ops/nms/src/soft_nms_cpu.pyx is compiled WHERE IT LIES into a throw-away directory outside the repository
(cython -> C -> shared object), and mmdet/ops/nms/nms_wrapper.py and mmdet/core/post_processing/bbox_nms.py are loaded on top of the
stub packages of make_golden.py (`install_reference`, untouched), so the fixture holds what nms_wrapper.soft_nms and
multiclass_nms(type='soft_nms') themselves return.  Nothing of the reference is copied: the script executes it and stores arrays.
The Cython and numpy versions are recorded (the .pyx's arithmetic is a mix of f32 and f64 that the Cython version decides, and its
gaussian weight is numpy's exp).

Every case also passes through tests/softnms_refs.py, which must reproduce it bit for bit, and satisfies the margin conditions --
asserted here on the reference's numbers alone; a seed that fails one is replaced by the next, the seed used is stored:
  gaussian cases   no round whose winner and runner-up differ by 1 .. 8 f32 ulp, no rescored score within 8 ulp of min_score
                   (the device's f64 exp and numpy's may differ in the last bit; exact ties are well defined and kept);
  multiclass cases no two equal rescored scores among the entries the max_num sort orders (torch's sort is not stable).
"""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402  (pins the CPU numeric path on import)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import softnms_refs as R  # noqa: E402

SIZES = (1, 2, 7, 64, 65, 150, 300, 512)
PARAMS = [   # name, iou_thr, method, sigma, min_score
    ('lin_a', 0.3, 'linear', 0.5, 1e-3),
    ('lin_b', 0.5, 'linear', 0.5, 0.05),
    ('gau_a', 0.3, 'gaussian', 0.5, 1e-3),
    ('gau_b', 0.5, 'gaussian', 0.3, 0.05),
]
MC_CFGS = [   # name, nms_cfg as a config file would say it
    ('lin', dict(type='soft_nms', iou_thr=0.3)),                                                    # method / sigma / min_score: the defaults
    ('gau', dict(type='soft_nms', iou_thr=0.5, method='gaussian', sigma=0.3, min_score=0.05)),
]
MC_MAX_NUMS = (300, 100, -1)
SCORE_THR = 0.001
ULP_MARGIN = 8


def install_soft_nms(ref, workdir):
    """The compiled soft_nms_cpu + the reference's real nms_wrapper.py and bbox_nms.py on top of install_reference()'s stubs."""
    import Cython
    pyx = os.path.join(MG.REF, 'mmdet/ops/nms/src/soft_nms_cpu.pyx')
    c = os.path.join(workdir, 'soft_nms_cpu.c')
    subprocess.check_call([sys.executable, '-m', 'cython', pyx, '-o', c])
    so = os.path.join(workdir, 'soft_nms_cpu' + sysconfig.get_config_var('EXT_SUFFIX'))
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-w', '-I', sysconfig.get_paths()['include'], '-I', np.get_include(), c, '-o', so])
    spec = importlib.util.spec_from_file_location('mmdet.ops.nms.soft_nms_cpu', so)
    mod = importlib.util.module_from_spec(spec)
    sys.modules['mmdet.ops.nms.soft_nms_cpu'] = mod
    spec.loader.exec_module(mod)
    pkg = sys.modules['mmdet.ops.nms']
    pkg.__path__ = [os.path.join(MG.REF, 'mmdet/ops/nms')]
    pkg.soft_nms_cpu = mod
    sys.modules['mmdet.ops.nms.nms_cpu'] = pkg.nms_cpu = ref.nms_cpu
    sys.modules['mmdet.ops.nms.nms_cuda'] = pkg.nms_cuda = types.ModuleType('mmdet.ops.nms.nms_cuda')     # CUDA only: never called here
    wrapper = MG._load('mmdet.ops.nms.nms_wrapper', 'mmdet/ops/nms/nms_wrapper.py')
    pkg.nms_wrapper = wrapper
    bn = MG._load('mmdet.core.post_processing.bbox_nms', 'mmdet/core/post_processing/bbox_nms.py')
    return wrapper.soft_nms, bn.multiclass_nms, Cython.__version__


def gaussian_margins_ok(info):
    return info['min_gap_ulp'] > ULP_MARGIN and info['min_thr_ulp'] > ULP_MARGIN


def run_single(soft_nms, dets, prm):
    _, iou_thr, method, sigma, min_score = prm
    new, inds = soft_nms(dets.copy(), iou_thr, method=method, sigma=sigma, min_score=min_score)
    info = {}
    mine, mine_inds = R.soft_nms(dets, iou_thr, method, sigma, min_score, info=info)
    assert np.array_equal(inds, mine_inds) and np.array_equal(new.view(np.int32), mine.view(np.int32)), \
        'tests/softnms_refs.py does not restate soft_nms bit for bit'
    assert np.array_equal(new[:, :4], dets[inds, :4])
    return new, inds, info


def main():
    import warnings
    warnings.filterwarnings('ignore')
    torch.set_num_threads(MG.numerics.THREADS)
    ref = MG.install_reference()
    out = {}
    with tempfile.TemporaryDirectory(prefix='softnms_ref_') as workdir:
        soft_nms, multiclass_nms, cy_version = install_soft_nms(ref, workdir)
        out.update(cython_version=np.array(cy_version), numpy_version=np.array(np.__version__), ulp_margin=np.int32(ULP_MARGIN))
        # ---- the docstring case of nms_wrapper.soft_nms ----
        doc = np.array([[4., 3., 5., 3., 0.9], [4., 3., 5., 4., 0.9], [3., 1., 3., 1., 0.5], [3., 1., 3., 1., 0.5],
                        [3., 1., 3., 1., 0.4], [3., 1., 3., 1., 0.0]], dtype=np.float32)
        new, inds = soft_nms(doc.copy(), 0.7, sigma=0.5)
        assert len(inds) == len(new) == 3
        mine, mine_inds = R.soft_nms(doc, 0.7, sigma=0.5)
        assert np.array_equal(inds, mine_inds) and np.array_equal(new, mine)
        out.update(doc_dets=doc, doc_iou_thr=np.float64(0.7), doc_sigma=np.float64(0.5), doc_scores=new[:, 4], doc_inds=inds)
        # ---- single lists ----
        out['param_names'] = np.array([p[0] for p in PARAMS])
        for p in PARAMS:
            out['param_' + p[0]] = np.array([p[1], R.METHODS[p[2]], p[3], p[4]], np.float64)
        names = []
        for n in SIZES:
            for kind in ('cont', 'quant'):
                name = 'n%d_%s' % (n, kind)
                seed = 2000 + 37 * n + (1000 if kind == 'quant' else 0)
                while True:
                    dets = R.clustered_dets(seed, n, quantised=kind == 'quant')
                    res = [run_single(soft_nms, dets, p) for p in PARAMS]
                    if all(gaussian_margins_ok(r[2]) for p, r in zip(PARAMS, res) if p[2] == 'gaussian'):
                        break
                    print('g20 %s: seed %d breaks a gaussian margin, next' % (name, seed))
                    seed += 1
                names.append(name)
                out['sl_%s_seed' % name], out['sl_%s_dets' % name] = np.int64(seed), dets
                for p, (new, inds, info) in zip(PARAMS, res):
                    out['sl_%s_%s_scores' % (name, p[0])], out['sl_%s_%s_inds' % (name, p[0])] = new[:, 4], inds.astype(np.int32)
                print('g20 %s: seed %d, kept %s' % (name, seed, [r[1].size for r in res]))
        out['single_names'] = np.array(names)
        # ---- multiclass_nms(type='soft_nms') ----
        out['mc_cfg_names'] = np.array([c[0] for c in MC_CFGS])
        for cname, cfg in MC_CFGS:
            out['mc_cfg_' + cname] = np.array([cfg['iou_thr'], R.METHODS[cfg.get('method', 'linear')], cfg.get('sigma', 0.5),
                                               cfg.get('min_score', 1e-3)], np.float64)
        out.update(mc_max_nums=np.array(MC_MAX_NUMS, np.int32), mc_score_thr=np.float64(SCORE_THR), mc_names=np.array(['r300', 'r32', 'none']))
        for name, Rn in (('r300', 300), ('r32', 32), ('none', 32)):
            seed = 2600 + Rn
            while True:
                boxes = R.clustered_dets(seed, Rn)[:, :4]
                scores = R.class_scores(seed + 1, Rn, 31)
                if name == 'none':
                    scores = np.zeros_like(scores)
                    scores[:, 0] = 1
                assert np.unique(boxes, axis=0).shape[0] == Rn
                ok, res = True, {}
                for cname, cfg in MC_CFGS:
                    for mx in MC_MAX_NUMS:
                        db, dl = multiclass_nms(torch.from_numpy(boxes), torch.from_numpy(scores), SCORE_THR, MG.AttrDict(cfg), mx)
                        info = {}
                        md, ml = R.multiclass(boxes, scores, SCORE_THR, cfg, mx, info=info)
                        ok = ok and not info['cut_ties']
                        if cfg.get('method') == 'gaussian':
                            for c in range(1, 31):
                                sel = np.nonzero(scores[:, c] > np.float32(SCORE_THR))[0]
                                sub = {}
                                R.soft_nms(np.concatenate([boxes[sel], scores[sel, c:c + 1]], 1), cfg['iou_thr'], 'gaussian', cfg['sigma'],
                                           cfg['min_score'], info=sub)
                                ok = ok and (sel.size == 0 or gaussian_margins_ok(sub))
                        if ok:
                            assert np.array_equal(dl.numpy(), ml) and np.array_equal(db.numpy().view(np.int32), md.view(np.int32)), \
                                'tests/softnms_refs.py does not restate multiclass_nms bit for bit (%s %s %d)' % (name, cname, mx)
                        res[(cname, mx)] = (db.numpy(), dl.numpy(), info['rows'])
                if ok:
                    break
                print('g20 %s: seed %d breaks a margin, next' % (name, seed))
                seed += 1
            out['mc_%s_seed' % name], out['mc_%s_boxes' % name], out['mc_%s_scores' % name] = np.int64(seed), boxes, scores
            for (cname, mx), (db, dl, rows) in res.items():
                tag = 'mc_%s_%s_%s' % (name, cname, 'm1' if mx < 0 else str(mx))
                assert np.array_equal(db[:, :4], boxes[rows])
                out[tag + '_scores'], out[tag + '_labels'], out[tag + '_rows'] = db[:, 4], dl.astype(np.int16), rows.astype(np.int16)
                print('g20 %s %s max_num %d: seed %d, %d detections' % (name, cname, mx, seed, db.shape[0]))
    MG.save('g20_soft_nms', **out)


if __name__ == '__main__':
    main()
