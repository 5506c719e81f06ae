"""bench.py --dump-outputs (CPU): the file layout two builds are compared by -- one file per clip of the last call and branch of
the head, float32 [n, 6] = x1, y1, x2, y2, score, class index, rows in class order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _classes(seed, n_classes=30):
    """per-class [k, 5] float32 arrays as bbox2result returns them, some classes empty"""
    rng = np.random.RandomState(seed)
    return [rng.rand(int(k), 5).astype(np.float32) * 100 for k in rng.randint(0, 4, n_classes)]


def _expect(br):
    return np.concatenate([np.concatenate([a, np.full((len(a), 1), c, np.float32)], 1) for c, a in enumerate(br)], 0)


def test_hvr_result_is_one_file_per_clip_and_branch(tmp_path):
    clips = [[_classes(10 * w + b) for b in range(2)] for w in range(3)]   # HVR: a list of test branches per clip
    bench.dump_outputs(str(tmp_path), clips, 'hvr')
    assert sorted(os.listdir(tmp_path)) == ['clip%d_branch%d.npy' % (w, b) for w in range(3) for b in range(2)]
    for w in range(3):
        for b in range(2):
            got = np.load(os.path.join(tmp_path, 'clip%d_branch%d.npy' % (w, b)))
            assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 6
            np.testing.assert_array_equal(got, _expect(clips[w][b]))
            assert np.all(np.diff(got[:, 5]) >= 0)   # class index column, rows in class order


def test_selsa_result_is_one_branch(tmp_path):
    clips = [_classes(7)]                                                   # SELSA: the per-class list itself
    bench.dump_outputs(str(tmp_path), clips, 'selsa')
    assert os.listdir(tmp_path) == ['clip0_branch0.npy']
    got = np.load(os.path.join(tmp_path, 'clip0_branch0.npy'))
    assert got.dtype == np.float32 and got.shape == (sum(len(a) for a in clips[0]), 6)
    np.testing.assert_array_equal(got, _expect(clips[0]))


def test_no_detections_is_an_empty_n_by_6_array(tmp_path):
    bench.dump_outputs(str(tmp_path), [[np.zeros((0, 5), np.float32) for _ in range(30)]], 'selsa')
    got = np.load(os.path.join(tmp_path, 'clip0_branch0.npy'))
    assert got.dtype == np.float32 and got.shape == (0, 6)
