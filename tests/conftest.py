import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def usable_cpus():
    """min(affinity, cgroup CPU quota): the GPU box exposes 256 logical CPUs under a 16-CPU quota, and a
    256-thread torch pool under that quota is ~200x slower than a 16-thread one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (IOError, OSError, ValueError):
        pass
    return max(1, n)


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu on the GPU box)')
    import torch
    if not torch.cuda.is_available():
        # without a GPU: the CPU numeric path the golden vectors were recorded on (tests/golden/numerics.py), set before torch
        # runs its first CPU kernel.  With a GPU the host keeps torch's own paths, on which the GPU tests' comparisons with the
        # oracle evaluated live on the host were settled (pinned, five of them move across their bars); the device's results
        # meet the recordings within tolerances either way.  So on a GPU host the CPU-only golden tests (test_oracle_golden.py)
        # are not guaranteed to match bit for bit: a CPU that rounds differently from the recording one fails the exact ones.
        from tests.golden import numerics
        numerics.pin()
    torch.set_num_threads(usable_cpus())


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason='no GPU in this container')
    for item in items:
        if 'gpu' in item.keywords:
            item.add_marker(skip)
