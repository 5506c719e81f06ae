"""One CPU numeric path for the golden vectors and for the tests that compare the CPU oracle against them.

Torch's CPU kernels pick their code at run time: ATen's vectorised kernels by the widest instruction set the CPU
offers, MKL's BLAS and vector math (exp, ...) by instruction set and CPU vendor, and how a product or a reduction is
split depends on the thread count.  Two CPUs therefore round the same float32 expression differently in the last
bit, and a fixture recorded on one CPU does not replay bit for bit on another.  make_golden.py records on the path
below -- AVX2 for ATen and oneDNN, MKL's conditional numerical reproducibility branch that every x86-64 CPU runs,
THREADS threads -- and the tests that replay those fixtures on the CPU run on the same path (tests/conftest.py,
tests/test_oracle_golden.py).  The variables are read when torch first runs a CPU kernel, so pin() runs before that."""
import os

CPU_PATH = {'ATEN_CPU_CAPABILITY': 'avx2', 'MKL_CBWR': 'COMPATIBLE,STRICT', 'ONEDNN_MAX_CPU_ISA': 'AVX2'}
THREADS = 8


def pin():
    os.environ.update(CPU_PATH)
