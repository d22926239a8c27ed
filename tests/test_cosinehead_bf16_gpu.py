"""The cosine-logit kernels and the zero-shot classifier on the bf16 library (GPU): tests/run_bf16_cosinehead_checks.py holds the checks and runs once in
a fresh child process with FD_DTYPE=bf16 (a process's working dtype is fixed at import), under its own time limit (import and device start-up dominate
it); a child that crashes or runs out of time is never started again: the test fails with the tail of its output."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120      # seconds


def test_bf16_cosine_head(dev):
    env = dict(os.environ, FD_DTYPE="bf16")
    env.pop("FAIRDIFF_LIB", None)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "run_bf16_cosinehead_checks.py")], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(out[-6000:])
        pytest.fail(f"the bf16 checks did not finish in {TIMEOUT} s (not retried)")
    print(r.stdout[-12000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, f"exit code {r.returncode} (not retried)"
    assert "BF16 COSINE HEAD CHECKS PASSED" in r.stdout
