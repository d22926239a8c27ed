"""The bf16 library kernel by kernel (GPU): tests/run_bf16_kernel_checks.py holds the checks and runs in its own process, because a process's working dtype
-- which library it loads -- is fixed at import.  One fresh child per group, one at a time, each under its own time limit (import and device start-up
dominate it); a child that crashes or runs out of time is never started again: the test fails with the tail of its output."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = dict(gemm=150, conv=150, attention=150, norm_elementwise=120, bitexact=120, small_classifier_eval=120)      # seconds


def _run(group):
    env = dict(os.environ, FD_DTYPE="bf16")
    env.pop("FAIRDIFF_LIB", None)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "run_bf16_kernel_checks.py"), group], env=env, capture_output=True, text=True, timeout=TIMEOUT[group])
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(out[-6000:])
        pytest.fail(f"group {group} did not finish in {TIMEOUT[group]} s (not retried)")
    print(r.stdout[-12000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, f"group {group}: exit code {r.returncode} (not retried)"
    assert f"BF16 KERNEL CHECKS PASSED {group}" in r.stdout


@pytest.mark.parametrize("group", list(TIMEOUT))
def test_bf16_kernels(dev, group):
    _run(group)
