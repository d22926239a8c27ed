"""Two processes, one GPU, a ``--experiment custom`` step that restates exp-3 (tests/run_two_rank_custom.py): both ranks derive their targets from
one global plan, and rank 0's slice is the single-process host statement on the gathered probabilities."""
import os
import socket
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import custom_cases as C  # noqa: E402
import run_two_rank_custom as R  # noqa: E402

pytestmark = pytest.mark.gpu
TIMEOUT = 300      # seconds, for the launcher and its two children together


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_custom_as_exp3(dev, tmp_path):
    from finetune_fair_diffusion_amd import fairness as FA
    env = dict(os.environ)
    for k in ("FD_DTYPE", "FAIRDIFF_LIB", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "run_two_rank_custom.py"), str(tmp_path)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the two-rank run did not finish in {TIMEOUT} s (not retried)")
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    for k in range(2):
        ep = os.path.join(tmp_path, f"rank{k}.err")
        if os.path.exists(ep):
            print(f"---- rank {k} traceback\n" + open(ep).read()[-2500:])
    assert r.returncode == 0, "two-rank run failed (not retried)"
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{k}.pt")) for k in range(2))
    assert r0["finite"] and r1["finite"] and set(r0["targets"]) == {"gender", "race"}
    for a, b in zip(r0["grads"] + r0["params"], r1["grads"] + r1["params"]):
        assert torch.equal(a, b)
    # both ranks saw the same gathered table, [world * B, 2 + 4] in rank order
    assert r0["gathered"].shape == (2 * R.B_PER_RANK, 6) and torch.equal(r0["gathered"], r1["gathered"])
    # the host statement: each rank's 100 draws on its own stream (1234 + rank), the plans summed, the targets of the global batch
    spec = FA.experiment_spec("custom", C.U.make_args(**C.RESTATED["exp-3"]))
    table = r0["gathered"]
    probs = [table[:, :2].contiguous(), table[:, 2:6].contiguous()]
    plans = [FA.mc_transport_plan(probs, spec.class_cdfs, 100, torch.Generator().manual_seed(1234 + k), spec.asymmetric_last) for k in range(2)]
    idx, sizes = plans[0][0], plans[0][2]
    res = FA.targets_from_plan(idx, plans[0][1] + plans[1][1], sizes)
    for (name, _, _), (t, u) in zip(spec.attrs, res):
        t = t.clone()
        t[u > C.THRESHOLD] = -1
        got = torch.cat([r0["targets"][name], r1["targets"][name]])
        print(name, "two ranks", got.tolist(), "host", t.tolist())
        assert torch.equal(got, t), name
        assert torch.equal(r0["targets"][name], t[:R.B_PER_RANK])
    assert sum(int((v != -1).sum()) for v in r0["targets"].values()) >= 1
