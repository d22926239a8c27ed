"""Two processes, one GPU: the validation pass's multi-rank branch (evaluation._gather_dev on the probability table, images and boxes; tally of
the concatenation in rank order; rank-0-only lines and grids), launched like tests/test_two_rank_gpu.py launches the training step."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_two_rank_gpu import _free_port  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(experiment, out_dir, world=2):
    env = dict(os.environ)
    for k in ("FD_DTYPE", "FAIRDIFF_LIB", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "run_two_rank_eval.py"), experiment, str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    for k in range(world):
        ep = os.path.join(out_dir, f"rank{k}.err")
        if os.path.exists(ep):
            print(f"---- rank {k} traceback\n" + open(ep).read()[-2500:])
    assert r.returncode == 0, f"{world}-rank validation failed"
    return [torch.load(os.path.join(out_dir, f"rank{k}.pt"), weights_only=False) for k in range(world)]


def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)


@pytest.mark.parametrize("experiment", ["exp-1", "exp-3"])
def test_two_ranks_tally_the_concatenation_in_rank_order(dev, tmp_path, experiment):
    from finetune_fair_diffusion_amd import evaluation as E
    from finetune_fair_diffusion_amd.fairness import EXPERIMENT_ATTRS
    import run_two_rank_eval as V
    r0, r1 = _launch(experiment, tmp_path)
    attrs = E.table_attrs(EXPERIMENT_ATTRS[experiment][1])
    assert not torch.equal(r0["tables"][0], r1["tables"][0])                  # each rank generated from its own noise
    for i in range(len(V.PROMPTS)):
        both = torch.cat([r0["tables"][i], r1["tables"][i]])                  # rank order, as customized_all_gather
        assert both.shape[0] == 2 * V.N_VAL and int((both != -1).all(dim=-1).sum()) > 0
        want = E.tally_host(both, attrs)
        assert torch.equal(r0["counts"][i], want), (r0["counts"][i].tolist(), want.tolist())
        assert torch.equal(r1["counts"][i], want)                             # every rank tallies the same gathered table
        assert _same(r0["metrics"]["main"][i], E.gap_metrics(experiment, want)) and _same(r0["main_again"][i], r0["metrics"]["main"][i])
        assert not torch.equal(want, E.tally_host(r0["tables"][i], attrs))    # ... which is not rank 0's own table
        assert torch.equal(r0["counts_ema"][i], want)                         # step 0: the EMA equals the live weights
    # rank 0 prints the lines and writes the grids of 2 x N_VAL gathered images; rank 1 prints nothing and writes no file
    assert [(json.loads(s)["eval"]) for s in r0["lines"]] == ["main", "EMA", "main"] and r1["lines"] == []
    want_files = sorted(f"eval_{n}_0_{p}_{t}.jpg" for n in ("main", "EMA") for p in V.PROMPTS for t in ("ori", "generated"))
    assert r0["files"] == want_files and r1["files"] is None
    from PIL import Image
    _, _, shape = E.grid_shape(2 * V.N_VAL, 256, 256)
    assert Image.open(tmp_path / "imgs_rank0" / want_files[0]).size == (shape[1], shape[0])
