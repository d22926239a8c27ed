"""One rank of a two-process run of a ``--experiment custom`` step that restates exp-3 (gender x race, Monte-Carlo transport targets): launched by
tests/test_two_rank_custom_gpu.py through ``python -m torch.distributed.run --nproc-per-node 2`` with the gloo backend, both ranks sharing cuda:0, as
tests/run_two_rank_step.py does for the named experiments.  Writes the step's targets and the gathered probability table every rank derived them
from to ``<out>/rank<k>.pt``."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import custom_cases as C  # noqa: E402
import util_models as U  # noqa: E402

B_PER_RANK, NOISE_SEED = 3, 4242


def global_noises(world):
    return torch.randn(world * B_PER_RANK, 4, 32, 32, generator=torch.Generator().manual_seed(NOISE_SEED))


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = C.build(dev, custom=C.RESTATED["exp-3"], rank=rank, world=world, batch=B_PER_RANK)
    assert tr.collectives and tr.spec.custom and tr.spec.solver == "mc"
    gathered = []
    gather = tr.gather_probs
    tr.gather_probs = lambda p: gathered.append(gather(p)) or gathered[-1]
    out = tr.train_step(U.tiny_tokens(), global_noises(world)[rank * B_PER_RANK:(rank + 1) * B_PER_RANK], C.S)
    torch.cuda.synchronize()
    torch.save(dict(targets={k: v.clone() for k, v in out["targets_by_attr"].items()}, gathered=gathered[0].clone(), finite=out["grad_is_finite"],
                    grads=[b.grad.detach().cpu().clone() for b in tr.banks], params=[b.flat.detach().cpu().clone() for b in tr.banks]),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        import traceback
        with open(os.path.join(sys.argv[1], f"rank{os.environ.get('RANK', '0')}.err"), "w") as f:     # the launcher's own traceback hides the child's
            traceback.print_exc(file=f)
        raise
