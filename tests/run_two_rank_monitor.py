"""One rank of a two-process training step with the training monitor on: launched by tests/test_trainplots_gpu.py through
``python -m torch.distributed.run`` with the gloo backend, both ranks sharing cuda:0, exactly as tests/run_two_rank_step.py runs the plain step.
The step is a plot step: probability tables, images and boxes of both sides are gathered in rank order on every rank, every rank tallies the
gathered table and only rank 0 paints.  Writes what the parent compares to ``<out>/rank<k>.pt``."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import util_models as U  # noqa: E402
import run_two_rank_step as R  # noqa: E402


def main():
    from finetune_fair_diffusion_amd import evaluation as E
    experiment, out_dir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = R.build(experiment, dev, rank, world)
    assert tr.collectives
    tr.monitor, tr.monitor_plot = "plots", True
    noises = R.global_noises(world)[rank * R.B_PER_RANK:(rank + 1) * R.B_PER_RANK]
    out = tr.train_step(U.tiny_tokens(), noises, R.S)
    torch.cuda.synchronize()
    mon = tr.last_monitor
    own = {tag: E.probability_table(tr, tr.classify_begin(out[key])).cpu() for tag, key in (("generated", "images"), ("ori", "images_ori"))}
    torch.save(dict(counts=mon["counts"].clone(), grids={k: v.clone() for k, v in mon["grids"].items()}, own_tables=own,
                    own_images={"generated": out["images"].cpu(), "ori": out["images_ori"].cpu()},
                    tables={k: v.cpu() for k, v in mon["tables"].items()}, images={k: v.cpu() for k, v in mon["images"].items()},
                    boxes={k: v.cpu() for k, v in mon["boxes"].items()}, loss_fair=out["loss_fair"].clone()),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        import traceback
        with open(os.path.join(sys.argv[2], f"rank{os.environ.get('RANK', '0')}.err"), "w") as f:     # the launcher's own traceback hides the child's
            traceback.print_exc(file=f)
        raise
