"""One rank of a two-process validation pass: launched by tests/test_two_rank_eval_gpu.py through ``python -m torch.distributed.run`` with the gloo
backend, both ranks sharing cuda:0, exactly as tests/run_two_rank_step.py runs the training step.  Each rank evaluates the same two prompts on
its OWN validation noise (``evaluation.evaluation_step``, grids on); the probability tables, images and boxes are gathered in rank order, every
rank tallies the concatenation and only rank 0 prints lines and writes files.  Writes what the parent compares to ``<out>/rank<k>.pt``."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import util_models as U  # noqa: E402
import run_two_rank_step as R  # noqa: E402

N_VAL, PROMPTS = 5, ["a", "b"]


def val_noises(rank):
    return torch.randn(len(PROMPTS), N_VAL, 4, 32, 32, generator=torch.Generator().manual_seed(7100 + rank))


def local_tables(tr, noises):
    """This rank's own probability tables for the live weights, per prompt (the networks are deterministic: the same images as in the pass)."""
    from finetune_fair_diffusion_amd import evaluation as E
    return [E.probability_table(tr, tr.classify_begin(E._generate(tr, tr.te, tr.unet, U.tiny_tokens(), n.to(tr.device)))).cpu() for n in noises]


def main():
    from finetune_fair_diffusion_amd import evaluation as E
    experiment, out_dir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = R.build(experiment, dev, rank, world)
    tr.args.val_GPU_batch_size = 4
    assert tr.collectives
    noises = val_noises(rank)
    lines = []
    imgs_dir = os.path.join(out_dir, f"imgs_rank{rank}")
    out = E.evaluation_step(tr, lambda p: U.tiny_tokens(), PROMPTS, 0, noises_val=noises, mode="grids", imgs_dir=imgs_dir, log=lines.append)
    counts_ema = [c.clone() for c in tr.last_eval_counts]
    main_logs = E.evaluate_process(tr, "main", "main", [(p, U.tiny_tokens()) for p in PROMPTS], noises, 0, log=lines.append)
    torch.cuda.synchronize()
    torch.save(dict(metrics=out, main_again=main_logs, counts=[c.clone() for c in tr.last_eval_counts], counts_ema=counts_ema, lines=lines,
                    files=sorted(os.listdir(imgs_dir)) if os.path.isdir(imgs_dir) else None, tables=local_tables(tr, noises)),
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
