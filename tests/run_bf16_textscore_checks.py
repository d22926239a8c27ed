"""The CLIP text-image score on the bf16 library (libfairdiff_hip_bf16.so, FD_DTYPE=bf16) -- run as a SCRIPT in its own process, because a process's
working dtype is fixed at import; tests/test_textscore_bf16_gpu.py starts it once:

    FD_DTYPE=bf16 python tests/run_bf16_textscore_checks.py

The cases of tests/textscore_cases.py: ``text_embeds`` against the fp64 statement, ids behind the end-of-text token (bit-equal, as in fp16), and the
evaluator on the trees against the oracle image encoder and the statement.  Bands are 8 x the fp16 ones (8 = the ratio of the unit roundoffs: three
fewer mantissa bits, the rule of tests/run_bf16_facealign_checks.py).  Every check prints its figure; failures are collected, printed, and the exit
code is non-zero, or the last line is ``BF16 TEXTSCORE CHECKS PASSED``."""
import math
import os
import pickle
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
BF = torch.bfloat16
FAILED = []


def expect(name, ok, detail=""):
    print(f"[{name}] {'ok' if ok else 'FAILED'} {detail}")
    if not ok:
        FAILED.append(name)


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from finetune_fair_diffusion_amd import evaluate_images as EI, lib, ops
    from finetune_fair_diffusion_amd.factory import TINY
    from finetune_fair_diffusion_amd.text_encoder import CLIPTextModel
    import textscore_cases as C
    import textscore_refs as R
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == BF
    cfg = TINY["clip_text_h"]
    band_embeds, band_oracle = 8 * C.BAND_EMBEDS, 8 * C.BAND_ORACLE

    tower = CLIPTextModel(cfg, EI.synthetic_text_state(TINY), dev)
    rows = R.rows_with_eot_at(C.EOT_AT, cfg.vocab_size)
    ref = C.text_reference(EI, TINY, rows)
    got = tower.text_embeds(rows)
    expect("dtype and shape", got.dtype == BF and tuple(got.shape) == (4, cfg.projection_dim))
    got = got.float().cpu()
    e = float((got.double() - ref).abs().max() / ref.abs().max())
    expect("text_embeds vs fp64 statement", math.isfinite(e) and e <= band_embeds, f"rel max err {e:.3e} (band {band_embeds:.1e})")
    tail = tower.text_embeds(R.rows_with_eot_at(C.EOT_AT, cfg.vocab_size, tail="random")).float().cpu()
    expect("ids behind the end-of-text token: bit-equal", torch.equal(tail, got))
    one = torch.cat([tower.text_embeds(rows[r:r + 1]).float().cpu() for r in range(4)])
    e = float((one - got).abs().max() / got.abs().max())
    expect("one row at a time vs the batch of four", math.isfinite(e) and e <= 8 * C.BAND_LAUNCH_FORM, f"rel max diff {e:.3e} (band {8 * C.BAND_LAUNCH_FORM:.1e})")

    with tempfile.TemporaryDirectory() as root:
        gen, _, prompts, u8_gen, _ = C.build_trees(root)
        own, other = C.own_and_other(C.score_reference(EI, TINY, u8_gen))
        moved = float((own - other).abs().max())
        # the bf16 band is wider than the fp16 one; the separation of the reference is stated against it as well
        expect("the reference separates the prompts", moved >= C.SEPARATION and moved > band_oracle, f"{moved:.3f} (band {band_oracle:.1e})")
        out = os.path.join(root, "out")
        C.run(EI, TINY, gen, out, 4, prompts=prompts)
        with open(os.path.join(out, "text_alignment.pkl"), "rb") as f:
            sims = pickle.load(f)
        s = torch.cat([sims[0][0], sims[0][1]]).double()
        e = float((s - own).abs().max())
        expect("sim_clip_text vs oracle", bool(torch.isfinite(s).all()) and e <= band_oracle,
               f"max abs err {e:.3e} (band {band_oracle:.1e}); against the other prompt's text {float((s - other).abs().max()):.3e}")
        expect("no originals: the second dict is empty", sims[1] == {})
        out1 = os.path.join(root, "out1")
        C.run(EI, TINY, gen, out1, 1, prompts=prompts)
        with open(os.path.join(out1, "text_alignment.pkl"), "rb") as f:
            sims1 = pickle.load(f)
        e = float((torch.cat([sims1[0][0], sims1[0][1]]).double() - s).abs().max())
        expect("batch size 1 vs 4", math.isfinite(e) and e <= 8 * C.BAND_LAUNCH_FORM, f"max abs diff {e:.3e} (band {8 * C.BAND_LAUNCH_FORM:.1e})")

    torch.cuda.synchronize()
    if FAILED:
        print("FAILED:", FAILED)
        sys.exit(1)
    print("BF16 TEXTSCORE CHECKS PASSED")


if __name__ == "__main__":
    main()
