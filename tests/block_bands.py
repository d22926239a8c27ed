"""Margins of the per-tensor block gates (tests/block_refs.py has the rule, tests/test_block_refs_cpu.py recomputes them, tests/test_blocks_gpu.py applies them).

A product tensor T passes when  e2_prod(T) <= MARGIN_E2 x max_v e2_emul_v(T)  and  emax_prod(T) <= MARGIN_MAX x max_v emax_emul_v(T),  v over the emulation
variants a .. e of block_refs.py.  Each margin is 1.25 x the largest ratio, per statistic, between a variant and variant a (either way round) over every arm
and tensor -- the rule of kernel_bands.py's C_MARGIN_* -- rounded up with 2 % of room (the emulations' fp32 matmuls sum in an order that depends on the
host's thread count).  Computed from the emulations alone; nothing measured on the product enters.

Largest ratio per arm, with the tensor and variant it occurred on (CPU, 8 threads):
      arm   e2                                   emax
      T1    1.441  attn2.to_v.down      c        1.878  h2                 b
      T3    1.463  attn2.to_out.down    c        1.590  attn2.to_out.down  c
      T4    1.412  out                  c        2.001  h2                 c
      T5    1.398  out                  c        1.711  h2                 c
      T6    1.431  out                  c        1.658  attn1.to_out.down  e
      T7    1.427  out                  c        1.696  attn2.to_out.down  e
      T9    1.494  attn2.to_v.down      c        1.878  h2@0               b
      T10   1.446  out@1                c        2.132  h2@1               c
      R1    1.024  out                  e        1.135  out                e
      R2    1.003  dx                   e        1.052  dx                 e
      R3    1.009  out                  e        1.317  dskip              e
      R4    1.006  dx                   e        1.312  dx                 e
      R5    1.026  dx                   e        1.079  out                e
  largest: e2 1.494 -> 1.25 x = 1.868 -> MARGIN_E2 1.90;  emax 2.132 -> 1.25 x = 2.665 -> MARGIN_MAX 2.72
The e2 ratios are set by variant c (the roundings the kernels state between leaf modules, on top of the leaf roundings); emax is a sample of a tail over
~10^4 .. 10^5 elements and moves that much from one set of rounding sites to another.  With these margins the bands of the block arms are 6e-4 .. 5e-3, against engine-level tolerances of 2e-2 (forward) and 5e-2 (gradients).

The whole U-Net (arm U of block_refs.py: eps and the 96 LoRA gradients of the "d40" model, e2 alone) has a margin of its own by the same rule over its own
emulations: a gradient that has crossed six transformer and eight ResNet blocks differs more from one set of rounding sites to another than a block's does.
      U     2.563  up_blocks.1.attentions.2.transformer_blocks.0.attn2.processor.to_q_lora.down.weight  b   -> 1.25 x = 3.204 -> MARGIN_E2_NET 3.27
The emulations' e2 there are 1e-3 (eps) and 1e-3 .. 1.8e-2 (LoRA gradients).  On four tensors -- attn1 to_q / to_k down of the mid block and two up blocks -- margin x
emulation would pass 5e-2; seeds 0, 2, 4, 6, 8 and gradient scales 2^10, 2^14, 2^17 all leave some tensor there, so those bands are the cap itself."""
MARGIN_E2 = 1.90
MARGIN_MAX = 2.72
MARGIN_E2_NET = 3.27
