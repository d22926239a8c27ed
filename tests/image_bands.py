"""Margins of the per-tensor gates of the image-side networks (tests/image_refs.py has the rule, tests/test_image_refs_cpu.py recomputes them,
tests/test_image_blocks_gpu.py applies them).

A product tensor T passes when  e2_prod(T) <= MARGIN_E2 x max_v e2_emul_v(T)  and  emax_prod(T) <= MARGIN_MAX x max_v emax_emul_v(T),  v over the emulation
variants a, c, e of image_refs.py, every statistic taken against the fp64 reference under the candidate's own activation branches.  Each margin is 1.25 x the
largest ratio, per statistic, between a variant and variant a (either way round) over every arm and tensor -- the rule of block_bands.py -- rounded up with 2 %
of room (the emulations' fp32 convolutions and matmuls sum in an order that depends on the host's thread count).  Computed from the emulations alone; nothing
measured on the product enters.

Largest ratio per arm, with the tensor and variant it occurred on (CPU, 16 threads):
      arm       e2                                   emax
      B0        1.334  out                    c        1.655  out                    e
      B1        1.064  out                    e        1.541  dx                     e
      B2        1.342  out                    c        1.985  out                    e
      B3        1.269  z1                     c        1.571  out                    e
      B4        1.532  out                    c        2.532  out                    c
      B6        1.054  dx                     e        1.401  out                    e
      B7        1.187  out                    c        1.828  out                    c
      B10       1.210  z1                     c        1.522  z1                     c
      B11       1.320  out                    c        1.609  out                    c
      B12       1.154  z1                     c        1.305  z1                     c
      B13       1.380  out                    c        1.574  dx                     c
      B12x10    1.217  z1                     c        1.224  z1                     e
      S_stem    1.071  dx                     e        1.103  dx                     e
      S_down7   1.017  y                      e        1.129  dx                     e
      S_down6   1.030  y                      e        1.158  y                      e
      S_block3  2.126  dx                     c        2.541  dx                     c
      S_block6  1.770  dx                     c        1.598  dx                     c
      SH        1.209  zf                     c        1.411  logits                 e
      VA64      2.281  out                    c        2.483  out                    c
      VA40      2.149  out                    c        2.186  out                    c
      VR_same   1.361  out                    c        1.867  out                    c
      VR_short  1.234  out                    c        1.382  out                    c
      VU        1.009  out                    e        1.272  dx                     e
      VH        1.068  dx                     e        1.362  dx                     e
      VT        1.145  out                    e        1.294  out                    e
  largest: e2 2.281 -> 1.25 x = 2.851 -> MARGIN_E2 2.91;  emax 2.541 -> 1.25 x = 3.176 -> MARGIN_MAX 3.24
The largest ratios sit where a residual sum is dominated by its exact term (the attention's  out = x + o,  a residual block's  dx = ds + conv1^T dh): variant a
leaves the sum unrounded, so its error is that of the small term alone, and variant c rounds the sum as the GEMM epilogue does -- one more fp16 rounding of the
whole tensor.  With these margins the bands of the block arms are 5e-4 .. 3e-3, against the whole-network tests' 5e-2 .. 2.5e-1.

The whole networks (arms CLF, SF, VAE, CLIP, DINO) have margins of their own by the same rule over their own emulations:
      CLF       1.610  z.b4.z1                c        1.961  z.b14.z_dw             e
      SF        1.150  z.v1.l3.b1.h           e        2.005  z.v2.l3.b3.y           e
      VAE       1.207  dz                     e        1.585  img                    e
      CLIP      1.624  cls                    c        2.116  cls                    c
      DINO      2.322  h1.2                   c        3.583  cls                    c
  largest: e2 2.322 -> 1.25 x = 2.903 -> MARGIN_E2_NET 2.96;  emax 3.583 -> 1.25 x = 4.479 -> MARGIN_MAX_NET 4.57
(the emax ratio comes from the ViTs' last class-token rows, 384 elements: a tail sampled on few elements)
The emulations' e2 there: classifier logits 2e-3, dchips and the fifteen trace entries 6e-3 .. 1.2e-2 (bands 1.8e-2 .. 3.6e-2); SFNet-20 features 5.5e-4,
dchips 8.6e-4; VAE image 1.7e-3, dz 2.2e-3; ViT embeddings 7e-4 .. 1e-3, dchips 1.3e-3 .. 1.6e-3, h1 / h2 4e-4 .. 8e-4.

No band exceeds CAP_FWD = 2e-2 (forward tensors) or CAP_GRAD = 5e-2 (gradients); where margin x emulation would, the band is the cap (``CAPPED``: (arm, tensor)),
and the emulation alone must clear the cap by a factor of two (test_caps_hold_and_name_the_capped_tensors).  That happens in emax alone, on the classifier's
gradient at the chips and at the inputs of blocks 0 .. 12 (emulation emax 1.0e-2 .. 1.6e-2 x 4.57; which of them pass 5e-2 moves with the host's summation order, so
``CAPPED`` lists them all and the test asks for a subset) and on the VAE's clamped image (emulation emax 6.8e-3 x 4.57 = 3.1e-2 against 2e-2)."""
MARGIN_E2 = 2.91
MARGIN_MAX = 3.24
MARGIN_E2_NET = 2.96
MARGIN_MAX_NET = 4.57
CAPPED = tuple(("CLF", f"trace{i}") for i in range(13)) + (("CLF", "dchips"), ("VAE", "img"))
