"""Inputs and references of the aligned-chip kernel checks (``fd_warp_affine_u8_fwd``), shared by tests/test_kernels_facealign_gpu.py (fp16 library) and
tests/run_bf16_facealign_checks.py (bf16 library).  Everything here is host work and is computed once per process."""
import functools
import math

import numpy as np
import torch

from finetune_fair_diffusion_amd import evaluate_images as EI
from finetune_fair_diffusion_amd.fairness import alignment_sampling_matrix
from oracle import nn_sfnet as OS


def face(rng, size, angle, centre, jitter=0.5):
    """Five landmarks: the template scaled to ``size`` pixels, rotated by ``angle`` about its middle, moved to ``centre`` (x, y) and jittered."""
    p = (OS.SRC_LANDMARKS - 56.0) / 112 * size
    c, s = math.cos(angle), math.sin(angle)
    return p @ np.array([[c, s], [-s, c]]) + np.array(centre) + rng.randn(5, 2) * jitter


def _matrices(lms, H, W, S):
    return torch.tensor(np.stack([alignment_sampling_matrix(l, H, W, S) for l in lms]), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def small_case(S=28, reference=True):
    """Two 48x64 images of random bytes, four chips: two of image 0, one of image 1 spilling over the top-right corner, one of image 1 minified 4.3 times
    (a face of 120 pixels on a 28-pixel chip, larger than the image).  -> (u8 [2,48,64,3], src [4], A [4,6] fp32, S, fp64 host statement as fp32 or None)"""
    H, W = 48, 64
    rng = np.random.RandomState(7)
    u8 = torch.from_numpy(rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8))
    lms = [face(rng, 30, 0.3, (32, 24)), face(rng, 20, -0.5, (20, 30)), face(rng, 36, 1.2, (60, 5)), face(rng, 120, 0.2, (32, 24))]
    src = [0, 0, 1, 1]
    A = _matrices(lms, H, W, S)
    ref = torch.from_numpy(EI.warp_affine_u8_host(u8.numpy(), src, A.numpy(), S, -1.0)).float() if reference else None
    return u8, src, A, S, ref


@functools.lru_cache(maxsize=None)
def production_case(reference=True):
    """Two 512^2 images to 112^2 chips through the three faces of ``test_warp_affine_production_size`` (the last spills over the corner), the reference
    being the oracle's image pipeline on ``u/255*2-1``."""
    B, H, W, S = 2, 512, 512, 112
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    rng = np.random.RandomState(3)
    lms = [face(rng, 120, 0.3, (200, 220)), face(rng, 260, -0.6, (300, 330)), face(rng, 180, 1.2, (470, 60))]
    src = [0, 0, 1]
    ref = None
    if reference:
        x = u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1
        ref = torch.stack([OS.image_pipeline(x[src[i]], lms[i], S) for i in range(3)])
    return u8, src, _matrices(lms, H, W, S), S, ref


def exact_case(dtype):
    """One 16x16 image; the identity map and the translation by (+3, -2) at S = 16.  -> (u8, A [2,6], the two expected chips in ``dtype``)"""
    u8 = torch.randint(0, 256, (1, 16, 16, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    A = torch.tensor([[1, 0, 0, 0, 1, 0], [1, 0, 3, 0, 1, -2]], dtype=torch.float32)
    x = (u8.float() / 255 * 2 - 1).permute(0, 3, 1, 2)[0]
    shifted = torch.full_like(x, -1.0)
    shifted[:, 2:, :13] = x[:, :14, 3:]
    return u8, A, x.to(dtype).contiguous(), shifted.to(dtype).contiguous()
