"""Inputs, references and the error bound of the ``fd_bank_norms`` checks, shared by tests/test_kernels_banknorms_gpu.py (fp16 library),
tests/run_bf16_banknorms_checks.py (bf16 library, own process) and tests/test_trainnorms_gpu.py.

The bound follows from the accumulation scheme (include/fairdiff_hip.h), with u = 2^-24 the unit roundoff of fp32 and n = CH / WG = 8192 / 256 = 32 the
most squares one thread sums:

  * a thread's fp32 sum of n squares: every term is >= 0, each square and each addition rounds once at the most (a fused multiply-add rounds once for
    both), so the sum carries a relative error of at most (1 + u)^(n+1) - 1 < (n + 2) u;
  * lanes (6 butterfly additions), waves (3 additions) and the chunks of a tensor (K - 1 additions; K <= 2^11 chunks here, all of a bank for its global norm) are added
    in fp64, as is the square root: less than (K + 10) 2^-53 < 2^-41 together;
  * the square root halves a relative error e up to a term e^2 / 2: (n + 2) u / 2 = 17 u, and (34 u)^2 / 2 < 2^-38.8;
  * the fp32 store rounds once more: u, and the cross term 17 u * u < 2^-43.

Hence |got - ref| <= BOUND * ref with BOUND = (n + 2) / 2 * u + u + 2^-38 = 18 * 2^-24 + 2^-38 for a per-tensor norm and for the global L2 norm (the same
sums over more chunks).  The mean is the fp64 mean of those fp32 norms -- no error of its own beyond 2^-53 per addition -- rounded once to fp32:
MEAN_BOUND = BOUND + u + 2^-40 against the mean of the reference norms.  The reference is ``torch.linalg.vector_norm`` of the same fp32 values in fp64
(its own error, ~ 2^-50, is inside the 2^-38 term's slack: 2^-38 - 2^-38.8 - 2^-41 - 2^-43 > 2^-40)."""
import numpy as np
import torch

CH, WG = 8192, 256
U = 2.0 ** -24
BOUND = (CH // WG + 2) / 2 * U + U + 2.0 ** -38
MEAN_BOUND = BOUND + U + 2.0 ** -40
SENTINEL = 12345.0
HAND_MADE = {"t1": (1,), "t3": (3,), "t_ch_minus_1": (CH - 1,), "t_ch": (CH,), "t_ch_plus_1": (CH + 1,), "t_2ch_plus_5": (2 * CH + 5,),
             "w1280x50": (1280, 50), "zeros": (CH + 7,)}
BUFFERS = ("flat", "ema", "grad", "exp_avg")       # what the four rows of the result stand for in these checks
SCALES = (0.05, 0.04, 3e-4, 2.0)


def make_bank(layers, dev, shapes=None, seed=0):
    """A ParamBank on ``dev`` whose four buffers hold seeded normal data (one scale per buffer) in every tensor but "zeros"; padding slots are 0."""
    bank = layers.ParamBank(dict(HAND_MADE if shapes is None else shapes), dev)
    g = torch.Generator().manual_seed(1000 + seed)
    for name, scale in zip(BUFFERS, SCALES):
        host = torch.zeros(bank.numel)
        for n in bank.names:
            if n != "zeros":
                off, num = bank.offsets[n]
                host[off:off + num] = torch.randn(num, generator=g) * scale
        getattr(bank, name).copy_(host)
    return bank


def padding_mask(bank):
    m = torch.ones(bank.numel, dtype=torch.bool)
    for off, num in bank.offsets.values():
        m[off:off + num] = False
    return m


def reference(bank, buf):
    """fp64 on the host: (per-tensor norms [nseg], their mean, the global L2 norm over the tensors) of one buffer of the bank's layout."""
    x = buf.detach().cpu().double()
    per = torch.stack([torch.linalg.vector_norm(x[off:off + num]) for off, num in (bank.offsets[n] for n in bank.names)])
    return per.numpy(), float(per.mean()), float(torch.linalg.vector_norm(per))


def norms_only(ops, plan, p=None, ema=None, g=None):
    """The reduction alone through the public wrapper; returns (norms [4, nseg], summary [4, 2]) as host fp32 arrays."""
    ops.adamw_ema(p, g, None, None, ema, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 0.0, norms=plan, apply=False)
    out = plan.out.cpu().numpy().copy()
    k = 4 * plan.nseg
    return out[:k].reshape(4, plan.nseg), out[k:].reshape(4, 2)


def check_row(tag, got_norms, got_summary, ref, show=True):
    """One buffer's row against ``reference``: every figure is printed before it is asserted."""
    per, mean, l2 = ref
    rel = np.abs(got_norms.astype(np.float64) - per) / np.where(per > 0, per, 1.0)
    e_mean, e_l2 = abs(float(got_summary[0]) - mean) / mean, abs(float(got_summary[1]) - l2) / l2
    if show:
        print(f"[{tag}] per-tensor max rel err {rel.max():.3e} (bound {BOUND:.3e}); mean {e_mean:.3e} (bound {MEAN_BOUND:.3e}); l2 {e_l2:.3e} (bound {BOUND:.3e})")
    assert np.all(rel <= BOUND), (tag, rel)
    assert np.all(got_norms[per == 0] == 0), f"{tag}: an all-zero tensor has norm exactly 0"
    assert e_mean <= MEAN_BOUND and e_l2 <= BOUND, (tag, e_mean, e_l2)
    want_mean = np.float32(np.mean(got_norms.astype(np.float64)))
    assert got_summary[0] == want_mean, f"{tag}: the mean is np.mean of the returned fp32 norms in fp64, rounded once ({got_summary[0]!r} vs {want_mean!r})"
