"""Problems, references and the gate of the LoRA weight-gradient tests at ranks 17..64, generic over the 16-bit working dtype:
tests/test_lora_wgrad_rank_gpu.py uses them on the fp16 library, tests/run_bf16_wgrad_rank_checks.py on the bf16 one.

G[n, r] (+)= scale * sum_m X[m, n] T[m, r].  The reference is the fp64 product of the 16-bit operands, the gate band B1 of tests/kernel_bands.py for an
fp32 output: |err| <= 2^-24 max(|ref|, |got|) + 2 T 2^-24 S with S = scale |X|^T |T| (+ the pre-filled value) and T = M terms, + 1 where G is pre-filled.
Products of two 16-bit operands are exact in fp32, so an fp32-accumulating kernel meets the band in any summation order."""
import contextlib

import torch

import kernel_bands as KB

# (M, N, [R, N] layout) of the mixed batch: M = 26 is less than one 32-row MFMA step; 77, 333, 1000 and 4100 are no multiples of 32 (row tails of 13, 13, 8 and
# 4 rows when a problem is one split); N = 648 ends in a partial 16-column tile, 768 and 1280 span several 320-column chunks
MIXED = [(1000, 320, False), (2048, 640, True), (77, 768, False), (4100, 1280, True), (26, 320, True), (333, 648, False)]
SCALE = 0.5


def rp_of(R):
    return 8 if R <= 8 else 16 if R <= 16 else 32 if R <= 32 else 64


def rnd(*shape, dev, seed, dtype):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev).to(dtype)


class Problem:
    """X is the column slice [:, 32:32 + N] of a buffer N + ``extra`` wide; T is padded to the rank's RP columns, the pad columns hold ``pad``.
    ``ref`` / ``S`` are [N, R], computed once and never modified."""

    def __init__(self, M, N, R, trans, dev, dtype, seed, pad=0.0, extra=64):
        self.M, self.N, self.R, self.trans = M, N, R, trans
        self.X = rnd(M, N + extra, dev=dev, seed=seed, dtype=dtype)[:, 32:32 + N]
        self.T = torch.full((M, rp_of(R)), pad, dtype=dtype, device=dev)
        self.T[:, :R] = rnd(M, R, dev=dev, seed=seed + 1000, dtype=dtype)
        self.ref = SCALE * self.X.double().t() @ self.T[:, :R].double()
        self.S = SCALE * self.X.double().abs().t() @ self.T[:, :R].double().abs()

    def with_pad(self, pad):
        """The same problem (operands and reference shared) with another value in T's pad columns."""
        q = object.__new__(Problem)
        q.__dict__.update(self.__dict__)
        q.T = self.T.clone()
        q.T[:, self.R:] = pad
        return q

    def out(self, fill):
        shape = (self.R, self.N) if self.trans else (self.N, self.R)
        return torch.full(shape, fill, dtype=torch.float32, device=self.X.device)

    def strides(self):
        return (1, self.N) if self.trans else (self.R, 1)


_MIXED = {}


def mixed(dev, dtype, R):
    """The six problems of the mixed batch at rank R (built once per dtype and rank)."""
    key = (dtype, R)
    if key not in _MIXED:
        _MIXED[key] = [Problem(M, N, R, trans, dev, dtype, seed=10 * R + i) for i, (M, N, trans) in enumerate(MIXED)]
    return _MIXED[key]


def run(ops, probs, fill=1.0, batched=True):
    """Issues the problems inside one ``wgrad_batch`` (or one by one) into fresh outputs pre-filled with ``fill``; returns the outputs."""
    outs = [p.out(fill) for p in probs]
    with (ops.wgrad_batch() if batched else contextlib.nullcontext()):
        for p, G in zip(probs, outs):
            ops.lora_wgrad(p.X, p.T, G, *p.strides(), p.R, scale=SCALE)
    return outs


def band(name, p, G, fill, dtype):
    """Prints the figures of problem ``p``'s output G (pre-filled with ``fill``) under B1, then asserts."""
    ref, S = (p.ref.t(), p.S.t()) if p.trans else (p.ref, p.S)
    r = KB.gate_b(G, fill + ref, abs(fill) + S, p.M + (1 if fill else 0), dtype, rounded=False)
    print(f"[B {name} M{p.M} N{p.N} R{p.R} {'[R, N]' if p.trans else '[N, R]'}] B1 max ratio {r['b1_ratio']:.5f}, {r['b1_bad']} elements over")
    assert r["ok_b1"], f"{name} ({p.M}x{p.N}, R={p.R}): gate B1, {r['b1_bad']} elements over the band (max ratio {r['b1_ratio']:.3f})"
    return r


@contextlib.contextmanager
def counted(ops):
    """Counts the C-ABI calls made through ``ops._call`` by name."""
    calls, orig = [], ops._call

    def wrapper(name, *args):
        calls.append(name)
        return orig(name, *args)

    ops._call = wrapper
    try:
        yield calls
    finally:
        ops._call = orig
