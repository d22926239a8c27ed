"""Inputs, fp64 references, the error gate and the checks of ``fd_lora_merge_multi``, shared by tests/test_kernels_loramerge_gpu.py (fp16 library) and
tests/run_bf16_loramerge_checks.py (bf16 library, own process).

    out[n, k] = base[n, k] + scale * sum_{j < r} up[n, j] * down[j, k]          ref = base + scale * (up @ down) in fp64

Gate per element, u = 2^-24 the unit roundoff of fp32:

    |out - ref| <= 1.01 * u * ((2 r + 2) * |scale| * (|up| @ |down|) + |ref|)

the first-order bound for r products and r additions in any order, contracted to fused multiply-adds or not ((2 r) u on the sum of absolute products),
plus the scale-and-add (2 u more on the scaled sum, u on the result, which |ref| carries); 1.01 covers the second-order terms ((2 r + 2) u < 1e-5).

``OddBank`` stands for the flat parameter bank: every tensor -- down, up, and here base and out too -- is a view at an ODD element offset of one flat
buffer, so nothing but 4-byte alignment holds, with ``GUARD`` sentinel elements on both sides of each."""
import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = 12345.0
GUARD = 3
# (r, N, K, scale): one element rows; sizes that are no multiple of the 32 x 64 tile; the reference's rank 50; the largest rank with whole tiles
SMALL = [(1, 3, 5, 1.0), (4, 40, 77, 1.0), (50, 33, 77, 0.37), (64, 64, 96, -2.5)]
REAL = (50, 3072, 768, 1.0)            # text-encoder mlp.fc1 at the reference's rank
CASES = SMALL + [REAL]
MIXED_17 = [SMALL[i % 4] for i in range(17)]      # one call, two launches of at most 16 pairs


class OddBank:
    """The part of ``layers.ParamBank`` that ``layers.LoRAPair`` and ``refresh_pairs`` read (``flat``, ``ema``, ``shape``, ``view``), with every tensor
    at an odd element offset and ``GUARD`` sentinels around it."""

    def __init__(self, shapes, dev):
        self._shape, self.offsets = dict(shapes), {}
        off = 1
        for n, s in shapes.items():
            num = int(np.prod(s))
            off += GUARD
            off += 1 - off % 2                           # odd
            self.offsets[n] = (off, num)
            off += num
        self.numel = off + GUARD
        self.names = list(shapes)
        self.flat = torch.full((self.numel,), SENTINEL, dtype=torch.float32, device=dev)
        self.ema = torch.full((self.numel,), SENTINEL, dtype=torch.float32, device=dev)

    def shape(self, n):
        return self._shape[n]

    def view(self, n, buf=None):
        off, num = self.offsets[n]
        return (self.flat if buf is None else buf)[off:off + num].view(self._shape[n])

    def outside(self, buf=None):
        """The elements no tensor owns (the guards), as one host array."""
        m = np.ones(self.numel, dtype=bool)
        for off, num in self.offsets.values():
            m[off:off + num] = False
        return (self.flat if buf is None else buf).cpu().numpy()[m]


def inputs(case, seed):
    """Host fp32 arrays (down [r, K], up [N, r], base [N, K]) of one case."""
    r, N, K, _ = case
    g = np.random.default_rng(7000 + seed)
    return (g.standard_normal((r, K)).astype(np.float32), (0.05 * g.standard_normal((N, r))).astype(np.float32),
            (0.02 * g.standard_normal((N, K))).astype(np.float32))


def reference(down, up, base, scale):
    """(ref, gate) in fp64."""
    d, u, b = down.astype(np.float64), up.astype(np.float64), base.astype(np.float64)
    ref = b + scale * (u @ d)
    gate = 1.01 * U * ((2 * down.shape[0] + 2) * abs(scale) * (np.abs(u) @ np.abs(d)) + np.abs(ref))
    return ref, gate


class Problem:
    """``cases`` laid out in one ``OddBank`` on ``dev`` (pair i: d{i}, u{i}, base{i}, out{i}), its ``LoRAPair`` objects and the host inputs."""

    def __init__(self, layers, dev, cases, seed=0):
        self.cases = list(cases)
        shapes = {}
        for i, (r, N, K, _) in enumerate(self.cases):
            shapes.update({f"d{i}": (r, K), f"u{i}": (N, r), f"base{i}": (N, K), f"out{i}": (N, K)})
        self.bank = OddBank(shapes, dev)
        self.host = [inputs(c, seed + i) for i, c in enumerate(self.cases)]
        for i, (d, u, b) in enumerate(self.host):
            for name, a in ((f"d{i}", d), (f"u{i}", u), (f"base{i}", b)):
                self.bank.view(name).copy_(torch.from_numpy(a))
        self.pairs = [layers.LoRAPair(self.bank, f"d{i}", f"u{i}") for i in range(len(self.cases))]
        for off, _ in self.bank.offsets.values():
            assert off % 2 == 1

    def base(self, i):
        return self.bank.view(f"base{i}")

    def out(self, i):
        return self.bank.view(f"out{i}")

    def run(self, layers, in_place, scale=None, ema=False):
        """One ``refresh_pairs(..., merge=...)`` call over all pairs (they share ``scale``: the wrapper's keyword); -> host results per pair."""
        n = len(self.cases)
        merge = [(self.base(i), self.base(i) if in_place else self.out(i)) for i in range(n)]
        layers.refresh_pairs(self.pairs, self.cases[0][3] if scale is None else scale, ema=ema, merge=merge)
        torch.cuda.synchronize()
        return [m[1].cpu().numpy().copy() for m in merge]


def check(tag, got, down, up, base, scale, show=True):
    """One pair against fp64: the worst ratio error / gate is printed before it is asserted."""
    ref, gate = reference(down, up, base, scale)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / gate).max())
    if show:
        print(f"[{tag}] r={down.shape[0]} N={up.shape[0]} K={down.shape[1]} scale={scale}: max |err| {err.max():.3e}, worst err / gate {worst:.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= gate), (tag, worst)


def run_table(layers, dev, tag, show=True):
    """Every case of ``CASES`` out of place and in place (one pair per call, its own scale), then the 17 mixed pairs in one call: each against fp64,
    ``base`` bit-unchanged when ``out`` is another tensor, the guards intact.  What both libraries run."""
    for ci, case in enumerate(CASES):
        for in_place in (False, True):
            p = Problem(layers, dev, [case], seed=ci)
            d, u, b = p.host[0]
            got = p.run(layers, in_place)[0]
            check(f"{tag} {'in place' if in_place else 'out != base'}", got, d, u, b, case[3], show)
            if not in_place:
                assert np.array_equal(p.base(0).cpu().numpy().view(np.uint32), b.view(np.uint32)), "base changed although out is another tensor"
            else:
                assert np.all(p.out(0).cpu().numpy() == SENTINEL), "the unused out tensor was written"
            assert np.all(p.bank.outside() == SENTINEL), "a guard element was overwritten"
    p = Problem(layers, dev, MIXED_17, seed=100)
    got = p.run(layers, in_place=False, scale=0.37)
    for i, (d, u, b) in enumerate(p.host):
        check(f"{tag} 17 pairs, pair {i}", got[i], d, u, b, 0.37, show and i in (0, 15, 16))
        assert np.array_equal(p.base(i).cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert np.all(p.bank.outside() == SENTINEL), "a guard element was overwritten"
