"""Inputs, fp64 references, the error gates and the checks of ``fd_cosine_logits_fwd`` / ``fd_cosine_logits_bwd``, shared by
tests/test_kernels_cosinehead_gpu.py (fp16 library) and tests/run_bf16_cosinehead_checks.py (bf16 library, own process).  The kernels are fp32 in both
libraries, so both run the same table under the same gates.

    inv_norm[n]  = 1 / max(|e_n|, 1e-12)                    logits[n, k] = scale * inv_norm[n] * <e_n, t_hat_k>
    d_e[n]       = scale * inv_norm[n] * (sum_k dl[n, k] t_hat_k - (sum_k dl[n, k] c[n, k]) e_n inv_norm[n]),   c = logits / scale;  0 for a row at the clamp

Gates, first order in u = 2^-24 (the unit roundoff of fp32), times 1.01 for the second-order terms ((E + 8) u < 3e-4 at E = 4096).  A sum of n products
taken in ANY order, contracted to fused multiply-adds or not, is off by at most n u sum|products| (one rounding per product, n - 1 additions).  The
library is built with fast-math: sqrt, reciprocal and division are the hardware's approximations, each good to one unit in the last place = 2 u.

  inv_norm:  the sum of E squares is off by E u relative (all terms positive), the square root halves that and adds 2 u, the reciprocal 2 u more:
                 |inv_norm - ref| <= (E / 2 + 4) u ref
  logits:    the E-term dot product, the two factors (2 u on the result) and inv_norm's error (relative, so on |ref|):
                 |logits - ref| <= u (E |scale| ref_inv (|e| @ |t_hat|^T) + (E / 2 + 6) |ref|)
  d_e:       the reference is the formula in fp64 on the SAME fp32 logits and inv_norm the kernel is handed, so only the kernel's own arithmetic counts.
             s = sum_k dl c: the division is 2 u (4 u allowed: reciprocal, then product), the product u, the sum K - 1 more: (K + 4) u sum|dl c|.
             a = sum_k dl t_hat: K u sum|dl||t_hat|.  e^ = e inv: u; s e^: u more.  The difference: u; the two outer factors: 2 u.
                 |d_e - ref| <= u (|scale| inv (K (|dl| @ |t_hat|) + ((K + 4) sum|dl c| + 2 |s|) |e^|) + 3 |ref|)

An all-zero row makes every term of its gates 0: its logits and its gradient must be exactly 0.

Layout: every tensor -- e, t_hat, logits, inv_norm, d_logits, d_e -- is a view at an ODD element offset of one flat buffer (nothing but 4-byte alignment
holds), with ``GUARD`` sentinel elements around each; e also with row stride E + 3, the gaps holding sentinels too."""
import itertools

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = 12345.0
GUARD = 3
CLAMP = float(np.float32(1e-12))
NS, ES, KS, PADS = (1, 3, 8), (48, 100, 1024), (1, 2, 12, 16), (0, 3)      # E: below one wave; no multiple of 4 or 64; 16 elements per lane
CASES = list(itertools.product(NS, ES, KS, PADS))                         # (N, E, K, lde - E)
SCALES = (100.0, 14.285714, -3.0)


class OddBuffer:
    """Named fp32 tensors as views of one flat device buffer, each at an odd element offset with ``GUARD`` sentinels on both sides.  A shape given as
    (rows, cols, ld) is a strided 2-D view with row stride ld >= cols; the elements between its rows are not its own."""

    def __init__(self, shapes, dev):
        self.views, own, off = {}, [], 1
        for name, shp in shapes.items():
            off += GUARD
            off += 1 - off % 2
            if len(shp) == 3:
                r, c, ld = shp
                span = (r - 1) * ld + c
                self.views[name] = (off, (r, c), (ld, 1))
                own += [(off + i * ld, c) for i in range(r)]
            else:
                span = int(np.prod(shp))
                self.views[name] = (off, tuple(shp), None)
                own.append((off, span))
            assert off % 2 == 1
            off += span
        self.numel = off + GUARD
        self.flat = torch.full((self.numel,), SENTINEL, dtype=torch.float32, device=dev)
        self.mask = np.ones(self.numel, dtype=bool)
        for o, n in own:
            self.mask[o:o + n] = False

    def view(self, name):
        off, shp, stride = self.views[name]
        if stride is None:
            return self.flat[off:off + int(np.prod(shp))].view(shp)
        return torch.as_strided(self.flat, shp, stride, off)

    def guards_intact(self):
        return bool(np.all(self.flat.cpu().numpy()[self.mask] == SENTINEL))


def inputs(case, seed):
    """Host fp32 arrays (e [N, E], t_hat [K, E] unit rows, d_logits [N, K]).  The last row of e is all zero when N > 1 (the clamp), row 0 equals class
    direction K - 1 times 3.5 (cos = 1)."""
    N, E, K, _ = case
    g = np.random.default_rng(9100 + seed)
    t = g.standard_normal((K, E))
    t = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
    e = (g.standard_normal((N, E)) * g.uniform(0.2, 3.0, (N, 1))).astype(np.float32)
    e[0] = 3.5 * t[K - 1]
    if N > 1:
        e[N - 1] = 0.0
    return e, t, g.standard_normal((N, K)).astype(np.float32)


def reference_fwd(e, t, scale):
    """(logits, inv_norm, logits gate, inv_norm gate) in fp64."""
    e64, t64 = e.astype(np.float64), t.astype(np.float64)
    E = e.shape[1]
    inv = 1.0 / np.maximum(np.linalg.norm(e64, axis=1), CLAMP)
    ref = scale * inv[:, None] * (e64 @ t64.T)
    gate = 1.01 * U * (E * abs(scale) * inv[:, None] * (np.abs(e64) @ np.abs(t64).T) + (E / 2 + 6) * np.abs(ref))
    return ref, inv, gate, 1.01 * U * (E / 2 + 4) * inv


def reference_bwd(e, t, logits, inv_norm, dl, scale):
    """(d_e, gate) in fp64 from the fp32 arrays the kernel is handed; a row at the clamp (inv_norm >= 5e11) has gradient 0."""
    e64, t64, lg, inv, d = (a.astype(np.float64) for a in (e, t, logits, inv_norm, dl))
    K = t.shape[0]
    c = lg / scale
    s = (d * c).sum(axis=1, keepdims=True)
    eh = e64 * inv[:, None]
    live = (inv < 5e11)[:, None]
    ref = np.where(live, scale * inv[:, None] * (d @ t64 - s * eh), 0.0)
    mag = abs(scale) * inv[:, None] * (K * (np.abs(d) @ np.abs(t64)) + ((K + 4) * np.abs(d * c).sum(axis=1, keepdims=True) + 2 * np.abs(s)) * np.abs(eh))
    return ref, np.where(live, 1.01 * U * (mag + 3 * np.abs(ref)), 0.0)


class Problem:
    """One case laid out in an ``OddBuffer`` on ``dev``; ``fwd`` / ``bwd`` run the wrappers into its output views and return host arrays."""

    def __init__(self, dev, case, seed=0):
        N, E, K, pad = case
        self.case, self.host = case, inputs(case, seed)
        self.buf = OddBuffer(dict(e=(N, E, E + pad), t_hat=(K, E), logits=(N, K), inv_norm=(N,), d_logits=(N, K), d_e=(N, E), lg_in=(N, K), inv_in=(N,)), dev)
        for name, a in zip(("e", "t_hat", "d_logits"), self.host):
            self.buf.view(name).copy_(torch.from_numpy(a))

    def fwd(self, ops, scale):
        lg, inv = ops.cosine_logits(self.buf.view("e"), self.buf.view("t_hat"), scale, out=(self.buf.view("logits"), self.buf.view("inv_norm")))
        torch.cuda.synchronize()
        return lg.cpu().numpy().copy(), inv.cpu().numpy().copy()

    def bwd(self, ops, scale, logits, inv_norm):
        """``logits`` / ``inv_norm``: the host fp32 arrays the backward is handed (copied into views of their own)."""
        self.buf.view("lg_in").copy_(torch.from_numpy(logits))
        self.buf.view("inv_in").copy_(torch.from_numpy(inv_norm))
        de = ops.cosine_logits_bwd(self.buf.view("e"), self.buf.view("t_hat"), self.buf.view("lg_in"), self.buf.view("inv_in"), self.buf.view("d_logits"), scale,
                                   out=self.buf.view("d_e"))
        torch.cuda.synchronize()
        return de.cpu().numpy().copy()


def check_case(ops, dev, case, seed, scale, tag, show=True):
    """Forward and backward of one case against fp64; every worst error / gate ratio is printed before it is asserted.  Returns the three ratios."""
    N, E, K, pad = case
    p = Problem(dev, case, seed)
    e, t, dl = p.host
    lg, inv = p.fwd(ops, scale)
    ref, inv_ref, gate, inv_gate = reference_fwd(e, t, scale)
    err, ierr = np.abs(lg - ref), np.abs(inv - inv_ref)
    # the backward is handed fp32 roundings of the REFERENCE forward, so that it is judged on its own
    lg32, inv32 = ref.astype(np.float32), inv_ref.astype(np.float32)
    de = p.bwd(ops, scale, lg32, inv32)
    dref, dgate = reference_bwd(e, t, lg32, inv32, dl, scale)
    derr = np.abs(de - dref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratios = [float(np.nanmax(np.where(g > 0, x / g, np.where(x == 0, 0.0, np.inf)))) for x, g in ((err, gate), (ierr, inv_gate), (derr, dgate))]
    if show:
        print(f"[{tag}] N={N} E={E} K={K} lde={E + pad} scale={scale}: logits max|err| {err.max():.3e} (err/gate {ratios[0]:.3f}), inv_norm err/gate {ratios[1]:.3f}, "
              f"d_e max|err| {derr.max():.3e} (err/gate {ratios[2]:.3f})")
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(inv)) and np.all(np.isfinite(de)), tag
    assert np.all(err <= gate) and np.all(ierr <= inv_gate) and np.all(derr <= dgate), (tag, case, ratios)
    cos = lg[0, K - 1] / scale                       # row 0 is a multiple of class direction K - 1
    assert abs(cos - 1.0) <= gate[0, K - 1] / abs(scale), (tag, cos)
    if N > 1:                                       # the all-zero row: exactly 0, through the clamp
        assert np.all(lg[N - 1] == 0) and np.all(de[N - 1] == 0) and inv[N - 1] >= 5e11, (tag, lg[N - 1], inv[N - 1])
    assert p.buf.guards_intact(), f"{tag} {case}: a guard element (or a gap between the rows of e) was overwritten"
    return ratios


def run_table(ops, dev, tag, show=True):
    """Every case of ``CASES``, the scales in rotation.  What both libraries run."""
    worst = [0.0, 0.0, 0.0]
    for i, case in enumerate(CASES):
        r = check_case(ops, dev, case, i, SCALES[i % len(SCALES)], tag, show)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"[{tag}] {len(CASES)} cases, worst err / gate: logits {worst[0]:.3f}, inv_norm {worst[1]:.3f}, d_e {worst[2]:.3f}")
    return worst


def repeat_bits(ops, dev, case=(8, 1024, 12, 3), scale=100.0):
    """Two calls, and a call on a side stream, give equal bits (forward and backward)."""
    p = Problem(dev, case, seed=77)
    lg1, inv1 = p.fwd(ops, scale)
    de1 = p.bwd(ops, scale, lg1, inv1)
    lg2, inv2 = p.fwd(ops, scale)
    de2 = p.bwd(ops, scale, lg1, inv1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lg3, inv3 = p.fwd(ops, scale)
        de3 = p.bwd(ops, scale, lg1, inv1)
    torch.cuda.current_stream().wait_stream(side)
    for a, b in ((lg1, lg2), (lg1, lg3), (inv1, inv2), (inv1, inv3), (de1, de2), (de1, de3)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two calls differ"
    assert p.buf.guards_intact()
